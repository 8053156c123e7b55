// stereofilter.hip — speckle filter of a disparity image and the collision-depth plane of vido_mask_propagate, on gfx950 (no reference counterpart: the reference takes its
// disparity from outside).  Rule (include/vido_c.h; the numpy statement is tests/refimpl/stereo_filter_np.py): a pixel is valid iff status == 0 and
// 1 <= q4 <= 65535; two valid 4-neighbours with |q4a - q4b| <= max_diff_q4 share an edge; a region is a connected component under these edges; a valid pixel of a region
// below min_region pixels becomes status 4.  The edge relation is NOT transitive (a ramp is one region whose ends differ arbitrarily), so nothing here reasons from "a ~ b
// and b ~ c": every horizontal and every vertical edge is united, in the tile or on the seam.  The one shortcut kept is a chain, not an implication: the pixels of a row
// between two missing horizontal edges are joined edge by edge, so they start under the first of them.
// Four launches on one stream (one with min_region = 1), union-find rooted at the smallest raster index (ccunion.hpp):
//   k_sf_local    a workgroup labels a 32 x 32 tile in LDS and writes global parent indices (-1: not valid) and area 0 — every pixel of both planes; it zeroes the counters;
//   k_sf_seam     the pixels of a tile's top row / left column unite with their upper / left neighbour in the next tile, each pair tested on its own.  EVERY access to the
//                 parent plane in this launch is an agent-scope atomic (another workgroup, maybe on another XCD, updates the same words);
//   k_sf_flatten  parent = root for every pixel, and the areas added at the root: equal roots of a wave are folded by ballot into one atomic (k_cc_flatten's loop);
//   k_sf_write    status_out, disp_out, depth_out and the four counters.  It reads status[i] before it writes status_out[i], in one thread: status_out may be status.
// Integer minima and sums only: no execution order matters.
#include "common.hpp"
#include "ccunion.hpp"
#include <cfloat>
#include <cmath>

struct StereoFilterState {
    int32_t* d_planes = nullptr;                                  // [2][px]: parent index per pixel (-1 = not valid), area at a root
    size_t cap_bytes = 0;
    int32_t* d_stats = nullptr;                                   // the counters when the caller asks for none
};

#define SF_T 32                                                   // tile edge
#define SF_PX (SF_T * SF_T)

__device__ __forceinline__ bool sf_valid(int st, int q) { return st == 0 && q >= 1 && q <= 65535; }

// One workgroup per tile, four pixels per thread (rows ry0, ry0 + 8, ...); half a wave holds a tile row.  val = q4 of a valid pixel, 0 elsewhere (0 is no valid q4).
__global__ __launch_bounds__(256) void k_sf_local(const int32_t* __restrict__ q4, const uint8_t* __restrict__ status, int H, int W, int max_diff, int32_t* __restrict__ parent,
                                                  int32_t* __restrict__ area, int32_t* __restrict__ stats)
{
    __shared__ int val[SF_PX], par[SF_PX];
    const int x0 = blockIdx.x * SF_T, y0 = blockIdx.y * SF_T;
    const int rx = threadIdx.x & (SF_T - 1), ry0 = threadIdx.x / SF_T;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 4) stats[threadIdx.x] = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int ry = ry0 + 8 * k, l = ry * SF_T + rx, x = x0 + rx, y = y0 + ry;
        int v = 0;
        if (x < W && y < H) { const size_t i = (size_t)y * W + x; const int q = q4[i]; if (sf_valid(status[i], q)) v = q; }
        val[l] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {                                   // a pixel starts under the first pixel of its chain of horizontal edges
        const int ry = ry0 + 8 * k, l = ry * SF_T + rx;
        const int v = val[l];
        const bool starts = rx == 0 || v == 0 || val[l - 1] == 0 || abs(v - val[l - 1]) > max_diff;
        const unsigned long long b = __ballot(starts);
        const unsigned row = (unsigned)(b >> (threadIdx.x & 32));   // the tile row of this half of the wave; bit 0 is set
        par[l] = ry * SF_T + (31 - __clz(row & (0xffffffffu >> (31 - rx))));
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {                                   // every vertical edge, one by one
        const int ry = ry0 + 8 * k, l = ry * SF_T + rx;
        const int v = val[l];
        if (v == 0 || ry == 0) continue;
        const int u = val[l - SF_T];
        if (u != 0 && abs(v - u) <= max_diff) cc_lunion(par, l, l - SF_T);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int ry = ry0 + 8 * k, l = ry * SF_T + rx, x = x0 + rx, y = y0 + ry;
        if (x >= W || y >= H) continue;
        int g = -1;
        if (val[l] != 0) { const int r = cc_lfind(par, l); g = (y0 + r / SF_T) * W + x0 + (r & (SF_T - 1)); }
        const size_t i = (size_t)y * W + x;
        parent[i] = g; area[i] = 0;
    }
}

// One wave per tile; thread j < 63 owns one border pixel: the top row (32), the left column below it (31).  Every pair of 4-neighbours in two tiles has exactly one member
// on its tile's top row (the pair is vertical) or left column (horizontal); that member tests the pair's own edge and unites.  Nothing is left out as implied.
__global__ __launch_bounds__(64) void k_sf_seam(const int32_t* __restrict__ q4, const uint8_t* __restrict__ status, int H, int W, int max_diff, int32_t* parent)
{
    const int j = threadIdx.x;
    int rx, ry;
    if (j < SF_T) { rx = j; ry = 0; }
    else if (j < 2 * SF_T - 1) { rx = 0; ry = j - SF_T + 1; }
    else return;
    const int x = blockIdx.x * SF_T + rx, y = blockIdx.y * SF_T + ry;
    if (x >= W || y >= H) return;
    const int i = y * W + x;
    const int v = q4[i];
    if (!sf_valid(status[i], v)) return;
    if (rx == 0 && x > 0) { const int u = q4[i - 1]; if (sf_valid(status[i - 1], u) && abs(v - u) <= max_diff) cc_gunion(parent, i, i - 1); }
    if (ry == 0 && y > 0) { const int u = q4[i - W]; if (sf_valid(status[i - W], u) && abs(v - u) <= max_diff) cc_gunion(parent, i, i - W); }
}

// parent[i] = root(i) and area[root] += 1.  The walk reads words that other threads of this launch overwrite with their roots (an ancestor replaces an ancestor: the walk
// still ends at the root); those accesses are agent-scope atomics as in k_sf_seam.
__global__ __launch_bounds__(256) void k_sf_flatten(int32_t* parent, unsigned npx, int32_t* __restrict__ area)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    int r = -1;
    if (i < npx) {
        const int p = __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p >= 0) {
            r = cc_gfind(parent, p);
            if (r != p) __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    bool todo = r >= 0;
    unsigned long long m = __ballot(todo);
    const int lane = threadIdx.x & 63;
    while (m) {                                                     // (m is wave-uniform)
        const int leader = __ffsll((long long)m) - 1;
        const int lr = __shfl(r, leader);
        const bool same = todo && r == lr;
        const unsigned long long b = __ballot(same);
        if (lane == leader) atomicAdd(area + lr, __popcll(b));
        todo = todo && !same;
        m &= ~b;
    }
}

// The counters alone, for the call that launches no labelling.
__global__ void k_sf_zero(int32_t* __restrict__ stats) { if (threadIdx.x < 4) stats[threadIdx.x] = 0; }

// One pixel per thread.  parent / area: null when min_region = 1 (nothing is removed).  status is read before status_out is written, by the same thread: they may be one.
__global__ __launch_bounds__(256) void k_sf_write(const int32_t* __restrict__ q4, const uint8_t* status, unsigned npx, const int32_t* __restrict__ parent,
                                                  const int32_t* __restrict__ area, int min_region, float bf, float* __restrict__ disp, uint8_t* status_out,
                                                  float* __restrict__ depth, int32_t* __restrict__ stats)
{
    __shared__ int s_cnt[4][4];
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int c_in = 0, c_reg = 0, c_px = 0, c_out = 0;
    if (i < npx) {
        const int q = q4[i]; int st = status[i];
        if (st == 0 && !sf_valid(0, q)) st = 3;
        else if (st == 0) {
            c_in = 1;
            if (parent) {
                const int r = parent[i];                            // (flattened: the root)
                if (area[r] < min_region) { st = 4; c_px = 1; c_reg = r == (int)i; }
            }
            c_out = st == 0;
        }
        const float d = st == 0 ? (float)q * (1.0f / 16.0f) : -1.0f;
        if (status_out) status_out[i] = (uint8_t)st;
        if (disp) disp[i] = d;
        if (depth) depth[i] = st == 0 ? __fdiv_rn(bf, d) : FLT_MAX;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { c_in += __shfl_xor(c_in, o, 64); c_reg += __shfl_xor(c_reg, o, 64); c_px += __shfl_xor(c_px, o, 64); c_out += __shfl_xor(c_out, o, 64); }
    if (lane == 0) { s_cnt[wv][0] = c_in; s_cnt[wv][1] = c_reg; s_cnt[wv][2] = c_px; s_cnt[wv][3] = c_out; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int cnt = s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
        if (cnt) atomicAdd(&stats[threadIdx.x], cnt);
    }
}

// ---- host ------------------------------------------------------------------------------------------
void stereofilter_state_destroy(vido_ctx* ctx)
{
    StereoFilterState* S = ctx->sfilter;
    if (!S) return;
    if (S->d_planes) (void)hipFree(S->d_planes);
    if (S->d_stats) (void)hipFree(S->d_stats);
    delete S; ctx->sfilter = nullptr;
}

// the state, the counters and two planes of px words; the first call of a size waits for earlier calls, which may still use the old planes
static int sf_prepare(vido_ctx* ctx, hipStream_t st, size_t px)
{
    if (!ctx->sfilter) ctx->sfilter = new StereoFilterState();
    StereoFilterState* S = ctx->sfilter;
    if (!S->d_stats) HIP_TRY(ctx, hipMalloc((void**)&S->d_stats, 16));
    return vido_grow_device(ctx, st, (void**)&S->d_planes, &S->cap_bytes, 2 * px * 4, GROW_EXACT);
}

// the launches of one call on device pointers
static void sf_enqueue(StereoFilterState* S, hipStream_t st, const int32_t* q4, const uint8_t* status, int w, int h, int max_diff, int min_region, float bf, float* disp,
                       uint8_t* status_out, float* depth, int32_t* stats)
{
    const size_t px = (size_t)w * h;
    const int32_t *P = nullptr, *A = nullptr;
    if (min_region > 1) {
        int32_t *par = S->d_planes, *area = S->d_planes + px;
        const dim3 tiles((w + SF_T - 1) / SF_T, (h + SF_T - 1) / SF_T);
        hipLaunchKernelGGL(k_sf_local, tiles, dim3(256), 0, st, q4, status, h, w, max_diff, par, area, stats);
        hipLaunchKernelGGL(k_sf_seam, tiles, dim3(64), 0, st, q4, status, h, w, max_diff, par);
        hipLaunchKernelGGL(k_sf_flatten, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, st, par, (unsigned)px, area);
        P = par; A = area;
    } else {
        hipLaunchKernelGGL(k_sf_zero, dim3(1), dim3(64), 0, st, stats);
    }
    hipLaunchKernelGGL(k_sf_write, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, st, q4, status, (unsigned)px, P, A, min_region, bf, disp, status_out, depth, stats);
}

extern "C" int vido_stereo_filter(vido_ctx* ctx, const int32_t* q4, const uint8_t* status, int width, int height, int max_diff_q4, int min_region, float bf, float* disp_out,
                                  uint8_t* status_out, float* depth_out, int32_t* stats_out, int on_device)
{
    if (!ctx) return VIDO_E_INVALID;
    if (!q4 || !status) return vido_set_error(ctx, VIDO_E_INVALID, "stereo_filter: null image");
    if (width < 1 || height < 1 || width > 4095 || height > 4095) return vido_set_error(ctx, VIDO_E_INVALID, "stereo_filter: size %d x %d outside 1 .. 4095", width, height);
    if (max_diff_q4 < 0 || max_diff_q4 > 65535) return vido_set_error(ctx, VIDO_E_INVALID, "stereo_filter: max_diff_q4 %d outside 0 .. 65535", max_diff_q4);
    if (min_region < 1 || min_region > (1 << 24)) return vido_set_error(ctx, VIDO_E_INVALID, "stereo_filter: min_region %d outside 1 .. 2^24", min_region);
    if (!disp_out && !status_out && !depth_out && !stats_out) return vido_set_error(ctx, VIDO_E_INVALID, "stereo_filter: no output asked for");
    if (depth_out && !(std::isfinite(bf) && bf > 0.0f)) return vido_set_error(ctx, VIDO_E_INVALID, "stereo_filter: bf = %g, a finite value > 0 expected with depth_out", (double)bf);
    const size_t px = (size_t)width * height;
    if (status_out && status_out != status && (uintptr_t)status_out < (uintptr_t)status + px && (uintptr_t)status < (uintptr_t)status_out + px)
        return vido_set_error(ctx, VIDO_E_INVALID, "stereo_filter: status_out overlaps status without being status");
    if (on_device && ((uintptr_t)q4 & 3) != 0) return vido_set_error(ctx, VIDO_E_INVALID, "stereo_filter: the device q4 image must be 4-byte aligned");
    if (on_device && ((((uintptr_t)disp_out | (uintptr_t)depth_out | (uintptr_t)stats_out) & 3) != 0))
        return vido_set_error(ctx, VIDO_E_INVALID, "stereo_filter: device outputs must be 4-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = on_device && ctx->has_ext_stream ? ctx->ext_stream : ctx->stream;
    if (int rc = sf_prepare(ctx, st, px)) return rc;
    StereoFilterState* S = ctx->sfilter;
    if (!on_device) {                                                      // the host form: from here on the pointers are their slots of the staging buffer
        HostStaging& T = ctx->staging;                                     // (the status image is read and written in one slot)
        T.begin(); T.in(&q4, px * 4); T.out(&disp_out, px * 4); T.out(&depth_out, px * 4); T.keep(&stats_out, 16); T.inout(&status, &status_out, px);
        if (int rc = staging_upload(ctx, st)) return rc;
    }
    sf_enqueue(S, st, q4, status, width, height, max_diff_q4, min_region, bf, disp_out, status_out, depth_out, stats_out ? stats_out : S->d_stats);
    HIP_TRY(ctx, hipGetLastError());
    if (!on_device) return staging_download(ctx, st);
    return VIDO_OK;
}
