// maskprop.hip — forward warp of a whole label image through dense flow on gfx950 (no reference counterpart: the reference's Tracking::UpdateMask, Tracking.cc:3291-3357,
// scatters ONE lost label; track.hip::k_mask_scatter restates that with its truncation and border quirks and is untouched).
// Rule (include/vido_c.h): every pixel with a label > 0, a usable flow vector and (when a depth map is given) a usable depth is a source; its target is
// (x + rint(dx), y + rint(dy)), ties to even; a target hit by several sources takes the minimum of (depth bits << 32 | label) — the nearer source, on equal depth the
// smaller label; an unhit target takes label L when at least 5 of its 8 neighbours were hit and resolved to L (one pass over the resolved image, no cascade).
// Two launches: k_maskprop_scatter (one 64-bit atomic minimum per source into the context's key plane) and k_maskprop_resolve (decodes a 32 x 8 tile + halo of the plane
// into LDS, fills holes, writes EVERY pixel of the output).  The key plane and the three counters are re-initialised by two memsets in FRONT of the scatter, on the same
// stream: the resolve kernel cannot restore the plane itself (its halo reads of a neighbouring tile would race with that tile's workgroup restoring it), and a call that
// starts from its own memset does not depend on how the previous one ended.  Results depend on no execution order: integer minima and integer sums only.
#include "common.hpp"

struct MaskPropState {
    unsigned long long* d_keys = nullptr; size_t cap_px = 0;      // [cap_px] keys, all ones = not hit
    int32_t* d_stats = nullptr;                                   // 4 words: the counters of a call without a caller's stats buffer, and of the slot call
    int32_t* h_stats = nullptr;                                   // pinned mirror (vido_frame_propagate_mask's host result)
};

#define MP_TW 32
#define MP_TH 8

// stats[0] += sources kept.  flow is read as two scalars: a caller's map need not be 8-byte aligned.
__global__ __launch_bounds__(256) void k_maskprop_scatter(const int32_t* __restrict__ mask, const float* __restrict__ flow, const float* __restrict__ depth /* may be null */,
                                                          int H, int W, unsigned long long* __restrict__ keys, int32_t* __restrict__ stats)
{
    const unsigned n = (unsigned)H * (unsigned)W;                 // H, W <= 4095
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    bool kept = false;
    if (p < n) {
        const int L = mask[p];
        if (L > 0) {
            const float fx = flow[2 * (size_t)p], fy = flow[2 * (size_t)p + 1];
            bool ok = fabsf(fx) < 32768.f && fabsf(fy) < 32768.f;                     // false for NaN and inf
            unsigned db = 0;
            if (depth) { const float d = depth[p]; ok = ok && d > 0.f && d < __builtin_inff(); db = __float_as_uint(d); }      // positive finite floats order like their bits
            if (ok) {
                const int x = (int)(p % (unsigned)W), y = (int)(p / (unsigned)W);
                const int tx = x + (int)rintf(fx), ty = y + (int)rintf(fy);           // round to nearest, ties to even
                if (tx >= 0 && tx < W && ty >= 0 && ty < H) {
                    kept = true;
                    atomicMin(keys + ((size_t)ty * W + tx), ((unsigned long long)db << 32) | (unsigned)L);
                }
            }
        }
    }
    const unsigned long long b = __ballot(kept);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(stats, __popcll(b));
}

// stats[1] += pixels hit, stats[2] += pixels filled.  A hit pixel's label is > 0, so 0 in the tile means "not hit" (also outside the image).
__global__ __launch_bounds__(256) void k_maskprop_resolve(const unsigned long long* __restrict__ keys, int H, int W, int32_t* __restrict__ out, int32_t* __restrict__ stats)
{
    __shared__ int32_t tile[MP_TH + 2][MP_TW + 4];               // 34 columns used
    const int x0 = blockIdx.x * MP_TW, y0 = blockIdx.y * MP_TH;
    for (int i = threadIdx.x; i < (MP_TH + 2) * (MP_TW + 2); i += 256) {
        const int r = i / (MP_TW + 2), c = i - r * (MP_TW + 2);
        const int gx = x0 + c - 1, gy = y0 + r - 1;
        int32_t v = 0;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) { const unsigned long long k = keys[(size_t)gy * W + gx]; v = (k == ~0ull) ? 0 : (int32_t)(unsigned)k; }
        tile[r][c] = v;
    }
    __syncthreads();
    const int lx = threadIdx.x & (MP_TW - 1), ly = threadIdx.x / MP_TW;
    const int x = x0 + lx, y = y0 + ly;
    const bool inside = x < W && y < H;
    int32_t v = tile[ly + 1][lx + 1];
    const bool hit = inside && v != 0;
    bool filled = false;
    if (inside && v == 0) {
        int32_t nb[8];
        nb[0] = tile[ly][lx]; nb[1] = tile[ly][lx + 1]; nb[2] = tile[ly][lx + 2]; nb[3] = tile[ly + 1][lx];
        nb[4] = tile[ly + 1][lx + 2]; nb[5] = tile[ly + 2][lx]; nb[6] = tile[ly + 2][lx + 1]; nb[7] = tile[ly + 2][lx + 2];
        int32_t cand = 0; int votes = 0;                          // majority vote: a value held by 5 of 8 survives it; then it is counted
#pragma unroll
        for (int k = 0; k < 8; k++) { if (votes == 0) { cand = nb[k]; votes = 1; } else votes += (nb[k] == cand) ? 1 : -1; }
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) cnt += nb[k] == cand;
        if (cand != 0 && cnt >= 5) { v = cand; filled = true; }
    }
    if (inside) out[(size_t)y * W + x] = v;
    const unsigned long long bh = __ballot(hit), bf = __ballot(filled);
    if ((threadIdx.x & 63) == 0) { if (bh) atomicAdd(stats + 1, __popcll(bh)); if (bf) atomicAdd(stats + 2, __popcll(bf)); }
}

// ---- host ------------------------------------------------------------------------------------------
static int maskprop_state(vido_ctx* ctx, MaskPropState** out)
{
    if (ctx->mprop) { *out = ctx->mprop; return VIDO_OK; }
    MaskPropState* S = new MaskPropState();
    ctx->mprop = S;                                               // (a failed allocation below leaves a partial state: vido_destroy frees what exists)
    S->cap_px = (size_t)ctx->cfg.width * ctx->cfg.height;
    HIP_TRY(ctx, hipMalloc((void**)&S->d_keys, S->cap_px * 8));
    HIP_TRY(ctx, hipMalloc((void**)&S->d_stats, 16));
    HIP_TRY(ctx, hipHostMalloc((void**)&S->h_stats, 16));
    *out = S;
    return VIDO_OK;
}

void maskprop_state_destroy(vido_ctx* ctx)
{
    MaskPropState* S = ctx->mprop;
    if (!S) return;
    if (S->d_keys) hipFree(S->d_keys);
    if (S->d_stats) hipFree(S->d_stats);
    if (S->h_stats) hipHostFree(S->h_stats);
    delete S; ctx->mprop = nullptr;
}

// memsets + the two launches on `st`; stats: DEVICE, three words (never null here)
static int maskprop_enqueue(vido_ctx* ctx, MaskPropState* S, hipStream_t st, const int32_t* mask_prev, const float* flow, const float* depth_prev, int H, int W,
                            int32_t* out, int32_t* stats)
{
    const size_t px = (size_t)H * W;
    HIP_TRY(ctx, hipMemsetAsync(S->d_keys, 0xff, px * 8, st));
    HIP_TRY(ctx, hipMemsetAsync(stats, 0, stats == S->d_stats ? 16 : 12, st));
    hipLaunchKernelGGL(k_maskprop_scatter, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, st, mask_prev, flow, depth_prev, H, W, S->d_keys, stats);
    hipLaunchKernelGGL(k_maskprop_resolve, dim3((W + MP_TW - 1) / MP_TW, (H + MP_TH - 1) / MP_TH), dim3(256), 0, st, (const unsigned long long*)S->d_keys, H, W, out, stats);
    HIP_TRY(ctx, hipGetLastError());
    return VIDO_OK;
}

extern "C" {

int vido_mask_propagate(vido_ctx* ctx, const int32_t* mask_prev, const float* flow, const float* depth_prev, int H, int W, int32_t* out, int32_t* stats_out)
{
    if (!ctx) return VIDO_E_INVALID;
    if (!mask_prev || !flow || !out || out == mask_prev) return vido_set_error(ctx, VIDO_E_INVALID, "mask_propagate: null map, or out aliases mask_prev");
    if (H < 1 || W < 1 || H > 4095 || W > 4095 || (size_t)H * W > (size_t)ctx->cfg.width * ctx->cfg.height)
        return vido_set_error(ctx, VIDO_E_INVALID, "mask_propagate: %d x %d outside the context's %d x %d pixels", W, H, ctx->cfg.width, ctx->cfg.height);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    MaskPropState* S; int rc = maskprop_state(ctx, &S); if (rc) return rc;
    hipStream_t st = ctx->has_ext_stream ? ctx->ext_stream : ctx->stream;
    return maskprop_enqueue(ctx, S, st, mask_prev, flow, depth_prev, H, W, out, stats_out ? stats_out : S->d_stats);
}

int vido_frame_propagate_mask(vido_ctx* ctx, int slot_last, int slot_cur, int32_t* stats_out)
{
    if (!ctx) return VIDO_E_INVALID;
    float *d_last, *f_last, *d_cur, *f_cur; int32_t *m_last, *m_cur; int W = 0, H = 0;
    if (slot_last == slot_cur || track_slot_maps(ctx, slot_last, &d_last, &f_last, &m_last, &W, &H) != VIDO_OK || track_slot_maps(ctx, slot_cur, &d_cur, &f_cur, &m_cur, &W, &H) != VIDO_OK)
        return vido_set_error(ctx, VIDO_E_INVALID, "frame_propagate_mask: bad slots %d -> %d", slot_last, slot_cur);
    if (m_last == m_cur) return vido_set_error(ctx, VIDO_E_INVALID, "frame_propagate_mask: both slots refer to one mask buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    MaskPropState* S; int rc = maskprop_state(ctx, &S); if (rc) return rc;
    hipStream_t st = ctx->stream;                                 // the tracker's stream: the slot maps are ordered on it
    if ((rc = maskprop_enqueue(ctx, S, st, m_last, f_last, d_last, H, W, m_cur, S->d_stats))) return rc;
    if (stats_out) {
        HIP_TRY(ctx, hipMemcpyAsync(S->h_stats, S->d_stats, 12, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        memcpy(stats_out, S->h_stats, 12);
    }
    return VIDO_OK;
}

}  // extern "C"
