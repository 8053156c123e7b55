// disflow.hip — vido_dis_flow: dense optical flow of the Dense Inverse Search kind between two u8 images, to 1/256 px and entirely in integers (gfx950 only): per-patch
// translation-only inverse-compositional Gauss-Newton with a bias term (patchrefine.hip's arithmetic on all 64 pixels of an 8 x 8 patch, e in 1/16 grey) on a factor-2
// pyramid, coarse to fine, each level densified by photometric-weighted averaging.  The statement is tests/refimpl/dis_flow_np.py; every output is equal to it bit for bit.
// Launches of one call, all on one stream, no host synchronisation in the device form: a 16-byte memset of the counters, k_dis_ingest (grey + level 0 of both images),
// k_dis_down per level above 0 (both images), and per level from the coarsest down k_dis_patch then k_dis_densify — separate launches because a level's densification needs
// every patch of the level and no workgroup may wait for another.  Results depend on no execution order: integer sums only, the counters included.
// vido_dis_flow_pair: both directions (image 0 -> 1 and 1 -> 0) from one ingest and one pyramid build — the pyramids are symmetric in the two images — with the direction as a
// grid dimension of k_dis_patch (blockIdx.y) and k_dis_densify (blockIdx.z), so the same number of launches as one direction, and flowcheck.hip's k_flow_check behind them.
#include "common.hpp"

constexpr int DF_MAX_LEVELS = 7;                                   // coarsest in 0..6
constexpr int DF_MAX_ITERS = 16, DF_MAX_SHIFT_Q8 = 2048;
constexpr int DF_MAX_C = (DF_MAX_SHIFT_Q8 + 255) >> 8;             // whole pixels an offset can reach: 8
constexpr int DF_WIN = 9 + 2 * DF_MAX_C;                           // rows and columns of the staged window at the largest C: 25
constexpr int DF_STRIDE = 28;                                      // bytes per staged row

struct DisFlowState {
    // scratch of one (w, h, coarsest): the two pyramids (tight rows, image 1 at +pyr_bytes), the dense fields of the levels above 0 and the patch flows of one level;
    // the pair call: the last two per direction, and both level-0 fields (the check reads them whether or not the caller asks for them)
    uint8_t* d_scratch = nullptr; size_t scratch_cap = 0;
    int32_t* d_stats = nullptr;                                    // the counters (12 words) of a call without a caller's stats buffer
};

struct DisGeom {
    int L, w[DF_MAX_LEVELS], h[DF_MAX_LEVELS], nx[DF_MAX_LEVELS], ny[DF_MAX_LEVELS];
    size_t pyr_off[DF_MAX_LEVELS], pyr_bytes, u_off[2][DF_MAX_LEVELS], up_off[2], q8_off[2], total;      // [direction]
};

static int df_origins(int n) { return ((n - 8) >> 2) + 1 + (((n - 8) & 3) != 0); }

// ndir = 1: vido_dis_flow's layout; 2: the pair call's — the same groups in the same order, each once per direction, then both level-0 fields.  Every offset is a multiple of 8
static DisGeom df_geom(int w, int h, int L, int ndir)
{
    DisGeom G{}; G.L = L; size_t o = 0;
    for (int l = 0; l <= L; l++) {
        G.w[l] = w >> l; G.h[l] = h >> l; G.nx[l] = df_origins(G.w[l]); G.ny[l] = df_origins(G.h[l]);
        G.pyr_off[l] = o; o += ((size_t)G.w[l] * G.h[l] + 15) & ~(size_t)15;
    }
    G.pyr_bytes = o; o *= 2;
    for (int d = 0; d < ndir; d++)                                  // (level 0's field is the caller's q8, or q8_off)
        for (int l = 1; l <= L; l++) { G.u_off[d][l] = o; o += (size_t)G.w[l] * G.h[l] * 8; }
    for (int d = 0; d < ndir; d++) { G.up_off[d] = o; o += (size_t)G.nx[0] * G.ny[0] * 8; }
    if (ndir == 2) for (int d = 0; d < 2; d++) { G.q8_off[d] = o; o += (size_t)w * h * 8; }
    G.total = o;
    return G;
}

// the LDS writes of this wave have landed before any of its lanes reads another lane's
__device__ __forceinline__ void df_wave_lds_sync() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_s_waitcnt(0xc07f); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }

__device__ __forceinline__ int df_wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// a / d to the nearest, halves away from zero; d > 0, |a| < 2^63
__device__ __forceinline__ long long df_rdiv(long long a, long long d)
{
    const unsigned long long m = a < 0 ? 0ull - (unsigned long long)a : (unsigned long long)a, ud = (unsigned long long)d;
    unsigned long long q = m / ud; const unsigned long long r = m - q * ud;
    q += r >= ud - r;
    return a < 0 ? -(long long)q : (long long)q;
}

// rdiv(-32 num, det) clamped to +-256 in two divisions that stay below 2^63: |2 num| = q1 det + r1 (|2 num| < 2^62), then 16 min(q1, 17) + rdiv(16 r1, det) (r1 < det < 2^56)
__device__ __forceinline__ int df_step(long long num, long long det)
{
    const unsigned long long m = 2ull * (num < 0 ? 0ull - (unsigned long long)num : (unsigned long long)num), ud = (unsigned long long)det;
    unsigned long long q1 = m / ud; const unsigned long long r1 = 16ull * (m - q1 * ud);
    if (q1 > 17ull) q1 = 17ull;
    unsigned long long q2 = r1 / ud; const unsigned long long r2 = r1 - q2 * ud;
    q2 += r2 >= ud - r2;
    const unsigned long long q = 16ull * q1 + q2;
    const int qi = q > 256ull ? 256 : (int)q;
    return num > 0 ? -qi : qi;
}

// Grey of both images (blockIdx.z) into level 0 of the two pyramids, one thread per pixel.  CN = 1: the bytes; 3 | 4: OpenCV's 14-bit form, the bits of orb.hip::k_ingest_color
template <int CN>
__global__ __launch_bounds__(256) void k_dis_ingest(const uint8_t* __restrict__ img0, const uint8_t* __restrict__ img1, int stride, int w, int h, int rgb, uint8_t* __restrict__ pyr, size_t pyr_bytes)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const uint8_t* s = (blockIdx.z ? img1 : img0) + (size_t)y * stride + (size_t)x * CN;
    uint32_t g;
    if (CN == 1) g = s[0];
    else { const int c0 = s[0], c1 = s[1], c2 = s[2]; const int b = rgb ? c2 : c0, r = rgb ? c0 : c2; g = (uint32_t)(b * 1868 + c1 * 9617 + r * 4899 + 8192) >> 14; }
    pyr[(size_t)blockIdx.z * pyr_bytes + (size_t)y * w + x] = (uint8_t)g;
}

// One pyramid level of both images (blockIdx.z): the rounded mean of 2 x 2; dw = sw >> 1, dh = sh >> 1, so every source index is inside the source
__global__ __launch_bounds__(256) void k_dis_down(uint8_t* __restrict__ pyr, size_t pyr_bytes, size_t soff, int sw, size_t doff, int dw, int dh)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= dw || y >= dh) return;
    const uint8_t* s = pyr + (size_t)blockIdx.z * pyr_bytes + soff + (size_t)(2 * y) * sw + 2 * x;
    pyr[(size_t)blockIdx.z * pyr_bytes + doff + (size_t)y * dw + x] = (uint8_t)((s[0] + s[1] + s[sw] + s[sw + 1] + 2) >> 2);
}

// origin of patch j along an axis of length n with nreg regular origins 0, 4, ...; j == nreg is the edge-aligned one
__device__ __forceinline__ int df_origin(int j, int nreg, int n) { return j < nreg ? 4 * j : n - 8; }

// cost, bx, by at offset (dx, dy) from u0 for the whole wave; lane = pixel (r, c) of the patch.  (fx0, fy0) = u0 & 255; the window's origin is u0 >> 8 minus C, so
// X = c 256 + fx0 + dx + C 256 >= 0 and ix + 1 <= 8 + 2 C for every |dx| <= 256 C: every index stays inside the staged (9 + 2 C)^2 window.
__device__ __forceinline__ void df_eval(const uint8_t* win, int X0, int Y0, int t, int gx, int gy, int sgx, int sgy, int dx, int dy, long long& cost, long long& bx, long long& by)
{
    const int X = X0 + dx, Y = Y0 + dy, ix = X >> 8, fx = X & 255, iy = Y >> 8, fy = Y & 255;
    const uint8_t* q = win + iy * DF_STRIDE + ix;
    const int I = (256 - fx) * (256 - fy) * q[0] + fx * (256 - fy) * q[1] + (256 - fx) * fy * q[DF_STRIDE] + fx * fy * q[DF_STRIDE + 1];
    const int e = (I - 65536 * t + 2048) >> 12;                            // |e| <= 4080
    const int se = df_wave_sum(e), sxe = df_wave_sum(gx * e), sye = df_wave_sum(gy * e), see = df_wave_sum(e * e);      // 64 * 255 * 4080 < 2^26, 64 * 4080^2 < 2^30.1
    cost = 64ll * see - (long long)se * se;
    bx = 64ll * sxe - (long long)sgx * se;
    by = 64ll * sye - (long long)sgy * se;
}

// One wave per patch, four patches per workgroup, lane = pixel.  The wave stages rows and columns (u0 >> 8) - C .. (u0 >> 8) + 8 + C around the patch of image 1 into its own
// LDS slice with the definition's clamping applied (a clamped coordinate reads the border pixel twice, which is the clamped sample), keeps its pixel's T, gx, gy in registers,
// the sums are wave reductions that leave the total in every lane, and lane 0 alone divides; the step it finds is broadcast, so the loop is wave-uniform.  up[p] = the
// patch's flow.  The four counters take one atomic add per counter and workgroup; no workgroup waits for another.  blockIdx.y = the direction: 0 aligns Ga's patches to Gb
// with (Uc0, up0, stats), 1 Gb's patches to Ga with (Uc1, up1, stats + 4); the choice is wave-uniform, scalar registers only.  A one-direction launch has gridDim.y = 1.
__global__ __launch_bounds__(256) void k_dis_patch(const uint8_t* __restrict__ Ga, const uint8_t* __restrict__ Gb, int w, int h, const int* __restrict__ Uc0 /* null at the coarsest level */,
                                                   const int* __restrict__ Uc1, int w1, int h1, int nx, int ny, int iters, int max_shift, long long min_eig, int* __restrict__ up0,
                                                   int* __restrict__ up1, int* __restrict__ stats)
{
    __shared__ uint8_t s_win[4][DF_WIN * DF_STRIDE];
    __shared__ int s_status[4], s_steps[4];
    const int dir = blockIdx.y;
    const uint8_t* __restrict__ G0 = dir ? Gb : Ga; const uint8_t* __restrict__ G1 = dir ? Ga : Gb;
    const int* __restrict__ Uc = dir ? Uc1 : Uc0; int* __restrict__ up = dir ? up1 : up0;
    stats += 4 * dir;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, p = blockIdx.x * 4 + wv;
    int status = 99, steps = 0;                                            // a wave past the last patch counts nowhere
    if (p < nx * ny) {                                                     // (wave-uniform, like every branch below that is not marked per lane)
        const int jy = p / nx, jx = p - jy * nx;
        const int x0 = df_origin(jx, ((w - 8) >> 2) + 1, w), y0 = df_origin(jy, ((h - 8) >> 2) + 1, h);
        int u0x = 0, u0y = 0;
        if (Uc) { const size_t i = (size_t)min((y0 + 4) >> 1, h1 - 1) * w1 + min((x0 + 4) >> 1, w1 - 1); u0x = 2 * Uc[2 * i]; u0y = 2 * Uc[2 * i + 1]; }
        const int C = (max_shift + 255) >> 8, ws = 9 + 2 * C;
        uint8_t* win = s_win[wv];
        const int ox = x0 + (u0x >> 8) - C, oy = y0 + (u0y >> 8) - C;
        for (int i = lane; i < ws * ws; i += 64) {
            const int r = i / ws, c = i - r * ws;
            win[r * DF_STRIDE + c] = G1[(size_t)min(max(oy + r, 0), h - 1) * w + min(max(ox + c, 0), w - 1)];
        }
        const int r = lane >> 3, c = lane & 7, x = x0 + c, y = y0 + r;
        const uint8_t* row = G0 + (size_t)y * w;
        const int t = row[x], gx = (int)row[min(x + 1, w - 1)] - (int)row[max(x - 1, 0)], gy = (int)G0[(size_t)min(y + 1, h - 1) * w + x] - (int)G0[(size_t)max(y - 1, 0) * w + x];
        df_wave_lds_sync();
        const int sgx = df_wave_sum(gx), sgy = df_wave_sum(gy), sxx = df_wave_sum(gx * gx), syy = df_wave_sum(gy * gy), sxy = df_wave_sum(gx * gy);
        const long long hxx = 64ll * sxx - (long long)sgx * sgx, hyy = 64ll * syy - (long long)sgy * sgy, hxy = 64ll * sxy - (long long)sgx * sgy;
        const long long det = hxx * hyy - hxy * hxy, tr = hxx + hyy;       // H < 2^28, det < 2^56
        int bdx = 0, bdy = 0;                                              // the best iterate, as an offset from u0
        if (det <= 0 || tr < 2 * min_eig || det - min_eig * tr + min_eig * min_eig < 0) status = 1;      // flat; min_eig < 2^31: every term below 2^62
        else {
            const int X0 = (c + C) * 256 + (u0x & 255), Y0 = (r + C) * 256 + (u0y & 255);
            int dx = 0, dy = 0;
            long long cost, bx, by, best;
            df_eval(win, X0, Y0, t, gx, gy, sgx, sgy, 0, 0, cost, bx, by);
            best = cost; status = 0;
            for (int it = 0; it < iters; it++) {
                int sx = 0, sy = 0;
                if (lane == 0) { sx = df_step(hyy * bx - hxy * by, det); sy = df_step(hxx * by - hxy * bx, det); }      // (per lane) |num| < 2^61
                sx = __builtin_amdgcn_readfirstlane(sx); sy = __builtin_amdgcn_readfirstlane(sy);
                if (sx == 0 && sy == 0) break;
                dx += sx; dy += sy; steps++;
                if (abs(dx) > max_shift || abs(dy) > max_shift) { status = 2; bdx = bdy = 0; break; }      // rejected: keeps u0
                df_eval(win, X0, Y0, t, gx, gy, sgx, sgy, dx, dy, cost, bx, by);
                if (cost < best) { best = cost; bdx = dx; bdy = dy; }
            }
        }
        if (lane == 0) { up[2 * (size_t)p] = u0x + bdx; up[2 * (size_t)p + 1] = u0y + bdy; }
    }
    if (lane == 0) { s_status[wv] = status; s_steps[wv] = steps; }
    __syncthreads();
    if (threadIdx.x < 4) {
        int cnt;
        if (threadIdx.x < 3) cnt = (s_status[0] == (int)threadIdx.x) + (s_status[1] == (int)threadIdx.x) + (s_status[2] == (int)threadIdx.x) + (s_status[3] == (int)threadIdx.x);
        else cnt = s_steps[0] + s_steps[1] + s_steps[2] + s_steps[3];
        if (cnt) atomicAdd(&stats[threadIdx.x], cnt);
    }
}

// S(X, Y) of the definition: clamped Q8 coordinates, clamped neighbours
__device__ __forceinline__ int df_sample(const uint8_t* __restrict__ G, int w, int h, int X, int Y)
{
    X = min(max(X, 0), (w - 1) * 256); Y = min(max(Y, 0), (h - 1) * 256);
    const int ix = X >> 8, fx = X & 255, iy = Y >> 8, fy = Y & 255, ix1 = min(ix + 1, w - 1), iy1 = min(iy + 1, h - 1);
    const uint8_t *r0 = G + (size_t)iy * w, *r1 = G + (size_t)iy1 * w;
    return (256 - fx) * (256 - fy) * r0[ix] + fx * (256 - fy) * r0[ix1] + (256 - fx) * fy * r1[ix] + fx * fy * r1[ix1];
}

// One thread per pixel: the photometric-weighted mean of the flows of the 1..9 patches that hold it.  Along an axis the candidates are the regular origins 4 (x >> 2) - 4 and
// 4 (x >> 2) where they exist, and the edge-aligned origin n - 8 (index nreg, when n - 8 is no multiple of 4) from x = n - 8 on.  U (null at level 0 without a q8 output)
// takes the Q8 field, flow (level 0 only, direction 0 only) the same in pixels.  blockIdx.z = the direction, as in k_dis_patch: 1 densifies up1 into U1 with the images swapped.
__global__ __launch_bounds__(256) void k_dis_densify(const uint8_t* __restrict__ Ga, const uint8_t* __restrict__ Gb, int w, int h, const int* __restrict__ up0, const int* __restrict__ up1,
                                                     int nx, int ny, int* __restrict__ U0, int* __restrict__ U1, float* __restrict__ flow)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const int dir = blockIdx.z;
    const uint8_t* __restrict__ G0 = dir ? Gb : Ga; const uint8_t* __restrict__ G1 = dir ? Ga : Gb;
    const int* __restrict__ up = dir ? up1 : up0; int* __restrict__ U = dir ? U1 : U0;
    if (dir) flow = nullptr;
    const int nrx = ((w - 8) >> 2) + 1, nry = ((h - 8) >> 2) + 1;
    int cx[3], cy[3];
    cx[0] = (x >> 2) - 1; cx[1] = x >> 2; cx[2] = (nx > nrx && x >= w - 8) ? nrx : -1;
    cy[0] = (y >> 2) - 1; cy[1] = y >> 2; cy[2] = (ny > nry && y >= h - 8) ? nry : -1;
    if (cx[1] >= nrx) cx[1] = -1;
    if (cx[0] >= nrx) cx[0] = -1;
    if (cy[1] >= nry) cy[1] = -1;
    if (cy[0] >= nry) cy[0] = -1;
    const int t = 65536 * (int)G0[(size_t)y * w + x];
    long long sw = 0, sx = 0, sy = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
#pragma unroll
        for (int b = 0; b < 3; b++) {
            if (cy[a] < 0 || cx[b] < 0) continue;
            const size_t p = (size_t)cy[a] * nx + cx[b];
            const int ux = up[2 * p], uy = up[2 * p + 1];
            const int d = abs(df_sample(G1, w, h, x * 256 + ux, y * 256 + uy) - t) >> 16;
            const int wgt = 65536 / max(1, d);
            sw += wgt; sx += (long long)wgt * ux; sy += (long long)wgt * uy;      // |u| < 2^19: below 2^39
        }
    }
    const int qx = (int)df_rdiv(sx, sw), qy = (int)df_rdiv(sy, sw);        // (sw >= 65536 / 255: the regular or the edge patch holds every pixel)
    const size_t i = (size_t)y * w + x;
    if (U) { U[2 * i] = qx; U[2 * i + 1] = qy; }
    if (flow) { flow[2 * i] = (float)qx * (1.0f / 256.0f); flow[2 * i + 1] = (float)qy * (1.0f / 256.0f); }
}

void disflow_state_destroy(vido_ctx* ctx)
{
    DisFlowState* S = ctx->disflow;
    if (!S) return;
    if (S->d_scratch) (void)hipFree(S->d_scratch);
    if (S->d_stats) (void)hipFree(S->d_stats);
    delete S; ctx->disflow = nullptr;
}

// the argument rules vido_dis_flow and vido_dis_flow_pair share; 0 = fine
static int df_check_args(vido_ctx* ctx, const char* who, const uint8_t* img0, const uint8_t* img1, int channels, int stride, int width, int height, int coarsest, int iters, int max_shift_q8, int min_eig)
{
    if (!img0 || !img1) return vido_set_error(ctx, VIDO_E_INVALID, "%s: null image", who);
    if (width < 16 || height < 16 || width > 4095 || height > 4095) return vido_set_error(ctx, VIDO_E_INVALID, "%s: size %d x %d outside 16 .. 4095", who, width, height);
    if (channels != 1 && channels != 3 && channels != 4) return vido_set_error(ctx, VIDO_E_INVALID, "%s: channels must be 1, 3 or 4 (got %d)", who, channels);
    if (stride < width * channels) return vido_set_error(ctx, VIDO_E_INVALID, "%s: stride %d below width * channels = %d", who, stride, width * channels);
    if (coarsest < 0 || coarsest >= DF_MAX_LEVELS || (std::min(width, height) >> coarsest) < 8)
        return vido_set_error(ctx, VIDO_E_INVALID, "%s: coarsest %d outside 0 .. %d, or min(w, h) >> coarsest below 8", who, coarsest, DF_MAX_LEVELS - 1);
    if (iters < 1 || iters > DF_MAX_ITERS) return vido_set_error(ctx, VIDO_E_INVALID, "%s: iters %d outside 1 .. %d", who, iters, DF_MAX_ITERS);
    if (max_shift_q8 < 0 || max_shift_q8 > DF_MAX_SHIFT_Q8) return vido_set_error(ctx, VIDO_E_INVALID, "%s: max_shift_q8 %d outside 0 .. %d", who, max_shift_q8, DF_MAX_SHIFT_Q8);
    if (min_eig < 0) return vido_set_error(ctx, VIDO_E_INVALID, "%s: min_eig %d is negative", who, min_eig);
    return VIDO_OK;
}

// the state, the counters and a scratch of G.total bytes; the first call of a size waits for earlier calls, which may still read the old scratch
static int df_prepare(vido_ctx* ctx, hipStream_t st, const DisGeom& G)
{
    if (!ctx->disflow) ctx->disflow = new DisFlowState();
    DisFlowState* S = ctx->disflow;
    if (!S->d_stats) HIP_TRY(ctx, hipMalloc((void**)&S->d_stats, 48));
    return vido_grow_device(ctx, st, (void**)&S->d_scratch, &S->scratch_cap, G.total, GROW_EXACT);
}

// The launches of one call on device pointers: the counters' memset (16 bytes per direction), ingest, the pyramid, and per level k_dis_patch and k_dis_densify over ndir
// directions.  q8[d] = direction d's level-0 field (null: not kept; the pair call always gives both), flow = direction 0's in pixels or null.
static hipError_t df_enqueue(DisFlowState* S, hipStream_t st, const DisGeom& G, int ndir, const uint8_t* d_img0, const uint8_t* d_img1, int channels, int rgb_order, int stride, int width, int height,
                       int coarsest, int iters, int max_shift_q8, int min_eig, float* d_flow, int32_t* const q8[2], int32_t* d_stats)
{
    uint8_t* pyr = S->d_scratch;
    if (hipError_t e = hipMemsetAsync(d_stats, 0, 16 * ndir, st)) return e;
    const dim3 blk(256);
    auto grid = [](int w, int h, int z) { return dim3((w + 63) / 64, (h + 3) / 4, z); };
    if (channels == 1)      hipLaunchKernelGGL(k_dis_ingest<1>, grid(width, height, 2), blk, 0, st, d_img0, d_img1, stride, width, height, rgb_order != 0, pyr, G.pyr_bytes);
    else if (channels == 3) hipLaunchKernelGGL(k_dis_ingest<3>, grid(width, height, 2), blk, 0, st, d_img0, d_img1, stride, width, height, rgb_order != 0, pyr, G.pyr_bytes);
    else                    hipLaunchKernelGGL(k_dis_ingest<4>, grid(width, height, 2), blk, 0, st, d_img0, d_img1, stride, width, height, rgb_order != 0, pyr, G.pyr_bytes);
    for (int l = 1; l <= coarsest; l++)
        hipLaunchKernelGGL(k_dis_down, grid(G.w[l], G.h[l], 2), blk, 0, st, pyr, G.pyr_bytes, G.pyr_off[l - 1], G.w[l - 1], G.pyr_off[l], G.w[l], G.h[l]);
    int* up[2] = {(int*)(S->d_scratch + G.up_off[0]), ndir == 2 ? (int*)(S->d_scratch + G.up_off[1]) : nullptr};
    for (int l = coarsest; l >= 0; l--) {
        const uint8_t *g0 = pyr + G.pyr_off[l], *g1 = pyr + G.pyr_bytes + G.pyr_off[l];
        const int *Uc[2] = {nullptr, nullptr}; int* U[2] = {nullptr, nullptr};
        for (int d = 0; d < ndir; d++) {
            if (l < coarsest) Uc[d] = (const int*)(S->d_scratch + G.u_off[d][l + 1]);
            U[d] = l > 0 ? (int*)(S->d_scratch + G.u_off[d][l]) : q8[d];
        }
        const int w1 = l < coarsest ? G.w[l + 1] : 0, h1 = l < coarsest ? G.h[l + 1] : 0, np = G.nx[l] * G.ny[l];
        hipLaunchKernelGGL(k_dis_patch, dim3((np + 3) / 4, ndir), blk, 0, st, g0, g1, G.w[l], G.h[l], Uc[0], Uc[1], w1, h1, G.nx[l], G.ny[l], iters, max_shift_q8, (long long)min_eig, up[0], up[1], d_stats);
        hipLaunchKernelGGL(k_dis_densify, grid(G.w[l], G.h[l], ndir), blk, 0, st, g0, g1, G.w[l], G.h[l], (const int*)up[0], (const int*)up[1], G.nx[l], G.ny[l], U[0], U[1], l == 0 ? d_flow : nullptr);
    }
    return hipSuccess;
}

extern "C" int vido_dis_flow(vido_ctx* ctx, const uint8_t* img0, const uint8_t* img1, int channels, int rgb_order, int stride, int width, int height, int coarsest, int iters,
                             int max_shift_q8, int min_eig, float* flow_out, int32_t* q8_out, int32_t* stats, int on_device)
{
    if (!ctx) return VIDO_E_INVALID;
    if (int rc = df_check_args(ctx, "dis_flow", img0, img1, channels, stride, width, height, coarsest, iters, max_shift_q8, min_eig)) return rc;
    if (!flow_out && !q8_out && !stats) return vido_set_error(ctx, VIDO_E_INVALID, "dis_flow: no output asked for");
    if (on_device && ((((uintptr_t)flow_out | (uintptr_t)q8_out | (uintptr_t)stats) & 3) != 0)) return vido_set_error(ctx, VIDO_E_INVALID, "dis_flow: device outputs must be 4-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = on_device && ctx->has_ext_stream ? ctx->ext_stream : ctx->stream;
    const DisGeom G = df_geom(width, height, coarsest, 1);
    if (int rc = df_prepare(ctx, st, G)) return rc;
    DisFlowState* S = ctx->disflow;
    const size_t img_bytes = (size_t)(height - 1) * stride + (size_t)width * channels, px = (size_t)width * height;
    int32_t* q8[2] = {q8_out, nullptr};
    if (!on_device) {                                                      // the host form: from here on the pointers are their slots of the staging buffer
        HostStaging& T = ctx->staging;
        T.begin(); T.in(&img0, img_bytes); T.in(&img1, img_bytes); T.out(&flow_out, px * 8); T.out(&q8[0], px * 8); T.keep(&stats, 16);
        if (int rc = staging_upload(ctx, st)) return rc;
    }
    HIP_TRY(ctx, df_enqueue(S, st, G, 1, img0, img1, channels, rgb_order, stride, width, height, coarsest, iters, max_shift_q8, min_eig, flow_out, q8, stats ? stats : S->d_stats));
    HIP_TRY(ctx, hipGetLastError());
    if (!on_device) return staging_download(ctx, st);
    return VIDO_OK;
}

extern "C" int vido_dis_flow_pair(vido_ctx* ctx, const uint8_t* img0, const uint8_t* img1, int channels, int rgb_order, int stride, int width, int height, int coarsest, int iters,
                                  int max_shift_q8, int min_eig, int alpha_q10, int beta_q16, float* flow_out, int32_t* fwd_q8_out, int32_t* bwd_q8_out, uint8_t* status_out,
                                  int32_t* stats_out, int on_device)
{
    if (!ctx) return VIDO_E_INVALID;
    if (int rc = df_check_args(ctx, "dis_flow_pair", img0, img1, channels, stride, width, height, coarsest, iters, max_shift_q8, min_eig)) return rc;
    if (int rc = flowcheck_params(ctx, "dis_flow_pair", alpha_q10, beta_q16)) return rc;
    if (!flow_out && !fwd_q8_out && !bwd_q8_out && !status_out && !stats_out) return vido_set_error(ctx, VIDO_E_INVALID, "dis_flow_pair: no output asked for");
    if (on_device && ((((uintptr_t)flow_out | (uintptr_t)fwd_q8_out | (uintptr_t)bwd_q8_out) & 7) != 0 || ((uintptr_t)stats_out & 3) != 0))
        return vido_set_error(ctx, VIDO_E_INVALID, "dis_flow_pair: device flow and q8 outputs must be 8-byte aligned, stats 4-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = on_device && ctx->has_ext_stream ? ctx->ext_stream : ctx->stream;
    const DisGeom G = df_geom(width, height, coarsest, 2);
    if (int rc = df_prepare(ctx, st, G)) return rc;
    DisFlowState* S = ctx->disflow;
    const size_t img_bytes = (size_t)(height - 1) * stride + (size_t)width * channels, px = (size_t)width * height;
    int32_t* q8[2] = {fwd_q8_out, bwd_q8_out};                             // the check reads both fields whether or not the caller asks for them
    if (!on_device) {                                                      // the host form: from here on the pointers are their slots of the staging buffer
        HostStaging& T = ctx->staging;
        T.begin(); T.in(&img0, img_bytes); T.in(&img1, img_bytes); T.out(&flow_out, px * 8); T.keep(&q8[0], px * 8); T.keep(&q8[1], px * 8); T.keep(&stats_out, 48); T.out(&status_out, px);
        if (int rc = staging_upload(ctx, st)) return rc;
    }
    for (int d = 0; d < 2; d++) if (!q8[d]) q8[d] = (int32_t*)(S->d_scratch + G.q8_off[d]);
    int32_t* d_stats = stats_out ? stats_out : S->d_stats;
    HIP_TRY(ctx, df_enqueue(S, st, G, 2, img0, img1, channels, rgb_order, stride, width, height, coarsest, iters, max_shift_q8, min_eig, nullptr, q8, d_stats));
    HIP_TRY(ctx, flowcheck_enqueue(st, q8[0], q8[1], height, width, alpha_q10, beta_q16, status_out, flow_out, d_stats + 8));
    HIP_TRY(ctx, hipGetLastError());
    if (!on_device) return staging_download(ctx, st);
    return VIDO_OK;
}
