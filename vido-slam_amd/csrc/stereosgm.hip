// stereosgm.hip — vido_stereo_sgm: semi-global matching of a rectified u8 pair to 1/16 px, entirely in integers (gfx950 only): 9 x 7 census, Hamming cost, eight
// aggregation paths, winner with sub-pixel parabola, and a left-right, a uniqueness and a zero-disparity verdict per pixel.  The statement is
// tests/refimpl/stereo_sgm_np.py; every output is equal to it bit for bit.
// Launches of one call, all on one stream, no host synchronisation in the device form: k_sgm_zero (the S volume and the four counters), k_sgm_ingest (grey
// of both images), k_sgm_census (both images), ONE k_sgm_path launch over the eight directions (blockIdx.y) and k_sgm_select.  The cost C is never stored: it is one
// xor and popcount of two census words.  S (u16 [h][w][D], S <= 8 (64 + p2) <= 8512) is the traffic: every path wave adds its L into S with packed 32-bit atomic adds of
// two u16 cells (no cell can carry into its neighbour, and integer sums do not depend on the order), so that the eight directions run side by side — a path is a chain
// of w or h dependent steps of a few hundred cycles each, and eight times as many waves in flight is what shortens the call.  Results depend on no execution order.
#include "common.hpp"

constexpr int SG_BIG = 1 << 20;                                    // above every L plus a penalty; a disparity outside [0, D) holds it and is never a candidate
constexpr int SG_MAX_W = 4095;

struct StereoState {
    // scratch of one (w, h, D): [grey left | grey right | census left | census right | S], each 16-byte aligned
    uint8_t* d_scratch = nullptr; size_t scratch_cap = 0;
    int32_t* d_stats = nullptr;                                    // the counters of a call without a caller's stats buffer
};

struct SgmGeom { size_t grey_bytes, o_cen, cen_bytes, o_S, S_bytes, total; };

static SgmGeom sg_geom(int w, int h, int D)
{
    SgmGeom G{}; const size_t px = (size_t)w * h;
    G.grey_bytes = (px + 15) & ~(size_t)15; G.o_cen = 2 * G.grey_bytes; G.cen_bytes = px * 8; G.o_S = G.o_cen + 2 * G.cen_bytes; G.S_bytes = px * D * 2;
    G.total = G.o_S + G.S_bytes;
    return G;
}

// S = 0 in 16-byte stores (n16 of them: the volume's bytes are a multiple of 32) and the four counters = 0, grid-stride
__global__ __launch_bounds__(256) void k_sgm_zero(uint4* __restrict__ S, size_t n16, int32_t* __restrict__ stats)
{
    const size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i0 < 4) stats[i0] = 0;
    for (size_t i = i0; i < n16; i += (size_t)gridDim.x * 256) S[i] = make_uint4(0, 0, 0, 0);
}

// Grey of both images (blockIdx.z) into tight planes, one thread per pixel: disflow.hip::k_dis_ingest's rule
template <int CN>
__global__ __launch_bounds__(256) void k_sgm_ingest(const uint8_t* __restrict__ img0, const uint8_t* __restrict__ img1, int stride, int w, int h, int rgb, uint8_t* __restrict__ grey, size_t plane)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const uint8_t* s = (blockIdx.z ? img1 : img0) + (size_t)y * stride + (size_t)x * CN;
    uint32_t g;
    if (CN == 1) g = s[0];
    else { const int c0 = s[0], c1 = s[1], c2 = s[2]; const int b = rgb ? c2 : c0, r = rgb ? c0 : c2; g = (uint32_t)(b * 1868 + c1 * 9617 + r * 4899 + 8192) >> 14; }
    grey[(size_t)blockIdx.z * plane + (size_t)y * w + x] = (uint8_t)g;
}

// Census of both images (blockIdx.z), one thread per pixel: the 62 neighbours of the 9 x 7 window row-major, coordinates clamped, bit = neighbour < centre
__global__ __launch_bounds__(256) void k_sgm_census(const uint8_t* __restrict__ grey, size_t plane, int w, int h, uint64_t* __restrict__ cen)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const uint8_t* g = grey + (size_t)blockIdx.z * plane;
    const int c = g[(size_t)y * w + x];
    uint64_t word = 0;
#pragma unroll
    for (int dy = -3; dy <= 3; dy++) {
        const uint8_t* row = g + (size_t)min(max(y + dy, 0), h - 1) * w;
#pragma unroll
        for (int dx = -4; dx <= 4; dx++)
            if (dx != 0 || dy != 0) word = (word << 1) | (uint64_t)(row[min(max(x + dx, 0), w - 1)] < c);
    }
    cen[(size_t)blockIdx.z * ((size_t)w * h) + (size_t)y * w + x] = word;
}

// One wave per workgroup walks 64 / G lines of one direction (blockIdx.y; the statement's order (1,0) (-1,0) (0,1) (0,-1) (1,1) (-1,1) (1,-1) (-1,-1)); G lanes hold a
// line's D disparities, DPL consecutive ones per lane (lanes whose disparities lie at or past D hold SG_BIG and store nothing).  A horizontal line is a row walked along
// x.  Every other line starts at a column of the first row and moves one row per step and dx columns, wrapping round the image: the step that wraps has entered from the
// side, so it restarts (L = C) — every pixel of a row is met by exactly one line, and all lines are h steps long.  min_k is a reduction over the G lanes, d +- 1 a lane
// shift plus the in-register neighbour.  The census words of the next step are loaded before this step's recurrence.  Cells of S touched by a lane: DPL consecutive u16,
// added as packed 32-bit words (DPL = 1: the even lane adds its own cell and its odd neighbour's).
template <int DPL, int G>
__global__ __launch_bounds__(64) void k_sgm_path(const uint64_t* __restrict__ cl, const uint64_t* __restrict__ cr, uint16_t* __restrict__ S, int w, int h, int D, int p1, int p2)
{
    const int dir = blockIdx.y;
    const int dx = dir < 2 ? (dir == 0 ? 1 : -1) : dir < 4 ? 0 : ((dir & 1) ? -1 : 1);
    const int dy = dir < 2 ? 0 : dir < 4 ? (dir == 2 ? 1 : -1) : (dir < 6 ? 1 : -1);
    const int nlines = dy == 0 ? h : w, nsteps = dy == 0 ? w : h;
    const int l0 = blockIdx.x * (64 / G);
    if (l0 >= nlines) return;                                              // (the whole wave)
    const int lane = threadIdx.x, li = lane & (G - 1), l = l0 + lane / G;
    const bool live = l < nlines;
    const int lc = min(l, nlines - 1), d0 = li * DPL;
    const bool has = d0 < D;                                               // D and d0 are multiples of DPL: a lane's disparities are inside or outside together
    int x = dy == 0 ? (dx > 0 ? 0 : w - 1) : lc, y = dy == 0 ? lc : (dy > 0 ? 0 : h - 1);
    int Lp[DPL];
    uint64_t a, b[DPL];
    a = cl[(size_t)y * w + x];
#pragma unroll
    for (int j = 0; j < DPL; j++) { Lp[j] = SG_BIG; b[j] = cr[(size_t)y * w + max(x - d0 - j, 0)]; }
    bool restart = true;
    for (int t = 0; t < nsteps; t++) {
        int xn = x + dx; const int yn = y + dy; bool restart_n = false;
        if (dy != 0) { if (xn >= w) { xn = 0; restart_n = true; } else if (xn < 0) { xn = w - 1; restart_n = true; } }
        uint64_t an = 0, bn[DPL];
#pragma unroll
        for (int j = 0; j < DPL; j++) bn[j] = 0;
        if (t + 1 < nsteps) {                                              // (wave-uniform) inside the image: 0 <= xn < w, 0 <= yn < h
            an = cl[(size_t)yn * w + xn];
#pragma unroll
            for (int j = 0; j < DPL; j++) bn[j] = cr[(size_t)yn * w + max(xn - d0 - j, 0)];
        }
        int mloc = Lp[0];
#pragma unroll
        for (int j = 1; j < DPL; j++) mloc = min(mloc, Lp[j]);
#pragma unroll
        for (int o = G >> 1; o >= 1; o >>= 1) mloc = min(mloc, __shfl_xor(mloc, o, 64));
        int up = __shfl_up(Lp[DPL - 1], 1, 64), dn = __shfl_down(Lp[0], 1, 64);
        if (li == 0) up = SG_BIG;
        if (li == G - 1) dn = SG_BIG;
        int L[DPL];
#pragma unroll
        for (int j = 0; j < DPL; j++) {
            const int c = x - d0 - j >= 0 ? __popcll(a ^ b[j]) : 64;
            const int lo = j > 0 ? Lp[j - 1] : up, hi = j < DPL - 1 ? Lp[j + 1] : dn;
            const int best = min(min(Lp[j], mloc + p2), min(lo, hi) + p1);
            L[j] = !has ? SG_BIG : restart ? c : c + best - mloc;
        }
        const size_t cell = ((size_t)y * w + x) * D + d0;                  // even: D is a multiple of 16, d0 = li DPL with li even where it is used for DPL = 1
        if (DPL == 1) {
            const int odd = __shfl_down(L[0], 1, 64);
            if (live && has && !(li & 1)) atomicAdd(reinterpret_cast<unsigned*>(S + cell), (unsigned)L[0] | ((unsigned)odd << 16));
        } else if (live && has) {
#pragma unroll
            for (int j = 0; j < DPL; j += 2) atomicAdd(reinterpret_cast<unsigned*>(S + cell + j), (unsigned)L[j] | ((unsigned)L[j + (DPL > 1)] << 16));
        }
#pragma unroll
        for (int j = 0; j < DPL; j++) { Lp[j] = L[j]; b[j] = bn[j]; }
        a = an; x = xn; y = yn; restart = restart_n;
    }
}

// One workgroup per image row.  First, 64 / GS pixels per wave and step, GS lanes per pixel, 8 consecutive disparities per lane (one 16-byte load): key = S << 8 | d, so
// the minimum key is (s0, d0) with the lowest d on ties; every cell also bids its key for the right view's pixel x - d with an LDS atomic min (dR of the row, at most
// 4095 entries; a minimum does not depend on the order).  S2 and S(d0 +- 1) are two more reductions over the GS lanes; the pixel's first lane finishes q4 and the
// uniqueness verdict into LDS.  Then one thread per pixel: the left-right check against dR, the status, the outputs (each may be null), four counters per workgroup.
__global__ __launch_bounds__(256) void k_sgm_select(const uint16_t* __restrict__ S, int w, int D, int gs_log2, int uniqueness, int lr_tol, float* __restrict__ disp,
                                                    int32_t* __restrict__ q4_out, uint8_t* __restrict__ status, int32_t* __restrict__ stats)
{
    __shared__ unsigned s_key[SG_MAX_W + 1];
    __shared__ int s_q4[SG_MAX_W + 1];
    __shared__ uint8_t s_d0[SG_MAX_W + 1], s_dup[SG_MAX_W + 1];
    __shared__ int s_cnt[4][4];
    const int y = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    for (int i = tid; i < w; i += 256) s_key[i] = 0xffffffffu;
    __syncthreads();
    const uint16_t* row = S + (size_t)y * w * D;
    const int GS = 1 << gs_log2, ppw = 64 >> gs_log2, li = lane & (GS - 1), dl = li * 8;
    const bool has = dl < D;                                               // D is a multiple of 16: a lane's eight disparities are inside or outside together
    for (int xb = wv * ppw; xb < w; xb += 4 * ppw) {                       // (wave-uniform)
        const int x = xb + (lane >> gs_log2);
        const bool live = x < w && has;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (live) v = *reinterpret_cast<const uint4*>(row + (size_t)x * D + dl);      // 16-byte aligned: (x D + dl) is a multiple of 8 cells
        int s[8] = {(int)(v.x & 0xffff), (int)(v.x >> 16), (int)(v.y & 0xffff), (int)(v.y >> 16), (int)(v.z & 0xffff), (int)(v.z >> 16), (int)(v.w & 0xffff), (int)(v.w >> 16)};
        unsigned kmin = 0x7fffffffu;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const unsigned key = ((unsigned)s[j] << 8) | (unsigned)(dl + j);
            if (has) kmin = min(kmin, key);
            if (live && x - dl - j >= 0) atomicMin(&s_key[x - dl - j], key);
        }
        for (int o = GS >> 1; o >= 1; o >>= 1) kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, o, 64));
        const int d0 = (int)(kmin & 255u), s0 = (int)(kmin >> 8);
        int s2 = SG_BIG; unsigned mp = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int d = dl + j;
            if (has && abs(d - d0) > 1) s2 = min(s2, s[j]);
            if (has && d == d0 - 1) mp |= (unsigned)s[j] << 16;
            if (has && d == d0 + 1) mp |= (unsigned)s[j];
        }
        for (int o = GS >> 1; o >= 1; o >>= 1) { s2 = min(s2, __shfl_xor(s2, o, 64)); mp |= (unsigned)__shfl_xor((int)mp, o, 64); }
        if (li == 0 && x < w) {
            const int sm = (int)(mp >> 16), sp = (int)(mp & 0xffff), den = sm + sp - 2 * s0;
            int off = 0;
            if (d0 >= 1 && d0 <= D - 2 && den > 0) {                       // rdiv(8 (sm - sp), den): to the nearest, halves away from zero
                const int a = 8 * (sm - sp), m = abs(a); int q = m / den; const int r = m - q * den;
                q += r >= den - r;
                off = a < 0 ? -q : q;
            }
            s_q4[x] = 16 * d0 + off; s_d0[x] = (uint8_t)d0; s_dup[x] = (uint8_t)((100 - uniqueness) * s2 <= 100 * s0);
        }
    }
    __syncthreads();
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int x = tid; x < w; x += 256) {
        const int d0 = s_d0[x], q4 = s_q4[x], xr = x - d0;
        int st;
        if (xr < 0 || abs((int)(s_key[max(xr, 0)] & 255u) - d0) > lr_tol) st = 2;
        else if (s_dup[x]) st = 1;
        else if (q4 <= 0) st = 3;
        else st = 0;
        const size_t i = (size_t)y * w + x;
        if (disp) disp[i] = st == 0 ? (float)q4 * (1.0f / 16.0f) : -1.0f;
        if (q4_out) q4_out[i] = q4;
        if (status) status[i] = (uint8_t)st;
        c0 += st == 0; c1 += st == 1; c2 += st == 2; c3 += st == 3;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { c0 += __shfl_xor(c0, o, 64); c1 += __shfl_xor(c1, o, 64); c2 += __shfl_xor(c2, o, 64); c3 += __shfl_xor(c3, o, 64); }
    if (lane == 0) { s_cnt[wv][0] = c0; s_cnt[wv][1] = c1; s_cnt[wv][2] = c2; s_cnt[wv][3] = c3; }
    __syncthreads();
    if (tid < 4) {
        const int cnt = s_cnt[0][tid] + s_cnt[1][tid] + s_cnt[2][tid] + s_cnt[3][tid];
        if (cnt) atomicAdd(&stats[tid], cnt);
    }
}

void stereo_state_destroy(vido_ctx* ctx)
{
    StereoState* S = ctx->stereo;
    if (!S) return;
    if (S->d_scratch) (void)hipFree(S->d_scratch);
    if (S->d_stats) (void)hipFree(S->d_stats);
    delete S; ctx->stereo = nullptr;
}

// the state, the counters and a scratch of G.total bytes; the first call of a size waits for earlier calls, which may still read the old scratch
static int sg_prepare(vido_ctx* ctx, hipStream_t st, const SgmGeom& G)
{
    if (!ctx->stereo) ctx->stereo = new StereoState();
    StereoState* S = ctx->stereo;
    if (!S->d_stats) HIP_TRY(ctx, hipMalloc((void**)&S->d_stats, 16));
    return vido_grow_device(ctx, st, (void**)&S->d_scratch, &S->scratch_cap, G.total, GROW_EXACT);
}

// the launches of one call on device pointers
static hipError_t sg_enqueue(StereoState* St, hipStream_t st, const SgmGeom& G, const uint8_t* d_left, const uint8_t* d_right, int channels, int rgb_order, int stride, int w, int h, int D,
                             int p1, int p2, int uniqueness, int lr_tol, float* d_disp, int32_t* d_q4, uint8_t* d_status, int32_t* d_stats)
{
    uint8_t* grey = St->d_scratch; uint64_t* cen = (uint64_t*)(St->d_scratch + G.o_cen); uint16_t* S = (uint16_t*)(St->d_scratch + G.o_S);
    const uint64_t *cl = cen, *cr = cen + (size_t)w * h;
    const size_t n16 = G.S_bytes / 16;
    hipLaunchKernelGGL(k_sgm_zero, dim3((unsigned)std::min<size_t>((n16 + 255) / 256, 4096)), dim3(256), 0, st, (uint4*)S, n16, d_stats);
    const dim3 blk(256), grid((w + 63) / 64, (h + 3) / 4, 2);
    if (channels == 1)      hipLaunchKernelGGL(k_sgm_ingest<1>, grid, blk, 0, st, d_left, d_right, stride, w, h, rgb_order != 0, grey, G.grey_bytes);
    else if (channels == 3) hipLaunchKernelGGL(k_sgm_ingest<3>, grid, blk, 0, st, d_left, d_right, stride, w, h, rgb_order != 0, grey, G.grey_bytes);
    else                    hipLaunchKernelGGL(k_sgm_ingest<4>, grid, blk, 0, st, d_left, d_right, stride, w, h, rgb_order != 0, grey, G.grey_bytes);
    hipLaunchKernelGGL(k_sgm_census, grid, blk, 0, st, (const uint8_t*)grey, G.grey_bytes, w, h, cen);
    const int nl = std::max(w, h);
    auto pgrid = [&](int g) { const int lpw = 64 / g; return dim3((nl + lpw - 1) / lpw, 8); };
    if (D <= 16)       hipLaunchKernelGGL((k_sgm_path<1, 16>), pgrid(16), dim3(64), 0, st, cl, cr, S, w, h, D, p1, p2);
    else if (D <= 32)  hipLaunchKernelGGL((k_sgm_path<1, 32>), pgrid(32), dim3(64), 0, st, cl, cr, S, w, h, D, p1, p2);
    else if (D <= 64)  hipLaunchKernelGGL((k_sgm_path<1, 64>), pgrid(64), dim3(64), 0, st, cl, cr, S, w, h, D, p1, p2);
    else if (D <= 128) hipLaunchKernelGGL((k_sgm_path<2, 64>), pgrid(64), dim3(64), 0, st, cl, cr, S, w, h, D, p1, p2);
    else               hipLaunchKernelGGL((k_sgm_path<4, 64>), pgrid(64), dim3(64), 0, st, cl, cr, S, w, h, D, p1, p2);
    int gs_log2 = 1;                                                       // lanes per pixel of the selection: the power of two at or above D / 8
    while ((8 << gs_log2) < D) gs_log2++;
    hipLaunchKernelGGL(k_sgm_select, dim3(h), blk, 0, st, (const uint16_t*)S, w, D, gs_log2, uniqueness, lr_tol, d_disp, d_q4, d_status, d_stats);
    return hipSuccess;
}

extern "C" int vido_stereo_sgm(vido_ctx* ctx, const uint8_t* left, const uint8_t* right, int channels, int rgb_order, int stride, int width, int height, int max_disp, int p1, int p2,
                               int uniqueness, int lr_tol, float* disp_out, int32_t* q4_out, uint8_t* status_out, int32_t* stats_out, int on_device)
{
    if (!ctx) return VIDO_E_INVALID;
    if (!left || !right) return vido_set_error(ctx, VIDO_E_INVALID, "stereo_sgm: null image");
    if (width < 16 || height < 16 || width > SG_MAX_W || height > SG_MAX_W) return vido_set_error(ctx, VIDO_E_INVALID, "stereo_sgm: size %d x %d outside 16 .. 4095", width, height);
    if (channels != 1 && channels != 3 && channels != 4) return vido_set_error(ctx, VIDO_E_INVALID, "stereo_sgm: channels must be 1, 3 or 4 (got %d)", channels);
    if (stride < width * channels) return vido_set_error(ctx, VIDO_E_INVALID, "stereo_sgm: stride %d below width * channels = %d", stride, width * channels);
    if (max_disp < 16 || max_disp > 256 || (max_disp & 15) != 0) return vido_set_error(ctx, VIDO_E_INVALID, "stereo_sgm: max_disp %d is no multiple of 16 in 16 .. 256", max_disp);
    if ((long long)width * height * max_disp > (1ll << 28)) return vido_set_error(ctx, VIDO_E_INVALID, "stereo_sgm: volume width * height * max_disp = %lld above 2^28", (long long)width * height * max_disp);
    if (p1 < 0 || p2 < p1 || p2 > 1000) return vido_set_error(ctx, VIDO_E_INVALID, "stereo_sgm: penalties p1 %d, p2 %d outside 0 <= p1 <= p2 <= 1000", p1, p2);
    if (uniqueness < 0 || uniqueness > 99) return vido_set_error(ctx, VIDO_E_INVALID, "stereo_sgm: uniqueness %d outside 0 .. 99", uniqueness);
    if (lr_tol < 0 || lr_tol > 255) return vido_set_error(ctx, VIDO_E_INVALID, "stereo_sgm: lr_tol %d outside 0 .. 255", lr_tol);
    if (!disp_out && !q4_out && !status_out && !stats_out) return vido_set_error(ctx, VIDO_E_INVALID, "stereo_sgm: no output asked for");
    if (on_device && ((((uintptr_t)disp_out | (uintptr_t)q4_out | (uintptr_t)stats_out) & 3) != 0)) return vido_set_error(ctx, VIDO_E_INVALID, "stereo_sgm: device outputs must be 4-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = on_device && ctx->has_ext_stream ? ctx->ext_stream : ctx->stream;
    const SgmGeom G = sg_geom(width, height, max_disp);
    if (int rc = sg_prepare(ctx, st, G)) return rc;
    StereoState* S = ctx->stereo;
    const size_t img_bytes = (size_t)(height - 1) * stride + (size_t)width * channels, px = (size_t)width * height;
    if (!on_device) {                                                      // the host form: from here on the pointers are their slots of the staging buffer
        HostStaging& T = ctx->staging;
        T.begin(); T.in(&left, img_bytes); T.in(&right, img_bytes); T.out(&disp_out, px * 4); T.out(&q4_out, px * 4); T.keep(&stats_out, 16); T.out(&status_out, px);
        if (int rc = staging_upload(ctx, st)) return rc;
    }
    HIP_TRY(ctx, sg_enqueue(S, st, G, left, right, channels, rgb_order, stride, width, height, max_disp, p1, p2, uniqueness, lr_tol, disp_out, q4_out, status_out,
                            stats_out ? stats_out : S->d_stats));
    HIP_TRY(ctx, hipGetLastError());
    if (!on_device) return staging_download(ctx, st);
    return VIDO_OK;
}
