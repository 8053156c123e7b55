// patchrefine.hip — vido_orb_patch_refine: translation-only inverse-compositional alignment, with a bias term, of a carried 8 x 8 reference patch to one frame's pyramid
// slab, to 1/256 px and entirely in integers (gfx950 only).  The statement is tests/refimpl/patch_refine_np.py; every output is equal to it bit for bit.
#include "common.hpp"


constexpr int PR_N = 36;                                           // interior pixels of the patch: r, c in 1..6
constexpr int PR_MAX_ITERS = 8, PR_MAX_SHIFT_Q8 = 512;
constexpr int PR_MAX_C = (PR_MAX_SHIFT_Q8 + 255) >> 8;             // whole pixels an offset can reach: 2
constexpr int PR_WIN = 7 + 2 * PR_MAX_C;                           // rows and columns of the staged window at the largest C: 11
constexpr int PR_STRIDE = 12;                                      // bytes per staged row

// the LDS writes of this wave have landed before any of its lanes reads another lane's
__device__ __forceinline__ void pr_wave_lds_sync() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_s_waitcnt(0xc07f); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }

__device__ __forceinline__ int pr_wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ long long pr_wave_sum64(long long v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// a / d to the nearest, halves away from zero, clamped to +-256; d > 0, |a| < 2^63
__device__ __forceinline__ int pr_rdiv_clamped(long long a, long long d)
{
    const unsigned long long m = a < 0 ? 0ull - (unsigned long long)a : (unsigned long long)a, ud = (unsigned long long)d;
    unsigned long long q = m / ud; const unsigned long long r = m - q * ud;
    q += r >= ud - r;
    const int qi = q > 256ull ? 256 : (int)q;
    return a < 0 ? -qi : qi;
}

// cost, bx, by at offset (px, py) for the whole wave.  Lane < 36 is the interior pixel (r, c) = (1 + lane / 6, 1 + lane % 6) with window position (wr, wc) at offset 0; the
// other lanes add zeros.  |px|, |py| <= 256 C, so every index stays inside the staged (7 + 2 C)^2 window.
__device__ __forceinline__ void pr_eval(const uint8_t* win, bool active, int wr, int wc, int t, int gx, int gy, int sgx, int sgy, int px, int py, long long& cost, long long& bx, long long& by)
{
    int e = 0;
    if (active) {                                                          // (per lane)
        const int X = wc * 256 + px, Y = wr * 256 + py, ix = X >> 8, fx = X & 255, iy = Y >> 8, fy = Y & 255;
        const uint8_t* q = win + iy * PR_STRIDE + ix;
        const int I = (256 - fx) * (256 - fy) * q[0] + fx * (256 - fy) * q[1] + (256 - fx) * fy * q[PR_STRIDE] + fx * fy * q[PR_STRIDE + 1];
        e = (I - 65536 * t + 128) >> 8;                                    // |e| <= 65 280
    }
    const int se = pr_wave_sum(e), sxe = pr_wave_sum(gx * e), sye = pr_wave_sum(gy * e);      // 36 * 255 * 65 280 < 2^30
    const long long see = pr_wave_sum64((long long)e * e);
    cost = PR_N * see - (long long)se * se;
    bx = (long long)PR_N * sxe - (long long)sgx * se;
    by = (long long)PR_N * sye - (long long)sgy * se;
}

// One point by one wave; returns its status.  The wave stages the reference and rows y-3-C .. y+3+C, columns x-3-C .. x+3+C of the level into its own LDS slice (rule 1
// has them inside the level), lane < 36 keeps its pixel's T, gx, gy in registers, the sums are wave reductions that leave the total in every lane, and lane 0 alone
// divides; the step it finds is broadcast, so the loop is wave-uniform.
__device__ __forceinline__ int pr_point(const uint8_t* __restrict__ plane, const PyrDev& P, const int* __restrict__ xyl, int kk, const uint8_t* __restrict__ ref, int iters, int max_shift,
                                        long long min_eig, uint8_t* win, uint32_t* sref, int lane, int* __restrict__ q8_out, long long* __restrict__ cost_out, int* __restrict__ iters_out,
                                        int* __restrict__ status_out)
{
    const int x = xyl[3 * (size_t)kk], y = xyl[3 * (size_t)kk + 1], level = xyl[3 * (size_t)kk + 2];
    int status = -1, o_qx = 0, o_qy = 0, steps = 0; long long o_c0 = 0, o_cb = 0;
    const int C = (max_shift + 255) >> 8, ws = 7 + 2 * C;
    bool valid = level >= 0 && level < P.n_levels;
    const int lc = valid ? level : 0, w = P.w[lc], h = P.h[lc];
    valid = valid && (long long)x - 3 - C >= 0 && (long long)x + 3 + C <= (long long)w - 1 && (long long)y - 3 - C >= 0 && (long long)y + 3 + C <= (long long)h - 1;      // (64-bit: x is any int)
    if (valid) {                                                           // (wave-uniform, like every branch below that is not marked per lane)
        if (lane < 16) sref[lane] = ((const uint32_t*)ref)[(size_t)kk * 16 + lane];
        const uint8_t* lv = plane + (size_t)P.off[level]; const int pitch = P.pitch[level], ox = x - 3 - C, oy = y - 3 - C;
        for (int i = lane; i < ws * ws; i += 64) { const int r = i / ws, c = i - r * ws; win[r * PR_STRIDE + c] = lv[(size_t)(oy + r) * pitch + (ox + c)]; }
        pr_wave_lds_sync();
        const bool active = lane < PR_N;
        const int r = active ? 1 + lane / 6 : 1, c = active ? 1 + lane % 6 : 1;
        const uint8_t* T = (const uint8_t*)sref;
        const int t = T[r * 8 + c], gx = active ? (int)T[r * 8 + c + 1] - (int)T[r * 8 + c - 1] : 0, gy = active ? (int)T[r * 8 + 8 + c] - (int)T[r * 8 - 8 + c] : 0;
        const int sgx = pr_wave_sum(gx), sgy = pr_wave_sum(gy), sxx = pr_wave_sum(gx * gx), syy = pr_wave_sum(gy * gy), sxy = pr_wave_sum(gx * gy);
        const long long hxx = (long long)PR_N * sxx - (long long)sgx * sgx, hyy = (long long)PR_N * syy - (long long)sgy * sgy, hxy = (long long)PR_N * sxy - (long long)sgx * sgy;
        const long long det = hxx * hyy - hxy * hxy, tr = hxx + hyy;       // H < 2^26.4, det < 2^53
        if (det <= 0 || tr < 2 * min_eig || det - min_eig * tr + min_eig * min_eig < 0) status = 2;      // min_eig < 2^31: every term below 2^62
        else {
            const int wr = r - 1 + C, wc = c - 1 + C;                      // level pixel (x - 4 + c, y - 4 + r) in window coordinates
            int px = 0, py = 0;
            long long cost, bx, by;
            pr_eval(win, active, wr, wc, t, gx, gy, sgx, sgy, 0, 0, cost, bx, by);
            o_c0 = o_cb = cost; status = 0;
            for (int it = 0; it < iters; it++) {
                int dx = 0, dy = 0;
                if (lane == 0) {                                           // (per lane) |2 num| < 2^62.7
                    dx = pr_rdiv_clamped(-2 * (hyy * bx - hxy * by), det); dy = pr_rdiv_clamped(-2 * (hxx * by - hxy * bx), det);
                }
                dx = __builtin_amdgcn_readfirstlane(dx); dy = __builtin_amdgcn_readfirstlane(dy);
                if (dx == 0 && dy == 0) break;
                px += dx; py += dy; steps++;
                if (abs(px) > max_shift || abs(py) > max_shift) { status = 3; o_qx = o_qy = 0; o_cb = o_c0; break; }
                pr_eval(win, active, wr, wc, t, gx, gy, sgx, sgy, px, py, cost, bx, by);
                if (cost < o_cb) { o_cb = cost; o_qx = px; o_qy = py; }
            }
        }
    }
    if (lane == 0) {
        if (q8_out) { q8_out[2 * (size_t)kk] = o_qx; q8_out[2 * (size_t)kk + 1] = o_qy; }
        if (cost_out) { cost_out[2 * (size_t)kk] = o_c0; cost_out[2 * (size_t)kk + 1] = o_cb; }
        if (iters_out) iters_out[kk] = steps;
        if (status_out) status_out[kk] = status;
    }
    return status;
}

// One wave per point, four points per workgroup, points in caller order; a wave reads nothing but its own point's row of the inputs and its own window, so a result depends
// neither on n nor on the order.  The four counters take one atomic add per counter and workgroup, never one per point; no workgroup waits for another.
__global__ __launch_bounds__(256) void k_patch_refine(const uint8_t* __restrict__ plane, PyrDev P, const int* __restrict__ xyl, int n, const uint8_t* __restrict__ ref, int iters, int max_shift,
                                                      long long min_eig, int* __restrict__ q8_out, long long* __restrict__ cost_out, int* __restrict__ iters_out, int* __restrict__ status_out,
                                                      int* __restrict__ stats_out)
{
    __shared__ uint8_t s_win[4][PR_WIN * PR_STRIDE];
    __shared__ uint32_t s_ref[4][16];
    __shared__ int s_status[4];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, kk = blockIdx.x * 4 + wv;
    int status = 99;                                                       // a wave past the end of the list counts nowhere
    if (kk < n) status = pr_point(plane, P, xyl, kk, ref, iters, max_shift, min_eig, s_win[wv], s_ref[wv], lane, q8_out, cost_out, iters_out, status_out);
    if (lane == 0) s_status[wv] = status;
    __syncthreads();
    if (stats_out && threadIdx.x < 4) {
        const int want = threadIdx.x == 0 ? 0 : threadIdx.x == 1 ? 2 : threadIdx.x == 2 ? 3 : -1;
        const int cnt = (s_status[0] == want) + (s_status[1] == want) + (s_status[2] == want) + (s_status[3] == want);
        if (cnt) atomicAdd(&stats_out[threadIdx.x], cnt);
    }
}

extern "C" int vido_orb_patch_refine(vido_ctx* ctx, int frame, const int32_t* xyl, int n, int blurred, const uint8_t* ref_patch, int iters, int max_shift_q8, int min_eig, int32_t* q8_out,
                                     int64_t* cost_out, int32_t* iters_out, int32_t* status_out, int32_t* stats_out, int on_device)
{
    if (!ctx || !ctx->orb) return VIDO_E_INVALID;
    const uint8_t *pyr = nullptr, *blur = nullptr; PyrDev P;
    const int B = orb_frame_planes(ctx, frame, &pyr, &blur, &P);
    if (!B) return vido_set_error(ctx, VIDO_E_INVALID, "patch_refine: frame %d outside the context's batch", frame);
    if (n < 0 || (n > 0 && !xyl)) return vido_set_error(ctx, VIDO_E_INVALID, "patch_refine: bad point list");
    if (n > 0 && !ref_patch) return vido_set_error(ctx, VIDO_E_INVALID, "patch_refine: no reference patches");
    if (iters < 1 || iters > PR_MAX_ITERS) return vido_set_error(ctx, VIDO_E_INVALID, "patch_refine: iters %d outside 1 .. %d", iters, PR_MAX_ITERS);
    if (max_shift_q8 < 0 || max_shift_q8 > PR_MAX_SHIFT_Q8) return vido_set_error(ctx, VIDO_E_INVALID, "patch_refine: max_shift_q8 %d outside 0 .. %d", max_shift_q8, PR_MAX_SHIFT_Q8);
    if (min_eig < 0) return vido_set_error(ctx, VIDO_E_INVALID, "patch_refine: min_eig %d is negative", min_eig);
    if (blurred && (!ctx->cfg.compute_descriptors || !blur)) return vido_set_error(ctx, VIDO_E_INVALID, "patch_refine: the context keeps no blurred pyramid (compute_descriptors = 0)");
    if (on_device && (((((uintptr_t)xyl | (uintptr_t)ref_patch | (uintptr_t)q8_out | (uintptr_t)iters_out | (uintptr_t)status_out | (uintptr_t)stats_out) & 3) != 0) || ((uintptr_t)cost_out & 7) != 0))
        return vido_set_error(ctx, VIDO_E_INVALID, "patch_refine: device pointers must be 4-byte aligned (cost_out: 8-byte)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (n == 0) {                                                          // a successful no-op that still answers: the counters are zero
        if (stats_out && on_device) HIP_TRY(ctx, hipMemsetAsync(stats_out, 0, 4 * sizeof(int32_t), st));
        if (stats_out && !on_device) memset(stats_out, 0, 4 * sizeof(int32_t));
        return VIDO_OK;
    }
    if (!q8_out && !cost_out && !iters_out && !status_out && !stats_out) return VIDO_OK;
    if (!on_device) {                                                      // the host form: from here on the pointers are their slots of the staging buffer
        HostStaging& T = ctx->staging;
        T.begin(); T.in(&xyl, (size_t)n * 12); T.in(&ref_patch, (size_t)n * 64); T.out(&cost_out, (size_t)n * 16); T.out(&q8_out, (size_t)n * 8); T.out(&iters_out, (size_t)n * 4);
        T.out(&status_out, (size_t)n * 4); T.out(&stats_out, 4 * sizeof(int32_t));
        if (int rc = staging_upload(ctx, st)) return rc;
    }
    if (stats_out) HIP_TRY(ctx, hipMemsetAsync(stats_out, 0, 4 * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_patch_refine, dim3((n + 3) / 4), dim3(256), 0, st, blurred ? blur : pyr, P, xyl, n, ref_patch, iters, max_shift_q8, (long long)min_eig, q8_out, (long long*)cost_out, iters_out, status_out, stats_out);
    HIP_TRY(ctx, hipGetLastError());
    if (!on_device) return staging_download(ctx, st);
    return VIDO_OK;
}
