// patchsearch.hip — vido_orb_patch_search: the offset inside a square window at which the 8 x 8 patch of one frame's pyramid slab correlates best with a caller-given
// reference patch, the runner-up outside the winner's own peak, and an integer verdict (gfx950 only).  The statement is tests/refimpl/patch_search_np.py; every output
// is equal to it bit for bit.
#include "common.hpp"


constexpr int PS_MAX_R = 16;
constexpr int PS_ROWS = 2 * PS_MAX_R + 8;                          // window rows at the largest radius
constexpr int PS_STRIDE_W = (PS_ROWS + 3) / 4 + 1;                 // dwords per window row: the row itself and one dword more, read (and shifted out) by a candidate at its end
constexpr int PS_MAX_IT = ((2 * PS_MAX_R + 1) * (2 * PS_MAX_R + 1) + 63) / 64;      // candidates per lane: 18

// a lane's, then the wave's, first candidate in the statement's order; cov == 0 (var 1): none.  c = (dy + R) (2R + 1) + (dx + R), so "smaller dy, then smaller dx" is
// "smaller c".
struct PsCand { int cov, var, d2, c; };

// p before q: cov_p^2 var_q > cov_q^2 var_p as exact integers (cov^2 < 2^52, var < 2^26: each side below 2^78), then the smaller distance, then the smaller c.  A lane
// without a candidate (cov 0, var 1) loses against every eligible one and ties with its like, where d2 and c still give all lanes the same answer.
__device__ __forceinline__ bool ps_before(const PsCand& p, const PsCand& q)
{
    const unsigned __int128 l = (unsigned __int128)((unsigned long long)p.cov * (unsigned long long)p.cov) * (unsigned)q.var;
    const unsigned __int128 r = (unsigned __int128)((unsigned long long)q.cov * (unsigned long long)q.cov) * (unsigned)p.var;
    if (l != r) return l > r;
    if (p.d2 != q.d2) return p.d2 < q.d2;
    return p.c < q.c;
}

__device__ __forceinline__ PsCand ps_wave_first(PsCand b)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        PsCand t; t.cov = __shfl_xor(b.cov, o, 64); t.var = __shfl_xor(b.var, o, 64); t.d2 = __shfl_xor(b.d2, o, 64); t.c = __shfl_xor(b.c, o, 64);
        if (ps_before(t, b)) b = t;
    }
    return b;
}

// the LDS writes of this wave have landed before any of its lanes reads another lane's
__device__ __forceinline__ void ps_wave_lds_sync() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_s_waitcnt(0xc07f); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }

// One point by one wave; returns its status.  The wave stages rows y-R-4 .. y+R+3, columns x-R-4 .. x+R+3 of the level into its own LDS slice (bytes outside the level are
// written as 0 and never read from the slab; no candidate uses them) and the reference into 16 registers per lane.  Lane takes candidates lane, lane + 64, ...; a
// candidate's row is three aligned LDS dwords funnel-shifted to its eight bytes, and S2, S22, S12 are six 8-bit dot products per row.  Adjacent lanes read adjacent bytes,
// i.e. the same or the neighbouring dword: LDS serves them as a broadcast, no bank is hit twice with different addresses inside a row of candidates (a group of 32 lanes
// that spans many short rows, radius 1 to 3, can share a bank two-way).  Every lane keeps
// (cov, var) of its <= 18 candidates in registers (statically indexed: the loop is unrolled), so the runner-up, which needs the winner's position, costs no second pass
// over the pixels.
__device__ __forceinline__ int ps_point(const uint8_t* __restrict__ plane, const PyrDev& P, const int* __restrict__ xyl, int kk, const uint8_t* __restrict__ ref, int R, int excl,
                                        int min_var, unsigned min_q, unsigned ratio_q, uint32_t* win, uint32_t* sref, int lane, int* __restrict__ dxy_out, int* __restrict__ sums_out,
                                        int* __restrict__ second_out, int* __restrict__ status_out)
{
    const int x = xyl[3 * (size_t)kk], y = xyl[3 * (size_t)kk + 1], level = xyl[3 * (size_t)kk + 2];
    int status = -1, o_dx = 0, o_dy = 0, o_cov = 0, o_vr = 0, o_vc = 0, o_c2 = 0, o_v2 = 0;
    bool valid = level >= 0 && level < P.n_levels;
    const int lc = valid ? level : 0, w = P.w[lc], h = P.h[lc];
    // candidate centres: [x - R, x + R] cut to [4, w - 4] (64-bit: x is any int)
    valid = valid && std::max((long long)x - R, 4LL) <= std::min((long long)x + R, (long long)w - 4) && std::max((long long)y - R, 4LL) <= std::min((long long)y + R, (long long)h - 4);
    if (valid) {                                                           // (wave-uniform, like every branch below that is not marked per lane)
        if (lane < 16) sref[lane] = ((const uint32_t*)ref)[(size_t)kk * 16 + lane];
        ps_wave_lds_sync();
        uint32_t a[16]; int s1 = 0, s11 = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) { a[i] = sref[i]; s1 = (int)__builtin_amdgcn_udot4(a[i], 0x01010101u, (unsigned)s1, false); s11 = (int)__builtin_amdgcn_udot4(a[i], a[i], (unsigned)s11, false); }
        const int var_ref = 64 * s11 - s1 * s1;
        o_vr = var_ref;
        if (var_ref < min_var) status = 2;
        else {
            const int D = 2 * R + 1, rows = 2 * R + 8, sw = (rows + 3) / 4 + 1, ncand = D * D, ox = x - R - 4, oy = y - R - 4;      // (|x|, |y| are small here: a candidate exists)
            const uint8_t* lv = plane + (size_t)P.off[level]; const int pitch = P.pitch[level];
            for (int i = lane; i < rows * sw; i += 64) {                    // per lane: one dword of the window, byte by byte (the window starts at any alignment)
                const int r = i / sw, gx0 = ox + 4 * (i - r * sw), gy = oy + r;
                uint32_t v = 0;
                if (gy >= 0 && gy < h) {
#pragma unroll
                    for (int j = 0; j < 4; j++) { const int gx = gx0 + j; if (gx >= 0 && gx < w) v |= (uint32_t)lv[(size_t)gy * pitch + gx] << (8 * j); }
                }
                win[i] = v;
            }
            ps_wave_lds_sync();
            int cv[PS_MAX_IT], vc[PS_MAX_IT];
            PsCand best = {0, 1, 0x7fffffff, 0x7fffffff};
#pragma unroll
            for (int it = 0; it < PS_MAX_IT; it++) {
                cv[it] = 0; vc[it] = 1;
                const int c = it * 64 + lane;
                if (it * 64 < ncand && c < ncand) {                         // (per lane)
                    const int iy = c / D, ix = c - iy * D, dx = ix - R, dy = iy - R, px = x + dx, py = y + dy;
                    if (px >= 4 && px <= w - 4 && py >= 4 && py <= h - 4) {
                        const uint32_t* q = win + iy * sw + (ix >> 2); const unsigned sh = ix & 3;
                        int s2 = 0, s22 = 0, s12 = 0;
#pragma unroll
                        for (int r = 0; r < 8; r++) {
                            const uint32_t q0 = q[r * sw], q1 = q[r * sw + 1], q2 = q[r * sw + 2];
                            const uint32_t b0 = __builtin_amdgcn_alignbyte(q1, q0, sh), b1 = __builtin_amdgcn_alignbyte(q2, q1, sh);
                            s2 = (int)__builtin_amdgcn_udot4(b0, 0x01010101u, (unsigned)s2, false); s2 = (int)__builtin_amdgcn_udot4(b1, 0x01010101u, (unsigned)s2, false);
                            s22 = (int)__builtin_amdgcn_udot4(b0, b0, (unsigned)s22, false); s22 = (int)__builtin_amdgcn_udot4(b1, b1, (unsigned)s22, false);
                            s12 = (int)__builtin_amdgcn_udot4(a[2 * r], b0, (unsigned)s12, false); s12 = (int)__builtin_amdgcn_udot4(a[2 * r + 1], b1, (unsigned)s12, false);
                        }
                        const int var_cur = 64 * s22 - s2 * s2, cov = 64 * s12 - s1 * s2;
                        if (var_cur >= min_var && cov > 0) {
                            cv[it] = cov; vc[it] = var_cur;
                            const PsCand t = {cov, var_cur, dx * dx + dy * dy, c};
                            if (ps_before(t, best)) best = t;
                        }
                    }
                }
            }
            best = ps_wave_first(best);
            if (best.cov == 0) status = 1;                                  // no eligible candidate
            else {
                const int iy1 = best.c / D, ix1 = best.c - iy1 * D;
                PsCand sec = {0, 1, 0x7fffffff, 0x7fffffff};
#pragma unroll
                for (int it = 0; it < PS_MAX_IT; it++) {
                    const int c = it * 64 + lane;
                    if (cv[it] > 0) {                                       // (per lane)
                        const int iy = c / D, ix = c - iy * D;
                        if (std::max(abs(ix - ix1), abs(iy - iy1)) > excl) {
                            const PsCand t = {cv[it], vc[it], (ix - R) * (ix - R) + (iy - R) * (iy - R), c};
                            if (ps_before(t, sec)) sec = t;
                        }
                    }
                }
                sec = ps_wave_first(sec);
                o_dx = ix1 - R; o_dy = iy1 - R; o_cov = best.cov; o_vc = best.var;
                if (sec.cov > 0) { o_c2 = sec.cov; o_v2 = sec.var; }
                const unsigned long long c1sq = (unsigned long long)best.cov * (unsigned long long)best.cov;
                const unsigned __int128 gate_l = (unsigned __int128)c1sq << 20, gate_r = (unsigned __int128)((unsigned long long)var_ref * (unsigned long long)best.var) * (min_q * min_q);
                if (!(gate_l >= gate_r)) status = 1;
                else {
                    status = 0;
                    if (ratio_q > 0 && sec.cov > 0) {
                        const unsigned __int128 amb_l = ((unsigned __int128)((unsigned long long)sec.cov * (unsigned long long)sec.cov) * (unsigned)best.var) << 20;
                        const unsigned __int128 amb_r = ((unsigned __int128)c1sq * (unsigned)sec.var) * (ratio_q * ratio_q);
                        if (amb_l > amb_r) status = 3;
                    }
                }
            }
        }
    }
    if (lane == 0) {
        if (dxy_out) { dxy_out[2 * (size_t)kk] = o_dx; dxy_out[2 * (size_t)kk + 1] = o_dy; }
        if (sums_out) { sums_out[3 * (size_t)kk] = o_cov; sums_out[3 * (size_t)kk + 1] = o_vr; sums_out[3 * (size_t)kk + 2] = o_vc; }
        if (second_out) { second_out[2 * (size_t)kk] = o_c2; second_out[2 * (size_t)kk + 1] = o_v2; }
        if (status_out) status_out[kk] = status;
    }
    return status;
}

// One wave per point, four points per workgroup, points in caller order; a wave reads nothing but its own point's row of the inputs and its own window, so a result depends
// neither on n nor on the order.  The five counters take one atomic add per counter and workgroup (at most five, on five addresses), never one per point; no workgroup
// waits for another.
__global__ __launch_bounds__(256) void k_patch_search(const uint8_t* __restrict__ plane, PyrDev P, const int* __restrict__ xyl, int n, const uint8_t* __restrict__ ref, int R, int excl,
                                                      int min_var, unsigned min_q, unsigned ratio_q, int* __restrict__ dxy_out, int* __restrict__ sums_out, int* __restrict__ second_out,
                                                      int* __restrict__ status_out, int* __restrict__ stats_out)
{
    __shared__ uint32_t s_win[4][PS_ROWS * PS_STRIDE_W];
    __shared__ uint32_t s_ref[4][16];
    __shared__ int s_status[4];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, kk = blockIdx.x * 4 + wv;
    int status = 99;                                                       // a wave past the end of the list counts nowhere
    if (kk < n) status = ps_point(plane, P, xyl, kk, ref, R, excl, min_var, min_q, ratio_q, s_win[wv], s_ref[wv], lane, dxy_out, sums_out, second_out, status_out);
    if (lane == 0) s_status[wv] = status;
    __syncthreads();
    if (stats_out && threadIdx.x < 5) {
        const int want = threadIdx.x == 4 ? -1 : (int)threadIdx.x;
        const int cnt = (s_status[0] == want) + (s_status[1] == want) + (s_status[2] == want) + (s_status[3] == want);
        if (cnt) atomicAdd(&stats_out[threadIdx.x], cnt);
    }
}

extern "C" int vido_orb_patch_search(vido_ctx* ctx, int frame, const int32_t* xyl, int n, int blurred, const uint8_t* ref_patch, int radius, int excl, int min_var, int min_zncc_q10,
                                     int peak_ratio_q10, int32_t* dxy_out, int32_t* sums_out, int32_t* second_out, int32_t* status_out, int32_t* stats_out, int on_device)
{
    if (!ctx || !ctx->orb) return VIDO_E_INVALID;
    const uint8_t *pyr = nullptr, *blur = nullptr; PyrDev P;
    const int B = orb_frame_planes(ctx, frame, &pyr, &blur, &P);
    if (!B) return vido_set_error(ctx, VIDO_E_INVALID, "patch_search: frame %d outside the context's batch", frame);
    if (n < 0 || (n > 0 && !xyl)) return vido_set_error(ctx, VIDO_E_INVALID, "patch_search: bad point list");
    if (n > 0 && !ref_patch) return vido_set_error(ctx, VIDO_E_INVALID, "patch_search: no reference patches");
    if (radius < 0 || radius > PS_MAX_R) return vido_set_error(ctx, VIDO_E_INVALID, "patch_search: radius %d outside 0 .. %d", radius, PS_MAX_R);
    if (excl < 1 || excl > 16) return vido_set_error(ctx, VIDO_E_INVALID, "patch_search: excl %d outside 1 .. 16", excl);
    if (min_var < 0) return vido_set_error(ctx, VIDO_E_INVALID, "patch_search: min_var %d is negative", min_var);
    if (min_zncc_q10 < 0 || min_zncc_q10 > 1024) return vido_set_error(ctx, VIDO_E_INVALID, "patch_search: min_zncc_q10 %d outside 0 .. 1024", min_zncc_q10);
    if (peak_ratio_q10 < 0 || peak_ratio_q10 > 1024) return vido_set_error(ctx, VIDO_E_INVALID, "patch_search: peak_ratio_q10 %d outside 0 .. 1024", peak_ratio_q10);
    if (blurred && (!ctx->cfg.compute_descriptors || !blur)) return vido_set_error(ctx, VIDO_E_INVALID, "patch_search: the context keeps no blurred pyramid (compute_descriptors = 0)");
    if (on_device && ((((uintptr_t)xyl | (uintptr_t)ref_patch | (uintptr_t)dxy_out | (uintptr_t)sums_out | (uintptr_t)second_out | (uintptr_t)status_out | (uintptr_t)stats_out) & 3) != 0))
        return vido_set_error(ctx, VIDO_E_INVALID, "patch_search: device pointers must be 4-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (n == 0) {                                                          // a successful no-op that still answers: the counters are zero
        if (stats_out && on_device) HIP_TRY(ctx, hipMemsetAsync(stats_out, 0, 5 * sizeof(int32_t), st));
        if (stats_out && !on_device) memset(stats_out, 0, 5 * sizeof(int32_t));
        return VIDO_OK;
    }
    if (!dxy_out && !sums_out && !second_out && !status_out && !stats_out) return VIDO_OK;
    if (!on_device) {                                                      // the host form: from here on the pointers are their slots of the staging buffer
        HostStaging& T = ctx->staging;
        T.begin(); T.in(&xyl, (size_t)n * 12); T.in(&ref_patch, (size_t)n * 64); T.out(&dxy_out, (size_t)n * 8); T.out(&sums_out, (size_t)n * 12); T.out(&second_out, (size_t)n * 8);
        T.out(&status_out, (size_t)n * 4); T.out(&stats_out, 5 * sizeof(int32_t));
        if (int rc = staging_upload(ctx, st)) return rc;
    }
    if (stats_out) HIP_TRY(ctx, hipMemsetAsync(stats_out, 0, 5 * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_patch_search, dim3((n + 3) / 4), dim3(256), 0, st, blurred ? blur : pyr, P, xyl, n, ref_patch, radius, excl, min_var, (unsigned)min_zncc_q10, (unsigned)peak_ratio_q10,
                       dxy_out, sums_out, second_out, status_out, stats_out);
    HIP_TRY(ctx, hipGetLastError());
    if (!on_device) return staging_download(ctx, st);
    return VIDO_OK;
}
