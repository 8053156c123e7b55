// patchpts.hip — vido_orb_patch_points: the 8 x 8 grey patch at caller-given points of one frame's pyramid slab, and its zero-mean normalised cross-correlation with a
// caller-given reference patch as an integer verdict (gfx950 only).  The statement is tests/refimpl/patch_points_np.py; every output is equal to it bit for bit.
#include "common.hpp"


// One wave per point, four points per workgroup, lane = pixel (row lane >> 3, column lane & 7), points in caller order; a wave reads nothing but its own point's row of the
// inputs and its own 8 x 8 pixels, so a result depends neither on n nor on the order.  The pixel is ONE byte load per lane: the 8 rows are 8 runs of 8 bytes, i.e. the same
// 8 (at most 16) cache lines an aligned-dword form would touch, but that form needs three dwords per row for x = 1, 2, 3 (mod 4), reads up to 3 bytes outside the patch and
// then shifts bytes across lanes; with one instruction per wave either way the byte form has nothing to win back.  A point whose patch is not wholly inside its level, or
// whose level is out of range, is invalid: status -1, sums 0, zero patch, and no read of the slab at all.
// The verdict is on integers only.  With S1 = sum a, S11 = sum a^2, S12 = sum a b ... over the 64 pixels: var = 64 S11 - S1^2 <= 66 585 600 (0 / 255 checkerboard) and
// |cov| <= sqrt(var_ref var_cur), so the three fit i32, cov^2 and var_ref var_cur fit 53 bits, and  cov^2 2^20 >= q^2 var_ref var_cur  is compared as two 128-bit numbers.
__global__ __launch_bounds__(256) void k_patch_points(const uint8_t* __restrict__ plane, PyrDev P, const int* __restrict__ xyl, int n, const uint8_t* __restrict__ ref,
                                                      int min_var, unsigned min_q, uint8_t* __restrict__ patch_out, int* __restrict__ sums_out, int* __restrict__ status_out)
{
    const int kk = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (kk >= n) return;
    const int x = xyl[3 * kk], y = xyl[3 * kk + 1], level = xyl[3 * kk + 2];
    bool valid = level >= 0 && level < P.n_levels;
    const int lc = valid ? level : 0;
    valid = valid && x >= 4 && x <= P.w[lc] - 4 && y >= 4 && y <= P.h[lc] - 4;      // (x + 3 < w, written so that no sum can wrap for any int x)
    if (!valid) {                                                          // (wave-uniform)
        if (patch_out) patch_out[(size_t)kk * 64 + lane] = 0;
        if (lane == 0) { if (sums_out) { sums_out[3 * (size_t)kk] = 0; sums_out[3 * (size_t)kk + 1] = 0; sums_out[3 * (size_t)kk + 2] = 0; } if (status_out) status_out[kk] = -1; }
        return;
    }
    const int b = plane[(size_t)P.off[level] + (size_t)(y - 4 + (lane >> 3)) * P.pitch[level] + (x - 4 + (lane & 7))];
    if (patch_out) patch_out[(size_t)kk * 64 + lane] = (uint8_t)b;
    if (!ref) return;
    const int a = ref[(size_t)kk * 64 + lane];
    int s1 = a, s2 = b, s11 = a * a, s22 = b * b, s12 = a * b;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); s11 += __shfl_xor(s11, o, 64); s22 += __shfl_xor(s22, o, 64); s12 += __shfl_xor(s12, o, 64); }
    if (lane != 0) return;
    const int var_ref = 64 * s11 - s1 * s1, var_cur = 64 * s22 - s2 * s2, cov = 64 * s12 - s1 * s2;
    if (sums_out) { sums_out[3 * (size_t)kk] = cov; sums_out[3 * (size_t)kk + 1] = var_ref; sums_out[3 * (size_t)kk + 2] = var_cur; }
    if (!status_out) return;
    int st;
    if (var_ref < min_var || var_cur < min_var) st = 2;
    else if (cov <= 0) st = 1;
    else {
        const unsigned long long c2 = (unsigned long long)cov * (unsigned long long)cov, vv = (unsigned long long)var_ref * (unsigned long long)var_cur, q2 = (unsigned long long)min_q * min_q;
        const unsigned long long lhs_hi = c2 >> 44, lhs_lo = c2 << 20, rhs_hi = __umul64hi(vv, q2), rhs_lo = vv * q2;
        st = (lhs_hi > rhs_hi || (lhs_hi == rhs_hi && lhs_lo >= rhs_lo)) ? 0 : 1;
    }
    status_out[kk] = st;
}

extern "C" int vido_orb_patch_points(vido_ctx* ctx, int frame, const int32_t* xyl, int n, int blurred, const uint8_t* ref_patch, int min_var, int min_zncc_q10,
                                     uint8_t* patch_out, int32_t* sums_out, int32_t* status_out, int on_device)
{
    if (!ctx || !ctx->orb) return VIDO_E_INVALID;
    const uint8_t *pyr = nullptr, *blur = nullptr; PyrDev P;
    const int B = orb_frame_planes(ctx, frame, &pyr, &blur, &P);
    if (!B) return vido_set_error(ctx, VIDO_E_INVALID, "patch_points: frame %d outside the context's batch", frame);
    if (n < 0 || (n > 0 && !xyl)) return vido_set_error(ctx, VIDO_E_INVALID, "patch_points: bad point list");
    if ((sums_out || status_out) && !ref_patch) return vido_set_error(ctx, VIDO_E_INVALID, "patch_points: sums and verdicts need reference patches");
    if (min_var < 0) return vido_set_error(ctx, VIDO_E_INVALID, "patch_points: min_var %d is negative", min_var);
    if (min_zncc_q10 < 0 || min_zncc_q10 > 1024) return vido_set_error(ctx, VIDO_E_INVALID, "patch_points: min_zncc_q10 %d outside 0 .. 1024", min_zncc_q10);
    if (blurred && (!ctx->cfg.compute_descriptors || !blur)) return vido_set_error(ctx, VIDO_E_INVALID, "patch_points: the context keeps no blurred pyramid (compute_descriptors = 0)");
    if (on_device && ((((uintptr_t)xyl | (uintptr_t)ref_patch | (uintptr_t)patch_out | (uintptr_t)sums_out | (uintptr_t)status_out) & 3) != 0))
        return vido_set_error(ctx, VIDO_E_INVALID, "patch_points: device pointers must be 4-byte aligned");
    if (n == 0 || (!patch_out && !sums_out && !status_out)) return VIDO_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (!on_device) {                                                      // the host form: from here on the pointers are their slots of the staging buffer
        HostStaging& T = ctx->staging;
        T.begin(); T.in(&xyl, (size_t)n * 12); T.in(&ref_patch, (size_t)n * 64); T.out(&patch_out, (size_t)n * 64); T.out(&sums_out, (size_t)n * 12); T.out(&status_out, (size_t)n * 4);
        if (int rc = staging_upload(ctx, st)) return rc;
    }
    hipLaunchKernelGGL(k_patch_points, dim3((n + 3) / 4), dim3(256), 0, st, blurred ? blur : pyr, P, xyl, n, ref_patch, min_var, (unsigned)min_zncc_q10, patch_out, sums_out, status_out);
    HIP_TRY(ctx, hipGetLastError());
    if (!on_device) return staging_download(ctx, st);              // only what was asked for comes back (the tracker's verification wants 4 bytes per point, its patch taking 64)
    return VIDO_OK;
}
