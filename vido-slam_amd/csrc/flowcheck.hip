// flowcheck.hip — vido_flow_consistency: the forward-backward check of two dense flow fields in 1/256 px, entirely in integers (gfx950 only).  The statement is
// tests/refimpl/flow_consistency_np.py; status, marked flow and counters are equal to it bit for bit.  One launch (k_flow_check, one thread per pixel on k_dis_densify's
// grid) behind a 16-byte memset of the counters, on one stream, no host synchronisation in the device form.  vido_dis_flow_pair (disflow.hip) ends with the same launch
// through flowcheck_enqueue.  Bounds: |f|, |tap| < 2^19, so |s| < 2^35, |b| < 2^19, |r| < 2^20; 1024 |r|^2 < 2^51, alpha_q10 (|f|^2 + |b|^2) < 2^50, 1024 beta_q16 <= 2^40:
// every term stays below 2^52.
#include "common.hpp"

constexpr int FC_LIMIT = 1 << 19;                                  // a component at or past it is not a flow
constexpr unsigned FC_NAN = 0x7FC00000u;

// |v| >= 2^19 as one unsigned comparison (v + 2^19 - 1 wraps for no int32 v at or above -(2^19 - 1), and lands above the bound for every other)
__device__ __forceinline__ bool fc_past(int v) { return (unsigned)v + (unsigned)(FC_LIMIT - 1) > 2u * (FC_LIMIT - 1); }
__device__ __forceinline__ bool fc_not_flow(int2 v) { return fc_past(v.x) || fc_past(v.y); }

// One thread per pixel.  Every index below is inside the field: 0 <= tx <= 256 (W - 1) gives 0 <= x0 <= W - 1, and x1 is clamped (y likewise).  The counters take one wave
// reduction (a ballot per status) and one atomic add per counter and workgroup; integer sums, so no result depends on an execution order.
__global__ __launch_bounds__(256) void k_flow_check(const int2* __restrict__ fwd, const int2* __restrict__ bwd, int H, int W, int alpha, long long beta1024,
                                                    uint8_t* __restrict__ status_out, uint2* __restrict__ marked, int* __restrict__ stats)
{
    __shared__ int s_cnt[4][4];
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const bool in = x < W && y < H;
    int status = -1;
    if (in) {                                                              // (per lane)
        const size_t i = (size_t)y * W + x;
        const int2 f = fwd[i];
        const bool nf = fc_not_flow(f);
        const int tx = nf ? 0 : 256 * x + f.x, ty = nf ? 0 : 256 * y + f.y;      // |t| < 2^21
        if (nf) status = 3;
        else if (tx < 0 || tx > 256 * (W - 1) || ty < 0 || ty > 256 * (H - 1)) status = 2;
        else {
            const int x0 = tx >> 8, ax = tx & 255, y0 = ty >> 8, ay = ty & 255, x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
            const int2 t00 = bwd[(size_t)y0 * W + x0], t01 = bwd[(size_t)y0 * W + x1], t10 = bwd[(size_t)y1 * W + x0], t11 = bwd[(size_t)y1 * W + x1];
            if (fc_not_flow(t00) || fc_not_flow(t01) || fc_not_flow(t10) || fc_not_flow(t11)) status = 3;
            else {
                const long long w00 = (256 - ax) * (256 - ay), w01 = ax * (256 - ay), w10 = (256 - ax) * ay, w11 = ax * ay;
                const long long sx = w00 * t00.x + w01 * t01.x + w10 * t10.x + w11 * t11.x, sy = w00 * t00.y + w01 * t01.y + w10 * t10.y + w11 * t11.y;      // |s| < 2^35
                const long long bx = (sx + 32768) >> 16, by = (sy + 32768) >> 16, rx = f.x + bx, ry = f.y + by;
                const long long lhs = 1024 * (rx * rx + ry * ry);                                                                                           // < 2^51
                const long long rhs = (long long)alpha * ((long long)f.x * f.x + (long long)f.y * f.y + bx * bx + by * by) + beta1024;                      // < 2^51
                status = lhs > rhs ? 1 : 0;
            }
        }
        if (status_out) status_out[i] = (uint8_t)status;
        if (marked) {
            uint2 m = make_uint2(FC_NAN, FC_NAN);
            if (status == 0) { m.x = __float_as_uint((float)f.x * (1.0f / 256.0f)); m.y = __float_as_uint((float)f.y * (1.0f / 256.0f)); }      // exact: |f| < 2^19
            marked[i] = m;
        }
    }
    if (!stats) return;                                                    // (uniform over the grid)
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int c = __popcll(__ballot(status == k));
        if (lane == 0) s_cnt[wv][k] = c;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int cnt = s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
        if (cnt) atomicAdd(&stats[threadIdx.x], cnt);
    }
}

// (also disflow.hip's vido_dis_flow_pair) zeroes stats when given and launches the check; every pointer is a device pointer
hipError_t flowcheck_enqueue(hipStream_t st, const int32_t* fwd, const int32_t* bwd, int H, int W, int alpha_q10, int beta_q16, uint8_t* status, float* marked, int32_t* stats)
{
    if (stats) if (hipError_t e = hipMemsetAsync(stats, 0, 16, st)) return e;
    hipLaunchKernelGGL(k_flow_check, dim3((W + 63) / 64, (H + 3) / 4), dim3(256), 0, st, (const int2*)fwd, (const int2*)bwd, H, W, alpha_q10, 1024ll * beta_q16, status, (uint2*)marked, stats);
    return hipSuccess;
}

// the argument rules the check shares with vido_dis_flow_pair; 0 = fine
int flowcheck_params(vido_ctx* ctx, const char* who, int alpha_q10, int beta_q16)
{
    if (alpha_q10 < 0 || alpha_q10 > 1024) return vido_set_error(ctx, VIDO_E_INVALID, "%s: alpha_q10 %d outside 0 .. 1024", who, alpha_q10);
    if (beta_q16 < 0 || beta_q16 > (1 << 30)) return vido_set_error(ctx, VIDO_E_INVALID, "%s: beta_q16 %d outside 0 .. 2^30", who, beta_q16);
    return VIDO_OK;
}

extern "C" int vido_flow_consistency(vido_ctx* ctx, const int32_t* fwd_q8, const int32_t* bwd_q8, int H, int W, int alpha_q10, int beta_q16, uint8_t* status_out, float* flow_marked_out,
                                     int32_t* stats_out, int on_device)
{
    if (!ctx) return VIDO_E_INVALID;
    if (!fwd_q8 || !bwd_q8) return vido_set_error(ctx, VIDO_E_INVALID, "flow_consistency: null field");
    if (W < 1 || H < 1 || W > 4095 || H > 4095) return vido_set_error(ctx, VIDO_E_INVALID, "flow_consistency: size %d x %d outside 1 .. 4095", W, H);
    if (int rc = flowcheck_params(ctx, "flow_consistency", alpha_q10, beta_q16)) return rc;
    if (!status_out && !flow_marked_out && !stats_out) return vido_set_error(ctx, VIDO_E_INVALID, "flow_consistency: no output asked for");
    if (on_device && ((((uintptr_t)fwd_q8 | (uintptr_t)bwd_q8 | (uintptr_t)flow_marked_out) & 7) != 0 || ((uintptr_t)stats_out & 3) != 0))
        return vido_set_error(ctx, VIDO_E_INVALID, "flow_consistency: device fields and the marked flow must be 8-byte aligned, stats 4-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = on_device && ctx->has_ext_stream ? ctx->ext_stream : ctx->stream;
    if (!on_device) {                                                      // the host form: from here on the five pointers are their slots of the staging buffer
        const size_t px = (size_t)W * H;
        HostStaging& T = ctx->staging;
        T.begin(); T.in(&fwd_q8, px * 8); T.in(&bwd_q8, px * 8); T.out(&flow_marked_out, px * 8); T.out(&stats_out, 16); T.out(&status_out, px);
        if (int rc = staging_upload(ctx, st)) return rc;
    }
    HIP_TRY(ctx, flowcheck_enqueue(st, fwd_q8, bwd_q8, H, W, alpha_q10, beta_q16, status_out, flow_marked_out, stats_out));
    HIP_TRY(ctx, hipGetLastError());
    if (!on_device) return staging_download(ctx, st);
    return VIDO_OK;
}
