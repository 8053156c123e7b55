// The detector's stem as ONE launch: maxpool3x3s2p1(relu(conv7x7s2p3(x, w) + bias)) for one image, 3 -> 64 channels (maskrcnn_benchmark resnet.py:375-395 with the frozen
// batch norm folded into w / bias, nets/fuse.py).
//
// What it replaces: the library's 7x7 stride-2 convolution, our bias + ReLU pass over its output and the framework's max-pool — at 800 x 1088 the 64 x 400 x 544 map (55.7 MB)
// is written, read and rewritten, and read again: ~220 MB of traffic for 13.9 MB of result computed from a 10 MB image.  Here that map never reaches memory.
//
// A workgroup (4 waves) owns 7 x 8 pooled outputs of one 32-channel half.  Their pool windows cover 15 x 17 = 255 convolution outputs, which read a 35 x 39 window of
// each of the 3 image planes: staged once in LDS (zeros outside the image = the convolution's padding).  The convolution is an implicit GEMM on v_mfma_f32_32x32x2f32
// (fp32 operands, fp32 accumulation): M = 32 output channels, N = 32 convolution outputs per matrix instruction, a wave owns 64 of the 255 (two columns-of-32, one
// after the other).  K runs over (plane, dx, row pair): the two k of a pair are the rows dy = 2 j and 2 j + 1 of one column, so that the B operand of lane l is
// ONE LDS read at (a per-lane base that carries the row parity l >> 5) + (a compile-time offset) — no vector arithmetic beside the matrix instructions.  dy = 7 is the
// padding of K (147 -> 168): its weights are zero, its LDS row exists and holds zeros.  The A operand — 84 k-pairs of this half's weights, packed in operand order by
// nets/ops.py::pack_stem7x7 — lives in registers for the whole kernel.
// bias + ReLU are applied in the accumulators; the values go to LDS as [channel][15 x 17], convolution outputs OUTSIDE the map as -inf: the pool ignores them (torch pads
// the pool with -inf; it is not a zero padding of pre-activation values).  Then a thread takes the maximum of a 3 x 3 window and stores one pooled value.
#include "common.hpp"
#include <math.h>

namespace {
typedef float f32x16t __attribute__((ext_vector_type(16)));
constexpr int TPH = 7, TPW = 8;                                  // pooled tile
constexpr int CTH = 2 * TPH + 1, CTW = 2 * TPW + 1, NPOS = CTH * CTW;      // convolution outputs under it: 15 x 17 = 255 (8 matrix columns-of-32, one slot idle)
constexpr int PH = 2 * (CTH - 1) + 7 + 1, PWU = 2 * (CTW - 1) + 7, PW = 41, PLANE = PH * PW, NPATCH = 3 * PLANE;      // image window: 35 rows + the zero row of dy = 7, 39 columns (row stride 41: odd)
constexpr int NKP = 3 * 7 * 4;                                   // k-pairs: (plane, dx, row pair)
constexpr int CS = NPOS + 2;                                     // channel stride of the convolution tile in LDS

__global__ __launch_bounds__(256, 2) void k_stem7x7s2_pool(const float* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ bias, float* __restrict__ y,
                                                        int H, int W, int Hc, int Wc, int Hp, int Wp)
{
    __shared__ float patch[NPATCH];                                           // [3][PH][PW]
    __shared__ float cbuf[32 * CS];                                           // [32][NPOS (+ 2)]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, cb = blockIdx.z;
    const int px0 = blockIdx.x * TPW, py0 = blockIdx.y * TPH, iy0 = 4 * py0 - 5, ix0 = 4 * px0 - 5;      // pooled p <- conv 2 p - 1 .. 2 p + 1 <- image 2 c - 3 .. 2 c + 3
    const size_t HW = (size_t)H * W;

    float a[NKP];                                                             // this half's weights in operand order: in flight while the window is staged
#pragma unroll
    for (int kp = 0; kp < NKP; kp++) a[kp] = wp[(size_t)(cb * NKP + kp) * 64 + lane];

    constexpr int NL = (NPATCH + 255) / 256;
    float tv[NL];                                                             // unconditional loads (clamped address, then a select), all in flight together
#pragma unroll
    for (int j = 0; j < NL; j++) {
        const int i = min(tid + 256 * j, NPATCH - 1), c = i / PLANE, r = i - c * PLANE, yy = r / PW, xx = r - yy * PW, gy = iy0 + yy, gx = ix0 + xx;
        const bool in = yy < PH - 1 && xx < PWU && gy >= 0 && gy < H && gx >= 0 && gx < W;
        const float v = x[(size_t)c * HW + (size_t)min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1)];
        tv[j] = in ? v : 0.f;
    }
#pragma unroll
    for (int j = 0; j < NL; j++) if (tid + 256 * j < NPATCH) patch[tid + 256 * j] = tv[j];
    __syncthreads();

    // this wave's two columns-of-32 of convolution outputs, one after the other (slots past the 255th repeat the last one: computed, not kept).  K is summed in SIX
    // independent chains — (plane, upper / lower half of the rows) — that meet pairwise at the end: one chain of 84 steps carries 1.6x the rounding error (rms against
    // float64) of the library's convolution, six chains of 14 carry less than it; consecutive matrix instructions also never wait for each other's accumulator.
    const float ninf = -INFINITY;
#pragma unroll 1
    for (int g = 0; g < 2; g++) {
        const int q = (2 * wv + g) * 32 + (lane & 31), qc = min(q, NPOS - 1);
        const float* pq = patch + (2 * (qc / CTW) + (lane >> 5)) * PW + 2 * (qc % CTW);
        f32x16t acc[6];
#pragma unroll
        for (int n = 0; n < 6; n++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[n][r] = 0.f;
#pragma unroll
        for (int dx = 0; dx < 7; dx++)
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const int kp = (c * 7 + dx) * 4 + j, off = c * PLANE + 2 * j * PW + dx, n = 2 * c + (j >> 1);
                    acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kp], pq[off], acc[n], 0, 0, 0);
                }
        // bias + ReLU; register r of lane l is output channel 8 (r >> 2) + 4 (l >> 5) + (r & 3) at convolution output l & 31
        const int cy = 2 * py0 - 1 + q / CTW, cx = 2 * px0 - 1 + q % CTW;
        const bool inmap = cy >= 0 && cy < Hc && cx >= 0 && cx < Wc;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int co = 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
            const float v = ((acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r])) + (acc[4][r] + acc[5][r]) + bias[cb * 32 + co];
            if (q < NPOS) cbuf[co * CS + q] = inmap ? fmaxf(v, 0.f) : ninf;
        }
    }
    __syncthreads();

    constexpr int NO = 32 * TPH * TPW / 256;                                  // 7 pooled values per thread
    static_assert(NO * 256 == 32 * TPH * TPW, "pooled tile x 32 channels is a multiple of the workgroup");
#pragma unroll
    for (int j = 0; j < NO; j++) {
        const int i = tid + 256 * j, co = i / (TPH * TPW), r = i - co * (TPH * TPW), pyl = r / TPW, pxl = r - pyl * TPW, py = py0 + pyl, px = px0 + pxl;
        const float* s = cbuf + co * CS + 2 * pyl * CTW + 2 * pxl;
        float m = ninf;
#pragma unroll
        for (int dy = 0; dy < 3; dy++)
#pragma unroll
            for (int dx = 0; dx < 3; dx++) m = fmaxf(m, s[dy * CTW + dx]);
        if (py < Hp && px < Wp) y[((size_t)(cb * 32 + co) * Hp + py) * Wp + px] = m;
    }
}
}  // namespace

extern "C" {

/* y = max_pool2d(relu(conv2d(x, w, stride 2, padding 3) + bias), 3, 2, 1) for one image, 7x7 kernel, 3 -> 64 channels: x [3][h][w], bias [64], y [64][hp][wp] with
 * hc = (h - 1) / 2 + 1, hp = (hc - 1) / 2 + 1 (likewise w), f32 DEVICE tensors; w_packed [2][84][64]: the weight in operand order (vido_slam_amd/nets/ops.py::pack_stem7x7).
 * The detector's stem (resnet.py:375-395) in one launch; the convolution's output never reaches memory.  Enqueues on the adopted stream; capturable. */
int vido_stem7x7s2_pool(vido_ctx* ctx, const float* x, const float* w_packed, const float* bias, float* y, int h, int w)
{
    if (!ctx) return VIDO_E_INVALID;
    if (!x || !w_packed || !bias || !y || x == y || h < 1 || w < 1 || h > 16384 || w > 16384) return vido_set_error(ctx, VIDO_E_INVALID, "stem7x7s2_pool: bad arguments (%d x %d)", h, w);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->has_ext_stream ? ctx->ext_stream : ctx->stream;
    const int hc = (h - 1) / 2 + 1, wc = (w - 1) / 2 + 1, hp = (hc - 1) / 2 + 1, wp = (wc - 1) / 2 + 1;
    const dim3 grid((wp + TPW - 1) / TPW, (hp + TPH - 1) / TPH, 2), blk(256);
    hipLaunchKernelGGL(k_stem7x7s2_pool, grid, blk, 0, st, x, w_packed, bias, y, h, w, hc, wc, hp, wp);
    HIP_TRY(ctx, hipGetLastError());
    return VIDO_OK;
}

}  // extern "C"
