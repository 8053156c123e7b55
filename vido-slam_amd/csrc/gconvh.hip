// Grouped 3x3 stride-1 `same` convolution + bias + ReLU with 32 or 64 channels per group in split-fp16 arithmetic (gfx950), one launch.
//
// What it replaces: k_gconv3x3_m32d (csrc/gconv.hip, fp32 matrix instruction) on `conv2` of the ResNeXt bottlenecks of layer3 / layer4 (maskrcnn_benchmark/modeling/backbone/
// resnet.py:300-372, groups = 32 with 32 / 64 channels each) when the 1x1 convolution in front has applied its own bias + ReLU.  The arithmetic is that of csrc/conv3x3h.hip and
// k_conv1x1_b3<NP 2>: every fp32 operand is h + 2^-11 l' with h = rne16(x), l' = rne16(2^11 (x - h)); the three products w_h x_h (-> acc), w_h x_l' and w_l' x_h (-> acl) run on
// v_mfma_f32_32x32x16_f16 with fp32 accumulators, the result is (acc + 2^-11 acl) times the output channel's inverse weight scale (a power of two chosen at pack time), then
// bias and ReLU.  54 matrix instructions of 32 cycles per 32 positions x 32 input channels where the fp32 instruction needs 144 of 64.
//
// Formulation.  As in csrc/gconv.hip the rows are zero-padded to Wp = W + 2 columns and flattened: output position q = y Wp + x reads the padded input at q + dy Wp + dx, so a
// tile is 32 CONSECUTIVE flattened positions (the two pad positions per row are computed and dropped) and a tap is a constant offset.  A work item is (group, 32-channel output
// block, chunk of CL positions); its workgroup of four waves
//   * copies the item's weight planes — [16-channel step][tap][plane][64 lanes][8 fp16], 1 KB pieces in the A operand's order, 36 KB per 32 x 32 block — global -> LDS ONCE and
//     keeps them for all its positions;
//   * walks the chunk in rounds of 128 positions (one tile per wave).  A round's band — 128 + 2 Wp + 2 padded positions x all input channels of the group — is loaded into
//     registers by buffer loads whose per-lane offsets are out of range for padding, halo rows outside the image and positions past it (zeros, nothing is read outside x),
//     split ONCE into the two fp16 planes and stored as [8-channel group][position][8 fp16]: the B operand of a (tap, step, plane) is one 16-byte read, 32 consecutive slots
//     per half wave;
//   * requests the next round's band before the current round's matrix phase and converts it behind it: the loads fly beside the matrix instructions and the stores.
// The launch is cut into about (workgroups that fit a CU) x 256 items of equal length, so every CU carries the same share; a second resident workgroup multiplies while the
// first one loads.  Every output's sum runs over (tap, step, product) in that order whatever the chunking: same input, same bits.
#include "common.hpp"

namespace {
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

#define GH_OOB 0x40000000u
#define GH_CUS 256          // items are sized for this many CUs

struct GhArgs { const float* x; const void* wp; const float* bias; float* y; unsigned* range_flag; int H, W, gx, total, CL, BPX, BP, nunits; float slope; unsigned xbytes, wbytes, m_wp, m_bpx; };
// CL: positions per chunk (a multiple of 32); BPX = 130 + 2 Wp band positions of a round, BP >= BPX the plane pitch; nunits = BPX x channel groups; m_*: ceil(2^32 / d) for d = Wp, BPX

template <int CPG> struct GhForm {
    static constexpr int NCG = CPG / 8, NKS = CPG / 16, NCOB = CPG / 32;
    static constexpr int MAXU = CPG == 32 ? 5 : 7;                  // (position, channel group) units per thread and round
    static_assert(MAXU <= 7, "the kernel's unit arrays hold seven");
    static constexpr int MAXBP = MAXU * 256 / NCG;                  // band positions the units cover: 320 / 224
    static constexpr int WB = NKS * 18 * 1024;                      // weight bytes of a (group, output block): 36 / 72 KB
};

template <int CPG>
__global__ __launch_bounds__(256) void k_gconv3x3_h(GhArgs A)
{
    typedef GhForm<CPG> F;
    constexpr int NCG = F::NCG, NKS = F::NKS, NCOB = F::NCOB, MAXU = F::MAXU, WB = F::WB;
    extern __shared__ __attribute__((aligned(16))) char gh_lds[];
    char* const WL = gh_lds;                    // weights
    char* const PH = gh_lds + WB;               // plane h: [NCG][BP][16 bytes]; plane l' behind it
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = A.H, W = A.W, Wp = W + 2, npos = H * Wp, BPX = A.BPX, BP = A.BP;
    const unsigned HW = (unsigned)H * (unsigned)W, PLANE = (unsigned)(NCG * BP) * 16u;
    // an XCD walks a contiguous range of items, the chunks of a (group, output block) next to each other (see gc_item in csrc/gconv.hip)
    const int per = gridDim.x >> 3, item = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
    if (item >= A.total) return;
    const int gc = item / A.gx, chunk = item - gc * A.gx, g = gc / NCOB, cob = gc - g * NCOB;
    const int qc = chunk * A.CL, qn = min(A.CL, npos - qc), nrounds = (qn + 127) >> 7;      // (the host sizes gx so that every chunk starts inside the image)

    // ---- weights: 1 KB pieces, wave wv copies pieces wv, wv + 4, ...
    {
        const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)A.wp, 0, A.wbytes, 0x00020000);
#pragma unroll
        for (int i = 0; i < NKS * 18 / 4; i++) {
            const int piece = wv + 4 * i;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (__attribute__((address_space(3))) void*)(WL + piece * 1024), 16, 16u * (unsigned)lane, (unsigned)gc * (unsigned)WB + 1024u * (unsigned)piece, 0, 0);
        }
    }
    // ---- the band.  Unit u = tid + 256 j -> channel group u / BPX, band position u % BPX
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)A.x, 0, A.xbytes, 0x00020000);
    const unsigned xbase = 4u * (unsigned)(g * CPG) * HW;
    int ui[7]; unsigned ucg[7];              // (fixed bounds: an array of template-dependent size captured by a lambda makes the host pass drop the kernel's stub, see csrc/conv1x1.hip)
#pragma unroll
    for (int j = 0; j < MAXU; j++) { const unsigned u = (unsigned)(tid + 256 * j), cg = __umulhi(u, A.m_bpx); ucg[j] = u < (unsigned)A.nunits ? cg : 0xffffffffu; ui[j] = (int)(u - cg * (unsigned)BPX); }
    float pre[7][8];
    auto load_band = [&](int q0) {              // band position i of the round at q0 = padded flat position q0 + i = (row + 1) Wp + (column + 1)
#pragma unroll
        for (int j = 0; j < MAXU; j++) {
            const unsigned f = (unsigned)(q0 + ui[j]), yr = __umulhi(f, A.m_wp), xc = f - yr * (unsigned)Wp;
            const bool ok = ucg[j] != 0xffffffffu && yr >= 1u && yr <= (unsigned)H && xc >= 1u && xc <= (unsigned)W;
            const unsigned vo = ok ? 4u * (ucg[j] * 8u * HW + (yr - 1u) * (unsigned)W + (xc - 1u)) : GH_OOB;
#pragma unroll
            for (int e = 0; e < 8; e++) pre[j][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, vo, xbase + 4u * (unsigned)e * HW, 0));
        }
    };
    float xmax = 0.f;
    auto convert = [&]() {
#pragma unroll
        for (int j = 0; j < MAXU; j++) {
            f16x8 h8, l8;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const float v = pre[j][e];
                const _Float16 h = (_Float16)v;
                const float r = __builtin_fmaf((float)h, -2048.f, v * 2048.f);      // 2^11 (v - h): exact
                h8[e] = h; l8[e] = (_Float16)r;
                xmax = __builtin_elementwise_maximum(xmax, __builtin_fabsf(v));     // (the IEEE maximum: a NaN sticks)
            }
            if (ucg[j] != 0xffffffffu) {
                const unsigned o = (ucg[j] * (unsigned)BP + (unsigned)ui[j]) * 16u;
                *(f16x8*)(PH + o) = h8; *(f16x8*)(PH + PLANE + o) = l8;
            }
        }
    };

    // this lane's 16 output channels: bias and inverse weight scale
    const int co_base = g * CPG + cob * 32;
    const float* wsc = (const float*)((const char*)A.wp + A.wbytes);
    float bv[16], sv[16];
#pragma unroll
    for (int r = 0; r < 16; r++) { const int co = co_base + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3); bv[r] = A.bias[co]; sv[r] = wsc[co]; }

    load_band(qc);
    convert();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // the weight pieces
    typedef const __attribute__((address_space(3))) f16x8* lds_h8;
    for (int rd = 0; rd < nrounds; rd++) {
        __syncthreads();                                              // the round's planes (and the weights) are visible
        if (rd + 1 < nrounds) load_band(qc + 128 * (rd + 1));
        const int qt = qc + 128 * rd + 32 * wv;                       // this wave's tile
        if (128 * rd + 32 * wv < qn) {
            f32x16 acc, acl;
#pragma unroll
            for (int r = 0; r < 16; r++) { acc[r] = 0.f; acl[r] = 0.f; }
            const unsigned a_lane = 16u * (unsigned)lane;
            const unsigned b_lane = ((unsigned)(lane >> 5) * (unsigned)BP + (unsigned)(32 * wv + (lane & 31))) * 16u;
            // step s = (tap, 16-channel step); its four operands are requested two steps ahead (scheduling barriers: left alone, the scheduler sinks every read to just before
            // its matrix instruction and the loop runs at LDS latency, see csrc/gconv.hip)
            f16x8 ah[3], al[3], bh[3], bl[3];
            auto ld = [&](int s) {
                const int tap = s / NKS, ks = s - tap * NKS;
                const char* ap = WL + ((ks * 9 + tap) * 2) * 1024 + a_lane;
                const char* bp = PH + b_lane + (unsigned)((tap / 3) * Wp + tap % 3) * 16u + (unsigned)(2 * ks * BP) * 16u;
                ah[s % 3] = *(lds_h8)ap; al[s % 3] = *(lds_h8)(ap + 1024);
                bh[s % 3] = *(lds_h8)bp; bl[s % 3] = *(lds_h8)(bp + PLANE);
            };
            ld(0); ld(1);
#pragma unroll
            for (int s = 0; s < 9 * NKS; s++) {
                if (s + 2 < 9 * NKS) ld(s + 2);
                __builtin_amdgcn_sched_barrier(0);
                acl = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[s % 3], bl[s % 3], acl, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[s % 3], bh[s % 3], acc, 0, 0, 0);
                acl = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[s % 3], bh[s % 3], acl, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            // D[i][j]: lane = 32 ((i / 4) & 1) + j, register = 4 (i / 8) + (i & 3): a register holds one output channel of 32 consecutive positions per half wave
            const int q = qt + (lane & 31), yy = (int)__umulhi((unsigned)q, A.m_wp), xx = q - yy * Wp;
            if (q < npos && xx < W) {
                float* yo = A.y + (size_t)co_base * HW + (size_t)yy * W + xx;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int co = 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
                    const float v = (acc[r] + acl[r] * 0x1p-11f) * sv[r] + bv[r];
                    yo[(size_t)co * HW] = fmaxf(v, v * A.slope);
                }
            }
        }
        if (rd + 1 < nrounds) {
            __syncthreads();                                          // everybody is done with the round's planes
            convert();
        }
    }
    if (!(xmax < 65504.f) && A.range_flag) atomicOr(A.range_flag, 1u);      // (also a NaN)
}

// geometry of a call; gx == 0: not supported
struct GhPlan { int gx, CL, BPX, BP, nunits; size_t lds; };
static GhPlan gh_plan(int groups, int H, int W, int cpg_in, int cpg_out)
{
    GhPlan p{};
    if (H < 1 || W < 1 || cpg_in != cpg_out || (cpg_in != 32 && cpg_in != 64)) return p;
    const int ncg = cpg_in / 8, ncob = cpg_in / 32, maxbp = cpg_in == 32 ? GhForm<32>::MAXBP : GhForm<64>::MAXBP;
    const long long Wp = W + 2, npos = (long long)H * Wp, bpx = 130 + 2 * Wp;
    if (bpx > maxbp || (npos + 2 * bpx + 256) * Wp >= (1ll << 32)) return p;      // (the second: the kernel's reciprocal divisions are exact)
    p.BPX = (int)bpx; p.BP = (p.BPX + 15) & ~15; p.nunits = p.BPX * ncg;
    p.lds = (size_t)(cpg_in / 16) * 18 * 1024 + (size_t)2 * ncg * p.BP * 16;
    // items: as many as are resident at once on GH_CUS CUs, all of one length
    static const int force = [] { const char* e = getenv("VIDO_GCONV_H_ITEMS"); return e ? atoi(e) : 0; }();      // (measurement only: the number of items a launch is cut into)
    const int per_cu = std::max(1, (int)(160 * 1024 / p.lds)), target = force > 0 ? force : GH_CUS * std::min(per_cu, 2);
    const int ntile = (int)((npos + 31) / 32), gcs = std::max(groups, 1) * ncob;
    int gx = std::min(std::max((target + gcs / 2) / gcs, 1), ntile);
    p.CL = ((ntile + gx - 1) / gx) * 32;
    p.gx = (int)((npos + p.CL - 1) / p.CL);
    return p;
}
}  // namespace

extern "C" {

/* 1 when vido_gconv3x3_h_bias_act has a kernel for the shape: 32 -> 32 or 64 -> 64 channels per group and rows short enough for the band of a round to fit (W <= 93 / 45). */
int vido_gconv3x3_h_supported(int H, int W, int cpg_in, int cpg_out)
{
    return gh_plan(1, H, W, cpg_in, cpg_out).gx != 0;
}

/* y = leaky_relu(conv2d(x, w, stride 1, padding 1, groups) + bias, slope) for one image in the split-fp16 arithmetic of vido_conv3x3_h_bias_act: x [groups * cpg_in][H][W],
 * y [groups * cpg_out][H][W] f32 DEVICE tensors (4-byte aligned, x != y), bias [groups * cpg_out]; w_packed (16-byte aligned): two fp16 planes of the output channels scaled
 * by powers of two, plane p of element (co, ci, dy, dx) of group g at [g][(co % cpg) / 32][ci / 16][3 dy + dx][p][32 ((ci % 16) / 8) + co % 32][ci % 8], then
 * [groups * cpg_out] floats: the inverse scales (vido_slam_amd/nets/ops.py::pack_gconv3x3_h).  slope: 0 = ReLU, 1 = none.  Activations must be finite and below 65504 in
 * magnitude (vido_conv1x1_range_flag otherwise).  Enqueues on the adopted stream; capturable. */
int vido_gconv3x3_h_bias_act(vido_ctx* ctx, const float* x, const void* w_packed, const float* bias, float* y, int groups, int cpg_in, int cpg_out, int H, int W, float slope)
{
    if (!ctx) return VIDO_E_INVALID;
    if (!x || !w_packed || !bias || !y || (const void*)x == (const void*)y || groups < 1 || groups > 65535 || !(slope >= 0.f && slope <= 1.f) || (((uintptr_t)x | (uintptr_t)y) & 3) || ((uintptr_t)w_packed & 15))
        return vido_set_error(ctx, VIDO_E_INVALID, "gconv3x3_h: bad arguments");
    const GhPlan p = gh_plan(groups, H, W, cpg_in, cpg_out);
    const long long xb = 4ll * groups * cpg_in * H * W, wb = 36ll * groups * cpg_out * cpg_in;
    if (!p.gx || xb >= (1ll << 30) || wb >= (1ll << 31)) return vido_set_error(ctx, VIDO_E_INVALID, "gconv3x3_h: no kernel for %d -> %d channels per group at %d x %d", cpg_in, cpg_out, H, W);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    static bool attr[64] = {};
    if (!attr[ctx->device & 63]) {
        HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_gconv3x3_h<32>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_gconv3x3_h<64>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr[ctx->device & 63] = true;
    }
    hipStream_t st = ctx->has_ext_stream ? ctx->ext_stream : ctx->stream;
    auto magic = [](unsigned d) { return (unsigned)((0x100000000ull + d - 1) / d); };      // d >= 2
    const int total = p.gx * groups * (cpg_out / 32);
    GhArgs A{x, w_packed, bias, y, ctx->c1_range_flag, H, W, p.gx, total, p.CL, p.BPX, p.BP, p.nunits, slope, (unsigned)xb, (unsigned)wb, magic((unsigned)(W + 2)), magic((unsigned)p.BPX)};
    const dim3 grid(8 * ((total + 7) / 8)), blk(256);
    if (cpg_in == 32) hipLaunchKernelGGL(k_gconv3x3_h<32>, grid, blk, p.lds, st, A); else hipLaunchKernelGGL(k_gconv3x3_h<64>, grid, blk, p.lds, st, A);
    HIP_TRY(ctx, hipGetLastError());
    return VIDO_OK;
}

}  // extern "C"
