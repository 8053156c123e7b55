// Grouped 3x3 stride-1 `same` convolution + bias + ReLU with 8 or 16 channels per group in split-fp16 arithmetic (gfx950), one launch.
//
// What it replaces: k_gconv3x3_m16d (csrc/gconv.hip, fp32 matrix instruction) on `conv2` of the ResNeXt bottlenecks of layer1 / layer2 (maskrcnn_benchmark/modeling/backbone/
// resnet.py:300-372, groups = 32 with 8 / 16 channels each) when the 1x1 convolution in front has applied its own bias + ReLU.  The arithmetic is that of csrc/gconvh.hip and
// k_conv1x1_b3<NP 2>: every fp32 operand is h + 2^-11 l' with h = rne16(x), l' = rne16(2^11 (x - h)); the three products w_h x_h (-> acc), w_h x_l' and w_l' x_h (-> acl) run on
// v_mfma_f32_16x16x32_f16 with fp32 accumulators, the result is (acc + 2^-11 acl) times the output channel's inverse weight scale (a power of two chosen at pack time), then
// bias and ReLU.
//
// Formulation.  As in csrc/gconvh.hip the rows are zero-padded to Wp = W + 2 columns and flattened: output position q = y Wp + x reads the padded input at q + dy Wp + dx, a
// tile is 16 CONSECUTIVE flattened positions (the two pad positions per row are computed and dropped) and a tap is a constant offset.  The K = 32 of an instruction is four
// blocks of 8 (lanes 16 b .. 16 b + 15 hold block b of both operands), and a block is the 8 input channels of one (tap, channel group) SLOT:
//   8 per group:  instruction i, block b = tap 4 i + b                                   -> 3 instructions per product, three zero slots (taps 9 .. 11);
//   16 per group: instruction i, block b = tap 2 i + (b >> 1) of channel group b & 1     -> 5 instructions per product, one zero tap (two blocks).
// The A operand (weights: rows = the group's output channels, rows 8 .. 15 zero at 8 per group) of every (instruction, plane) is 16 bytes per lane and stays in REGISTERS for the
// whole work item; a zero slot has zero weights and reads the position of tap 0 (an address inside the band, finite data).  The B operand of a slot is ONE 16-byte LDS read per
// lane from planes stored [channel group][position][8 fp16], as in csrc/gconvh.hip.
//
// Work items and the ring.  An item is (group, chunk of CL flattened positions); its workgroup of four waves walks the chunk in rounds of RL positions (tiles dealt round-robin
// to the waves).  The planes live in a RING of RING = 2^k >= RL + 2 Wp + 2 positions addressed by (padded position) & (RING - 1): the first round fills its whole band, every
// later round loads ONLY its RL new positions — requested before the current round's matrix phase, split and stored behind it, into the slots of the positions the finished
// round no longer needs.  So every input element is loaded and split once per item, plus the 2 Wp + 2 halo positions at its start.  Loads are buffer loads whose per-lane offsets
// are out of range for padding, halo rows outside the image and positions past the item (zeros; nothing is read outside x).  Items are of equal length, cut so that all of them
// are resident at once where the halo allows (CL >= max(512, 3 halo): an item never re-reads more than a third of what it computes).
// Every output's sum runs over (instruction, product) in that order whatever the chunking: same input, same bits.
#include "common.hpp"

namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

#define GHS_OOB 0x40000000u
#define GHS_CUS 256          // items are sized for this many CUs
#define GHS_MAXU 4           // (position, channel group) units per thread and load step
#define GHS_MAXI 5           // matrix instructions per product at the most

struct GhsArgs { const float* x; const void* wp; const float* bias; float* y; unsigned* range_flag; int H, W, gx, total, CL, RL, RING; float slope; unsigned xbytes, wbytes, m_wp; };
// CL: positions per chunk (a multiple of 16); RL: positions per round (a multiple of 64); RING: ring positions (a power of two >= RL + 2 Wp + 2); m_wp: ceil(2^32 / Wp)

template <int CPG> struct GhsForm {
    static constexpr int NCG = CPG / 8, NI = CPG == 8 ? 3 : 5;
    static constexpr int STEP = 256 * GHS_MAXU / NCG;               // positions of a load step: 1024 / 512
    static constexpr int WB = NI * 2048;                            // weight bytes of a group: [instruction][plane][64 lanes][8 fp16]
};

template <int CPG>
__global__ __launch_bounds__(256) void k_gconv3x3_hs(GhsArgs A)
{
    typedef GhsForm<CPG> F;
    constexpr int NCG = F::NCG, NI = F::NI, STEP = F::STEP;
    extern __shared__ __attribute__((aligned(16))) char ghs_lds[];
    char* const PH = ghs_lds;                   // plane h: [NCG][RING][16 bytes]; plane l' behind it
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = A.H, W = A.W, Wp = W + 2, npos = H * Wp, halo = 2 * Wp + 2, RL = A.RL, RING = A.RING;
    const unsigned HW = (unsigned)H * (unsigned)W, RM = (unsigned)RING - 1u, PLANE = (unsigned)(NCG * RING) * 16u;
    // an XCD walks a contiguous range of items, the chunks of a group next to each other (see gc_item in csrc/gconv.hip)
    const int per = gridDim.x >> 3, item = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
    if (item >= A.total) return;
    const int g = item / A.gx, chunk = item - g * A.gx;
    const int qc = chunk * A.CL, qn = min(A.CL, npos - qc), nrounds = (qn + RL - 1) / RL;      // (the host sizes gx so that every chunk starts inside the image)
    const int pend = qc + qn + halo;            // the first padded position the item does not read

    // ---- weights: this lane's A operands, kept for the whole item
    f16x8 ah[GHS_MAXI], al[GHS_MAXI];
    {
        const f16x8* wg = (const f16x8*)((const char*)A.wp + (size_t)g * F::WB) + lane;
#pragma unroll
        for (int i = 0; i < NI; i++) { ah[i] = wg[(2 * i) * 64]; al[i] = wg[(2 * i + 1) * 64]; }
    }
    // this lane's slot of instruction i: offset of its tap in positions, byte offset of its channel group's plane
    const int kb = lane >> 4;
    unsigned toff[GHS_MAXI];
#pragma unroll
    for (int i = 0; i < NI; i++) { const int tap = CPG == 8 ? 4 * i + kb : 2 * i + (kb >> 1); toff[i] = tap < 9 ? (unsigned)((tap / 3) * Wp + tap % 3) : 0u; }
    const unsigned cgo = CPG == 8 ? 0u : (unsigned)(kb & 1) * (unsigned)RING * 16u;

    // ---- loads.  Unit u = tid + 256 j of a step at p0 -> position p0 + upos[j] of channel group ucg[j] (16 per group: the halves of a wave take the two channel groups)
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)A.x, 0, A.xbytes, 0x00020000);
    const unsigned xbase = 4u * (unsigned)(g * CPG) * HW;
    int upos[GHS_MAXU]; unsigned ucg[GHS_MAXU];
#pragma unroll
    for (int j = 0; j < GHS_MAXU; j++) { const int u = tid + 256 * j; upos[j] = NCG == 1 ? u : (((u >> 6) << 5) | (u & 31)); ucg[j] = NCG == 1 ? 0u : (unsigned)((u >> 5) & 1); }
    float pre[GHS_MAXU][8];
    auto load = [&](int p0, int n) {            // padded flat positions [p0, p0 + n), n <= STEP; position f = (row + 1) Wp + (column + 1)
#pragma unroll
        for (int j = 0; j < GHS_MAXU; j++) {
            const unsigned f = (unsigned)(p0 + upos[j]), yr = __umulhi(f, A.m_wp), xc = f - yr * (unsigned)Wp;
            const bool ok = upos[j] < n && (int)f < pend && yr >= 1u && yr <= (unsigned)H && xc >= 1u && xc <= (unsigned)W;
            const unsigned vo = ok ? 4u * (ucg[j] * 8u * HW + (yr - 1u) * (unsigned)W + (xc - 1u)) : GHS_OOB;
#pragma unroll
            for (int e = 0; e < 8; e++) pre[j][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, vo, xbase + 4u * (unsigned)e * HW, 0));
        }
    };
    float xmax = 0.f;
    auto convert = [&](int p0, int n) {         // split what load(p0, n) fetched and store it into the ring
#pragma unroll
        for (int j = 0; j < GHS_MAXU; j++) {
            f16x8 h8, l8;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const float v = pre[j][e];
                const _Float16 h = (_Float16)v;
                const float r = __builtin_fmaf((float)h, -2048.f, v * 2048.f);      // 2^11 (v - h): exact
                h8[e] = h; l8[e] = (_Float16)r;
                xmax = __builtin_elementwise_maximum(xmax, __builtin_fabsf(v));     // (the IEEE maximum: a NaN sticks)
            }
            if (upos[j] < n) {
                const unsigned o = (ucg[j] * (unsigned)RING + ((unsigned)(p0 + upos[j]) & RM)) * 16u;
                *(f16x8*)(PH + o) = h8; *(f16x8*)(PH + PLANE + o) = l8;
            }
        }
    };

    // this lane's 4 output channels: bias and inverse weight scale (8 per group: lanes 32 .. 63 hold the zero rows and store nothing)
    const bool rows = 4 * kb < CPG;
    const int co_base = g * CPG + (rows ? 4 * kb : 0);
    const float* wsc = (const float*)((const char*)A.wp + A.wbytes);
    float bv[4], sv[4];
#pragma unroll
    for (int r = 0; r < 4; r++) { bv[r] = A.bias[co_base + r]; sv[r] = wsc[co_base + r]; }

    // ---- the first round's band: RL + halo positions (<= RING)
    {
        const int n0 = min(RL + halo, pend - qc);
        for (int s = 0; s < n0; s += STEP) { const int n = min(STEP, n0 - s); load(qc + s, n); convert(qc + s, n); }
    }
    typedef const __attribute__((address_space(3))) f16x8* lds_h8;
    for (int rd = 0; rd < nrounds; rd++) {
        __syncthreads();                                              // the round's planes are visible
        const int q0 = qc + rd * RL, pn = q0 + RL + halo, nn = min(RL, pend - pn);      // the next round's new positions [pn, pn + nn)
        if (rd + 1 < nrounds) load(pn, nn);
        const int ntr = (min(RL, qn - rd * RL) + 15) >> 4;            // tiles of this round
        for (int t = wv; t < ntr; t += 4) {
            const int qt = q0 + 16 * t;
            const unsigned base = (unsigned)(qt + (lane & 15));
            f16x8 bh[GHS_MAXI], bl[GHS_MAXI];
#pragma unroll
            for (int i = 0; i < NI; i++) {
                const char* bp = PH + cgo + ((base + toff[i]) & RM) * 16u;
                bh[i] = *(lds_h8)bp; bl[i] = *(lds_h8)(bp + PLANE);
            }
            f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acl = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < NI; i++) {
                acl = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bl[i], acl, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bh[i], acc, 0, 0, 0);
                acl = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bh[i], acl, 0, 0, 0);
            }
            // D[i][j]: lane = 16 (i / 4) + j, register = i & 3: a register holds one output channel of 16 consecutive positions per quarter wave
            const int q = qt + (lane & 15), yy = (int)__umulhi((unsigned)q, A.m_wp), xx = q - yy * Wp;
            if (rows && q < qc + qn && xx < W) {
                float* yo = A.y + (size_t)co_base * HW + (size_t)yy * W + xx;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float v = (acc[r] + acl[r] * 0x1p-11f) * sv[r] + bv[r];
                    yo[(size_t)r * HW] = fmaxf(v, v * A.slope);
                }
            }
        }
        if (rd + 1 < nrounds) {
            __syncthreads();                                          // everybody is done with the positions the new ones replace
            convert(pn, nn);
        }
    }
    if (!(xmax < 65504.f) && A.range_flag) atomicOr(A.range_flag, 1u);      // (also a NaN)
}

// geometry of a call; gx == 0: not supported
struct GhsPlan { int gx, CL, RL, RING; size_t lds; };
static GhsPlan ghs_plan(int groups, int H, int W, int cpg_in, int cpg_out)
{
    GhsPlan p{};
    if (H < 1 || W < 1 || cpg_in != cpg_out || (cpg_in != 8 && cpg_in != 16)) return p;
    const int ncg = cpg_in / 8, step = cpg_in == 8 ? GhsForm<8>::STEP : GhsForm<16>::STEP;
    const long long Wp = W + 2, npos = (long long)H * Wp, halo = 2 * Wp + 2;
    long long ring = 256;
    while (ring < halo + 128) ring *= 2;
    if (ring * 32 * ncg > 64 * 1024) return p;                                    // two workgroups per CU at the least: W <= 957 / 445
    if ((npos + halo + 2048) * Wp >= (1ll << 32)) return p;                       // (the kernel's reciprocal divisions are exact)
    p.RING = (int)ring; p.RL = std::min((int)((ring - halo) & ~63ll), step); p.lds = (size_t)ring * 32 * ncg;
    // items: as many as are resident at once on GHS_CUS CUs, all of one length, none shorter than max(512, 3 halo) positions
    static const int force = [] { const char* e = getenv("VIDO_GCONV_HS_ITEMS"); return e ? atoi(e) : 0; }();      // (measurement only: the number of items a launch is cut into)
    const int per_cu = std::min(std::max(1, (int)(160 * 1024 / p.lds)), 4), target = force > 0 ? force : GHS_CUS * per_cu;
    const long long ntile = (npos + 15) / 16, minlen = std::max(512ll, 3 * halo);
    const int G = std::max(groups, 1);
    long long gx = std::min<long long>(std::max((target + G / 2) / G, 1), ntile);
    if (force <= 0) gx = std::min(gx, std::max(1ll, npos / minlen));
    p.CL = (int)((ntile + gx - 1) / gx) * 16;
    p.gx = (int)((npos + p.CL - 1) / p.CL);
    return p;
}
// input elements per channel that the items of a plan load: the image positions among the padded positions [chunk CL, chunk CL + qn + halo) of every chunk
static long long ghs_loaded(const GhsPlan& p, int H, int W)
{
    const long long Wp = W + 2, npos = (long long)H * Wp, halo = 2 * Wp + 2;
    auto below = [&](long long f) {             // image positions among the padded positions [0, f)
        const long long yr = f / Wp, xc = f % Wp;
        return std::min(std::max(yr - 1, 0ll), (long long)H) * W + (yr >= 1 && yr <= H ? std::min(std::max(xc - 1, 0ll), (long long)W) : 0ll);
    };
    long long n = 0;
    for (int c = 0; c < p.gx; c++) { const long long qc = (long long)c * p.CL, qn = std::min<long long>(p.CL, npos - qc); n += below(qc + qn + halo) - below(qc); }
    return n;
}
}  // namespace

extern "C" {

/* 1 when vido_gconv3x3_hs_bias_act has a kernel for the shape: 8 -> 8 or 16 -> 16 channels per group and rows short enough for the ring of a round to fit (W <= 957 / 445). */
int vido_gconv3x3_hs_supported(int H, int W, int cpg_in, int cpg_out)
{
    return ghs_plan(1, H, W, cpg_in, cpg_out).gx != 0;
}

/* test hook (tests/test_gconv_hs_cpu.py walks the ring addressing on the CPU): the geometry of a call as out[0..6] = gx (chunks per group), CL (positions per chunk), RL (positions
 * per round), RING (ring positions), Wp (flattened row pitch), positions per load step, matrix instructions per product; *loaded = input elements PER CHANNEL the launch loads;
 * 0 = no kernel */
int vido_debug_ghs_plan(int groups, int H, int W, int cpg_in, int cpg_out, int* out, long long* loaded)
{
    const GhsPlan p = ghs_plan(groups, H, W, cpg_in, cpg_out);
    if (!p.gx || !out) return 0;
    out[0] = p.gx; out[1] = p.CL; out[2] = p.RL; out[3] = p.RING; out[4] = W + 2; out[5] = cpg_in == 8 ? GhsForm<8>::STEP : GhsForm<16>::STEP; out[6] = cpg_in == 8 ? GhsForm<8>::NI : GhsForm<16>::NI;
    if (loaded) *loaded = ghs_loaded(p, H, W);
    return 1;
}

/* y = leaky_relu(conv2d(x, w, stride 1, padding 1, groups) + bias, slope) for one image in the split-fp16 arithmetic of vido_gconv3x3_h_bias_act with 8 -> 8 or 16 -> 16 channels
 * per group: x [groups * cpg_in][H][W], y [groups * cpg_out][H][W] f32 DEVICE tensors (4-byte aligned, x != y, any W), bias [groups * cpg_out]; w_packed (16-byte aligned): two
 * fp16 planes of the output channels scaled by powers of two in the A operand order of v_mfma_f32_16x16x32_f16, [g][instruction i][plane][16 b + co % cpg][ci % 8] with block b of
 * instruction i = tap 4 i + b (8 per group; rows 8 .. 15 zero) or tap 2 i + (b >> 1) of input channels 8 (b & 1) .. + 7 (16 per group), taps >= 9 zero; then [groups * cpg_out]
 * floats: the inverse scales (vido_slam_amd/nets/ops.py::pack_gconv3x3_hs).  slope: 0 = ReLU, 1 = none.  Activations must be finite and below 65504 in magnitude
 * (vido_conv1x1_range_flag otherwise).  Enqueues on the adopted stream; capturable. */
int vido_gconv3x3_hs_bias_act(vido_ctx* ctx, const float* x, const void* w_packed, const float* bias, float* y, int groups, int cpg_in, int cpg_out, int H, int W, float slope)
{
    if (!ctx) return VIDO_E_INVALID;
    if (!x || !w_packed || !bias || !y || (const void*)x == (const void*)y || groups < 1 || groups > 65535 || !(slope >= 0.f && slope <= 1.f) || (((uintptr_t)x | (uintptr_t)y) & 3) || ((uintptr_t)w_packed & 15))
        return vido_set_error(ctx, VIDO_E_INVALID, "gconv3x3_hs: bad arguments");
    const GhsPlan p = ghs_plan(groups, H, W, cpg_in, cpg_out);
    const long long xb = 4ll * groups * cpg_in * H * W, wb = (long long)groups * (cpg_in == 8 ? GhsForm<8>::WB : GhsForm<16>::WB), total = (long long)p.gx * groups;
    if (!p.gx || xb >= (1ll << 30) || wb >= (1ll << 31) || total >= (1ll << 24)) return vido_set_error(ctx, VIDO_E_INVALID, "gconv3x3_hs: no kernel for %d -> %d channels per group at %d x %d", cpg_in, cpg_out, H, W);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    static bool attr[64] = {};
    if (!attr[ctx->device & 63]) {
        HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_gconv3x3_hs<8>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
        HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_gconv3x3_hs<16>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
        attr[ctx->device & 63] = true;
    }
    hipStream_t st = ctx->has_ext_stream ? ctx->ext_stream : ctx->stream;
    GhsArgs A{x, w_packed, bias, y, ctx->c1_range_flag, H, W, p.gx, (int)total, p.CL, p.RL, p.RING, slope, (unsigned)xb, (unsigned)wb, (unsigned)((0x100000000ull + (unsigned)(W + 2) - 1) / (unsigned)(W + 2))};
    const dim3 grid(8 * (((int)total + 7) / 8)), blk(256);
    if (cpg_in == 8) hipLaunchKernelGGL(k_gconv3x3_hs<8>, grid, blk, p.lds, st, A); else hipLaunchKernelGGL(k_gconv3x3_hs<16>, grid, blk, p.lds, st, A);
    HIP_TRY(ctx, hipGetLastError());
    return VIDO_OK;
}

}  // extern "C"
