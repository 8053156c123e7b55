// maskassoc.hip — instance ids that persist across frames: overlap association of the previous label image (already warped into this frame by maskprop.hip) with the
// detector's new instance image, on gfx950 (no reference counterpart: the reference's labels are class indices; Tracking::UpdateMask repaints ONE lost label and is untouched).
// Rule (include/vido_c.h; the numpy statement is tests/refimpl/mask_associate_np.py): count the pixels of every (previous id p, detector slot c) pair; c takes
// over the id p whose IoU with it is strictly above 1/2 (such a p is unique and no two c share one: both follow from "more than half", so there is no order and no tie
// rule); every other detected instance gets the next free id after a cursor that only moves forward over 1..254; an id of the previous image that nothing matched is held
// in place for `hold` calls and then retired.
// A memset and three launches on one stream: k_assoc_overlap (the 256 x 256 count table, one atomic per run of equal pairs a wave sees), k_assoc_assign (ONE workgroup:
// sums, match test, the serial cursor walk, state and counters) and k_assoc_relabel (every output pixel through two 256-entry lookups in LDS).  The table is cleared by the
// memset in FRONT of the first launch, never by a kernel afterwards: a call then does not depend on how the previous one ended (as for the key plane).
// Integer sums only: the result depends on no execution order.
#include "common.hpp"

struct MaskAssocState {
    unsigned* d_table = nullptr;                                  // [256][256] pair counts C[p][c]; rows: previous id p (0..254), columns: detector slot + 1 (0..127)
    int32_t* d_lut = nullptr;                                     // [256] LUT (by c), [256] KEEP (by p), [4] the counters of a call without a caller's stats buffer
};

#define MA_TW 32
#define MA_TH 8
#define MA_TILES 4                                                // 32 x 8 tiles a workgroup walks downwards: a wave carries its run of equal pairs from tile to tile
#define MA_IDS 254
#define MA_SLOTS 127

// One thread per pixel of a 32 x 8 tile (k_maskprop_resolve's shape), MA_TILES tiles per workgroup.  Most waves see one or two distinct (p, c) pairs: a wave picks the pair of
// its first lane left, ballots on it, and adds the popcount to a pending (pair, count) it keeps in uniform registers; the pending pair goes to memory — one atomic add by
// one lane — only when another pair takes its place or the workgroup ends.  A tile of pure background (pair (0, 0), also outside the image) adds nothing, so a workgroup
// over background alone touches no memory beyond its loads (k_paste_instance's block culling, here without a list to cull).
__global__ __launch_bounds__(256) void k_assoc_overlap(const int32_t* __restrict__ prev /* may be null */, const int32_t* __restrict__ cur, int H, int W,
                                                       const int64_t* __restrict__ classes /* may be null */, int n, unsigned* __restrict__ table)
{
    __shared__ unsigned char live[128];
    const int t = threadIdx.x;
    if (t < 128) live[t] = (t >= 1 && t <= n && (!classes || classes[t - 1] != 0)) ? 1 : 0;
    __syncthreads();
    const int x = blockIdx.x * MA_TW + (t & (MA_TW - 1));
    unsigned key[MA_TILES];
#pragma unroll
    for (int k = 0; k < MA_TILES; k++) {
        const int y = (blockIdx.y * MA_TILES + k) * MA_TH + t / MA_TW;
        key[k] = 0;
        if (x < W && y < H) {
            const size_t i = (size_t)y * W + x;
            const int cv = cur[i], pv = prev ? prev[i] : 0;
            const unsigned c = (cv >= 1 && cv <= n && live[cv]) ? (unsigned)cv : 0u;       // (cv <= n <= 127: inside live[])
            const unsigned p = (pv >= 1 && pv <= MA_IDS) ? (unsigned)pv : 0u;
            key[k] = p << 8 | c;
        }
    }
    unsigned pend_key = 0, pend_n = 0;                              // wave-uniform
#pragma unroll
    for (int k = 0; k < MA_TILES; k++) {
        bool todo = key[k] != 0;
        unsigned long long m = __ballot(todo);
        while (m) {                                                 // (m is the same in every lane: the whole wave walks the loop together)
            const int leader = __ffsll((long long)m) - 1;
            const unsigned lk = __shfl(key[k], leader);
            const bool same = todo && key[k] == lk;
            const unsigned long long b = __ballot(same);
            const unsigned cnt = (unsigned)__popcll(b);
            if (lk == pend_key) pend_n += cnt;
            else {
                if (pend_n && (t & 63) == 0) atomicAdd(table + pend_key, pend_n);
                pend_key = lk; pend_n = cnt;
            }
            todo = todo && !same;
            m &= ~b;
        }
    }
    if (pend_n && (t & 63) == 0) atomicAdd(table + pend_key, pend_n);
}

// Steps 2 to 5, one workgroup of 256.  Thread t sums row t (Ap) with 16-byte loads; thread c < 128 then walks column c (coalesced over the threads) for Ac and the column's
// strict maximum over p >= 1 — the only p that can match c, because a match holds more than half of c's pixels — and tests it.  One lane hands out the fresh ids; a thread
// per id updates the state.  stats: matched, fresh, lost, left out.
__global__ __launch_bounds__(256) void k_assoc_assign(const unsigned* __restrict__ table, const int64_t* __restrict__ classes /* may be null */, int n, int hold,
                                                      int32_t* __restrict__ state, int32_t* __restrict__ lut_g, int32_t* __restrict__ keep_g,
                                                      int32_t* __restrict__ lut_out /* may be null */, int32_t* __restrict__ stats)
{
    __shared__ unsigned Ap[256], Ac[128];
    __shared__ int lut[256], owner[256], cnt[4];
    const int t = threadIdx.x;
    {
        const uint4* row = (const uint4*)(table + t * 256);
        const int nv = (n + 4) / 4;                                 // columns 0 .. n, rounded up to whole vectors (n = 127: 32); the columns past n hold zeros
        unsigned s = 0;
#pragma unroll 8
        for (int j = 0; j < nv; j++) { const uint4 v = row[j]; s += v.x + v.y + v.z + v.w; }
        Ap[t] = (t >= 1 && t <= MA_IDS) ? s : 0u;
        lut[t] = 0; owner[t] = 0;
        if (t < 4) cnt[t] = 0;
    }
    __syncthreads();
    if (t < 128) {
        unsigned ac = 0, best = 0; int bp = 0;
        if (t >= 1 && t <= n) {
#pragma unroll 8
            for (int p = 0; p <= MA_IDS; p++) {
                const unsigned v = table[p * 256 + t];
                ac += v;
                if (p >= 1 && v > best) { best = v; bp = p; }
            }
        }
        Ac[t] = ac;
        if (ac > 0 && bp > 0 && 3u * best > Ap[bp] + ac) { lut[t] = bp; owner[bp] = t; atomicAdd(&cnt[0], 1); }      // counts <= 4095^2 < 2^24
    }
    __syncthreads();
    if (t == 0) {
        int cursor = state[0];
        if (cursor < 0 || cursor > MA_IDS) cursor = 0;
        // the scan position moves once around the ring at most: an id it has passed is either taken in this call or present in the previous image, so the ids ahead of it
        // are exactly those "not handed out earlier in this call"; when the round is used up no id is free for anybody
        int pos = cursor, budget = MA_IDS, fresh = 0, left = 0;
        for (int c = 1; c <= n; c++) {
            if (Ac[c] == 0 || lut[c] != 0) continue;
            int got = 0;
            while (budget > 0) {
                pos = pos >= MA_IDS ? 1 : pos + 1; budget--;
                if (Ap[pos] == 0) { got = pos; break; }
            }
            if (got) { lut[c] = got; owner[got] = c; cursor = got; fresh++; }
            else left++;
        }
        state[0] = cursor; cnt[1] = fresh; cnt[3] = left;
    }
    __syncthreads();
    int keep = 0;
    if (t >= 1 && t <= MA_IDS) {
        const int c = owner[t];
        if (c) { state[256 + t] = classes ? (int32_t)classes[c - 1] : 1; state[512 + t] = 0; }
        else {
            bool held = false;
            if (Ap[t] > 0) {
                atomicAdd(&cnt[2], 1);
                const long long l = (long long)state[512 + t] + 1;
                if (l <= (long long)hold) { state[512 + t] = (int32_t)l; keep = t; held = true; }
            }
            if (!held) { state[256 + t] = 0; state[512 + t] = 0; }
        }
    }
    keep_g[t] = keep; lut_g[t] = lut[t];
    if (lut_out) lut_out[t] = lut[t];
    __syncthreads();
    if (t < 4) stats[t] = cnt[t];
}

// out = LUT[c] where that is nonzero, else KEEP[p]; EVERY pixel is written.  LUT is zero for a slot that is not live, so the cleaning of step 0 is the lookup itself.
// [0, npx): `head` scalars, n4 vectors of four from there, `tail` scalars behind them (k_depth_prescale's split; the host picks head so that the three images are on a
// 16-byte boundary there, or makes everything head).  out may be cur itself: a thread reads the elements it writes before it writes them.
__device__ __forceinline__ int32_t assoc_one(const int* lut, const int* keep, int cv, int pv)
{
    int r = (cv >= 1 && cv <= 255) ? lut[cv] : 0;
    if (r == 0 && pv >= 1 && pv <= MA_IDS) r = keep[pv];
    return r;
}
__global__ __launch_bounds__(256) void k_assoc_relabel(const int32_t* prev /* may be null */, const int32_t* cur, int32_t* out, int head, size_t n4, int tail,
                                                       const int32_t* __restrict__ lut_g, const int32_t* __restrict__ keep_g)
{
    __shared__ int lut[256], keep[256];
    lut[threadIdx.x] = lut_g[threadIdx.x]; keep[threadIdx.x] = keep_g[threadIdx.x];
    __syncthreads();
    const size_t t0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    const int4* c4 = (const int4*)(cur + head); const int4* p4 = prev ? (const int4*)(prev + head) : nullptr; int4* o4 = (int4*)(out + head);
    for (size_t i = t0; i < n4; i += stride) {
        const int4 c = c4[i]; const int4 p = p4 ? p4[i] : make_int4(0, 0, 0, 0);
        int4 r;
        r.x = assoc_one(lut, keep, c.x, p.x); r.y = assoc_one(lut, keep, c.y, p.y); r.z = assoc_one(lut, keep, c.z, p.z); r.w = assoc_one(lut, keep, c.w, p.w);
        o4[i] = r;
    }
    for (size_t j = t0; j < (size_t)head + (size_t)tail; j += stride) {
        const size_t e = j < (size_t)head ? j : (size_t)head + 4 * n4 + (j - (size_t)head);
        out[e] = assoc_one(lut, keep, cur[e], prev ? prev[e] : 0);
    }
}

// ---- host ------------------------------------------------------------------------------------------
static int maskassoc_state(vido_ctx* ctx, MaskAssocState** out)
{
    if (ctx->massoc) { *out = ctx->massoc; return VIDO_OK; }
    // the state is published only when BOTH buffers exist: after a failed first call the next one allocates again instead of launching through a null pointer
    unsigned* table = nullptr; int32_t* lut = nullptr;
    HIP_TRY(ctx, hipMalloc((void**)&table, 256 * 256 * sizeof(unsigned)));
    const hipError_t e = hipMalloc((void**)&lut, (256 + 256 + 4) * sizeof(int32_t));
    if (e != hipSuccess) { hipFree(table); HIP_TRY(ctx, e); }
    MaskAssocState* S = new MaskAssocState();
    S->d_table = table; S->d_lut = lut;
    ctx->massoc = S;
    *out = S;
    return VIDO_OK;
}

void maskassoc_state_destroy(vido_ctx* ctx)
{
    MaskAssocState* S = ctx->massoc;
    if (!S) return;
    if (S->d_table) hipFree(S->d_table);
    if (S->d_lut) hipFree(S->d_lut);
    delete S; ctx->massoc = nullptr;
}

extern "C" {

int vido_mask_associate(vido_ctx* ctx, const int32_t* prev, const int32_t* cur, int H, int W, const int64_t* classes, int n, int hold, int32_t* state, int32_t* out,
                        int32_t* lut_out, int32_t* stats_out)
{
    if (!ctx) return VIDO_E_INVALID;
    if (!cur || !state || !out || out == prev) return vido_set_error(ctx, VIDO_E_INVALID, "mask_associate: null image or state, or out aliases prev");
    if (H < 1 || W < 1 || H > 4095 || W > 4095 || (size_t)H * W > (size_t)ctx->cfg.width * ctx->cfg.height)
        return vido_set_error(ctx, VIDO_E_INVALID, "mask_associate: %d x %d outside the context's %d x %d pixels", W, H, ctx->cfg.width, ctx->cfg.height);
    if (hold < 0 || n < 0) return vido_set_error(ctx, VIDO_E_INVALID, "mask_associate: hold = %d, n = %d: neither may be negative", hold, n);
    if (n > MA_SLOTS) return vido_set_error(ctx, VIDO_E_CAPACITY, "mask_associate: %d instances, the id space holds %d per frame", n, MA_SLOTS);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    MaskAssocState* S; int rc = maskassoc_state(ctx, &S); if (rc) return rc;
    hipStream_t st = ctx->has_ext_stream ? ctx->ext_stream : ctx->stream;
    int32_t *lut = S->d_lut, *keep = S->d_lut + 256, *stats = stats_out ? stats_out : S->d_lut + 512;
    const size_t px = (size_t)H * W;
    HIP_TRY(ctx, hipMemsetAsync(S->d_table, 0, 256 * 256 * sizeof(unsigned), st));
    hipLaunchKernelGGL(k_assoc_overlap, dim3((W + MA_TW - 1) / MA_TW, (H + MA_TH * MA_TILES - 1) / (MA_TH * MA_TILES)), dim3(256), 0, st, prev, cur, H, W, classes, n, S->d_table);
    hipLaunchKernelGGL(k_assoc_assign, dim3(1), dim3(256), 0, st, (const unsigned*)S->d_table, classes, n, hold, state, lut, keep, lut_out, stats);
    // the vector body starts where out reaches a 16-byte boundary; cur and prev must reach one at the same element, otherwise every element goes the scalar way
    size_t head = std::min<size_t>(px, ((16 - ((uintptr_t)out & 15)) & 15) / 4);
    if ((((uintptr_t)cur ^ (uintptr_t)out) & 15) || (prev && (((uintptr_t)prev ^ (uintptr_t)out) & 15)) || ((uintptr_t)out & 3)) head = px;
    const size_t n4 = (px - head) / 4; const int tail = (int)(px - head - 4 * n4);
    const unsigned grid = (unsigned)std::min<size_t>(std::max<size_t>((std::max<size_t>(n4, head + tail) + 255) / 256, 1), 2048);
    hipLaunchKernelGGL(k_assoc_relabel, dim3(grid), dim3(256), 0, st, prev, cur, out, (int)head, n4, tail, (const int32_t*)lut, (const int32_t*)keep);
    HIP_TRY(ctx, hipGetLastError());
    return VIDO_OK;
}

}  // extern "C"
