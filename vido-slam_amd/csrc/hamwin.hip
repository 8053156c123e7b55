// hamwin.hip — windowed 256-bit Hamming matcher on gfx950: spatial window, level gate, best and second best, acceptance tests and a one-to-one rule
// (no reference counterpart: the reference associates features by optical flow only; hamming.hip's vido_hamming_match is the bare global 1-NN and is
// untouched).  The rule is include/vido_c.h's, the numpy statement tests/refimpl/hamming_window_np.py.
// Mapping: the train set is cut into chunks of HW_CH entries; workgroup (bx, by) stages chunk by's (x, y, level) in LDS as three planes; each of its four waves owns HW_QW
// queries (wave-uniform: descriptor, position and level sit in scalar registers); lanes stride over the chunk, test window and level from LDS, and only a lane whose entry
// passes for at least one of the wave's queries loads that entry's 32-byte descriptor and popcounts.  Every lane keeps its two smallest keys (distance << 32 | j) per
// query; a wavefront-shuffle butterfly merges (a1, a2) with (b1, b2) into the minimum and second minimum of the union (the two sides of every butterfly step hold disjoint
// j) and lane 0 writes the pair to a [query][chunk][2] table.  k_hamwin_finish folds the chunks of a query (one thread each), applies the tests in the header's order and,
// under `unique`, claims its train entry with a 64-bit atomic minimum of (distance << 32 | i) into the context's owner plane (maskprop.hip's key scheme);
// k_hamwin_resolve then turns the losers into status 4.  Nothing but integer minima and integer sums decides a result, so it depends on no execution order and on no
// launch geometry.  Three launches with `unique`, two without; no memset: the first kernel re-initialises the owner plane and the counters.
#include "common.hpp"

#define HW_QW 4
#define HW_CH 512
#define HW_EMPTY (~0ull)

typedef uint32_t hw_u32x4 __attribute__((ext_vector_type(4)));
typedef hw_u32x4 hw_u32x4_a4 __attribute__((aligned(4)));                     // a descriptor needs 4-byte alignment only
struct HwDesc { hw_u32x4_a4 lo, hi; };

struct HamWinState {
    unsigned long long* d_part = nullptr; size_t cap_part = 0;     // [nq][chunks][2] smallest and second smallest key of a chunk (capacities in bytes)
    unsigned long long* d_owner = nullptr; size_t cap_owner = 0;   // [nt] owner plane of the one-to-one rule
    int32_t* d_stats = nullptr;                                    // the five counters of a device call without a counter array
};

__device__ __forceinline__ void hw_insert(unsigned long long& k1, unsigned long long& k2, unsigned long long key)
{
    const bool lt1 = key < k1, lt2 = key < k2;                  // selects, not branches: a conditional store through either reference would put the arrays in scratch
    k2 = lt1 ? k1 : (lt2 ? key : k2); k1 = lt1 ? key : k1;
}

// minimum and second minimum of the union of two pairs over disjoint j (HW_EMPTY = no entry, larger than every key)
__device__ __forceinline__ void hw_merge(unsigned long long& a1, unsigned long long& a2, unsigned long long b1, unsigned long long b2)
{
    const unsigned long long lo = a1 < b1 ? a1 : b1, hi = a1 < b1 ? b1 : a1, s = a2 < b2 ? a2 : b2;
    a1 = lo; a2 = hi < s ? hi : s;
}

__global__ __launch_bounds__(256) void k_hamwin(const uint32_t* __restrict__ qd, const float* __restrict__ qxy, const int32_t* __restrict__ qlev, int nq,
                                                const HwDesc* __restrict__ td, const float* __restrict__ txy, const int32_t* __restrict__ tlev, int nt,
                                                float radius, int level_tol, int nch, unsigned long long* __restrict__ part,
                                                unsigned long long* __restrict__ owner /* null without `unique` */, int32_t* __restrict__ stats)
{
    __shared__ float sx[HW_CH], sy[HW_CH];
    __shared__ int32_t sl[HW_CH];
    const int jbeg = blockIdx.y * HW_CH, cnt = max(0, min(HW_CH, nt - jbeg));
    for (int t = threadIdx.x; t < cnt; t += 256) {
        sx[t] = txy[2 * (size_t)(jbeg + t)]; sy[t] = txy[2 * (size_t)(jbeg + t) + 1]; sl[t] = tlev[jbeg + t];
        if (owner && blockIdx.x == 0) owner[jbeg + t] = HW_EMPTY;
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 5) stats[threadIdx.x] = 0;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q0 = __builtin_amdgcn_readfirstlane((blockIdx.x * 4 + wave) * HW_QW);
    if (q0 >= nq) return;
    uint32_t Q[HW_QW][8]; float qx[HW_QW], qy[HW_QW]; int ql[HW_QW];
#pragma unroll
    for (int q = 0; q < HW_QW; q++) {
        const int qi = min(q0 + q, nq - 1);                          // wave-uniform addresses -> scalar loads
#pragma unroll
        for (int w = 0; w < 8; w++) Q[q][w] = qd[(size_t)qi * 8 + w];
        qx[q] = qxy[2 * (size_t)qi]; qy[q] = qxy[2 * (size_t)qi + 1]; ql[q] = qlev[qi];
    }
    unsigned long long k1[HW_QW], k2[HW_QW];
#pragma unroll
    for (int q = 0; q < HW_QW; q++) k1[q] = k2[q] = HW_EMPTY;
    for (int t = lane; t < cnt; t += 64) {
        const float tx = sx[t], ty = sy[t]; const int tl = sl[t];
        unsigned pass = 0;
#pragma unroll
        for (int q = 0; q < HW_QW; q++) {
            const long long dl = (long long)tl - (long long)ql[q];
            const bool in = fabsf(tx - qx[q]) <= radius && fabsf(ty - qy[q]) <= radius;      // one fp32 subtraction and one compare each; false for NaN
            const bool lv = level_tol < 0 || (dl < 0 ? -dl : dl) <= (long long)level_tol;
            pass |= (in && lv) ? 1u << q : 0u;
        }
        if (pass) {
            const int j = jbeg + t;
            const hw_u32x4 b0 = td[j].lo, b1 = td[j].hi;
#pragma unroll
            for (int q = 0; q < HW_QW; q++) {
                const int d = __popc(b0.x ^ Q[q][0]) + __popc(b0.y ^ Q[q][1]) + __popc(b0.z ^ Q[q][2]) + __popc(b0.w ^ Q[q][3]) +
                              __popc(b1.x ^ Q[q][4]) + __popc(b1.y ^ Q[q][5]) + __popc(b1.z ^ Q[q][6]) + __popc(b1.w ^ Q[q][7]);
                hw_insert(k1[q], k2[q], (pass >> q & 1u) ? ((unsigned long long)(uint32_t)d << 32) | (uint32_t)j : HW_EMPTY);      // HW_EMPTY inserts nothing
            }
        }
    }
#pragma unroll
    for (int q = 0; q < HW_QW; q++) {
        unsigned long long a1 = k1[q], a2 = k2[q];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const unsigned long long b1 = __shfl_xor(a1, o, 64), b2 = __shfl_xor(a2, o, 64);
            hw_merge(a1, a2, b1, b2);
        }
        if (lane == 0 && q0 + q < nq) { unsigned long long* p = part + ((size_t)(q0 + q) * nch + blockIdx.y) * 2; p[0] = a1; p[1] = a2; }
    }
}

__device__ __forceinline__ void hw_count(int st, bool live, int32_t* __restrict__ stats)
{
#pragma unroll
    for (int s = 0; s < 5; s++) {
        const unsigned long long b = __ballot(live && st == s);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(stats + s, __popcll(b));
    }
}

// folds the chunks, writes dist / dist2 and the verdict; under `unique` a query that passed claims its train entry and the counting is left to k_hamwin_resolve
__global__ __launch_bounds__(256) void k_hamwin_finish(const unsigned long long* __restrict__ part, int nch, int nq, int max_dist, int ratio_num, int ratio_den,
                                                       unsigned long long* __restrict__ owner, int32_t* __restrict__ idx, int32_t* __restrict__ dist,
                                                       int32_t* __restrict__ dist2, int32_t* __restrict__ status, int32_t* __restrict__ stats)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < nq;
    int st = 1;
    if (live) {
        unsigned long long a1 = HW_EMPTY, a2 = HW_EMPTY;
        for (int c = 0; c < nch; c++) { const unsigned long long* p = part + ((size_t)i * nch + c) * 2; hw_merge(a1, a2, p[0], p[1]); }
        const int d1 = a1 == HW_EMPTY ? -1 : (int)(a1 >> 32), d2 = a2 == HW_EMPTY ? -1 : (int)(a2 >> 32), j = (int)(uint32_t)a1;
        if (d1 < 0) st = 1;
        else if (d1 > max_dist) st = 2;
        else if (ratio_num > 0 && d2 >= 0 && !(d1 * ratio_den < d2 * ratio_num)) st = 3;
        else st = 0;
        if (st == 0 && owner) atomicMin(owner + j, ((unsigned long long)(uint32_t)d1 << 32) | (uint32_t)i);
        idx[i] = st == 0 ? j : -1; dist[i] = d1; dist2[i] = d2; status[i] = st;
    }
    if (!owner) hw_count(st, live, stats);
}

__global__ __launch_bounds__(256) void k_hamwin_resolve(const unsigned long long* __restrict__ owner, int nq, int32_t* __restrict__ idx, const int32_t* __restrict__ dist,
                                                        int32_t* __restrict__ status, int32_t* __restrict__ stats)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < nq;
    int st = 1;
    if (live) {
        st = status[i];
        if (st == 0 && owner[idx[i]] != (((unsigned long long)(uint32_t)dist[i] << 32) | (uint32_t)i)) { st = 4; status[i] = 4; idx[i] = -1; }
    }
    hw_count(st, live, stats);
}

// ---- host ------------------------------------------------------------------------------------------
void hamwin_state_destroy(vido_ctx* ctx)
{
    HamWinState* S = ctx->hamwin;
    if (!S) return;
    if (S->d_part) (void)hipFree(S->d_part);
    if (S->d_owner) (void)hipFree(S->d_owner);
    if (S->d_stats) (void)hipFree(S->d_stats);
    delete S; ctx->hamwin = nullptr;
}

extern "C" int vido_hamming_match_window(vido_ctx* ctx, const uint8_t* q_desc, const float* q_xy, const int32_t* q_level, int nq,
                                         const uint8_t* t_desc, const float* t_xy, const int32_t* t_level, int nt,
                                         float radius, int level_tol, int max_dist, int ratio_num, int ratio_den, int unique,
                                         int32_t* idx_out, int32_t* dist_out, int32_t* dist2_out, int32_t* status_out, int32_t* stats_out, int on_device)
{
    if (!ctx) return VIDO_E_INVALID;
    if (nq < 0 || nt < 0 || (nq > 0 && (!q_desc || !q_xy || !q_level || !idx_out || !dist_out || !dist2_out || !status_out)) || (nt > 0 && (!t_desc || !t_xy || !t_level)))
        return vido_set_error(ctx, VIDO_E_INVALID, "hamming_match_window: bad arguments");
    if (!(radius >= 0.f) || !(radius < __builtin_inff()))
        return vido_set_error(ctx, VIDO_E_INVALID, "hamming_match_window: radius must be finite and >= 0");
    if (ratio_num != 0 && !(0 < ratio_num && ratio_num <= ratio_den && ratio_den <= 1024))
        return vido_set_error(ctx, VIDO_E_INVALID, "hamming_match_window: ratio %d / %d outside 0 < num <= den <= 1024", ratio_num, ratio_den);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (nq == 0) {
        if (stats_out) { if (on_device) HIP_TRY(ctx, hipMemsetAsync(stats_out, 0, 5 * sizeof(int32_t), st)); else memset(stats_out, 0, 5 * sizeof(int32_t)); }
        return VIDO_OK;
    }
    if (!ctx->hamwin) ctx->hamwin = new HamWinState();
    HamWinState* S = ctx->hamwin;
    const int nch = std::max(1, (nt + HW_CH - 1) / HW_CH);
    if (!S->d_stats) HIP_TRY(ctx, hipMalloc((void**)&S->d_stats, 5 * sizeof(int32_t)));
    if (int rc = vido_grow_device(ctx, st, (void**)&S->d_part, &S->cap_part, (size_t)nq * nch * 16, GROW_HEADROOM)) return rc;
    if (unique) if (int rc = vido_grow_device(ctx, st, (void**)&S->d_owner, &S->cap_owner, (size_t)std::max(nt, 1) * 8, GROW_HEADROOM)) return rc;
    if (!on_device) {                                                      // the host form: from here on the pointers are their slots of the staging buffer
        HostStaging& T = ctx->staging;
        T.begin(); T.in(&q_desc, (size_t)nq * 32); T.in(&q_xy, (size_t)nq * 8); T.in(&q_level, (size_t)nq * 4); T.in(&t_desc, (size_t)nt * 32); T.in(&t_xy, (size_t)nt * 8); T.in(&t_level, (size_t)nt * 4);
        T.out(&idx_out, (size_t)nq * 4); T.out(&dist_out, (size_t)nq * 4); T.out(&dist2_out, (size_t)nq * 4); T.out(&status_out, (size_t)nq * 4); T.keep(&stats_out, 5 * sizeof(int32_t));
        if (int rc = staging_upload(ctx, st)) return rc;
    }
    int32_t* dstats = stats_out ? stats_out : S->d_stats;
    unsigned long long* owner = unique ? S->d_owner : nullptr;
    const int qblocks = (nq + 4 * HW_QW - 1) / (4 * HW_QW);
    hipLaunchKernelGGL(k_hamwin, dim3(qblocks, nch), dim3(256), 0, st, (const uint32_t*)q_desc, q_xy, q_level, nq, (const HwDesc*)t_desc, t_xy, t_level, nt, radius, level_tol, nch,
                       S->d_part, owner, dstats);
    hipLaunchKernelGGL(k_hamwin_finish, dim3((nq + 255) / 256), dim3(256), 0, st, (const unsigned long long*)S->d_part, nch, nq, max_dist, ratio_num, ratio_den, owner,
                       idx_out, dist_out, dist2_out, status_out, dstats);
    if (unique)
        hipLaunchKernelGGL(k_hamwin_resolve, dim3((nq + 255) / 256), dim3(256), 0, st, (const unsigned long long*)owner, nq, idx_out, (const int32_t*)dist_out, status_out, dstats);
    HIP_TRY(ctx, hipGetLastError());
    if (!on_device) return staging_download(ctx, st);
    return VIDO_OK;
}
