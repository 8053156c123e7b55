// maskcc.hip — split a class label image into instances: connected-component labelling on gfx950 (no reference counterpart: the reference's label image is
// sum(mask * class_index), one label per class; Tracking::DynObjTracking then gives every car of a frame one motion).
// Rule (include/vido_c.h; the numpy statement is tests/refimpl/mask_components_np.py): a pixel is foreground iff mask > 0; a component is a maximal set of
// foreground pixels of EQUAL value joined by 4- or 8-neighbour steps; its anchor is its smallest raster index, its area its pixel count.  Components below min_area are
// dropped; the survivors in ascending anchor order are k = 0, 1, ...: k < cap is written as id_base + 1 + k with its class and area, every other pixel is written 0.
// One memset and seven launches on one stream, union-find rooted at the smallest index throughout (a parent never exceeds its child, so a root IS the anchor):
//   k_cc_local    a workgroup labels a 32 x 32 tile in LDS and writes global parent indices (-1: background) — every pixel of the parent plane;
//   k_cc_seam     the pixels on a tile's border union with their backward neighbours in other tiles: find both roots, atomicMin(&parent[larger], smaller), continue from
//                 the returned value.  Values only decrease, so every loop ends; no workgroup waits for another.  EVERY access to the parent plane in this launch is an
//                 agent-scope atomic (another workgroup, maybe on another XCD, updates the same words); plain loads are for words that earlier launches wrote;
//   k_cc_flatten  parent = root for every pixel, and the areas added at the root: equal roots of a wave are folded by ballot into one atomic (k_assoc_overlap's loop);
//   k_cc_rowcount roots and surviving roots per image row;   k_cc_scan  ONE workgroup: exclusive scan of the <= 4095 row counts, the four counters, zeros behind `kept`;
//   k_cc_rank     a workgroup per row that holds a root: rank = row base + ballot / popcount position; the root's word of the area plane becomes its output id, its class
//                 (read here, BEFORE the relabel may overwrite mask) and area go to the per-component outputs;
//   k_cc_relabel  out = id of the pixel's root, EVERY pixel, 16-byte stores from out's first 16-byte boundary with scalar head and tail.
// The area plane is cleared by the memset in FRONT of the first launch, never by a kernel afterwards (the key plane's reasons).  Both planes are addressed
// from an element offset chosen per call so that they reach a 16-byte boundary at the same pixel as `out`.  Integer minima and sums only: no execution order matters.
#include "common.hpp"
#include "ccunion.hpp"                                          // cc_lfind / cc_lunion (LDS) and cc_gfind / cc_gunion (global, agent-scope atomics)

struct MaskCCState {
    int32_t* d_parent = nullptr;                                  // [cap_px + 8] parent index per pixel, -1 = background
    int32_t* d_area = nullptr;                                    // [cap_px + 8] area at a root, later the root's output id; 0 elsewhere
    int32_t* d_rows = nullptr;                                    // [3][4096] per row: surviving roots, roots, exclusive base of the survivors; then 4 words: the counters
    int32_t* h_stats = nullptr;                                   // pinned mirror (vido_frame_split_mask's host result)
    size_t cap_px = 0;
};

#define CC_T 32                                                   // tile edge
#define CC_PX (CC_T * CC_T)
#define CC_ROWS 4096

// One workgroup per 32 x 32 tile, four pixels per thread (rows ry0, ry0 + 8, ...).  Local index l = ry * 32 + rx orders like the raster index inside the tile, so the local
// root is the tile part's smallest raster index.  A pixel starts under the first pixel of its horizontal run (half a wave holds a tile row: the run's start is the highest
// "differs from its left neighbour" bit of the ballot at or below the lane), and rows are then joined run by run, not pixel by pixel: a pixel whose upper neighbour is equal
// unions with it only where one of the two runs starts (further right the pixel to the left has joined the same two runs); where the upper neighbour differs, an equal
// upper-left / upper-right neighbour is the end / start of a run that touches this one by the corner only.  A tile inside a blob makes 31 unions instead of 4 000.
__global__ __launch_bounds__(256) void k_cc_local(const int32_t* __restrict__ mask, int H, int W, int conn8, int32_t* __restrict__ parent)
{
    __shared__ int val[CC_PX], par[CC_PX];
    const int x0 = blockIdx.x * CC_T, y0 = blockIdx.y * CC_T;
    const int rx = threadIdx.x & (CC_T - 1), ry0 = threadIdx.x / CC_T;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int ry = ry0 + 8 * k, l = ry * CC_T + rx, x = x0 + rx, y = y0 + ry;
        int v = 0;
        if (x < W && y < H) { v = mask[(size_t)y * W + x]; if (v < 0) v = 0; }
        val[l] = v;
    }
    __syncthreads();
    bool starts[4];                                                 // this pixel is the first of its run
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int ry = ry0 + 8 * k, l = ry * CC_T + rx;
        const int v = val[l];
        starts[k] = rx == 0 || val[l - 1] != v;
        const unsigned long long b = __ballot(starts[k]);
        const unsigned row = (unsigned)(b >> (threadIdx.x & 32));   // the tile row of this half of the wave; bit 0 is set
        par[l] = ry * CC_T + (31 - __clz(row & (0xffffffffu >> (31 - rx))));
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int ry = ry0 + 8 * k, l = ry * CC_T + rx;
        const int v = val[l];
        if (v == 0 || ry == 0) continue;
        if (val[l - CC_T] == v) {
            if (starts[k] || val[l - CC_T - 1] != v) cc_lunion(par, l, l - CC_T);      // (starts[k] covers rx == 0: no read left of the row)
        } else if (conn8) {
            if (rx > 0 && val[l - CC_T - 1] == v) cc_lunion(par, l, l - CC_T - 1);
            if (rx < CC_T - 1 && val[l - CC_T + 1] == v) cc_lunion(par, l, l - CC_T + 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int ry = ry0 + 8 * k, l = ry * CC_T + rx, x = x0 + rx, y = y0 + ry;
        if (x >= W || y >= H) continue;
        int g = -1;
        if (val[l] != 0) { const int r = cc_lfind(par, l); g = (y0 + r / CC_T) * W + x0 + (r & (CC_T - 1)); }
        parent[(size_t)y * W + x] = g;
    }
}

// One workgroup of 128 per tile; thread j < 94 owns one border pixel: the top row (32), the left column below it (31), the right column below it (31).  Each looks at its
// backward neighbours (left, up-left, up, up-right) and unions with those that lie in ANOTHER tile and hold the same value; every pair of neighbours across a seam has
// exactly one backward member, and that member is on its tile's top row, left column or (up-right only) right column.  Unions that others imply are left out: with an
// equal upper neighbour both upper diagonals are (they sit in the upper neighbour's row run, and a row run is joined across tiles by the left-column unions), and so is
// the upper one itself where the left and the upper-left pixels are equal too (the pixel to the left, a border pixel of its own tile's top row, joins the same two row
// runs); with an equal left neighbour the upper-left one is (it sits right above the left neighbour in that neighbour's tile, except on the top row, where the upper
// neighbour's rule has already spoken).  A seam through the inside of a blob costs one union per row of the left column and none along the top row.
__global__ __launch_bounds__(128) void k_cc_seam(const int32_t* __restrict__ mask, int H, int W, int conn8, int32_t* parent)
{
    const int j = threadIdx.x;
    int rx, ry;
    if (j < CC_T) { rx = j; ry = 0; }
    else if (j < 2 * CC_T - 1) { rx = 0; ry = j - CC_T + 1; }
    else if (j < 3 * CC_T - 2) { rx = CC_T - 1; ry = j - (2 * CC_T - 1) + 1; }
    else return;
    const int x = blockIdx.x * CC_T + rx, y = blockIdx.y * CC_T + ry;
    if (x >= W || y >= H) return;
    const int i = y * W + x;
    const int v = mask[i];
    if (v <= 0) return;
    const bool hl = x > 0, hu = y > 0, hr = x + 1 < W;
    const bool el = hl && mask[i - 1] == v, eu = hu && mask[i - W] == v, eul = hl && hu && mask[i - W - 1] == v, eur = hr && hu && mask[i - W + 1] == v;
    if (rx == 0 && el) cc_gunion(parent, i, i - 1);                                  // the vertical seam, row by row
    if (ry == 0) {                                                                   // the horizontal seam
        if (eu) { if (!(el && eul)) cc_gunion(parent, i, i - W); }
        else if (conn8) { if (eul) cc_gunion(parent, i, i - W - 1); if (eur) cc_gunion(parent, i, i - W + 1); }
    } else if (conn8) {                                                              // below the top row only the diagonals across the vertical seams are left
        if (rx == 0 && eul && !el) cc_gunion(parent, i, i - W - 1);
        if (rx == CC_T - 1 && eur && !eu) cc_gunion(parent, i, i - W + 1);
    }
}

// parent[i] = root(i) and area[root] += 1.  A wave holds 64 consecutive pixels: one or two roots mostly, folded by ballot.  The walk reads words that other threads of this
// launch overwrite with their roots (an ancestor replaces an ancestor: the walk still ends at the root); those accesses are agent-scope atomics as in k_cc_seam.
__global__ __launch_bounds__(256) void k_cc_flatten(int32_t* parent, unsigned npx, int32_t* __restrict__ area)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    int r = -1;
    if (i < npx) {
        const int p = __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p >= 0) {
            r = cc_gfind(parent, p);
            if (r != p) __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    bool todo = r >= 0;
    unsigned long long m = __ballot(todo);
    const int lane = threadIdx.x & 63;
    while (m) {                                                     // (m is wave-uniform)
        const int leader = __ffsll((long long)m) - 1;
        const int lr = __shfl(r, leader);
        const bool same = todo && r == lr;
        const unsigned long long b = __ballot(same);
        if (lane == leader) atomicAdd(area + lr, __popcll(b));
        todo = todo && !same;
        m &= ~b;
    }
}

// rows[y] = roots of row y with area >= min_area, rows[4096 + y] = roots of row y.  One workgroup per row.
__global__ __launch_bounds__(256) void k_cc_rowcount(const int32_t* __restrict__ parent, const int32_t* __restrict__ area, int W, int min_area, int32_t* __restrict__ rows)
{
    __shared__ int acc[2];
    const int y = blockIdx.x, t = threadIdx.x;
    if (t < 2) acc[t] = 0;
    __syncthreads();
    int found = 0, surv = 0;
    for (int x = t; x < W; x += 256) {
        const int i = y * W + x;
        if (parent[i] == i) { found++; if (area[i] >= min_area) surv++; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { found += __shfl_down(found, o); surv += __shfl_down(surv, o); }
    if ((t & 63) == 0 && found) { atomicAdd(&acc[0], surv); atomicAdd(&acc[1], found); }
    __syncthreads();
    if (t == 0) { rows[y] = acc[0]; rows[CC_ROWS + y] = acc[1]; }
}

// ONE workgroup: rows[8192 + y] = survivors in the rows above y; stats = found, dropped for area, left out for cap, kept; the per-component outputs from `kept` to cap: 0.
__global__ __launch_bounds__(256) void k_cc_scan(int32_t* __restrict__ rows, int H, int cap, int64_t* __restrict__ classes_out /* may be null */,
                                                 int32_t* __restrict__ area_out /* may be null */, int32_t* __restrict__ stats)
{
    __shared__ int part[256], fnd[256];
    const int t = threadIdx.x;
    int s = 0, f = 0;
    for (int k = 0; k < 16; k++) { const int y = t * 16 + k; if (y < H) { s += rows[y]; f += rows[CC_ROWS + y]; } }
    part[t] = s; fnd[t] = f;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {                             // inclusive scan of the survivors, plain sum of the roots
        const int a = t >= o ? part[t - o] : 0, b = t + o < 256 && (t & (2 * o - 1)) == 0 ? fnd[t + o] : 0;
        __syncthreads();
        part[t] += a; fnd[t] += b;
        __syncthreads();
    }
    int base = part[t] - s;
    for (int k = 0; k < 16; k++) { const int y = t * 16 + k; if (y < H) { rows[2 * CC_ROWS + y] = base; base += rows[y]; } }
    const int surv = part[255], found = fnd[0], kept = surv < cap ? surv : cap;
    if (t == 0) { stats[0] = found; stats[1] = found - surv; stats[2] = surv - kept; stats[3] = kept; }
    if (t >= kept && t < cap) { if (classes_out) classes_out[t] = 0; if (area_out) area_out[t] = 0; }      // cap <= 254 < 256
}

// A workgroup per row, gone at once when the row holds no root.  The row is walked in chunks of 256 pixels in order; a surviving root's rank is the row's base + the
// survivors of the chunks before + of the waves before in this chunk + of the lanes before in this wave.
__global__ __launch_bounds__(256) void k_cc_rank(const int32_t* __restrict__ mask, const int32_t* __restrict__ parent, int32_t* __restrict__ area, int W, int min_area,
                                                 int id_base, int cap, const int32_t* __restrict__ rows, int64_t* __restrict__ classes_out /* may be null */,
                                                 int32_t* __restrict__ area_out /* may be null */)
{
    __shared__ int wcnt[4];
    const int y = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (rows[CC_ROWS + y] == 0) return;                             // (uniform over the workgroup)
    int run = rows[2 * CC_ROWS + y];
    for (int xb = 0; xb < W; xb += 256) {
        const int x = xb + t, i = y * W + x;
        bool root = false, surv = false; int a = 0;
        if (x < W && parent[i] == i) { root = true; a = area[i]; surv = a >= min_area; }
        const unsigned long long b = __ballot(surv);
        if (lane == 0) wcnt[wave] = __popcll(b);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) { const int c = wcnt[w]; all += c; if (w < wave) before += c; }
        if (root) {
            int id = 0;
            if (surv) {
                const int k = run + before + __popcll(b & ((1ull << lane) - 1ull));
                if (k < cap) {
                    id = id_base + 1 + k;
                    if (classes_out) classes_out[k] = (int64_t)mask[i];
                    if (area_out) area_out[k] = a;
                }
            }
            area[i] = id;
        }
        run += all;
        __syncthreads();
    }
}

// out = id of the root, 0 on background; EVERY pixel is written.  [0, npx): `head` scalars, n4 vectors of four from there, `tail` scalars (k_assoc_relabel's split); the
// parent plane is addressed so that it reaches a 16-byte boundary where out does.  mask is not read: out may be mask.
__device__ __forceinline__ int32_t cc_one(const int32_t* __restrict__ ids, int p) { return p >= 0 ? ids[p] : 0; }
__global__ __launch_bounds__(256) void k_cc_relabel(const int32_t* __restrict__ parent, const int32_t* __restrict__ ids, int32_t* __restrict__ out, int head, size_t n4, int tail)
{
    const size_t t0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    const int4* p4 = (const int4*)(parent + head); int4* o4 = (int4*)(out + head);
    for (size_t i = t0; i < n4; i += stride) {
        const int4 p = p4[i];
        int4 r;
        r.x = cc_one(ids, p.x); r.y = cc_one(ids, p.y); r.z = cc_one(ids, p.z); r.w = cc_one(ids, p.w);
        o4[i] = r;
    }
    for (size_t j = t0; j < (size_t)head + (size_t)tail; j += stride) {
        const size_t e = j < (size_t)head ? j : (size_t)head + 4 * n4 + (j - (size_t)head);
        out[e] = cc_one(ids, parent[e]);
    }
}

// ---- host ------------------------------------------------------------------------------------------
static int maskcc_state(vido_ctx* ctx, MaskCCState** out)
{
    if (ctx->mcc) { *out = ctx->mcc; return VIDO_OK; }
    MaskCCState* S = new MaskCCState();
    ctx->mcc = S;                                                 // (a failed allocation below leaves a partial state: vido_destroy frees what exists, the next call refuses)
    const size_t px = (size_t)ctx->cfg.width * ctx->cfg.height;
    HIP_TRY(ctx, hipMalloc((void**)&S->d_parent, (px + 8) * 4));
    HIP_TRY(ctx, hipMalloc((void**)&S->d_area, (px + 8) * 4));
    HIP_TRY(ctx, hipMalloc((void**)&S->d_rows, (3 * CC_ROWS + 4) * 4));
    HIP_TRY(ctx, hipHostMalloc((void**)&S->h_stats, 16));
    S->cap_px = px;
    *out = S;
    return VIDO_OK;
}

void maskcc_state_destroy(vido_ctx* ctx)
{
    MaskCCState* S = ctx->mcc;
    if (!S) return;
    if (S->d_parent) hipFree(S->d_parent);
    if (S->d_area) hipFree(S->d_area);
    if (S->d_rows) hipFree(S->d_rows);
    if (S->h_stats) hipHostFree(S->h_stats);
    delete S; ctx->mcc = nullptr;
}

static int maskcc_check(vido_ctx* ctx, const char* who, int H, int W, int connectivity, int id_base, int cap)
{
    if (connectivity != 4 && connectivity != 8) return vido_set_error(ctx, VIDO_E_INVALID, "%s: connectivity %d, 4 or 8 expected", who, connectivity);
    if (H < 1 || W < 1 || H > 4095 || W > 4095 || (size_t)H * W > (size_t)ctx->cfg.width * ctx->cfg.height)
        return vido_set_error(ctx, VIDO_E_INVALID, "%s: %d x %d outside the context's %d x %d pixels", who, W, H, ctx->cfg.width, ctx->cfg.height);
    if (id_base < 0 || cap < 1) return vido_set_error(ctx, VIDO_E_INVALID, "%s: id_base = %d (>= 0), cap = %d (>= 1)", who, id_base, cap);
    if ((long long)id_base + cap > 254) return vido_set_error(ctx, VIDO_E_CAPACITY, "%s: id_base %d + cap %d, the id space ends at 254", who, id_base, cap);
    return VIDO_OK;
}

// the memset + the seven launches on `st`; stats: DEVICE, four words (never null here)
static int maskcc_enqueue(vido_ctx* ctx, MaskCCState* S, hipStream_t st, const int32_t* mask, int H, int W, int connectivity, int min_area, int id_base, int cap,
                          int32_t* out, int64_t* classes_out, int32_t* area_out, int32_t* stats)
{
    if (!S->h_stats || S->cap_px < (size_t)H * W) return vido_set_error(ctx, VIDO_E_HIP, "mask_components: the context's planes were not allocated");
    const size_t px = (size_t)H * W;
    const int conn8 = connectivity == 8;
    // pixel e of both planes lives at element e + sh: the planes are 16-byte aligned where out is (an out that is not 4-byte aligned goes the scalar way throughout)
    const bool vec = ((uintptr_t)out & 3) == 0;
    const size_t head = vec ? std::min<size_t>(px, ((16 - ((uintptr_t)out & 15)) & 15) / 4) : px;
    const int sh = vec ? (int)((4 - head % 4) % 4) : 0;
    int32_t *P = S->d_parent + sh, *A = S->d_area + sh;
    HIP_TRY(ctx, hipMemsetAsync(S->d_area, 0, ((px + 4) * 4 + 15) & ~(size_t)15, st));
    const dim3 tiles((W + CC_T - 1) / CC_T, (H + CC_T - 1) / CC_T);
    hipLaunchKernelGGL(k_cc_local, tiles, dim3(256), 0, st, mask, H, W, conn8, P);
    hipLaunchKernelGGL(k_cc_seam, tiles, dim3(128), 0, st, mask, H, W, conn8, P);
    hipLaunchKernelGGL(k_cc_flatten, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, st, P, (unsigned)px, A);
    hipLaunchKernelGGL(k_cc_rowcount, dim3(H), dim3(256), 0, st, (const int32_t*)P, (const int32_t*)A, W, min_area, S->d_rows);
    hipLaunchKernelGGL(k_cc_scan, dim3(1), dim3(256), 0, st, S->d_rows, H, cap, classes_out, area_out, stats);
    hipLaunchKernelGGL(k_cc_rank, dim3(H), dim3(256), 0, st, mask, (const int32_t*)P, A, W, min_area, id_base, cap, (const int32_t*)S->d_rows, classes_out, area_out);
    const size_t n4 = (px - head) / 4; const int tail = (int)(px - head - 4 * n4);
    const unsigned grid = (unsigned)std::min<size_t>(std::max<size_t>((std::max<size_t>(n4, head + tail) + 255) / 256, 1), 2048);
    hipLaunchKernelGGL(k_cc_relabel, dim3(grid), dim3(256), 0, st, (const int32_t*)P, (const int32_t*)A, out, (int)head, n4, tail);
    HIP_TRY(ctx, hipGetLastError());
    return VIDO_OK;
}

extern "C" {

int vido_mask_components(vido_ctx* ctx, const int32_t* mask, int H, int W, int connectivity, int min_area, int id_base, int cap, int32_t* out, int64_t* classes_out,
                         int32_t* area_out, int32_t* stats_out)
{
    if (!ctx) return VIDO_E_INVALID;
    if (!mask || !out) return vido_set_error(ctx, VIDO_E_INVALID, "mask_components: null image");
    int rc = maskcc_check(ctx, "mask_components", H, W, connectivity, id_base, cap); if (rc) return rc;
    const size_t bytes = (size_t)H * W * 4;
    if (out != mask && (uintptr_t)out < (uintptr_t)mask + bytes && (uintptr_t)mask < (uintptr_t)out + bytes)
        return vido_set_error(ctx, VIDO_E_INVALID, "mask_components: out overlaps mask without being mask");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    MaskCCState* S; rc = maskcc_state(ctx, &S); if (rc) return rc;
    hipStream_t st = ctx->has_ext_stream ? ctx->ext_stream : ctx->stream;
    return maskcc_enqueue(ctx, S, st, mask, H, W, connectivity, min_area, id_base, cap, out, classes_out, area_out, stats_out ? stats_out : S->d_rows + 3 * CC_ROWS);
}

int vido_frame_split_mask(vido_ctx* ctx, int slot, int connectivity, int min_area, int id_base, int cap, int32_t* stats_out)
{
    if (!ctx) return VIDO_E_INVALID;
    float *d, *f; int32_t* m; int W = 0, H = 0;
    if (track_slot_maps(ctx, slot, &d, &f, &m, &W, &H) != VIDO_OK) return vido_set_error(ctx, VIDO_E_INVALID, "frame_split_mask: bad slot %d", slot);
    int rc = maskcc_check(ctx, "frame_split_mask", H, W, connectivity, id_base, cap); if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    MaskCCState* S; rc = maskcc_state(ctx, &S); if (rc) return rc;
    hipStream_t st = ctx->stream;                                 // the tracker's stream: the slot maps are ordered on it
    int32_t* stats = S->d_rows + 3 * CC_ROWS;
    if ((rc = maskcc_enqueue(ctx, S, st, m, H, W, connectivity, min_area, id_base, cap, m, nullptr, nullptr, stats))) return rc;
    if (stats_out) {
        HIP_TRY(ctx, hipMemcpyAsync(S->h_stats, stats, 16, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        memcpy(stats_out, S->h_stats, 16);
    }
    return VIDO_OK;
}

}  // extern "C"
