// common.hpp — ctx layout and error plumbing shared by the HIP translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/vido_c.h"


struct LevelInfo {
    int w, h, pitch;               // level size, row pitch in bytes (multiple of 64)
    int off;                       // byte offset of the level inside one frame's pyramid slab
    int first_cell, n_cells;       // cells of this level inside the cell table (reference order)
    int xtab_off, ytab_off;        // offsets (elements) into the resize tables
    int n_budget;                  // mnFeaturesPerLevel
    float scale;                   // mvScaleFactor
    int rs_rows, rs_ndw;           // resize staging tile: max source rows / dwords per row of a 128x8 output tile
};

struct PyrDev {                    // passed by value to kernels
    int n_levels;
    int w[VIDO_MAX_LEVELS], h[VIDO_MAX_LEVELS], pitch[VIDO_MAX_LEVELS], off[VIDO_MAX_LEVELS];
};

struct CellDesc { int level, x0, y0, sw, sh, pad0, pad1, pad2; };   // FAST sub-image of one cell (level coords)
struct BlurTile { int level, tx, ty, pad; };

// Host staging (ctx.cpp): the one device + pinned buffer pair behind every host form (on_device = 0).  A call declares its fields in order — inputs, outputs, then
// fields read and written in one slot — each by the address of the pointer it will launch with, which holds the caller's HOST pointer: staging_upload copies the inputs
// over and repoints every such pointer at the field's device slot (offsets are multiples of 16); staging_download brings back each output that was asked for and waits
// for the stream.  A field whose host pointer is NULL takes no copy and gets a null device pointer, unless it was declared with keep(): then the slot is there for the
// kernels and nothing comes back.  One user at a time: a host form ends in staging_download's wait, so the buffers are free at every entry; the device forms never
// touch them.
struct HostStaging {
    static constexpr int MAX_FIELDS = 12;
    struct Field { void **in, **out; const void* src; void* dst; size_t bytes, off; bool keep; };
    uint8_t *d = nullptr, *h = nullptr; size_t cap = 0;
    Field f[MAX_FIELDS]; int n = 0; size_t total = 0;
    void begin() { n = 0; total = 0; }
    void add(void** in, void** out, size_t bytes, bool keep)
    {
        if (n < MAX_FIELDS) f[n] = Field{in, out, in ? *in : nullptr, out ? *out : nullptr, bytes, total, keep};
        n++; total += (bytes + 15) & ~(size_t)15;
    }
    template <class T> void in(const T** p, size_t bytes) { add((void**)p, nullptr, bytes, false); }
    template <class T> void out(T** p, size_t bytes) { add(nullptr, (void**)p, bytes, false); }
    template <class T> void keep(T** p, size_t bytes) { add(nullptr, (void**)p, bytes, true); }                    // an output whose slot the kernels need even when the caller passes NULL
    template <class T> void inout(const T** pi, T** po, size_t bytes) { add((void**)pi, (void**)po, bytes, false); }
};

struct OrbState;                   // orb.hip
struct TrackState;                 // track.hip
struct BaState;                    // ba.hip

struct vido_ctx {
    vido_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;
    hipStream_t ext_stream = nullptr;  // vido_set_stream: caller-owned stream for the on_device network ops
    bool has_ext_stream = false;
    std::string err;
    char dev_name[256] = {0};
    OrbState* orb = nullptr;
    TrackState* trk = nullptr;
    BaState* ba = nullptr;
    struct HamState* ham = nullptr;
    struct HamWinState* hamwin = nullptr;    // hamwin.hip: chunk partials, owner plane and spare counters of vido_hamming_match_window
    struct DisFlowState* disflow = nullptr;  // disflow.hip: pyramids and per-level fields of vido_dis_flow
    struct StereoState* stereo = nullptr;    // stereosgm.hip: grey and census planes and the S volume of vido_stereo_sgm
    struct StereoFilterState* sfilter = nullptr; // stereofilter.hip: parent and area planes of vido_stereo_filter
    HostStaging staging;                     // the buffers of every host form (above)
    struct PoseState* pose = nullptr;
    struct NetState* net = nullptr;
    struct PnpState* pnp = nullptr;
    struct MaskPropState* mprop = nullptr;   // maskprop.hip: key plane + counters of vido_mask_propagate / vido_frame_propagate_mask
    struct MaskAssocState* massoc = nullptr; // maskassoc.hip: count table + lookups of vido_mask_associate
    struct MaskCCState* mcc = nullptr;       // maskcc.hip: parent plane, area / id plane and row counts of vido_mask_components / vido_frame_split_mask
    struct BaWin* bawin = nullptr;     // bawin.hip: the device-resident local-BA window
    void* detpost_buf = nullptr; size_t detpost_cap = 0; unsigned long long detpost_sig = 0;   // detpost.hip: scratch of the RPN selection (keys, histograms, state)
    void* rccl_comm = nullptr;         // ncclComm_t of vido_rccl_init (rccl.cpp): the sharded BA's all-reduce on this context's stream
    int rccl_rank = 0, rccl_world = 1;
    unsigned* c1_range_flag = nullptr; // rangelatch.hip: pinned host word the split-fp16 kernels raise when an activation leaves fp16's range (vido_conv1x1_range_flag)
};

int vido_set_error(vido_ctx* ctx, int code, const char* fmt, ...);
// (ctx.cpp) the two halves of a host form around its launches, over the fields declared on ctx->staging since begin()
int staging_upload(vido_ctx* ctx, hipStream_t st);
int staging_download(vido_ctx* ctx, hipStream_t st);
// (ctx.cpp) device scratch of at least `need` bytes: growing waits for the call's stream, and for the context's if that is another one (earlier calls may still use the
// old buffer), frees, records capacity 0 and allocates `need` bytes (GROW_EXACT) or need + need / 2 + 512 (GROW_HEADROOM)
enum GrowPolicy { GROW_EXACT, GROW_HEADROOM };
int vido_grow_device(vido_ctx* ctx, hipStream_t st, void** p, size_t* cap, size_t need, GrowPolicy policy);
// VIDO_CALL_PROF=1: named host-side sections inside the library (ctx.cpp keeps the table, prints it at exit next to the facade's per-call table).  A section that ends with
// `sync` waits for the stream first, so that the section owns the device time of what it enqueued (diagnosis only: the waits change the overlap they measure).
bool vido_prof_on();
void vido_prof_add(const char* name, double ms);
struct VidoProfScope {
    const char* name; hipStream_t st; bool sync; std::chrono::steady_clock::time_point t0;
    VidoProfScope(const char* n, hipStream_t s = nullptr, bool sy = false) : name(n), st(s), sync(sy) { if (vido_prof_on()) t0 = std::chrono::steady_clock::now(); }
    ~VidoProfScope() { if (!vido_prof_on()) return; if (sync) (void)hipStreamSynchronize(st); vido_prof_add(name, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count()); }
};

#define HIP_TRY(ctx, expr)                                                                  \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess)                                                               \
            return vido_set_error((ctx), VIDO_E_HIP, "%s failed: %s (%s:%d)", #expr,       \
                                  hipGetErrorString(_e), __FILE__, __LINE__);               \
    } while (0)

int orb_state_create(vido_ctx* ctx);
// extractor split used by the fused front end (track.hip): enqueue everything, then wait + check (+ mirror the rows)
int orb_enqueue(vido_ctx* ctx, const uint8_t* imgs, int on_device, int nf, size_t frame_stride, int stride, int width, int height);
int orb_collect(vido_ctx* ctx, int nf, int copy);
int orb_mirror_async(vido_ctx* ctx, int nf);
struct OrbView { const vido_keypoint* d_kpf; const int* d_nkp; int row_cap; const vido_keypoint* h_kpf; const uint8_t* h_descf; const int* h_frame_beg; };
OrbView orb_view(vido_ctx* ctx);
int orb_frame_planes(vido_ctx* ctx, int frame, const uint8_t** pyr, const uint8_t** blur, PyrDev* P);      // (orb.hip) for patchpts.hip, patchsearch.hip, patchrefine.hip: 0 = frame outside the batch
void track_state_destroy(vido_ctx* ctx);
int track_slot_maps(vido_ctx* ctx, int slot, float** depth, float** flow, int32_t** mask, int* W, int* H);      // (track.hip) for maskprop.hip, maskcc.hip
void maskprop_state_destroy(vido_ctx* ctx);
void maskassoc_state_destroy(vido_ctx* ctx);
void maskcc_state_destroy(vido_ctx* ctx);
void ham_state_destroy(vido_ctx* ctx);
void hamwin_state_destroy(vido_ctx* ctx);
void disflow_state_destroy(vido_ctx* ctx);
void stereo_state_destroy(vido_ctx* ctx);
void stereofilter_state_destroy(vido_ctx* ctx);
// (flowcheck.hip) for disflow.hip's vido_dis_flow_pair: the parameter rules of the check (0 = fine), and its memset + launch on device pointers
int flowcheck_params(vido_ctx* ctx, const char* who, int alpha_q10, int beta_q16);
hipError_t flowcheck_enqueue(hipStream_t st, const int32_t* fwd, const int32_t* bwd, int H, int W, int alpha_q10, int beta_q16, uint8_t* status, float* marked, int32_t* stats);
void pose_state_destroy(vido_ctx* ctx);
void ba_state_destroy(vido_ctx* ctx);
// device-resident inputs of the local-window solve (bawin.hip assembles them, ba.hip solves): observations sorted by camera, landmark-major slot tables, points (in / out)
struct BaDevInputs { int no, n_ptl, kcap; const int *obs_cam, *obs_pt, *obs_pos, *pt_start, *slot_cam; const double* obs_meas; double* pt; };
int ba_run_device_inputs(vido_ctx* ctx, vido_ba_problem* prob, vido_ba_result* res, const BaDevInputs* DI);
void bawin_state_destroy(vido_ctx* ctx);
void net_state_destroy(vido_ctx* ctx);
void pnp_state_destroy(vido_ctx* ctx);
void orb_state_destroy(vido_ctx* ctx);
