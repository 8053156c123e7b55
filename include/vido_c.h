/* vido_c.h — the C-ABI drop-in boundary of the MI355X-native VIDO-SLAM hot path.
 *
 * Everything behind this header is hand-written HIP for gfx950 (libvido_slam_hip.so).  There is NO
 * CPU fallback: every entry point returns VIDO_E_NO_DEVICE / VIDO_E_HIP when the GPU path cannot run.
 * Plain C types, caller-owned buffers, int status (0 = ok, <0 = VIDO_E_*), no exceptions, no exit().
 * One vido_ctx = one HIP stream + one device arena; a ctx is not thread-safe; several ctxs may coexist.
 *
 * Each entry point names the reference interface it replaces (paths relative to the reference root):
 *   vido_orb_extract*      ORBextractor::operator()            vido_slam/include/ORBextractor.h:49,  src/ORBextractor.cc:1034-1105
 *   vido_hamming_match*    (no reference call site; north_star-defined brute-force matcher)
 *   vido_frame_features*   Frame::Frame RGB-D ctor             vido_slam/src/Frame.cc:36-241 (+ depth pre-scale Tracking.cc:299-322)
 *   vido_pose_opt_*        Optimizer::PoseOptimization{New,Flow2Cam,ObjMot,Flow2}   vido_slam/include/Optimizer.h:26-29
 *   vido_local_ba          Optimizer::PartialBatchOptimization vido_slam/include/Optimizer.h:31, src/Optimizer.cc:43-1228
 *   vido_global_ba         Optimizer::FullBatchOptimization    vido_slam/include/Optimizer.h:30, src/Optimizer.cc:1235-2178
 * The C++ facade (headers under include/vido_slam/) re-exports the reference's VIDO_SLAM::System/Tracking/Optimizer
 * class surface on top of these calls; INTEGRATION.md shows the binding a maintainer adds.
 */
#ifndef VIDO_C_H
#define VIDO_C_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VIDO_OK              0
#define VIDO_E_INVALID      -1   /* bad argument / size beyond what the ctx was created for */
#define VIDO_E_NO_DEVICE    -2   /* no gfx950 device visible: the product never falls back to the CPU */
#define VIDO_E_HIP          -3   /* a HIP runtime call failed; see vido_last_error */
#define VIDO_E_CAPACITY     -4   /* an internal fixed-capacity buffer overflowed (see message) */
#define VIDO_E_NOMEM        -5

#define VIDO_MAX_LEVELS 16

typedef struct vido_ctx vido_ctx;

/* cv::KeyPoint fields the reference reads (pt, size, angle, response, octave). */
typedef struct vido_keypoint { float x, y, size, angle, response; int32_t octave; } vido_keypoint;

typedef struct vido_config {
    int32_t device;            /* HIP device ordinal */
    int32_t width, height;     /* frame size the arena is laid out for */
    int32_t max_batch;         /* frames in flight per *_batch call (>=1) */
    /* ORBextractor ctor arguments (ORBextractor.h:39-40); YAML keys ORBextractor.* (Tracking.cc:137-141) */
    int32_t n_features; float scale_factor; int32_t n_levels; int32_t ini_th_fast; int32_t min_th_fast;
    int32_t compute_descriptors;   /* 1: blur + rBRIEF (north_star); 0: reference behaviour (call commented out) */
    int32_t host_threads;      /* unused since the quadtree stage moved to the device (kept for ABI stability) */
} vido_config;

void        vido_config_default(vido_config* cfg);           /* 640x480, batch 1, KAIST ORB params */
int         vido_create(const vido_config* cfg, vido_ctx** out);
void        vido_destroy(vido_ctx* ctx);
const char* vido_last_error(const vido_ctx* ctx);            /* valid until the next call on ctx (NULL ctx: global create error) */
int         vido_device_name(const vido_ctx* ctx, char* buf, int buflen);
void*       vido_stream(vido_ctx* ctx);                      /* the ctx's hipStream_t (for callers that enqueue device work) */
int         vido_synchronize(vido_ctx* ctx);
/* Network ops called with on_device != 0 enqueue on `hip_stream` (a caller-owned hipStream_t, e.g. torch's current
 * stream; NULL = the legacy default stream) while enable != 0; enable == 0 restores the ctx stream. */
int         vido_set_stream(vido_ctx* ctx, void* hip_stream, int enable);
/* The ctx's own stream waits (on the device) for `hip_event` (a hipEvent_t the producer recorded on its stream): how device buffers written by another stream — the
 * network nodes' — are handed to the tracker without a host-side wait. */
int         vido_stream_wait_event(vido_ctx* ctx, void* hip_event);

/* ---- ORB ---------------------------------------------------------------------------------------
 * Single frame, host buffers (what ORBextractor::operator() is handed): gray CV_8UC1 `stride` bytes/row.
 * kp_out[max_kp], desc_out[max_kp*32] (may be NULL); *n_out = number of keypoints.
 * Keypoints come out in the reference's order: level 0..L-1, within a level the quadtree list order. */
int vido_orb_extract(vido_ctx* ctx, const uint8_t* gray, int stride, int width, int height,
                     vido_keypoint* kp_out, int max_kp, int* n_out, uint8_t* desc_out);

/* Batch of n_frames (<= max_batch) frames.  `imgs` is a DEVICE pointer when on_device!=0 (frames
 * `frame_stride` bytes apart, rows `stride` bytes apart), else a host pointer.  Outputs are host
 * arrays: kp_out[n_frames*max_kp], desc_out[n_frames*max_kp*32] (NULL ok), n_out[n_frames]. */
int vido_orb_extract_batch(vido_ctx* ctx, const uint8_t* imgs, int on_device, int n_frames,
                           size_t frame_stride, int stride, int width, int height,
                           vido_keypoint* kp_out, int max_kp, int* n_out, uint8_t* desc_out);

/* cvtColor(BGR|RGB|BGRA|RGBA -> GRAY) + ORBextractor::operator() in one stream of launches: what Tracking::GrabImageRGBD does with the
 * caller's colour image before the Frame is built (Tracking.cc:327-340: cvtColor(mImGray, mImGray, CV_RGB2GRAY / CV_BGR2GRAY / ...A2GRAY),
 * then Frame.cc:62 ExtractORB).  img: n_frames interleaved u8 images, `channels` (3 or 4) bytes per pixel, rows `stride` bytes apart;
 * rgb_order != 0: the first channel is red (Camera.RGB: 1).  gray_out (may be NULL): tight width*height bytes per frame, in the same memory
 * space as img (host pointer when on_device == 0, device pointer otherwise) — the mImGray the reference keeps.  Other arguments as
 * vido_orb_extract_batch.  The converted image is written straight into level 0 of the pyramid (no host pass over the pixels). */
int vido_orb_extract_color(vido_ctx* ctx, const uint8_t* img, int channels, int rgb_order, int on_device, int n_frames,
                           size_t frame_stride, int stride, int width, int height, uint8_t* gray_out,
                           vido_keypoint* kp_out, int max_kp, int* n_out, uint8_t* desc_out);

/* Diagnostics for the parity tests: copy pyramid level `level` (tight lw*lh bytes) of frame `frame` of the
 * last extract call back to the host; blurred!=0 selects the 7x7-blurred copy. */
/* enqueue the extraction of a device-resident colour frame and return; the next vido_orb_extract_color call for the same pointer and size only collects (csrc/orb.hip) */
int vido_orb_prefetch_color(vido_ctx* ctx, const uint8_t* img_dev, int channels, int rgb_order, int stride, int width, int height, void* ready_event);
int vido_orb_level_size(const vido_ctx* ctx, int level, int* lw, int* lh);
int vido_orb_read_level(vido_ctx* ctx, int frame, int level, int blurred, uint8_t* out);
/* FAST candidates of the last call for (frame, level) in reference order: packed x | y<<12 | score<<24
 * (level coordinates).  Returns count (or <0). */
int vido_orb_read_candidates(vido_ctx* ctx, int frame, int level, uint32_t* out, int cap);
/* Which kernel forms the context's tables (built at creation from the frame size) select; reads the tables only: nothing is launched, no state changes.
 * out: [0] n_levels [1] tiles of the single-launch pyramid (0: no tile launch — one level, or the per-level resize chain) [2] [3] its tile grid NX, NY (0 0: none laid out)
 * [4] interior width of the FAST strip kernel's instantiation (37 or 74) [5] rows a FAST strip holds [6] widest FAST cell interior [7] FAST strips per frame
 * [8] FAST cells per frame [9] blur strips per frame [10] most blur strips in one row of any level [11] candidate slots per frame */
int vido_orb_geometry(const vido_ctx* ctx, int32_t out[12]);
/* per-stage time of the last batch call (HIP events on the ctx stream), ms: [0] pyramid (level-0 copy + resize
 * launches) [1] k_fast_cells alone [2] device quadtree + keypoint list [3] blur [4] orient/rBRIEF
 * [5] total wall [6] scan+gather [7] number of FAST candidates in the batch */
int vido_orb_last_timing(const vido_ctx* ctx, float ms[8]);

/* Orientation, rBRIEF descriptor and Hamming distance at CALLER-GIVEN points (not detected keypoints) of pyramid slab `frame`: the slab of the most recent extraction or
 * prefetch of that frame index of the context (no reference call site: the reference never evaluates a descriptor away from a keypoint; defined by the oracle's per-point
 * vo_ic_angle / vo_brief on the build's own pyramid).  xyl [n*3]: x, y in LEVEL coordinates (integer pixels of that pyramid level), level.  For point i: angle_out[i] is the
 * intensity-centroid angle over the radius-15 disc of the unblurred level and desc_out[32 i ..] the steered rBRIEF on the blurred level, both exactly what the extractor
 * computes for a keypoint at that pixel; dist_out[i] = Hamming distance between that descriptor and ref_desc[32 i ..], computed in the same launch.  Any output may be NULL
 * (dist_out needs ref_desc: VIDO_E_INVALID without).  A point closer than 19 px (the extractor's edge margin) to a border of its level, or with a level outside
 * [0, n_levels), is INVALID: angle -1, zero descriptor, distance -1, and nothing is read for it.  n == 0 is a successful no-op.  on_device != 0: every pointer is a device
 * pointer (descriptors 4-byte aligned) and the call only enqueues on the ctx stream; otherwise it returns when the results are in the caller's arrays.  Results depend
 * neither on n nor on the order of the points.  Needs compute_descriptors != 0 for desc_out / dist_out (the blurred pyramid). */
int vido_orb_describe_points(vido_ctx* ctx, int frame, const int32_t* xyl, int n, const uint8_t* ref_desc, float* angle_out, uint8_t* desc_out, int32_t* dist_out, int on_device);

/* The 8 x 8 grey patch at CALLER-GIVEN points of pyramid slab `frame`, and its zero-mean normalised cross-correlation with a caller-given reference patch as an integer
 * verdict (no reference call site; defined by tests/refimpl/patch_points_np.py, exact to the bit).  xyl [n*3] as for vido_orb_describe_points; blurred != 0 reads the
 * blurred pyramid (needs compute_descriptors != 0), 0 the unblurred one.  The patch of point i is rows y-4 .. y+3, columns x-4 .. x+3 of its level, row-major, 64 bytes at
 * patch_out[64 i ..].  With a = ref_patch[64 i ..], b = that patch, S1 = sum a, S2 = sum b, S11 = sum a^2, S22 = sum b^2, S12 = sum a b:
 *   sums_out[3 i ..] = cov, var_ref, var_cur = 64 S12 - S1 S2, 64 S11 - S1^2, 64 S22 - S2^2          (each fits i32: at most 66 585 600)
 *   status_out[i]    = 2 (no texture) if var_ref < min_var or var_cur < min_var; else 0 (accepted) iff cov > 0 and cov^2 * 1024^2 >= min_zncc_q10^2 * var_ref * var_cur,
 *                      compared as exact 128-bit integers (no float, no square root, no division: equality accepts); else 1 (rejected).
 * A point whose level is outside [0, n_levels) or whose patch is not wholly inside its level (x < 4, x + 3 >= w, likewise y) is INVALID: status -1, sums 0 0 0, zero
 * patch, and nothing is read for it.  Any output may be NULL; sums_out / status_out need ref_patch, min_var >= 0 and 0 <= min_zncc_q10 <= 1024 (VIDO_E_INVALID otherwise).
 * n == 0 is a successful no-op.  on_device != 0: every pointer is a device pointer (4-byte aligned) and the call only enqueues on the ctx stream; otherwise it returns
 * when the results are in the caller's arrays.  Results depend neither on n nor on the order of the points. */
int vido_orb_patch_points(vido_ctx* ctx, int frame, const int32_t* xyl, int n, int blurred, const uint8_t* ref_patch, int min_var, int min_zncc_q10,
                          uint8_t* patch_out, int32_t* sums_out, int32_t* status_out, int on_device);

/* The offset inside a square window at which the 8 x 8 patch of pyramid slab `frame` correlates best with a caller-given reference patch, the runner-up outside the
 * winner's own peak, and an integer verdict (no reference call site; defined by tests/refimpl/patch_search_np.py, exact to the bit).  xyl [n*3], blurred, the patch, the
 * three sums and "wholly inside the level" as for vido_orb_patch_points; a = ref_patch[64 i ..] (required).  0 <= radius <= 16, 1 <= excl <= 16, min_var >= 0,
 * 0 <= min_zncc_q10 <= 1024, 0 <= peak_ratio_q10 <= 1024 (0: no peak test); VIDO_E_INVALID otherwise.  In the order the rules apply, per point:
 *   candidates  the offsets (dx, dy), |dx| <= radius, |dy| <= radius, whose patch at (x + dx, y + dy) lies wholly inside the level
 *   status -1   level outside [0, n_levels) or no candidate: every output of the point is 0
 *   status  2   var_ref < min_var: nothing is searched; sums = 0, var_ref, 0 and the rest 0.  A point of status -1 or 2 reads nothing of the slab
 *   eligible    a candidate with var_cur >= min_var and cov > 0
 *   order       p before q iff cov_p^2 var_q > cov_q^2 var_p (exact 128-bit integers: ZNCC^2 without a division); on equality the smaller dx^2 + dy^2, then the
 *               smaller dy, then the smaller dx
 *   best        the first eligible candidate in that order; none: status 1, dxy = 0, sums = 0, var_ref, 0, second = 0
 *   dxy_out[2 i ..] = dx, dy of the best; sums_out[3 i ..] = its cov, var_ref, var_cur
 *   second_out[2 i ..] = cov, var_cur of the first eligible candidate in that order with max(|dx - dx1|, |dy - dy1|) > excl, 0 0 if there is none (reported whenever
 *               there is a best, whatever the status)
 *   status  1   the best fails cov^2 * 1024^2 >= min_zncc_q10^2 * var_ref * var_cur (equality accepts)
 *   status  3   else, with peak_ratio_q10 > 0 and a second: cov2^2 * var1 * 1024^2 > peak_ratio_q10^2 * cov1^2 * var2 (ZNCC2 > r ZNCC1: ambiguous)
 *   status  0   otherwise: found
 * stats_out[0..3] count the statuses 0..3 of this call, stats_out[4] status -1.  Any output may be NULL; every element of a given output is written.  n == 0 is a
 * successful no-op that zeroes stats_out.  on_device != 0: every pointer is a device pointer (4-byte aligned) and the call only enqueues on the ctx stream; otherwise it
 * returns when the results are in the caller's arrays.  Results depend neither on n nor on the order of the points. */
int vido_orb_patch_search(vido_ctx* ctx, int frame, const int32_t* xyl, int n, int blurred, const uint8_t* ref_patch, int radius, int excl, int min_var, int min_zncc_q10,
                          int peak_ratio_q10, int32_t* dxy_out, int32_t* sums_out, int32_t* second_out, int32_t* status_out, int32_t* stats_out, int on_device);

/* Sub-pixel alignment of a caller-given 8 x 8 reference patch to pyramid slab `frame` around CALLER-GIVEN points: translation-only inverse-compositional Gauss-Newton with a
 * bias term, to 1/256 px and entirely in integers (no reference call site; defined by tests/refimpl/patch_refine_np.py, exact to the bit).  xyl [n*3], blurred and
 * T = ref_patch[64 i ..] (required; T[r][c] belongs to level pixel (x - 4 + c, y - 4 + r)) as for vido_orb_patch_search.  Only the 36 interior pixels r, c in 1..6 are
 * compared (N = 36); the border ring serves the template's gradients.  1 <= iters <= 8, 0 <= max_shift_q8 <= 512 (1/256 px), min_eig >= 0; VIDO_E_INVALID otherwise.
 * In the order the rules apply, per point:
 *   status -1   level outside [0, n_levels), or not (x - 3 - C >= 0 and x + 3 + C <= w - 1 and the same in y), C = (max_shift_q8 + 255) >> 8: every output of the point is
 *               0 and nothing is read for it.  Otherwise the footprint is inside the level for every admissible offset
 *   gradients   gx = T[r][c+1] - T[r][c-1], gy = T[r+1][c] - T[r-1][c]
 *   Hessian     Hxx = N sum gx^2 - (sum gx)^2, Hyy = N sum gy^2 - (sum gy)^2, Hxy = N sum gx gy - sum gx sum gy, det = Hxx Hyy - Hxy^2, tr = Hxx + Hyy
 *   status  2   det <= 0 or tr < 2 min_eig or det - min_eig tr + min_eig^2 < 0 (smaller eigenvalue of H below min_eig: no texture, or an edge only): outputs 0
 *   evaluation  at offset p = (px, py): X = (x - 4 + c) 256 + px, ix = X >> 8, fx = X & 255 (Y likewise),
 *               I = (256 - fx)(256 - fy) L[iy][ix] + fx (256 - fy) L[iy][ix+1] + (256 - fx) fy L[iy+1][ix] + fx fy L[iy+1][ix+1], e = (I - 65536 T[r][c] + 128) >> 8,
 *               cost = N sum e^2 - (sum e)^2, bx = N sum gx e - sum gx sum e, by likewise
 *   step        numx = Hyy bx - Hxy by, numy = Hxx by - Hxy bx, d = rdiv(-2 num, det) per axis, clamped to +-256; rdiv rounds to the nearest, halves away from zero
 *   loop        p = (0, 0); at most iters times: step; d = (0, 0) stops; p += d; |px| or |py| > max_shift_q8: status 3, q8 = 0, cost = cost0, cost0; else the cost is
 *               evaluated at the new p
 *   status  0   q8_out[2 i ..] = the iterate of the smallest cost (the earliest on ties), cost_out[2 i ..] = cost at (0, 0), cost at q8
 *   iters_out[i] = the number of steps taken (the one that left the window included)
 * stats_out[0..3] count the statuses 0, 2, 3, -1 of this call.  Every intermediate fits int64 (|2 num| < 2^62.7).  Any output may be NULL; every element of a given output
 * is written.  n == 0 is a successful no-op that zeroes stats_out.  on_device != 0: every pointer is a device pointer (4-byte aligned, cost_out 8-byte) and the call only
 * enqueues on the ctx stream; otherwise it returns when the results are in the caller's arrays.  Results depend neither on n nor on the order of the points. */
int vido_orb_patch_refine(vido_ctx* ctx, int frame, const int32_t* xyl, int n, int blurred, const uint8_t* ref_patch, int iters, int max_shift_q8, int min_eig, int32_t* q8_out,
                          int64_t* cost_out, int32_t* iters_out, int32_t* status_out, int32_t* stats_out, int on_device);

/* Dense optical flow of the Dense Inverse Search kind from img0 to img1, two u8 images of one size, to 1/256 px and entirely in integers (no reference call site; defined by
 * tests/refimpl/dis_flow_np.py, exact to the bit).  16 <= width, height <= 4095; channels 1, 3 or 4 (interleaved; rgb_order as in vido_orb_extract_color), stride in bytes
 * >= width * channels; 0 <= coarsest <= 6 with min(width, height) >> coarsest >= 8; 1 <= iters <= 16; 0 <= max_shift_q8 <= 2048 (1/256 px); min_eig >= 0; VIDO_E_INVALID
 * otherwise, and when all three outputs are NULL.  Needs no extractor state and not the context's configured frame size.  In the order the rules apply:
 *   grey        1 channel: the bytes; else (1868 B + 9617 G + 4899 R + 8192) >> 14
 *   pyramid     levels 0 .. coarsest of both images, w[l+1] = w[l] >> 1, h likewise, G[l+1][y][x] = (sum of the 2 x 2 block + 2) >> 2
 *   flow        U[l][y][x] = (ux, uy) in 1/256 px of level l, from level coarsest down to 0; the initial field is 0 at the coarsest level and
 *               2 U[l+1][min(y >> 1, h[l+1] - 1)][min(x >> 1, w[l+1] - 1)] below
 *   patches     8 x 8, origins 0, 4, 8, ... while o + 8 <= n along an axis of length n, plus n - 8 when that is not among them; u0 = the initial field at (x0 + 4, y0 + 4)
 *   template    N = 64; T = the patch of image 0, gx = G0[y][min(x+1, w-1)] - G0[y][max(x-1, 0)], gy likewise; Hxx = N sum gx^2 - (sum gx)^2, Hyy, Hxy likewise,
 *               det = Hxx Hyy - Hxy^2, tr = Hxx + Hyy; flat (keeps u0) when det <= 0 or tr < 2 min_eig or det - min_eig tr + min_eig^2 < 0
 *   sample      S(X, Y) of image 1 at 1/256 px: X clamped to [0, (w-1) 256], ix = X >> 8, fx = X & 255, right neighbour min(ix+1, w-1), y likewise; bilinear, weights sum 65536
 *   evaluation  at u: e = (S((x0+c) 256 + ux, (y0+r) 256 + uy) - 65536 T[r][c] + 2048) >> 12 (1/16 grey), cost = N sum e^2 - (sum e)^2, bx = N sum gx e - sum gx sum e, by likewise
 *   step        d = rdiv(-32 (Hyy bx - Hxy by), det), rdiv(-32 (Hxx by - Hxy bx), det), each clamped to +-256; rdiv rounds to the nearest, halves away from zero
 *   loop        u = u0; at most iters times: step; d = (0, 0) stops; u += d; max(|ux - u0x|, |uy - u0y|) > max_shift_q8: rejected (keeps u0); else the cost is evaluated at
 *               the new u.  The iterate of the smallest cost wins, the earliest on ties
 *   densify     pixel (x, y) of level l over every patch p that holds it: d = |S(x 256 + u_p.x, y 256 + u_p.y) - 65536 G0[y][x]| >> 16, wgt = 65536 / max(1, d) (integer),
 *               U = rdiv(sum wgt u_p.x, sum wgt), rdiv(sum wgt u_p.y, sum wgt)
 * q8_out [h*w*2] = U[0]; flow_out [h*w*2] = q8 / 256 in pixels (dx, dy; exact); stats [4], summed over the levels: patches that kept an iterate, flat patches, rejected
 * patches, steps taken.  Every intermediate fits int64 (H < 2^28, |b| < 2^32, |2 num| < 2^62, cost < 2^36; the step's division is taken in two parts).  Any output may be
 * NULL, not all.  on_device != 0: every pointer is a device pointer (outputs 4-byte aligned) and the call only enqueues on the ctx stream (vido_set_stream's when one is
 * set): no host synchronisation, so a call can sit inside a stream capture — except the first call of a size, which grows the context's scratch (the two pyramids, the
 * fields of the levels above 0, one level's patch flows).  Otherwise the images and outputs are the caller's host arrays, staged through pinned buffers that grow on demand,
 * and the call returns when the results are there.  A result depends on nothing but the two images and the parameters. */
int vido_dis_flow(vido_ctx* ctx, const uint8_t* img0, const uint8_t* img1, int channels, int rgb_order, int stride, int width, int height,
                  int coarsest, int iters, int max_shift_q8, int min_eig,
                  float* flow_out /* [h*w*2], NULL ok */, int32_t* q8_out /* [h*w*2], NULL ok */, int32_t* stats /* [4], NULL ok */, int on_device);

/* Forward-backward check of two dense flow fields, entirely in integers (no reference call site; defined by tests/refimpl/flow_consistency_np.py, exact to the bit).
 * fwd_q8, bwd_q8 [H*W*2] (dx, dy) in 1/256 px: the flow of image 0 -> 1 on image 0's grid and of image 1 -> 0 on image 1's grid, the layout of vido_dis_flow's q8.
 * 1 <= H, W <= 4095; 0 <= alpha_q10 <= 1024 (alpha = alpha_q10 / 1024); 0 <= beta_q16 <= 2^30 (beta = beta_q16 / 65536 px^2); VIDO_E_INVALID otherwise, for a NULL
 * field and when all three outputs are NULL.  Needs no other state of the context.  For pixel (x, y) with f = fwd[y][x], in the order the rules apply:
 *   status 3    not a flow: |f.x| or |f.y| >= 2^19
 *   status 2    leaves the image: tx = 256 x + f.x, ty = 256 y + f.y; tx < 0, tx > 256 (W - 1), ty < 0 or ty > 256 (H - 1)
 *   taps        x0 = tx >> 8, ax = tx & 255, x1 = min(x0 + 1, W - 1), y likewise; bwd[y0][x0], bwd[y0][x1], bwd[y1][x0], bwd[y1][x1], all four also where a weight is 0;
 *               status 3 when a component of one of them has |.| >= 2^19
 *   b           s = (256-ax)(256-ay) B[y0][x0] + ax (256-ay) B[y0][x1] + (256-ax) ay B[y1][x0] + ax ay B[y1][x1] per component, b = (s + 32768) >> 16 (arithmetic shift)
 *   r           r = f + b
 *   status 1    inconsistent: 1024 |r|^2 > alpha_q10 (|f|^2 + |b|^2) + 1024 beta_q16 (squares summed over both components); else status 0
 * status_out [H*W] = the status; flow_marked_out [H*W*2] = f / 256 in pixels (exact) where the status is 0, elsewhere the quiet NaN with bits 0x7FC00000 on both
 * components — the front end drops such a vector by failing comparisons, and vido_mask_propagate defines a NaN source as not voting; stats_out [4] = the count of each
 * status (zeroed by the call).  Bounds: |f|, |tap| < 2^19, |s| < 2^35, |b| < 2^19, |r| < 2^20; 1024 |r|^2 < 2^51, alpha_q10 (|f|^2 + |b|^2) < 2^50, 1024 beta_q16 <= 2^40:
 * every term stays below 2^52.  Any output may be NULL, not all.  on_device != 0: every pointer is a device pointer (the fields and flow_marked_out 8-byte aligned,
 * stats_out 4-byte) and the call only enqueues on the ctx stream (vido_set_stream's when one is set): a memset of the counters and one launch, no host synchronisation,
 * so it can sit inside a stream capture.  Otherwise the arrays are the caller's host arrays, staged through pinned buffers that grow on demand, and the call returns when
 * the results are there.  A result depends on nothing but the two fields and the two parameters. */
int vido_flow_consistency(vido_ctx* ctx, const int32_t* fwd_q8, const int32_t* bwd_q8, int H, int W, int alpha_q10, int beta_q16,
                          uint8_t* status_out /* [H*W], NULL ok */, float* flow_marked_out /* [H*W*2], NULL ok */, int32_t* stats_out /* [4], NULL ok */, int on_device);

/* vido_dis_flow in both directions from one ingest and one pyramid build, and vido_flow_consistency of the two fields.  Arguments and their limits as in those two calls.
 * All bit for bit: fwd_q8_out = vido_dis_flow(img0, img1)'s q8, bwd_q8_out = vido_dis_flow(img1, img0)'s q8, stats_out[0..3] and [4..7] = those two calls' stats,
 * and flow_out (the MARKED flow), status_out and stats_out[8..11] = vido_flow_consistency(fwd, bwd, alpha_q10, beta_q16)'s outputs.  Any output may be NULL, not all.
 * At every level both directions run in one k_dis_patch and one k_dis_densify launch (the direction is a grid dimension), so the call has vido_dis_flow's launches plus
 * the check's.  on_device != 0: device pointers (flow_out and the q8 outputs 8-byte aligned, stats_out 4-byte), the call only enqueues on the ctx stream — except the
 * first call of a size, which grows the scratch it shares with vido_dis_flow (the second direction's per-level fields and patch flows, and both level-0 fields). */
int vido_dis_flow_pair(vido_ctx* ctx, const uint8_t* img0, const uint8_t* img1, int channels, int rgb_order, int stride, int width, int height,
                       int coarsest, int iters, int max_shift_q8, int min_eig, int alpha_q10, int beta_q16,
                       float* flow_out /* [h*w*2] marked, NULL ok */, int32_t* fwd_q8_out /* [h*w*2], NULL ok */, int32_t* bwd_q8_out /* [h*w*2], NULL ok */,
                       uint8_t* status_out /* [h*w], NULL ok */, int32_t* stats_out /* [12]: forward 4, backward 4, check 4; NULL ok */, int on_device);

/* Semi-global stereo matching of a rectified pair: the disparity of every pixel of `left` against `right` to 1/16 px, entirely in integers (the reference receives such a
 * disparity from outside, Tracking.cc:305-309; defined by tests/refimpl/stereo_sgm_np.py, exact to the bit).  16 <= width, height <= 4095; channels, rgb_order and stride
 * as in vido_dis_flow; D = max_disp a multiple of 16 with 16 <= D <= 256 and width * height * D <= 2^28; 0 <= p1 <= p2 <= 1000; 0 <= uniqueness <= 99; 0 <= lr_tol <= 255;
 * VIDO_E_INVALID otherwise, for a NULL image and when all four outputs are NULL.  Needs no extractor state and not the context's configured frame size.  In the order the
 * rules apply:
 *   grey        1 channel: the bytes; else (1868 B + 9617 G + 4899 R + 8192) >> 14
 *   census      window 9 wide x 7 high around the pixel, coordinates clamped to the image; the 62 neighbours row-major, the centre skipped; bit = neighbour < centre:
 *               a 64-bit word cL / cR per pixel of each image
 *   cost        C(x, y, d) = popcount(cL(x, y) ^ cR(x - d, y)) for 0 <= d < D and x - d >= 0; C = 64 where x - d < 0
 *   paths       eight directions r = (+-1, 0), (0, +-1), (+-1, +-1).  L_r(p, d) = C(p, d) at every pixel whose predecessor p - r lies outside the image (diagonal paths
 *               restart at the side columns).  Elsewhere, with m = min_k L_r(p - r, k): L_r(p, d) = C(p, d) + min(L_r(p - r, d), L_r(p - r, d - 1) + p1,
 *               L_r(p - r, d + 1) + p1, m + p2) - m; a d +- 1 outside [0, D) is no candidate.  S = sum_r L_r.  L <= 64 + p2 <= 1064, S <= 8512
 *   winner      d0 = argmin_d S(x, y, d), the lowest d on ties; s0 = S(d0)
 *   right view  dR(x, y) = argmin_d S(x + d, y, d) over the d with x + d <= width - 1, the lowest d on ties
 *   sub-pixel   sm = S(d0 - 1), sp = S(d0 + 1), den = sm + sp - 2 s0; off = rdiv(8 (sm - sp), den) when 1 <= d0 <= D - 2 and den > 0, else 0 (rdiv as in
 *               vido_dis_flow: to the nearest, halves away from zero; |off| <= 8); q4 = 16 d0 + off, in 1/16 px
 *   status      2 (left-right) x - d0 < 0 or |dR(x - d0, y) - d0| > lr_tol; else 1 (not unique) (100 - uniqueness) S2 <= 100 s0, S2 = min S(d) over |d - d0| > 1;
 *               else 3 (zero disparity) q4 <= 0; else 0
 * q4_out [h*w] = q4 of every pixel, whatever its status; disp_out [h*w] = q4 / 16 in pixels (exact) where the status is 0, -1 elsewhere (vido_frame_upload turns a
 * negative raw depth into 0 and the lists drop depth 0: the front end's own "no depth"); status_out [h*w]; stats_out [4] = the count of each status (zeroed by the call).
 * With the KITTI ChooseData code, DepthMapFactor 1 and Camera.bf = fx * baseline, the front end turns disp_out into metres as it does a KITTI disparity image
 * (bf / (raw / DepthMapFactor)).  Any output may be NULL, not all.  on_device != 0: every pointer is a device pointer (disp_out, q4_out and stats_out 4-byte aligned) and
 * the call only enqueues on the ctx stream (vido_set_stream's when one is set): five launches, no host synchronisation, so a call can sit inside a stream
 * capture — except the first call of a size, which grows the op's own scratch (two grey planes, two census planes and the u16 S volume; shared with no other op).
 * Otherwise the images and outputs are the caller's host arrays, staged through pinned buffers that grow on demand, and the call returns when the results are there.
 * A result depends on nothing but the two images and the five parameters: the eight paths add into S with integer atomics, whose sums do not depend on the order. */
int vido_stereo_sgm(vido_ctx* ctx, const uint8_t* left, const uint8_t* right, int channels, int rgb_order, int stride, int width, int height,
                    int max_disp, int p1, int p2, int uniqueness, int lr_tol,
                    float* disp_out /* [h*w], NULL ok */, int32_t* q4_out /* [h*w], NULL ok */, uint8_t* status_out /* [h*w], NULL ok */,
                    int32_t* stats_out /* [4], NULL ok */, int on_device);

/* Speckle filter of a disparity image: removes the small islands of valid disparity that semi-global matching leaves at occlusion edges, and makes the depth plane that
 * vido_mask_propagate takes for its collisions (defined by tests/refimpl/stereo_filter_np.py, exact to the bit; no reference counterpart).  q4 / status: vido_stereo_sgm's
 * q4_out / status_out, or any images of that form.  1 <= width, height <= 4095; 0 <= max_diff_q4 <= 65535; 1 <= min_region <= 2^24; bf finite and > 0 when depth_out is
 * given (ignored otherwise); VIDO_E_INVALID otherwise, for a NULL input, when all three image outputs and stats_out are NULL, for a status_out that overlaps status
 * without being it, and for a misaligned device output.  Needs no other state of the context and not its configured frame size.  In the order the rules apply:
 *   valid       status == 0 and 1 <= q4 <= 65535.  A status-0 pixel with q4 outside that range gets status_out = 3 (vido_stereo_sgm gives such a pixel status 3 itself);
 *               every other input status, values above 3 included, is copied through and is not valid
 *   edge        two 4-neighbours (left / right, up / down), both valid, with |q4a - q4b| <= max_diff_q4
 *   region      a connected component of the valid pixels under these edges; its area is its pixel count.  The relation is NOT transitive: a ramp 16, 32, 48, ... with
 *               max_diff_q4 = 16 is one region whose ends differ arbitrarily, and two pixels may share a region through a detour only
 *   speckle     a valid pixel whose region has area < min_region gets status_out = 4.  min_region = 1 removes nothing, and the call then launches no labelling
 * status_out [h*w] as above (it may BE status); disp_out [h*w] = q4 / 16 in pixels (exact) where status_out is 0, -1 elsewhere (vido_stereo_sgm's disp_out convention);
 * depth_out [h*w] = bf / disp_out, ONE correctly rounded fp32 division, where status_out is 0, FLT_MAX elsewhere: finite and positive, so vido_mask_propagate still
 * scatters such a source, which loses every collision against a measured depth and falls back to "smaller label" against another unknown; stats_out [4] = valid pixels
 * in, regions removed, pixels removed, valid pixels out (zeroed by a kernel of the call).  Any output may be NULL, not all.  on_device != 0: every pointer is a device
 * pointer (disp_out, depth_out and stats_out 4-byte aligned) and the call only enqueues on the ctx stream (vido_set_stream's when one is set): one launch with
 * min_region = 1, else four (tile labelling in LDS, seam merge, flatten + areas, write), no host synchronisation, so a call can sit inside a stream capture — except the
 * first call of a size, which grows the op's own scratch (two i32 planes: parent and area; shared with no other op).  Otherwise the arrays are the caller's host arrays,
 * staged through pinned buffers that grow on demand, and the call returns when the results are there.  A result depends on nothing but the two images and the three
 * parameters: the labelling uses integer minima and sums only, whose results do not depend on the order. */
int vido_stereo_filter(vido_ctx* ctx, const int32_t* q4 /* [h*w], 1/16 px */, const uint8_t* status /* [h*w] */, int width, int height,
                       int max_diff_q4, int min_region, float bf,
                       float* disp_out /* [h*w], NULL ok */, uint8_t* status_out /* [h*w], NULL ok; may BE status */, float* depth_out /* [h*w], NULL ok */,
                       int32_t* stats_out /* [4], NULL ok */, int on_device);

/* Rectification of one camera image, or of the two of a stereo rig in one launch: dst(u, v) = the bilinear mean of src at the map's entry for (u, v), entirely in integers
 * (defined by tests/refimpl/stereo_rectify_np.py, exact to the bit; no reference counterpart: its datasets come rectified).  The maps are vido_rectify_map's (below), or
 * any int32 [dst_h][dst_w][2] arrays of that form: (mx, my), x first, in 1/256 px of the source.  src: src_w x src_h u8 pixels of 1, 3 or 4 interleaved channels, rows
 * src_stride bytes apart; dst: dst_w x dst_h pixels of the same channels, rows dst_stride bytes apart; both cameras share the sizes, the channels and the strides.
 *   inside      0 <= mx <= (src_w - 1) 256 and 0 <= my <= (src_h - 1) 256
 *   corners     x0 = mx >> 8, ax = mx & 255, x1 = min(x0 + 1, src_w - 1); likewise y0, ay, y1
 *   value       ((256 - ax)(256 - ay) s[y0][x0][c] + ax (256 - ay) s[y0][x1][c] + (256 - ax) ay s[y1][x0][c] + ax ay s[y1][x1][c] + 32768) >> 16 for every channel c alike,
 *               a fourth one included; the sum stays below 2^31
 *   elsewhere   every channel 0.  No source byte is read for a pixel that is not inside, whatever the map holds (INT32_MIN, vido_rectify_map's "no source", included)
 * insideK_out [dst_h*dst_w] = 1 where inside, 0 elsewhere; NULL ok.  src1 NULL: one camera; then map1, dst1 and inside1_out are NULL too.  VIDO_E_INVALID, with no output
 * written, for a NULL src0 / map0 / dst0, for src1, map1, dst1 not all given or all NULL, channels outside {1, 3, 4}, a stride below width * channels, sizes outside
 * 16 .. 4095, a destination (image or inside plane) that overlaps a source image or a map, and device maps that are not 4-byte aligned.  Needs no extractor state and not
 * the context's configured frame size.  on_device != 0: every pointer is a device pointer and the call only enqueues on the ctx stream (vido_set_stream's when one is
 * set): one launch for both cameras, no host synchronisation, no scratch, so a call can sit inside a stream capture from the first call on.  Any byte alignment of the
 * images and any stride work; a thread writes its four pixels in one dword / three dwords / 16 bytes where their address allows it (a 4-byte aligned row; for 4 channels
 * a 16-byte aligned one) and reads their map entries as two 16-byte loads where the entries' address is 16-byte aligned (a 16-byte aligned map of an even dst_w).
 * Otherwise the arrays are the caller's host arrays, staged through pinned buffers that grow on demand (the bytes between the destination's rows are kept), and the call
 * returns when the results are there. */
int vido_rectify(vido_ctx* ctx, const uint8_t* src0, const uint8_t* src1 /* NULL: one camera */, int channels, int src_stride, int src_w, int src_h,
                 const int32_t* map0 /* [dst_h*dst_w*2] */, const int32_t* map1, int dst_w, int dst_h, uint8_t* dst0, uint8_t* dst1, int dst_stride,
                 uint8_t* inside0_out /* [dst_h*dst_w], NULL ok */, uint8_t* inside1_out /* NULL ok */, int on_device);

/* ---- Hamming -------------------------------------------------------------------------------------
 * For each of the na 256-bit descriptors in a: index of the closest descriptor in b (smallest Hamming
 * distance, lowest index on ties) and that distance.  on_device!=0: a, b, idx_out, dist_out are device
 * pointers and the call only enqueues on the ctx stream. */
int vido_hamming_match(vido_ctx* ctx, const uint8_t* a, int na, const uint8_t* b, int nb,
                       int32_t* idx_out, int32_t* dist_out, int on_device);
/* Windowed matcher: for each of the nq queries (256-bit descriptor q_desc[32 i ..], position q_xy[2 i ..] in pixels, pyramid level q_level[i]) the best and second best of
 * the nt train entries (t_desc, t_xy, t_level) inside a spatial window and a level gate, an acceptance verdict, and optionally a one-to-one rule.  No reference call site
 * (as above); bit-exact against tests/refimpl/hamming_window_np.py.
 *   candidates of query i: the train entries j with  fabsf(tx - qx) <= radius && fabsf(ty - qy) <= radius  (one fp32 subtraction and one compare per term: a SQUARE window,
 *             edge included, independent of contraction and evaluation order)  and  level_tol < 0 || |t_level[j] - q_level[i]| <= level_tol.  A NaN or infinite
 *             coordinate fails the window test: such a query has no candidates, such a train entry is nobody's candidate.
 *   best      the candidate with the smallest Hamming distance, lowest j on ties; dist_out[i] = that distance, -1 with no candidate.
 *   second    dist2_out[i] = the smallest distance among the candidates other than the best one (a duplicate descriptor gives dist2 == dist), -1 with fewer than two.
 *   status_out[i], the first test that fires decides:
 *             1  no candidate
 *             2  dist > max_dist
 *             3  the ratio test failed.  It applies only when ratio_num > 0 and dist2 >= 0, and passes iff dist * ratio_den < dist2 * ratio_num (integers).
 *             4  only with unique != 0: among the queries that reached this point with the same best j, the one with the smallest (dist, i) keeps it; the others get 4
 *                (they do not fall back to their second candidate)
 *             0  matched
 *   idx_out[i] = j for status 0, otherwise -1.  stats_out[s] = number of queries with status s (5 x i32; may be NULL).  Every element of every output is written.
 * ratio_num == 0 switches the ratio test off (ratio_den is then ignored); otherwise 0 < ratio_num <= ratio_den <= 1024.  A ratio outside that, a radius that is negative,
 * NaN or infinite, a negative count or a null array with a non-zero count: VIDO_E_INVALID.  nq == 0 is a successful no-op (stats_out, when given, is zeroed); nt == 0
 * gives status 1 everywhere.  Results depend neither on the order in which train entries are processed nor on launch geometry: integer minima and integer sums decide
 * everything (the one-to-one rule is a 64-bit atomic minimum of dist << 32 | i into an owner plane the context owns, then a resolve pass).
 * on_device != 0: every pointer, stats_out included, is a device pointer (4-byte aligned) and the call only enqueues on the ctx stream (two launches, three with unique; no
 * memset); the context's buffers grow on demand, so a first call of the largest size comes before a stream capture.  Otherwise the call returns with the results in the
 * caller's arrays.  One set of buffers per context: calls on one context do not overlap. */
int vido_hamming_match_window(vido_ctx* ctx, const uint8_t* q_desc, const float* q_xy, const int32_t* q_level, int nq,
                              const uint8_t* t_desc, const float* t_xy, const int32_t* t_level, int nt,
                              float radius, int level_tol, int max_dist, int ratio_num, int ratio_den, int unique,
                              int32_t* idx_out, int32_t* dist_out, int32_t* dist2_out, int32_t* status_out, int32_t stats_out[5], int on_device);

/* ---- Tracking front-end, data-parallel stages ---------------------------------------------------------
 * Frame maps (depth f32, flow f32x2, mask i32; width*height of the ctx) live in device "slots"
 * (vido_track_slots() of them, >= 2 so that frame k and k-1 are both resident). */
typedef struct vido_track_params {
    int32_t dataset;            /* YAML ChooseData: 0 OMD (d/f), 1 KITTI (bf/(d/f)), 2 KAIST (scale*bf/(d/f))  Tracking.cc:306-319 */
    float depth_map_factor, bf, kaist_scale;
    float th_depth_bg, th_depth_obj;     /* ThDepthBG / ThDepthOBJ (Frame::mThDepth, mThDepthObj) */
    int32_t dense_step;         /* 4 (Frame.cc:184) */
    float fx, fy, cx, cy;       /* Camera.fx.. (Frame.cc:229-234) */
} vido_track_params;

/* Host-side list outputs of vido_frame_features, [n_frames][max_*] each (caller-owned). */
typedef struct vido_frame_lists {
    int32_t max_stat, max_obj;
    int32_t* n_stat; int32_t* stat_idx; float* stat_corr; float* stat_flow; float* stat_depth;      /* mvStatKeysTmp(idx into kps)/mvCorres/mvFlowNext/mvStatDepthTmp */
    int32_t* n_obj; float* obj_keys; float* obj_corr; float* obj_depth; int32_t* obj_label; float* obj_flow;  /* mvObjKeys/mvObjCorres/mvObjDepth/vSemObjLabel/mvObjFlowNext */
} vido_frame_lists;

int vido_track_slots(vido_ctx* ctx);
/* diagnosis only (VIDO_DIAG_FIRSTOP=n in the facade): n rounds of a trivial stream operation + host wait on the context's stream, timed; means printed at exit */
int vido_debug_first_op(vido_ctx* ctx, int rounds);
/* Tracking::GrabImageRGBD depth pre-scale (Tracking.cc:299-322): copies the maps of n_frames frames into
 * slots [slot0, slot0+n_frames), rescales depth on the device and writes the rescaled depth back into the
 * caller's `depth` buffer (the reference mutates it in place).  on_device: 1 = the three pointers are device pointers; 2 = device pointers that the slots ADOPT (zero-copy: no
 * copy in either direction, depth rescaled in place; the caller keeps a frame's maps alive and untouched while its slot is in use — the current and the previous frame). */
int vido_frame_upload(vido_ctx* ctx, int slot0, int n_frames, float* depth, const float* flow, const int32_t* mask,
                      int on_device, const vido_track_params* p);
/* Frame::Frame RGB-D ctor lists (Frame.cc:72-100, 165-177, 184-211) for the frames in the slots, from the
 * ORB keypoints kps[n_frames][max_kp] (host). */
int vido_frame_features(vido_ctx* ctx, int slot0, int n_frames, const vido_keypoint* kps, const int32_t* n_kps, int max_kp,
                        const vido_track_params* p, vido_frame_lists* out);
/* Fused batch front end (what Tracking::GrabImageRGBD does per frame before Track(): ORBextractor::operator() +
 * depth pre-scale + the Frame::Frame lists), one stream of launches, keypoints handed over on the device.  Results are
 * returned as a VIEW into ctx-owned pinned host memory, valid until the next call on ctx: kps/desc rows are
 * [frame][kp_pitch], list rows [frame][stat_pitch] / [frame][obj_pitch]; frame f has frame_beg[f+1]-frame_beg[f]
 * keypoints.  `depth` is rescaled in place like the reference does.  maps_on_device: 0 host buffers, 1 device buffers copied into the
 * ctx's slots, 2 device buffers used ZERO-COPY: the slots refer to them until they are overwritten (the reference keeps shallow
 * references to the caller's Mats the same way, Tracking.cc:343-345), so the caller must keep them alive and unmodified. */
typedef struct vido_frontend_view {
    int32_t n_frames, kp_pitch, stat_pitch, obj_pitch;
    const vido_keypoint* kps; const uint8_t* desc; const int32_t* frame_beg;
    const int32_t* n_stat; const int32_t* stat_idx; const float* stat_corr; const float* stat_flow; const float* stat_depth;
    const int32_t* n_obj; const float* obj_keys; const float* obj_corr; const float* obj_depth; const int32_t* obj_label; const float* obj_flow;
} vido_frontend_view;
int vido_frontend_batch(vido_ctx* ctx, const uint8_t* imgs, int imgs_on_device, int n_frames, size_t frame_stride, int stride, int width, int height,
                        float* depth, const float* flow, const int32_t* mask, int maps_on_device, int slot0, const vido_track_params* p,
                        vido_frontend_view* view);
/* Tracking.cc:369-391 / 398-421: depth (and label) of the current frame at last frame's correspondences. */
int vido_gather_static_depth(vido_ctx* ctx, int slot, const float* keys_xy, int n, float* depth_out);
int vido_gather_object_depth_label(vido_ctx* ctx, int slot, const float* keys_xy, int n, float th_depth_obj,
                                   float* depth_out, int32_t* label_out);
/* Tracking::UpdateMask (Tracking.cc:3291-3357): mask of slot_cur is patched in place on the device. */
int vido_update_mask(vido_ctx* ctx, int slot_last, int slot_cur, const int32_t* last_label, const float* last_corr_xy, int n,
                     int32_t* recovered_out, int cap, int32_t* n_recovered);
int vido_read_maps(vido_ctx* ctx, int slot, float* depth_out, float* flow_out, int32_t* mask_out);   /* any pointer may be NULL */
/* Forward warp of a whole label image through dense flow (no reference counterpart; vido_update_mask above repaints ONE lost label with the reference's quirks and is
 * independent of this).  DEVICE pointers: mask_prev i32 [H,W], flow f32 [H,W,2] (dx, dy) from mask_prev's frame into the target frame, depth_prev f32 [H,W] or NULL,
 * out i32 [H,W] (another buffer than mask_prev; EVERY pixel is written), stats_out 3 x i32 or NULL.
 *   sources   a pixel (x, y) with L = mask_prev > 0, both flow components finite with |f| < 32768 and, with a depth map, depth finite and > 0; its target is
 *             (x + rint(dx), y + rint(dy)), round to nearest with ties to even, kept iff inside the image.  Labels <= 0 never scatter.
 *   collisions a target takes the minimum of (depth bits as u32) << 32 | (u32)L over the sources that land on it (upper half 0 without depth): the nearer source, on equal
 *             depth the smaller label.
 *   holes     an unhit target takes L iff at least 5 of its 8 neighbours (outside the image = not hit) were hit and resolved to L; one pass, no cascade; else 0.
 *   stats_out sources kept, target pixels hit, pixels filled.
 * The result is independent of execution order (bit-exact against tests/refimpl/mask_propagate_np.py).  Two memsets and two launches on the context's adopted stream
 * (vido_set_stream), no host synchronisation; the context's key plane (8 bytes per pixel of its width x height) is allocated by the FIRST call, so one call comes before a
 * stream capture.  One plane per context: calls on different streams must not overlap.  out == mask_prev, a null map, H or W outside [1, 4095] or
 * H * W > width * height of the context: VIDO_E_INVALID. */
int vido_mask_propagate(vido_ctx* ctx, const int32_t* mask_prev, const float* flow, const float* depth_prev /* NULL ok */, int H, int W, int32_t* out,
                        int32_t* stats_out /* NULL ok */);
/* The same on the tracker's slot maps, on the context's own stream: mask, flow and (pre-scaled, metric) depth of slot_last -> the mask of slot_cur, whose previous content
 * is overwritten (after vido_frame_upload of slot_cur; with on_device = 2 that is the CALLER's adopted mask buffer).  stats_out: HOST, 3 x i32; NULL: nothing is waited
 * for.  slot_last == slot_cur, a slot outside [0, vido_track_slots()) or two slots adopting one mask buffer: VIDO_E_INVALID. */
int vido_frame_propagate_mask(vido_ctx* ctx, int slot_last, int slot_cur, int32_t* stats_out /* HOST, NULL ok */);
/* Instance ids that persist across frames: association of the previous handed-over label image, already warped into this frame (vido_mask_propagate's output), with the
 * detector's new instance image by pixel overlap (no reference counterpart).  ALL pointers are DEVICE pointers: prev i32 [H,W] or NULL (all zero: first frame), cur i32
 * [H,W] with value 1 + slot (id base 0), classes i64 [n] or NULL (every slot live; values are kept as their low 32 bits), state i32 [768] read and written, out i32 [H,W]
 * (may be cur; EVERY pixel is written), lut_out i32 [256] or NULL, stats_out i32 [4] or NULL.
 *   state      [0] the cursor; [256 + id] the class of id, nonzero exactly when the id is live or held; [512 + id] the calls the id has been lost.  All zeros: new sequence.
 *   0 clean    p = prev where 1 <= prev <= 254, else 0;  c = cur where 1 <= cur <= n and classes[cur - 1] != 0, else 0.
 *   1 count    C[p][c] over all pixels; Ap[p] = sum_c C[p][c] (p >= 1), Ac[c] = sum_p C[p][c] (c >= 1), zero column and row included.
 *   2 match    c with Ac[c] > 0 takes the p >= 1 with 2 C[p][c] > Ap[p] + Ac[c] - C[p][c] (IoU strictly above 1/2).  Such a p is unique and no two c share one (more than
 *              half of a pixel set can go to one partner only): no order, no tie rule.  The threshold is fixed.
 *   3 fresh    each unmatched c with Ac[c] > 0, ascending: the next id after the cursor, cyclic over 1..254, with Ap[id] == 0 and not handed out in this call; cursor = id.
 *              The cursor only moves forward: a retired id comes back only after 254 others were handed out.  No id free: the instance gets 0 and counts as left out.
 *   4 lut      LUT[c] = the matched p, the fresh id, or 0; an assigned id: class[id] = classes[c - 1] (1 without classes), lost[id] = 0.
 *   5 lost     each p with Ap[p] > 0 that nothing matched: lost[p] += 1; lost[p] <= hold: KEEP[p] = p (held in place), else KEEP[p] = 0 and class[p] = lost[p] = 0.  Ids
 *              with Ap == 0 not assigned in this call are cleared the same way (no re-identification once an id is retired).
 *   6 image    out = LUT[c] where that is nonzero, else KEEP[p].  stats_out: matched, fresh, lost (held or retired), left out.
 * Bit-exact against tests/refimpl/mask_associate_np.py whatever the execution order (integer counts).  One memset and three launches on the context's adopted stream
 * (vido_set_stream), no host synchronisation; the context's 256 KB count table is allocated by the FIRST call, so one call comes before a stream capture.  One table per
 * context: calls on different streams must not overlap.  cur, state or out NULL, out == prev, H or W outside [1, 4095], H * W > width * height of the context, hold < 0 or
 * n < 0: VIDO_E_INVALID; n > 127: VIDO_E_CAPACITY. */
int vido_mask_associate(vido_ctx* ctx, const int32_t* prev /* NULL ok */, const int32_t* cur, int H, int W, const int64_t* classes /* NULL ok */, int n, int hold,
                        int32_t* state /* DEVICE i32[768], in/out */, int32_t* out, int32_t* lut_out /* i32[256], NULL ok */, int32_t* stats_out /* i32[4], NULL ok */);
/* Split a class label image into instances: connected-component labelling (no reference counterpart: the reference's label image holds one value per class).  ALL
 * pointers are DEVICE pointers: mask i32 [H,W], out i32 [H,W] (may be mask itself; EVERY pixel is written), classes_out i64 [cap] or NULL, area_out i32 [cap] or NULL,
 * stats_out i32 [4] or NULL.
 *   foreground a pixel with mask > 0; any positive i32 value is a class; anything <= 0 is background.
 *   component  a maximal set of foreground pixels of EQUAL value joined by `connectivity` (4 or 8) neighbour steps; touching pixels of different values never join.
 *              Its anchor is its smallest raster index y * W + x, its area its pixel count.
 *   drop       components with area < min_area are dropped (min_area <= 1 keeps all).
 *   order      the survivors in ascending anchor order are k = 0, 1, ...; k < cap is KEPT: out = id_base + 1 + k on its pixels, classes_out[k] = its value,
 *              area_out[k] = its area; the rest are LEFT OUT: out = 0 (as on dropped components and background).  classes_out / area_out entries >= kept: 0.
 *   stats_out  components found, dropped for area, left out for cap, kept.
 * With id_base 0 and cap 127 `out` and `classes_out` are what vido_mask_associate takes as cur and classes.  Bit-exact against tests/refimpl/mask_components_np.py whatever
 * the execution order (integer minima and sums).  One memset and seven launches on the context's adopted stream (vido_set_stream), no host synchronisation; the context's
 * planes (8 bytes per pixel of its width x height) are allocated by the FIRST call, so one call comes before a stream capture.  One set of planes per context: calls on
 * different streams must not overlap.  mask or out NULL, out overlapping mask without being mask, connectivity not 4 or 8, H or W outside [1, 4095], H * W > width * height
 * of the context, id_base < 0 or cap < 1: VIDO_E_INVALID; id_base + cap > 254: VIDO_E_CAPACITY. */
int vido_mask_components(vido_ctx* ctx, const int32_t* mask, int H, int W, int connectivity, int min_area, int id_base, int cap, int32_t* out,
                         int64_t* classes_out /* i64[cap], NULL ok */, int32_t* area_out /* i32[cap], NULL ok */, int32_t* stats_out /* i32[4], NULL ok */);
/* The same rule on the tracker's slot: the mask of `slot` is split in place, on the context's own stream (after vido_frame_upload of the slot; with on_device = 2 that is
 * the buffer the slot adopted).  stats_out: HOST, 4 x i32; NULL: nothing is waited for.  A slot outside [0, vido_track_slots()): VIDO_E_INVALID; the other refusals as above. */
int vido_frame_split_mask(vido_ctx* ctx, int slot, int connectivity, int min_area, int id_base, int cap, int32_t* stats_out /* HOST i32[4], NULL ok */);
/* mask / depth / flow of slot `slot` at ((int)x, (int)y) of n points (host xy in, host values out; points outside the image give 0): the only map data the host-side
 * renew stages need (vido_renew_*_sampled) — a few thousand points instead of three whole maps.  Inside means 0 <= (int)x < width and 0 <= (int)y < height: x in (-1, 0)
 * truncates to column 0.  Capacity: n <= 2 * max(2 * n_features + 256, ceil(width / 4) * ceil(height / 4)); a larger n is VIDO_E_INVALID.  n == 0 is a successful no-op. */
int vido_gather_point_samples(vido_ctx* ctx, int slot, const float* xy, int n, int32_t* mask_out, float* depth_out, float* flow_out);
/* Frame::UnprojectStereoStat/Object, addnoise=0 (Frame.cc:706-771): Tcw row-major 4x4 f32. */
int vido_unproject_world(vido_ctx* ctx, const float* keys_xy, const float* z, int n, const vido_track_params* p,
                         const float* Tcw, float* xyz_out);
/* Tracking::GetSceneFlowObj (Tracking.cc:1582-1668). */
int vido_scene_flow(vido_ctx* ctx, const float* xyz_last, const float* xyz_cur, const int32_t* sem_last, const int32_t* sem_cur,
                    int n, float* flow3d_out, int32_t* obj_label_inout);

/* ---- Per-frame pose / object-motion optimisers (Levenberg-Marquardt on the device, FP64) -----------------
 * One problem = one of the reference's four optimiser calls; the constants each of them hard-codes
 * (information, Huber delta, rounds, iteration caps, chi2 thresholds) are explicit fields so the caller
 * (C++ facade Optimizer::PoseOptimization*, or vido-slam_amd/problems.py) states them once.
 *   mode 0  EdgeSE3ProjectXYZOnlyPose     e = obs - pi_K(T Xw)                  PoseOptimizationNew      Optimizer.cc:2180
 *   mode 1  EdgeSE3ProjectFlow2 + prior   e = (obs+f) - pi_K(T Twl K^-1(obs,d)) PoseOptimizationFlow2Cam :2622 / Flow2 :3037
 *   mode 2  EdgeSE3ProjectXYZOnlyObjMotion e = obs - proj(P (H Xw))             PoseOptimizationObjMot   :2826
 * All matrices row-major double; T is updated as exp(delta) * T (VertexSE3Expmap). */
typedef struct vido_pose_problem {
    int32_t mode, n;
    const double* Xw;          /* [n*3] world points (modes 0, 2) */
    const double* obs;         /* [n*2] measurement: current keypoint (0, 2) or LAST-frame keypoint (1) */
    const double* flow0;       /* [n*2] initial optical flow (mode 1) */
    const double* depth;       /* [n]   depth in the last frame (mode 1) */
    double Twl[16];            /* last camera -> world (mode 1) */
    double P[12];              /* K [R|t]_cw, 3x4 (mode 2) */
    double fx, fy, cx, cy;
    double T_init[16];         /* initial estimate; every round restarts from it (Optimizer.cc:2266, 2742) */
    double info_edge, info_prior, huber_delta;
    int32_t use_huber, rounds, drop_kernel_after_round;
    int32_t iters[4];
    float chi2_th[4];
} vido_pose_problem;

typedef struct vido_pose_result { double T[16]; int32_t n_inliers, lm_iterations; double chi2_final; } vido_pose_result;

/* outlier_out[n] (1 = rejected), flow_out[n*2] refined flow (mode 1; zeros otherwise); either may be NULL. */
int vido_pose_optimize(vido_ctx* ctx, const vido_pose_problem* prob, vido_pose_result* result, uint8_t* outlier_out, double* flow_out);
/* n_prob independent problems in one launch (one workgroup each): e.g. all dynamic objects of a frame. */
int vido_pose_optimize_batch(vido_ctx* ctx, const vido_pose_problem* probs, int n_prob, vido_pose_result* results,
                             uint8_t* const* outlier_out, double* const* flow_out);

/* ---- Bundle adjustment (windowed = PartialBatchOptimization, global = FullBatchOptimization) ---------------
 * Flat SoA problem, all f64 / i32, caller-owned; mirrors what the reference assembles from Map
 * (Optimizer.cc:216-350): camera-to-world poses (Map::vmCameraPose), one 3-D point per static tracklet,
 * observations = the point in the camera frame (Get3DinCamera), odometry = Map::vmRigidMotion[k][0],
 * optional prior on one camera.  Poses are row-major 3x4 [R|t].  cam_T and pt_xyz are updated in place.
 * Factor set of this build: EdgeSE3PointXYZ + EdgeSE3 + EdgeSE3Prior (the STATIC_ONLY graph); the
 * object-motion factors of FullBatchOptimization are listed under "next" in DESIGN.md.
 * Sharding (global BA over several GPUs, one process per GPU): every rank passes the whole problem with its own
 * landmark range [pt_lo, pt_hi) and rank/world; partial reduced systems are summed through `allreduce`. */
typedef struct vido_ba_problem {
    int32_t n_cam, n_pt, n_obs, n_odo, prior_cam, use_huber, max_iters, pad;
    double* cam_T; double* pt_xyz;
    const int32_t* obs_cam; const int32_t* obs_pt; const double* obs_meas;
    const int32_t* odo_i; const int32_t* odo_j; const double* odo_T;
    double prior_T[12];
    double info_obs, info_odo, info_prior, huber_obs, huber_odo, gain_threshold;
    int32_t pt_lo, pt_hi;      /* landmark shard of this rank; pt_hi <= pt_lo means "all" */
    int32_t rank, world;       /* rank 0 owns the camera-camera factors (odometry, prior) */
} vido_ba_problem;

typedef struct vido_ba_result { int32_t iterations, lm_trials; double chi2_initial, chi2_final, lambda_final;
                                double ms_setup;        /* host preprocessing + upload (wall) */
                                double ms_solve_loop;   /* the LM loop proper, inputs resident in HBM (wall) */
                                double ms_linearize_kernel;   /* mean k_ba_linearize duration (HIP events on the ctx stream) */
                                double ms_schur_kernel;       /* mean k_ba_schur_mfma duration (global path; 0 when another Schur kernel ran) */
} vido_ba_result;

/* In-place all-reduce of `count` doubles at DEVICE address `dev_ptr` over all ranks (op 0 = sum, 1 = max);
 * return 0 on success.  The ctx stream is idle when it is called.  NULL = single GPU. */
typedef int (*vido_allreduce_fn)(void* user, void* dev_ptr, size_t count, int op);

int vido_ba_optimize(vido_ctx* ctx, vido_ba_problem* prob, vido_ba_result* result, vido_allreduce_fn allreduce, void* user);
/* The all-reduce issued by the library itself: RCCL (over xGMI) on the context's stream, in place, no host synchronisation — the role the reference gives nothing to
 * (it is single-process).  One process per GPU: rank 0 calls vido_rccl_unique_id and distributes the 128 bytes by any means (bench.py: a
 * torch.distributed broadcast), every rank calls vido_rccl_init on its context, then passes `vido_rccl_allreduce` as `allreduce` and the context as `user`.
 * librccl is resolved at run time (dlopen); a process that never calls these does not load it. */
int vido_rccl_unique_id(uint8_t id_out[128]);
int vido_rccl_init(vido_ctx* ctx, const uint8_t id[128], int rank, int world);
int vido_rccl_allreduce(void* user_ctx, void* dev_ptr, size_t count, int op);
int vido_rccl_destroy(vido_ctx* ctx);

/* Object part of Optimizer::FullBatchOptimization (Optimizer.cc:1235-2178 with STATIC_ONLY = false): per (object, frame)
 * motion vertices H (VertexSE3, the reference initialises them to identity, :1592), one dynamic point vertex per
 * observation with its EdgeSE3PointXYZ to camera dyn_cam[k] (:1560-1582, :1683-1726), LandmarkMotionTernaryEdge
 * (tern_prev, tern_cur, tern_H), e = p_prev - H^-1 p_cur (:1728-1745, types/types_dyn_slam3d.cpp:53-85) and EdgeSE3
 * smoothness edges with identity measurement between motion vertices sm_i -> sm_j (:1604-1636).  The ternary edges
 * must link the dynamic points into chains (every point has at most one predecessor and one successor), which is what
 * the reference's tracklets produce.  H_T / dyn_xyz are updated in place.  With an all-reduce hook rank 0 owns this part. */
typedef struct vido_ba_dynamic {
    int32_t n_H, n_dyn, n_tern, n_smooth;
    double* H_T;                 /* [n_H*12] row-major 3x4 */
    double* dyn_xyz;             /* [n_dyn*3] world */
    const int32_t* dyn_cam; const double* dyn_meas;                            /* [n_dyn], [n_dyn*3] (point in the camera frame) */
    const int32_t* tern_prev; const int32_t* tern_cur; const int32_t* tern_H;  /* [n_tern] */
    const int32_t* sm_i; const int32_t* sm_j;                                  /* [n_smooth] indices into H */
    double info_dyn, info_tern, info_smooth, huber_dyn, huber_tern, huber_smooth;
} vido_ba_dynamic;
int vido_ba_optimize_dynamic(vido_ctx* ctx, vido_ba_problem* prob, vido_ba_dynamic* dyn, vido_ba_result* result,
                             vido_allreduce_fn allreduce, void* user);

/* ---- Native ops of the three network nodes (the nets' conv/GEMM layers run on PyTorch-ROCm) -----------------
 * All tensors f32, NCHW contiguous.  on_device != 0: every pointer is a device pointer and the call only
 * enqueues on the ctx stream (this is how the torch modules call them); otherwise host pointers, synchronous. */
/* correlation.FunctionCorrelation(first, second, intStride) — flow_net/src/correlation/correlation.py:277-335.
 * out: [B, 49, ceil(H/stride), ceil(W/stride)]. */
int vido_correlation(vido_ctx* ctx, const float* first, const float* second, int B, int C, int H, int W, int stride,
                     float* out, int on_device);
/* the static detector head's tail (confidence test, stable descending order by score, labels of the live slots, their count) in one launch: csrc/nets.hip::k_det_order */
int vido_det_order(vido_ctx* ctx, const float* scores, const long long* labels, const int* n_det, float confidence, int cap, long long* order, long long* labels_out, long long* n_live);
/* vido_det_order that also writes the count as an int32 DEVICE word (n_live32, may be NULL): the word the `_n` entry points of the mask head read. */
int vido_det_order_n(vido_ctx* ctx, const float* scores, const long long* labels, const int* n_det, float confidence, int cap, long long* order, long long* labels_out, long long* n_live,
                     int32_t* n_live32);
/* FPN level of every box (LevelMapper, modeling/poolers.py:11-45: floor(4 + log2(sqrt(area) / 224 + 1e-6)) clamped to [k_min, k_max], minus k_min) in one launch */
int vido_roi_levels(vido_ctx* ctx, const float* boxes, int n, float k_min, float k_max, int* out);
/* The mask head's tail for the one class channel a detection needs (mask_head/roi_mask_predictors.py:27-31 + inference.py:29-47): out[n][p] = sigmoid(sum_c w[label[n]][c]
 * feat[n][c][p] + b[label[n]]); feat [n][c][hw] f32, w [classes][c], labels int64 [n], out [n][hw] (csrc/nets.hip). */
int vido_mask_logit_select(vido_ctx* ctx, const float* feat, const float* w, const float* b, const long long* labels, float* out, int n, int c, int hw, int classes);
/* The `_n` forms of the mask head (vido_roi_align_fpn_nhwc_n, vido_conv3x3_h_bias_act_n, vido_deconv2x2_bias_act_n, vido_mask_logit_select_n): the call over a batch of n
 * slots of which only the first *n_live are LIVE.  n_live is a DEVICE int32 word read when the kernel runs, hence at every replay of a captured graph, and clamped to [0, n];
 * NULL means all n (the plain entry points forward that).  The launch shape is that of n slots; the work is that of n_live: the slots behind the count are never READ (their
 * rows may hold stale bytes) and, except here, never written.  vido_mask_logit_select_n writes ZEROS to them, so the masks tensor is fully defined. */
int vido_mask_logit_select_n(vido_ctx* ctx, const float* feat, const float* w, const float* b, const long long* labels, float* out, int n, int c, int hw, int classes, const int32_t* n_live);
/* Conv epilogue on a DEVICE tensor x[N,C,H,W] (f32, contiguous), in place: x = leaky_relu(x + bias[c], slope) — the bias add and the
 * LeakyReLU(0.1) that follow every convolution of flow_net/src/layers.py fused into one pass (slope = 1: plain bias add). */
int vido_bias_act(vido_ctx* ctx, float* x, const float* bias, int N, int C, int H, int W, float slope);
/* MonoDepth2's decoder glue as single passes (mono_depth2/src/networks/depth_decoder.py:51-66, layers.py ConvBlock / Conv3x3 / upsample; run_mono_depth.py:137-145), DEVICE tensors:
 * vido_bias_unary: x = f(x + bias[c]) in place, kind 1 = ELU (ConvBlock), 2 = logistic function (the disparity head);
 * vido_upcat_reflect: ReflectionPad2d(1)(cat([upsample(x, 2, nearest), skip], 1)) — upsample + cat + the next Conv3x3's pad; x [C1][h][w], skip [C2][2h][2w] or NULL, out [C1+C2][2h+2][2w+2];
 * vido_minmax_norm_u16: the node's min-max normalisation to MONO16, out = (int) clamp((d - min) / (max - min + 1e-12) * 65536, 0, 65535), mm = {min, max} on the device. */
int vido_bias_unary(vido_ctx* ctx, float* x, const float* bias, int N, int C, int H, int W, int kind);
int vido_upcat_reflect(vido_ctx* ctx, const float* x, const float* skip, int C1, int C2, int h, int w, float* out);
int vido_minmax_norm_u16(vido_ctx* ctx, const float* d, const float* mm, int64_t n, int32_t* out);
/* x = act(x + bias[c] + res), res a DEVICE tensor shaped like x (NULL: vido_bias_act): closes a ResNe(X)t bottleneck whose FrozenBatchNorm2d
 * (maskrcnn_benchmark/layers/batch_norm.py:19-31) has been folded into the convolution weights and this bias
 * (modeling/backbone/resnet.py:352-372: out = bn3(conv3(.)); out += identity; relu). */
int vido_bias_res_act(vido_ctx* ctx, float* x, const float* bias, const float* res, int N, int C, int H, int W, float slope);
/* Node pre-processing in one pass: u8 H x W x 3 interleaved BGR (DEVICE) -> f32 [3][OH][OW] planar RGB, resized with the area rule of the nodes' cv2.resize(..., INTER_AREA) /
 * torch interpolate(mode="area") (mask_rcnn/src/predictor.py:267-283, mono_depth2/src/run_mono_depth.py:113-118), divided by `div` (255 for the depth node, 1 for the detector). */
int vido_area_feed(vido_ctx* ctx, const uint8_t* bgr, int H, int W, float* out, int OH, int OW, float div);
/* flow_net/src/layers.py:25-37 `Backward`: bilinear warp of x[B,C,H,W] by flow[B,2,H,W] (pixels; grid_sample with zero padding, align_corners False on the grid
 * -1 + (2i+1)/n + flow / ((n-1)/2)); DEVICE tensors, f32, contiguous. */
int vido_backwarp(vido_ctx* ctx, const float* x, const float* flow, int B, int C, int H, int W, float* out);
/* LiteFlowNet's regularisation stage (flow_net/src/layers.py:213-262, Regularization.forward) outside its convolutions, as two passes over DEVICE tensors (f32, NCHW):
 * front: out[:, 0] = sqrt(sum_c (im1 - Backward(im2, flow * scale))^2), out[:, 1:3] = flow - mean (mean [B,2] = the spatial mean of flow, a device tensor); out has
 *        out_channels >= 3 channels, the caller copies netFeat's features behind the first three (the stage's torch.cat);
 * tail:  dist [B, K*K, H, W] = netDist's output -> out [B, 2, H, W] = (netScaleX(d * unfold(flow_x, K)), netScaleY(d * unfold(flow_y, K))) / sum_c d with
 *        d = exp(-dist^2 - max_c(-dist^2)); wx / wy [K*K] and bx / by [1] are the two 1x1 convolutions' parameters; K in {3, 5, 7}. */
/* Depthwise ConvTranspose2d(C, C, 4, stride 2, padding 1, groups = C, bias = False) on DEVICE tensors: x [B,C,H,W] -> out [B,C,2H,2W], weight [C,1,4,4]; the input passes
 * through LeakyReLU(input_slope) first (1 = none).  LiteFlowNet's netUpflow / netUpcorr (flow_net/src/layers.py:105-108, 130-135). */
int vido_deconv4s2_depthwise(vido_ctx* ctx, const float* x, const float* weight, int B, int C, int H, int W, float input_slope, float* out);

/* Grouped 3x3 convolution + bias + ReLU on the fp32 matrix cores (csrc/gconv.hip): `conv2` of BottleneckWithFixedBatchNorm with the frozen batch norm folded in
 * (maskrcnn_benchmark/modeling/backbone/resnet.py:300-372, layers/batch_norm.py:19-31) — Conv2d(width, width, 3, 1, 1, groups) + FrozenBatchNorm2d + relu_ as ONE launch.
 * x [groups * cpg_in][H][W], y [groups * cpg_out][H][W] f32 DEVICE tensors of one image (x != y), bias [groups * cpg_out]; w_packed: the folded weight rearranged into
 * matrix-core operand order (vido_gconv3x3_packed_size floats; layout in csrc/gconv.hip, built by vido_slam_amd/nets/ops.py::pack_gconv3x3).  slope: 0 = ReLU, 1 = none.
 * in_bias (NULL or [groups * cpg_in]): the convolution reads relu(x + in_bias[channel]) instead of x — conv1's folded batch norm + relu_ of the same bottleneck applied on
 * the way in, so that the 1x1 convolution in front needs no pass of its own over its output.
 * vido_gconv3x3_supported: 1 when a kernel exists for the shape (8, 16 or a multiple of 32 channels per group and a row band that fits LDS); otherwise the call returns
 * VIDO_E_INVALID and the caller keeps the library convolution. */
/* 1x1 convolution (stride 1, batch 1) + bias + residual + leaky-ReLU as one matrix-core GEMM (csrc/conv1x1.hip): conv1 / conv3 / the stride-1 shortcut of
 * BottleneckWithFixedBatchNorm with their folded FrozenBatchNorm2d (maskrcnn_benchmark/modeling/backbone/resnet.py:300-372, layers/batch_norm.py:19-31).  x [cin][hw],
 * y / residual [cout][hw], f32 DEVICE, 16-byte aligned, y != x; bias [cout] or NULL; residual NULL = none; w_packed: [cout][cin] in operand order
 * (vido_slam_amd/nets/ops.py::pack_conv1x1) and `layout` the number of that order: 0 = fp32 [co / 32][k / 8][32 (k & 1) + co % 32][(k % 8) / 2] (4 cin cout bytes: the fp32
 * matrix instruction), 2 = split-bf16 (6 cin cout bytes), 3 = split-fp16 (4 cin cout + 4 cout bytes), both described at vido_conv1x1_set_arith.  The launch runs the kernel
 * of the layout it is given and reads that many bytes, whatever the arithmetic setting is by then; any other `layout` returns VIDO_E_INVALID.
 * slope: 0 = ReLU, 1 = none.  vido_conv1x1_supported: cout % 128 == 0, cin % 32 == 0, hw >= 128. */
int vido_conv1x1_supported(int cin, int cout, int hw);
/* the weight packing to MAKE for a shape under the current arithmetic setting (vido_conv1x1_set_arith): 3, 2 or 0.  A recommendation to the packer: a launch is told the
 * layout of the weight it is handed and never asks this function. */
int vido_conv1x1_layout(int cin, int cout, int hw);
/* Arithmetic of the 1x1 GEMM (round 6): fp32-equivalent results from the 16-bit matrix instructions (error against float64 not above the fp32 instruction's:
 * tests/test_maskrcnn_gpu.py).
 *   0 (default) = split-fp16: every fp32 operand is h + 2^-11 l' with h = rne16(x), l' = rne16(2^11 (x - h)) (|x - h - 2^-11 l'| <= 2^-22 |x|, 2^-24.5 |x| rms); the three products
 *       w_h x_h, w_h x_l', w_l' x_h run on v_mfma_f32_32x32x16_f16 with fp32 accumulators.  vido_conv1x1_layout answers 3 =
 *       [co / 32][k / 16][plane 2][32 ((k % 16) / 8) + co % 32][k % 8] fp16 of the weight scaled per OUTPUT CHANNEL by the power of two that puts the channel's largest |w| into
 *       [2^14, 2^15), followed by [cout] floats: the inverse scales (4 bytes per weight + 4 per channel).  Activations: full precision for 2.5e-4 <= |x| < 65504 (smaller ones: an absolute error <= 1.5e-11); a launch
 *       that meets |x| >= 65504, an infinity or a NaN raises vido_conv1x1_range_flag (its outputs are not valid then).
 *   2 = split-bf16: three bf16 planes, the six plane products with i + j <= 2 on v_mfma_f32_32x32x16_bf16; fp32's range, twice the matrix work; layout 2 =
 *       [co / 32][k / 16][plane 3][32 ((k % 16) / 8) + co % 32][k % 8] bf16 (6 bytes per weight).
 *   1 = the fp32 matrix instruction (layout 0 above).
 * Also selected by VIDO_CONV1X1_ARITH = f16x2 | bf16x3 | f32 in the environment.  Returns the previous setting; process-wide.  The setting selects what vido_conv1x1_layout
 * recommends (and with it whether vido_deconv2x2_supported answers 1) and nothing else: weights already packed keep running in the arithmetic they were packed for,
 * because every launch is handed its weight's layout. */
int vido_conv1x1_set_arith(int arith);
/* the current setting (0 / 1 / 2) */
int vido_conv1x1_get_arith(void);
/* non-zero when a split-fp16 launch on this context (1x1, 3x3, fully connected, 2x2 transposed) met an activation outside fp16's range, an infinity or a NaN since the last
 * reset; read after the stream has been waited for.  reset != 0: read and clear in one atomic exchange. */
int vido_conv1x1_range_flag(vido_ctx* ctx, int reset);
/* Per-frame latch of that flag (csrc/rangelatch.hip): enqueues on the context's adopted stream (vido_set_stream) a one-lane launch that exchanges the flag with 0 and ORs
 * the old value into *dst (a pinned host word or a device word, system-scope atomics).  In stream order *dst then holds the trips of the split-fp16 launches enqueued before
 * the latch, and launches after it raise the flag afresh: a frame's latch names that frame even while the next frame's networks are already queued.  dst is not cleared:
 * the caller zeroes it before the launches it is to cover.  Capturable. */
int vido_range_latch(vido_ctx* ctx, unsigned* dst);
int vido_conv1x1_bias_act(vido_ctx* ctx, const float* x, const float* w_packed, const float* bias, const float* residual, float* y, int cin, int cout, int hw, float slope, int layout);
/* 2 x 2 stride-2 transposed convolution + bias + leaky-ReLU of a batch as one split-fp16 GEMM with a scatter epilogue (the mask head's conv5_mask,
 * roi_heads/mask_head/roi_mask_predictors.py:17-31): x [n][cin][h][w] -> y [n][cout][2 h][2 w]; w_packed: pack_conv1x1 layout 3 of [(2 a + b) cout + co][ci] = w[ci][co][a][b]
 * (vido_slam_amd/nets/ops.py::pack_deconv2x2).  vido_deconv2x2_supported: cout % 128 == 0, cin % 32 == 0, (h w) % 4 == 0, n h w >= 128, split-fp16 arithmetic selected. */
int vido_deconv2x2_supported(int n, int cin, int cout, int h, int w);
int vido_deconv2x2_bias_act(vido_ctx* ctx, const float* x, const float* w_packed, const float* bias, float* y, int n, int cin, int cout, int h, int w, float slope);
/* ... of the first *n_live images only (see vido_mask_logit_select_n): a tile of columns that straddles the count reads zeros for the images behind it and stores nothing there. */
int vido_deconv2x2_bias_act_n(vido_ctx* ctx, const float* x, const float* w_packed, const float* bias, float* y, int n, int cin, int cout, int h, int w, float slope, const int32_t* n_live);
/* ... with the residual at half the resolution [cout][h/2][w/2], added nearest-upsampled: the FPN's lateral convolution + top-down sum (backbone/fpn.py:55-66); h, w even */
int vido_conv1x1_bias_up2_act(vido_ctx* ctx, const float* x, const float* w_packed, const float* bias, const float* residual_half, float* y, int cin, int cout, int h, int w, float slope, int layout);

/* k x k convolution (k = 3, 5, 7; stride 1, padding k / 2) to TWO output channels + bias + residual for one image (csrc/convsmall.hip): the last layer of LiteFlowNet's
 * matching / sub-pixel heads with the `flow + netMain(...)` behind it (flow_net/src/layers.py:152-160, 191-199).  x [cin][h][w], w [2][cin][k][k], bias [2] or NULL,
 * residual [2][h][w] or NULL, y [2][h][w]: f32 DEVICE tensors. */
int vido_conv_kxk_c2(vido_ctx* ctx, const float* x, const float* w, const float* bias, const float* residual, float* y, int cin, int k, int h, int w_);
/* 1x1 convolution with FEW input channels (even, <= 256; cout <= 256) + bias + residual + leaky ReLU for one image, no LDS: LiteFlowNet's netFeat layers
 * (layers.py:99, 125, 140), the detector's layer1 and RPN heads.  w_packed: element (co, k) at [co / 32][k / 2][32 * (k & 1) + co % 32], cout padded to 32 with zeros.
 * cout <= 32: 16 k-pairs requested ahead of the matrix instructions; VIDO_SKINNY_DEPTH=4 | 8 | 16 (read per call) selects the depth, every depth gives the same bits. */
int vido_conv1x1_skinny(vido_ctx* ctx, const float* x, const float* w_packed, const float* bias, const float* residual, float* y, int cin, int cout, long long hw, float slope);
/* The detector's stem in one launch (csrc/stem.hip): y = max_pool2d(relu(conv2d(x, w, stride 2, padding 3) + bias), 3, 2, 1) for one image, 7x7 kernel, 3 -> 64 channels.
 * x [3][h][w], bias [64], y [64][hp][wp] with hc = (h - 1) / 2 + 1, hp = (hc - 1) / 2 + 1 (likewise w): f32 DEVICE tensors.  w_packed [2][84][64]: element (co, c, dy, dx)
 * of the weight at [co / 32][(c * 7 + dx) * 4 + dy / 2][32 * (dy & 1) + co % 32], the dy = 7 entries zero (nets/ops.py::pack_stem7x7).  fp32 matrix instructions, fp32
 * accumulation; the convolution's output never reaches memory.  Enqueues on the adopted stream; capturable. */
int vido_stem7x7s2_pool(vido_ctx* ctx, const float* x, const float* w_packed, const float* bias, float* y, int h, int w);

/* k x k convolution (7x7, 5x5, 3x3, 7x1, 1x7, 5x1, 1x5, 1x1; strides 1-4; zero padding) + bias + leaky ReLU as a direct implicit GEMM on the fp32 matrix pipe, one launch
 * (csrc/convdirect.hip): the layers of LiteFlowNet that the library ran as im2col / transposes + GEMM + a bias pass — the 7x7 stem, the stride-2 3x3 convolutions of the
 * feature pyramid, the separable distance layers of the regularisation (flow_net/src/layers.py:39-73, 217-235).  x [n][cin][h][w], y [n][cout][ho][wo] f32 DEVICE tensors,
 * w_packed = vido_conv_direct_pack(w [cout][cin][kh][kw]) (host) copied to the device, vido_conv_direct_packed_floats floats; bias [cout] or NULL; slope 0 = ReLU, 1 = none. */
int vido_conv_direct_supported(int cin, int cout, int h, int w, int kh, int kw, int sh, int sw, int ph, int pw);
long long vido_conv_direct_packed_floats(int cin, int cout, int kh, int kw);
int vido_conv_direct_pack(const float* w, int cin, int cout, int kh, int kw, float* w_packed);
int vido_conv_direct_bias_act(vido_ctx* ctx, const float* x, const float* w_packed, const float* bias, float* y, int n, int cin, int cout, int h, int w,
                              int kh, int kw, int sh, int sw, int ph, int pw, float slope);

/* 3x3 stride-1 padding-1 convolution + bias + leaky-ReLU as Winograd F(2x2, 3x3) with its sixteen channel contractions on the fp32 matrix pipe (csrc/wino.hip): the
 * dense 3x3 convolutions of LiteFlowNet (flow_net/src/layers.py:39-315), the FPN output / RPN head / mask head convolutions of the detector
 * (maskrcnn_benchmark/modeling/backbone/fpn.py, rpn/rpn.py:74-107, roi_heads/mask_head/roi_mask_feature_extractors.py) — what the library runs as a vector-ALU Winograd
 * kernel followed by a bias + activation pass.  x [n][cin][h][w], y [n][cout][h][w] f32 DEVICE tensors (y != x), bias [cout] or NULL, slope 0 = ReLU, 1 = none.
 * u_packed: vido_wino3x3_pack(w) copied to the device (16-byte aligned), vido_wino3x3_packed_floats(cin, cout) floats.  vido_wino3x3_pack runs on the HOST:
 * w [cout][cin][3][3] -> U = G g G^T in float64, rounded once, in the kernel's operand order.  vido_wino3x3_supported: cin >= 8, cout >= 32, h, w >= 2, tensors < 1 GB.
 * The result differs from a direct fp32 convolution by rounding only (the class of the library's own Winograd kernels).  Enqueues on the adopted stream; capturable. */
int vido_wino3x3_supported(int cin, int cout, int h, int w);
int vido_wino3x3_fills_chip(int n, int cout, int h, int w, int min_wgs);   /* 1 when the launch has >= min_wgs (0: 128) workgroups: below that the library's kernels win */
long long vido_wino3x3_packed_floats(int cin, int cout);
int vido_wino3x3_pack(const float* w, int cin, int cout, float* u_packed);
int vido_wino3x3_bias_act(vido_ctx* ctx, const float* x, const float* u_packed, const float* bias, float* y, int n, int cin, int cout, int h, int w, float slope);
/* The two launch forms.  0: the tile form above (a wave walks ALL input channels of its 32 channels x 32 tiles).  1: the K-split form for launches that would leave most of
 * the chip idle (fewer than 128 workgroups of the tile form: FPN P4-P6, the flow network's levels 3-6): a workgroup = 32 channels x 32 tiles, its four waves take a quarter of
 * the input channels each, the partial sums meet in LDS in a fixed order.  2: two channel slices x two tile blocks per workgroup (same packing as 1).  vido_wino3x3_form: the
 * form the library recommends for a launch (VIDO_WINO_KSPLIT=0/4/2: never / always 1 / always 2 for under-filled launches);
 * the packed weight must be of the form the launch is given (form 1 packs 4-channel chunks for every cout).  The un-suffixed entries are form 0. */
int vido_wino3x3_form(int n, int cin, int cout, int h, int w);
/* Fully connected layer y[rows][outs] = leaky_relu(x[rows][k] w[outs][k]^T + bias, slope) in the split-fp16 arithmetic of vido_conv1x1_set_arith(0), split over k (csrc/fch.hip,
 * round 6): the box head's fc6 (roi_heads/box_head/roi_box_feature_extractors.py:50-81).  w_packed: pack_conv1x1 layout 3 of w viewed as [outs][k][1][1]; part: scratch of
 * vido_fc_h_splitk(rows, k, outs) x rows x outs floats.  vido_fc_h_splitk: 0 = shape not taken (outs % 128, k % (32 S)). */
int vido_fc_h_splitk(int rows, int k, int outs);
int vido_fc_h(vido_ctx* ctx, const float* x, const void* w_packed, const float* bias, float* part, float* y, int rows, int k, int outs, float slope);
/* Dense 3x3 stride-1 `same` convolution + bias + leaky-ReLU as a DIRECT implicit GEMM in the split-fp16 arithmetic of vido_conv1x1_set_arith(0) (csrc/conv3x3h.hip, round 6):
 * the detector's chip-filling 256 -> 256 layers (FPN outputs and RPN head on P2 / P3: backbone/fpn.py:55-66, rpn/rpn.py:74-107; the mask head: roi_mask_feature_extractors.py).
 * x [n][cin][h][w], y [n][cout][h][w] f32 DEVICE; w_packed: two fp16 planes of the output channels scaled by powers of two, plane p of element (co, ci, dy, dx) at
 * [co / 32][ci / 16][dy][dx][p][32 ((ci % 16) / 8) + co % 32][ci % 8], then [cout] floats: the inverse scales (vido_slam_amd/nets/ops.py::pack_conv3x3_h).
 * vido_conv3x3_h_supported: cout 32, 64 or a multiple of 128 (input channels are padded to a multiple of 16 with zero weights), tensors below 1 GB.  Activations must be finite and below 65504 in magnitude (vido_conv1x1_range_flag otherwise); the padded channels never read
 * the next image's activations. */
int vido_conv3x3_h_supported(int n, int cin, int cout, int h, int w);
int vido_conv3x3_h_workgroups(int n, int cout, int h, int w);
int vido_conv3x3_h_bias_act(vido_ctx* ctx, const float* x, const void* w_packed, const float* bias, float* y, int n, int cin, int cout, int h, int w, float slope);
/* ... of the first *n_live images only (see vido_mask_logit_select_n); the live workgroups are dealt over the chip as a launch of n_live images would deal them. */
int vido_conv3x3_h_bias_act_n(vido_ctx* ctx, const float* x, const void* w_packed, const float* bias, float* y, int n, int cin, int cout, int h, int w, float slope, const int32_t* n_live);
/* Layers of >= 128 output channels: the counted launch is ONE kernel that picks its form from the count when it runs — a fine form (fewer channels per workgroup, so more
 * and shorter-lived workgroups) while the live images leave most of the chip idle, the uncounted launch's form otherwise; every form gives the same bits.
 * vido_conv3x3_h_live_form: what a count word `live` (clamped to [0, n] like the kernel's) selects — returns 1 for the fine form, 0 for the coarse one, and stores the form's
 * output channels per workgroup and rows per position block (either pointer may be NULL).
 * vido_mask_head_coarse: 1 when VIDO_MASK_HEAD_COARSE=1 is set (read once per process): the counted launches of the mask head (this one, vido_roi_align_fpn_nhwc_n,
 * vido_mask_logit_select_n, vido_mask_label_image_n) then keep the launch shapes of the uncounted calls — an attribution switch, same results.
 * vido_conv3x3_h_bias_act_form: measurement only — the uncounted launch forced into the form <rpw, cg> (32 rpw cg channels per workgroup, 16 / cg block rows). */
int vido_conv3x3_h_live_form(int n, int cout, int h, int w, int live, int* channels, int* block_rows);
int vido_mask_head_coarse(void);
int vido_conv3x3_h_bias_act_form(vido_ctx* ctx, const float* x, const void* w_packed, const float* bias, float* y, int n, int cin, int cout, int h, int w, float slope, int rpw, int cg);
long long vido_wino3x3_packed_floats_form(int cin, int cout, int form);
int vido_wino3x3_pack_form(const float* w, int cin, int cout, int form, float* u_packed);
int vido_wino3x3_bias_act_form(vido_ctx* ctx, const float* x, const float* u_packed, const float* bias, float* y, int n, int cin, int cout, int h, int w, float slope, int form);
int vido_gconv3x3_supported(int H, int W, int cpg_in, int cpg_out);
int64_t vido_gconv3x3_packed_size(int groups, int cpg_in, int cpg_out);
int vido_gconv3x3_bias_act(vido_ctx* ctx, const float* x, const float* in_bias, const float* w_packed, const float* bias, float* y, int groups, int cpg_in, int cpg_out, int H, int W, float slope);
/* The same convolution (no in_bias) with 32 -> 32 or 64 -> 64 channels per group in the split-fp16 arithmetic of vido_conv3x3_h_bias_act (csrc/gconvh.hip): `conv2` of the
 * ResNeXt bottlenecks of layer3 / layer4.  w_packed (16-byte aligned): two fp16 planes of the output channels scaled by powers of two, plane p of element (co, ci, dy, dx) of
 * group g at [g][(co % cpg) / 32][ci / 16][3 dy + dx][p][32 ((ci % 16) / 8) + co % 32][ci % 8], then [groups * cpg] floats: the inverse scales
 * (vido_slam_amd/nets/ops.py::pack_gconv3x3_h).  Activations must be finite and below 65504 in magnitude (vido_conv1x1_range_flag otherwise).
 * vido_gconv3x3_h_supported: 1 when the kernel takes the shape (cpg_in == cpg_out in {32, 64}, W <= 93 / 45). */
int vido_gconv3x3_h_supported(int H, int W, int cpg_in, int cpg_out);
int vido_gconv3x3_h_bias_act(vido_ctx* ctx, const float* x, const void* w_packed, const float* bias, float* y, int groups, int cpg_in, int cpg_out, int H, int W, float slope);
/* ... and with 8 -> 8 or 16 -> 16 channels per group on v_mfma_f32_16x16x32_f16 (csrc/gconvhs.hip): `conv2` of the ResNeXt bottlenecks of layer1 / layer2, any W.  w_packed
 * (16-byte aligned): plane p of element (co, ci, dy, dx) of group g at [g][instruction i][p][16 b + co % cpg][ci % 8], where block b of instruction i is tap 3 dy + dx = 4 i + b
 * (8 per group, 3 instructions, rows 8 .. 15 zero) or tap 2 i + (b >> 1) of input channels 8 (b & 1) .. + 7 (16 per group, 5 instructions), taps >= 9 zero; then [groups * cpg]
 * floats: the inverse scales (vido_slam_amd/nets/ops.py::pack_gconv3x3_hs).  vido_gconv3x3_hs_supported: 1 when the kernel takes the shape (cpg_in == cpg_out in {8, 16},
 * W <= 957 / 445).  vido_debug_ghs_plan: test hook, see csrc/gconvhs.hip. */
int vido_gconv3x3_hs_supported(int H, int W, int cpg_in, int cpg_out);
int vido_gconv3x3_hs_bias_act(vido_ctx* ctx, const float* x, const void* w_packed, const float* bias, float* y, int groups, int cpg_in, int cpg_out, int H, int W, float slope);
int vido_debug_ghs_plan(int groups, int H, int W, int cpg_in, int cpg_out, int* out, long long* loaded);
/* ... with stride 2 (padding 1): the strided `conv2` of the first bottleneck of a ResNeXt stage (resnet.py:300-372 with STRIDE_IN_1X1 = False).  y [groups * cpg_out][(H + 1) / 2][W / 2];
 * W a multiple of 4, 8 / 16 / a multiple of 32 output channels per group (same w_packed), x 16-byte aligned, no in_bias.  vido_gconv3x3_s2_supported: 1 when the shape has a kernel. */
int vido_gconv3x3_s2_supported(int H, int W, int cpg_in, int cpg_out);
int vido_gconv3x3_s2_bias_act(vido_ctx* ctx, const float* x, const float* w_packed, const float* bias, float* y, int groups, int cpg_in, int cpg_out, int H, int W, float slope);
int vido_lfn_reg_front(vido_ctx* ctx, const float* im1, const float* im2, const float* flow, const float* mean, float scale, int B, int C, int H, int W, float* out, int out_channels);
int vido_lfn_reg_tail(vido_ctx* ctx, const float* dist, const float* flow, const float* wx, const float* bx, const float* wy, const float* by, int B, int K, int H, int W, float* out);
/* layers.ROIAlign forward — mask_rcnn/maskrcnn_benchmark/csrc/cuda/ROIAlign_cuda.cu:257-299.  rois [n,5] =
 * (batch index, x1, y1, x2, y2); out [n, C, pooled_h, pooled_w]. */
int vido_roi_align(vido_ctx* ctx, const float* feat, int B, int C, int H, int W, const float* rois, int n_rois,
                   float spatial_scale, int pooled_h, int pooled_w, int sampling_ratio, float* out, int on_device);
/* layers.nms(boxes, scores, thresh) — csrc/cuda/nms.cu:70-131 (IoU with the +1 convention, suppress when > thresh).
 * Host mode returns the kept ORIGINAL indices in ascending order like the reference.  Device mode: boxes already
 * sorted by descending score, keep_out/n_keep are device pointers receiving kept positions (ascending). */
int vido_nms(vido_ctx* ctx, const float* boxes_xyxy, const float* scores, int n, float thresh, int32_t* keep_out,
             int32_t* n_keep, int on_device);
/* The per-class NMS loop of the box head (modeling/roi_heads/box_head/inference.py:96-118: layers.nms once per class) in one
 * pass: boxes with different `groups` never suppress each other.  Conventions as vido_nms. */
int vido_nms_grouped(vido_ctx* ctx, const float* boxes_xyxy, const float* scores, const int32_t* groups, int n, float thresh,
                     int32_t* keep_out, int32_t* n_keep, int on_device);
/* Device-only batched NMS (layers.nms semantics per segment): the five per-level NMS calls of the RPN (modeling/rpn/inference.py:106-113), or the per-class
 * loop of the box head with `groups`, as ONE pair of launches without a host round trip.  boxes [total,4] DEVICE, segments back to back, each sorted by descending
 * score; seg_off / seg_n DEVICE int32 [n_seg]; max_n >= every segment length.  keep_out [n_seg, max_n]: kept positions relative to the segment start, ascending,
 * padded with -1; n_keep [n_seg].  Enqueues on the adopted stream (vido_set_stream), synchronises nothing. */
int vido_nms_segments(vido_ctx* ctx, const float* boxes_xyxy, const int32_t* groups, const int32_t* seg_off, const int32_t* seg_n, int n_seg, int max_n, int total,
                      float thresh, int32_t* keep_out, int32_t* n_keep);
/* Pooler.forward (modeling/poolers.py:97-121: LevelMapper, one ROIAlign per FPN level, scatter back by index) in one launch: feat[l] DEVICE [1,C,H[l],W[l]] f32,
 * boxes [n,4] x1 y1 x2 y2, level [n] in 0..3 (the LevelMapper's result, computed by the caller), out [n,C,pooled_h,pooled_w]. */
int vido_roi_align_fpn(vido_ctx* ctx, const float* const feat[4], const int H[4], const int W[4], const float scale[4], int C, const float* boxes, const int32_t* level,
                       int n, int pooled_h, int pooled_w, int sampling_ratio, float* out);
/* The layout the ROI-Align kernel reads: [B][C][H][W] -> [B][H][W][C] (DEVICE, f32).  ROIAlign_cuda.cu:15-122 gives every thread one output element and four scattered
 * 4-byte gathers per sample from channel-planar maps; this build reads channels-last (lanes across channels: one coalesced 256-byte load per tap and 64 channels). */
int vido_nchw_to_nhwc(vido_ctx* ctx, const float* src, int B, int C, int H, int W, float* dst);
/* vido_roi_align_fpn with CHANNELS-LAST maps feat[l] = [H[l]][W[l]][C] (vido_nchw_to_nhwc once per frame; the box and the mask pooler share the copies). */
int vido_roi_align_fpn_nhwc(vido_ctx* ctx, const float* const feat[4], const int H[4], const int W[4], const float scale[4], int C, const float* boxes, const int32_t* level,
                            int n, int pooled_h, int pooled_w, int sampling_ratio, float* out);
/* ... of the first *n_live boxes only (see vido_mask_logit_select_n). */
int vido_roi_align_fpn_nhwc_n(vido_ctx* ctx, const float* const feat[4], const int H[4], const int W[4], const float scale[4], int C, const float* boxes, const int32_t* level,
                              int n, int pooled_h, int pooled_w, int sampling_ratio, float* out, const int32_t* n_live);
/* ---- The local-BA window resident on the device between frames (vido-slam_amd/csrc/bawin.hip).  The reference re-assembles the graph of
 * Optimizer::PartialBatchOptimization from the Map on every call (Optimizer.cc:56-94, 276-350).  Here a ring of the last frames' static features stays on the device:
 * vido_bawin_push_frame sends one frame's rows (Get3DinCamera measurement, world point, index of the previous frame's feature it continues: Map::vpFeatSta / vfDepSta /
 * vp3DPointSta / vnAssoSta), vido_bawin_set_labels the tracklet-label changes ((frame, feature, tracklet, position) quads: Map::vnTrkSta / vnPosSta), vido_bawin_solve assembles
 * the window's graph on the device exactly like the Map walk does (observations in (frame, feature) order, landmark ids in order of first appearance, chains that start before
 * the window dropped), solves it in place and writes the refined landmarks back into the ring.  prob: cameras (n_cam = N - start), odometry factors, prior, weights and LM
 * parameters as for vido_ba_optimize; its observation / point fields are ignored.  vido_bawin_read_points: one stored frame's world points (f32 [n][3]).
 * Order of the label quads: they apply in the order given, within one call and across calls, so when a (frame, feature) pair occurs more than once the LAST quad holds.
 * Quads of a negative frame, of a frame that is not (or no longer) in the ring, or of a feature >= that frame's count are ignored; vido_bawin_push_frame resets the labels
 * of the slot it fills. */
int vido_bawin_create(vido_ctx* ctx, int cap_frames, int cap_features);
int vido_bawin_push_frame(vido_ctx* ctx, int frame, int n, const double* meas, const float* xyz, const int32_t* asso);
int vido_bawin_set_labels(vido_ctx* ctx, int n, const int32_t* quads);
int vido_bawin_solve(vido_ctx* ctx, int start, int N, vido_ba_problem* prob, vido_ba_result* res, int32_t* n_obs_out, int32_t* n_pt_out);
int vido_bawin_read_points(vido_ctx* ctx, int frame, int n, float* xyz_out);
/* ---- The detector's selection logic between its convolutions, device-side with fixed shapes (vido-slam_amd/csrc/detpost.hip).  Keys are (score bits << 32) | ~index, so a
 * descending key order is the reference's stable descending sort (ties -> lower index).
 * vido_rpn_select: RPNPostProcessor.forward_for_single_feature_map without the NMS (modeling/rpn/inference.py:73-105) for all FPN levels in one launch: sigmoid(objectness),
 *   the K = pre_nms_top_n best anchors of every level (anchors counted (y, x, a)), BoxCoder(1,1,1,1).decode + clip_to_image.  logits[l] [A,h,w], deltas[l] [4A,h,w] DEVICE;
 *   cell_anchors [n_levels][A][4] HOST; boxes_out [n_levels*K, 4], scores_out [n_levels*K] (-1 = padding row), n_out [n_levels] DEVICE.
 * vido_rpn_merge: select_over_all_levels (test branch, :125-159) after vido_nms_segments: the n_final best kept boxes over all levels.
 * vido_det_class_sort / vido_det_select: PostProcessor.filter_results (modeling/roi_heads/box_head/inference.py:96-137) around the per-class NMS: score threshold + descending
 *   order per class with decoded, clipped boxes; then the detections_per_img rule (threshold = k-th largest kept score, the reference's kthvalue) and the detections in
 *   (class, proposal) order in `cap` fixed slots; n_det (DEVICE) = the count the reference returns.  scratch: DEVICE, >= (nc + 1) int32. */
int vido_rpn_select(vido_ctx* ctx, int n_levels, const float* const* logits, const float* const* deltas, const int* h, const int* w, const int* stride, const float* cell_anchors,
                    int A, int K, int img_w, int img_h, float* boxes_out, float* scores_out, int32_t* n_out);
int vido_rpn_merge(vido_ctx* ctx, const float* boxes, const float* scores, const int32_t* keep, const int32_t* cnt, int n_levels, int K, int post_nms_top_n, int n_final,
                   float* out_boxes, float* out_scores, int32_t* n_valid);
int vido_det_class_sort(vido_ctx* ctx, const float* prob, const float* deltas, const float* proposals, const float* objectness, int N, int nc, float thresh, const float weights[4],
                        int img_w, int img_h, float* seg_boxes, int32_t* order, int32_t* seg_n);
int vido_det_select(vido_ctx* ctx, const float* prob, const float* seg_boxes, const int32_t* order, const int32_t* keep, const int32_t* cnt, int N, int nc, int detections_per_img, int cap,
                    int32_t* scratch, float* out_boxes, float* out_scores, int64_t* out_labels, int32_t* n_det);
/* Masker(threshold 0.5, padding 1).forward (modeling/roi_heads/mask_head/inference.py:87-160, per detection on the host in the reference) fused with the node's
 * label image (src/run_mask_rcnn.py:112-118: blank_mask += mask * class_index): masks [n,1,M,M] f32, boxes [n,4] f32 in the output image, labels [n] i64,
 * all DEVICE, detections in the order the node adds them; out [H,W] u8 = (sum over detections of pasted mask * class index) mod 256. */
int vido_mask_label_image(vido_ctx* ctx, const float* masks, const float* boxes, const int64_t* labels, int n, int M, int padding, float thresh, int H, int W, uint8_t* out);
/* ... for a list whose slots behind *n_live (DEVICE int32 word read by the kernel, clamped to [0, n]; NULL: none) all have label 0, as the static head's ordered list has:
 * the walk over the list stops at the count; the image is the same. */
int vido_mask_label_image_n(vido_ctx* ctx, const float* masks, const float* boxes, const int64_t* labels, int n, int M, int padding, float thresh, int H, int W, uint8_t* out,
                            const int32_t* n_live);
/* Masker + INSTANCE image: same inputs as vido_mask_label_image (device pointers; detections in the caller's priority order, highest first).
 * out[y,x] = id_base + 1 + (index of the FIRST detection with labels[i] != 0 whose pasted mask probability at (x,y) > thresh), 0 if none: the footprint of every
 * detection is the one vido_mask_label_image adds its class to, overlaps go to the earlier detection instead of summing.  labels[i] == 0 (an unused slot of the
 * static head) is skipped and still consumes its id, so id - id_base - 1 is the slot index.  area_out [n] i32 (may be NULL): pixels each detection owns in `out`
 * (cleared by the call).  id_base_dev: DEVICE int32 word read by the kernel (NULL: 0), so a captured graph follows a base that changes per frame; its owner keeps
 * n + id_base <= 255 (the sum is stored in u8).  n + id_base > 255 is refused (VIDO_E_CAPACITY) where the base is known to the host (NULL: n > 255; a device word:
 * n > 255 as well, the largest n any base admits); n == 0 clears out.  Enqueues on the adopted stream, no host synchronisation. */
int vido_mask_instance_image(vido_ctx* ctx, const float* masks, const float* boxes, const int64_t* labels, int n, int M, int padding, float thresh, int H, int W,
                             const int32_t* id_base_dev, uint8_t* out, int32_t* area_out);
/* BoxCoder(weights).decode(deltas [n,4k], boxes [n,4]) — modeling/box_coder.py:52-95. */
int vido_box_decode(vido_ctx* ctx, const float* deltas, const float* boxes, int n, int k, const float weights[4],
                    float* out, int on_device);

/* ---- Initial model: seeded P3P-RANSAC (Tracking::GetInitModelCam / GetInitModelObj, Tracking.cc:1965-1970, 2068-2073:
 * cv::solvePnPRansac(pre_3d, cur_2d, K, 0, ..., 500, 0.4, 0.98, inliers, SOLVEPNP_P3P)).  pts3d [n*3] f32 (previous frame,
 * world), pts2d [n*2] f32 (current keypoints); T_out row-major 4x4 world->camera; inlier_mask[n] may be NULL.
 * All max_iters hypotheses are scored in parallel; OpenCV's adaptive early stop is replayed on the counts.
 * DEVIATION from cv::solvePnPRansac: OpenCV refits the winning model on its inlier set before returning (solvepnp.cpp, the final solvePnP over the inliers); this entry
 * returns the winning minimal-sample P3P pose itself.  Both reference call sites hand the pose straight to PoseOptimizationFlow2Cam / PoseOptimizationFlow2, which
 * re-optimise it over the same inliers, so only the optimiser's starting point differs; the sampling sequence (counter-based RNG) also differs from cv::RNG by design. */
int vido_pnp_ransac(vido_ctx* ctx, const float* pts3d, const float* pts2d, int n, double fx, double fy, double cx, double cy,
                    int max_iters, double reproj_err, double confidence, uint64_t seed, double T_out[16], uint8_t* inlier_mask,
                    int32_t* n_inliers);

/* All dynamic objects of a frame in one pair of launches and ONE synchronisation (Tracking::Track loops GetInitModelObj over the objects, Tracking.cc:1192-1228):
 * problem p has n[p] points pts3d[p] / pts2d[p], seed seeds[p]; T_out [n_prob][16], inlier_mask[p] (may be NULL) [n[p]], n_inliers [n_prob].  Results are identical to
 * n_prob calls of vido_pnp_ransac. */
int vido_pnp_ransac_batch(vido_ctx* ctx, int n_prob, const float* const* pts3d, const float* const* pts2d, const int32_t* n, double fx, double fy, double cx, double cy,
                          int max_iters, double reproj_err, double confidence, const uint64_t* seeds, double* T_out, uint8_t* const* inlier_mask, int32_t* n_inliers);

/* ---- Host-side bookkeeping stages of the tracker on flat arrays (no device work, no ctx; vido-slam_amd/csrc/trackhost.cpp) ---------------------------------
 * What the C++ facade's Tracking / Frame methods of the same names run; exported so that hosts in other languages and the parity tests can call them. */
typedef struct vido_host_maps { const int32_t* mask; const float* depth; const float* flow; int32_t width, height; } vido_host_maps;   /* mSegMap / mDepthMap / mFlowMap */
/* Frame::UndistortKeyPoints (Frame.cc:603-633): cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK) — five fixed-point iterations of the Brown model;
 * K = (fx, fy, cx, cy), dist = (k1, k2, p1, p2, k3); k1 == 0: copy (Frame.cc:605-609). */
/* Frame::UnprojectStereo* / ObtainFlowDepth* with addnoise = 1 (Frame.cc:706-716 ...): the depth with ONE draw of a fresh cv::RNG(seed) added,
 * z + gaussian(z*z / (725*0.5) * 0.15); seed 0 = time(NULL) as the reference.  Host function (cv::RNG's multiply-with-carry + ziggurat restated; OpenCV side unpinned). */
float vido_depth_noise(float z, unsigned seed);
int vido_undistort_points(const float* xy, int n, const float K[4], const float dist[5], float* xy_out);
/* The rectification map of one camera for vido_rectify: for every pixel (u, v) of the rectified view, the raw pixel that shows the same ray, in 1/256 px (defined by
 * tests/refimpl/stereo_rectify_np.py; EXACT equality: the library is built without contraction).  K = (fx, fy, cx, cy) of the raw camera, dist = (k1, k2, p1, p2, k3),
 * R 3 x 3 row-major from raw-camera to rectified coordinates (OpenCV's R1 / R2, ORB-SLAM's LEFT.R), P = (fx', fy', cx', cy') of the rectified camera.  Each operation is
 * one IEEE double operation in this order, nothing fused:
 *   x = (u - cx') / fx';  y = (v - cy') / fy'
 *   X = R00 x + R10 y + R20;  Y = R01 x + R11 y + R21;  W = R02 x + R12 y + R22                (R transposed times (x, y, 1))
 *   xn = X / W;  yn = Y / W;  r2 = xn xn + yn yn;  rad = 1 + ((k3 r2 + k2) r2 + k1) r2
 *   xd = xn rad + (2 p1 xn yn + p2 (r2 + 2 xn xn));  yd = yn rad + (p1 (r2 + 2 yn yn) + 2 p2 xn yn)
 *   us = fx xd + cx;  vs = fy yd + cy;  mx = floor(us 256 + 0.5);  my = floor(vs 256 + 0.5)
 * W <= 0, a value that is not finite, or |mx| or |my| >= 2^30: both entries INT32_MIN ("no source").  map_out int32 [dst_h][dst_w][2], x first; inside_out [dst_h*dst_w]
 * = vido_rectify's inside for a src_w x src_h source, NULL ok; *inside_count_out = their count, NULL ok.  Host only: no context, no GPU call.  VIDO_E_INVALID for a NULL
 * parameter array or map_out, sizes outside 16 .. 4095, parameters that are not finite and fx, fy, fx', fy' <= 0. */
int vido_rectify_map(const double K[4], const double dist[5], const double R[9], const double P[4], int src_w, int src_h, int dst_w, int dst_h,
                     int32_t* map_out, uint8_t* inside_out /* NULL ok */, int32_t* inside_count_out /* NULL ok */);
/* Tracking::RenewFrameInfo, static part (Tracking.cc:2973-3075): the inliers TM_sta (indices into stat_xy = mvStatKeys, -1 = rejected) that still pass the mask /
 * depth <= 40 / flow tests, then top-up from sample_xy (= mvKeys) in stride-20 passes, skipping samples closer than 1 px to a kept inlier, until max_num.
 * Element k of the result: src_out[k] = index into stat_xy (inlier_out[k] >= 0) or into sample_xy (inlier_out[k] == -1), inlier_out[k] (nStaInlierID),
 * flow_out[2k..] (mvFlowNext).  *n_out = count (VIDO_E_CAPACITY if > cap). */
int vido_renew_static(const vido_host_maps* maps, const float* stat_xy, int n_stat, const int32_t* TM_sta, int n_tm, const float* sample_xy, int n_sample,
                      int max_num, int32_t* src_out, int32_t* inlier_out, float* flow_out, int cap, int32_t* n_out);
/* Tracking::RenewFrameInfo, object part (Tracking.cc:3116-3270).  obj_xy / obj_label: mvObjKeys / vObjLabel of the current frame (n_obj_pts); per tracked object i:
 * inlier ids inl_ids[inl_off[i] .. inl_off[i+1]) (vnObjInlierID), obj_stat (bObjStat), sem_position (nSemPosition), mod_label (nModLabel); tmp_*: the dense samples
 * of this frame set aside by GrabImageRGBD (mvTmpObjKeys / Depth / SemObjLabel / FlowNext / Corres).  Outputs = the new mvObjKeys, mvObjDepth, vSemObjLabel,
 * mvObjFlowNext, mvObjCorres, nDynInlierID, vObjLabel. */
int vido_renew_objects(const vido_host_maps* maps, const float* obj_xy, const int32_t* obj_label, int n_obj_pts,
                       int n_objects, const int32_t* inl_off, const int32_t* inl_ids, const uint8_t* obj_stat, const int32_t* sem_position, const int32_t* mod_label,
                       const float* tmp_xy, const float* tmp_depth, const int32_t* tmp_sem, const float* tmp_flow, const float* tmp_corr, int n_tmp, int max_num_obj,
                       float* keys_out, float* depth_out, int32_t* sem_out, float* flow_out, float* corr_out, int32_t* inlier_out, int32_t* label_out, int cap, int32_t* n_out);
/* The same two stages for maps that live on the DEVICE (the in-process network -> tracker hand-over): instead of whole host maps they take the map
 * values AT the candidate points — mask / depth / flow at ((int)x, (int)y) of every point of the list, gathered on the device (vido_gather_point_samples).  Entries of
 * points outside the image are never read.  vido_renew_static / vido_renew_objects sample their host maps and call these. */
typedef struct vido_point_samples { const int32_t* mask; const float* depth; const float* flow; } vido_point_samples;   /* [n], [n], [2n] */
int vido_renew_static_sampled(int width, int height, const float* stat_xy, int n_stat, const vido_point_samples* stat_samples, const int32_t* TM_sta, int n_tm,
                              const float* sample_xy, int n_sample, const vido_point_samples* sample_samples, int max_num,
                              int32_t* src_out, int32_t* inlier_out, float* flow_out, int cap, int32_t* n_out);
int vido_renew_objects_sampled(int width, int height, const float* obj_xy, const int32_t* obj_label, int n_obj_pts, const vido_point_samples* obj_samples,
                               int n_objects, const int32_t* inl_off, const int32_t* inl_ids, const uint8_t* obj_stat, const int32_t* sem_position, const int32_t* mod_label,
                               const float* tmp_xy, const float* tmp_depth, const int32_t* tmp_sem, const float* tmp_flow, const float* tmp_corr, int n_tmp, int max_num_obj,
                               float* keys_out, float* depth_out, int32_t* sem_out, float* flow_out, float* corr_out, int32_t* inlier_out, int32_t* label_out, int cap, int32_t* n_out);
/* Tracking::DynObjTracking (Tracking.cc:1670-1912): groups the n object points by semantic label, drops objects mostly on the image border / static (scene flow) /
 * far / smaller than 150 points (obj_label is updated in place: -1 outlier, 0 static, else the track id), and assigns track ids from the last frame's objects
 * (last_sem_position / last_obj_stat / last_mod_label, n_last) or from *max_id.  Result: n_objects objects, points of object i = obj_ids[obj_off[i] .. obj_off[i+1]),
 * mod_label_out (nModLabel), sem_position_out (nSemPosition). */
int vido_dyn_obj_tracking(const int32_t* sem_label, int32_t* obj_label, const float* obj_xy, const float* obj_depth, const float* flow3d, const int32_t* last_sem_label, int n,
                          const int32_t* last_sem_position, const uint8_t* last_obj_stat, const int32_t* last_mod_label, int n_last, int rows, int cols,
                          float sf_mg_thres, float sf_ds_thres, float th_depth_obj, int f_id, int32_t* max_id,
                          int32_t* obj_off, int32_t* obj_ids, int32_t* mod_label_out, int32_t* sem_position_out, int max_objects, int32_t* n_objects);

/* Tracking::GetStaticTrack / GetDynamicTrackNew (Tracking.cc:2514-2720) through the facade's INCREMENTAL store (Map::UpdateTracklets, one association row per call like
 * Tracking::Track): row i belongs to frame i+1, TM[row_off[i] + j] = feature of frame i matched by its feature j (-1: none), labels (dynamic store; NULL = static store)
 * the per-feature object labels.  Tracklet t = (frame, feature) pairs pairs[2*trk_off[t] .. 2*trk_off[t+1]); obj_id[t] (dynamic).  owner_trk / owner_pos (may be NULL):
 * for every feature of every frame (concatenated), the tracklet of length >= 3 that owns it and its position in it, -1 if none. */
int vido_tracklets_incremental(int n_rows, const int32_t* row_off, const int32_t* row_n, const int32_t* TM, const int32_t* labels, int n_feat0,
                               int32_t* trk_off, int32_t* pairs, int32_t* obj_id, int32_t* owner_trk, int32_t* owner_pos, int cap_trk, int cap_pairs, int32_t* n_trk);

/* ---- The whole per-frame pipeline behind one C handle ---------------------------------------------------------------------------
 * VIDO_SLAM::System (System.h:72-114) for hosts that bind C instead of C++ (ctypes / cgo / JNI): System::System() + Init(yaml, RGBD)
 * (System.cc:23-48), TrackRGBD (System.cc:51-63 -> Tracking::GrabImageRGBD, Tracking.cc:283-782 -> Track(), :1081-1509) and
 * SaveResultsIJRR2020 (System.cc:80-240).  Errors that the C++ facade throws come back as VIDO_E_* + vido_system_last_error.
 * One live system per process, like the reference (Frame's statics, Frame.cc:26-30). */
typedef struct vido_system vido_system;
typedef struct vido_system_stats {          /* of the last vido_system_track_rgbd call */
    int32_t frame_id, n_keypoints, n_static, n_static_inliers, n_objects, n_object_points, ba_window;
    int32_t mask_propagated;                 /* Mask.PropagateMissing: 1 — 1 when this frame came without a mask and took the previous frame's, propagated (vido_frame_propagate_mask); else 0 */
    float ms_total;                          /* TrackRGBD wall time */
    float ms_update_mask, ms_frame;          /* Tracking::UpdateMask; Frame::Frame (cvtColor + ORB + lists) + hand-over gathers */
    float ms_cam_pose, ms_obj_tracking, ms_obj_motion, ms_renew;   /* the reference's all_timing[1..4] (Tracking.cc:1120-1324); obj_motion = sum over objects */
    float ms_local_ba;                       /* Map::fLBA_time (Tracking.cc:1436-1451) */
    float ms_wait_inputs;                    /* vido_system_track_rgbd_device only: host time spent waiting for the producer's ready event (the networks of this frame) — inside ms_total,
                                                outside every stage time above */
    float ms_orb, ms_lists;                  /* inside ms_frame: the extractor call (cvtColor + pyramid + FAST + quadtree + rBRIEF, keypoints on the host) | Frame's static / object lists */
} vido_system_stats;
int         vido_system_create(const char* settings_yaml, vido_system** out);
void        vido_system_destroy(vido_system* sys);
const char* vido_system_last_error(const vido_system* sys);      /* NULL sys: error of the last failed vido_system_create */
/* im: u8 interleaved, `channels` 1 (gray), 3 or 4 (BGR[A], or RGB[A] when the settings say Camera.RGB: 1), tight rows; depth f32 (raw sensor
 * units; REWRITTEN IN PLACE with the pre-scaled depth like the reference does to the caller's Mat, Tracking.cc:299-322); flow f32 x2; mask i32;
 * all width*height, host memory, alive until the NEXT call returns (the reference keeps shallow references, Tracking.cc:343-345, 777-780).
 * n_image: StopFrame = n_image - 1.  Tcw_out: row-major 4x4 world->camera pose of this frame (identity for the first).
 * Settings key Mask.PropagateMissing: 1 (default 0): `mask` (here, and mask_dev of the device form) may be NULL on every frame but the first of a sequence; the frame's mask is
 * then the previous frame's, warped through the previous frame's flow with the nearer pre-scaled depth winning a collision (vido_frame_propagate_mask), before any list is
 * built from it; vido_system_stats.mask_propagated reports it.  With the key at 0 a NULL mask is VIDO_E_INVALID as before.
 * Settings keys Mask.SplitInstances: 1 (default 0) and Mask.MinInstanceArea (default 1): on every frame that arrives WITH a mask, the tracker's own copy of the mask is
 * split into its 8-connected components of equal value with at least that many pixels (vido_frame_split_mask, at most 127 per frame, in anchor order) after the upload
 * and before any list is built from it, so that the objects of one class in a class image (the reference node's sum of mask * class index, a dataset's semantic mask)
 * are tracked separately.  The id base alternates 0 / 127 per split frame (Tracking::UpdateMask repaints a lost label under its last-frame value); a propagated frame is
 * not split and keeps its source's ids.  The caller's mask buffer is never written (with zero-copy maps the split goes into a tracker-owned buffer that the slot adopts).
 * vido_system_mask_split_stats reads the frame's counters.  With the key at 0 nothing changes. */
int         vido_system_track_rgbd(vido_system* sys, const uint8_t* im, int channels, int width, int height, float* depth, const float* flow,
                                   const int32_t* mask, double timestamp, int n_image, float Tcw_out[16]);
/* The same with the image (u8, 1 / 3 / 4 interleaved channels) and the three maps already RESIDENT ON THE DEVICE (plain device pointers; depth is rescaled in place on the
 * device): the in-process replacement of the reference's three service round trips (src/realtime_demo/src/run_vido.cc:57-171 -> :229-235).  Nothing is uploaded, no map is
 * downloaded; ready_event (hipEvent_t, may be NULL) orders the tracker's stream behind the producer of the buffers. */
/* zero_copy != 0: vido_system_track_rgbd_device ADOPTS the three map buffers instead of copying them into the tracker's slots (vido_frame_upload on_device = 2): the caller
 * keeps the maps of a frame alive and untouched until the call AFTER the next one has returned (a ring of >= 3 frames; pipeline.EndToEnd's has 4).  Default 0. */
int         vido_system_set_zero_copy_maps(vido_system* sys, int zero_copy);
/* The ORB extraction of the NEXT vido_system_track_rgbd_device call's image, put on the tracker's stream now (it needs nothing but the image: a pipeline calls this while it
 * still waits for the networks of the frame); image_ready_event (hipEvent_t or NULL) orders it behind the image's upload.  The track call for the same pointer and size then
 * only collects.  Same thread as the track calls; the image stays untouched until that call has returned. */
int         vido_system_prefetch_image_device(vido_system* sys, const void* im_dev, int channels, int width, int height, void* image_ready_event);
int         vido_system_track_rgbd_device(vido_system* sys, const void* im_dev, int channels, int width, int height, float* depth_dev, const float* flow_dev,
                                          const int32_t* mask_dev, void* ready_event, double timestamp, int n_image, float Tcw_out[16]);
int         vido_system_get_stats(const vido_system* sys, vido_system_stats* out);
/* Verify.Descriptor: 1: static points of the last frame whose seed descriptor was compared with the frame at the flow-predicted position
 * (n_checked: those with a distance, i.e. a seed and a position outside the extractor's edge margin) and how many of them exceeded Verify.MaxHamming (n_rejected).
 * Both 0 with the option off.  (A call of its own: vido_system_stats keeps the layout existing callers see.) */
int         vido_system_get_verify_stats(const vido_system* sys, int* n_checked, int* n_rejected);
/* Mask.SplitInstances: 1 — the counters of the last frame's split: components found, dropped for Mask.MinInstanceArea, left out beyond 127, kept.  Zeros when the frame was
 * not split (the key at 0, or a propagated frame).  (A call of its own: vido_system_stats keeps the layout existing callers see.) */
int         vido_system_mask_split_stats(const vido_system* sys, int32_t out[4]);
/* Debug read of the same frame's per-point state, index-aligned with the frame's static list (any array may be NULL): xy [2n] the position that was checked, prev_xy [2n]
 * the last frame's point it came from, xyl [3n] = lrintf(xy / scale[level]) and the seed's level (-1 x 3: no seed), dist [n] (-1: no evidence), rejected [n], seed_desc [32n].
 * *n_out = n (0 with the option off or before the second frame); VIDO_E_CAPACITY if n > cap. */
int         vido_system_get_verify_points(const vido_system* sys, float* xy, float* prev_xy, int32_t* xyl, int32_t* dist, uint8_t* rejected, uint8_t* seed_desc, int cap, int* n_out);
/* Verify.Recover: 1 (needs Verify.Descriptor: 1): the static points the verification has just rejected are searched among the frame's own static
 * keypoints with vido_hamming_match_window (one call per frame, unique = 1; keys Verify.RecoverRadius / RecoverLevelTol / RecoverMaxHamming / RecoverRatio); a re-found
 * point moves onto its keypoint and is no longer rejected, so vido_system_get_verify_stats' n_rejected counts what STAYS rejected.  n_tried: the points searched on the last
 * frame, n_recovered: those re-found.  Both 0 with the option off. */
int         vido_system_get_recover_stats(const vido_system* sys, int* n_tried, int* n_recovered);
/* Debug read of the same frame's per-point state, index-aligned with vido_system_get_verify_points (any array may be NULL): status [n] (-1: not searched, else the op's
 * status, 0 = re-found), idx [n] the matched entry of the train list (-1: none), match_xy [2n] its position ((-1, -1): none), dist / dist2 [n] (-1: none), after [5n] per
 * point x, y, depth and the last frame's flow x, y as the step left them (what the pose stages read).  The train list of the frame's call — the frame's static candidate
 * list as Frame::Frame built it — comes back as train_xy [2 nt], train_level [nt], train_desc [32 nt], train_depth [nt], so that a caller can recompute the call.
 * *n_out = n, *n_train_out = nt (both 0 with the option off or before the second frame); VIDO_E_CAPACITY if n > cap or nt > train_cap. */
int         vido_system_get_recover_points(const vido_system* sys, int32_t* status, int32_t* idx, float* match_xy, int32_t* dist, int32_t* dist2, float* after, int cap, int* n_out,
                                           float* train_xy, int32_t* train_level, uint8_t* train_desc, float* train_depth, int train_cap, int* n_train_out);
/* Verify.ObjectPatch (default 0): counts of the last tracked frame's dense object points — n_checked (textured on both sides: accepted or rejected), n_rejected (taken off
 * their object before the scene flow), n_no_texture (kept for lack of evidence).  All 0 with the key off.  vido_system_stats keeps its layout. */
int         vido_system_get_object_verify_stats(const vido_system* sys, int* n_checked, int* n_rejected, int* n_no_texture);
/* Debug read of the same frame's per-point state, index-aligned with the object points the frame carried over from the last one (any array may be NULL): xyl [n*3] where
 * each was evaluated (level 0), sums [n*3] and status [n] as vido_orb_patch_points returned them, prev_xy [n*2] the last frame's point, ref_patch [n*64] the last frame's
 * patch it was compared with.  *n_out = the number of points (0 with the key off or on a frame that verified nothing); VIDO_E_CAPACITY if cap is smaller. */
int         vido_system_get_object_verify_points(const vido_system* sys, int32_t* xyl, int32_t* sums, int32_t* status, float* prev_xy, uint8_t* ref_patch, int cap, int* n_out);
/* Verify.ObjectRecover (default 0; needs Verify.ObjectPatch: 1): of the last tracked frame, n_tried = the object points the patch verification rejected and the search
 * looked for, n_recovered = those put back on their object at a re-found pixel (they no longer count in n_rejected of vido_system_get_object_verify_stats).  Both 0 with
 * the key off.  vido_system_stats keeps its layout. */
int         vido_system_get_object_recover_stats(const vido_system* sys, int* n_tried, int* n_recovered);
/* Debug read of the same step, index-aligned with vido_system_get_object_verify_points (any array may be NULL): status [n] of vido_orb_patch_search (-2: the point was
 * not searched), dxy [n*2], sums [n*3], second [n*2] as the call returned them (0 where not searched); gather [n*2] = depth, label the frame's maps hold at the re-found
 * pixel (-1 -1 where status != 0); after [n*6] = x, y, depth, label, last frame's flow x, y of every point as the step left them.  With xyl and ref_patch of
 * vido_system_get_object_verify_points a caller can recompute the call.  *n_out = n (0 with the key off or on a frame that verified nothing); VIDO_E_CAPACITY if cap is
 * smaller. */
int         vido_system_get_object_recover_points(const vido_system* sys, int32_t* status, int32_t* dxy, int32_t* sums, int32_t* second, float* gather, float* after, int cap, int* n_out);
/* Verify.ObjectRecoverSubpixel (default 0; needs Verify.ObjectRecover: 1): of the last tracked frame, n_tried = the object points the search re-found and
 * vido_orb_patch_refine was given, n_refined = those it aligned (status 0), which moved to a sub-pixel position before the gather.  Both 0 with the key off. */
int         vido_system_get_object_refine_stats(const vido_system* sys, int* n_tried, int* n_refined);
/* Debug read of the same step, index-aligned with vido_system_get_object_recover_points (any array may be NULL): status [n] of vido_orb_patch_refine (-2: the point was
 * not sent), q8 [n*2] and cost [n*2] as the call returned them (0 where not sent).  The call's centre is xyl + dxy of the two sibling read-backs at level 0, its reference
 * their ref_patch, so a caller can recompute it.  *n_out = n (0 with the key off or on a frame that verified nothing); VIDO_E_CAPACITY if cap is smaller. */
int         vido_system_get_object_refine_points(const vido_system* sys, int32_t* q8, int64_t* cost, int32_t* status, int cap, int* n_out);
int         vido_system_save_results(vido_system* sys, const char* prefix);
/* the vido_ctx the system's tracker runs on (NULL before the first frame): lets a caller share the device / query timings */
vido_ctx*   vido_system_context(vido_system* sys);
/* The reference's addnoise = 1 depth noise (Frame.cc:711-716) is seeded with time(NULL): PoseOptimizationNew's result then differs from one wall-clock second to the next.
 * seed != 0 pins cv::RNG's seed for every later draw of this process (tests, reproducible runs); 0 restores the reference behaviour.  (C++ callers: detail::SetDepthNoiseSeed.) */
int         vido_system_set_depth_noise_seed(vido_system* sys, unsigned seed);

#ifdef __cplusplus
}
#endif
#endif
