"""In-process network -> tracker hand-off.

The reference's realtime demo (src/realtime_demo/src/run_vido.cc:57-171) asks three ROS services for the optical flow (TYPE_32FC2), the
depth (MONO16) and the instance mask (MONO8) of every frame: the image goes to each node over the wire, each node uploads it, downloads its
result and sends it back, and TrackRGBD uploads the three maps again.  Here the networks and the tracker share one device: the frame is
uploaded once, the three networks write device tensors, and `vido_frontend_batch` takes those buffers as they are (maps_on_device = 2: the
tracker's map slots alias the caller's tensors, which this object keeps alive for the two frames the tracker may still read them).
Nothing is quantised on the way except what the reference's interfaces quantise themselves (depth to 16 bit, mask to 8 bit), so the
front-end results are identical to the round trip through host arrays (tests/test_pipeline_gpu.py).
"""
import numpy as np
import torch

from . import nets as _nets
from .host import FrameFeatures


def bgr_to_gray(bgr):
    """cvtColor(BGR2GRAY) in 14-bit fixed point on the device: (B*1868 + G*9617 + R*4899 + 8192) >> 14 (Tracking.cc:327-340; same formula as
    the facade's to_gray)."""
    x = bgr.to(torch.int32)
    return ((x[..., 0] * 1868 + x[..., 1] * 9617 + x[..., 2] * 4899 + 8192) >> 14).to(torch.uint8).contiguous()


class NetFrontEnd:
    """RunNet + the Frame construction of the frame that follows (run_vido.cc:138-171, Frame.cc:41-230).

    push(bgr) -> None for the first frame, then a dict with the front-end lists of the frame (FrameFeatures.frontend_batch views: keypoints,
    descriptors, static candidates, dense object samples) plus `labels` (Mask R-CNN class indices) and `slot` (the tracker map slot the
    frame's depth / flow / mask now live in, for vido_gather_* / vido_update_mask)."""

    def __init__(self, ctx, frame_params, flow_net, depth_net, mask_net, mask_feed=(1088, 800), depth_feed=(192, 640), confidence=0.8, keep_raw=False):
        self.ctx = ctx; self.flow_net, self.depth_net, self.mask_net = flow_net, depth_net, mask_net
        self.ff = FrameFeatures(ctx, frame_params)
        self.mask_feed, self.depth_feed, self.confidence = mask_feed, depth_feed, confidence
        self.dev = next(flow_net.parameters()).device
        self.prev = None
        self.slot = 0
        self._hold = {}                    # slot -> tensors the tracker's slot aliases
        self.keep_raw, self.raw = keep_raw, None      # keep_raw: copies of the network outputs of the last frame (the tracker rescales the depth map in place)

    @torch.no_grad()
    def infer(self, prev_bgr, cur_bgr):
        """The three service calls of RunNet on device tensors: flow HxWx2 f32, depth HxW f32 (MONO16 values), mask HxW i32, labels."""
        flow = _nets.analyse_flow(self.flow_net, prev_bgr, cur_bgr)
        mask_u8, labels = _nets.analyse_image(self.mask_net, cur_bgr, feed=self.mask_feed, confidence=self.confidence)
        depth_u16 = _nets.analyse_depth(self.depth_net, cur_bgr, feed=self.depth_feed)
        return flow.contiguous(), depth_u16.to(torch.float32).contiguous(), mask_u8.to(torch.int32).contiguous(), labels

    @torch.no_grad()
    def push(self, bgr):
        cur = torch.as_tensor(np.ascontiguousarray(bgr, np.uint8)).to(self.dev, non_blocking=True)      # the only upload of the frame
        if self.prev is None:
            self.prev = cur
            return None
        # RunNet's queue entry: the CURRENT image with the flow of the pair (previous, current) and the depth / mask of the current image
        flow, depth, mask, labels = self.infer(self.prev, cur)
        gray = bgr_to_gray(cur)
        if self.keep_raw: self.raw = (flow.clone(), depth.clone(), mask.clone())
        h, w = gray.shape
        torch.cuda.current_stream().synchronize()          # the tracker runs on the ctx's own stream
        slot = self.slot
        out = self.ff.frontend_batch(slot, (gray.data_ptr(), 1, h, w, h * w, w), depth.data_ptr(), flow.data_ptr(), mask.data_ptr(), alias=True)
        self._hold[slot] = (gray, depth, flow, mask)        # alive until the slot is overwritten (two frames later)
        self.slot ^= 1
        self.prev = cur
        out = dict(out); out["labels"] = labels; out["slot"] = slot
        return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# The whole realtime chain of the reference (src/realtime_demo/src/run_vido.cc): RunNet (:131-171, three service calls per frame) feeding
# RunVidoSlam (:229-235, System::TrackRGBD), with the two stages overlapped: the networks of frame k+1 run while frame k is tracked.
import queue as _queue
import threading as _threading
import time as _time
import os as _os

# MIOpen user find-db recorded once on an MI355X with `bench.py --miopen-find` (MIOPEN_USER_DB_PATH pointing here): the measured best solver per convolution shape of the
# three nodes at their feed sizes.  With it the default immediate-mode path picks those solvers without searching (the search costs ~3.5 minutes of start-up; the
# heuristic pick without the db is 0.7 ms per frame slower).  Read by MIOpen when its handle is created, i.e. at the first convolution; an explicit setting wins.
# The db is keyed to one MIOpen build (file name gfx950100.HIP.<major>_<minor>_<patch>_...): it is offered only when this process' MIOpen has that version, MIOpen
# writes new entries into the directory it is given, so it is given a private copy (build/miopen_db next to the library's objects, or under the temp directory when the
# package is read-only) and the shipped files stay as committed; a shipped file newer than its copy replaces it.  VIDO_NO_MIOPEN_DB=1 opts out.
_MIOPEN_DB = _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "miopen_db")
_MIOPEN_DB_COPY = _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "build", "miopen_db")


def _offer_miopen_db():
    if "MIOPEN_USER_DB_PATH" in _os.environ or _os.environ.get("VIDO_NO_MIOPEN_DB") or not _os.path.isdir(_MIOPEN_DB):
        return None
    try:
        import torch as _t
        v = int(_t.backends.cudnn.version() or 0)                # MIOpen's version on ROCm builds: major * 1e6 + minor * 1e3 + patch
    except Exception:
        return None
    tag = "HIP.%d_%d_%d_" % (v // 1000000, (v // 1000) % 1000, v % 1000)
    files = [f for f in _os.listdir(_MIOPEN_DB) if tag in f]
    if not files:
        return None
    import shutil, tempfile
    path = _MIOPEN_DB_COPY
    try:
        _os.makedirs(path, exist_ok=True)
    except OSError:
        pass
    if not (_os.path.isdir(path) and _os.access(path, _os.W_OK)):
        path = _os.path.join(tempfile.gettempdir(), "vido_slam_miopen_db_%d" % _os.getuid())
        _os.makedirs(path, exist_ok=True)
    for f in files:
        src, dst = _os.path.join(_MIOPEN_DB, f), _os.path.join(path, f)
        if not _os.path.exists(dst) or _os.path.getmtime(dst) < _os.path.getmtime(src):
            shutil.copy2(src, dst)
    _os.environ["MIOPEN_USER_DB_PATH"] = path
    return path


_offer_miopen_db()


class InstanceIds:
    """Instance ids that persist across frames (csrc/maskassoc.hip): what an external detector, NetNodes(stable_ids=True) or a test drives.  Owns two
    int32 HxW label images (the one handed over last and the one being written), the association state (int32 [768]: cursor, class and lost count per id) and the
    counters of the last detected() call (stats, int32 [4]: matched, fresh, lost, left out).  Everything is enqueued on torch's current stream; nothing waits for the device.

    detected(inst_mask, classes, flow=None): inst_mask int32 HxW at id base 0 (value 1 + slot), classes int64 [n <= 127] (0 = unused slot), flow float32 HxWx2 from the
    previous frame into this one, or None on the first frame of a sequence.  The image handed over last is warped through the flow (HipOps.mask_propagate) and associated
    with inst_mask (HipOps.mask_associate): an instance takes over the id it overlaps with IoU > 1/2, any other gets a fresh id; an id the detector misses stays in the
    image at its flow-predicted place for `hold` detector frames.  propagated(flow): a frame without a detector run, the last image warped through the flow.  Both return
    the frame's mask, one of the two images: valid until the next call.  depth (both calls; default None): the metric depth of the PREVIOUS frame, float32 HxW — the frame
    the warped image belongs to — handed to mask_propagate, which then gives a pixel two labels land on to the nearer source.  mask is the image handed over last (writable: the next call starts from it),
    classes_by_id an int64 [255] device tensor refreshed in stream order by detected(): [id - 1] is the class of id, 0 when the id is neither live nor held.

    from_classes(class_mask, flow=None, connectivity=8, min_area=1): the same for a CLASS label image (the reference node's sum of mask * class index, a dataset's semantic
    mask; int32 HxW, > 0 a class): it is split into its connected components of equal value (HipOps.mask_components, csrc/maskcc.hip, INTEGRATION.md §34: id base 0, at
    most 127, in the order of their first pixel) into an image the object owns, and that image and its classes go through detected().  split_stats (int32 [4]: found,
    dropped for area, left out, kept) are the counters of the last split."""

    def __init__(self, ops, h, w, hold=0):
        import numbers as _numbers
        if isinstance(hold, bool) or not isinstance(hold, _numbers.Integral) or hold < 0:
            raise ValueError("hold: an integer >= 0, not %r" % (hold,))
        self.ops, self.h, self.w, self.hold = ops, int(h), int(w), int(hold)
        dev = torch.device("cuda", ops.ctx.cfg.device)
        self._img = [torch.zeros((self.h, self.w), dtype=torch.int32, device=dev) for _ in range(2)]
        self._i = 0
        self.state = torch.zeros((768,), dtype=torch.int32, device=dev)
        self.stats = torch.zeros((4,), dtype=torch.int32, device=dev)
        self.classes_by_id = torch.zeros((255,), dtype=torch.int64, device=dev)
        # the first call of either op allocates in its context (key plane, count table): here, so that a frame — or a capture — never does
        ops.mask_propagate(self._img[0], torch.zeros((self.h, self.w, 2), dtype=torch.float32, device=dev), out=self._img[1])
        ops.mask_associate(None, self._img[1], self.state, n=0, hold=self.hold, out=self._img[0], stats=self.stats)
        # from_classes' instance image, its classes and counters; the first mask_components call allocates the context's planes: here as well
        self._inst = torch.zeros((self.h, self.w), dtype=torch.int32, device=dev)
        self._inst_classes = torch.zeros((127,), dtype=torch.int64, device=dev)
        self.split_stats = torch.zeros((4,), dtype=torch.int32, device=dev)
        ops.mask_components(self._img[0], out=self._inst, classes=self._inst_classes, stats=self.split_stats)

    @property
    def mask(self):
        return self._img[self._i]

    def reset(self):
        """A new sequence: no ids live, the cursor back at the start, both images empty."""
        self.state.zero_(); self.stats.zero_(); self.classes_by_id.zero_(); self._i = 0      # (mask is the tensor it was after construction)
        for m in self._img:
            m.zero_()

    def detected(self, inst_mask, classes, flow=None, depth=None):
        last, other = self._img[self._i], self._img[self._i ^ 1]
        if flow is None:
            out = self.ops.mask_associate(None, inst_mask, self.state, classes=classes, hold=self.hold, out=other, stats=self.stats)
            self._i ^= 1
        else:
            self.ops.mask_propagate(last, flow, depth=depth, out=other)
            out = self.ops.mask_associate(other, inst_mask, self.state, classes=classes, hold=self.hold, out=last, stats=self.stats)
        self.classes_by_id.copy_(self.state[257:512], non_blocking=True)
        return out

    def from_classes(self, class_mask, flow=None, connectivity=8, min_area=1):
        self.ops.mask_components(class_mask, connectivity=connectivity, min_area=min_area, id_base=0, cap=127, out=self._inst, classes=self._inst_classes, stats=self.split_stats)
        return self.detected(self._inst, self._inst_classes, flow)

    def propagated(self, flow, depth=None):
        out = self.ops.mask_propagate(self._img[self._i], flow, depth=depth, out=self._img[self._i ^ 1])
        self._i ^= 1
        return out


class NetNodes:
    """The three network nodes (flow_net / mono_depth2 / mask_rcnn ROS services, run_vido.cc:142-157) resident on one device, fp32 like
    the reference.  infer(prev_bgr, cur_bgr) enqueues the three forwards — the detector on the caller's stream, LiteFlowNet and MonoDepth2 back to back on ONE side stream
    (streams="flow+depth", the default since round 3: with every network a graph and no host synchronisation left in the detector, the two chains fill each other's
    small-kernel phases: 13.8 ms per frame against 16.8 ms with everything on one stream; a stream per network gives 14.4, LiteFlowNet and MonoDepth2 on a stream EACH 19.0;
    round 2 had measured any overlap slower because its detector head still ran eagerly); the tracker of the previous frame overlaps with all of it (EndToEnd) — and returns device tensors in the tracker's input types (run_vido.cc:28-37: depth MONO16 -> CV_32F,
    mask MONO8 -> CV_32SC1, flow 32FC2).  optimize: frozen batch norms folded into the convolutions + fused HIP epilogues
    (nets/fuse.py); graphs: the static-shape parts (all of LiteFlowNet and MonoDepth2 incl. their resize wrappers, Mask R-CNN's backbone +
    FPN + RPN head) are captured into hipGraphs.

    on_range: what a frame whose split-fp16 launches left fp16's range (|x| >= 65504, an infinity or a NaN: its outputs are not valid) gets.  "raise" (default): the caller's
    check_conv1x1_range raises, the sequence stops.  "recompute": infer() ends each frame with a latch of both contexts' range flags into that frame's own words
    (vido_range_latch, in stream order), and the caller recomputes a tripped frame's networks in fp32's range (recompute(); infer_checked() does it all; EndToEnd does it
    before the frame is tracked).  Only LiteFlowNet (its context) and the detector launch split-fp16 kernels; MonoDepth2 shares the detector's context and launches none.

    detect_every = N (an integer >= 1; default 1: the detector runs on every frame and nothing below applies): the detector runs on calls 0, N, 2N, ...; on the calls in
    between it is not launched, and the frame's mask is the previous frame's mask warped through this call's flow (HipOps.mask_propagate, csrc/maskprop.hip) on the
    detector's stream behind the flow's event, into one of two buffers the nodes own (a graph's static output is overwritten by the next replay).  No depth is passed
    (unless propagate_bf is set, below): the
    networks' depth is a normalised disparity, not metric, so where two objects land on one pixel the SMALLER LABEL wins, not the nearer object.  A propagated frame returns
    the last detector frame's labels and reports no detections (so no overflow); label_mode="instance": the id base advances per detector RUN, a propagated frame keeps its
    source's ids and base (self.id_base).  carried_mask is the image the next propagated frame starts from — a device tensor an external detector or a test may write;
    detector_runs / propagated_frames count, last_propagated tells which the last call was.  Not with on_range="recompute": a flow recomputed after the fact would
    invalidate the masks already propagated through it (open).

    stable_ids = True (needs label_mode="instance"; stable_hold = h >= 0): instance ids that persist across frames (InstanceIds, csrc/maskassoc.hip).
    The detector paints at id base 0 on EVERY frame (id_base stays 0, the graph's id word is never switched); on a detector frame its stream waits for the flow's event,
    as it already does on propagated frames, and the mask handed over is InstanceIds.detected(detector image, slot classes, flow) — an instance keeps the id of the
    object it overlaps (IoU > 1/2) in the previous mask warped through the flow, a new one takes the next of 1..254, one the detector misses stays for stable_hold detector
    frames; on a propagated frame it is InstanceIds.propagated(flow).  labels is InstanceIds.classes_by_id (int64 [255]): labels[id - id_base - 1] still reads an id's
    class.  carried_mask is the image handed over last, also with detect_every = 1.  An overflow of the static head keeps the static head's slots: the redo through
    the dynamic head would rank the detections anew after the ids were given, so it is skipped and only counted in det_overflows.  Not with skip_detector (infer() raises
    ValueError: a frame without a detector image would leave the carried image and the id state behind the sequence).  Not with on_range="recompute", for
    the reason that applies to detect_every > 1: every later mask descends from the flows already used.  With stable_ids = False nothing of this exists: the launches,
    the id bases and the outputs are those of before.

    flow_source = "dis" (default "net": LiteFlowNet, and nothing below applies): the flow is HipOps.dis_flow of the two BGR frames (csrc/disflow.hip, INTEGRATION.md §39;
    dis_params: a dict of coarsest / iters / max_shift_q8 / min_eig, the op's defaults otherwise) on the flow context and the flow stream, captured into g_flow like
    LiteFlowNet.  LiteFlowNet is not constructed (flow_net is None).  The op is all-integer: the flow half of the range words stays 0 and recompute() leaves the flow alone.
    detect_every, stable_ids and EndToEnd take the tensor as they take LiteFlowNet's.

    dis_consistency (with flow_source = "dis" only; default None: off, and the flow function is exactly the one above): True, or a dict that may hold alpha_q10 and beta_q16
    (the op's defaults otherwise: 10 and 32768, i.e. alpha 0.01 and beta 0.5 px^2) — the flow is HipOps.dis_flow_pair's MARKED flow: both directions
    from one pyramid build, and every vector whose backward flow does not bring it back, or whose target leaves the image, is NaN.  The front end drops a NaN vector by
    failing comparisons, and vido_mask_propagate defines a NaN source as not voting — which is what an occluded pixel should do: it has no counterpart in the next frame,
    so it carries no label there.  flow_status: the uint8 HxW status image of the last frame (0 consistent, 1 inconsistent, 2 leaves the image, 3 not a flow), valid in
    stream order with the flow; None when off.  Anything else raises ValueError before anything is built, and so does dis_consistency with flow_source = "net".

    depth_source = "stereo" (default "net": MonoDepth2, and nothing below applies): the depth is HipOps.stereo_sgm of the frame and its rectified right view
    (csrc/stereosgm.hip; stereo_params: a dict of max_disp / p1 / p2 / uniqueness / lr_tol, the op's defaults otherwise) on the detector's context and
    the depth stream, captured into g_depth like MonoDepth2.  MonoDepth2 is neither constructed nor launched (depth_net is None).  infer() then needs right_bgr, and the
    depth it returns is the op's disp_out: the disparity in pixels where the match is valid, -1 elsewhere.  That image is metric once the tracker knows the rig: with the
    KITTI ChooseData code (facade.cpp:876: the depth image is a disparity), DepthMapFactor: 1 and Camera.bf = fx * baseline in the settings, the front end computes
    bf / disparity metres and treats -1 as "no depth".  stereo_status: the uint8 HxW status image of the last frame (0 valid, 1 not unique, 2 left-right, 3 zero
    disparity), valid in stream order with the depth; None with "net".  Anything else raises ValueError before anything is built, and so do stereo_params with
    depth_source = "net" and a right_bgr handed to infer() under "net".

    stereo_filter (with depth_source = "stereo" only; default None: off, and the depth function is exactly the one above): True, or a dict that may hold max_diff_q4 and
    min_region (the op's defaults otherwise: 16 and 10) — SGM is followed by HipOps.stereo_filter (csrc/stereofilter.hip) in the same capture: a valid
    pixel whose region of similar disparity holds fewer than min_region pixels is dropped.  infer() returns the filtered disparity, and stereo_status shows 4 on speckles.

    propagate_bf (default None: off) = fx x baseline, a float > 0; needs depth_source = "stereo" and detect_every > 1 or stable_ids = True.  The filter op also writes
    the collision depth of the frame (bf / disparity metres where the status is 0, FLT_MAX elsewhere; without stereo_filter the op runs with min_region = 1: it makes the
    plane and launches no labelling) into one of two planes the nodes alternate between, and EVERY mask_propagate call of the nodes, the one inside InstanceIds included,
    receives the PREVIOUS frame's plane as its depth — the frame the carried mask belongs to: where two labels land on one pixel the nearer source wins, and a source
    without a measured depth loses to one with.  On the first frame of a sequence no depth is passed.  Any other combination raises ValueError before anything is built.

    rectify (default None: off, and nothing anywhere changes) = dict(left=cal, right=cal or None, raw_size=(h, w)) for cameras that deliver RAW frames (lens distortion,
    a rig that is not aligned): cal = dict(K=(fx, fy, cx, cy) of the raw camera, dist=(k1, k2, p1, p2[, k3]), R=3 x 3 from raw-camera to rectified coordinates, P=(fx',
    fy', cx', cy') of the rectified camera) as calibration files give them; raw_size defaults to the nodes' size.  The nodes build the maps once (host.rectify_map), keep
    them on the device and offer rectify_frames(raw_left, raw_right=None, out_left=None, out_right=None) — HipOps.rectify (csrc/stereorectify.hip),
    one launch for both cameras — and rect_inside, the bool HxW image of the left view's pixels that have a raw source.  infer() still takes RECTIFIED frames;
    EndToEnd.push() takes the raw ones.  A `right` calibration needs depth_source = "stereo", and depth_source = "stereo" with rectify needs `right`.  With stereo depth,
    every pixel outside rect_inside leaves infer() with disparity -1, shows stereo_status 5 ("outside the rectified view") and holds FLT_MAX in the collision depth
    (propagate_bf): the black border of a rectified image matches the other view's border perfectly and must not become depth.  Unknown keys, a missing or malformed
    calibration and sizes outside 16..4095 raise ValueError before anything is built."""

    RANGE_MODES = ("raise", "recompute")
    ID_BASES = (0, 127)                                               # label_mode="instance": the id base of even / odd frames (ids 1..127 / 128..254)

    def __init__(self, ctx, height=480, width=640, optimize=True, graphs=True, streams="flow+depth", miopen_find=False, seed=1,
                 mask_feed=(1088, 800), depth_feed=(192, 640), confidence=0.8, calibrate_scores=True, static_detector=True, on_range="raise", label_mode="class",
                 detect_every=1, stable_ids=False, stable_hold=0, flow_source="net", dis_params=None, dis_consistency=None, depth_source="net", stereo_params=None,
                 stereo_filter=None, propagate_bf=None, rectify=None):
        self._check_detect_every(detect_every, on_range)              # (first: nothing is built for a bad argument)
        self.rectify = self._check_rectify(rectify, depth_source, height, width)
        self.rect_inside = None; self._rect_maps = None; self._rect_outside = None
        self.depth_source, self.stereo_params = self._check_depth_source(depth_source, stereo_params)
        self.stereo_filter, self.propagate_bf = self._check_stereo_filter(stereo_filter, propagate_bf, depth_source, detect_every, stable_ids)
        self.stereo_status = None
        self._coll = None; self._coll_static = None; self._coll_i = 0; self._coll_have = False      # propagate_bf: the collision-depth planes (the last one written: _coll_i)
        self.flow_source, self.dis_params = self._check_flow_source(flow_source, dis_params)
        self.dis_consistency = self._check_dis_consistency(dis_consistency, flow_source)
        self.flow_status = None
        self._check_stable_ids(stable_ids, stable_hold, label_mode, on_range)
        self.stable_ids = bool(stable_ids); self.stable_hold = int(stable_hold); self._ids = None
        self.detect_every = int(detect_every)
        self.detector_runs = self.propagated_frames = 0; self.last_propagated = False; self._calls = 0
        if on_range not in self.RANGE_MODES:
            raise ValueError("on_range: one of %s, not %r" % (self.RANGE_MODES, on_range))
        if label_mode not in _nets.maskrcnn.LABEL_MODES:
            raise ValueError("label_mode: one of %s, not %r" % (_nets.maskrcnn.LABEL_MODES, label_mode))
        self.label_mode = label_mode
        self.on_range = on_range
        self.range_recomputes = {"flow": 0, "detector": 0}           # networks recomputed in fp32's range (on_range="recompute")
        self._range_words = None                                      # infer()'s words when the caller passes none (pinned int32 [flow context, detector context])
        self.last_range = None
        self.ctx, self.h, self.w = ctx, height, width
        self.mask_feed, self.depth_feed, self.confidence = mask_feed, depth_feed, confidence
        if miopen_find:
            torch.backends.cudnn.benchmark = True                      # MIOpen find: measure the applicable solvers once per layer shape
        dev = torch.device("cuda", ctx.cfg.device)
        self.dev = dev
        # the nodes run concurrently on three streams: ops that use the ctx's device scratch (correlation partials, NMS bit matrix, paste table) must not share
        # it across streams, so the flow node gets its own ctx; the depth node's fused epilogue uses no scratch and shares the mask node's
        from .host import Context as _Context
        self.ctx2 = _Context(device=ctx.cfg.device, width=ctx.cfg.width, height=ctx.cfg.height, max_batch=1)
        self.ops = ops = _nets.HipOps(ctx)                # Mask R-CNN (ROI-Align, NMS, box decode, paste) + MonoDepth2 epilogues
        self.ops_flow = _nets.HipOps(self.ctx2)           # LiteFlowNet (cost volume, epilogues)
        self.flow_net = None if self.flow_source == "dis" else _nets.fill_deterministic(
            _nets.LiteFlowNet(self.ops_flow.correlation, epilogue=self.ops_flow.bias_act_, warp=self.ops_flow.backwarp, fused=None if _os.environ.get("VIDO_LFN_NO_FUSED") else self.ops_flow,
                              pair_batch=not _os.environ.get("VIDO_LFN_NO_PAIR_BATCH")), seed).eval().to(dev)
        self.depth_net = None if self.depth_source == "stereo" else _nets.fill_deterministic(_nets.MonoDepth2(), seed + 1).eval().to(dev)
        self.mask_net = _nets.fill_maskrcnn(_nets.MaskRCNN(ops), seed + 2).eval().to(dev)
        if label_mode == "instance" and self.mask_net.config.detections_per_img > self.ID_BASES[1]:
            raise ValueError("label_mode='instance': detections_per_img = %d, each id range holds %d" % (self.mask_net.config.detections_per_img, self.ID_BASES[1]))
        # the instance ids' base: constants per parity, and the word the detector's graph reads (set from them in stream order before each replay); id_base: the frame in flight
        self._id_bases = torch.tensor(self.ID_BASES, dtype=torch.int32, device=dev) if label_mode == "instance" else None
        self._id_word = torch.zeros((1,), dtype=torch.int32, device=dev) if label_mode == "instance" else None
        self.id_base = 0; self._frames = 0
        # detect_every > 1: the two mask buffers propagated frames alternate between (carried_mask: the one the next propagated frame reads), the labels and label count of
        # the last detector frame, and a zero for the detection count of propagated frames.  The first mask_propagate call allocates the context's key plane: here, not in a frame
        self._carry = None; self._carry_i = 0; self._last_labels = None; self._last_nlab = None
        if self.stable_ids:                                           # (its first calls allocate the key plane and the count table in the detector's context: here, not in a frame)
            self._ids = InstanceIds(ops, height, width, hold=self.stable_hold)
            self._zero_count = torch.zeros((), dtype=torch.int32, device=dev)
        self._set_detect_every(self.detect_every)
        # random-init detector: un-saturate the class scores so that the reference's detections_per_img cap binds (see nets/weights.py); a synthetic textured frame
        self.score_scale = 1.0
        if calibrate_scores:
            g = torch.Generator(device="cpu").manual_seed(seed + 3)
            cal = torch.randint(0, 256, (height // 8, width // 8, 3), generator=g, dtype=torch.uint8).repeat_interleave(8, 0).repeat_interleave(8, 1).to(dev)
            with torch.no_grad():
                self.score_scale = _nets.calibrate_detector_scores(self.mask_net, _nets.maskrcnn.image_to_feed(cal, dev, mask_feed, ops=ops))
        self.folded = 0
        if optimize:
            self.folded = (0 if self.depth_net is None else _nets.fold_batchnorm(self.depth_net, ops)) + _nets.fold_batchnorm(self.mask_net, ops)
        # streams: False = the three networks back to back on the caller's stream; True = one stream each; "depth" = MonoDepth2 alone on a side stream (its ~120 launches of a
        # few microseconds leave most CUs idle: next to the detector's convolutions they cost next to nothing, while three full networks side by side evict each other's L2 sets)
        if isinstance(streams, str):                              # e.g. "depth", "flow", "flow+depth" (those networks share ONE side stream), "flow,depth" (a side stream each)
            side = {}; self.streams = [None, None, None]
            for grp in streams.split(","):                          # a trailing "!" puts the group's stream at high priority
                hi = grp.endswith("!"); grp = grp.rstrip("!")
                st_ = torch.cuda.Stream(device=dev, priority=-1 if hi else 0)
                for name in grp.split("+"):
                    self.streams[{"flow": 0, "depth": 1, "det": 2}[name.strip()]] = st_
        else:
            self.streams = [torch.cuda.Stream(device=dev) for _ in range(3)] if streams else None
        self.g_flow = self.g_depth = self.g_trunk = self.g_det = None
        self.graph_error = None
        self.last_counts = None
        self.det_overflows = 0                                        # frames whose detection count exceeded the static head's slots (redone through the dynamic head)
        ex = torch.zeros((height, width, 3), dtype=torch.uint8, device=dev)
        if self.dis_consistency is not None:                          # both directions and the check; the status image is the nodes' own buffer, written by eager calls and replays alike
            self.flow_status = torch.zeros((height, width), dtype=torch.uint8, device=dev)
            self._flow_fn = lambda a, b: self.ops_flow.dis_flow_pair(a, b, status=self.flow_status, **self.dis_params, **self.dis_consistency)
        elif self.flow_source == "dis":                               # the op on the flow context (its first call of the size, below, grows the context's scratch: before any capture)
            self._flow_fn = lambda a, b: self.ops_flow.dis_flow(a, b, **self.dis_params)
        else:
            self._flow_fn = lambda a, b: _nets.analyse_flow(self.flow_net, a, b)
        self._depth_fn = lambda a: _nets.analyse_depth(self.depth_net, a, feed=self.depth_feed, ops=ops).to(torch.float32)
        dex = [ex]
        if self.rectify is not None:                                  # the maps, once: host code in float64, then device tensors for every rectify_frames call
            from .host import rectify_map as _rectify_map
            rh, rw = self.rectify["raw_size"]
            maps = [None if c is None else _rectify_map(c["K"], c["dist"], c["R"], c["P"], (rw, rh), (width, height)) for c in (self.rectify["left"], self.rectify["right"])]
            self._rect_maps = [None if m is None else torch.from_numpy(m[0]).to(dev) for m in maps]
            self.rect_inside = torch.from_numpy(maps[0][1]).to(dev).bool()
            self._rect_outside = ~self.rect_inside
        if self.depth_source == "stereo":                             # the op on (left, right); the status image is the nodes' own buffer, written by eager calls and replays alike
            self.stereo_status = torch.zeros((height, width), dtype=torch.uint8, device=dev)
            self._depth_fn = lambda a, b: ops.stereo_sgm(a, b, status=self.stereo_status, **self.stereo_params)
            if self.stereo_filter is not None or self.propagate_bf is not None:      # SGM, then the filter on its q4 / status: the status in place, the collision depth when asked for
                self._stereo_q4 = torch.zeros((height, width), dtype=torch.int32, device=dev)
                if self.propagate_bf is not None:                     # the plane the (captured) op writes, and the two the frames alternate between
                    self._coll_static = torch.zeros((height, width), dtype=torch.float32, device=dev)
                    self._coll = [torch.zeros((height, width), dtype=torch.float32, device=dev) for _ in range(2)]
                filt = self.stereo_filter if self.stereo_filter is not None else dict(min_region=1)
                def _stereo_fn(a, b):
                    disp = ops.stereo_sgm(a, b, q4=self._stereo_q4, status=self.stereo_status, **self.stereo_params)
                    return ops.stereo_filter(self._stereo_q4, self.stereo_status, out=disp, status_out=self.stereo_status, depth=self._coll_static, bf=self.propagate_bf, **filt)
                self._depth_fn = _stereo_fn
            if self.rectify is not None:                              # no depth outside the rectified view: the verdicts of the op(s) above, then the border's own
                _inner = self._depth_fn
                def _inside_fn(a, b):
                    disp = _inner(a, b)
                    disp.masked_fill_(self._rect_outside, -1.0); self.stereo_status.masked_fill_(self._rect_outside, 5)
                    if self._coll_static is not None:
                        self._coll_static.masked_fill_(self._rect_outside, torch.finfo(torch.float32).max)
                    return disp
                self._depth_fn = _inside_fn
            dex = [ex, ex]                                            # (its first call of the size, below, grows the op's scratch: before any capture)
        self._trunk_fn = lambda a: self.mask_net.trunk(_nets.maskrcnn.image_to_feed(a, dev, self.mask_feed, ops=ops))
        # the whole detector with static shapes (nets/maskrcnn.py: heads_static / analyse_image_static): trunk + device-side RPN selection + box head + fixed-slot
        # post-processing + mask head + label image, no host synchronisation -> ONE hipGraph; returns (mask i32 HxW, labels [cap], n_labels, n_det)
        def _det_fn(a, id_word=None):                                   # id_word: an eager call for an earlier frame (recompute) names that frame's constant word
            feats, logits, deltas = self._trunk_fn(a)
            img, labels, n_lab, n_det = _nets.analyse_image_static(self.mask_net, feats, logits, deltas, (height, width), feed=self.mask_feed, confidence=self.confidence,
                                                                   label_mode=self.label_mode, id_base=self._id_word if id_word is None else id_word)
            return img.to(torch.int32), labels, n_lab.to(torch.int32), n_det.to(torch.int32)
        self._det_fn = _det_fn
        with torch.no_grad():
            for _ in range(2):                                          # first calls: MIOpen compiles / finds its kernels
                self._flow_fn(ex, ex); self._depth_fn(*dex); self._trunk_fn(ex)
            # the mask head's detection-count buckets: every batch size its convolutions will ever see is compiled now, not in the middle of a sequence
            mh = self.mask_net.roi_heads.mask
            feats = self.mask_net.trunk(_nets.maskrcnn.image_to_feed(ex, dev, self.mask_feed, ops=ops))[0][:4]
            for b in mh.buckets:
                mh(feats, torch.tensor([[10.0, 10.0, 200.0, 300.0]], device=dev).repeat(b, 1), torch.ones(b, dtype=torch.int64, device=dev))
            torch.cuda.synchronize()
            if graphs:
                try:
                    self.g_flow = _nets.Graphed(self._flow_fn, [ex, ex])
                    self.g_depth = _nets.Graphed(self._depth_fn, dex)
                    self.g_trunk = _nets.Graphed(self._trunk_fn, [ex])
                    if not _os.environ.get("VIDO_NO_MASK_GRAPHS"):
                        mh.capture_buckets(self.g_trunk.static_out[0][:4], _nets.Graphed)      # the mask head per detection-count bucket, over the trunk's static feature maps
                except Exception as e:                                  # capture is an optimisation: report, run eagerly
                    self.graph_error = "%s: %s" % (type(e).__name__, e)
                    self.g_flow = self.g_depth = self.g_trunk = None
                    torch.cuda.synchronize()
                if self.g_trunk is not None and static_detector and not _os.environ.get("VIDO_NO_DET_GRAPH"):
                    try:                                                # on its own: a failure here leaves the three graphs above in place (dynamic head after the trunk graph)
                        self._det_fn(ex); torch.cuda.synchronize()
                        self.g_det = _nets.Graphed(self._det_fn, [ex])
                    except Exception as e:
                        self.graph_error = "detector graph: %s: %s" % (type(e).__name__, e)
                        self.g_det = None
                        torch.cuda.synchronize()

    @torch.no_grad()
    def infer(self, prev_bgr, cur_bgr, range_words=None, right_bgr=None):
        """prev_bgr / cur_bgr: u8 HxWx3 device tensors; right_bgr: with depth_source="stereo" the rectified right view of cur_bgr, u8 HxWx3 (required; the depth returned
        is then the op's disparity image, see the class docstring), with "net" it must be None.  Returns (flow HxWx2 f32, depth HxW f32, mask HxW i32, labels, events): work enqueued on the caller's stream after
        this call sees the complete outputs (the caller's stream waits for the side stream's events); another stream or the host waits for the three events.
        label_mode="instance": the mask holds per-frame instance ids above this frame's id base (self.id_base: ID_BASES alternate frame by frame), labels[id - id_base - 1]
        is an id's class.
        range_words (pinned int32 [2], or on_range="recompute": NetNodes' own, valid until the next call; self.last_range names them): zeroed, then the frame's range flags
        of the flow context / the detector context are latched into words 0 / 1 on the caller's stream after the three events — they hold this frame's trips alone,
        readable on the host once the caller's stream has passed this point."""
        if self._ids is not None and getattr(self, "skip_detector", False):
            raise ValueError("stable_ids with skip_detector: a frame without a detector image would leave the carried image and the id state behind the sequence")
        if (right_bgr is None) == (self.depth_source == "stereo"):
            raise ValueError("right_bgr: required with depth_source='stereo' and only there (depth_source=%r, right_bgr %s)" % (self.depth_source, "missing" if right_bgr is None else "given"))
        cur = torch.cuda.current_stream()
        ss = [s or cur for s in self.streams] if self.streams else [cur, cur, cur]
        for s in ss:
            if s is not cur:
                s.wait_stream(cur)
        with torch.cuda.stream(ss[0]):
            flow = (self.g_flow or self._flow_fn)(prev_bgr, cur_bgr)
            e0 = torch.cuda.Event(); e0.record()
        with torch.cuda.stream(ss[1]):
            depth = (self.g_depth or self._depth_fn)(cur_bgr) if right_bgr is None else (self.g_depth or self._depth_fn)(cur_bgr, right_bgr)
            if self._coll is not None:                                  # this frame's collision depth, kept past the next call (the next frame's propagation reads it)
                self._coll[self._coll_i ^ 1].copy_(self._coll_static, non_blocking=True)
            e1 = torch.cuda.Event(); e1.record()
        # the depth the carried mask belongs to: the previous frame's plane (written on the depth stream a call ago; this call's streams wait for the caller's, which waited for it)
        prev_depth = self._coll[self._coll_i] if self._coll is not None and self._coll_have else None
        if self._coll is not None:
            self._coll_i ^= 1; self._coll_have = True
        det_frame = self.detect_every == 1 or self._calls % self.detect_every == 0
        self._calls += 1
        with torch.cuda.stream(ss[2]):
            if self._ids is not None:                                   # stable ids: base 0 on every frame, the word the graph reads is never switched
                first = self._calls == 1
            elif self.label_mode == "instance" and det_frame:           # this frame's id base, into the word the graph reads: a device-to-device copy in stream order, nothing waits
                self.id_base = self.ID_BASES[self._frames & 1]; self._frames += 1      # (per detector run: a propagated frame keeps its source's ids)
                self._id_word.copy_(self._base_word(self.id_base), non_blocking=True)
            if not det_frame and self._ids is not None:                 # stable ids: the image handed over last through this call's flow
                ss[2].wait_event(e0)
                mask, labels = self._ids.propagated(flow, depth=prev_depth), self._ids.classes_by_id
                self.last_counts = None if self._last_nlab is None else (self._last_nlab, self._zero_count)
            elif not det_frame:                                         # the previous frame's mask through this call's flow; the detector is not launched
                ss[2].wait_event(e0)
                dst = self._carry[self._carry_i ^ 1]
                self.ops.mask_propagate(self._carry[self._carry_i], flow, depth=prev_depth, out=dst)
                self._carry_i ^= 1
                mask, labels = dst, self._last_labels
                self.last_counts = None if self._last_nlab is None else (self._last_nlab, self._zero_count)
            elif getattr(self, "skip_detector", False):                   # the literal "flow+depth+track+local-BA" chain of BASELINE's metric text (bench.py extra.e2e_without_detector)
                if getattr(self, "_no_det", None) is None:
                    z = torch.zeros((), dtype=torch.int32, device=self.dev)
                    self._no_det = (torch.zeros((self.h, self.w), dtype=torch.int32, device=self.dev), torch.zeros((1,), dtype=torch.int64, device=self.dev), z, z.clone())
                mask, labels, n_lab, n_det = self._no_det
                self.last_counts = (n_lab, n_det)
            elif self.g_det is not None:                                # one graph replay, nothing synchronised: labels [cap] (0 = unused slot), counts stay on the device
                mask, labels, n_lab, n_det = self.g_det(cur_bgr)
                self.last_counts = (n_lab, n_det)
            else:                                                       # dynamic head: its data-dependent tail synchronises the host while the other two networks run
                mask_u8, labels = _nets.analyse_image(self.mask_net, cur_bgr, feed=self.mask_feed, confidence=self.confidence, trunk=self.g_trunk, **self._label_args())
                mask = mask_u8.to(torch.int32); self.last_counts = None
            self.last_propagated = not det_frame
            if det_frame and self._ids is not None:
                # the detector's per-frame ids -> ids that persist: behind the flow's event, the last mask is warped into this frame and associated with the detector's image
                if not first:
                    ss[2].wait_event(e0)
                if not torch.is_tensor(labels):
                    labels = torch.as_tensor(labels, dtype=torch.int64)
                mask = self._ids.detected(mask.contiguous(), labels.to(device=self.dev, dtype=torch.int64).contiguous(), None if first else flow, depth=None if first else prev_depth)
                labels = self._ids.classes_by_id
                self._last_nlab = None if self.last_counts is None else self.last_counts[0]
            if det_frame:
                self.detector_runs += 1
                if self._carry is not None:                             # the image the next propagated frame starts from (the graph's static output does not outlive the next replay)
                    self._carry[self._carry_i].copy_(mask, non_blocking=True)
                    self._last_labels = labels; self._last_nlab = None if self.last_counts is None else self.last_counts[0]
            else:
                self.propagated_frames += 1
            e2 = torch.cuda.Event(); e2.record()
        for s, e in zip(ss, (e0, e1, e2)):                          # the outputs are valid in stream order on the CALLER's stream, whatever queue produced them
            if s is not cur:
                cur.wait_event(e)
        if range_words is None and self.on_range == "recompute":
            if self._range_words is None:
                self._range_words = torch.zeros((2,), dtype=torch.int32).pin_memory()
            range_words = self._range_words
        self.last_range = range_words
        if range_words is not None:                                   # (the words' previous frame has been read: the caller's contract)
            range_words.zero_()
            self.ops_flow.range_latch(range_words[0:1]); self.ops.range_latch(range_words[1:2])
        return flow, depth, mask, labels, (e0, e1, e2)

    @torch.no_grad()
    def rectify_frames(self, raw_left, raw_right=None, out_left=None, out_right=None):
        """NetNodes(rectify=...): raw_left (and raw_right, when a right calibration was given: then required) u8 raw_h x raw_w x 3 device tensors -> the rectified frame, or
        the pair, u8 HxWx3 (out_left / out_right, or new tensors): what infer() takes.  One launch on the caller's stream, nothing is waited for."""
        if self.rectify is None:
            raise ValueError("rectify_frames: these nodes were built without rectify=")
        if (raw_right is None) != (self._rect_maps[1] is None):
            raise ValueError("rectify_frames: raw_right goes with a right calibration (rectify['right'] %s, raw_right %s)" % (
                "missing" if self._rect_maps[1] is None else "given", "missing" if raw_right is None else "given"))
        rh, rw = self.rectify["raw_size"]
        for name, t in (("raw_left", raw_left), ("raw_right", raw_right)):
            if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != (rh, rw, 3)):
                raise ValueError("rectify_frames: %s must be a u8 device tensor [%d, %d, 3]" % (name, rh, rw))
        return self.ops.rectify(raw_left, self._rect_maps[0], raw_right, self._rect_maps[1], out_left=out_left, out_right=out_right)

    RECTIFY_KEYS = ("left", "right", "raw_size")
    CAL_SIZES = {"K": (4,), "dist": (4, 5), "R": (9,), "P": (4,)}

    @classmethod
    def _check_rectify(cls, rectify, depth_source, height, width):
        """-> None, or dict(left=cal, right=cal or None, raw_size=(h, w)) with every calibration as float64 arrays (dist padded to five)"""
        if rectify is None:
            return None
        import numpy as _np
        if not isinstance(rectify, dict) or any(k not in cls.RECTIFY_KEYS for k in rectify) or rectify.get("left") is None:
            raise ValueError("rectify: None or a dict with `left` and keys among %s, not %r" % (cls.RECTIFY_KEYS, rectify))
        def cal(name, c):
            if not isinstance(c, dict) or set(c) != set(cls.CAL_SIZES):
                raise ValueError("rectify[%r]: a dict with exactly the keys %s, not %r" % (name, tuple(cls.CAL_SIZES), c))
            out = {}
            for k, sizes in cls.CAL_SIZES.items():
                try:
                    a = _np.asarray(c[k], _np.float64).ravel()
                except (TypeError, ValueError):
                    a = _np.zeros(0)
                if a.size not in sizes or not _np.isfinite(a).all():
                    raise ValueError("rectify[%r][%r]: %s finite numbers expected, not %r" % (name, k, " or ".join(str(n) for n in sizes), c[k]))
                out[k] = a
            out["dist"] = _np.concatenate([out["dist"], _np.zeros(5 - out["dist"].size)])
            if not (out["K"][0] > 0 and out["K"][1] > 0 and out["P"][0] > 0 and out["P"][1] > 0):
                raise ValueError("rectify[%r]: focal lengths > 0 expected" % name)
            return out
        left = cal("left", rectify["left"])
        right = None if rectify.get("right") is None else cal("right", rectify["right"])
        if right is not None and depth_source != "stereo":
            raise ValueError("rectify: a `right` calibration needs depth_source='stereo' (nothing else reads a right view)")
        if right is None and depth_source == "stereo":
            raise ValueError("rectify: depth_source='stereo' needs the `right` calibration too (SGM matches two rectified views)")
        raw = rectify.get("raw_size", (height, width))
        try:
            rh, rw = (int(v) for v in raw)
            ok = tuple(raw) == (rh, rw)
        except (TypeError, ValueError):
            ok = False
        if not ok or not all(16 <= v <= 4095 for v in (rh, rw, int(height), int(width))):
            raise ValueError("rectify: raw_size = (h, w) with sizes in 16..4095 expected, not %r (nodes %r x %r)" % (raw, height, width))
        return dict(left=left, right=right, raw_size=(rh, rw))

    DEPTH_SOURCES = ("net", "stereo")
    STEREO_PARAMS = ("max_disp", "p1", "p2", "uniqueness", "lr_tol")

    @classmethod
    def _check_depth_source(cls, depth_source, stereo_params):
        if depth_source not in cls.DEPTH_SOURCES:
            raise ValueError("depth_source: one of %s, not %r" % (cls.DEPTH_SOURCES, depth_source))
        if stereo_params is not None and (depth_source != "stereo" or not isinstance(stereo_params, dict) or any(k not in cls.STEREO_PARAMS for k in stereo_params)):
            raise ValueError("stereo_params: with depth_source='stereo', a dict with keys among %s, not %r" % (cls.STEREO_PARAMS, stereo_params))
        return depth_source, dict(stereo_params or {})

    STEREO_FILTER = ("max_diff_q4", "min_region")

    @classmethod
    def _check_stereo_filter(cls, stereo_filter, propagate_bf, depth_source, detect_every, stable_ids):
        """-> (None (off) or the filter's parameters as a dict (empty: the op's defaults), None (off) or bf as a float)"""
        import math as _math
        import numbers as _numbers
        filt = None
        if stereo_filter is not None:
            ok = stereo_filter is True or (isinstance(stereo_filter, dict) and all(
                k in cls.STEREO_FILTER and isinstance(v, _numbers.Integral) and not isinstance(v, bool) for k, v in stereo_filter.items()))
            if depth_source != "stereo" or not ok:
                raise ValueError("stereo_filter: with depth_source='stereo', None, True or a dict with integer values under keys among %s, not %r" % (cls.STEREO_FILTER, stereo_filter))
            filt = {} if stereo_filter is True else {k: int(v) for k, v in stereo_filter.items()}
            if not 0 <= filt.get("max_diff_q4", 0) <= 65535 or not 1 <= filt.get("min_region", 1) <= 1 << 24:
                raise ValueError("stereo_filter: max_diff_q4 in 0..65535 and min_region in 1..2^24 expected, not %r" % (stereo_filter,))
        bf = None
        if propagate_bf is not None:
            if isinstance(propagate_bf, bool) or not isinstance(propagate_bf, _numbers.Real) or not _math.isfinite(propagate_bf) or not propagate_bf > 0:
                raise ValueError("propagate_bf: a finite float > 0 (fx x baseline), not %r" % (propagate_bf,))
            if depth_source != "stereo" or not (detect_every > 1 or stable_ids):
                raise ValueError("propagate_bf needs depth_source='stereo' (a metric depth) and detect_every > 1 or stable_ids=True (a mask that is propagated)")
            bf = float(propagate_bf)
        return filt, bf

    FLOW_SOURCES = ("net", "dis")
    DIS_PARAMS = ("coarsest", "iters", "max_shift_q8", "min_eig")

    @classmethod
    def _check_flow_source(cls, flow_source, dis_params):
        if flow_source not in cls.FLOW_SOURCES:
            raise ValueError("flow_source: one of %s, not %r" % (cls.FLOW_SOURCES, flow_source))
        if dis_params is not None and (flow_source != "dis" or not isinstance(dis_params, dict) or any(k not in cls.DIS_PARAMS for k in dis_params)):
            raise ValueError("dis_params: with flow_source='dis', a dict with keys among %s, not %r" % (cls.DIS_PARAMS, dis_params))
        return flow_source, dict(dis_params or {})

    DIS_CONSISTENCY = ("alpha_q10", "beta_q16")

    @classmethod
    def _check_dis_consistency(cls, dis_consistency, flow_source):
        """None (off) or the check's parameters as a dict (empty: the op's defaults)"""
        import numbers as _numbers
        if dis_consistency is None:
            return None
        ok = dis_consistency is True or (isinstance(dis_consistency, dict) and all(
            k in cls.DIS_CONSISTENCY and isinstance(v, _numbers.Integral) and not isinstance(v, bool) for k, v in dis_consistency.items()))
        if flow_source != "dis" or not ok:
            raise ValueError("dis_consistency: with flow_source='dis', None, True or a dict with integer values under keys among %s, not %r" % (cls.DIS_CONSISTENCY, dis_consistency))
        cons = {} if dis_consistency is True else {k: int(v) for k, v in dis_consistency.items()}
        if not 0 <= cons.get("alpha_q10", 0) <= 1024 or not 0 <= cons.get("beta_q16", 0) <= 1 << 30:
            raise ValueError("dis_consistency: alpha_q10 in 0..1024 and beta_q16 in 0..2^30 expected, not %r" % (dis_consistency,))
        return cons

    @staticmethod
    def _check_detect_every(detect_every, on_range):
        import numbers as _numbers
        if isinstance(detect_every, bool) or not isinstance(detect_every, _numbers.Integral) or detect_every < 1:
            raise ValueError("detect_every: an integer >= 1, not %r" % (detect_every,))
        if detect_every > 1 and on_range == "recompute":
            raise ValueError("detect_every = %d with on_range='recompute': a flow recomputed after the fact would invalidate the masks already propagated through it" % detect_every)

    @staticmethod
    def _check_stable_ids(stable_ids, stable_hold, label_mode, on_range):
        import numbers as _numbers
        if not stable_ids:
            return
        if label_mode != "instance":
            raise ValueError("stable_ids needs label_mode='instance', not %r: ids that persist are instance ids" % (label_mode,))
        if on_range == "recompute":
            raise ValueError("stable_ids with on_range='recompute': a flow recomputed after the fact would invalidate the ids already carried through it")
        if isinstance(stable_hold, bool) or not isinstance(stable_hold, _numbers.Integral) or stable_hold < 0:
            raise ValueError("stable_hold: an integer >= 0, not %r" % (stable_hold,))

    def _set_detect_every(self, detect_every):
        """The constructor's set-up of the cadence (also tools/prof_detect_every.py, between sequences, so that one set of networks serves every cadence): a new sequence starts —
        the next infer() is a detector frame under id base 0.  Not part of the interface; never while frames are in flight."""
        self._check_detect_every(detect_every, self.on_range)
        self.detect_every = int(detect_every); self._calls = 0; self._frames = 0; self.id_base = 0; self.last_propagated = False
        self._coll_have = False                                       # (the first frame of a sequence passes no depth)
        if self._ids is not None:                                     # stable ids: InstanceIds owns the images; a new sequence starts with no id live
            self._ids.reset(); self._last_nlab = None
            return
        if self.detect_every > 1 and self._carry is None:
            self._carry = [torch.zeros((self.h, self.w), dtype=torch.int32, device=self.dev) for _ in range(2)]
            self._zero_count = torch.zeros((), dtype=torch.int32, device=self.dev)
            self.ops.mask_propagate(self._carry[0], torch.zeros((self.h, self.w, 2), dtype=torch.float32, device=self.dev), out=self._carry[1])
        elif self.detect_every == 1:
            self._carry = None; self._carry_i = 0; self._last_labels = None; self._last_nlab = None

    @property
    def carried_mask(self):
        """detect_every > 1: the int32 HxW device tensor the next propagated frame is warped from (the last frame's mask); writable in place.  None with detect_every = 1.
        stable_ids: the image handed over last (InstanceIds.mask), at any detect_every: the next frame, detector frame or not, is warped from it."""
        if self._ids is not None:
            return self._ids.mask
        return None if self._carry is None else self._carry[self._carry_i]

    def _base_word(self, id_base):
        """The constant device word that holds `id_base` (one of ID_BASES)."""
        i = self.ID_BASES.index(int(id_base))
        return self._id_bases[i:i + 1]

    def _label_args(self, id_base=None):
        """analyse_image's label arguments for a frame whose id base is `id_base` (None: the frame infer() saw last).  The dynamic head's list is not bounded by the slot
        count (score ties at the cut: the overflow redo): only the ID_BASES[1] highest scores get an id, so that either range holds them and the sequence goes on."""
        if self.label_mode != "instance":
            return {}
        return dict(label_mode="instance", id_base=self.id_base if id_base is None else int(id_base), max_instances=self.ID_BASES[1])

    @torch.no_grad()
    def recompute(self, prev_bgr, cur_bgr, flow=True, detector=True, id_base=None):
        """The networks of a frame whose split-fp16 launches left the range, again in fp32's range: eager forwards inside nets.range_safe (no split-fp16 launch; nothing a
        captured graph reads is replaced) on the caller's stream.  Returns {"flow": HxWx2 f32 or None, "detector": (mask HxW i32, labels, n_lab, n_det) or None}; n_lab /
        n_det are None after the dynamic head (no static detector).  The caller serialises it with infer() (the nodes' host-side state has one user at a time).
        id_base (label_mode="instance"): the id base infer() gave THAT frame (its self.id_base then); None: the last frame's."""
        out = {"flow": None, "detector": None}
        if flow and self.flow_source == "net":                        # (the integer flow op launches nothing whose range can be left: nothing to recompute)
            with _nets.range_safe(self.flow_net):
                out["flow"] = self._flow_fn(prev_bgr, cur_bgr).contiguous()
            self.range_recomputes["flow"] += 1
        if detector and not getattr(self, "skip_detector", False):
            with _nets.range_safe(self.mask_net):
                if self.g_det is not None:                              # the static head, eagerly (its trunk without the captured graph): the graph's output form
                    # (that frame's constant base word, not the graph's, which may already hold the next frame's)
                    mask, labels, n_lab, n_det = self._det_fn(cur_bgr, self._base_word(self.id_base if id_base is None else id_base) if self.label_mode == "instance" else None)
                    out["detector"] = (mask, labels, n_lab, n_det)
                else:
                    mask_u8, labels = _nets.analyse_image(self.mask_net, cur_bgr, feed=self.mask_feed, confidence=self.confidence, **self._label_args(id_base))
                    out["detector"] = (mask_u8.to(torch.int32), labels, None, None)
            self.range_recomputes["detector"] += 1
        return out

    @torch.no_grad()
    def infer_checked(self, prev_bgr, cur_bgr, right_bgr=None):
        """infer() for callers outside EndToEnd, with this frame's range check: infer, wait for the caller's stream, and when a context tripped raise (on_range="raise") or
        recompute the tripped networks (on_range="recompute", see recompute()).  Returns infer()'s tuple; its events are recorded after any recomputation."""
        if self._range_words is None:
            self._range_words = torch.zeros((2,), dtype=torch.int32).pin_memory()
        flow, depth, mask, labels, evs = self.infer(prev_bgr, cur_bgr, range_words=self._range_words, right_bgr=right_bgr)
        torch.cuda.current_stream().synchronize()
        hit_flow, hit_det = bool(self._range_words[0]), bool(self._range_words[1])
        if not (hit_flow or hit_det):
            return flow, depth, mask, labels, evs
        if self.on_range == "raise":
            raise RuntimeError("split-fp16: an activation of the frame left the range of the arithmetic (|x| >= 65504, an infinity or a NaN) on the %s context; the frame's "
                               "outputs are not valid — NetNodes(on_range=\"recompute\") recomputes such frames in fp32's range"
                               % " and ".join(n for n, h in (("flow", hit_flow), ("detector / depth", hit_det)) if h))
        r = self.recompute(prev_bgr, cur_bgr, flow=hit_flow, detector=hit_det)
        if r["flow"] is not None:
            flow = r["flow"]
        if r["detector"] is not None:
            mask, labels, n_lab, n_det = r["detector"]
            self.last_counts = None if n_lab is None else (n_lab, n_det)
        e = torch.cuda.Event(); e.record()
        return flow, depth, mask, labels, (e, e, e)

    def check_conv1x1_range(self):
        """The split-fp16 kernels (csrc/conv1x1.hip 1x1 and 2x2 transposed, conv3x3h.hip, fch.hip: the default arithmetic) take finite activations below 65504; a launch that
        met a larger one, an infinity or a NaN raised its context's range flag and its outputs are not valid.  Both contexts are read (and reset): the detector's (ops) and
        LiteFlowNet's (ops_flow: its 3x3 layers on conv3x3h.hip).  Called where a frame's networks are known to be complete; never seen with the networks' weights
        (activations of a few hundred)."""
        hit = [name for name, o in (("detector / depth", self.ops), ("flow", getattr(self, "ops_flow", None)))
               if o is not None and hasattr(o, "conv1x1_range_flag") and o.conv1x1_range_flag(reset=True)]      # (every flag read, so that every one is reset)
        if hit:
            raise RuntimeError("split-fp16: an activation left the range of the arithmetic (|x| >= 65504, an infinity or a NaN) on the %s context; the frame's outputs are not "
                               "valid — run with VIDO_CONV3X3_H=0 VIDO_NO_FC_H=1 VIDO_CONV1X1_ARITH=bf16x3 (fp32's range: the 3x3 and fully connected layers back on fp32 "
                               "kernels, the 1x1 ones on split-bf16)" % " and ".join(hit))

    @torch.no_grad()
    def redo_detector_if_overflowed(self, cur_bgr, n_det_host, range_safe=False, id_base=None):
        """The static head stores detections_per_img slots; score ties at the reference's kthvalue cut (box_head/inference.py:131-137) can leave more.  The caller reads
        n_det with the frame's hand-over and, in that (rare) case, recomputes the label image through the dynamic head (range_safe: a frame recomputed in fp32's range —
        eagerly inside nets.range_safe, without the trunk's graph).  id_base: as in recompute(); in instance mode the 127 highest scores get an id (an id range holds no more),
        the rest are left out of that frame's image."""
        cap = self.mask_net.config.detections_per_img
        if n_det_host <= cap:
            return None
        self.det_overflows += 1
        if self._ids is not None:                                     # stable ids: the ids were given to the static head's slots; the frame keeps them (class docstring)
            return None
        if range_safe:
            with _nets.range_safe(self.mask_net):
                mask_u8, labels = _nets.analyse_image(self.mask_net, cur_bgr, feed=self.mask_feed, confidence=self.confidence, **self._label_args(id_base))
            return mask_u8.to(torch.int32), labels
        mask_u8, labels = _nets.analyse_image(self.mask_net, cur_bgr, feed=self.mask_feed, confidence=self.confidence, trunk=self.g_trunk, **self._label_args(id_base))
        return mask_u8.to(torch.int32), labels


class EndToEnd:
    """RunNet || RunVidoSlam on one GPU: the caller pushes BGR frames; the networks of frame k+1 are enqueued (three hipGraph replays) on the network stream while a
    worker thread tracks frame k through the System (the C++ facade: ORB, lists, P3P-RANSAC, the four optimisers, scene flow, object tracking, re-seeding, local BA)
    on the tracker's own stream.

    handover = "device" (default): the frame is uploaded ONCE (BGR, 0.9 MB), the three networks write device tensors, those are parked in a device
    ring (three device-to-device copies in stream order, because the next graph replay overwrites the graphs' static outputs) and System.TrackRGBDDevice takes the
    ring's pointers: the tracker's stream waits for the producer's event ON THE DEVICE, no map crosses PCIe in either direction and the host never waits for the
    networks before it starts enqueuing the tracker (the reference's chain being replaced: src/realtime_demo/src/run_vido.cc:57-171, three service calls with the
    image going out and a map coming back each, then TrackRGBD uploading the three maps again).
    handover = "host": round 2's form — one D2H copy per map into pinned buffers, TrackRGBD(host arrays) uploads them again (kept for A/B measurements).

    feed = "nets": the tracker consumes the networks' outputs.  feed = "given": the networks run at full cost and their outputs are parked exactly as above, but the
    tracker is handed caller-supplied depth / flow / mask maps of the frame (uploaded next to the BGR frame) — for synthetic benchmarks, where random-weight networks
    produce maps without any geometry for the tracker to work on.  Frame k is still tracked only after its three forwards have completed (same event).

    nodes.on_range = "recompute": each ring slot carries the frame's two range words (NetNodes.infer latches both contexts into them); before frame k is tracked the worker
    waits for the frame, reads ITS words (not the live flags, which may already hold frame k + 1's trips) and, when one is set, recomputes that network in fp32's range
    (NetNodes.recompute, on the network stream under net_lock) into the frame's ring buffers.  range_frames lists the frames recomputed, nodes.range_recomputes counts per network."""

    RING = 4                                  # buffer sets: the tracker keeps the maps of the previous frame in use (mask / flow of frame k-1 during frame k)

    def __init__(self, nodes, system, n_image=10000, feed="nets", handover="device"):
        self.nodes, self.system, self.n_image, self.feed, self.handover = nodes, system, n_image, feed, handover
        # (round 6) the tracker ADOPTS the ring's map buffers instead of copying them into its own slots: the ring holds RING = 4 frames, the tracker reads frames k and k - 1,
        # the networks write at most two frames ahead.  VIDO_TRACK_COPY_MAPS=1 keeps the copies (6.1 MB device-to-device per frame).
        if handover == "device" and hasattr(system, "SetZeroCopyMaps"):
            system.SetZeroCopyMaps(not _os.environ.get("VIDO_TRACK_COPY_MAPS"))
        self._prefetch = handover == "device" and hasattr(system, "PrefetchImageDevice") and not _os.environ.get("VIDO_TRACK_NO_PREFETCH")
        h, w = nodes.h, nodes.w; dev = nodes.dev
        pin = lambda shape, dt: torch.empty(shape, dtype=dt).pin_memory()
        self.host = [dict(bgr=pin((h, w, 3), torch.uint8), flow=pin((h, w, 2), torch.float32), depth=pin((h, w), torch.float32), mask=pin((h, w), torch.int32),
                          counts=pin((2,), torch.int32), range=pin((2,), torch.int32), id_base=0, propagated=False) for _ in range(self.RING)]
        self.range_frames = []                # frames whose networks were recomputed in fp32's range (nodes.on_range == "recompute")
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        self.dev = [dict(bgr=mk((h, w, 3), torch.uint8), flow=mk((h, w, 2), torch.float32), depth=mk((h, w), torch.float32), mask=mk((h, w), torch.int32),
                         gflow=mk((h, w, 2), torch.float32), gdepth=mk((h, w), torch.float32), gmask=mk((h, w), torch.int32)) for _ in range(self.RING)]
        if getattr(nodes, "depth_source", "net") == "stereo":          # the right view of every frame in flight: a pinned and a device buffer per ring slot
            for hb, db in zip(self.host, self.dev):
                hb["right"] = pin((h, w, 3), torch.uint8); db["right"] = mk((h, w, 3), torch.uint8)
        self.rectify = getattr(nodes, "rectify", None) is not None      # raw frames in: a pinned and a device buffer of the raw size per camera and ring slot
        if self.rectify:
            rh, rw = nodes.rectify["raw_size"]
            for hb, db in zip(self.host, self.dev):
                hb["raw"] = pin((rh, rw, 3), torch.uint8); db["raw"] = mk((rh, rw, 3), torch.uint8)
                if "right" in db:
                    hb["raw_right"] = pin((rh, rw, 3), torch.uint8); db["raw_right"] = mk((rh, rw, 3), torch.uint8)
        self.copy_stream = torch.cuda.Stream(device=dev)
        self.q = _queue.Queue(maxsize=1)      # the networks run at most one frame ahead of the tracker (+ the one in flight)
        self.poses, self.stats, self.err = [], [], None
        self.t_net, self.t_track, self.t_wait, self.n_det = [], [], [], []
        self.prev = None; self.k = 0
        self.net_lock = _threading.Lock()     # the networks' host-side state (stream adoption, ctx scratch, static trunk buffers) has ONE user at a time: push() or the overflow redo
        self.worker = _threading.Thread(target=self._track_loop, daemon=True); self.worker.start()

    def _track_loop(self):
        while True:
            item = self.q.get()
            if item is None:
                return
            k, slot, ev, img_ev = item
            try:
                if self.err is not None:                                 # a failed frame stops the sequence: later frames are drained, not tracked on a broken System
                    continue
                t0 = _time.perf_counter()
                hb, db = self.host[slot], self.dev[slot]
                T = None
                if self.handover == "device":
                    # (round 6) the ORB extraction needs nothing but the image: it goes onto the tracker's stream BEFORE the wait for the frame's networks and runs beside their
                    # tail, instead of starting — as the frame's first heavy tracker work — against the just-enqueued networks of frame k + 1 (VIDO_TRACK_NO_PREFETCH=1: as before)
                    if self._prefetch and not _os.environ.get("VIDO_E2E_SKIP_TRACK"):
                        self.system.PrefetchImageDevice(db["bgr"].data_ptr(), 3, self.nodes.w, self.nodes.h, img_ev.cuda_event)
                    safe = False
                    if self.nodes.on_range == "recompute":               # the frame's own range words: a host wait for its event, with or without the static head
                        ev.synchronize()
                        safe = self._recompute_if_tripped(k, slot)
                    if self.nodes.g_det is not None:                     # the static head's overflow flag (rare): needs the frame's counts, i.e. a host wait for this one event
                        ev.synchronize()
                        if not hb["propagated"]:                         # (a propagated frame ran no detector: nothing to redo)
                            self._redo_if_overflowed(slot, range_safe=safe)
                        if self.nodes.on_range == "raise":
                            self.nodes.check_conv1x1_range()             # (the frame's networks are complete: ev)
                    t1 = _time.perf_counter()
                    if not _os.environ.get("VIDO_E2E_SKIP_TRACK"):
                        d, f, m = (db["depth"], db["flow"], db["mask"]) if self.feed == "nets" else (db["gdepth"], db["gflow"], db["gmask"])
                        T = self.system.TrackRGBDDevice(db["bgr"].data_ptr(), 3, self.nodes.w, self.nodes.h, d.data_ptr(), f.data_ptr(), m.data_ptr(), ev.cuda_event,
                                                        float(k), self.n_image)
                else:
                    ev.synchronize()                                     # networks + hand-over copies of frame k are complete
                    if self.nodes.on_range == "recompute":
                        self._recompute_if_tripped(k, slot)
                    else:
                        self.nodes.check_conv1x1_range()
                    t1 = _time.perf_counter()
                    if self.feed == "nets":
                        d, f, m = hb["depth"].numpy(), hb["flow"].numpy(), hb["mask"].numpy()
                    else:
                        d, f, m = hb["given"]
                    if not _os.environ.get("VIDO_E2E_SKIP_TRACK"):       # diagnosis only: networks + hand-over without the tracker
                        T = self.system.TrackRGBD(hb["bgr"].numpy(), d, f, m, None, None, float(k), None, self.n_image)
                t2 = _time.perf_counter()
                self.poses.append(T); self.stats.append(self.system.stats() if T is not None else {})
                self.t_wait.append((t1 - t0) * 1e3); self.t_track.append((t2 - t1) * 1e3)
                self.n_det.append(int(hb["counts"][1]) if self.nodes.g_det is not None else int(getattr(self.nodes.mask_net.roi_heads.mask, "last_n", 0)))
            except Exception as e:                                       # surfaced by push() / finish()
                self.err = e
            finally:
                self.q.task_done()

    @torch.no_grad()
    def _recompute_if_tripped(self, k, slot):
        """Frame k's range words (its networks are complete) -> recompute what tripped into the frame's ring buffers (device, and the host maps in the host hand-over) and
        counts.  True when the detector was recomputed (an overflow redo of that frame must stay in fp32's range too)."""
        hb, db = self.host[slot], self.dev[slot]
        hit_flow, hit_det = bool(hb["range"][0]), bool(hb["range"][1])
        if not (hit_flow or hit_det):
            return False
        prev = self.dev[(slot - 1) % self.RING]["bgr"] if k > 0 else db["bgr"]          # (frame k - 1's slot is not reused before frame k has been tracked)
        # as in _redo_if_overflowed: on the network stream (stream order protects the contexts' scratch) and under the lock push() holds around infer()
        with self.net_lock, torch.cuda.stream(self.net_stream):
            r = self.nodes.recompute(prev, db["bgr"], flow=hit_flow, detector=hit_det, id_base=hb["id_base"])
            if r["flow"] is not None:
                db["flow"].copy_(r["flow"])
            if r["detector"] is not None:
                db["mask"].copy_(r["detector"][0])
            self.net_stream.synchronize()
        if r["detector"] is not None and r["detector"][2] is not None:
            hb["counts"][0] = int(r["detector"][2]); hb["counts"][1] = int(r["detector"][3])
        if self.handover != "device" and self.feed == "nets":
            hb["flow"].copy_(db["flow"]); hb["mask"].copy_(db["mask"])
        self.range_frames.append(k)
        return r["detector"] is not None

    @torch.no_grad()
    def _redo_if_overflowed(self, slot, range_safe=False):
        n_det = int(self.host[slot]["counts"][1])
        if n_det <= self.nodes.mask_net.config.detections_per_img:
            return
        # on the NETWORK stream (the detector's HIP ops share one device scratch, which stream order protects) and under the lock push() holds around infer():
        # the host-side state of the nodes (adopted stream, ctx scratch pointers, static trunk buffers) is not protected by stream order
        with self.net_lock, torch.cuda.stream(self.net_stream):
            r = self.nodes.redo_detector_if_overflowed(self.dev[slot]["bgr"], n_det, range_safe=range_safe, id_base=self.host[slot]["id_base"])
            if r is not None:
                self.dev[slot]["mask"].copy_(r[0])
            self.net_stream.synchronize()

    @torch.no_grad()
    def push(self, bgr, given=None, right=None):
        """bgr: HxWx3 u8 numpy; over NetNodes(rectify=...) the RAW frame, raw_h x raw_w x 3 (and `right` the raw right frame): both go up to raw ring buffers and one
        rectify launch writes the slot's frame (and right) buffers before the event the networks and the tracker wait for, so the tracker, ORB, the flow, the detector and
        SGM all see the rectified left view; the tracker's settings then hold P's intrinsics and zero distortion.  right: HxWx3 u8 numpy, the rectified right view of bgr — with NetNodes(depth_source="stereo") only, where it is required: it is uploaded next
        to the frame and the depth parked in the ring is the stereo op's disparity image (metres in the tracker through the KITTI ChooseData code, DepthMapFactor: 1 and
        Camera.bf = fx * baseline: NetNodes' docstring).  given = (depth f32 HxW raw sensor units, flow f32 HxWx2, mask i32 HxW) for feed == "given" (copied: the caller's arrays are not modified,
        although the tracker rescales the depth map it is handed in place)."""
        if self.err is not None:
            raise self.err
        stereo = getattr(self.nodes, "depth_source", "net") == "stereo"
        if (right is None) == stereo:
            raise ValueError("right: required with NetNodes(depth_source='stereo') and only there")
        t0 = _time.perf_counter()
        self.net_stream = torch.cuda.current_stream()
        slot = self.k % self.RING
        hb, db = self.host[slot], self.dev[slot]
        cur = db["bgr"]
        if self.rectify:                                                 # raw frames go up; ONE launch writes the rectified frame(s) into the slot's frame and right buffers
            hb["raw"].numpy()[...] = bgr
            db["raw"].copy_(hb["raw"], non_blocking=True)
            if stereo:
                hb["raw_right"].numpy()[...] = right
                db["raw_right"].copy_(hb["raw_right"], non_blocking=True)
            with self.net_lock:
                self.nodes.rectify_frames(db["raw"], db["raw_right"] if stereo else None, out_left=cur, out_right=db["right"] if stereo else None)
            if self.handover != "device":                                # the host hand-over gives the tracker the host frame: the rectified one comes back
                hb["bgr"].copy_(cur, non_blocking=True)
        else:
            hb["bgr"].numpy()[...] = bgr
            cur.copy_(hb["bgr"], non_blocking=True)                      # the only upload of the frame on the network side
        img_ev = torch.cuda.Event(); img_ev.record()                     # the image is on the device: all the tracker's ORB extraction needs (prefetched in _track_loop)
        if stereo and not self.rectify:
            hb["right"].numpy()[...] = right
            db["right"].copy_(hb["right"], non_blocking=True)
        if given is not None:
            hb["depth"].numpy()[...] = given[0]; hb["flow"].numpy()[...] = given[1]; hb["mask"].numpy()[...] = given[2]
            if self.handover == "device":                                # the stand-in maps go up next to the frame (feed == "nets" uploads nothing but the frame)
                db["gdepth"].copy_(hb["depth"], non_blocking=True); db["gflow"].copy_(hb["flow"], non_blocking=True); db["gmask"].copy_(hb["mask"], non_blocking=True)
            else:
                hb["given"] = (hb["depth"].numpy().copy(), hb["flow"].numpy().copy(), hb["mask"].numpy().copy())
        prev = cur if self.prev is None else self.prev                   # first frame: RunNet has no previous image yet; the tracker ignores the flow of frame 0's predecessor
        with self.net_lock:
            if stereo:
                flow, depth, mask, labels, evs = self.nodes.infer(prev, cur, range_words=hb["range"] if self.nodes.on_range == "recompute" else None, right_bgr=db["right"])
            else:
                flow, depth, mask, labels, evs = self.nodes.infer(prev, cur, range_words=hb["range"] if self.nodes.on_range == "recompute" else None)
            hb["id_base"] = self.nodes.id_base                           # (label_mode="instance": a later recomputation of this frame paints under the same ids)
            hb["propagated"] = bool(getattr(self.nodes, "last_propagated", False))      # (detect_every > 1: the mask was warped from the frame before, no detector ran)
        # graph outputs are static buffers that the next replay overwrites: park them in this slot's device buffers (three device-to-device copies of 4.8 MB in stream order)
        if self.nodes.streams is not None:
            for e in evs:
                torch.cuda.current_stream().wait_event(e)
        db["flow"].copy_(flow, non_blocking=True); db["depth"].copy_(depth, non_blocking=True); db["mask"].copy_(mask, non_blocking=True)
        if self.nodes.last_counts is not None:
            hb["counts"][0:1].copy_(self.nodes.last_counts[0].reshape(1), non_blocking=True); hb["counts"][1:2].copy_(self.nodes.last_counts[1].reshape(1), non_blocking=True)
        parked = torch.cuda.Event(); parked.record()
        done = parked
        if self.handover != "device":                                    # round 2's hand-over: the maps go to pinned host buffers on the copy stream
            cs = self.copy_stream
            cs.wait_event(parked)
            with torch.cuda.stream(cs):
                if self.feed == "nets":
                    hb["flow"].copy_(db["flow"], non_blocking=True); hb["depth"].copy_(db["depth"], non_blocking=True); hb["mask"].copy_(db["mask"], non_blocking=True)
                else:                                                    # same traffic, into a scratch set (hb[...] holds the given maps)
                    self._sink = getattr(self, "_sink", None) or [torch.empty_like(hb["flow"]).pin_memory(), torch.empty_like(hb["depth"]).pin_memory(), torch.empty_like(hb["mask"]).pin_memory()]
                    self._sink[0].copy_(db["flow"], non_blocking=True); self._sink[1].copy_(db["depth"], non_blocking=True); self._sink[2].copy_(db["mask"], non_blocking=True)
                done = torch.cuda.Event(); done.record()
        self._alive = (flow, depth, mask, labels)
        self.prev = cur
        self.t_net.append((_time.perf_counter() - t0) * 1e3)
        self.q.put((self.k, slot, done, img_ev))                         # blocks while the tracker is still two frames behind
        self.k += 1

    def finish(self):
        self.q.join()
        if self.err is not None:
            raise self.err

    def close(self):
        self.q.put(None)
        self.worker.join(timeout=10)
