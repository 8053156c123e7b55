"""`System` — ctypes mirror of VIDO_SLAM::System (vido_slam/include/System.h:72-114) over the C handle of include/vido_c.h
(vido_system_*).  Same three calls as the reference's callers make (vido_slam/demo/run_vido_slam.cc:82-135,
src/realtime_demo/src/run_vido.cc:229-235, 275):

    slam = System(); slam.Init("config.yaml", System.RGBD)
    Tcw = slam.TrackRGBD(im, depth, flow, mask, Tcw_gt, objpose_gt, timestamp, imTraj, nImage)
    slam.SaveResultsIJRR2020(prefix)

TrackRGBD releases the GIL for the whole call (ctypes), so a pipeline can run the three networks for frame k+1 from another
Python thread while frame k is being tracked (vido_slam_amd/pipeline.py::EndToEnd).
"""
import ctypes as C
import os
import numpy as np

from .host import load_library, VidoError, VIDO_OK


class SystemStats(C.Structure):
    """vido_system_stats."""
    _fields_ = [("frame_id", C.c_int32), ("n_keypoints", C.c_int32), ("n_static", C.c_int32), ("n_static_inliers", C.c_int32),
                ("n_objects", C.c_int32), ("n_object_points", C.c_int32), ("ba_window", C.c_int32), ("mask_propagated", C.c_int32),
                ("ms_total", C.c_float), ("ms_update_mask", C.c_float), ("ms_frame", C.c_float), ("ms_cam_pose", C.c_float),
                ("ms_obj_tracking", C.c_float), ("ms_obj_motion", C.c_float), ("ms_renew", C.c_float), ("ms_local_ba", C.c_float), ("ms_wait_inputs", C.c_float), ("ms_orb", C.c_float), ("ms_lists", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class System:
    MONOCULAR, STEREO, RGBD, IMU_RGBD = 0, 1, 2, 3      # System::eSensor (System.h:76-81)

    def __init__(self):
        self.lib = load_library()
        self.h = None
        self._keep = None                                 # the arrays of the last call (the tracker holds shallow references to them)

    def Init(self, strSettingsFile, sensor=2):
        if sensor != self.RGBD:
            raise VidoError(-1, "System.Init: only the RGBD sensor path is built (IMU_RGBD / VIO is out of scope)")
        h = C.c_void_p()
        rc = self.lib.vido_system_create(os.fsencode(strSettingsFile), C.byref(h))
        if rc != VIDO_OK:
            raise VidoError(rc, self.lib.vido_system_last_error(None).decode())
        self.h = h

    def TrackRGBD(self, im, depthmap, flowmap, masksem, mTcw_gt=None, vObjPose_gt=None, timestamp=0.0, imTraj=None, nImage=10000):
        """im u8 (H,W) / (H,W,3|4); depthmap f32 (H,W) — REWRITTEN IN PLACE with the pre-scaled depth (Tracking.cc:299-322);
        flowmap f32 (H,W,2); masksem i32 (H,W).  Returns Tcw (4,4) f32.  mTcw_gt / vObjPose_gt / imTraj: accepted and ignored
        (ground-truth metrics and the trajectory canvas are viewer / evaluation features).
        masksem=None (settings key Mask.PropagateMissing: 1, not on the first frame): the frame takes the previous frame's mask, propagated through the previous frame's
        flow (stats()["mask_propagated"] == 1); with the key at 0 the library refuses the call."""
        if self.h is None:
            raise VidoError(-1, "System.TrackRGBD before Init")
        if im.dtype != np.uint8 or not im.flags.c_contiguous:
            im = np.ascontiguousarray(im, np.uint8)
        if depthmap.dtype != np.float32 or not depthmap.flags.c_contiguous or not depthmap.flags.writeable:
            raise VidoError(-1, "TrackRGBD: depthmap must be a writable C-contiguous float32 array (it is rescaled in place)")
        if flowmap.dtype != np.float32 or not flowmap.flags.c_contiguous:
            flowmap = np.ascontiguousarray(flowmap, np.float32)
        if masksem is not None and (masksem.dtype != np.int32 or not masksem.flags.c_contiguous):
            masksem = np.ascontiguousarray(masksem, np.int32)
        h, w = im.shape[:2]
        cn = 1 if im.ndim == 2 else im.shape[2]
        T = np.empty((4, 4), np.float32)
        keep = (im, depthmap, flowmap, masksem)
        rc = self.lib.vido_system_track_rgbd(self.h, im.ctypes.data, cn, w, h, depthmap.ctypes.data, flowmap.ctypes.data, masksem.ctypes.data if masksem is not None else None,
                                             float(timestamp), int(nImage), T.ctypes.data)
        self._keep = keep
        if rc != VIDO_OK:
            raise VidoError(rc, self.lib.vido_system_last_error(self.h).decode())
        return T

    def PrefetchImageDevice(self, im_dev, channels, width, height, image_ready_event=None):
        """Put the ORB extraction of the next TrackRGBDDevice call's image on the tracker's stream now (it needs nothing but the image): call it, on the thread that tracks,
        while still waiting for the frame's networks; the track call for the same pointer then only collects (vido_system_prefetch_image_device)."""
        rc = self.lib.vido_system_prefetch_image_device(self.h, im_dev, int(channels), int(width), int(height), image_ready_event)
        if rc != 0:
            raise VidoError(rc, self.lib.vido_system_last_error(self.h).decode())

    def SetZeroCopyMaps(self, on=True):
        """TrackRGBDDevice adopts the three device map buffers instead of copying them into the tracker's slots (6.1 MB of device-to-device copies per 640x480 frame): the
        caller keeps a frame's maps alive and untouched until the call after the next one has returned (vido_system_set_zero_copy_maps)."""
        rc = self.lib.vido_system_set_zero_copy_maps(self.h, int(bool(on)))
        if rc != 0:
            raise VidoError(rc, "vido_system_set_zero_copy_maps")

    def TrackRGBDDevice(self, im_dev, channels, width, height, depth_dev, flow_dev, mask_dev, ready_event=None, timestamp=0.0, nImage=10000):
        """System::TrackRGBDDevice (extension): the same call on DEVICE-resident buffers given as raw pointers (e.g. tensor.data_ptr()): u8 image with
        `channels` interleaved channels, depth f32 (rescaled in place on the device), flow f32 x2, mask i32 of a width x height frame; ready_event: raw hipEvent_t
        (torch.cuda.Event.cuda_event) recorded by the producer of the buffers, or None.  The caller keeps the buffers alive for two frames.  Returns Tcw (4,4) f32.
        mask_dev = 0 / None with Mask.PropagateMissing: 1: as masksem=None of TrackRGBD."""
        if self.h is None:
            raise VidoError(-1, "System.TrackRGBDDevice before Init")
        T = np.empty((4, 4), np.float32)
        rc = self.lib.vido_system_track_rgbd_device(self.h, int(im_dev), int(channels), int(width), int(height), int(depth_dev), int(flow_dev), int(mask_dev or 0), int(ready_event or 0),
                                                    float(timestamp), int(nImage), T.ctypes.data)
        if rc != VIDO_OK:
            raise VidoError(rc, self.lib.vido_system_last_error(self.h).decode())
        return T

    def set_depth_noise_seed(self, seed):
        """Pins the seed of the reference's time(NULL)-seeded depth noise (Frame.cc:711-716; 0 = the reference behaviour): reproducible PoseOptimizationNew results."""
        rc = self.lib.vido_system_set_depth_noise_seed(self.h, int(seed) & 0xffffffff)
        if rc != 0:
            raise VidoError(rc, "set_depth_noise_seed: no system")

    def stats(self):
        s = SystemStats()
        self.lib.vido_system_get_stats(self.h, C.byref(s))
        return s.as_dict()

    def verify_stats(self):
        """(n_checked, n_rejected) of the last frame's descriptor verification (Verify.Descriptor: 1; both 0 otherwise)."""
        a, b = C.c_int(), C.c_int()
        self.lib.vido_system_get_verify_stats(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def mask_split_stats(self):
        """(found, dropped for area, left out for the cap, kept) of the last frame's mask split (settings key Mask.SplitInstances: 1: the frame's mask is split into its
        8-connected components of equal value of at least Mask.MinInstanceArea pixels, so that same-class objects track separately); zeros when the frame was not split."""
        st = (C.c_int32 * 4)()
        rc = self.lib.vido_system_mask_split_stats(self.h, st)
        if rc != VIDO_OK:
            raise VidoError(rc, "vido_system_mask_split_stats")
        return int(st[0]), int(st[1]), int(st[2]), int(st[3])

    def verify_points(self):
        """Debug read of the last frame's per-point verification state (vido_system_get_verify_points), index-aligned with the frame's static list:
        dict of xy (n,2) f32, prev_xy (n,2) f32, xyl (n,3) i32, dist (n,) i32, rejected (n,) bool, seed_desc (n,32) u8."""
        n = C.c_int()
        self.lib.vido_system_get_verify_points(self.h, None, None, None, None, None, None, 0, C.byref(n))
        n = n.value; m = max(n, 1)
        xy = np.empty((m, 2), np.float32); pxy = np.empty((m, 2), np.float32); xyl = np.empty((m, 3), np.int32); dist = np.empty(m, np.int32)
        rej = np.empty(m, np.uint8); seed = np.empty((m, 32), np.uint8)
        rc = self.lib.vido_system_get_verify_points(self.h, xy.ctypes.data, pxy.ctypes.data, xyl.ctypes.data, dist.ctypes.data, rej.ctypes.data, seed.ctypes.data, m, C.byref(C.c_int()))
        if rc != VIDO_OK:
            raise VidoError(rc, "vido_system_get_verify_points")
        return dict(xy=xy[:n], prev_xy=pxy[:n], xyl=xyl[:n], dist=dist[:n], rejected=rej[:n].astype(bool), seed_desc=seed[:n])

    def recover_stats(self):
        """(n_tried, n_recovered) of the last frame's Verify.Recover search (both 0 with the option off): the rejected points searched, and those re-found."""
        a, b = C.c_int(), C.c_int()
        self.lib.vido_system_get_recover_stats(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def recover_points(self):
        """Debug read of the last frame's Verify.Recover state (vido_system_get_recover_points), index-aligned with verify_points(): dict of status (n,) i32 (-1: not
        searched; else vido_hamming_match_window's status, 0 = re-found), idx (n,) i32, match_xy (n,2) f32, dist / dist2 (n,) i32, after (n,5) f32 = x, y, depth and the
        last frame's flow x, y as the step left them, and the train list of the frame's call: train_xy (nt,2) f32, train_level (nt,) i32, train_desc (nt,32) u8,
        train_depth (nt,) f32."""
        n, nt = C.c_int(), C.c_int()
        self.lib.vido_system_get_recover_points(self.h, None, None, None, None, None, None, 0, C.byref(n), None, None, None, None, 0, C.byref(nt))
        n, nt = n.value, nt.value; m, mt = max(n, 1), max(nt, 1)
        status = np.empty(m, np.int32); idx = np.empty(m, np.int32); mxy = np.empty((m, 2), np.float32); dist = np.empty(m, np.int32); dist2 = np.empty(m, np.int32)
        after = np.empty((m, 5), np.float32); txy = np.empty((mt, 2), np.float32); tlv = np.empty(mt, np.int32); tds = np.empty((mt, 32), np.uint8); tdp = np.empty(mt, np.float32)
        rc = self.lib.vido_system_get_recover_points(self.h, status.ctypes.data, idx.ctypes.data, mxy.ctypes.data, dist.ctypes.data, dist2.ctypes.data, after.ctypes.data, m,
                                                     C.byref(C.c_int()), txy.ctypes.data, tlv.ctypes.data, tds.ctypes.data, tdp.ctypes.data, mt, C.byref(C.c_int()))
        if rc != VIDO_OK:
            raise VidoError(rc, "vido_system_get_recover_points")
        return dict(status=status[:n], idx=idx[:n], match_xy=mxy[:n], dist=dist[:n], dist2=dist2[:n], after=after[:n],
                    train_xy=txy[:nt], train_level=tlv[:nt], train_desc=tds[:nt], train_depth=tdp[:nt])

    def object_verify_stats(self):
        """(n_checked, n_rejected, n_no_texture) of the last frame's patch verification of the dense object points (Verify.ObjectPatch: 1; all 0 otherwise)."""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self.lib.vido_system_get_object_verify_stats(self.h, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def object_verify_points(self):
        """Debug read of the last frame's Verify.ObjectPatch state (vido_system_get_object_verify_points), index-aligned with the object points the frame carried over
        from the last one: dict of xyl (n,3) i32, sums (n,3) i32 = cov, var_ref, var_cur, status (n,) i32 (0 kept, 1 rejected, 2 no texture, -1 patch outside the image),
        prev_xy (n,2) f32 = the last frame's point, ref_patch (n,64) u8 = the last frame's patch."""
        n = C.c_int()
        self.lib.vido_system_get_object_verify_points(self.h, None, None, None, None, None, 0, C.byref(n))
        n = n.value; m = max(n, 1)
        xyl = np.empty((m, 3), np.int32); sums = np.empty((m, 3), np.int32); status = np.empty(m, np.int32); pxy = np.empty((m, 2), np.float32); ref = np.empty((m, 64), np.uint8)
        rc = self.lib.vido_system_get_object_verify_points(self.h, xyl.ctypes.data, sums.ctypes.data, status.ctypes.data, pxy.ctypes.data, ref.ctypes.data, m, C.byref(C.c_int()))
        if rc != VIDO_OK:
            raise VidoError(rc, "vido_system_get_object_verify_points")
        return dict(xyl=xyl[:n], sums=sums[:n], status=status[:n], prev_xy=pxy[:n], ref_patch=ref[:n])

    def object_recover_stats(self):
        """(n_tried, n_recovered) of the last frame's search for the object points the patch verification rejected (Verify.ObjectRecover: 1; both 0 otherwise)."""
        a, b = C.c_int(), C.c_int()
        self.lib.vido_system_get_object_recover_stats(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def object_recover_points(self):
        """Debug read of the last frame's Verify.ObjectRecover step (vido_system_get_object_recover_points), index-aligned with object_verify_points(): dict of status (n,)
        i32 of vido_orb_patch_search (-2: not searched), dxy (n,2), sums (n,3), second (n,2) i32 as the call returned them, gather (n,2) f32 = depth, label at the re-found
        pixel (-1, -1 where status != 0), after (n,6) f32 = x, y, depth, label, last frame's flow x, y as the step left them."""
        n = C.c_int()
        self.lib.vido_system_get_object_recover_points(self.h, None, None, None, None, None, None, 0, C.byref(n))
        n = n.value; m = max(n, 1)
        status = np.empty(m, np.int32); dxy = np.empty((m, 2), np.int32); sums = np.empty((m, 3), np.int32); second = np.empty((m, 2), np.int32)
        gather = np.empty((m, 2), np.float32); after = np.empty((m, 6), np.float32)
        rc = self.lib.vido_system_get_object_recover_points(self.h, status.ctypes.data, dxy.ctypes.data, sums.ctypes.data, second.ctypes.data, gather.ctypes.data, after.ctypes.data, m, C.byref(C.c_int()))
        if rc != VIDO_OK:
            raise VidoError(rc, "vido_system_get_object_recover_points")
        return dict(status=status[:n], dxy=dxy[:n], sums=sums[:n], second=second[:n], gather=gather[:n], after=after[:n])

    def object_refine_stats(self):
        """(n_tried, n_refined) of the last frame's sub-pixel alignment of the re-found object points (Verify.ObjectRecoverSubpixel: 1; both 0 otherwise)."""
        a, b = C.c_int(), C.c_int()
        self.lib.vido_system_get_object_refine_stats(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def object_refine_points(self):
        """Debug read of the last frame's Verify.ObjectRecoverSubpixel step (vido_system_get_object_refine_points), index-aligned with object_recover_points(): dict of
        status (n,) i32 of vido_orb_patch_refine (-2: not sent), q8 (n,2) i32 and cost (n,2) i64 as the call returned them."""
        n = C.c_int()
        self.lib.vido_system_get_object_refine_points(self.h, None, None, None, 0, C.byref(n))
        n = n.value; m = max(n, 1)
        q8 = np.empty((m, 2), np.int32); cost = np.empty((m, 2), np.int64); status = np.empty(m, np.int32)
        rc = self.lib.vido_system_get_object_refine_points(self.h, q8.ctypes.data, cost.ctypes.data, status.ctypes.data, m, C.byref(C.c_int()))
        if rc != VIDO_OK:
            raise VidoError(rc, "vido_system_get_object_refine_points")
        return dict(status=status[:n], q8=q8[:n], cost=cost[:n])

    def SaveResultsIJRR2020(self, filename=""):
        rc = self.lib.vido_system_save_results(self.h, os.fsencode(filename))
        if rc != VIDO_OK:
            raise VidoError(rc, self.lib.vido_system_last_error(self.h).decode())

    def close(self):
        if self.h is not None:
            self.lib.vido_system_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
