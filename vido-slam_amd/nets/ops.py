"""torch <-> C-ABI glue for the network ops.  Device tensors are handed to the library as raw pointers
(on_device=1); the ctx adopts torch's current stream (vido_set_stream) so launches are ordered with the
surrounding torch kernels without any synchronisation."""
import contextlib
import ctypes as C
import os
import torch

_WINO_MIN_WGS = int(os.environ.get("VIDO_WINO_MIN_WGS", "0"))
_CONV3X3_H_MIN_WGS = 0 if os.environ.get("VIDO_CONV3X3_H") == "0" else int(os.environ.get("VIDO_CONV3X3_H_MIN_WGS", "128"))      # direct split-fp16 3x3 (csrc/conv3x3h.hip) from this many workgroups on
# which layers conv_direct_conv takes: "all", or "novalu" (default) = not the 7x7 stem / stride-2 3x3 layers, which the library runs as Winograd on the VECTOR ALUs — beside
# the detector (whose convolutions saturate the MATRIX pipe) those run in its shadow, while the direct kernel competes for the matrix pipe.  Measured (two pairs of 100
# steps, profiles/r5/convdirect_ab.txt): headline 90.3 frames/s without the direct kernel, 89.4 with it on every layer (LiteFlowNet alone 3.85 -> 3.65 ms), 90.6 with
# "novalu" (3.76 ms alone).  Leaving only the two miopenSp3AsmConv layers (stem, 32 -> 32 stride 2) to the library and taking the other stride-2 layers (implicit GEMM
# in the library) gives 90.0 against 90.4: the direct kernel's matrix-pipe time costs the frame more than the library's kernels there too.  The trade does NOT extend to
# the dense 3x3 layers: LiteFlowNet on the library's vector-ALU Winograd throughout gives 82 frames/s.
# Round 6 (detector in split fp16, profiles/r6/convdirect_set_ab.txt): 125.0 frames/s with "novalu" against 124.3 / 124.5 with "all" (the chain without the detector: 191.4 against 193.8).
_CONVDIRECT_SET = os.environ.get("VIDO_CONVDIRECT_SET", "novalu")
_GCONV_H = os.environ.get("VIDO_GCONV_H", "1") != "0"      # split-fp16 grouped 3x3 (csrc/gconvh.hip) for 32 / 64 channels per group; 0: the fp32 kernel of csrc/gconv.hip everywhere
_GCONV_HS = os.environ.get("VIDO_GCONV_HS", "1") != "0"    # ... and for 8 / 16 channels per group (csrc/gconvhs.hip); 0: only those layers back on the fp32 kernel (A/B runs)


def correlation_torch_reference(first, second, stride):
    """Plain-PyTorch fp32 reference of the 7x7 cost volume (used by the CPU tests only; the product path is the HIP
    kernel): out[b,(p+3)*7+(o+3),y,x] = mean_c f1[b,c,y*s,x*s] * f2[b,c,(y+p)*s,(x+o)*s]."""
    a, b = first[:, :, ::stride, ::stride], second[:, :, ::stride, ::stride]
    pad = torch.nn.functional.pad(b, (3, 3, 3, 3))
    H, W = a.shape[2], a.shape[3]
    return torch.stack([(a * pad[:, :, p:p + H, o:o + W]).mean(1) for p in range(7) for o in range(7)], 1)


def _p(t):
    """the pointer argument for a tensor: its data_ptr(), None (NULL) for an absent one"""
    return t.data_ptr() if t is not None else None


def _tensor_args(op, table):
    """The rules every tensor argument of a standalone op meets.  table: rows of (name, tensor, dtype, required), the first required tensor first: it is the device anchor.
    A tensor that is given (a required one must be) is a contiguous device tensor of its dtype on the anchor's device.  Returns `bad`, which raises
    VidoError(-1, "<op>: <why>"), for the op's own rules."""
    from ..host import VidoError
    def bad(why):
        raise VidoError(-1, "%s: %s" % (op, why))
    anchor_name, anchor = table[0][:2]
    for name, t, dt, required in table:
        if t is None and not required:
            continue
        if not torch.is_tensor(t) or not t.is_cuda:
            bad("%s must be a device tensor; there is no CPU fallback" % name)
        if t.dtype != dt:
            bad("%s must be %s, got %s" % (name, dt, t.dtype))
        if not t.is_contiguous():
            bad("%s must be contiguous" % name)
        if t.device != anchor.device:
            bad("%s is on another device than %s" % (name, anchor_name))
    return bad


def _need(bad, name, t, shape):
    """a tensor that is given has exactly this shape"""
    if t is not None and tuple(t.shape) != tuple(shape):
        bad("%s must be %s, got %s" % (name, list(shape), tuple(t.shape)))


def _need_count(bad, name, t, n):
    """a tensor that is given holds at least n elements"""
    if t is not None and t.numel() < n:
        bad("%s needs %d elements" % (name, n))


def _overlaps(a, b, nbytes):
    """the first nbytes of the two tensors share memory"""
    return a.data_ptr() < b.data_ptr() + nbytes and b.data_ptr() < a.data_ptr() + nbytes


def _image_pair(bad, name0, img0, name1, img1):
    """two images [H, W] or [H, W, 3|4] of one shape -> H, W, channels"""
    if img0.dim() not in (2, 3) or (img0.dim() == 3 and img0.shape[2] not in (3, 4)):
        bad("%s must be [H, W] or [H, W, 3|4], got %s" % (name0, tuple(img0.shape)))
    if tuple(img1.shape) != tuple(img0.shape):
        bad("%s must have %s's shape %s, got %s" % (name1, name0, tuple(img0.shape), tuple(img1.shape)))
    return int(img0.shape[0]), int(img0.shape[1]), 1 if img0.dim() == 2 else int(img0.shape[2])


def cached_pack(mod, slot, w, device, extra, pack):
    """pack() kept on `mod` as the attribute `slot`: made on first use and again when the weight tensor `w` (its storage or its version: a checkpoint loaded later), the
    device or one of the `extra` key parts differs from the call that made it."""
    key = (w.data_ptr(), w._version, str(device)) + tuple(extra)
    keys = mod.__dict__.setdefault("_pack_keys", {})
    if keys.get(slot) != key:
        setattr(mod, slot, pack()); keys[slot] = key
    return getattr(mod, slot)


class HipOps:
    """FunctionCorrelation / ROIAlign / nms / box decode on device tensors through libvido_slam_hip.so."""

    _range_safe = 0                        # range_safe(): > 0 while a scope holds this object — every split-fp16 entry point declines (the callers' fp32 fallbacks run)

    def __init__(self, ctx):
        self.ctx = ctx

    def _call(self, fn, *args):
        """fn(ctx, *args) for a library function `fn` (self.ctx.lib.vido_x) enqueued on torch's current stream; a negative return raises VidoError"""
        ctx = self.ctx
        ctx._check(ctx.lib.vido_set_stream(ctx.h, torch.cuda.current_stream().cuda_stream, 1))      # (_adopt_stream, without its frame: every eager launch comes through here)
        return ctx._check(fn(ctx.h, *args))

    def _count_flops(self, flops):
        """launches torch's FlopCounterMode does not see; bench.py resets and reads gconv_flops"""
        self.gconv_flops = getattr(self, "gconv_flops", 0.0) + flops

    @property
    def range_safe_active(self):
        """True inside range_safe(): conv1x1_conv / conv1x1_bias_act callers, the direct 3x3, the grouped 3x3 (gconv3x3_conv), fc_h_linear and deconv2x2_conv take their fp32 routes."""
        return self._range_safe > 0

    @staticmethod
    def _live_ptr(n_live):
        """The `_n` entry points' last argument: None, or a one-element int32 DEVICE tensor (the live count: read by the kernel when it runs, clamped to the batch)."""
        if n_live is None:
            return None
        assert n_live.is_cuda and n_live.dtype == torch.int32 and n_live.numel() == 1, "n_live: a one-element int32 device tensor"
        return n_live.data_ptr()

    def _adopt_stream(self):
        st = torch.cuda.current_stream().cuda_stream
        self.ctx._check(self.ctx.lib.vido_set_stream(self.ctx.h, st, 1))

    def correlation(self, first, second, stride):
        if not first.is_cuda:
            raise RuntimeError("HipOps.correlation needs CUDA(HIP) tensors; there is no CPU fallback")
        first = first.contiguous().float(); second = second.contiguous().float()
        B, Cc, H, W = first.shape
        out = torch.empty((B, 49, (H + stride - 1) // stride, (W + stride - 1) // stride), device=first.device, dtype=torch.float32)
        self._call(self.ctx.lib.vido_correlation, first.data_ptr(), second.data_ptr(), B, Cc, H, W, stride, out.data_ptr(), 1)
        return out

    def bias_act_(self, x, bias, slope):
        """in place: x = leaky_relu(x + bias[None, :, None, None], slope)"""
        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32
        N, Cc, H, W = x.shape
        self._call(self.ctx.lib.vido_bias_act, x.data_ptr(), bias.data_ptr(), N, Cc, H, W, slope)
        return x

    def deconv2x2_conv(self, conv, x, slope, n_live=None):
        """nn.ConvTranspose2d `conv` (2 x 2, stride 2, no padding) + bias + activation of a batch as one split-fp16 GEMM with a scatter epilogue (csrc/conv1x1.hip, RES 3), else
        None; the packed weight is cached on the module.  n_live (one int32 device word): only the first n_live images are read and written (vido_deconv2x2_bias_act_n)."""
        w = conv.weight
        if (tuple(w.shape[2:]) != (2, 2) or tuple(conv.stride) != (2, 2) or tuple(conv.padding) != (0, 0) or tuple(conv.output_padding) != (0, 0) or tuple(conv.dilation) != (1, 1)
                or conv.groups != 1 or not x.is_cuda or x.dtype != torch.float32 or os.environ.get("VIDO_NO_DECONV_H") or self._range_safe):
            return None
        n, cin, H, W = (int(v) for v in x.shape); cout = int(w.shape[1])
        if not self.ctx.lib.vido_deconv2x2_supported(n, cin, cout, H, W):
            return None
        wp = cached_pack(conv, "_dc_w", w, x.device, (), lambda: pack_deconv2x2(w).to(x.device))
        return self.deconv2x2_bias_act(x.contiguous(), wp, conv.bias, slope, n_live)

    def deconv2x2_bias_act(self, x, w_packed, bias, slope, n_live=None):
        """The launch of deconv2x2_conv on a packed weight: w_packed = pack_deconv2x2(w), i.e. pack_conv1x1 layout 3 of the [4 cout][cin] matrix — the only layout the
        transposed form exists in; any other tensor is refused here."""
        n, cin, H, W = (int(v) for v in x.shape)
        layout, rows = packed_conv1x1_layout(w_packed, cin)
        if layout != 3 or rows % 4:
            raise ValueError("deconv2x2: the weight must be packed by pack_deconv2x2 (pack_conv1x1 layout 3 of 4 cout rows), not layout %d of %d rows" % (layout, rows))
        cout = rows // 4
        out = torch.empty((n, cout, 2 * H, 2 * W), device=x.device, dtype=torch.float32)
        self._count_flops(2.0 * n * cin * cout * 4 * H * W)
        self._call(self.ctx.lib.vido_deconv2x2_bias_act_n, x.data_ptr(), w_packed.data_ptr(), _p(bias), out.data_ptr(), n, cin, cout, H, W, slope, self._live_ptr(n_live))
        return out

    def det_order(self, scores, labels, n_det, confidence, count32=False):
        """(order int64 [cap], labels in that order with 0 for slots that fail `scores > confidence and slot < n_det`, number of live slots) — analyse_image_static's tail
        in one launch (csrc/nets.hip::k_det_order); the order is torch.sort(where(live, scores, -1), descending=True, stable=True).
        count32: a fourth result, the count once more as an int32 [1] tensor — the word the mask head's counted launches read (n_live= of the ops below)."""
        assert scores.is_cuda and scores.dtype == torch.float32 and labels.dtype == torch.int64 and n_det.dtype == torch.int32 and scores.is_contiguous() and labels.is_contiguous()
        cap = int(scores.shape[0]); dev = scores.device
        order = torch.empty((cap,), device=dev, dtype=torch.int64); lab = torch.empty((cap,), device=dev, dtype=torch.int64); n_live = torch.empty((), device=dev, dtype=torch.int64)
        n32 = torch.empty((1,), device=dev, dtype=torch.int32) if count32 else None
        self._call(self.ctx.lib.vido_det_order_n, scores.data_ptr(), labels.data_ptr(), n_det.data_ptr(), confidence, cap, order.data_ptr(), lab.data_ptr(), n_live.data_ptr(), _p(n32))
        return (order, lab, n_live, n32) if count32 else (order, lab, n_live)

    def roi_levels(self, boxes, k_min, k_max):
        """LevelMapper of the FPN pooler for boxes [n, 4] f32 -> int32 [n] in 0 .. k_max - k_min, one launch (csrc/nets.hip::k_roi_levels: the torch expression's fp32 operations
        in the same order)."""
        assert boxes.is_cuda and boxes.dtype == torch.float32
        boxes = boxes.contiguous(); n = int(boxes.shape[0])
        out = torch.empty((n,), device=boxes.device, dtype=torch.int32)
        self._call(self.ctx.lib.vido_roi_levels, boxes.data_ptr(), n, k_min, k_max, out.data_ptr())
        return out

    def mask_logit_select(self, feat, conv, labels, n_live=None):
        """sigmoid(conv(feat))[arange(n), labels][:, None] for a 1x1 `conv` (the mask head's logits layer) computing only each detection's own class channel (csrc/nets.hip).
        n_live (one int32 device word): the slots behind it come out 0 and their features are not read."""
        assert feat.is_cuda and feat.is_contiguous() and feat.dtype == torch.float32 and labels.dtype == torch.int64 and labels.is_contiguous()
        n, c, H, W = feat.shape; classes = int(conv.weight.shape[0])
        w = conv.weight.reshape(classes, c)
        if not w.is_contiguous():
            w = w.contiguous()
        out = torch.empty((n, 1, H, W), device=feat.device, dtype=torch.float32)
        self._call(self.ctx.lib.vido_mask_logit_select_n, feat.data_ptr(), w.data_ptr(), _p(conv.bias), labels.data_ptr(), out.data_ptr(), int(n), int(c), int(H * W), classes, self._live_ptr(n_live))
        return out

    def bias_res_act_(self, x, bias, res, slope):
        """in place: x = leaky_relu(x + bias[None, :, None, None] + res, slope); res None -> bias_act_ (slope 0 = ReLU, 1 = none)"""
        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32
        N, Cc, H, W = x.shape
        if res is not None:
            assert res.shape == x.shape and res.is_contiguous() and res.dtype == torch.float32
        self._call(self.ctx.lib.vido_bias_res_act, x.data_ptr(), bias.data_ptr(), _p(res), N, Cc, H, W, slope)
        return x

    def bias_unary_(self, x, bias, kind):
        """in place: x = f(x + bias[None, :, None, None]); kind "elu" | "sigmoid" """
        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32
        N, Cc, H, W = x.shape
        self._call(self.ctx.lib.vido_bias_unary, x.data_ptr(), bias.data_ptr(), N, Cc, H, W, 1 if kind == "elu" else 2)
        return x

    def upcat_reflect(self, x, skip=None):
        """ReflectionPad2d(1)(cat([interpolate(x, scale_factor=2, mode="nearest"), skip], 1)) for one image, one pass."""
        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and x.shape[0] == 1
        _, C1, h, w = x.shape
        C2 = 0
        if skip is not None:
            assert skip.is_contiguous() and skip.shape[0] == 1 and tuple(skip.shape[2:]) == (2 * h, 2 * w)
            C2 = skip.shape[1]
        out = torch.empty((1, C1 + C2, 2 * h + 2, 2 * w + 2), device=x.device, dtype=torch.float32)
        self._call(self.ctx.lib.vido_upcat_reflect, x.data_ptr(), _p(skip), C1, C2, h, w, out.data_ptr())
        return out

    def minmax_norm_u16(self, d):
        """((d - d.min()) / (d.max() - d.min() + 1e-12) * 65536).clamp(0, 65535).to(int32) with one reduction and one pass."""
        d = d.contiguous()
        mm = torch.stack(torch.aminmax(d))
        out = torch.empty(d.shape, device=d.device, dtype=torch.int32)
        self._call(self.ctx.lib.vido_minmax_norm_u16, d.data_ptr(), mm.data_ptr(), d.numel(), out.data_ptr())
        return out

    def area_feed(self, bgr, feed, div=1.0):
        """u8 HxWx3 BGR device tensor -> f32 [1,3,feed_h,feed_w] RGB, area-resized, / div (flip + permute + float + interpolate(area) + div in one pass)"""
        assert bgr.is_cuda and bgr.dtype == torch.uint8 and bgr.is_contiguous() and bgr.dim() == 3 and bgr.shape[2] == 3
        out = torch.empty((1, 3, int(feed[0]), int(feed[1])), device=bgr.device, dtype=torch.float32)
        self._call(self.ctx.lib.vido_area_feed, bgr.data_ptr(), bgr.shape[0], bgr.shape[1], out.data_ptr(), int(feed[0]), int(feed[1]), div)
        return out

    def backwarp(self, x, flow):
        """layers.py Backward: bilinear warp of x by flow (pixels), zero padding"""
        assert x.is_cuda and x.dtype == torch.float32 and flow.dtype == torch.float32 and x.shape[0] == flow.shape[0] and x.shape[2:] == flow.shape[2:] and flow.shape[1] == 2
        x = x.contiguous(); flow = flow.contiguous()
        out = torch.empty_like(x)
        self._call(self.ctx.lib.vido_backwarp, x.data_ptr(), flow.data_ptr(), x.shape[0], x.shape[1], x.shape[2], x.shape[3], out.data_ptr())
        return out

    def deconv4s2_depthwise(self, x, weight, input_slope=1.0):
        """ConvTranspose2d(C, C, 4, 2, 1, groups=C, bias=False)(leaky_relu(x, input_slope)) in one HIP pass."""
        x = x.contiguous(); B, Cc, H, W = x.shape
        assert weight.shape == (Cc, 1, 4, 4) and weight.is_contiguous()
        out = torch.empty((B, Cc, 2 * H, 2 * W), device=x.device, dtype=torch.float32)
        self._call(self.ctx.lib.vido_deconv4s2_depthwise, x.data_ptr(), weight.data_ptr(), B, Cc, H, W, input_slope, out.data_ptr())
        return out

    def gconv3x3_supported(self, H, W, cpg_in, cpg_out):
        return bool(self.ctx.lib.vido_gconv3x3_supported(int(H), int(W), int(cpg_in), int(cpg_out)))

    def gconv3x3_bias_act(self, x, w_packed, bias, groups, slope=0.0, in_bias=None):
        """leaky_relu(conv2d(x', w, None, 1, 1, 1, groups) + bias, slope) for one image as one matrix-core launch; w_packed = pack_gconv3x3(w, groups);
        x' = x, or relu(x + in_bias[None, :, None, None]) when in_bias is given."""
        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and x.shape[0] == 1
        _, Cin, H, W = x.shape
        cpg_in = Cin // groups; cpg_out = bias.numel() // groups
        out = torch.empty((1, bias.numel(), H, W), device=x.device, dtype=torch.float32)
        self._count_flops(2.0 * bias.numel() * cpg_in * 9 * H * W)
        self._call(self.ctx.lib.vido_gconv3x3_bias_act, x.data_ptr(), _p(in_bias), w_packed.data_ptr(), bias.data_ptr(), out.data_ptr(), int(groups), cpg_in, cpg_out, H, W, slope)
        return out

    def gconv3x3_h_supported(self, H, W, cpg_in, cpg_out):
        return bool(self.ctx.lib.vido_gconv3x3_h_supported(int(H), int(W), int(cpg_in), int(cpg_out)))

    def gconv3x3_h_bias_act(self, x, w_packed, bias, groups, slope=0.0):
        """leaky_relu(conv2d(x, w, None, 1, 1, 1, groups) + bias, slope) for one image as one split-fp16 launch (csrc/gconvh.hip: 32 -> 32 or 64 -> 64 channels per group);
        w_packed = pack_gconv3x3_h(w, groups).  Activations must be finite and below 65504 in magnitude (conv1x1_range_flag otherwise)."""
        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and x.shape[0] == 1
        _, Cin, H, W = x.shape
        cpg = Cin // groups
        assert bias.numel() == Cin and w_packed.dtype == torch.int16 and w_packed.numel() == 2 * Cin * (cpg * 9 + 1), "gconv3x3_h: weight not packed by pack_gconv3x3_h for this layer"
        out = torch.empty((1, Cin, H, W), device=x.device, dtype=torch.float32)
        self._count_flops(2.0 * Cin * cpg * 9 * H * W)
        self._call(self.ctx.lib.vido_gconv3x3_h_bias_act, x.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), out.data_ptr(), int(groups), cpg, cpg, H, W, slope)
        return out

    def gconv3x3_hs_supported(self, H, W, cpg_in, cpg_out):
        return bool(self.ctx.lib.vido_gconv3x3_hs_supported(int(H), int(W), int(cpg_in), int(cpg_out)))

    def gconv3x3_hs_bias_act(self, x, w_packed, bias, groups, slope=0.0):
        """leaky_relu(conv2d(x, w, None, 1, 1, 1, groups) + bias, slope) for one image as one split-fp16 launch (csrc/gconvhs.hip: 8 -> 8 or 16 -> 16 channels per group, any W);
        w_packed = pack_gconv3x3_hs(w, groups).  Activations must be finite and below 65504 in magnitude (conv1x1_range_flag otherwise)."""
        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and x.shape[0] == 1
        _, Cin, H, W = x.shape
        cpg = Cin // groups
        assert cpg in (8, 16) and bias.numel() == Cin and w_packed.dtype == torch.int16 and w_packed.numel() == int(groups) * (3 if cpg == 8 else 5) * 1024 + 2 * Cin, \
            "gconv3x3_hs: weight not packed by pack_gconv3x3_hs for this layer"
        out = torch.empty((1, Cin, H, W), device=x.device, dtype=torch.float32)
        self._count_flops(2.0 * Cin * cpg * 9 * H * W)
        self._call(self.ctx.lib.vido_gconv3x3_hs_bias_act, x.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), out.data_ptr(), int(groups), cpg, cpg, H, W, slope)
        return out

    def gconv3x3_conv(self, x, w_packed, w_packed_h, bias, groups, slope=0.0, in_bias=None, w_packed_hs=None):
        """The grouped 3x3 convolution of a ResNeXt bottleneck: a split-fp16 kernel — gconv3x3_h_bias_act (w_packed_h = pack_gconv3x3_h(w, groups) or None: 32 / 64 channels per
        group) or gconv3x3_hs_bias_act (w_packed_hs = pack_gconv3x3_hs(w, groups) or None: 8 / 16 per group, unless VIDO_GCONV_HS is 0) — when the operand needs no input bias, the
        kernel takes the shape, the arithmetic setting is not f32 (conv1x1_set_arith(1) / VIDO_CONV1X1_ARITH=f32), no range_safe scope holds this object and VIDO_GCONV_H is not 0;
        in every other case gconv3x3_bias_act (fp32 matrix instruction, w_packed = pack_gconv3x3(w, groups))."""
        cpg = x.shape[1] // groups
        if (_GCONV_H and in_bias is None and not self._range_safe and bias.numel() == x.shape[1] and (w_packed_h is not None or (_GCONV_HS and w_packed_hs is not None))
                and int(self.ctx.lib.vido_conv1x1_get_arith()) != 1):
            if w_packed_h is not None and self.gconv3x3_h_supported(x.shape[2], x.shape[3], cpg, cpg):
                return self.gconv3x3_h_bias_act(x, w_packed_h, bias, groups, slope)
            if _GCONV_HS and w_packed_hs is not None and self.gconv3x3_hs_supported(x.shape[2], x.shape[3], cpg, cpg):
                return self.gconv3x3_hs_bias_act(x, w_packed_hs, bias, groups, slope)
        return self.gconv3x3_bias_act(x, w_packed, bias, groups, slope, in_bias=in_bias)

    def gconv3x3_s2_supported(self, H, W, cpg_in, cpg_out):
        return bool(self.ctx.lib.vido_gconv3x3_s2_supported(int(H), int(W), int(cpg_in), int(cpg_out)))

    def gconv3x3_s2_bias_act(self, x, w_packed, bias, groups, slope=0.0):
        """leaky_relu(conv2d(x, w, None, 2, 1, 1, groups) + bias, slope) for one image as one matrix-core launch (csrc/gconv.hip::k_gconv3x3_s2_m32); w_packed = pack_gconv3x3(w, groups)."""
        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and x.shape[0] == 1
        _, Cin, H, W = x.shape
        cpg_in = Cin // groups; cpg_out = bias.numel() // groups
        out = torch.empty((1, bias.numel(), (H + 1) // 2, W // 2), device=x.device, dtype=torch.float32)
        self._count_flops(2.0 * bias.numel() * cpg_in * 9 * out.shape[2] * out.shape[3])
        self._call(self.ctx.lib.vido_gconv3x3_s2_bias_act, x.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), out.data_ptr(), int(groups), cpg_in, cpg_out, H, W, slope)
        return out

    def conv1x1_supported(self, cin, cout, hw):
        return bool(self.ctx.lib.vido_conv1x1_supported(int(cin), int(cout), int(hw)))

    def conv1x1_set_arith(self, arith):
        """0: split-fp16 (two planes, three products; fp32-equivalent, the default), 1: the fp32 matrix instruction, 2: split-bf16 (three planes, six products; fp32's range);
        returns the previous setting (vido_conv1x1_set_arith, process-wide)."""
        return int(self.ctx.lib.vido_conv1x1_set_arith(int(arith)))

    def range_latch(self, dst):
        """Enqueue on the current stream: dst |= this context's range flag, flag = 0 (vido_range_latch).  dst: an int32 tensor of one element or more (its first word), on the
        device or pinned on the host; zero it before the launches it is to cover.  In stream order dst then holds the trips of the split-fp16 launches enqueued before the latch."""
        assert dst.dtype == torch.int32 and dst.numel() >= 1 and dst.is_contiguous() and (dst.is_cuda or dst.is_pinned()), "range_latch: an int32 word on the device or pinned"
        self._call(self.ctx.lib.vido_range_latch, dst.data_ptr())
        return dst

    def conv1x1_range_flag(self, reset=True):
        """non-zero when a split-fp16 launch met |x| >= 65504 since the last reset (its outputs are not valid); read after the stream has been waited for"""
        return int(self.ctx.lib.vido_conv1x1_range_flag(self.ctx.h, int(bool(reset))))

    def conv1x1_layout(self, cin, cout, hw):
        return int(self.ctx.lib.vido_conv1x1_layout(int(cin), int(cout), int(hw)))

    def conv1x1_bias_act(self, x, w_packed, bias=None, residual=None, slope=1.0, residual_up2=None):
        """leaky_relu(conv2d(x, w) + bias + residual, slope) for one image, 1x1 kernel, stride 1, as one matrix-core GEMM launch (csrc/conv1x1.hip);
        w_packed = pack_conv1x1(w, layout) of any layout — the launch runs in the arithmetic the weight was packed for, whatever conv1x1_set_arith says by now — or a
        PackedConv1x1.  slope 0 = ReLU, 1 = none.  residual_up2: a residual at half the resolution, added nearest-upsampled (the FPN's top-down sum)."""
        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and x.shape[0] == 1
        _, cin, H, W = x.shape
        if isinstance(w_packed, PackedConv1x1):                     # packed on first use, in the layout the library recommends under the current arithmetic setting
            w_packed = w_packed.get(self.conv1x1_layout(cin, w_packed.cout, H * W), x.device)
        layout, cout = packed_conv1x1_layout(w_packed, cin)
        assert 0.0 <= slope <= 1.0 and (residual is None or residual_up2 is None)
        out = torch.empty((1, cout, H, W), device=x.device, dtype=torch.float32)
        self._count_flops(2.0 * cout * cin * H * W)
        if residual_up2 is not None:
            residual_up2 = residual_up2.contiguous(); assert tuple(residual_up2.shape) == (1, cout, H // 2, W // 2) and H % 2 == 0 and W % 2 == 0
            self._call(self.ctx.lib.vido_conv1x1_bias_up2_act, x.data_ptr(), w_packed.data_ptr(), _p(bias), residual_up2.data_ptr(), out.data_ptr(), int(cin), int(cout), int(H), int(W), slope, layout)
            return out
        if residual is not None:
            residual = residual.contiguous(); assert residual.shape == out.shape
        self._call(self.ctx.lib.vido_conv1x1_bias_act, x.data_ptr(), w_packed.data_ptr(), _p(bias), _p(residual), out.data_ptr(), int(cin), int(cout), int(H * W), slope, layout)
        return out

    def conv1x1_conv(self, conv, x, slope=1.0, residual=None, residual_up2=None):
        """The 1x1 convolution `conv` (nn.Conv2d, stride 1) + bias (+ residual) + activation through conv1x1_bias_act when the layer has that form, else None; the packed weight
        is cached on the module (per layout) and rebuilt when the weight tensor changes."""
        w = conv.weight
        if (tuple(w.shape[2:]) != (1, 1) or tuple(conv.stride) != (1, 1) or tuple(conv.padding) != (0, 0) or conv.groups != 1 or not x.is_cuda or x.shape[0] != 1
                or self._range_safe or not self.conv1x1_supported(w.shape[1], w.shape[0], x.shape[2] * x.shape[3])):
            return None                                                       # (range_safe: the library convolution, not the fp32 form, whose layout follows vido_conv1x1_set_arith)
        if not conv1x1_fills_chip(w.shape[0], x.shape[2] * x.shape[3]):
            return None
        layout = self.conv1x1_layout(w.shape[1], w.shape[0], x.shape[2] * x.shape[3])
        wp = cached_pack(conv, "_c1_w", w, x.device, (layout,), lambda: pack_conv1x1(w, layout).to(x.device))      # (the layout is a key part: one pack, of the form last met)
        return self.conv1x1_bias_act(x.contiguous(), wp, conv.bias, residual, slope, residual_up2)

    def conv_kxk_c2(self, conv, x, residual=None):
        """conv(x) + residual for a k x k (3, 5, 7) stride-1 `same` convolution with TWO output channels on one image — the last layer of LiteFlowNet's flow heads — as one
        stencil launch (csrc/convsmall.hip) instead of the library's im2col + GEMM + our bias / residual pass; None when the layer is not of that form."""
        w = conv.weight
        k = int(w.shape[2])
        if (w.shape[0] != 2 or w.shape[2] != w.shape[3] or k not in (3, 5, 7) or tuple(conv.stride) != (1, 1) or tuple(conv.padding) != (k // 2, k // 2) or tuple(conv.dilation) != (1, 1)
                or conv.groups != 1 or not x.is_cuda or x.shape[0] != 1 or x.dtype != torch.float32):
            return None
        x = x.contiguous(); wc = w.contiguous()
        _, cin, H, W = x.shape
        out = torch.empty((1, 2, H, W), device=x.device, dtype=torch.float32)
        if residual is not None:
            residual = residual.contiguous(); assert residual.shape == out.shape
        self._count_flops(2.0 * 2 * cin * k * k * H * W)
        self._call(self.ctx.lib.vido_conv_kxk_c2, x.data_ptr(), wc.data_ptr(), _p(conv.bias), _p(residual), out.data_ptr(), int(cin), k, int(H), int(W))
        return out

    def conv1x1_skinny(self, x, w_packed, bias, cout, slope=1.0, residual=None):
        """leaky_relu(conv2d(x, w) + bias + residual, slope), 1x1, one image, cin even <= 256, cout <= 256: one launch without LDS (csrc/convsmall.hip::k_conv1x1_skinny);
        w_packed = pack_conv1x1_skinny(w) on the device."""
        assert x.is_cuda and x.dtype == torch.float32 and x.shape[0] == 1
        x = x.contiguous(); cin, H, W = int(x.shape[1]), int(x.shape[2]), int(x.shape[3])
        out = torch.empty((1, cout, H, W), device=x.device, dtype=torch.float32)
        if residual is not None:
            residual = residual.contiguous(); assert residual.shape == out.shape
        self._count_flops(2.0 * cout * cin * H * W)
        self._call(self.ctx.lib.vido_conv1x1_skinny, x.data_ptr(), w_packed.data_ptr(), _p(bias), _p(residual), out.data_ptr(), cin, int(cout), H * W, slope)
        return out

    def conv1x1_skinny_conv(self, conv, x, slope=1.0):
        """The same for an nn.Conv2d (LiteFlowNet's netFeat layers); None when the layer is not of that form.  Packed weight cached on the module."""
        w = conv.weight
        cout, cin = int(w.shape[0]), int(w.shape[1])
        if (tuple(w.shape[2:]) != (1, 1) or tuple(conv.stride) != (1, 1) or tuple(conv.padding) != (0, 0) or conv.groups != 1 or cin % 2 or cin > 256 or cout > 256
                or not x.is_cuda or x.shape[0] != 1 or x.dtype != torch.float32):
            return None
        return self.conv1x1_skinny(x, cached_pack(conv, "_c1s_w", w, x.device, (), lambda: pack_conv1x1_skinny(w).to(x.device)), conv.bias, cout, slope)

    def stem7x7s2_pool(self, x, w_packed, bias):
        """max_pool2d(relu(conv2d(x, w, None, 2, 3) + bias), 3, 2, 1) for one image, 7x7, 3 -> 64 channels, as ONE launch whose convolution output stays on the chip
        (csrc/stem.hip); w_packed = pack_stem7x7(w) on the device."""
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] == 1 and x.shape[1] == 3 and tuple(w_packed.shape) == (2, 84, 64) and bias.numel() == 64
        x = x.contiguous(); H, W = int(x.shape[2]), int(x.shape[3])
        Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        out = torch.empty((1, 64, (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1), device=x.device, dtype=torch.float32)
        self._count_flops(2.0 * 64 * 147 * Hc * Wc)
        self._call(self.ctx.lib.vido_stem7x7s2_pool, x.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), out.data_ptr(), H, W)
        return out

    def stem7x7s2_pool_conv(self, mod, w, bias, x):
        """The same for a folded stem weight `w` [64, 3, 7, 7] / `bias` [64]; None when they are not of that form.  Packed weight cached on `mod`, rebuilt when `w` changes."""
        if tuple(w.shape) != (64, 3, 7, 7) or bias is None or bias.numel() != 64 or not x.is_cuda or x.shape[0] != 1 or x.shape[1] != 3 or x.dtype != torch.float32 or w.dtype != torch.float32:
            return None
        wp, bp = cached_pack(mod, "_stem_w", w, x.device, (), lambda: (pack_stem7x7(w).to(x.device), bias.detach().to(x.device).contiguous()))
        return self.stem7x7s2_pool(x, wp, bp)

    def wino3x3_supported(self, cin, cout, H, W):
        return bool(self.ctx.lib.vido_wino3x3_supported(int(cin), int(cout), int(H), int(W)))

    def wino3x3_form(self, N, cin, cout, H, W):
        """0: the tile form, 1: the K-split form (launches that would leave most of the chip idle) — the library's own rule, vido_wino3x3_form"""
        return int(self.ctx.lib.vido_wino3x3_form(int(N), int(cin), int(cout), int(H), int(W)))

    def wino3x3_bias_act(self, x, u_packed, bias, cout, slope=1.0, form=0):
        """leaky_relu(conv2d(x, w, None, 1, 1) + bias, slope) for a batch, 3x3 kernel, as one Winograd launch whose channel contractions run on the matrix pipe (csrc/wino.hip);
        u_packed = pack_wino3x3(w, form) on x's device.  slope 0 = ReLU, 1 = none."""
        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and u_packed.is_cuda
        N, cin, H, W = x.shape
        out = torch.empty((N, cout, H, W), device=x.device, dtype=torch.float32)
        self._count_flops(2.0 * N * cout * cin * 9 * H * W)                                                  # direct-convolution count, as FlopCounterMode would give the library call
        self._call(self.ctx.lib.vido_wino3x3_bias_act_form, x.data_ptr(), u_packed.data_ptr(), _p(bias), out.data_ptr(), int(N), int(cin), int(cout), int(H), int(W), slope, int(form))
        return out

    def wino3x3_conv(self, conv, x, slope, weight=None, bias=None, n_live=None):
        """The convolution `conv` (nn.Conv2d, or the folded weight / bias given) + bias + activation through wino3x3_bias_act when the layer has that form, else None.  The
        packed weight is cached on the module and rebuilt when the weight tensor changes (a checkpoint loaded later).
        n_live (one int32 device word): the direct split-fp16 kernel computes the first n_live images only and never reads the others; the fp32 Winograd route computes all."""
        w = conv.weight if weight is None else weight
        b = conv.bias if bias is None and weight is None else bias
        if (tuple(w.shape[2:]) != (3, 3) or tuple(conv.stride) != (1, 1) or tuple(conv.padding) != (1, 1) or tuple(conv.dilation) != (1, 1) or conv.groups != 1
                or getattr(conv, "padding_mode", "zeros") != "zeros" or not x.is_cuda or not self.wino3x3_supported(w.shape[1], w.shape[0], x.shape[2], x.shape[3])
                or 4 * x.numel() >= 1 << 30 or 4 * x.shape[0] * w.shape[0] * x.shape[2] * x.shape[3] >= 1 << 30):
            return None
        # a launch of a few dozen workgroups of the tile form (small maps) runs as long as a chip-filling one; those take the K-split form (four waves of a workgroup share
        # the input channels).  VIDO_WINO_MIN_WGS=128 restores the rule of round 4 (the library's kernels below 128 workgroups).
        if _WINO_MIN_WGS > 0 and not self.ctx.lib.vido_wino3x3_fills_chip(int(x.shape[0]), int(w.shape[0]), int(x.shape[2]), int(x.shape[3]), _WINO_MIN_WGS):
            return None
        # (round 6) chip-filling launches of >= 128-channel layers take the DIRECT kernel in split-fp16 arithmetic (csrc/conv3x3h.hip): 256 -> 256 on 200 x 272 in 216 us
        # against the Winograd kernel's 325, the mask head's 100 x 14 x 14 in 97 against 156; below ~128 workgroups one workgroup's
        # K loop is the launch's time and Winograd (its K-split form) stays faster.  VIDO_CONV3X3_H=0 keeps Winograd everywhere; VIDO_CONV3X3_H_MIN_WGS moves the threshold.
        if (_CONV3X3_H_MIN_WGS > 0 and x.dtype == torch.float32 and not self._range_safe and self.ctx.lib.vido_conv3x3_h_supported(int(x.shape[0]), int(w.shape[1]), int(w.shape[0]), int(x.shape[2]), int(x.shape[3]))
                and self.ctx.lib.vido_conv3x3_h_workgroups(int(x.shape[0]), int(w.shape[0]), int(x.shape[2]), int(x.shape[3])) >= (1 if int(w.shape[0]) == 64 else _CONV3X3_H_MIN_WGS)):
            # (64-channel layers: the direct kernel wins at every size — 128 -> 64 on 30 x 40: 18 us against the K-split Winograd form's 26; profiles/r6/conv3x3_h_direct.txt)
            wp = cached_pack(conv, "_c3h_w", w, x.device, (), lambda: pack_conv3x3_h(w).to(x.device))
            return self.conv3x3_h_bias_act(x.contiguous(), wp, b, int(w.shape[0]), slope, n_live)
        form = self.wino3x3_form(x.shape[0], w.shape[1], w.shape[0], x.shape[2], x.shape[3])
        u = cached_pack(conv, "_wino_u", w, x.device, (), dict)                # per form: a layer shared by several map sizes (the RPN head over P2-P6) is launched in both
        if form not in u:
            u[form] = pack_wino3x3(w, form).to(x.device)
        return self.wino3x3_bias_act(x.contiguous(), u[form], b, int(w.shape[0]), slope, form)

    def conv3x3_h_bias_act(self, x, w_packed, bias, cout, slope, n_live=None):
        """leaky_relu(conv2d(x, w, stride 1, padding 1) + bias, slope) as one direct split-fp16 launch (csrc/conv3x3h.hip); w_packed = pack_conv3x3_h(w).
        n_live (one int32 device word): only the first n_live images are read and written (vido_conv3x3_h_bias_act_n); the rest of the result is uninitialised."""
        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32
        N, cin, H, W = x.shape
        assert w_packed.dtype == torch.int16 and w_packed.numel() == 2 * cout * ((cin + 15) // 16 * 16 * 9 + 1), "conv3x3_h: weight not packed by pack_conv3x3_h for this layer"
        out = torch.empty((N, cout, H, W), device=x.device, dtype=torch.float32)
        self._count_flops(2.0 * N * cout * cin * 9 * H * W)
        self._call(self.ctx.lib.vido_conv3x3_h_bias_act_n, x.data_ptr(), w_packed.data_ptr(), _p(bias), out.data_ptr(), int(N), int(cin), int(cout), int(H), int(W), slope, self._live_ptr(n_live))
        return out

    def conv3x3_h_live_form(self, n, cout, h, w, live):
        """(fine, channels per workgroup, block rows) of the form the counted conv3x3_h launch runs at the count word `live` (vido_conv3x3_h_live_form)"""
        ch, br = C.c_int(), C.c_int()
        fine = self.ctx.lib.vido_conv3x3_h_live_form(int(n), int(cout), int(h), int(w), int(live), C.byref(ch), C.byref(br))
        return bool(fine), ch.value, br.value

    def fc_h(self, x, w_packed, bias, outs, slope=1.0):
        """leaky_relu(x @ w.T + bias, slope) for x [rows, k] f32 as a split-fp16 matrix-pipe GEMM split over k (csrc/fch.hip); w_packed = pack_conv1x1(w[:, :, None, None], 3).
        None when the library does not take the shape."""
        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and x.dim() == 2
        rows, k = int(x.shape[0]), int(x.shape[1])
        S = int(self.ctx.lib.vido_fc_h_splitk(rows, k, int(outs)))
        if S <= 0:
            return None
        assert w_packed.dtype == torch.int16 and w_packed.numel() == 2 * outs * (k + 1), "fc_h: weight not packed (pack_conv1x1(w[:, :, None, None], 3))"
        part = torch.empty((S, rows, outs), device=x.device, dtype=torch.float32); y = torch.empty((rows, outs), device=x.device, dtype=torch.float32)
        self._count_flops(2.0 * rows * k * outs)
        self._call(self.ctx.lib.vido_fc_h, x.data_ptr(), w_packed.data_ptr(), _p(bias), part.data_ptr(), y.data_ptr(), rows, k, int(outs), slope)
        return y

    def fc_h_linear(self, lin, x, slope=1.0):
        """nn.Linear `lin` + activation through fc_h when the layer has that form (outputs a multiple of 128, inputs a multiple of 32 S), else None; the packed weight is cached
        on the module and rebuilt when the weight tensor changes."""
        w = lin.weight
        if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or os.environ.get("VIDO_NO_FC_H") or self._range_safe or int(self.ctx.lib.vido_fc_h_splitk(int(x.shape[0]), int(w.shape[1]), int(w.shape[0]))) <= 0:
            return None
        wp = cached_pack(lin, "_fch_w", w, x.device, (), lambda: pack_conv1x1(w.detach().reshape(int(w.shape[0]), int(w.shape[1]), 1, 1), 3).to(x.device))
        return self.fc_h(x.contiguous(), wp, lin.bias, int(w.shape[0]), slope)

    def conv_direct_conv(self, conv, x, slope):
        """The convolution `conv` (nn.Conv2d: groups 1, dilation 1, zero padding, a k x k of csrc/convdirect.hip) + bias + activation as ONE direct implicit-GEMM launch on
        the matrix pipe, else None.  The packed weight is cached on the module and rebuilt when the weight tensor changes."""
        w = conv.weight
        kh, kw = int(w.shape[2]), int(w.shape[3]); sh, sw = (int(v) for v in conv.stride); ph, pw = (int(v) for v in conv.padding)
        if _CONVDIRECT_SET == "novalu" and (kh, kw) in ((3, 3), (7, 7)) and int(w.shape[0]) >= 32:
            return None                                                       # layers the library runs as Winograd on the VECTOR ALUs (see _CONVDIRECT_SET)
        if (tuple(conv.dilation) != (1, 1) or conv.groups != 1 or getattr(conv, "padding_mode", "zeros") != "zeros" or not x.is_cuda or x.dtype != torch.float32
                or not self.ctx.lib.vido_conv_direct_supported(int(w.shape[1]), int(w.shape[0]), int(x.shape[2]), int(x.shape[3]), kh, kw, sh, sw, ph, pw)
                or 4 * x.numel() >= 1 << 30):
            return None
        N, cin, H, W = x.shape; cout = int(w.shape[0])
        Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
        if 4 * N * cout * Ho * Wo >= 1 << 30:
            return None
        wp = cached_pack(conv, "_cd_w", w, x.device, (), lambda: pack_conv_direct(w).to(x.device))
        x = x.contiguous()
        out = torch.empty((N, cout, Ho, Wo), device=x.device, dtype=torch.float32)
        self._count_flops(2.0 * N * cout * cin * kh * kw * Ho * Wo)
        self._call(self.ctx.lib.vido_conv_direct_bias_act, x.data_ptr(), wp.data_ptr(), _p(conv.bias), out.data_ptr(), int(N), int(cin), cout, int(H), int(W), kh, kw, sh, sw, ph, pw, slope)
        return out

    def lfn_reg_front(self, im1, im2, flow, scale, feat):
        """Regularization.forward up to netMain's input (layers.py:236-243): torch.cat([sqrt(sum((im1 - Backward(im2, flow * scale))^2)), flow - mean(flow), feat], 1) with the
        first three channels from one HIP pass."""
        im1 = im1.contiguous(); im2 = im2.contiguous(); flow = flow.contiguous()
        B, Cc, H, W = im1.shape
        out = torch.empty((B, 3 + feat.shape[1], H, W), device=im1.device, dtype=torch.float32)
        mean = flow.flatten(2).mean(2).contiguous()
        self._call(self.ctx.lib.vido_lfn_reg_front, im1.data_ptr(), im2.data_ptr(), flow.data_ptr(), mean.data_ptr(), scale, B, Cc, H, W, out.data_ptr(), out.shape[1])
        out[:, 3:] = feat
        return out

    def lfn_reg_tail(self, dist, flow, scale_x, scale_y, k):
        """Regularization.forward after netDist (layers.py:245-262); scale_x / scale_y: the netScaleX / netScaleY modules (Conv2d(k*k, 1, 1))."""
        dist = dist.contiguous(); flow = flow.contiguous()
        B, nd, H, W = dist.shape
        assert nd == k * k
        out = torch.empty((B, 2, H, W), device=dist.device, dtype=torch.float32)
        self._call(self.ctx.lib.vido_lfn_reg_tail, dist.data_ptr(), flow.data_ptr(), scale_x.weight.data_ptr(), scale_x.bias.data_ptr(), scale_y.weight.data_ptr(), scale_y.bias.data_ptr(),
                   B, int(k), H, W, out.data_ptr())
        return out

    def roi_align(self, feat, rois, output_size, spatial_scale, sampling_ratio):
        if not feat.is_cuda:
            raise RuntimeError("HipOps.roi_align needs CUDA(HIP) tensors; there is no CPU fallback")
        feat = feat.contiguous().float(); rois = rois.contiguous().float()
        B, Cc, H, W = feat.shape; ph, pw = output_size
        out = torch.empty((rois.shape[0], Cc, ph, pw), device=feat.device, dtype=torch.float32)
        self._call(self.ctx.lib.vido_roi_align, feat.data_ptr(), B, Cc, H, W, rois.data_ptr(), rois.shape[0], spatial_scale, ph, pw, sampling_ratio, out.data_ptr(), 1)
        return out

    def box_decode(self, deltas, boxes, weights):
        """BoxCoder(weights).decode(deltas [n,4k], boxes [n,4]) -> [n,4k]."""
        deltas = deltas.contiguous().float(); boxes = boxes.contiguous().float(); n = deltas.shape[0]
        out = torch.empty_like(deltas)
        if n:
            w = (C.c_float * 4)(*[float(x) for x in weights])
            self._call(self.ctx.lib.vido_box_decode, deltas.data_ptr(), boxes.data_ptr(), n, deltas.shape[1] // 4, w, out.data_ptr(), 1)
        return out

    def nms_grouped(self, boxes, scores, groups, thresh):
        """layers.nms applied independently per group (the box head's per-class loop in one launch pair): kept original
        indices, ascending."""
        if not boxes.is_cuda:
            raise RuntimeError("HipOps.nms_grouped needs CUDA(HIP) tensors; there is no CPU fallback")
        if boxes.shape[0] == 0:
            return torch.zeros((0,), dtype=torch.int64, device=boxes.device)
        order = torch.sort(scores, descending=True, stable=True)[1]
        n = boxes.shape[0]
        if n <= 65536:
            # one SEGMENT PER GROUP (k_nms_mask_seg / k_nms_sweep_seg: one wave per segment, all of them in one launch pair): the groups are independent NMS problems,
            # so sort by (group, score descending) and let every class sweep its own few hundred boxes — a single segment with a group mask swept all candidates
            # block by block on ONE wave (210 us at ~5 000 candidates)
            order = order[torch.sort(groups[order], stable=True)[1]]
            cnts = torch.bincount(groups, minlength=1).to(torch.int32)
            seg_off = (torch.cumsum(cnts, 0) - cnts).to(torch.int32)
            max_n = int(cnts.max().item())
            keep, cnt = self.nms_segments(boxes[order], seg_off, cnts, max_n, thresh)
            flat = (keep.long() + seg_off.long()[:, None])[keep >= 0]
            return torch.sort(order[flat])[0]
        sb = boxes[order].contiguous().float(); sg = groups[order].to(torch.int32).contiguous()
        keep = torch.empty(n, device=boxes.device, dtype=torch.int32); cnt = torch.zeros(1, device=boxes.device, dtype=torch.int32)
        self._call(self.ctx.lib.vido_nms_grouped, sb.data_ptr(), None, sg.data_ptr(), n, thresh, keep.data_ptr(), cnt.data_ptr(), 1)
        m = int(cnt.item())
        return torch.sort(order[keep[:m].long()])[0]

    def nms(self, boxes, scores, thresh):
        """maskrcnn_benchmark.layers.nms: kept original indices, ascending (sort on the device with torch, sweep in HIP)."""
        if not boxes.is_cuda:
            raise RuntimeError("HipOps.nms needs CUDA(HIP) tensors; there is no CPU fallback")
        if boxes.shape[0] == 0:
            return torch.zeros((0,), dtype=torch.int64, device=boxes.device)
        order = torch.sort(scores, descending=True, stable=True)[1]
        sb = boxes[order].contiguous().float(); n = sb.shape[0]
        keep = torch.empty(max(n, 1), device=boxes.device, dtype=torch.int32); cnt = torch.zeros(1, device=boxes.device, dtype=torch.int32)
        self._call(self.ctx.lib.vido_nms, sb.data_ptr(), None, n, thresh, keep.data_ptr(), cnt.data_ptr(), 1)
        m = int(cnt.item())
        return torch.sort(order[keep[:m].long()])[0]

    # ---- device-only variants used by the no-host-round-trip inference path (nets/maskrcnn.py fast path) ------------------------------------
    def nms_segments(self, boxes, seg_off, seg_n, max_n, thresh, groups=None):
        """layers.nms on len(seg_n) independent segments of `boxes` (each sorted by descending score): (keep [n_seg, max_n] positions relative to the
        segment start, ascending, -1 padded; n_keep [n_seg]) — device tensors, no synchronisation."""
        boxes = boxes.contiguous().float(); n_seg = seg_n.shape[0]
        keep = torch.empty((n_seg, max_n), device=boxes.device, dtype=torch.int32); cnt = torch.empty(n_seg, device=boxes.device, dtype=torch.int32)
        self._call(self.ctx.lib.vido_nms_segments, boxes.data_ptr(), _p(groups), seg_off.data_ptr(), seg_n.data_ptr(), n_seg, int(max_n), boxes.shape[0], thresh, keep.data_ptr(), cnt.data_ptr())
        return keep, cnt

    def roi_align_fpn(self, feats, boxes, level, output_size, scales, sampling_ratio):
        """Pooler.forward in one launch: feats = the 4 FPN maps [1,C,H,W], boxes [n,4], level [n] int32 in 0..3."""
        n = boxes.shape[0]; ph, pw = output_size; Cc = feats[0].shape[1]
        out = torch.empty((n, Cc, ph, pw), device=boxes.device, dtype=torch.float32)
        if n == 0:
            return out
        feats = [f.contiguous().float() for f in feats]; boxes = boxes.contiguous().float(); level = level.to(torch.int32).contiguous()
        fp = (C.c_void_p * 4)(*[f.data_ptr() for f in feats]); Hs = (C.c_int * 4)(*[f.shape[2] for f in feats]); Ws = (C.c_int * 4)(*[f.shape[3] for f in feats])
        sc = (C.c_float * 4)(*[float(x) for x in scales])
        self._call(self.ctx.lib.vido_roi_align_fpn, fp, Hs, Ws, sc, Cc, boxes.data_ptr(), level.data_ptr(), n, ph, pw, sampling_ratio, out.data_ptr())
        return out

    # ---- detpost.hip: the detector's selection logic as ordered device kernels -----------------------------------------------------------------------------
    def rpn_select(self, logits, deltas, cell_anchors, strides, K, image_wh):
        """rpn/inference.py:73-105 for all levels in one launch: (boxes [L*K,4], scores [L*K] (-1 = padding), n [L])."""
        L = len(logits); A = logits[0].shape[1]; dev = logits[0].device
        logits = [t.contiguous() for t in logits]; deltas = [t.contiguous() for t in deltas]
        boxes = torch.empty((L * K, 4), device=dev, dtype=torch.float32); scores = torch.empty((L * K,), device=dev, dtype=torch.float32); n = torch.empty((L,), device=dev, dtype=torch.int32)
        lp = (C.c_void_p * L)(*[t.data_ptr() for t in logits]); dp = (C.c_void_p * L)(*[t.data_ptr() for t in deltas])
        hs = (C.c_int * L)(*[t.shape[2] for t in logits]); ws = (C.c_int * L)(*[t.shape[3] for t in logits]); st = (C.c_int * L)(*[int(s) for s in strides])
        key = ("anch", L, A)
        if getattr(self, "_anch_key", None) != key:                 # host copy of the cell anchors (module buffers): made once, outside any capture
            self._anch = (C.c_float * (L * A * 4))(*[float(v) for a in cell_anchors for v in a.detach().cpu().reshape(-1).tolist()]); self._anch_key = key
        self._call(self.ctx.lib.vido_rpn_select, L, lp, dp, hs, ws, st, self._anch, A, int(K), int(image_wh[0]), int(image_wh[1]), boxes.data_ptr(), scores.data_ptr(), n.data_ptr())
        return boxes, scores, n

    def rpn_merge(self, boxes, scores, keep, cnt, K, post_nms_top_n, n_final):
        L = cnt.shape[0]; dev = boxes.device
        ob = torch.empty((n_final, 4), device=dev, dtype=torch.float32); osc = torch.empty((n_final,), device=dev, dtype=torch.float32); nv = torch.empty((1,), device=dev, dtype=torch.int32)
        self._call(self.ctx.lib.vido_rpn_merge, boxes.data_ptr(), scores.data_ptr(), keep.data_ptr(), cnt.data_ptr(), L, int(K), int(post_nms_top_n), int(n_final),
                   ob.data_ptr(), osc.data_ptr(), nv.data_ptr())
        return ob, osc, nv

    def det_class_sort(self, prob, deltas, proposals, objectness, thresh, weights, image_wh):
        prob = prob.contiguous(); deltas = deltas.contiguous(); proposals = proposals.contiguous()
        N, nc = prob.shape; dev = prob.device
        seg = torch.empty(((nc - 1) * N, 4), device=dev, dtype=torch.float32); order = torch.empty((nc - 1, N), device=dev, dtype=torch.int32); seg_n = torch.empty((nc - 1,), device=dev, dtype=torch.int32)
        wv = (C.c_float * 4)(*[float(x) for x in weights])
        self._call(self.ctx.lib.vido_det_class_sort, prob.data_ptr(), deltas.data_ptr(), proposals.data_ptr(), _p(objectness), N, nc, thresh, wv, int(image_wh[0]), int(image_wh[1]),
                   seg.data_ptr(), order.data_ptr(), seg_n.data_ptr())
        return seg, order, seg_n

    def det_select(self, prob, seg_boxes, order, keep, cnt, detections_per_img, cap):
        N, nc = prob.shape; dev = prob.device
        ob = torch.empty((cap, 4), device=dev, dtype=torch.float32); osc = torch.empty((cap,), device=dev, dtype=torch.float32); ol = torch.empty((cap,), device=dev, dtype=torch.int64)
        nd = torch.empty((1,), device=dev, dtype=torch.int32); scratch = torch.empty((nc + 3,), device=dev, dtype=torch.int32)
        self._call(self.ctx.lib.vido_det_select, prob.data_ptr(), seg_boxes.data_ptr(), order.data_ptr(), keep.data_ptr(), cnt.data_ptr(), N, nc, int(detections_per_img), int(cap),
                   scratch.data_ptr(), ob.data_ptr(), osc.data_ptr(), ol.data_ptr(), nd.data_ptr())
        return ob, osc, ol, nd

    def to_nhwc(self, x):
        """[B,C,H,W] f32 -> channels-last copy [B,H,W,C] (vido_nchw_to_nhwc): the layout roi_align_fpn_nhwc reads."""
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
        x = x.contiguous(); B, Cc, H, W = x.shape
        out = torch.empty((B, H, W, Cc), device=x.device, dtype=torch.float32)
        self._call(self.ctx.lib.vido_nchw_to_nhwc, x.data_ptr(), B, Cc, H, W, out.data_ptr())
        return out

    def roi_align_fpn_nhwc(self, feats_nhwc, boxes, level, output_size, scales, sampling_ratio, n_live=None):
        """Pooler.forward over channels-last maps [1,H,W,C] (to_nhwc of the 4 FPN maps, made once per frame).  n_live (one int32 device word): only the first n_live boxes
        are pooled (vido_roi_align_fpn_nhwc_n); the other rows of the result are uninitialised."""
        n = boxes.shape[0]; ph, pw = output_size; Cc = feats_nhwc[0].shape[3]
        out = torch.empty((n, Cc, ph, pw), device=boxes.device, dtype=torch.float32)
        if n == 0:
            return out
        boxes = boxes.contiguous().float(); level = level.to(torch.int32).contiguous()
        fp = (C.c_void_p * 4)(*[f.data_ptr() for f in feats_nhwc]); Hs = (C.c_int * 4)(*[f.shape[1] for f in feats_nhwc]); Ws = (C.c_int * 4)(*[f.shape[2] for f in feats_nhwc])
        sc = (C.c_float * 4)(*[float(x) for x in scales])
        self._call(self.ctx.lib.vido_roi_align_fpn_nhwc_n, fp, Hs, Ws, sc, Cc, boxes.data_ptr(), level.data_ptr(), n, ph, pw, sampling_ratio, out.data_ptr(), self._live_ptr(n_live))
        return out

    def mask_label_image(self, masks, boxes, labels, H, W, thresh=0.5, padding=1, n_live=None):
        """Masker + label image: masks [n,1,M,M], boxes [n,4] (output image), labels [n] int64 -> [H,W] u8.  n_live (one int32 device word): the slots behind it all have
        label 0 (the static head's ordered list) and the walk stops there (vido_mask_label_image_n); the image is the same."""
        out = torch.empty((H, W), device=masks.device, dtype=torch.uint8)
        n = masks.shape[0]
        masks = masks.contiguous().float(); boxes = boxes.contiguous().float(); labels = labels.contiguous().to(torch.int64)
        self._call(self.ctx.lib.vido_mask_label_image_n, masks.data_ptr() if n else None, boxes.data_ptr() if n else None, labels.data_ptr() if n else None, n, masks.shape[-1] if n else 28,
                   padding, thresh, H, W, out.data_ptr(), self._live_ptr(n_live))
        return out

    def mask_propagate(self, mask, flow, depth=None, out=None, stats=None):
        """vido_mask_propagate on device tensors: mask int32 [H,W] of frame k-1, flow float32 [H,W,2] (dx, dy) from k-1 into k, depth float32 [H,W] of k-1 or None ->
        the label image of frame k, int32 [H,W] (`out`, or a new tensor).  A pixel with label > 0 and a usable flow vector (and depth, when given) lands on
        (x + rint(dx), y + rint(dy)); several on one pixel: the nearer, then the smaller label; an unhit pixel with 5 of 8 neighbours of one label takes it.  stats: an
        int32 tensor of >= 3 elements that receives (sources kept, pixels hit, pixels filled), or None.  Enqueued on torch's current stream, nothing is waited for; the
        first call of a context allocates, so it comes before a graph capture.  CPU tensors, other dtypes or shapes, non-contiguous tensors and out aliasing mask raise."""
        bad = _tensor_args("mask_propagate", (("mask", mask, torch.int32, True), ("flow", flow, torch.float32, True), ("depth", depth, torch.float32, False),
                                              ("out", out, torch.int32, False), ("stats", stats, torch.int32, False)))
        if mask.dim() != 2:
            bad("mask must be [H, W]")
        H, W = int(mask.shape[0]), int(mask.shape[1])
        if out is None:
            out = torch.empty((H, W), device=mask.device, dtype=torch.int32)
        _need(bad, "flow", flow, (H, W, 2)); _need(bad, "depth", depth, (H, W)); _need(bad, "out", out, (H, W))
        if _overlaps(out, mask, 4 * H * W):
            bad("out aliases mask")
        _need_count(bad, "stats", stats, 3)
        self._call(self.ctx.lib.vido_mask_propagate, mask.data_ptr(), flow.data_ptr(), _p(depth), H, W, out.data_ptr(), _p(stats))
        return out

    def dis_flow(self, prev, cur, out=None, q8=None, stats=None, coarsest=4, iters=6, max_shift_q8=1024, min_eig=0, rgb_order=0):
        """vido_dis_flow on device tensors: prev, cur uint8 [H,W] or [H,W,3|4] of one shape -> the dense flow from prev into cur, float32 [H,W,2] (dx, dy) in pixels
        (`out`, or a new tensor).  q8: an int32 [H,W,2] tensor that receives the same field in 1/256 px, or None; stats: an int32 tensor of >= 4 elements that receives
        (patches that kept an iterate, flat, rejected, steps), or None.  The rule is include/vido_c.h's, the numpy statement tests/refimpl/dis_flow_np.py.  Enqueued on
        torch's current stream, nothing is waited for; the first call of a size grows the context's scratch, so it comes before a graph capture.  CPU tensors, other
        dtypes or shapes and non-contiguous tensors raise."""
        bad = _tensor_args("dis_flow", (("prev", prev, torch.uint8, True), ("cur", cur, torch.uint8, True), ("out", out, torch.float32, False), ("q8", q8, torch.int32, False),
                                        ("stats", stats, torch.int32, False)))
        H, W, cn = _image_pair(bad, "prev", prev, "cur", cur)
        if out is None:
            out = torch.empty((H, W, 2), device=prev.device, dtype=torch.float32)
        _need(bad, "out", out, (H, W, 2)); _need(bad, "q8", q8, (H, W, 2))
        _need_count(bad, "stats", stats, 4)
        self._call(self.ctx.lib.vido_dis_flow, prev.data_ptr(), cur.data_ptr(), cn, int(rgb_order), W * cn, W, H, int(coarsest), int(iters), int(max_shift_q8), int(min_eig),
                   out.data_ptr(), _p(q8), _p(stats), 1)
        return out

    def flow_consistency(self, fwd_q8, bwd_q8, status=None, out=None, stats=None, alpha_q10=None, beta_q16=None):
        """vido_flow_consistency on device tensors: fwd_q8, bwd_q8 int32 [H,W,2] in 1/256 px (dis_flow's q8 of the pair in either order) -> the marked flow, float32 [H,W,2]
        (`out`, or a new tensor): fwd / 256 where the backward flow at the target brings the pixel back (1024 |f + b|^2 <= alpha_q10 (|f|^2 + |b|^2) + 1024 beta_q16), NaN
        elsewhere.  status: a uint8 [H,W] tensor that receives 0 consistent / 1 inconsistent / 2 leaves the image / 3 not a flow, or None; stats: an int32 tensor of >= 4
        elements that receives the four counts, or None.  The rule is include/vido_c.h's, the numpy statement tests/refimpl/flow_consistency_np.py.  Enqueued on torch's
        current stream, nothing is waited for.  CPU tensors, other dtypes or shapes and non-contiguous tensors raise."""
        from ..host import FLOW_ALPHA_Q10, FLOW_BETA_Q16
        bad = _tensor_args("flow_consistency", (("fwd_q8", fwd_q8, torch.int32, True), ("bwd_q8", bwd_q8, torch.int32, True), ("status", status, torch.uint8, False),
                                                ("out", out, torch.float32, False), ("stats", stats, torch.int32, False)))
        if fwd_q8.dim() != 3 or fwd_q8.shape[2] != 2:
            bad("fwd_q8 must be [H, W, 2], got %s" % (tuple(fwd_q8.shape),))
        H, W = int(fwd_q8.shape[0]), int(fwd_q8.shape[1])
        if out is None:
            out = torch.empty((H, W, 2), device=fwd_q8.device, dtype=torch.float32)
        _need(bad, "bwd_q8", bwd_q8, (H, W, 2)); _need(bad, "out", out, (H, W, 2)); _need(bad, "status", status, (H, W))
        _need_count(bad, "stats", stats, 4)
        self._call(self.ctx.lib.vido_flow_consistency, _p(fwd_q8), _p(bwd_q8), H, W, int(FLOW_ALPHA_Q10 if alpha_q10 is None else alpha_q10),
                   int(FLOW_BETA_Q16 if beta_q16 is None else beta_q16), _p(status), _p(out), _p(stats), 1)
        return out

    def dis_flow_pair(self, prev, cur, out=None, fwd_q8=None, bwd_q8=None, status=None, stats=None, coarsest=4, iters=6, max_shift_q8=1024, min_eig=0, rgb_order=0,
                      alpha_q10=None, beta_q16=None):
        """vido_dis_flow_pair on device tensors: prev, cur as for dis_flow -> the MARKED flow from prev into cur, float32 [H,W,2] (`out`, or a new tensor): dis_flow(prev, cur)
        where flow_consistency of it and dis_flow(cur, prev) gives status 0, NaN elsewhere; both directions come from one pyramid build.  fwd_q8 / bwd_q8: int32 [H,W,2]
        tensors that receive the two fields in 1/256 px, or None; status: uint8 [H,W] or None; stats: int32 of >= 12 elements (the forward call's four counters, the
        backward call's, the check's) or None.  Enqueued on torch's current stream, nothing is waited for; the first call of a size grows the context's scratch, so it comes
        before a graph capture.  The argument checks are dis_flow's."""
        from ..host import FLOW_ALPHA_Q10, FLOW_BETA_Q16
        bad = _tensor_args("dis_flow_pair", (("prev", prev, torch.uint8, True), ("cur", cur, torch.uint8, True), ("out", out, torch.float32, False),
                                             ("fwd_q8", fwd_q8, torch.int32, False), ("bwd_q8", bwd_q8, torch.int32, False), ("status", status, torch.uint8, False),
                                             ("stats", stats, torch.int32, False)))
        H, W, cn = _image_pair(bad, "prev", prev, "cur", cur)
        if out is None:
            out = torch.empty((H, W, 2), device=prev.device, dtype=torch.float32)
        _need(bad, "out", out, (H, W, 2)); _need(bad, "fwd_q8", fwd_q8, (H, W, 2)); _need(bad, "bwd_q8", bwd_q8, (H, W, 2)); _need(bad, "status", status, (H, W))
        _need_count(bad, "stats", stats, 12)
        self._call(self.ctx.lib.vido_dis_flow_pair, _p(prev), _p(cur), cn, int(rgb_order), W * cn, W, H, int(coarsest), int(iters), int(max_shift_q8), int(min_eig),
                   int(FLOW_ALPHA_Q10 if alpha_q10 is None else alpha_q10), int(FLOW_BETA_Q16 if beta_q16 is None else beta_q16), _p(out), _p(fwd_q8), _p(bwd_q8), _p(status), _p(stats), 1)
        return out

    def stereo_sgm(self, left, right, out=None, q4=None, status=None, stats=None, max_disp=128, p1=10, p2=120, uniqueness=10, lr_tol=1, rgb_order=0):
        """vido_stereo_sgm on device tensors: left, right uint8 [H,W] or [H,W,3|4] of one shape (a rectified pair) -> the disparity of left's pixels, float32 [H,W] in pixels
        where the status is 0 and -1 elsewhere (`out`, or a new tensor).  q4: an int32 [H,W] tensor that receives every pixel's disparity in 1/16 px, or None; status: a
        uint8 [H,W] tensor that receives 0 valid / 1 not unique / 2 left-right / 3 zero disparity, or None; stats: an int32 tensor of >= 4 elements that receives the four
        counts, or None.  The rule is include/vido_c.h's, the numpy statement tests/refimpl/stereo_sgm_np.py.  Enqueued on torch's current stream, nothing is waited for;
        the first call of a size grows the op's scratch, so it comes before a graph capture.  The argument checks are dis_flow's: CPU tensors, other dtypes or shapes and
        non-contiguous tensors raise."""
        bad = _tensor_args("stereo_sgm", (("left", left, torch.uint8, True), ("right", right, torch.uint8, True), ("out", out, torch.float32, False), ("q4", q4, torch.int32, False),
                                          ("status", status, torch.uint8, False), ("stats", stats, torch.int32, False)))
        H, W, cn = _image_pair(bad, "left", left, "right", right)
        if out is None:
            out = torch.empty((H, W), device=left.device, dtype=torch.float32)
        _need(bad, "out", out, (H, W)); _need(bad, "q4", q4, (H, W)); _need(bad, "status", status, (H, W))
        _need_count(bad, "stats", stats, 4)
        self._call(self.ctx.lib.vido_stereo_sgm, left.data_ptr(), right.data_ptr(), cn, int(rgb_order), W * cn, W, H, int(max_disp), int(p1), int(p2), int(uniqueness), int(lr_tol),
                   out.data_ptr(), _p(q4), _p(status), _p(stats), 1)
        return out

    def stereo_filter(self, q4, status, out=None, status_out=None, depth=None, stats=None, bf=None, max_diff_q4=None, min_region=None):
        """vido_stereo_filter on device tensors: q4 int32 [H,W] in 1/16 px and status uint8 [H,W] (stereo_sgm's, or of that form) -> the filtered disparity, float32 [H,W]:
        q4 / 16 where the new status is 0 and -1 elsewhere (`out`, or a new tensor).  A valid pixel (status 0, 1 <= q4 <= 65535) whose region — connected through valid
        4-neighbours that differ by at most max_diff_q4 — holds fewer than min_region pixels gets status 4.  status_out: a uint8 [H,W] tensor that receives the new status
        (it may be `status`), or None; depth: a float32 [H,W] tensor that receives bf / disparity where the new status is 0 and FLT_MAX elsewhere (mask_propagate's
        collision depth; needs bf, a float > 0), or None; stats: an int32 tensor of >= 4 elements that receives valid in / regions removed / pixels removed / valid out,
        or None.  The rule is include/vido_c.h's, the numpy statement tests/refimpl/stereo_filter_np.py.  Enqueued on torch's current stream, nothing is waited for; the
        first call of a size grows the op's scratch, so it comes before a graph capture.  CPU tensors, other dtypes or shapes and non-contiguous tensors raise."""
        from ..host import STEREO_FILTER_MAX_DIFF_Q4, STEREO_FILTER_MIN_REGION
        bad = _tensor_args("stereo_filter", (("q4", q4, torch.int32, True), ("status", status, torch.uint8, True), ("out", out, torch.float32, False),
                                             ("status_out", status_out, torch.uint8, False), ("depth", depth, torch.float32, False), ("stats", stats, torch.int32, False)))
        if q4.dim() != 2:
            bad("q4 must be [H, W], got %s" % (tuple(q4.shape),))
        H, W = int(q4.shape[0]), int(q4.shape[1])
        if out is None:
            out = torch.empty((H, W), device=q4.device, dtype=torch.float32)
        _need(bad, "status", status, (H, W)); _need(bad, "out", out, (H, W)); _need(bad, "status_out", status_out, (H, W)); _need(bad, "depth", depth, (H, W))
        _need_count(bad, "stats", stats, 4)
        if depth is not None and bf is None:
            bad("depth needs bf")
        self._call(self.ctx.lib.vido_stereo_filter, q4.data_ptr(), status.data_ptr(), W, H, int(STEREO_FILTER_MAX_DIFF_Q4 if max_diff_q4 is None else max_diff_q4),
                   int(STEREO_FILTER_MIN_REGION if min_region is None else min_region), 0.0 if bf is None else float(bf), out.data_ptr(), _p(status_out), _p(depth), _p(stats), 1)
        return out

    def rectify(self, left, map_left, right=None, map_right=None, out_left=None, out_right=None, inside_left=None, inside_right=None):
        """vido_rectify on device tensors: left uint8 [H,W] or [H,W,3|4] (a raw camera image) and map_left int32 [h,w,2] (host.rectify_map's, uploaded) -> the rectified
        image, uint8 [h,w] or [h,w,3|4] (`out_left`, or a new tensor).  right / map_right: the rig's second camera, of left's shape and map_left's shape, rectified in the
        same launch into `out_right` or a new tensor; the call then returns the pair.  inside_left / inside_right: uint8 [h,w] tensors that receive 1 where the map entry
        lies in the source and 0 elsewhere, or None.  A pixel outside is 0 in every channel.  The rule is include/vido_c.h's, the numpy statement
        tests/refimpl/stereo_rectify_np.py.  One launch enqueued on torch's current stream, no scratch, nothing is waited for: it can be captured from the first call on.
        CPU tensors, other dtypes or shapes, non-contiguous tensors and an output that shares memory with an input raise."""
        two = right is not None
        bad = _tensor_args("rectify", (("left", left, torch.uint8, True), ("map_left", map_left, torch.int32, True), ("right", right, torch.uint8, two),
                                       ("map_right", map_right, torch.int32, two), ("out_left", out_left, torch.uint8, False), ("out_right", out_right, torch.uint8, False),
                                       ("inside_left", inside_left, torch.uint8, False), ("inside_right", inside_right, torch.uint8, False)))
        if not two and (map_right is not None or out_right is not None or inside_right is not None):
            bad("map_right, out_right and inside_right need right")
        H, W, cn = _image_pair(bad, "left", left, "right", right if two else left)
        if map_left.dim() != 3 or map_left.shape[2] != 2:
            bad("map_left must be [h, w, 2], got %s" % (tuple(map_left.shape),))
        h, w = int(map_left.shape[0]), int(map_left.shape[1])
        shape = (h, w) if left.dim() == 2 else (h, w, cn)
        _need(bad, "map_right", map_right, (h, w, 2))
        if out_left is None:
            out_left = torch.empty(shape, device=left.device, dtype=torch.uint8)
        if two and out_right is None:
            out_right = torch.empty(shape, device=left.device, dtype=torch.uint8)
        _need(bad, "out_left", out_left, shape); _need(bad, "out_right", out_right, shape); _need(bad, "inside_left", inside_left, (h, w)); _need(bad, "inside_right", inside_right, (h, w))
        self._call(self.ctx.lib.vido_rectify, left.data_ptr(), _p(right), cn, W * cn, W, H, map_left.data_ptr(), _p(map_right), w, h, out_left.data_ptr(), _p(out_right), w * cn,
                   _p(inside_left), _p(inside_right), 1)
        return (out_left, out_right) if two else out_left

    def mask_associate(self, prev, cur, state, classes=None, n=None, hold=0, out=None, lut=None, stats=None):
        """vido_mask_associate on device tensors: prev int32 [H,W] (the previous handed-over label image warped into this frame, i.e. mask_propagate's output) or None
        (first frame), cur int32 [H,W] (the detector's instance image at id base 0: value 1 + slot), state int32 [768] (read and written; zeros start a sequence),
        classes int64 [>= n] or None (every slot live), n (default: classes' length, 127 without classes), hold >= 0 -> the label image under ids that persist, int32 [H,W]
        (`out`, which may be `cur`, or a new tensor).  An instance takes over the previous id it overlaps with IoU > 1/2, any other gets the next free id of 1..254 behind the
        state's cursor; a previous id nothing matched is held in place for `hold` calls, then retired.  lut: int32 [>= 256] that receives slot + 1 -> id; stats: int32
        [>= 4] that receives (matched, fresh, lost, left out).  Enqueued on torch's current stream, nothing is waited for; the first call of a context allocates, so it
        comes before a graph capture.  CPU tensors, other dtypes or shapes, non-contiguous tensors and out overlapping prev (or cur, other than being cur) raise."""
        bad = _tensor_args("mask_associate", (("cur", cur, torch.int32, True), ("prev", prev, torch.int32, False), ("state", state, torch.int32, True),
                                              ("classes", classes, torch.int64, False), ("out", out, torch.int32, False), ("lut", lut, torch.int32, False),
                                              ("stats", stats, torch.int32, False)))
        if cur.dim() != 2:
            bad("cur must be [H, W]")
        H, W = int(cur.shape[0]), int(cur.shape[1])
        _need(bad, "prev", prev, (H, W))
        if state.numel() != 768:
            bad("state needs 768 elements")
        if n is None:
            n = int(classes.numel()) if classes is not None else 127
        n = int(n)
        _need_count(bad, "classes", classes, n)
        if out is None:
            out = torch.empty((H, W), device=cur.device, dtype=torch.int32)
        _need(bad, "out", out, (H, W))
        if prev is not None and _overlaps(out, prev, 4 * H * W):
            bad("out aliases prev")
        if out.data_ptr() != cur.data_ptr() and _overlaps(out, cur, 4 * H * W):      # (out may be cur)
            bad("out aliases cur")
        _need_count(bad, "lut", lut, 256); _need_count(bad, "stats", stats, 4)
        self._call(self.ctx.lib.vido_mask_associate, _p(prev), _p(cur), H, W, _p(classes), n, int(hold), _p(state), _p(out), _p(lut), _p(stats))
        return out

    def mask_components(self, mask, connectivity=8, min_area=1, id_base=0, cap=127, out=None, classes=None, areas=None, stats=None):
        """vido_mask_components on device tensors: mask int32 [H,W], a class label image (> 0: a class, <= 0: background) -> the instance image, int32 [H,W] (`out`, which
        may be `mask`, or a new tensor).  Every connected component (4 or 8 neighbours) of pixels of EQUAL value with at least min_area pixels gets, in the order of its
        first pixel in raster order, the id id_base + 1 + k; the first `cap` are kept, everything else is 0.  classes: int64 [>= cap] that receives the value of component
        k (0 behind the kept ones), areas: int32 [>= cap] the pixel counts, stats: int32 [>= 4] (found, dropped for area, left out for cap, kept).  With id_base 0 and
        cap 127 the result and `classes` are mask_associate's cur and classes.  Enqueued on torch's current stream, nothing is waited for; the first call of a context
        allocates, so it comes before a graph capture.  CPU tensors, other dtypes or shapes, non-contiguous tensors and out overlapping mask (other than being mask) raise."""
        bad = _tensor_args("mask_components", (("mask", mask, torch.int32, True), ("out", out, torch.int32, False), ("classes", classes, torch.int64, False),
                                               ("areas", areas, torch.int32, False), ("stats", stats, torch.int32, False)))
        if mask.dim() != 2:
            bad("mask must be [H, W]")
        H, W = int(mask.shape[0]), int(mask.shape[1])
        if out is None:
            out = torch.empty((H, W), device=mask.device, dtype=torch.int32)
        _need(bad, "out", out, (H, W))
        if out.data_ptr() != mask.data_ptr() and _overlaps(out, mask, 4 * H * W):      # (out may be mask)
            bad("out aliases mask")
        cap = int(cap)
        _need_count(bad, "classes", classes, cap); _need_count(bad, "areas", areas, cap); _need_count(bad, "stats", stats, 4)
        self._call(self.ctx.lib.vido_mask_components, _p(mask), H, W, int(connectivity), int(min_area), int(id_base), cap, _p(out), _p(classes), _p(areas), _p(stats))
        return out

    def mask_instance_image(self, masks, boxes, labels, H, W, thresh=0.5, padding=1, id_base=None, areas=False):
        """Masker + instance image (vido_mask_instance_image): mask_label_image's inputs in priority order (highest first) -> [H,W] u8 = id_base + 1 + index of the first
        detection with a nonzero label whose pasted mask covers the pixel, 0 elsewhere.  id_base: None (0), an int, or a DEVICE int32 tensor of one element that the kernel
        reads (a captured graph then follows the word's value at replay).  areas=True: also the pixels per detection, int32 [n]."""
        from ..host import VidoError
        out = torch.empty((H, W), device=masks.device, dtype=torch.uint8)
        n = masks.shape[0]
        masks = masks.contiguous().float(); boxes = boxes.contiguous().float(); labels = labels.contiguous().to(torch.int64)
        if id_base is not None and not torch.is_tensor(id_base):
            if id_base < 0 or n + int(id_base) > 255:
                raise VidoError(-4, "mask_instance_image: %d detections above id base %d, ids are u8 (n + id_base <= 255)" % (n, id_base))
            id_base = torch.full((1,), int(id_base), dtype=torch.int32, device=masks.device) if id_base else None
        if id_base is not None:
            assert id_base.is_cuda and id_base.dtype == torch.int32 and id_base.numel() == 1
        area = torch.empty((n,), device=masks.device, dtype=torch.int32) if areas else None
        self._call(self.ctx.lib.vido_mask_instance_image, masks.data_ptr() if n else None, boxes.data_ptr() if n else None, labels.data_ptr() if n else None, n, masks.shape[-1] if n else 28,
                   padding, thresh, H, W, _p(id_base), out.data_ptr(), area.data_ptr() if areas and n else None)
        return (out, area) if areas else out


def _ops_of(obj, out):
    """The HipOps objects `obj` launches through: itself, or those held by a module's sub-modules (attributes such as _ops / wino / fused, and the objects behind bound
    methods such as LiteFlowNet's correlation / epilogue)."""
    if isinstance(obj, HipOps):
        out.setdefault(id(obj), obj)
    elif isinstance(obj, torch.nn.Module):
        for m in obj.modules():
            for v in vars(m).values():
                v = getattr(v, "__self__", v)
                if isinstance(v, HipOps):
                    out.setdefault(id(v), v)
    else:
        raise TypeError("range_safe: a HipOps or an nn.Module, not %s" % type(obj).__name__)
    return out


@contextlib.contextmanager
def range_safe(*targets):
    """Scope in which every split-fp16 entry point of the HipOps objects behind `targets` (HipOps objects or modules) declines, so that their callers take the fp32 routes they
    already have: the 1x1 convolutions (conv1x1_conv, the fused bottleneck's conv1 / conv3 / shortcut, the FPN laterals) the library convolution, the direct 3x3 (wino3x3_conv)
    the fp32 Winograd kernel, the grouped 3x3 of 32 / 64 channels per group (gconv3x3_conv) the fp32 grouped kernel, fc_h_linear F.linear, deconv2x2_conv F.conv_transpose2d.
    The fp32 matrix kernels (gconv, convdirect, convsmall, correlation, Winograd) stay.
    Results then have fp32's range: any finite activation is legal.  Only EAGER calls see the scope (a captured graph replays what it captured).  Nothing process-wide is read or
    changed, and no cached packed weight is replaced or freed (a captured graph reads them): a layer that normally runs on the direct 3x3 gains a Winograd pack on first use."""
    ops = list(_ops_of_all(targets))
    for o in ops:
        o._range_safe += 1
    try:
        yield ops
    finally:
        for o in ops:
            o._range_safe -= 1


def range_checked(run, targets, on_range, what):
    """run(safe) under the per-call range check of the standalone node functions (analyse_flow / analyse_image, on_range="raise" | "recompute"): a latch of every context
    behind `targets` before the call (it takes the trips of earlier launches away from this call's) and one after it, then a wait for the current stream.  A call that tripped
    raises ("raise") or is repeated as run(True) inside range_safe(*targets) ("recompute": fp32's range, no split-fp16 launch)."""
    if on_range not in ("raise", "recompute"):
        raise ValueError("on_range: None, 'raise' or 'recompute', not %r" % (on_range,))
    ops = list(_ops_of_all(targets))
    words = torch.zeros((2, max(len(ops), 1)), dtype=torch.int32).pin_memory()
    for i, o in enumerate(ops):
        o.range_latch(words[0, i:i + 1])
    out = run(False)
    for i, o in enumerate(ops):
        o.range_latch(words[1, i:i + 1])
    torch.cuda.current_stream().synchronize()
    if not bool(words[1].any()):
        return out
    if on_range == "raise":
        raise RuntimeError("split-fp16: an activation of %s left the range of the arithmetic (|x| >= 65504, an infinity or a NaN); its outputs are not valid — "
                           "on_range=\"recompute\" repeats the call in fp32's range" % what)
    with range_safe(*targets):
        return run(True)


def _ops_of_all(targets):
    out = {}
    for t in targets:
        _ops_of(t, out)
    return out.values()


_C1X1_MIN_TILES = int(os.environ.get("VIDO_CONV1X1_MIN_TILES", "100"))      # (160 through round 5: the fp32-instruction kernel lost to the library at layer4's 112 tiles; the split-bf16 one wins there)


def conv1x1_fills_chip(cout, hw):
    """csrc/conv1x1.hip works on 128 x 128 tiles, one per CU, each walking ALL input channels: a layer with few tiles (layer4's 2048 -> 2048 on 25 x 34: 112; the FPN laterals of
    P4 / P5: 54 / 14) leaves most of the 256 CUs idle for as long as a chip-filling layer takes — measured 119 us against the library's 68 at 112 tiles with the fp32 matrix
    instruction, 64 us with the split-bf16 form (round 6; headline 100.8 -> 103.9 frames/s with layer4 on it, profiles/r6/headline_ab.txt).  Callers keep the library below
    VIDO_CONV1X1_MIN_TILES (default 100)."""
    return (int(cout) // 128) * ((int(hw) + 127) // 128) >= _C1X1_MIN_TILES


def split_bf16x3(x):
    """fp32 tensor -> three bf16 tensors with x0 + x1 + x2 == x EXACTLY (x0 = rne(x), x1 = rne(x - x0), x2 = x - x0 - x1: three 8-bit significands + signs cover the 24 bits
    of fp32; exponents far above the bf16 subnormal range assumed) — the operand form of csrc/conv1x1.hip::k_conv1x1_b3 and of the Winograd kernel's split-bf16 form."""
    x = x.float()
    x0 = x.to(torch.bfloat16); r1 = x - x0.float()
    x1 = r1.to(torch.bfloat16); r2 = r1 - x1.float()
    x2 = r2.to(torch.bfloat16)
    return x0, x1, x2


def split_f16x2(w):
    """fp32 matrix [rows, k] -> (h, l, inv): fp16 planes of the rows scaled by powers of two, w == inv[:, None] * (h + l / 2048) to within 2^-22 |w| (two roundings to 11 bits; 2^-24.5 rms) (h = rne16(s w),
    l = rne16(2048 (s w - h)); s = 1 / inv puts the row's largest |w| into [2^14, 2^15): no overflow; full precision down to 2^-26 of the row's maximum, below that an absolute error under 2^-48 of it) — the weight
    side of csrc/conv1x1.hip::k_conv1x1_b3<.., NP = 2>."""
    w = w.float()
    m = w.abs().amax(1)
    _, ex = torch.frexp(torch.where(m > 0, m, torch.ones_like(m)))          # m = mant 2^ex, mant in [0.5, 1)
    e = torch.where(m > 0, 15 - ex, torch.zeros_like(ex)).clamp(-100, 100).to(torch.int32)
    pow2 = lambda k: ((k + 127) << 23).view(torch.float32)                  # 2^k from its bit pattern: exact on every device (ldexp goes through pow on some)
    ws = w * pow2(e)[:, None]
    h = ws.to(torch.float16)
    l = ((ws - h.float()) * 2048.0).to(torch.float16)
    return h, l, pow2(-e)


def pack_conv1x1(w, layout=0):
    """1x1 convolution weight [cout, cin, 1, 1] (or [cout, cin]) -> the operand order of csrc/conv1x1.hip (layout = HipOps.conv1x1_layout(cin, cout, H * W) = vido_conv1x1_layout
    for the current arithmetic setting, or any of the three by choice: a launch runs the layout it is handed):
    0: element (co, k) at [co / 32][k / 8][32 * (k & 1) + co % 32][(k % 8) / 2] (a lane's four operands of a group of four k-pairs are one 16-byte read; a (32-channel block, group)
       is one 1 KB copy piece) — the fp32 matrix instruction (32 x 32 x 2);
    2: the weight split into three bf16 planes (split_bf16x3), plane p of element (co, k) at [co / 32][k / 16][p][32 * ((k % 16) / 8) + co % 32][k % 8] (int16 tensor: a 1 KB copy
       piece = the A operand of v_mfma_f32_32x32x16_bf16 for one (32-channel block, 16 input channels, plane)) — the split-bf16 form k_conv1x1_b3.
    3: the weight as two fp16 planes of its rows scaled by powers of two (split_f16x2), in the order of 2 with two planes, followed by the [cout] inverse row scales
       (flat int16 tensor of 2 cout (cin + 1) elements) — the split-fp16 form, the default.
    None when the kernel does not take the shape; ValueError for any other layout."""
    if layout not in (0, 2, 3):
        raise ValueError("pack_conv1x1: no layout %r (0 = fp32 instruction, 2 = split-bf16, 3 = split-fp16)" % (layout,))
    cout, cin = int(w.shape[0]), int(w.shape[1])
    if w.dim() == 4 and tuple(w.shape[2:]) != (1, 1):
        return None
    if cout % 128 or cin % 32:
        return None
    if layout == 3:
        h, l, inv = split_f16x2(w.detach().reshape(cout, cin))
        w6 = torch.stack([h, l], 0).view(torch.int16).reshape(2, cout // 32, 32, cin // 16, 2, 8)              # [plane][mb][co32][step][k half][8]
        planes = w6.permute(1, 3, 0, 4, 2, 5).contiguous().reshape(-1)
        return torch.cat([planes, inv.contiguous().view(torch.int16).reshape(-1)])
    if layout == 2:
        p0, p1, p2 = split_bf16x3(w.detach().reshape(cout, cin).float())
        w6 = torch.stack([p0, p1, p2], 0).view(torch.int16).reshape(3, cout // 32, 32, cin // 16, 2, 8)      # [plane][mb][co32][step][k half][8]
        return w6.permute(1, 3, 0, 4, 2, 5).contiguous().reshape(cout // 32, cin // 16, 3, 64, 8)
    w5 = w.detach().reshape(cout // 32, 32, cin // 8, 4, 2)            # [mb][co32][group][kk][half]
    return w5.permute(0, 2, 4, 1, 3).contiguous().reshape(cout // 32, cin // 8, 64, 4)


def packed_conv1x1_layout(wp, cin):
    """(layout, cout) of a tensor made by pack_conv1x1 for `cin` input channels, read off its dtype and shape: float32 (cout / 32, cin / 8, 64, 4) is layout 0, int16
    (cout / 32, cin / 16, 3, 64, 8) layout 2, flat int16 of 2 cout (cin + 1) elements layout 3.  ValueError when it is none of them: a pack for another cin, or no pack."""
    cin = int(cin); sh = tuple(int(v) for v in wp.shape)
    if wp.dtype == torch.float32 and len(sh) == 4 and sh[1:] == (cin // 8, 64, 4) and cin % 8 == 0:
        return 0, 32 * sh[0]
    if wp.dtype == torch.int16 and len(sh) == 5 and sh[1:] == (cin // 16, 3, 64, 8) and cin % 16 == 0:
        return 2, 32 * sh[0]
    if wp.dtype == torch.int16 and len(sh) == 1 and sh[0] > 0 and sh[0] % (2 * (cin + 1)) == 0:
        return 3, sh[0] // (2 * (cin + 1))
    raise ValueError("conv1x1: a %s tensor of shape %s is no pack_conv1x1 weight for %d input channels" % (wp.dtype, sh, cin))


def pack_conv3x3_h(w):
    """3x3 convolution weight [cout, cin, 3, 3] -> the operand order of csrc/conv3x3h.hip (the direct split-fp16 kernel): two fp16 planes of the output channels scaled by
    powers of two (split_f16x2 over a channel's cin x 9 weights), plane p of element (co, ci, dy, dx) at [co / 32][ci / 16][dy][dx][p][32 * ((ci % 16) / 8) + co % 32][ci % 8],
    followed by the [cout] inverse scales (flat int16 tensor); input channels are padded to a multiple of 16 with zero weights.  None when the kernel does not take the shape."""
    cout, cin0 = int(w.shape[0]), int(w.shape[1])
    if tuple(w.shape[2:]) != (3, 3) or not (cout in (32, 64) or (cout >= 128 and cout % 128 == 0)):
        return None
    cin = (cin0 + 15) // 16 * 16                                              # input channels padded with zero weights
    if cin != cin0:
        w = torch.cat([w.detach(), torch.zeros(cout, cin - cin0, 3, 3, dtype=w.dtype, device=w.device)], 1)
    h, l, inv = split_f16x2(w.detach().reshape(cout, cin * 9))
    planes = torch.stack([h, l], 0).view(torch.int16).reshape(2, cout // 32, 32, cin // 16, 2, 8, 3, 3)        # [plane][mb][co32][chunk][k half][k8][dy][dx]
    planes = planes.permute(1, 3, 6, 7, 0, 4, 2, 5).contiguous().reshape(-1)                                 # [mb][chunk][dy][dx][plane][k half][co32][k8]
    return torch.cat([planes, inv.contiguous().view(torch.int16).reshape(-1)])


def pack_deconv2x2(w):
    """nn.ConvTranspose2d weight [cin, cout, 2, 2] -> the split-fp16 packing of the GEMM matrix [(2 a + b) cout + co][ci] = w[ci][co][a][b] (pack_conv1x1 layout 3): the operand of
    vido_deconv2x2_bias_act."""
    cin, cout = int(w.shape[0]), int(w.shape[1])
    wm = w.detach().permute(2, 3, 1, 0).reshape(4 * cout, cin, 1, 1)
    return pack_conv1x1(wm, 3)


class PackedConv1x1:
    """A 1x1 convolution weight whose operand order depends on the arithmetic setting at its first use (pack_conv1x1 layouts 0 / 2 / 3): packed lazily per (layout, device),
    outside any graph capture (the warm-up calls of fuse.Graphed come first).  None-like when no layout takes the shape: use PackedConv1x1.make."""

    def __init__(self, w):
        self.w = w.detach(); self.cout = int(w.shape[0]); self.cin = int(w.shape[1]); self._p = {}

    @staticmethod
    def make(w):
        return PackedConv1x1(w) if pack_conv1x1(w, 0) is not None else None

    def get(self, layout, device):
        key = (int(layout), str(device))
        if key not in self._p:
            p = pack_conv1x1(self.w, layout)
            assert p is not None, "conv1x1: layout %d does not take %d -> %d channels" % (layout, self.cin, self.cout)
            self._p[key] = p.to(device)
        return self._p[key]


def pack_conv1x1_skinny(w):
    """1x1 convolution weight [cout, cin, 1, 1] (cin even) -> the operand order of csrc/convsmall.hip::k_conv1x1_skinny: element (co, k) at [co / 32][k / 2][32 * (k & 1) + co % 32],
    output channels padded to a multiple of 32 with zeros."""
    cout, cin = int(w.shape[0]), int(w.shape[1])
    cop = (cout + 31) // 32 * 32
    wz = w.detach().reshape(cout, cin).new_zeros((cop, cin)); wz[:cout] = w.detach().reshape(cout, cin)
    return wz.reshape(cop // 32, 32, cin // 2, 2).permute(0, 2, 3, 1).contiguous().reshape(cop // 32, cin // 2, 64)


def pack_stem7x7(w):
    """Stem weight [64, 3, 7, 7] -> the operand order of csrc/stem.hip::k_stem7x7s2_pool, [2][84][64]: K runs over (plane c, column dx, row pair j) and the two k of a pair are
    the rows dy = 2 j and 2 j + 1 (dy = 7: zeros); element (co, c, dy, dx) at [co / 32][(c * 7 + dx) * 4 + dy / 2][32 * (dy & 1) + co % 32]."""
    assert tuple(w.shape) == (64, 3, 7, 7)
    wz = w.detach().new_zeros((64, 3, 8, 7)); wz[:, :, :7] = w.detach()
    # [cb][co][c][j][par][dx] -> [cb][c][dx][j][par][co]
    return wz.reshape(2, 32, 3, 4, 2, 7).permute(0, 2, 5, 3, 4, 1).contiguous().reshape(2, 84, 64)


def pack_gconv3x3(w, groups):
    """Convolution weight [groups * cpg_out, cpg_in, 3, 3] -> the operand order of csrc/gconv.hip: per (group, 32-channel output block, 8-channel input chunk) [tap][ci][co];
    with 16 or 8 output channels per group: [group][chunk][tap][ci][16 co] (missing output channels zero).  None when the kernels do not take the shape."""
    cout, cpg_in = int(w.shape[0]), int(w.shape[1])
    cpg_out = cout // groups
    if tuple(w.shape[2:]) != (3, 3) or cpg_in % 8 or not (cpg_out % 32 == 0 or cpg_out in (8, 16)):
        return None
    w9 = w.detach().reshape(groups, cpg_out, cpg_in // 8, 8, 9)
    if cpg_out % 32 == 0:
        return w9.reshape(groups, cpg_out // 32, 32, cpg_in // 8, 8, 9).permute(0, 1, 3, 5, 4, 2).contiguous()
    pad = w9.new_zeros((groups, 16, cpg_in // 8, 8, 9)); pad[:, :cpg_out] = w9
    return pad.permute(0, 2, 4, 3, 1).contiguous()


def pack_gconv3x3_h(w, groups):
    """Grouped convolution weight [groups * cpg, cpg, 3, 3] (cpg = 32 or 64 channels per group, in and out) -> the operand order of csrc/gconvh.hip: two fp16 planes of the output
    channels scaled by powers of two (split_f16x2 over a channel's cpg x 9 weights), plane p of element (co, ci, dy, dx) of group g at
    [g][(co % cpg) / 32][ci / 16][3 dy + dx][p][32 * ((ci % 16) / 8) + co % 32][ci % 8], followed by the [groups * cpg] inverse scales (flat int16 tensor).  None when the kernel
    does not take the shape."""
    cout, cpg = int(w.shape[0]), int(w.shape[1])
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or groups < 1 or cout != groups * cpg or cpg not in (32, 64):
        return None
    h, l, inv = split_f16x2(w.detach().reshape(cout, cpg * 9))
    planes = torch.stack([h, l], 0).view(torch.int16).reshape(2, groups, cpg // 32, 32, cpg // 16, 2, 8, 9)      # [plane][g][cob][co32][step][k half][k8][tap]
    planes = planes.permute(1, 2, 4, 7, 0, 5, 3, 6).contiguous().reshape(-1)                                   # [g][cob][step][tap][plane][k half][co32][k8]
    return torch.cat([planes, inv.contiguous().view(torch.int16).reshape(-1)])


def pack_gconv3x3_hs(w, groups):
    """Grouped convolution weight [groups * cpg, cpg, 3, 3] (cpg = 8 or 16 channels per group, in and out) -> the operand order of csrc/gconvhs.hip: two fp16 planes of the output
    channels scaled by powers of two (split_f16x2 over a channel's cpg x 9 weights) as A operands of v_mfma_f32_16x16x32_f16, plane p of element (co, ci, dy, dx) of group g at
    [g][i][p][16 * b + co % cpg][ci % 8]: block b (of 8 k) of instruction i is the slot of tap 3 dy + dx = 4 i + b at 8 per group (3 instructions; rows 8 .. 15 of every block are
    zero) and of (tap 2 i + b // 2, input channels 8 (b % 2) .. + 7) at 16 per group (5 instructions); the slots of taps 9 .. 11 / tap 9 are zero.  Followed by the
    [groups * cpg] inverse scales (flat int16 tensor of groups * (3 | 5) * 1024 + 2 * groups * cpg elements).  None when the kernel does not take the shape."""
    if w.dim() != 4:
        return None
    cout, cpg = int(w.shape[0]), int(w.shape[1])
    if tuple(w.shape[2:]) != (3, 3) or groups < 1 or cout != groups * cpg or cpg not in (8, 16):
        return None
    h, l, inv = split_f16x2(w.detach().reshape(cout, cpg * 9))
    planes = torch.stack([h, l], 0).view(torch.int16).reshape(2, groups, cpg, cpg // 8, 8, 9)                  # [plane][g][co][channel group][k8][tap]
    ni = 3 if cpg == 8 else 5
    out = torch.zeros((groups, ni, 2, 4, 16, 8), dtype=torch.int16, device=planes.device)                       # [g][i][plane][b][row][k8]
    for i in range(ni):
        for b in range(4):
            tap, cg = (4 * i + b, 0) if cpg == 8 else (2 * i + (b >> 1), b & 1)
            if tap < 9:
                out[:, i, :, b, :cpg, :] = planes[:, :, :, cg, :, tap].permute(1, 0, 2, 3)
    return torch.cat([out.reshape(-1), inv.contiguous().view(torch.int16).reshape(-1)])


def pack_conv_direct(w):
    """convolution weight [cout, cin, kh, kw] -> the operand order of csrc/convdirect.hip (the library's vido_conv_direct_pack), a flat CPU tensor"""
    import numpy as np
    from ..host import load_library
    lib = load_library()
    cout, cin, kh, kw = (int(v) for v in w.shape)
    wh = np.ascontiguousarray(w.detach().to("cpu", torch.float32).numpy())
    n = int(lib.vido_conv_direct_packed_floats(cin, cout, kh, kw))
    if n <= 0:
        raise RuntimeError("vido_conv_direct_pack: no kernel for %d x %d taps" % (kh, kw))
    out = np.empty(n, np.float32)
    rc = lib.vido_conv_direct_pack(wh.ctypes.data, cin, cout, kh, kw, out.ctypes.data)
    if rc != 0:
        raise RuntimeError("vido_conv_direct_pack: %d" % rc)
    return torch.from_numpy(out)


def pack_wino3x3(w, form=0):
    """3x3 convolution weight [cout, cin, 3, 3] -> U = G g G^T (float64, rounded once) in the operand order of csrc/wino.hip, as a CPU tensor
    [cout_pad / 32, cin_pad / KC, 16, 64, KC / 2] (the library's vido_wino3x3_pack_form: ONE implementation of the layout, also what a C caller uses).
    form 0: KC by cout (8, or 4 for 32 / 96 .. channels), form 1 (K-split launches): KC = 4."""
    import numpy as np
    from ..host import load_library
    lib = load_library()
    cout, cin =int(w.shape[0]), int(w.shape[1])
    assert tuple(w.shape[2:]) == (3, 3) and form in (0, 1, 2)
    wh = np.ascontiguousarray(w.detach().to("cpu", torch.float32).numpy())
    n = int(lib.vido_wino3x3_packed_floats_form(cin, cout, int(form)))
    out = np.empty(n, np.float32)
    rc = lib.vido_wino3x3_pack_form(wh.ctypes.data, cin, cout, int(form), out.ctypes.data)
    if rc != 0:
        raise RuntimeError("vido_wino3x3_pack_form: %d" % rc)
    kc = 8 if (((cout + 63) // 64) * 64 - cout) < 32 and form == 0 else 4
    cop = ((cout + 63) // 64) * 64 if kc == 8 else ((cout + 31) // 32) * 32
    cip = ((cin + kc - 1) // kc) * kc
    return torch.from_numpy(out).reshape(cop // 32, cip // kc, 16, 64, kc // 2)
