"""Python handle on a native UNet context (libunet_hip.so).

One ``UNetRuntime`` per (device, network configuration).  It exposes the native
parameter / BN-buffer tables (so the ``nn.Module`` can lay its tensors out in the flat
arenas the kernels read) and thin, shape-checked wrappers of the C entry points that
take torch tensors and enqueue on torch's current stream.
"""
import collections
import ctypes

import torch

from . import _lib

_RUNTIMES = {}


class UNetRuntime:
    def __init__(self, device, in_channels=1, out_channels=1, variant=_lib.VARIANT_MODEL,
                 base_filters=0, depth=0, math=_lib.MATH_F32):
        lib = _lib.load()
        self.lib = lib
        self.device = torch.device(device)
        cfg = _lib.UnetCfg(in_channels, out_channels, variant, base_filters, depth, math)
        h = ctypes.c_void_p()
        _lib.check(lib.unet_create(ctypes.byref(cfg), self.device.index or 0, ctypes.byref(h)),
                   None, "unet_create")
        self.ctx = h
        n, nf = ctypes.c_int(), ctypes.c_int64()
        lib.unet_num_params(h, ctypes.byref(n), ctypes.byref(nf))
        self.n_param_floats = nf.value
        self.params = []  # (name, shape, offset)
        for i in range(n.value):
            name, nd, off = ctypes.c_char_p(), ctypes.c_int(), ctypes.c_int64()
            shape = (ctypes.c_int64 * 4)()
            lib.unet_param_info(h, i, ctypes.byref(name), ctypes.byref(nd), shape, ctypes.byref(off))
            self.params.append((name.value.decode(), tuple(shape[k] for k in range(nd.value)),
                                off.value))
        lib.unet_num_bn(h, ctypes.byref(n), ctypes.byref(nf))
        self.n_bn_floats = nf.value
        self.bn = []  # (name, channels, offset)
        for i in range(n.value):
            name, ch, off = ctypes.c_char_p(), ctypes.c_int(), ctypes.c_int64()
            lib.unet_bn_info(h, i, ctypes.byref(name), ctypes.byref(ch), ctypes.byref(off))
            self.bn.append((name.value.decode(), ch.value, off.value))
        nb = ctypes.c_int()
        lib.unet_num_buckets(h, ctypes.byref(nb))
        self.buckets = []
        for b in range(nb.value):
            o, l = ctypes.c_int64(), ctypes.c_int64()
            lib.unet_bucket_range(h, b, ctypes.byref(o), ctypes.byref(l))
            self.buckets.append((o.value, l.value))
        # the context's schedule options as created (reset_options restores them)
        self._default_options = {k: self.get_option(k) for k in _lib.option_names()}

    def __del__(self):
        try:
            if getattr(self, "ctx", None):
                self.lib.unet_destroy(self.ctx)
        except Exception:
            pass

    @staticmethod
    def get(device, in_channels=1, out_channels=1, variant=_lib.VARIANT_MODEL, base_filters=0,
            depth=0, math=_lib.MATH_F32):
        key = (str(torch.device(device)), in_channels, out_channels, variant, base_filters, depth,
               math)
        rt = _RUNTIMES.get(key)
        if rt is None:
            rt = UNetRuntime(device, in_channels, out_channels, variant, base_filters, depth, math)
            _RUNTIMES[key] = rt
        return rt

    # ------------------------------------------------------------------ entry points
    def workspace_bytes(self, N, H, W, training):
        b = ctypes.c_size_t()
        _lib.check(self.lib.unet_workspace_size(self.ctx, N, H, W, int(training), ctypes.byref(b)),
                   self.ctx, "unet_workspace_size")
        return b.value

    def forward(self, params, bn_running, bn_count, x, training, workspace=None):
        N, _, H, W = x.shape
        nb = self.workspace_bytes(N, H, W, training)
        if workspace is None or workspace.numel() < nb:
            workspace = torch.empty(nb, dtype=torch.uint8, device=x.device)
        logits = torch.empty((N, self.out_channels(), H, W), dtype=torch.float32, device=x.device)
        rc = self.lib.unet_forward(self.ctx, _lib.ptr(params), _lib.ptr(bn_running), _lib.ptr(bn_count),
                                   _lib.ptr(x), _lib.ptr(logits), _lib.ptr(workspace),
                                   workspace.numel(), N, H, W, int(training), _lib.stream_ptr(x.device))
        _lib.check(rc, self.ctx, "unet_forward")
        return logits, workspace

    def backward(self, params, dlogits, grads, workspace):
        N, _, H, W = dlogits.shape
        rc = self.lib.unet_backward(self.ctx, _lib.ptr(params), _lib.ptr(dlogits), _lib.ptr(grads),
                                    _lib.ptr(workspace), workspace.numel(), N, H, W,
                                    _lib.stream_ptr(dlogits.device))
        _lib.check(rc, self.ctx, "unet_backward")

    def out_channels(self):
        return self.params[-1][1][0]

    def loss_stats(self, logits, targets):
        """Per-sample partials fp32[4N] and the batch sums fp64[8] (unet_loss_stats)."""
        N, C, H, W = logits.shape
        stats = torch.empty(4 * N, dtype=torch.float32, device=logits.device)
        sums = torch.empty(8, dtype=torch.float64, device=logits.device)
        rc = self.lib.unet_loss_stats(self.ctx, _lib.ptr(logits), _lib.ptr(targets), N, C, H, W,
                                      _lib.ptr(stats), _lib.ptr(sums), _lib.stream_ptr(logits.device))
        _lib.check(rc, self.ctx, "unet_loss_stats")
        return stats, sums

    def loss_finalize(self, sums, alpha=0.4, beta=0.6, gamma=2.0):
        losses = torch.empty(3, dtype=torch.float32, device=sums.device)
        rc = self.lib.unet_loss_finalize(self.ctx, _lib.ptr(sums), _lib.ptr(losses), alpha, beta,
                                         gamma, _lib.stream_ptr(sums.device))
        _lib.check(rc, self.ctx, "unet_loss_finalize")
        return losses

    def loss_fwd(self, logits, targets, alpha=0.4, beta=0.6, gamma=2.0):
        stats, sums = self.loss_stats(logits, targets)
        return self.loss_finalize(sums, alpha, beta, gamma), stats, sums

    def loss_bwd(self, logits, targets, stats, sums, w, alpha=0.4, beta=0.6, gamma=2.0):
        N, C, H, W = logits.shape
        d = torch.empty_like(logits)
        rc = self.lib.unet_loss_bwd(self.ctx, _lib.ptr(logits), _lib.ptr(targets), N, C, H, W,
                                    _lib.ptr(stats), _lib.ptr(sums), _lib.ptr(w), _lib.ptr(d), alpha,
                                    beta, gamma, _lib.stream_ptr(logits.device))
        _lib.check(rc, self.ctx, "unet_loss_bwd")
        return d

    def edt(self, targets):
        """dist (N, 1, H, W): exact Euclidean distance transform of targets[:, 0] (unet_edt)."""
        N, C, H, W = targets.shape
        dist = torch.empty((N, 1, H, W), dtype=torch.float32, device=targets.device)
        rc = self.lib.unet_edt(self.ctx, _lib.ptr(targets), N, C, H, W, _lib.ptr(dist),
                               _lib.stream_ptr(targets.device))
        _lib.check(rc, self.ctx, "unet_edt")
        return dist

    def boundary_fwd(self, logits, targets, dist):
        """BoundaryLoss value (0-dim fp32) of logits / targets / dist (unet_boundary_fwd)."""
        N, C, H, W = logits.shape
        s = torch.empty(1, dtype=torch.float64, device=logits.device)
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        rc = self.lib.unet_boundary_fwd(self.ctx, _lib.ptr(logits), _lib.ptr(targets), _lib.ptr(dist),
                                        N, C, H, W, _lib.ptr(s), _lib.ptr(loss),
                                        _lib.stream_ptr(logits.device))
        _lib.check(rc, self.ctx, "unet_boundary_fwd")
        return loss

    def boundary_bwd(self, logits, targets, dist, w):
        N, C, H, W = logits.shape
        d = torch.empty_like(logits)
        rc = self.lib.unet_boundary_bwd(self.ctx, _lib.ptr(logits), _lib.ptr(targets), _lib.ptr(dist),
                                        N, C, H, W, _lib.ptr(w), _lib.ptr(d),
                                        _lib.stream_ptr(logits.device))
        _lib.check(rc, self.ctx, "unet_boundary_bwd")
        return d

    def lovasz_fwd(self, logits, targets, want_perm=False):
        """Lovasz hinge loss (0-dim fp32), gmap (N, C, H, W) fp32, the batch sum fp64[1] and, when
        wanted, perm int32 (N, C, H W) of logits / targets (unet_lovasz_fwd)."""
        N, C, H, W = logits.shape
        gmap = torch.empty_like(logits)
        perm = torch.empty((N, C, H * W), dtype=torch.int32, device=logits.device) if want_perm else None
        s = torch.empty(1, dtype=torch.float64, device=logits.device)
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        rc = self.lib.unet_lovasz_fwd(self.ctx, _lib.ptr(logits), _lib.ptr(targets), N, C, H, W,
                                      _lib.ptr(gmap), _lib.ptr(perm), _lib.ptr(s), _lib.ptr(loss),
                                      _lib.stream_ptr(logits.device))
        _lib.check(rc, self.ctx, "unet_lovasz_fwd")
        return loss, gmap, s, perm

    def lovasz_bwd(self, logits, targets, gmap, w):
        N, C, H, W = logits.shape
        d = torch.empty_like(logits)
        rc = self.lib.unet_lovasz_bwd(self.ctx, _lib.ptr(logits), _lib.ptr(targets), _lib.ptr(gmap),
                                      N, C, H, W, _lib.ptr(w), _lib.ptr(d), _lib.stream_ptr(logits.device))
        _lib.check(rc, self.ctx, "unet_lovasz_bwd")
        return d

    def adamw(self, params, grads, m, v, step, lr, beta1, beta2, eps, wd, grad_scale=1.0):
        rc = self.lib.unet_adamw(self.ctx, _lib.ptr(params), _lib.ptr(grads), _lib.ptr(m), _lib.ptr(v),
                                 params.numel(), step, float(lr), float(beta1), float(beta2),
                                 float(eps), float(wd), float(grad_scale),
                                 _lib.stream_ptr(params.device))
        _lib.check(rc, self.ctx, "unet_adamw")

    def adamw_repack(self, params, grads, m, v, step, lr, beta1, beta2, eps, wd, grad_scale=1.0):
        """AdamW over this context's whole parameter arena fused with the next forward's weight
        repack (unet_adamw_repack; bit-identical to adamw)."""
        rc = self.lib.unet_adamw_repack(self.ctx, _lib.ptr(params), _lib.ptr(grads), _lib.ptr(m),
                                        _lib.ptr(v), params.numel(), step, float(lr), float(beta1),
                                        float(beta2), float(eps), float(wd), float(grad_scale),
                                        _lib.stream_ptr(params.device))
        _lib.check(rc, self.ctx, "unet_adamw_repack")

    def params_changed(self):
        """Some parameter arena changed outside adamw_repack: the next forward repacks,
        whichever model's images this (shared) context holds."""
        _lib.check(self.lib.unet_params_changed(self.ctx), self.ctx, "unet_params_changed")

    def arena_changed(self, arena):
        """`arena` (a parameter arena or any part of one) was written outside adamw_repack:
        the context drops its weight images only if they are that arena's
        (unet_arena_changed), so other models of this configuration keep theirs."""
        _lib.check(self.lib.unet_arena_changed(self.ctx, _lib.ptr(arena), arena.numel()), self.ctx,
                   "unet_arena_changed")

    # ------------------------------------------------------------------ schedule options
    def set_option(self, name, value):
        """Kernel-schedule option (include/unet_hip.h unet_set_option); A/B runs and tests."""
        _lib.check(self.lib.unet_set_option(self.ctx, name.encode(), int(value)), self.ctx,
                   f"unet_set_option({name})")

    def reset_options(self):
        """Every schedule option back to its value at creation (this runtime is shared by
        every model of its configuration on the device)."""
        for k, v in self._default_options.items():
            if self.get_option(k) != v:
                self.set_option(k, v)

    def get_option(self, name):
        v = ctypes.c_int64()
        _lib.check(self.lib.unet_get_option(self.ctx, name.encode(), ctypes.byref(v)), self.ctx,
                   f"unet_get_option({name})")
        return v.value

    def mask_counts(self, logits, targets, counts, mask=None):
        rc = self.lib.unet_mask_counts(self.ctx, _lib.ptr(logits), _lib.ptr(targets), logits.numel(),
                                       _lib.ptr(mask), _lib.ptr(counts), _lib.stream_ptr(logits.device))
        _lib.check(rc, self.ctx, "unet_mask_counts")

    def surface_stats(self, logits, targets):
        """Per-sample surface-distance statistics (unet_surface_stats): int64 (N, 6)
        {defined, n_PG, n_GP, max_d2, d2_lo, d2_hi} and float64 (N, 2) {sum_PG, sum_GP}."""
        N, C, H, W = logits.shape
        oi = torch.empty((N, 6), dtype=torch.int64, device=logits.device)
        of = torch.empty((N, 2), dtype=torch.float64, device=logits.device)
        rc = self.lib.unet_surface_stats(self.ctx, _lib.ptr(logits), _lib.ptr(targets), N, C, H, W,
                                         _lib.ptr(oi), _lib.ptr(of), _lib.stream_ptr(logits.device))
        _lib.check(rc, self.ctx, "unet_surface_stats")
        return oi, of

    def components(self, x, kind, connectivity=1):
        """labels int32 (N, H, W) and count int32 (N,) of x (N, C, H, W), channel 0
        (unet_components; kind 0 uint8 mask, 1 logits, 2 targets)."""
        N, C, H, W = x.shape
        labels = torch.empty((N, H, W), dtype=torch.int32, device=x.device)
        count = torch.empty(N, dtype=torch.int32, device=x.device)
        rc = self.lib.unet_components(self.ctx, _lib.ptr(x), kind, N, C, H, W, connectivity,
                                      _lib.ptr(labels), _lib.ptr(count), _lib.stream_ptr(x.device))
        _lib.check(rc, self.ctx, "unet_components")
        return labels, count

    def postprocess(self, x, kind, connectivity=1, keep_largest=False, min_area=0, fill_holes=False):
        """mask uint8 (N, H, W) and info int64 (N, 4) {components before, components kept,
        foreground pixels after, pixels filled} (unet_postprocess)."""
        N, C, H, W = x.shape
        out = torch.empty((N, H, W), dtype=torch.uint8, device=x.device)
        info = torch.empty((N, 4), dtype=torch.int64, device=x.device)
        rc = self.lib.unet_postprocess(self.ctx, _lib.ptr(x), kind, N, C, H, W, connectivity,
                                       int(bool(keep_largest)), int(min_area), int(bool(fill_holes)),
                                       _lib.ptr(out), _lib.ptr(info), _lib.stream_ptr(x.device))
        _lib.check(rc, self.ctx, "unet_postprocess")
        return out, info

    def lesion_stats(self, pred, kind, targets, connectivity=1):
        """int64 (N, 4) {n_pred, n_gt, gt_hit, pred_hit} (unet_lesion_stats); pred and targets
        are both (N, C, H, W)."""
        N, C, H, W = pred.shape
        out = torch.empty((N, 4), dtype=torch.int64, device=pred.device)
        rc = self.lib.unet_lesion_stats(self.ctx, _lib.ptr(pred), kind, _lib.ptr(targets), N, C, H, W,
                                        connectivity, _lib.ptr(out), _lib.stream_ptr(pred.device))
        _lib.check(rc, self.ctx, "unet_lesion_stats")
        return out

    def morphometry(self, labels, count, max_rows):
        """table int64 (N, max_rows, 16) of labels int32 (N, H, W) and count int32 (N,)
        (unet_morphometry; the fields in csrc/morph.h)."""
        N, H, W = labels.shape
        table = torch.empty((N, max_rows, 16), dtype=torch.int64, device=labels.device)
        rc = self.lib.unet_morphometry(self.ctx, _lib.ptr(labels), _lib.ptr(count), N, H, W, max_rows,
                                       _lib.ptr(table), _lib.stream_ptr(labels.device))
        _lib.check(rc, self.ctx, "unet_morphometry")
        return table

    def lesion_echo(self, gray, labels, count, max_rows, levels, ring):
        """table int32 (N, max_rows, 512 + levels^2) of gray uint8 (N, H, W), labels int32 (N, H, W) and
        count int32 (N,) (unet_lesion_echo; the columns in csrc/echo.h).  The call clears the table."""
        N, H, W = labels.shape
        table = torch.empty((N, max_rows, 512 + levels * levels), dtype=torch.int32, device=labels.device)
        rc = self.lib.unet_lesion_echo(self.ctx, _lib.ptr(gray), _lib.ptr(labels), _lib.ptr(count), N, H, W,
                                       max_rows, levels, ring, _lib.ptr(table), _lib.stream_ptr(labels.device))
        _lib.check(rc, self.ctx, "unet_lesion_echo")
        return table

    def tta_views(self, x, views):
        """(K N, C, H, W): the views of x (N, C, H, W) in ascending k, view-major (unet_tta_views;
        views is the bit mask)."""
        N, C, H, W = x.shape
        out = torch.empty((bin(views).count("1") * N, C, H, W), dtype=torch.float32, device=x.device)
        rc = self.lib.unet_tta_views(self.ctx, _lib.ptr(x), N, C, H, W, views, _lib.ptr(out),
                                     _lib.stream_ptr(x.device))
        _lib.check(rc, self.ctx, "unet_tta_views")
        return out

    def tta_merge(self, logits, n, views, mode, want_mask=True, want_votes=True):
        """score float32, mask uint8, votes uint8, each (n, C, H, W) (None where not wanted), of
        the per-view logits (K n, C, H, W) (unet_tta_merge; mode 0 logit, 1 prob)."""
        _, C, H, W = logits.shape
        shape = (n, C, H, W)
        score = torch.empty(shape, dtype=torch.float32, device=logits.device)
        mask = torch.empty(shape, dtype=torch.uint8, device=logits.device) if want_mask else None
        votes = torch.empty(shape, dtype=torch.uint8, device=logits.device) if want_votes else None
        rc = self.lib.unet_tta_merge(self.ctx, _lib.ptr(logits), n, C, H, W, views, mode, _lib.ptr(score),
                                     _lib.ptr(mask), _lib.ptr(votes), _lib.stream_ptr(logits.device))
        _lib.check(rc, self.ctx, "unet_tta_merge")
        return score, mask, votes

    def curve_hist(self, logits, targets, edges, total):
        """plane_hist int32 (planes, 2, B) of logits / targets (planes, hw) against the B - 1 device
        edges; total int64 (2 B + 1) is accumulated (unet_curve_hist)."""
        planes, hw = logits.shape
        B = edges.numel() + 1
        ph = torch.empty((planes, 2, B), dtype=torch.int32, device=logits.device)
        rc = self.lib.unet_curve_hist(self.ctx, _lib.ptr(logits), _lib.ptr(targets), planes, hw, _lib.ptr(edges),
                                      B, _lib.ptr(ph), _lib.ptr(total), _lib.stream_ptr(logits.device))
        _lib.check(rc, self.ctx, "unet_curve_hist")
        return ph

    def curve_stats(self, plane_hist, dice_sum):
        """int64 (planes, 8) {P, Nn, best_k, TP, FP, FN, auc2, 0} of plane_hist (planes, 2, B);
        dice_sum float64 (B + 1) is accumulated in ascending plane order (unet_curve_stats)."""
        planes, _, B = plane_hist.shape
        out = torch.empty((planes, 8), dtype=torch.int64, device=plane_hist.device)
        rc = self.lib.unet_curve_stats(self.ctx, _lib.ptr(plane_hist), planes, B, _lib.ptr(out),
                                       _lib.ptr(dice_sum), _lib.stream_ptr(plane_hist.device))
        _lib.check(rc, self.ctx, "unet_curve_stats")
        return out

    EXPORT_PLAN_CACHE = 256  # axis plans kept per runtime (the least recently used leaves)

    def export_plan(self, n_in, n_out):
        """(coeffs float64, bounds int32, ksize) of unet_resize_f32_plan on this runtime's device,
        cached per (in, out); None for an unchanged axis."""
        if n_in == n_out:
            return None
        cache = self.__dict__.setdefault("_export_plans", collections.OrderedDict())
        key = (int(n_in), int(n_out))
        if key in cache:
            cache.move_to_end(key)
            return cache[key]
        from .functional import resize_f32_plan
        k, b = resize_f32_plan(*key)
        cache[key] = (torch.from_numpy(k).to(self.device), torch.from_numpy(b).to(self.device), k.shape[1])
        while len(cache) > self.EXPORT_PLAN_CACHE:
            cache.popitem(last=False)
        return cache[key]

    def resize_f32_mask(self, src, oh, ow, plan_h, plan_v, kind, thr, want_plane):
        """mask uint8 (oh, ow) and, when wanted, the float32 plane (oh, ow) of src (h, w) resized as
        Pillow resizes a mode "F" image (unet_resize_f32_mask).  plan_h / plan_v: (coeffs, bounds,
        ksize) on the device for w -> ow / h -> oh, None for an unchanged axis."""
        h, w = src.shape
        mask = torch.empty((oh, ow), dtype=torch.uint8, device=src.device)
        plane = torch.empty((oh, ow), dtype=torch.float32, device=src.device) if want_plane else None
        kh, bh, ksh = plan_h or (None, None, 0)
        kv, bv, ksv = plan_v or (None, None, 0)
        rc = self.lib.unet_resize_f32_mask(self.ctx, _lib.ptr(src), h, w, oh, ow, _lib.ptr(kh), _lib.ptr(bh), ksh,
                                           _lib.ptr(kv), _lib.ptr(bv), ksv, kind, float(thr), _lib.ptr(plane),
                                           _lib.ptr(mask), _lib.stream_ptr(src.device))
        _lib.check(rc, self.ctx, "unet_resize_f32_mask")
        return mask, plane

    def overlay_u8(self, gray, pred, gt, r, alpha):
        """rgb uint8 (h, w, 3) and stats int64 (6,) {area, contour pixels, x0, y0, x1, y1} of the
        uint8 planes gray, pred and gt (or None), each (h, w) (unet_overlay_u8)."""
        h, w = gray.shape
        rgb = torch.empty((h, w, 3), dtype=torch.uint8, device=gray.device)
        stats = torch.empty(6, dtype=torch.int64, device=gray.device)
        rc = self.lib.unet_overlay_u8(self.ctx, _lib.ptr(gray), _lib.ptr(pred), _lib.ptr(gt), h, w, int(r),
                                      int(alpha), _lib.ptr(rgb), _lib.ptr(stats), _lib.stream_ptr(gray.device))
        _lib.check(rc, self.ctx, "unet_overlay_u8")
        return rgb, stats

    def stream_wait_bucket(self, b, stream):
        rc = self.lib.unet_stream_wait_bucket(self.ctx, b, ctypes.c_void_p(stream.cuda_stream))
        _lib.check(rc, self.ctx, "unet_stream_wait_bucket")

    def bucket_event(self, b):
        """The hipEvent_t (as an int handle) the last backward recorded for bucket b -- what a
        caller driving RCCL without torch streams waits on (hipStreamWaitEvent)."""
        e = ctypes.c_void_p()
        _lib.check(self.lib.unet_bucket_event(self.ctx, b, ctypes.byref(e)), self.ctx,
                   "unet_bucket_event")
        return e.value

    # ------------------------------------------------------------------ timing
    def timing(self, enable, only=None):
        """Per-launch HIP-event timing; `only`: time just the labels containing it."""
        self.lib.unet_timing_enable(self.ctx, int(enable))
        self.lib.unet_timing_filter(self.ctx, only.encode() if only else None)
        self.lib.unet_timing_reset(self.ctx)

    def timing_records(self):
        n = ctypes.c_int()
        self.lib.unet_timing_count(self.ctx, ctypes.byref(n))
        out = []
        for i in range(n.value):
            fam, cnt, ms, fl = ctypes.c_char_p(), ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
            _lib.check(self.lib.unet_timing_read(self.ctx, i, ctypes.byref(fam), ctypes.byref(cnt),
                                                 ctypes.byref(ms), ctypes.byref(fl)), self.ctx, "timing")
            out.append((fam.value.decode(), ms.value, fl.value))
        self.lib.unet_timing_reset(self.ctx)
        return out

    # ------------------------------------------------------------------ debug views
    def debug_view(self, workspace, N, H, W, training, kind, index):
        """A tensor view (NHWC pixels x channels, or a vector) of an intermediate buffer."""
        bo, cnt, ld, off = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int(), ctypes.c_int()
        _lib.check(self.lib.unet_debug_view(self.ctx, N, H, W, int(training), kind, index,
                                            ctypes.byref(bo), ctypes.byref(cnt), ctypes.byref(ld),
                                            ctypes.byref(off)), self.ctx, "unet_debug_view")
        if kind == 8:  # uint8 max-pool winner index
            return workspace[bo.value:bo.value + cnt.value].view(-1, ld.value), off.value
        flat = workspace[bo.value:bo.value + 4 * cnt.value].view(torch.float32)
        if kind in (1, 2, 3, 4):
            return flat
        return flat.view(-1, ld.value), off.value
