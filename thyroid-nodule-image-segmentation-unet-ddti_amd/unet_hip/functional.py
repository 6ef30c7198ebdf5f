"""autograd bridges from PyTorch to the native kernels.

* ``UNetFunction``  - forward/backward of the whole encoder-decoder
  (models/model.py:53-73 forward, utils/trainer.py:91 backward).  Gradients land in one
  flat arena laid out like the parameter arena, a fresh one per backward; autograd receives
  views of it.  A graph runs backward once: the backward consumes the forward's workspace.
* ``SegLossFunction`` - the fused BCEWithLogits (mean) + Dice + FocalTversky statistics
  kernel (utils/trainer.py:85-87, models/loss.py:13-46), with an optional all-reduce of
  the 8 batch sums between the statistics and the finalize (data parallelism = the loss of
  the gathered batch, as nn.DataParallel computes it).  It returns the 3-vector
  ``[bce, dice, focal]``; its backward takes the incoming gradient of that vector as the
  per-term weights, so ``bce_ratio*l[0] + dice_ratio*l[1] + ...`` (utils/trainer.py:90)
  differentiates into ONE dlogits kernel with no host synchronisation.
* ``BoundaryLossFunction`` - BoundaryLoss (models/loss.py:48-66) over a distance map computed
  on the device (``distance_maps``: the exact Euclidean distance transform kernels); its
  backward is one dlogits kernel weighted by the incoming gradient, again with no host sync.
* ``LovaszHingeFunction`` - the Lovasz hinge loss over a stable segmented radix sort of every
  plane's margin errors on the device (``lovasz_hinge``); the forward saves the per-pixel weights
  ``gmap`` and the backward is one dlogits kernel over them, with no host sync.
"""
import functools

import torch
import torch.distributed as dist

from ._lib import HipUnavailable


class UNetFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, state, *params):
        state.sync_params()
        logits, ws = state.rt.forward(state.param_arena, state.bn_arena, state.nbt_arena, x,
                                      training=True)
        ctx.state = state
        ctx.ws = ws
        ctx.n_params = len(params)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        st = ctx.state
        if ctx.ws is None:
            raise RuntimeError("UNetFunction: the workspace of a training forward is consumed by "
                               "its backward, so a graph runs backward once (retain_graph=True "
                               "does not keep it); run the forward again for another backward")
        grads = st.grad_arena_for_backward()
        st.rt.backward(st.param_arena, dlogits.contiguous(), grads, ctx.ws)
        ctx.ws = None
        return (None, None) + tuple(st.grad_views(grads))


class SegLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, rt, alpha, beta, gamma, group):
        logits = logits.contiguous()
        targets = targets.contiguous().float()
        stats, sums = rt.loss_stats(logits, targets)
        if group is not None:
            # nn.DataParallel evaluates the losses on the gathered batch (utils/trainer.py:
            # 28-30,85-90): summing the 8 batch sums over the ranks makes every rank's
            # finalize see exactly that batch (incl. FocalTversky's global TP/FP/FN)
            dist.all_reduce(sums, group=group)
        losses = rt.loss_finalize(sums, alpha, beta, gamma)
        ctx.save_for_backward(logits, targets, stats, sums)
        ctx.rt, ctx.abg = rt, (alpha, beta, gamma)
        return losses

    @staticmethod
    def backward(ctx, g):
        logits, targets, stats, sums = ctx.saved_tensors
        w = g.contiguous().float()
        d = ctx.rt.loss_bwd(logits, targets, stats, sums, w, *ctx.abg)
        return d, None, None, None, None, None, None


def seg_losses(logits, targets, alpha=0.4, beta=0.6, gamma=2.0, group=None):
    """[bce_mean, dice_loss, focal_tversky] of logits vs targets on the HIP path.

    group: a torch.distributed process group whose ranks each hold one shard of the batch.
    The losses (and their gradients) are then those of the GATHERED batch, as with the
    reference's nn.DataParallel: every rank returns the same three values, its dlogits are
    its slice of the gathered batch's dlogits, and the ranks' parameter gradients must be
    SUMMED (``DistributedUNet`` does that).  Unequal shards are handled exactly."""
    if logits.device.type != "cuda":
        raise HipUnavailable("seg_losses runs on the HIP path only (got a CPU tensor)")
    from .runtime import UNetRuntime
    rt = UNetRuntime.get(logits.device)
    if targets.shape != logits.shape:
        raise ValueError(f"targets {tuple(targets.shape)} != logits {tuple(logits.shape)}")
    return SegLossFunction.apply(logits, targets, rt, float(alpha), float(beta), float(gamma),
                                 group)


class BoundaryLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, dist, rt):
        logits = logits.contiguous()
        loss = rt.boundary_fwd(logits, targets, dist)
        ctx.save_for_backward(logits, targets, dist)
        ctx.rt = rt
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, targets, dist = ctx.saved_tensors
        w = g.contiguous().float().reshape(1)
        return ctx.rt.boundary_bwd(logits, targets, dist, w), None, None, None


def _boundary_runtime(t, what):
    if t.device.type != "cuda":
        raise HipUnavailable(f"{what} runs on the HIP path only (got a CPU tensor)")
    from .runtime import UNetRuntime
    return UNetRuntime.get(t.device)


def distance_maps(targets):
    """float32 (N, 1, H, W): Euclidean distance of every pixel to the nearest pixel of
    targets[:, 0] whose uint8 cast is 1 -- bit for bit
    ``scipy.ndimage.distance_transform_edt(1 - targets.astype(np.uint8)[n, 0])`` cast to
    float32 (models/loss.py:55-61), including scipy's result for a sample without any such
    pixel.  Computed on the device, on the current stream; max(H, W) <= 2048."""
    rt = _boundary_runtime(targets, "distance_maps")
    if targets.dim() != 4:
        raise ValueError(f"targets must be (N, C, H, W), got {tuple(targets.shape)}")
    return rt.edt(targets.detach().contiguous().float())


def boundary_loss(logits, targets, dist=None):
    """mean_n mean_hw |sigmoid(logits[n, 0]) - targets[n, 0]| * dist[n] (models/loss.py:48-66)
    on the HIP path.  dist: a precomputed ``distance_maps(targets)``; None computes it."""
    rt = _boundary_runtime(logits, "boundary_loss")
    if targets.shape != logits.shape:
        raise ValueError(f"targets {tuple(targets.shape)} != logits {tuple(logits.shape)}")
    targets = targets.detach().contiguous().float()
    if dist is None:
        dist = rt.edt(targets)
    else:
        N, _, H, W = logits.shape
        if tuple(dist.shape) != (N, 1, H, W) or dist.device != logits.device:
            raise ValueError(f"dist must be {(N, 1, H, W)} on {logits.device}, got "
                             f"{tuple(dist.shape)} on {dist.device}")
        dist = dist.detach().contiguous().float()
    return BoundaryLossFunction.apply(logits, targets, dist, rt)


class LovaszHingeFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, rt):
        logits = logits.contiguous()
        loss, gmap, _, _ = rt.lovasz_fwd(logits, targets)
        ctx.save_for_backward(logits, targets, gmap)
        ctx.rt = rt
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, targets, gmap = ctx.saved_tensors
        w = g.contiguous().float().reshape(1)
        return ctx.rt.lovasz_bwd(logits, targets, gmap, w), None, None


def _lovasz_args(logits, targets):
    if logits.dim() != 4 or targets.shape != logits.shape:
        raise ValueError(f"logits / targets must be equal (N, C, H, W), got {tuple(logits.shape)} / "
                         f"{tuple(targets.shape)}")
    return targets.detach().contiguous().float()


def lovasz_hinge(logits, targets):
    """The Lovasz hinge loss (Berman et al., CVPR 2018, ``per_image=True``) on the HIP path and the
    current stream, no host synchronisation: the mean over the (n, c) planes of
    sum_r max(e_r, 0) g_r, e = 1 - s x sorted descending (ties by raster index: a stable radix sort
    on the device) and g the increments of the Jaccard loss along the sorted order.  Soft targets
    are binarised at 0.5 (``t >= 0.5`` is positive).  H W <= 2^24."""
    rt = _boundary_runtime(logits, "lovasz_hinge")
    targets = _lovasz_args(logits, targets)
    return LovaszHingeFunction.apply(logits.float(), targets, rt)


def lovasz_hinge_parts(logits, targets, want_perm=False):
    """What ``unet_lovasz_fwd`` writes, without autograd: a dict of ``loss`` (0-dim float32),
    ``gmap`` (N, C, H, W) float32 (the per-pixel weight g_rank(i), 0 where e_i <= 0), ``sum``
    (float64[1], the planes' losses added up) and ``perm`` (int32 (N, C, H W): every plane's raster
    indices in sorted order; None unless wanted)."""
    rt = _boundary_runtime(logits, "lovasz_hinge_parts")
    targets = _lovasz_args(logits, targets)
    loss, gmap, s, perm = rt.lovasz_fwd(logits.detach().contiguous().float(), targets, want_perm)
    return dict(loss=loss, gmap=gmap, sum=s, perm=perm)


def lovasz_hinge_host(logits, targets, want_perm=False):
    """``lovasz_hinge_parts`` of CPU tensors through the library's host twin (unet_lovasz_host: the
    device kernels' rules with a stable sort by key)."""
    _cc_cpu(logits, "lovasz_hinge_host")
    _cc_cpu(targets, "lovasz_hinge_host")
    t = _lovasz_args(logits, targets)
    x = logits.detach().contiguous().float()
    N, C, H, W = x.shape
    gmap = torch.empty_like(x)
    perm = torch.empty((N, C, H * W), dtype=torch.int32) if want_perm else None
    s = torch.empty(1, dtype=torch.float64)
    loss = torch.empty((), dtype=torch.float32)
    _cc_host_call("unet_lovasz_host", x, t, N, C, H, W, gmap, perm, s, loss)
    return dict(loss=loss, gmap=gmap, sum=s, perm=perm)


SURFACE_FIELDS = ("defined", "n_pg", "n_gp", "max_d2", "d2_lo", "d2_hi")


def _sqrt_i64(t):
    """float64 sqrt of an int64 tensor, correctly rounded: the device's sqrt is; torch's
    vectorised CPU sqrt is not (an ulp off for about 1 integer in 150), numpy's is."""
    if t.device.type == "cpu":
        import numpy as np
        return torch.from_numpy(np.sqrt(t.numpy().astype(np.float64)))
    return t.double().sqrt()


def _surface_finalize(oi, of):
    """The per-sample fields of unet_surface_stats -> a dict with them (int64 / float64, shape
    (N,)) and hd, hd95, assd (float64, NaN where defined == 0).  Torch on the input's device:
    a square root, numpy's linear interpolation and two means per sample."""
    out = {k: oi[:, i] for i, k in enumerate(SURFACE_FIELDS)}
    out["sum_pg"], out["sum_gp"] = of[:, 0], of[:, 1]
    ok = out["defined"] != 0
    nan = torch.full_like(of[:, 0], float("nan"))
    lo, hi = _sqrt_i64(out["d2_lo"]), _sqrt_i64(out["d2_hi"])
    pos = 0.95 * (out["n_pg"] + out["n_gp"] - 1).double()  # numpy: (n - 1) * (95 / 100)
    g = pos - pos.floor()
    d = hi - lo  # numpy's _lerp: a + (b - a) t, and b - (b - a) (1 - t) from t = 0.5 on
    lerp = torch.where(g >= 0.5, hi - d * (1 - g), lo + d * g)
    out["hd"] = torch.where(ok, _sqrt_i64(out["max_d2"]), nan)
    out["hd95"] = torch.where(ok, lerp, nan)
    mean_pg = of[:, 0] / out["n_pg"].clamp(min=1).double()
    mean_gp = of[:, 1] / out["n_gp"].clamp(min=1).double()
    out["assd"] = torch.where(ok, (mean_pg + mean_gp) / 2, nan)
    return out


def _surface_args(logits, targets):
    if logits.dim() != 4 or targets.shape != logits.shape:
        raise ValueError(f"logits / targets must be equal (N, C, H, W), got {tuple(logits.shape)} / "
                         f"{tuple(targets.shape)}")
    return logits.detach().contiguous().float(), targets.detach().contiguous().float()


def surface_metrics(logits, targets):
    """Surface-distance metrics of the masks ``Trainer.test`` counts, per sample, on the device
    and the current stream (no host synchronisation): MedPy's ``hd``, ``hd95`` and ``assd`` at
    connectivity 1, in pixels, of P = sigmoid(logits[:, 0]) > 0.5 against G = (targets[:, 0]
    cast to an integer == 1).  Returns a dict of (N,) device tensors: int64 ``defined``, ``n_pg``,
    ``n_gp``, ``max_d2``, ``d2_lo``, ``d2_hi``; float64 ``sum_pg``, ``sum_gp``, ``hd``, ``hd95``,
    ``assd``.  A sample whose P or G is empty has defined == 0, zeros in the other fields and
    NaN in the three metrics.  max(H, W) <= 2048."""
    rt = _boundary_runtime(logits, "surface_metrics")
    return _surface_finalize(*rt.surface_stats(*_surface_args(logits, targets)))


def surface_metrics_host(logits, targets):
    """``surface_metrics`` of CPU tensors through the library's host hook
    (unet_surface_stats_host: the device kernels' source, compiled for the host)."""
    import ctypes

    from . import _lib
    if logits.device.type != "cpu" or targets.device.type != "cpu":
        raise ValueError("surface_metrics_host takes CPU tensors")
    x, t = _surface_args(logits, targets)
    N, C, H, W = x.shape
    oi = torch.empty((N, 6), dtype=torch.int64)
    of = torch.empty((N, 2), dtype=torch.float64)
    rc = _lib.load().unet_surface_stats_host(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(t.data_ptr()),
                                             N, C, H, W, ctypes.c_void_p(oi.data_ptr()),
                                             ctypes.c_void_p(of.data_ptr()))
    _lib.check(rc, None, "unet_surface_stats_host")
    return _surface_finalize(oi, of)


# ---------------------------------------------------------------- connected components
CC_KINDS = {"mask": 0, "logits": 1, "targets": 2}
LESION_FIELDS = ("n_pred", "n_gt", "gt_hit", "pred_hit")
POSTPROCESS_FIELDS = ("components", "kept", "pixels", "filled")


def _cc_args(x, kind):
    """x as a contiguous (N, C, H, W) tensor the library reads channel 0 of, and its kind code.
    (H, W) is one sample, (N, H, W) a batch of planes; uint8 (or bool) is a mask, float logits
    unless kind says "targets"."""
    x = x.detach()
    if x.dim() == 2:
        x = x[None, None]
    elif x.dim() == 3:
        x = x[:, None]
    elif x.dim() != 4:
        raise ValueError(f"expected (H, W), (N, H, W) or (N, C, H, W), got {tuple(x.shape)}")
    if kind is None:
        kind = "logits" if x.dtype.is_floating_point else "mask"
    if kind not in CC_KINDS:
        raise ValueError(f"kind must be one of {sorted(CC_KINDS)} or None, got {kind!r}")
    if kind == "mask":
        if x.dtype == torch.bool:
            x = x.to(torch.uint8)
        if x.dtype != torch.uint8:
            raise ValueError(f"a mask must be uint8 or bool, got {x.dtype}")
    else:
        x = x.float()
    return x.contiguous(), CC_KINDS[kind]


def _cc_host_call(name, *args):
    import ctypes

    from . import _lib
    conv = [ctypes.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]
    _lib.check(getattr(_lib.load(), name)(*conv), None, name)


def _cc_cpu(x, what):
    if x.device.type != "cpu":
        raise ValueError(f"{what} takes CPU tensors")


def connected_components(x, connectivity=1, kind=None):
    """``scipy.ndimage.label`` of every sample of x on the device and the current stream (no host
    synchronisation): (labels int32 (N, H, W), count int32 (N,)), 0 background and 1..count[n]
    the components in raster order of their first pixel, bit for bit scipy's numbering.
    connectivity 1 = 4 neighbours, 2 = 8.  x: a uint8 / bool mask (nonzero is foreground), float
    logits (the mask ``Trainer.test`` counts, sigmoid(x) > 0.5) or, with kind="targets", float
    targets ((int)t == 1); (H, W), (N, H, W) or (N, C, H, W), channel 0 read."""
    rt = _boundary_runtime(x, "connected_components")
    x, k = _cc_args(x, kind)
    return rt.components(x, k, int(connectivity))


def connected_components_host(x, connectivity=1, kind=None):
    """``connected_components`` of a CPU tensor through the library's host twin."""
    _cc_cpu(x, "connected_components_host")
    x, k = _cc_args(x, kind)
    N, C, H, W = x.shape
    labels = torch.empty((N, H, W), dtype=torch.int32)
    count = torch.empty(N, dtype=torch.int32)
    _cc_host_call("unet_components_host", x, k, N, C, H, W, int(connectivity), labels, count)
    return labels, count


def postprocess_mask(x, keep_largest=False, min_area=0, fill_holes=False, connectivity=1, kind=None):
    """Clean the masks of x (as ``connected_components`` reads them) on the device: drop the
    components with fewer than min_area pixels, then keep only the largest one left (ties: the
    first in raster order) if keep_largest, then fill holes as ``scipy.ndimage.binary_fill_holes``
    does if fill_holes.  Returns (mask uint8 (N, H, W) in {0, 1}, info int64 (N, 4) =
    {components before, components kept, foreground pixels after, pixels filled})."""
    rt = _boundary_runtime(x, "postprocess_mask")
    x, k = _cc_args(x, kind)
    return rt.postprocess(x, k, int(connectivity), keep_largest, min_area, fill_holes)


def postprocess_mask_host(x, keep_largest=False, min_area=0, fill_holes=False, connectivity=1, kind=None):
    """``postprocess_mask`` of a CPU tensor through the library's host twin."""
    _cc_cpu(x, "postprocess_mask_host")
    x, k = _cc_args(x, kind)
    N, C, H, W = x.shape
    out = torch.empty((N, H, W), dtype=torch.uint8)
    info = torch.empty((N, 4), dtype=torch.int64)
    _cc_host_call("unet_postprocess_host", x, k, N, C, H, W, int(connectivity), int(bool(keep_largest)),
                  int(min_area), int(bool(fill_holes)), out, info)
    return out, info


def _lesion_args(pred, targets, kind):
    p, k = _cc_args(pred, kind)
    t, _ = _cc_args(targets, "targets")
    if p.shape[0] != t.shape[0] or p.shape[2:] != t.shape[2:]:
        raise ValueError(f"pred {tuple(pred.shape)} and targets {tuple(targets.shape)} differ")
    if p.shape[1] != t.shape[1]:  # one channel count for both: channel 0 of each
        p, t = p[:, :1].contiguous(), t[:, :1].contiguous()
    return p, k, t


def lesion_metrics(pred, targets, connectivity=1, kind=None):
    """Lesion-level detection counts per sample, on the device: a dict of int64 (N,) tensors
    ``n_pred`` and ``n_gt`` (components of the prediction and of the targets), ``gt_hit`` (target
    components holding a predicted pixel) and ``pred_hit`` (predicted components holding a target
    pixel).  pred as in ``connected_components``; targets float, (int)t == 1 is foreground."""
    rt = _boundary_runtime(pred, "lesion_metrics")
    if targets.device != pred.device:
        raise ValueError("pred and targets must be on one device")
    p, k, t = _lesion_args(pred, targets, kind)
    out = rt.lesion_stats(p, k, t, int(connectivity))
    return {f: out[:, i] for i, f in enumerate(LESION_FIELDS)}


def lesion_metrics_host(pred, targets, connectivity=1, kind=None):
    """``lesion_metrics`` of CPU tensors through the library's host twin."""
    _cc_cpu(pred, "lesion_metrics_host")
    _cc_cpu(targets, "lesion_metrics_host")
    p, k, t = _lesion_args(pred, targets, kind)
    N, C, H, W = p.shape
    out = torch.empty((N, 4), dtype=torch.int64)
    _cc_host_call("unet_lesion_stats_host", p, k, t, N, C, H, W, int(connectivity), out)
    return {f: out[:, i] for i, f in enumerate(LESION_FIELDS)}


# ---------------------------------------------------------------- lesion morphometry
MORPH_FIELDS = ("area", "sx", "sy", "sxx", "sxy", "syy", "x0", "y0", "x1", "y1", "q1", "q2", "qd", "q3", "d2max",
                "first")
LESION_COLUMNS = ("name", "label", "area", "centroid_x", "centroid_y", "x0", "y0", "x1", "y1", "feret_max",
                  "major_axis", "minor_axis", "orientation", "eccentricity", "perimeter", "circularity", "holes",
                  "taller_than_wide")
LESION_COLUMNS_MM = ("feret_max_mm", "area_mm2")


def _morph_args(labels, count, max_rows):
    """labels as contiguous int32 (N, H, W), count as int32 (N,), max_rows as an int (None: the
    largest count, at least 1; reading it is the caller's one synchronisation)."""
    labels, count = labels.detach(), count.detach()
    if labels.dim() == 2:
        labels = labels[None]
    if labels.dim() != 3 or labels.dtype != torch.int32:
        raise ValueError(f"labels must be int32 (H, W) or (N, H, W), got {labels.dtype} {tuple(labels.shape)}")
    count = count.reshape(-1)
    if count.dtype != torch.int32 or count.numel() != labels.shape[0] or count.device != labels.device:
        raise ValueError(f"count must be int32 ({labels.shape[0]},) on the labels' device, got {count.dtype} "
                         f"{tuple(count.shape)} on {count.device}")
    if max_rows is None:
        max_rows = max(int(count.max()), 1)
    return labels.contiguous(), count.contiguous(), int(max_rows)


def morphometry_table(labels, count, max_rows=None):
    """The size and shape integers of every component of the label planes ``connected_components``
    returned, on the device and the current stream: int64 (N, max_rows, 16), row l - 1 for label l,
    the columns in ``MORPH_FIELDS`` order (area; sx, sy, sxx, sxy, syy over the pixels' column x and
    row y; the inclusive box x0, y0, x1, y1; the bit-quad counts q1, q2, qd, q3; d2max, the squared
    maximum Feret diameter between pixel centres; first, the smallest linear index).  Rows beyond
    count[n] are zero and components beyond max_rows are dropped (count says so).  All integer and
    exact.  max_rows=None reads ``count.max()`` (the only host synchronisation)."""
    rt = _boundary_runtime(labels, "morphometry_table")
    labels, count, max_rows = _morph_args(labels, count, max_rows)
    return rt.morphometry(labels, count, max_rows)


def morphometry_table_host(labels, count, max_rows=None):
    """``morphometry_table`` of CPU tensors through the library's host twin."""
    _cc_cpu(labels, "morphometry_table_host")
    labels, count, max_rows = _morph_args(labels, count, max_rows)
    N, H, W = labels.shape
    table = torch.empty((N, max(max_rows, 0), 16), dtype=torch.int64)
    _cc_host_call("unet_morphometry_host", labels, count, N, H, W, max_rows, table)
    return table


def lesion_morphometry(x, connectivity=1, kind=None, max_rows=None):
    """``connected_components`` of x, then ``morphometry_table`` of its labels, on the device: a dict
    of ``table`` int64 (N, max_rows, 16), ``count`` int32 (N,) and ``labels`` int32 (N, H, W)."""
    labels, count = connected_components(x, connectivity, kind)
    return {"table": morphometry_table(labels, count, max_rows), "count": count, "labels": labels}


def lesion_morphometry_host(x, connectivity=1, kind=None, max_rows=None):
    """``lesion_morphometry`` of a CPU tensor through the library's host twins."""
    labels, count = connected_components_host(x, connectivity, kind)
    return {"table": morphometry_table_host(labels, count, max_rows), "count": count, "labels": labels}


def shape_descriptors(table, spacing=1.0, connectivity=1):
    """Shape descriptors of the rows of a morphometry table, in NumPy float64 on the host from the
    integer rows alone.  table: int64 (..., 16) (a tensor or an array); every returned array has the
    shape ``table.shape[:-1]``, and a row without pixels gives zeros.  x is the column, y the row
    (y grows downwards); lengths are multiplied by ``spacing``, areas by ``spacing ** 2``.

    ``area``; ``centroid_x``, ``centroid_y`` = sx / area, sy / area; ``mu20``, ``mu11``, ``mu02`` the
    normalised second central moments, e.g. (area sxx - sx^2) / area^2 with the numerator formed in
    Python integers before the one division; ``major_axis``, ``minor_axis`` = 4 sqrt(lambda) of the
    eigenvalues of [[mu20, mu11], [mu11, mu02]] (the axes of the ellipse with the same moments);
    ``orientation`` the angle of the major axis from the x axis towards the y axis, radians in
    (-pi/2, pi/2]; ``eccentricity`` = sqrt(1 - lambda_min / lambda_max); ``feret_max`` = sqrt(d2max);
    ``box_w``, ``box_h``; ``taller_than_wide`` = box_h > box_w (image rows run along the beam, so on
    a transverse frame this is the TI-RADS taller-than-wide sign: the antero-posterior extent exceeds
    the transverse one); ``extent`` = area / box area; ``perimeter_crack`` = q1 + q2 + q3 + 2 qd
    (the pixel-edge length of the outline, holes included); ``perimeter`` = q2 + (q1 + q3 + 2 qd) /
    sqrt(2) (the bit-quad estimate); ``circularity`` = 4 pi area / perimeter^2; ``euler`` = (q1 - q3
    + 2 qd) / 4 at connectivity 1, (q1 - q3 - 2 qd) / 4 at 2; ``holes`` = 1 - euler."""
    import math

    import numpy as np
    if connectivity not in (1, 2):
        raise ValueError(f"connectivity must be 1 or 2, got {connectivity!r}")
    spacing = float(spacing)
    if not spacing > 0:
        raise ValueError(f"spacing must be positive, got {spacing!r}")
    t = table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    if t.shape[-1:] != (16,) or t.dtype != np.int64:
        raise ValueError(f"table must be int64 (..., 16), got {t.dtype} {t.shape}")
    shape = t.shape[:-1]
    rows = t.reshape(-1, 16)
    names = ("area", "centroid_x", "centroid_y", "mu20", "mu11", "mu02", "major_axis", "minor_axis", "orientation",
             "eccentricity", "feret_max", "box_w", "box_h", "extent", "perimeter_crack", "perimeter", "circularity",
             "euler", "holes")
    out = {k: np.zeros(len(rows), np.float64) for k in names}
    out["taller_than_wide"] = np.zeros(len(rows), bool)
    out["euler"] = np.zeros(len(rows), np.int64)
    out["holes"] = np.zeros(len(rows), np.int64)
    s2 = spacing * spacing
    for i, r in enumerate(rows.tolist()):  # Python ints: the central moments pass 2^64
        a, sx, sy, sxx, sxy, syy, x0, y0, x1, y1, q1, q2, qd, q3, d2, _ = r
        if a <= 0:
            continue
        a2 = a * a
        m20, m11, m02 = (a * sxx - sx * sx) / a2, (a * sxy - sx * sy) / a2, (a * syy - sy * sy) / a2
        mid, dev = (m20 + m02) / 2, math.hypot((m20 - m02) / 2, m11)
        l1, l2 = mid + dev, max(mid - dev, 0.0)
        bw, bh = x1 - x0 + 1, y1 - y0 + 1
        per = q2 + (q1 + q3 + 2 * qd) / math.sqrt(2.0)
        e4 = q1 - q3 + 2 * qd if connectivity == 1 else q1 - q3 - 2 * qd
        out["area"][i] = a * s2
        out["centroid_x"][i] = sx / a * spacing
        out["centroid_y"][i] = sy / a * spacing
        out["mu20"][i], out["mu11"][i], out["mu02"][i] = m20 * s2, m11 * s2, m02 * s2
        out["major_axis"][i] = 4 * math.sqrt(l1) * spacing
        out["minor_axis"][i] = 4 * math.sqrt(l2) * spacing
        out["orientation"][i] = 0.5 * math.atan2(2 * m11, m20 - m02) if dev > 0 else 0.0
        out["eccentricity"][i] = math.sqrt(max(1 - l2 / l1, 0.0)) if l1 > 0 else 0.0
        out["feret_max"][i] = math.sqrt(d2) * spacing
        out["box_w"][i], out["box_h"][i] = bw * spacing, bh * spacing
        out["taller_than_wide"][i] = bh > bw
        out["extent"][i] = a / (bw * bh)
        out["perimeter_crack"][i] = (q1 + q2 + q3 + 2 * qd) * spacing
        out["perimeter"][i] = per * spacing
        out["circularity"][i] = 4 * math.pi * a / (per * per)
        out["euler"][i] = e4 // 4
        out["holes"][i] = 1 - e4 // 4
    return {k: v.reshape(shape) for k, v in out.items()}


SHAPE_SUMS = ("n_pairs", "feret_abs", "area_rel", "centroid_dist", "ttw_both", "ttw_pred_only", "ttw_gt_only",
              "ttw_neither")


def shape_agreement(pred_rows, gt_rows):
    """How the size and shape of predicted lesions agree with the annotated ones: pred_rows, gt_rows
    int64 (n, 16), one table row per sample (its largest component; area 0 = none).  Over the pairs
    with both present, a float64 (8,) array in ``SHAPE_SUMS`` order: the pairs, the sums of
    |feret_max difference| (pixels), of |area_pred - area_gt| / area_gt and of the centroid distance,
    and the 2 x 2 counts of ``taller_than_wide`` (both, prediction only, annotation only, neither)."""
    import numpy as np
    dp, dg = shape_descriptors(pred_rows), shape_descriptors(gt_rows)
    both = (dp["area"] > 0) & (dg["area"] > 0)
    tp, tg = dp["taller_than_wide"][both], dg["taller_than_wide"][both]
    return np.array([both.sum(), np.abs(dp["feret_max"] - dg["feret_max"])[both].sum(),
                     (np.abs(dp["area"] - dg["area"])[both] / dg["area"][both]).sum(),
                     np.hypot(dp["centroid_x"] - dg["centroid_x"], dp["centroid_y"] - dg["centroid_y"])[both].sum(),
                     (tp & tg).sum(), (tp & ~tg).sum(), (~tp & tg).sum(), (~tp & ~tg).sum()], np.float64)


def shape_summary(sums):
    """The SHAPE block's numbers from the ``SHAPE_SUMS`` (summed over the test set): ``n_pairs``, the
    means ``feret_mae``, ``area_rel_err`` and ``centroid_dist`` (nan without a pair), the agreement
    counts ``ttw`` and Cohen's ``kappa`` of them (nan when chance agreement is 1)."""
    n, fe, ar, ce, a, b, c, d = (float(v) for v in sums)
    nan = float("nan")
    out = dict(n_pairs=int(n), feret_mae=fe / n if n else nan, area_rel_err=ar / n if n else nan,
               centroid_dist=ce / n if n else nan, ttw=[int(a), int(b), int(c), int(d)])
    pe = ((a + b) * (a + c) + (c + d) * (b + d)) / (n * n) if n else 1.0
    out["kappa"] = ((a + d) / n - pe) / (1 - pe) if pe != 1.0 else nan
    return out


def lesion_csv_lines(name, table, count, pixel_spacing=None, connectivity=1, echo=None):
    """The lines of lesions.csv (no newline) for one frame: one per component, the ``LESION_COLUMNS``
    in pixels (integers as such, real numbers with four decimals, the orientation in radians), then
    with a spacing in millimetres per pixel the ``LESION_COLUMNS_MM``, then with ``echo`` (the frame's
    ``echo_table`` rows, int32 (rows, 512 + G^2)) the ``LESION_COLUMNS_ECHO`` of ``echo_descriptors``:
    the reals with four decimals (``nan`` where undefined), and, by this file's integers-as-such rule,
    the five columns that are whole numbers by construction (echo_median, echo_p10, echo_p90: grey
    values; ring_pixels: a count; echo_class: -1, 0 or 1) without a decimal point.
    table: int64 (rows, 16), count: the frame's component count (rows beyond the table were dropped
    and write no line)."""
    k = min(int(count), int(table.shape[0]))
    d = shape_descriptors(table[:k], 1.0, connectivity)
    rows = (table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else table)[:k]
    if echo is not None:
        if int(echo.shape[0]) < k:
            raise ValueError(f"echo has {int(echo.shape[0])} rows for {k} components")
        e = echo_descriptors(echo[:k])
    lines = []
    for i in range(k):
        f = [str(name), str(i + 1), str(int(rows[i][0])), f"{d['centroid_x'][i]:.4f}", f"{d['centroid_y'][i]:.4f}"]
        f += [str(int(rows[i][c])) for c in (6, 7, 8, 9)]
        f += [f"{d[c][i]:.4f}" for c in ("feret_max", "major_axis", "minor_axis", "orientation", "eccentricity",
                                         "perimeter", "circularity")]
        f += [str(int(d["holes"][i])), str(int(d["taller_than_wide"][i]))]
        if pixel_spacing is not None:
            sp = float(pixel_spacing)
            f += [f"{d['feret_max'][i] * sp:.4f}", f"{int(rows[i][0]) * sp * sp:.4f}"]
        if echo is not None:
            for c in LESION_COLUMNS_ECHO:
                v = e[_ECHO_CSV_SOURCE.get(c, c)][i]
                whole = c in _ECHO_CSV_INTEGERS and v == v
                f.append(str(int(v)) if whole else f"{v:.4f}")
        lines.append(",".join(f))
    return lines


# ---------------------------------------------------------------- lesion echogenicity and texture
ECHO_LEVELS = (8, 16, 32)
ECHO_MAX_RING = 16
LESION_COLUMNS_ECHO = ("echo_mean", "echo_std", "echo_median", "echo_p10", "echo_p90", "echo_entropy", "ring_pixels",
                       "ring_mean", "ring_std", "echo_ratio", "echo_cnr", "echo_class", "glcm_contrast",
                       "glcm_homogeneity", "glcm_energy", "glcm_correlation", "glcm_entropy")
# the CSV column -> the key of echo_descriptors, where they differ; the columns written as integers
_ECHO_CSV_SOURCE = {"echo_mean": "mean", "echo_std": "std", "echo_median": "median", "echo_p10": "p10",
                    "echo_p90": "p90", "echo_entropy": "entropy"}
_ECHO_CSV_INTEGERS = ("echo_median", "echo_p10", "echo_p90", "ring_pixels", "echo_class")


def _echo_args(gray, labels, count, max_rows, levels, ring):
    """``_morph_args`` of labels and count; gray as contiguous uint8 of the labels' shape on their
    device; levels and ring as checked ints."""
    labels, count, max_rows = _morph_args(labels, count, max_rows)
    gray = gray.detach()
    if gray.dim() == 2:
        gray = gray[None]
    if gray.dtype != torch.uint8 or gray.shape != labels.shape or gray.device != labels.device:
        raise ValueError(f"gray must be uint8 {tuple(labels.shape)} on the labels' device, got {gray.dtype} "
                         f"{tuple(gray.shape)} on {gray.device}")
    if isinstance(levels, bool) or levels not in ECHO_LEVELS:
        raise ValueError(f"levels must be one of {ECHO_LEVELS}, got {levels!r}")
    if isinstance(ring, bool) or not isinstance(ring, int) or not 0 <= ring <= ECHO_MAX_RING:
        raise ValueError(f"ring must be an int in 0..{ECHO_MAX_RING}, got {ring!r}")
    return gray.contiguous(), labels, count, max_rows, int(levels), int(ring)


def echo_table(gray, labels, count, max_rows=None, levels=16, ring=8):
    """The grey-value counts of every component of the label planes ``connected_components`` returned,
    on the device and the current stream: int32 (N, max_rows, 512 + levels^2), row l - 1 for label l.
    gray: uint8 (N, H, W), the planes the labels were found on.  Columns 0..255 the histogram of the
    component's pixels; 256..511 the histogram of the background pixels within chessboard distance
    ``ring`` that it owns (the smallest label in reach owns a pixel; ring 0: all zero); from 512 the
    levels x levels co-occurrence counts of the quantised levels (g levels) >> 8 over the ordered pairs
    (p, p + (0, 1)), (1, 1), (1, 0), (1, -1) inside the component, the four directions summed.  Rows
    beyond count[n] are zero and components beyond max_rows are dropped (count says so).  All integer
    and exact.  max_rows=None reads ``count.max()`` (the only host synchronisation)."""
    rt = _boundary_runtime(labels, "echo_table")
    gray, labels, count, max_rows, levels, ring = _echo_args(gray, labels, count, max_rows, levels, ring)
    return rt.lesion_echo(gray, labels, count, max_rows, levels, ring)


def echo_table_host(gray, labels, count, max_rows=None, levels=16, ring=8):
    """``echo_table`` of CPU tensors through the library's host twin."""
    _cc_cpu(labels, "echo_table_host")
    gray, labels, count, max_rows, levels, ring = _echo_args(gray, labels, count, max_rows, levels, ring)
    N, H, W = labels.shape
    table = torch.empty((N, max(max_rows, 0), 512 + levels * levels), dtype=torch.int32)
    _cc_host_call("unet_lesion_echo_host", gray, labels, count, N, H, W, max_rows, levels, ring, table)
    return table


def lesion_echo(x, gray, connectivity=1, kind=None, max_rows=None, levels=16, ring=8):
    """``connected_components`` of x, then ``echo_table`` of its labels over gray, on the device: a
    dict of ``table`` int32 (N, max_rows, 512 + levels^2), ``count`` int32 (N,) and ``labels``."""
    labels, count = connected_components(x, connectivity, kind)
    return {"table": echo_table(gray, labels, count, max_rows, levels, ring), "count": count, "labels": labels}


def lesion_echo_host(x, gray, connectivity=1, kind=None, max_rows=None, levels=16, ring=8):
    """``lesion_echo`` of CPU tensors through the library's host twins."""
    labels, count = connected_components_host(x, connectivity, kind)
    return {"table": echo_table_host(gray, labels, count, max_rows, levels, ring), "count": count, "labels": labels}


def _hist_quantile(cum, n, p):
    """The smallest g with 100 cum[g] >= p n (NumPy's ``inverted_cdf``), cum the running integer sum."""
    for g, c in enumerate(cum):
        if 100 * c >= p * n:
            return g
    return len(cum) - 1


def _hist_moments(h):
    """n and the integers n^k m_k (k = 2, 3, 4) of the central moments m_k of an integer histogram,
    with S1 = sum g h[g]: exact in Python ints."""
    n = sum(h)
    s1 = sum(g * c for g, c in enumerate(h))
    s2 = sum(g * g * c for g, c in enumerate(h))
    s3 = sum(g ** 3 * c for g, c in enumerate(h))
    s4 = sum(g ** 4 * c for g, c in enumerate(h))
    m2 = n * s2 - s1 * s1
    m3 = n * n * s3 - 3 * n * s1 * s2 + 2 * s1 ** 3
    m4 = n ** 3 * s4 - 4 * n * n * s1 * s3 + 6 * n * s1 * s1 * s2 - 3 * s1 ** 4
    return n, s1, m2, m3, m4


def echo_descriptors(table, levels=None):
    """Echogenicity and texture descriptors of the rows of an ``echo_table``, in NumPy float64 on the
    host from the integer rows alone (moments formed in Python ints before the one division).  table:
    int32 (..., 512 + levels^2) (a tensor or an array; levels=None reads it off the width); every
    returned array has the shape ``table.shape[:-1]``.  A row without pixels gives zeros; a quantity
    without a defined value gives nan (skewness of constant grey, anything of an empty ring, a ratio
    over 0, the co-occurrence descriptors without a pair).

    From the lesion histogram: ``pixels``, ``mean``, ``std`` (population), ``skewness``, ``kurtosis``
    (excess), ``min``, ``max``, ``median``, ``p10``, ``p90`` (quantile p: the smallest g whose cumulative
    count c has 100 c >= p n, NumPy's ``inverted_cdf``), ``entropy`` (bits over the 256 bins).  From the
    ring histogram: ``ring_pixels``, ``ring_mean``, ``ring_std``, ``ring_p25``, ``ring_p75``.  Lesion
    against ring: ``echo_ratio`` = mean / ring_mean, ``echo_cnr`` = |mean - ring_mean| / sqrt(std^2 +
    ring_std^2), ``echo_class`` = -1 (hypoechoic) if median < ring_p25, +1 (hyperechoic) if median >
    ring_p75, else 0 (isoechoic, and with an empty ring).  From P = (C + C^T) / (2 pairs) of the
    co-occurrence counts C: ``glcm_pairs``, ``glcm_contrast`` = sum (i - j)^2 P, ``glcm_dissimilarity``
    = sum |i - j| P, ``glcm_homogeneity`` = sum P / (1 + (i - j)^2), ``glcm_energy`` = sqrt(sum P^2),
    ``glcm_correlation`` (1 when the level variance is 0), ``glcm_entropy`` (bits)."""
    import math

    import numpy as np
    t = table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    width = t.shape[-1] if t.ndim else 0
    G = math.isqrt(max(width - 512, 0)) if levels is None else levels
    if G not in ECHO_LEVELS or width != 512 + G * G or t.dtype != np.int32:
        raise ValueError(f"table must be int32 (..., 512 + levels^2) with levels in {ECHO_LEVELS}, got {t.dtype} "
                         f"{t.shape} (levels {levels!r})")
    shape = t.shape[:-1]
    rows = t.reshape(-1, width)
    reals = ("mean", "std", "skewness", "kurtosis", "min", "max", "median", "p10", "p90", "entropy", "ring_mean",
             "ring_std", "ring_p25", "ring_p75", "echo_ratio", "echo_cnr", "glcm_contrast", "glcm_dissimilarity",
             "glcm_homogeneity", "glcm_energy", "glcm_correlation", "glcm_entropy")
    out = {k: np.zeros(len(rows), np.float64) for k in reals}
    for k in ("pixels", "ring_pixels", "glcm_pairs", "echo_class"):
        out[k] = np.zeros(len(rows), np.int64)
    nan = float("nan")
    ii, jj = np.mgrid[:G, :G]
    d2 = ((ii - jj) ** 2).astype(np.int64)

    def entropy(counts, total):
        p = counts[counts > 0].astype(np.float64) / total
        return float(-(p * np.log2(p)).sum()) + 0.0  # one bin: 0, not -0

    for r, row in enumerate(rows):
        h = row[:256].tolist()
        n, s1, m2, m3, m4 = _hist_moments(h)
        if n <= 0:
            continue
        cum = np.cumsum(row[:256].astype(np.int64)).tolist()
        mean, var = s1 / n, m2 / (n * n)
        out["pixels"][r] = n
        out["mean"][r], out["std"][r] = mean, math.sqrt(var)
        out["skewness"][r] = m3 / math.sqrt(m2) ** 3 if m2 > 0 else nan
        out["kurtosis"][r] = m4 / (m2 * m2) - 3 if m2 > 0 else nan
        nz = [g for g, c in enumerate(h) if c]
        out["min"][r], out["max"][r] = nz[0], nz[-1]
        med = _hist_quantile(cum, n, 50)
        out["median"][r], out["p10"][r], out["p90"][r] = med, _hist_quantile(cum, n, 10), _hist_quantile(cum, n, 90)
        out["entropy"][r] = entropy(row[:256], n)
        # the ring
        rn, rs1, rm2, _, _ = _hist_moments(row[256:512].tolist())
        out["ring_pixels"][r] = rn
        if rn > 0:
            rcum = np.cumsum(row[256:512].astype(np.int64)).tolist()
            rmean, rvar = rs1 / rn, rm2 / (rn * rn)
            p25, p75 = _hist_quantile(rcum, rn, 25), _hist_quantile(rcum, rn, 75)
            out["ring_mean"][r], out["ring_std"][r] = rmean, math.sqrt(rvar)
            out["ring_p25"][r], out["ring_p75"][r] = p25, p75
            out["echo_ratio"][r] = mean / rmean if rs1 > 0 else nan
            out["echo_cnr"][r] = abs(mean - rmean) / math.sqrt(var + rvar) if m2 > 0 or rm2 > 0 else nan
            out["echo_class"][r] = -1 if med < p25 else (1 if med > p75 else 0)
        else:
            for k in ("ring_mean", "ring_std", "ring_p25", "ring_p75", "echo_ratio", "echo_cnr"):
                out[k][r] = nan
        # the co-occurrence matrix
        C = row[512:].astype(np.int64).reshape(G, G)
        S = C + C.T  # 2 pairs P
        T = int(S.sum())
        out["glcm_pairs"][r] = T // 2
        if T == 0:
            for k in reals:
                if k.startswith("glcm_"):
                    out[k][r] = nan
            continue
        out["glcm_contrast"][r] = int((d2 * S).sum()) / T
        out["glcm_dissimilarity"][r] = int((np.abs(ii - jj) * S).sum()) / T
        out["glcm_homogeneity"][r] = float((S / (1.0 + d2)).sum()) / T
        out["glcm_energy"][r] = math.sqrt(int((S * S).sum())) / T
        marg = S.sum(axis=1)
        a, b = int((np.arange(G) * marg).sum()), int((np.arange(G) ** 2 * marg).sum())
        cij = int((ii * jj * S).sum())
        out["glcm_correlation"][r] = (T * cij - a * a) / (T * b - a * a) if T * b - a * a > 0 else 1.0
        out["glcm_entropy"][r] = entropy(S, T)
    return {k: v.reshape(shape) for k, v in out.items()}


# ---------------------------------------------------------------- test-time augmentation
TTA_SETS = {"hflip": 0x03, "flips": 0x0F, "d4": 0xFF}
TTA_MODES = {"logit": 0, "prob": 1}


def tta_view_mask(views):
    """The bit mask (bit k = view k) of a named set ("hflip", "flips", "d4"), an iterable of view
    numbers or a mask.  View k: h = k & 1, v = k >> 1 & 1, t = k >> 2 & 1 and
    T_k(x) = x, transposed if t, then flipped vertically if v, then horizontally if h."""
    if isinstance(views, str):
        if views not in TTA_SETS:
            raise ValueError(f"views must be one of {sorted(TTA_SETS)}, a mask or view numbers, got {views!r}")
        return TTA_SETS[views]
    if isinstance(views, int):
        return views
    m = 0
    for k in views:
        if not 0 <= int(k) <= 7:
            raise ValueError(f"a view number must be in 0..7, got {k}")
        m |= 1 << int(k)
    return m


def tta_view_numbers(views):
    """The view numbers of a set, ascending: the order of the stacked views."""
    m = tta_view_mask(views)
    return [k for k in range(8) if m >> k & 1]


def _tta_mode(mode):
    if mode not in TTA_MODES:
        raise ValueError(f"mode must be one of {sorted(TTA_MODES)}, got {mode!r}")
    return TTA_MODES[mode]


tta_mode = _tta_mode  # the public name: the code of a merge mode, or the refusal of an unknown one


def _tta_4d(x, what):
    if x.dim() != 4:
        raise ValueError(f"{what} must be (N, C, H, W), got {tuple(x.shape)}")
    x = x.detach()
    # a float32 view is passed as it is (a 4-byte aligned base is legal)
    return x if x.dtype == torch.float32 and x.is_contiguous() else x.float().contiguous()


def _tta_split(logits, n, views):
    m = tta_view_mask(views)
    K = bin(m & 0xFF).count("1")
    if K and logits.shape[0] != K * int(n):
        raise ValueError(f"logits hold {logits.shape[0]} planes, expected {K} views x {n} samples")
    return m


def tta_views(x, views):
    """The test-time-augmentation views of x (N, C, H, W) on the device and the current stream:
    (K N, C, H, W), view-major (out[q N + n] = T_{k_q}(x[n]), the views in ascending k).  A pure
    permutation.  A view with k >= 4 (transpose, quarter turns) needs H == W."""
    rt = _boundary_runtime(x, "tta_views")
    return rt.tta_views(_tta_4d(x, "x"), tta_view_mask(views))


def tta_views_host(x, views):
    """``tta_views`` of a CPU tensor through the library's host twin."""
    _cc_cpu(x, "tta_views_host")
    x, m = _tta_4d(x, "x"), tta_view_mask(views)
    N, C, H, W = x.shape
    out = torch.empty((bin(m & 0xFF).count("1") * N, C, H, W), dtype=torch.float32)
    _cc_host_call("unet_tta_views_host", x, N, C, H, W, m, out)
    return out


def tta_merge(logits, n, views, mode="prob"):
    """Un-warp and merge the model's logits of ``tta_views`` ((K n, C, H, W), the same order) in
    one pass on the device: a dict of (n, C, H, W) tensors ``score`` (float32: the mean over the
    views of the probabilities for mode "prob", of the logits for "logit", summed in float32 in
    ascending view order), ``mask`` (uint8: score > 0.5, resp. sigmoid(score) > 0.5 as
    ``Trainer.test`` forms it) and ``votes`` (uint8: how many views predict foreground)."""
    rt = _boundary_runtime(logits, "tta_merge")
    logits = _tta_4d(logits, "logits")
    m = _tta_split(logits, n, views)
    score, mask, votes = rt.tta_merge(logits, int(n), m, _tta_mode(mode))
    return dict(score=score, mask=mask, votes=votes)


def tta_merge_host(logits, n, views, mode="prob"):
    """``tta_merge`` of a CPU tensor through the library's host twin."""
    _cc_cpu(logits, "tta_merge_host")
    logits = _tta_4d(logits, "logits")
    m = _tta_split(logits, n, views)
    _, C, H, W = logits.shape
    shape = (int(n), C, H, W)
    score = torch.empty(shape, dtype=torch.float32)
    mask = torch.empty(shape, dtype=torch.uint8)
    votes = torch.empty(shape, dtype=torch.uint8)
    _cc_host_call("unet_tta_merge_host", logits, int(n), C, H, W, m, _tta_mode(mode), score, mask, votes)
    return dict(score=score, mask=mask, votes=votes)


def tta_predict(model, images, views="d4", mode="prob"):
    """Test-time augmentation of ``model`` on ``images`` (N, C, H, W) on the device: the model
    runs once per view at the caller's batch size (its workspace does not grow, and the first
    view of every named set is the plain forward), then the logits are merged.  Returns the dict
    of ``tta_merge`` plus ``logits``, the (K N, C', H, W) per-view logits (``logits[:N]`` is the
    first view's)."""
    m = tta_view_mask(views)
    _tta_mode(mode)
    v = tta_views(images, m)
    N = images.shape[0]
    with torch.no_grad():
        logits = torch.cat([model(v[q * N:(q + 1) * N]).detach().float() for q in range(v.shape[0] // N)])
    out = tta_merge(logits, N, m, mode)
    out["logits"] = logits
    return out


# ---------------------------------------------------------------- threshold sweep
CURVE_FIELDS = ("P", "Nn", "best_k", "TP", "FP", "FN", "auc2")
THRESHOLD_CRITERIA = ("val-dice", "val-image-dice")


def _curve_bins(bins):
    bins = int(bins)
    if not 2 <= bins <= 1024 or bins & (bins - 1):
        raise ValueError(f"bins must be a power of two in 2..1024, got {bins}")
    return bins


def curve_edges(bins=256):
    """The standard edges of the threshold sweep: a float32 CPU tensor of bins - 1 strictly increasing
    logits, e[j] = logit((j + 1) / bins), exactly antisymmetric with e[bins / 2 - 1] == 0
    (unet_curve_edges, a host function).  bins: a power of two in 2..1024."""
    e = torch.empty(_curve_bins(bins) - 1, dtype=torch.float32)
    _cc_host_call("unet_curve_edges", int(bins), e)
    return e


def _curve_planes(x, what):
    """x as a contiguous float32 (planes, hw) view: (planes, hw) as it is, (..., H, W) with every
    leading dimension a plane.  A float32 contiguous view is passed as it is (a 4-byte aligned base
    is legal)."""
    x = x.detach()
    if x.dim() < 2:
        raise ValueError(f"{what} must be (planes, hw) or (..., H, W), got {tuple(x.shape)}")
    if not (x.dtype == torch.float32 and x.is_contiguous()):
        x = x.float().contiguous()
    hw = x.shape[-1] if x.dim() == 2 else x.shape[-1] * x.shape[-2]
    return x.reshape(-1, hw) if hw else x.reshape(0, 0)


def _curve_hist_args(logits, targets, edges, total):
    if targets.shape != logits.shape:
        raise ValueError(f"targets {tuple(targets.shape)} != logits {tuple(logits.shape)}")
    x, t = _curve_planes(logits, "logits"), _curve_planes(targets, "targets")
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"logits hold no pixel: {tuple(logits.shape)}")
    edges = edges.detach().to(device=x.device, dtype=torch.float32).contiguous()
    B = _curve_bins(edges.numel() + 1)
    if total is None:
        total = torch.zeros(2 * B + 1, dtype=torch.int64, device=x.device)
    elif total.dtype != torch.int64 or total.numel() != 2 * B + 1 or total.device != x.device \
            or not total.is_contiguous():
        raise ValueError(f"total must be a contiguous int64 tensor of {2 * B + 1} on {x.device}")
    return x, t, edges, B, total


def curve_hist(logits, targets, edges, total=None):
    """The class-split histogram of the logits on the device and the current stream (no host
    synchronisation).  logits, targets: (planes, hw) or (..., H, W), every leading dimension a
    plane.  With B = len(edges) + 1, a pixel's bin is the number of edges below its logit and its
    class the integer cast of its target (1 positive, 0 negative, anything else ignored).  Returns
    (plane_hist int32 (planes, 2, B), row 0 the negatives and row 1 the positives; total int64
    (2 B + 1): the two rows summed over the planes, then the ignored pixels).  A given ``total`` is
    accumulated into (and returned)."""
    rt = _boundary_runtime(logits, "curve_hist")
    x, t, edges, _, total = _curve_hist_args(logits, targets, edges, total)
    return rt.curve_hist(x, t, edges, total), total


def curve_hist_host(logits, targets, edges, total=None):
    """``curve_hist`` of CPU tensors through the library's host twin."""
    _cc_cpu(logits, "curve_hist_host")
    _cc_cpu(targets, "curve_hist_host")
    x, t, edges, B, total = _curve_hist_args(logits, targets, edges, total)
    ph = torch.empty((x.shape[0], 2, B), dtype=torch.int32)
    _cc_host_call("unet_curve_hist_host", x, t, x.shape[0], x.shape[1], edges, B, ph, total)
    return ph, total


def _curve_stats_args(plane_hist, dice_sum):
    if plane_hist.dim() != 3 or plane_hist.shape[1] != 2 or plane_hist.dtype != torch.int32 or plane_hist.shape[0] < 1:
        raise ValueError(f"plane_hist must be int32 (planes, 2, B), got {plane_hist.dtype} {tuple(plane_hist.shape)}")
    B = _curve_bins(plane_hist.shape[2])
    plane_hist = plane_hist.contiguous()
    if dice_sum is None:
        dice_sum = torch.zeros(B + 1, dtype=torch.float64, device=plane_hist.device)
    elif dice_sum.dtype != torch.float64 or dice_sum.numel() != B + 1 or dice_sum.device != plane_hist.device \
            or not dice_sum.is_contiguous():
        raise ValueError(f"dice_sum must be a contiguous float64 tensor of {B + 1} on {plane_hist.device}")
    return plane_hist, dice_sum


def _curve_stats_dict(out, dice_sum):
    d = {k: out[:, i] for i, k in enumerate(CURVE_FIELDS)}
    d["dice_sum"] = dice_sum
    return d


def curve_stats(plane_hist, dice_sum=None):
    """The per-plane statistics of ``curve_hist``'s plane_hist on the device: a dict of int64
    (planes,) tensors ``P``, ``Nn`` (positives, negatives), ``best_k`` (the operating point of the
    plane's largest Dice; ties: nearest to B / 2, then the smaller), ``TP``, ``FP``, ``FN`` there and
    ``auc2`` (AUROC = auc2 / (2 P Nn)), plus ``dice_sum`` float64 (B + 1): the planes' Dice at every
    operating point k = 0..B, added in ascending plane order to a given ``dice_sum``."""
    rt = _boundary_runtime(plane_hist, "curve_stats")
    plane_hist, dice_sum = _curve_stats_args(plane_hist, dice_sum)
    return _curve_stats_dict(rt.curve_stats(plane_hist, dice_sum), dice_sum)


def curve_stats_host(plane_hist, dice_sum=None):
    """``curve_stats`` of a CPU tensor through the library's host twin."""
    _cc_cpu(plane_hist, "curve_stats_host")
    plane_hist, dice_sum = _curve_stats_args(plane_hist, dice_sum)
    planes, _, B = plane_hist.shape
    out = torch.empty((planes, 8), dtype=torch.int64)
    _cc_host_call("unet_curve_stats_host", plane_hist, planes, B, out, dice_sum)
    return _curve_stats_dict(out, dice_sum)


def curve_best(values):
    """The operating point of the largest of the B + 1 values; ties: the k nearest to B / 2, then the
    smaller k (curve.h's curve_better)."""
    B = len(values) - 1
    return min(range(B + 1), key=lambda k: (-values[k], abs(k - B // 2), k))


def curve_summary(total, dice_sum, n_planes, edges):
    """Read the curves off what one transfer brings back: ``total`` (2 B + 1 Python ints: the
    negatives' and the positives' histogram, the ignored pixels), ``dice_sum`` (B + 1 floats) over
    ``n_planes`` planes, and the B - 1 ``edges``.  Pure Python.  Operating point k in 0..B predicts a
    pixel positive iff its bin is >= k and is reported as the probability k / B.  Returns a dict:
    ``auroc`` (exact from the global histogram, ties counted half; NaN without both classes), ``ap``
    (sum over k ascending of (R_k - R_{k+1}) Prec_k, Prec = 1 where nothing is predicted; NaN without
    positives), ``dice_global`` (B + 1 values) with ``best_global_k`` / ``_threshold`` / ``_dice``,
    ``dice_image`` = dice_sum / n_planes with ``best_image_k`` / ``_threshold`` / ``_dice``, both at
    k = B / 2 (``dice_global_half``, ``dice_image_half``), and ``bins``, ``positives``, ``negatives``,
    ``ignored``, ``planes``."""
    total = [int(v) for v in total]
    dice_sum = [float(v) for v in dice_sum]
    B = _curve_bins(len(edges) + 1)
    if len(total) != 2 * B + 1 or len(dice_sum) != B + 1:
        raise ValueError(f"{B} bins need {2 * B + 1} totals and {B + 1} Dice sums, got {len(total)} and {len(dice_sum)}")
    neg, pos, ignored = total[:B], total[B:2 * B], total[2 * B]
    P, Nn = sum(pos), sum(neg)
    tp, fp = [0] * (B + 1), [0] * (B + 1)
    for b in range(B - 1, -1, -1):
        tp[b], fp[b] = tp[b + 1] + pos[b], fp[b + 1] + neg[b]
    below = auc2 = 0
    for b in range(B):
        auc2 += pos[b] * (2 * below + neg[b])
        below += neg[b]
    nan = float("nan")
    auroc = auc2 / (2 * P * Nn) if P and Nn else nan
    if P:
        prec = [tp[k] / (tp[k] + fp[k]) if tp[k] + fp[k] else 1.0 for k in range(B + 1)]
        ap = sum((tp[k] - tp[k + 1]) / P * prec[k] for k in range(B))
    else:
        ap = nan
    dice_global = [2 * tp[k] / (tp[k] + fp[k] + P) if tp[k] + fp[k] + P else 1.0 for k in range(B + 1)]
    n = int(n_planes)
    dice_image = [v / n if n else nan for v in dice_sum]
    gk = curve_best(dice_global)
    ik = curve_best(dice_image) if n else B // 2
    return dict(bins=B, planes=n, positives=P, negatives=Nn, ignored=ignored, auroc=auroc, ap=ap,
                dice_global=dice_global, best_global_k=gk, best_global_threshold=gk / B,
                best_global_dice=dice_global[gk], dice_global_half=dice_global[B // 2],
                dice_image=dice_image, best_image_k=ik, best_image_threshold=ik / B,
                best_image_dice=dice_image[ik], dice_image_half=dice_image[B // 2])


def parse_threshold(value, bins=256):
    """``config.threshold`` -> (criterion or None, k or None).  0.5 (the default) is (None, None):
    the plain readout.  A float in (0, 1) is snapped to the nearest operating point k / bins with
    1 <= k <= bins - 1; "val-dice" / "val-image-dice" name the criterion the validation split
    decides k by."""
    if value is None:
        return None, None
    if isinstance(value, str) and value in THRESHOLD_CRITERIA:
        return value, None
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if not 0.0 < v < 1.0:
        raise ValueError(f"threshold must be a float in (0, 1) or one of {THRESHOLD_CRITERIA}, got {value!r}")
    if v == 0.5:
        return None, None
    B = _curve_bins(bins)
    return None, min(max(int(v * B + 0.5), 1), B - 1)


def curve_predict(logits, k, edges):
    """The bool mask of operating point k in 0..B: bin(logits) >= k, i.e. logits > edges[k - 1] for
    1 <= k <= B - 1, everything for k = 0 and nothing for k = B."""
    B = edges.numel() + 1
    if k <= 0:
        return torch.ones_like(logits, dtype=torch.bool)
    if k >= B:
        return torch.zeros_like(logits, dtype=torch.bool)
    return logits > edges[k - 1]


# ---------------------------------------------------------------- predict-mode export
EXPORT_KINDS = {"sigmoid": 0, "greater": 1}
OVERLAY_FIELDS = ("area", "contour", "x0", "y0", "x1", "y1")


def resize_f32_plan(in_size, out_size):
    """Pillow's BILINEAR plan of one axis for mode "F" images (unet_resize_f32_plan, a host
    function): float64 coefficients (out, ksize) and int32 bounds (out, 2) = {first, count}."""
    import ctypes

    import numpy as np

    from . import _lib
    lib = _lib.load()
    ks = ctypes.c_int()
    _lib.check(lib.unet_resize_f32_plan(int(in_size), int(out_size), None, None, ctypes.byref(ks)), None,
               "unet_resize_f32_plan")
    k = np.zeros((out_size, ks.value), np.float64)
    b = np.zeros((out_size, 2), np.int32)
    _lib.check(lib.unet_resize_f32_plan(int(in_size), int(out_size), k.ctypes.data, b.ctypes.data,
                                        ctypes.byref(ks)), None, "unet_resize_f32_plan")
    return k, b


@functools.lru_cache(maxsize=64)
def _host_plan(n_in, n_out):
    """(coeffs, bounds, ksize) as CPU tensors for the host twin, a bounded cache per (in, out)."""
    k, b = resize_f32_plan(n_in, n_out)
    return torch.from_numpy(k), torch.from_numpy(b), k.shape[1]


def _export_resize_args(score, size, kind, threshold):
    if score.dim() != 2 or score.shape[0] < 1 or score.shape[1] < 1:
        raise ValueError(f"score must be one (S_h, S_w) plane, got {tuple(score.shape)}")
    if kind not in EXPORT_KINDS:
        raise ValueError(f"kind must be one of {sorted(EXPORT_KINDS)}, got {kind!r}")
    oh, ow = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if oh < 1 or ow < 1:
        raise ValueError(f"size must be positive, got {(oh, ow)}")
    score = score.detach()
    if not (score.dtype == torch.float32 and score.is_contiguous()):
        score = score.float().contiguous()
    return score, oh, ow, EXPORT_KINDS[kind], float(threshold)


def resize_back(score, size, kind="sigmoid", threshold=0.5, return_plane=False):
    """One (S_h, S_w) score plane resized back to ``size`` = (h, w) on the device and the current
    stream, bit for bit ``PIL.Image.fromarray(score, "F").resize((w, h), BILINEAR)``, and
    thresholded there in the same pass: the uint8 {0, 1} mask (h, w), and the float32 plane when
    ``return_plane`` (otherwise it is never written).  The axis plans are cached on the device's
    runtime per (in, out), at most ``UNetRuntime.EXPORT_PLAN_CACHE`` of them.  kind "sigmoid": sigmoid(v) > 0.5 as
    ``Trainer.test`` reads logits (threshold ignored); "greater": v > threshold (a probability plane
    at 0.5, or logits against an edge of ``curve_edges``)."""
    rt = _boundary_runtime(score, "resize_back")
    score, oh, ow, k, thr = _export_resize_args(score, size, kind, threshold)
    h, w = score.shape
    mask, plane = rt.resize_f32_mask(score, oh, ow, rt.export_plan(w, ow), rt.export_plan(h, oh), k, thr,
                                     bool(return_plane))
    return (mask, plane) if return_plane else mask


def resize_back_host(score, size, kind="sigmoid", threshold=0.5, return_plane=False):
    """``resize_back`` of a CPU tensor through the library's host twin."""
    _cc_cpu(score, "resize_back_host")
    score, oh, ow, k, thr = _export_resize_args(score, size, kind, threshold)
    h, w = score.shape
    kh, bh, ksh = _host_plan(w, ow) if w != ow else (None, None, 0)
    kv, bv, ksv = _host_plan(h, oh) if h != oh else (None, None, 0)
    mask = torch.empty((oh, ow), dtype=torch.uint8)
    plane = torch.empty((oh, ow), dtype=torch.float32) if return_plane else None
    _cc_host_call("unet_resize_f32_mask_host", score, h, w, oh, ow, kh, bh, ksh, kv, bv, ksv, k, thr, plane, mask)
    return (mask, plane) if return_plane else mask


def _overlay_args(gray, pred, gt, width, alpha):
    def plane(t, what):
        t = t.detach()
        if t.dtype == torch.bool:
            t = t.to(torch.uint8)
        if t.dtype != torch.uint8 or t.dim() != 2:
            raise ValueError(f"{what} must be an (H, W) uint8 plane, got {t.dtype} {tuple(t.shape)}")
        return t.contiguous()
    gray, pred = plane(gray, "gray"), plane(pred, "pred")
    gt = None if gt is None else plane(gt, "gt")
    if gray.numel() == 0:
        raise ValueError(f"gray holds no pixel: {tuple(gray.shape)}")
    for t, what in ((pred, "pred"), (gt, "gt")):
        if t is not None and (t.shape != gray.shape or t.device != gray.device):
            raise ValueError(f"{what} must be {tuple(gray.shape)} on {gray.device}")
    width, alpha = int(width), int(alpha)
    if not 1 <= width <= 3:
        raise ValueError(f"width must be 1, 2 or 3, got {width}")
    if not 0 <= alpha <= 256:
        raise ValueError(f"alpha must be in 0..256, got {alpha}")
    return gray, pred, gt, width, alpha


def overlay(gray, pred, gt=None, width=1, alpha=0):
    """The contour overlay of one frame on the device: (rgb uint8 (H, W, 3), stats int64 (6,)).
    gray: the (H, W) uint8 frame; pred / gt: (H, W) uint8 or bool masks, nonzero foreground.  The
    inside of pred is tinted red at alpha / 256 (0: none), the contour of gt (when given) is solid
    blue and that of pred solid red on top; a contour of ``width`` in 1..3 holds the foreground
    pixels within that city-block distance of a background pixel or of the frame.  stats =
    {area, contour pixels, x0, y0, x1, y1} of pred, the box inclusive, -1 when pred is empty."""
    rt = _boundary_runtime(gray, "overlay")
    return rt.overlay_u8(*_overlay_args(gray, pred, gt, width, alpha))


def overlay_host(gray, pred, gt=None, width=1, alpha=0):
    """``overlay`` of CPU tensors through the library's host twin."""
    _cc_cpu(gray, "overlay_host")
    gray, pred, gt, width, alpha = _overlay_args(gray, pred, gt, width, alpha)
    h, w = gray.shape
    rgb = torch.empty((h, w, 3), dtype=torch.uint8)
    stats = torch.empty(6, dtype=torch.int64)
    _cc_host_call("unet_overlay_u8_host", gray, pred, gt, h, w, width, alpha, rgb, stats)
    return rgb, stats
