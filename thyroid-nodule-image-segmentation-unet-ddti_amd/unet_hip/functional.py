"""autograd bridges from PyTorch to the native kernels.

* ``UNetFunction``  - forward/backward of the whole encoder-decoder
  (models/model.py:53-73 forward, utils/trainer.py:91 backward).  Gradients land in one
  flat arena laid out like the parameter arena; autograd receives views of it.
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
"""
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
