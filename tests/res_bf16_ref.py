"""bf16 oracle of models/mod.py:ResUNet (helper of the tests, not a test).

Assembled from what oracle/mod_ref_cpu.py exports: every 3x3 conv, every 1x1 skip conv and
every ConvTranspose takes its activation and weight rounded to bf16 (round to nearest even)
and, in backward, its output gradient rounded to bf16 before both the input- and the
weight-gradient products (``_BF16Operands``); sums, BN, ReLU, the residual add, pooling, the
head and the losses stay in the evaluation dtype.  Block 0 (Cin = 1) keeps its first conv and
its skip unrounded, the ``first=True`` rule of ``mod_ref_cpu._block``: the HIP path runs them
in f32 (conv_first_fwd, res_first_fwd, res_first_wgrad).  That is exactly what the HIP bf16
kernels round.  With ``bf16=False`` the forward is ``mod_ref_cpu.make_res_forward`` op for op.
"""
import torch
import torch.nn.functional as F

from oracle import mod_ref_cpu as MO
from oracle import unet_ref_cpu as O


def _skip(x, w, bf16):
    if not bf16:
        return F.conv2d(x, w)
    return MO._BF16Operands.apply(lambda a, b: F.conv2d(a, b), x, w)


def _res_block(x, P, B, prefix, training, bf16=False, first=False):
    y = MO._conv3(x, P[f"{prefix}.conv.0.weight"], bf16 and not first)
    y = MO._relu(O._bn(y, P, B, f"{prefix}.conv.1", training))
    y = MO._conv3(y, P[f"{prefix}.conv.3.weight"], bf16)
    y = O._bn(y, P, B, f"{prefix}.conv.4", training)
    return MO._relu(y + _skip(x, P[f"{prefix}.skip.weight"], bf16 and not first))


def make_res_forward(depth, bf16=False):
    """forward(x, P, B, training) of mod.py:ResUNet with `depth` levels; relu_masks / pool_idx /
    record are the branch hooks of mod_ref_cpu.make_res_forward."""

    def forward(x, P, B, training=True, relu_masks=None, pool_idx=None, record=None):
        return MO.run_with_branches(lambda: _forward(x, P, B, training), relu_masks, pool_idx, record)

    def _forward(x, P, B, training):
        skips = []
        for i in range(depth):
            x = _res_block(x, P, B, f"encoders.{i}", training, bf16, first=(i == 0))
            skips.append(x)
            x = MO._maxpool(x)
        x = _res_block(x, P, B, "bottleneck", training, bf16)
        for j, skip in enumerate(reversed(skips)):
            x = MO._convT(x, P[f"upconvs.{j}.weight"], P[f"upconvs.{j}.bias"], bf16)
            x = torch.cat([skip, x], dim=1)
            x = _res_block(x, P, B, f"decoders.{j}", training, bf16)
        return F.conv2d(x, P["final_conv.weight"], P["final_conv.bias"])

    return forward


def res_train_step(P, B, opt, x, t, depth, bf16=False, relu_masks=None, pool_idx=None, record=None):
    """One trainer step (loss = BCE + Dice) of the residual network; P's dtype is the
    evaluation dtype.  B is updated in place (running statistics)."""
    return O.train_step(P, B, opt, x, t, forward_fn=MO._pinned(make_res_forward(depth, bf16),
                                                               relu_masks, pool_idx, record))


def to64(d):
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in d.items()}


_ORACLES = {}


def oracles(base, depth, size, seed=42, xseed=5, batch=2):
    """(bf16 helper in fp32, bf16 helper in fp64, plain fp32 oracle, buffers after the bf16
    fp32 step) for one configuration, computed once and shared: do not modify."""
    from oracle import weights as Wt
    key = (base, depth, size, seed, xseed, batch)
    if key not in _ORACLES:
        P = MO.res_make_params(seed, base, depth)
        x = torch.from_numpy(Wt.make_input(xseed, batch, 1, size, size))
        t = torch.from_numpy(Wt.make_target(xseed, batch, size, size))
        B32 = MO.res_init_buffers(base, depth)
        r32 = res_train_step(P, B32, None, x, t, depth, bf16=True)
        r64 = res_train_step(to64(P), to64(MO.res_init_buffers(base, depth)), None, x.double(),
                             t.double(), depth, bf16=True)
        plain = MO.res_train_step(P, MO.res_init_buffers(base, depth), None, x, t, depth=depth)
        _ORACLES[key] = (r32, r64, plain, B32, P, x, t)
    return _ORACLES[key]
