"""One training step of the models/mod.py networks against the fp64 oracle on this path's own
ReLU / max-pool branches (tests/masked.py), at the edges where kernels go wrong: ragged M and W
no multiple of 64 (1x48x80), odd batch with a 2x2 bottleneck (3x32x32 at depth 4), padded
widths (base 24 / 48: padded channels must stay out of every gradient), negative BN gammas,
depth 1, and the bf16 paths (mod (64, 3), (128, 3); ResUNet base 64 -- register-staged level 0
--, base 128 and base 256, the widest documented, at depth 2).  The f32 cases run on the x3 kernels and on the f32-MFMA kernels (x3 = 0).

Compared per case with the fp64 step on the device's branches (bf16: the bf16-operand oracle in
fp64): logits norm-relative; per-tensor norm-relative and max|a - ref| / max|ref| gradient
errors, conv / ConvT weights and every other tensor apart.  The bars are computed here from the
oracle alone (tests/masked.py: f32 4x, x3 = 0 12x the pinned fp32 CPU oracle's own error over
x, x (1 +- 1e-7); bf16 2x the pinned bf16 oracle's fp32-vs-fp64 spread, at most 5e-2) and
recorded with the measured errors in profiles/masked_bars.txt.
"""
import os

import pytest
import torch

import masked as MK
from _helpers import inputs, options

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(autouse=True, scope="module")
def _threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def _case(id, net, math, base, depth, shape, gamma=(0.5, 1.5), seed=7):
    return dict(id=id, net=net, math=math, base=base, depth=depth, shape=shape, gamma=gamma, seed=seed)


F32 = [
    _case("mod64_48x80", "mod", "fp32", 64, 3, (1, 48, 80)),
    _case("res64_48x80", "res", "fp32", 64, 3, (1, 48, 80)),
    _case("mod64_d4_n3", "mod", "fp32", 64, 4, (3, 32, 32)),
    _case("res64_d4_n3", "res", "fp32", 64, 4, (3, 32, 32)),
    _case("mod24", "mod", "fp32", 24, 3, (2, 32, 32)),
    _case("res48", "res", "fp32", 48, 3, (2, 32, 32)),
    _case("mod64_neg_gamma", "mod", "fp32", 64, 3, (2, 32, 32), (-1.0, 1.0), 5),
    _case("res64_neg_gamma", "res", "fp32", 64, 3, (2, 32, 32), (-1.0, 1.0), 5),
    _case("mod64_d1", "mod", "fp32", 64, 1, (2, 32, 32)),
    _case("res64_d1", "res", "fp32", 64, 1, (2, 32, 32)),
]
BF16 = [
    _case("mod64_bf16", "mod", "bf16", 64, 3, (2, 64, 64)),
    _case("mod128_bf16", "mod", "bf16", 128, 3, (2, 64, 64)),
    _case("mod64_bf16_48x80", "mod", "bf16", 64, 3, (1, 48, 80)),
    _case("res64_bf16", "res", "bf16", 64, 3, (2, 64, 64)),
    _case("res128_bf16", "res", "bf16", 128, 3, (2, 64, 64)),
    _case("res256_bf16", "res", "bf16", 256, 2, (2, 32, 32)),
]
_RAN = set()


def _model(c, P):
    import unet_hip
    cls = unet_hip.ModUNet if c["net"] == "mod" else unet_hip.ResUNet
    m = cls(1, 1, base_filters=c["base"], depth=c["depth"], mfma_dtype=c["math"])
    sd = m.state_dict()
    for k, v in list(P.items()) + list(MK.init_buffers(c).items()):
        sd[k] = v.clone()
    m.load_state_dict(sd)
    return m.to(DEV).train()


def _run(c, tag, **opts):
    import unet_hip
    P = MK.make_params(c, c["seed"], c["gamma"])
    x, t = inputs(33, *c["shape"])
    m = _model(c, P)
    with options(m.flatten_().rt, **opts):
        br = MK.device_branches(m, x, c)
        logits = m(x.to(DEV))
        losses = unet_hip.seg_losses(logits, t.to(DEV))
        (losses[0] + losses[1]).backward()
        torch.cuda.synchronize()
    MK.check_on_branches(c, P, x, t, br, logits.detach().cpu().double(), MK.grads_of(m), tag,
                         opts.get("x3", 1))
    _RAN.add(tag)


@pytest.mark.parametrize("x3", [1, 0])
@pytest.mark.parametrize("case", [c["id"] for c in F32])
def test_f32_step_vs_pinned_fp64(case, x3):
    c = {c["id"]: c for c in F32}[case]
    _run(c, f"{case}/x3={x3}", x3=x3)


@pytest.mark.parametrize("case", [c["id"] for c in BF16])
def test_bf16_step_vs_pinned_bf16_oracle(case):
    c = {c["id"]: c for c in BF16}[case]
    _run(c, case)


def test_bars_table_written():
    """profiles/masked_bars.txt: bar and measured error of every pinned check of this session
    (the small cases of tests/test_gpu_kernel_coverage.py too when the whole suite runs)."""
    assert _RAN, "the pinned cases must run before this test (run the whole file)"
    assert MK.write_table() >= len(_RAN)
