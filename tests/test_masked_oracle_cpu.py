"""The branch-pinned fp64 method of tests/masked.py, checked on the CPU: the hooks reproduce a
run from its own recorded decisions bit for bit, pinning removes the ReLU-flip slack from the
fp32-vs-fp64 spread, and the comparison the GPU tests use fails gradients with one seeded fault
each that the unpinned bars (floor 1e-2; 2x the unpinned bf16 spread) let through."""
import os

import pytest
import torch

import masked as MK
from _helpers import inputs, norm_rel


@pytest.fixture(autouse=True, scope="module")
def _threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def _case(net, math, base, depth, shape):
    return dict(id=f"{net}{base}d{depth}_{math}", net=net, math=math, base=base, depth=depth, shape=shape)


REPRO = [_case("mod", "fp32", 16, 1, (2, 16, 16)), _case("mod", "fp32", 16, 3, (1, 24, 40)),
         _case("mod", "bf16", 16, 3, (2, 32, 32)), _case("mod", "bf16", 32, 1, (1, 16, 16)),
         _case("res", "fp32", 16, 1, (2, 16, 16)), _case("res", "fp32", 16, 3, (1, 24, 40)),
         _case("res", "bf16", 16, 3, (2, 32, 32)), _case("res", "bf16", 32, 1, (1, 16, 16))]


@pytest.mark.parametrize("c", REPRO, ids=[c["id"] for c in REPRO])
def test_recorded_branches_reproduce_the_run(c):
    """An fp64 step fed the masks and winner indices recorded from itself is the unpinned step
    bit for bit (logits, loss, every gradient), takes 2 (2 depth + 1) ReLU and `depth` pool
    decisions, and consumes all of them."""
    P = MK.make_params(c, 7)
    x, t = inputs(33, *c["shape"])
    rec = ([], [])
    a = MK.step(c, P, x, t, True, record=rec)
    assert (len(rec[0]), len(rec[1])) == MK.n_decisions(c)
    assert all(m.dtype == torch.bool for m in rec[0]) and all(int(i.max()) <= 3 for i in rec[1])
    rec2 = ([], [])
    b = MK.step(c, P, x, t, True, branches=rec, record=rec2)
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["loss"], b["loss"])
    for k, g in a["grads"].items():
        assert torch.equal(g, b["grads"][k]), k
    assert all(torch.equal(p, q) for p, q in zip(rec[0] + rec[1], rec2[0] + rec2[1]))
    with pytest.raises(AssertionError, match="more branch decisions"):
        MK.step(c, P, x, t, True, branches=(rec[0] + rec[0][:1], rec[1]))


def test_hooks_absent_leave_the_oracles_unchanged():
    """Without the arguments the forwards take F.relu / F.max_pool2d themselves: a pinned run on
    masks that differ from its own decisions differs, the unpinned run does not see them."""
    c = _case("res", "fp32", 16, 2, (1, 16, 16))
    P = MK.make_params(c, 7)
    x, t = inputs(33, *c["shape"])
    rec = ([], [])
    a = MK.step(c, P, x, t, True, record=rec)
    flipped = ([~rec[0][0]] + rec[0][1:], rec[1])
    b = MK.step(c, P, x, t, True, branches=flipped)
    assert not torch.equal(a["logits"], b["logits"])
    assert torch.equal(a["logits"], MK.step(c, P, x, t, True)["logits"])


RES = _case("res", "fp32", 64, 3, (2, 64, 64))
BF = _case("mod", "bf16", 64, 3, (2, 64, 64))
_SHARED = {}


def _shared(c):
    """Per case, computed once: parameters, inputs, the unpinned fp64 step with its recorded
    branches, the pinned bars on them and the pinned fp32 oracle's gradients.  Do not modify."""
    if c["id"] not in _SHARED:
        P = MK.make_params(c, 7)
        x, t = inputs(33, *c["shape"])
        rec = ([], [])
        r64 = MK.step(c, P, x, t, True, record=rec)
        _SHARED[c["id"]] = dict(P=P, x=x, t=t, br=rec, r64=r64, bar=MK.bars(c, P, x, t, rec, r64),
                                r32=MK.step(c, P, x, t, False, rec))
    return _SHARED[c["id"]]


def _spread(r, ref):
    return max(norm_rel(g, ref["grads"][k]) for k, g in r["grads"].items())


def test_pinning_removes_the_relu_flip_slack():
    """ResUNet(64, 3) at 2x64x64: the fp32 oracle's worst per-tensor gradient error against the
    fp64 step, pinned to the fp64 run's branches, under x (1 + 1e-7) stays within 2x the
    unperturbed one (unpinned, a perturbation of that size moves a few ReLU inputs across zero
    and the same figure grows by orders of magnitude: printed, the reason the method exists)."""
    s = _shared(RES)
    xp = s["x"] * (1 + 1e-7)
    pinned0 = _spread(s["r32"], s["r64"])
    pinned1 = _spread(MK.step(RES, s["P"], xp, s["t"], False, s["br"]), s["r64"])
    free0 = _spread(MK.step(RES, s["P"], s["x"], s["t"], False), s["r64"])
    free1 = _spread(MK.step(RES, s["P"], xp, s["t"], False), s["r64"])
    print(f"fp32 vs fp64, worst tensor: pinned {pinned0:.2e} / {pinned1:.2e} (x, x (1 + 1e-7)); "
          f"unpinned {free0:.2e} / {free1:.2e}")
    assert pinned1 <= 2 * pinned0
    assert pinned0 <= 1e-4  # two orders below the floor it replaces


def _faulted(grads, fault):
    """A copy of `grads` with one seeded fault in the first 3x3 weight gradient of 64 x 64 (f32)
    or 128 x 128 (bf16) channels; the rolled tap pattern goes into the largest one."""
    g = {k: v.clone() for k, v in grads.items()}
    co = 128 if fault == "channel_zeroed" else 64
    name = next(k for k, v in g.items() if v.dim() == 4 and tuple(v.shape) == (co, co, 3, 3))
    if fault == "tap_shifted":  # (in the bottleneck's 512x512x3x3: 18 wrong elements of 2.4 M)
        name = max((k for k, v in g.items() if v.dim() == 4 and v.shape[-1] == 3), key=lambda k: g[k].numel())
    w = g[name]
    if fault == "element_zeroed":  # the element of median magnitude: a typical one
        flat = w.view(-1)
        flat[flat.abs().argsort()[flat.numel() // 2]] = 0
    elif fault == "tap_shifted":
        w[5, 9] = w[5, 9].reshape(9).roll(1).reshape(3, 3)
    elif fault == "channel_scaled":
        w[11] *= 1.01
    else:
        w[17] = 0
    return g, name


def _old_f32_passes(c, s, grads):
    """The unpinned f32 check of tests/test_gpu_kernel_coverage.py _check_f32."""
    r64 = MK.step(c, s["P"], s["x"], s["t"], True)
    e32 = [max(norm_rel(g, r64["grads"][k]), norm_rel(gp, r64["grads"][k]))
           for (k, g), gp in zip(MK.step(c, s["P"], s["x"], s["t"], False)["grads"].items(),
                                 MK.step(c, s["P"], s["x"] * (1 + 1e-7), s["t"], False)["grads"].values())]
    env = max(2 * max(e32), MK.OLD_FLOOR)
    return max(norm_rel(grads[k], g) for k, g in r64["grads"].items()) <= env


@pytest.mark.parametrize("fault", ["element_zeroed", "tap_shifted", "channel_scaled"])
def test_seeded_f32_fault_fails_the_pinned_bars(fault):
    """ResUNet(64, 3) f32: the fp32 oracle's own gradients pass the comparison the GPU tests use;
    with one element of a 64x64x3x3 weight gradient zeroed, one 3x3 tap pattern rolled by a tap or
    one output channel scaled by 1.01 they fail it -- and pass the unpinned envelope (floor
    1e-2) the small cases had."""
    s = _shared(RES)
    MK.check(s["r32"]["grads"], s["r32"]["logits"], s["r64"], s["bar"], "cpu_res_f32")
    bad, name = _faulted(s["r32"]["grads"], fault)
    with pytest.raises(AssertionError, match="w_"):
        MK.check(bad, s["r32"]["logits"], s["r64"], s["bar"], f"cpu_res_f32_{fault}")
    print(f"{fault} in {name}: norm-rel {norm_rel(bad[name], s['r64']['grads'][name]):.2e}, pinned "
          f"bar {s['bar']['w_norm']:.2e}")
    assert _old_f32_passes(RES, s, bad)


def test_seeded_bf16_fault_fails_the_pinned_bars():
    """mod.UNet(64, 3), bf16 operands: one output channel of a 128x128x3x3 weight gradient zeroed
    (8.8e-2 of its norm) fails the pinned bars (2x the pinned spread, at most 5e-2) and passes the
    envelope the bf16 cases had, 2x the unpinned spread of the bf16 oracle."""
    s = _shared(BF)
    MK.check(s["r32"]["grads"], s["r32"]["logits"], s["r64"], s["bar"], "cpu_mod_bf16")
    bad, name = _faulted(s["r32"]["grads"], "channel_zeroed")
    with pytest.raises(AssertionError, match="w_"):
        MK.check(bad, s["r32"]["logits"], s["r64"], s["bar"], "cpu_mod_bf16_channel_zeroed")
    free32 = MK.step(BF, s["P"], s["x"], s["t"], False)
    old = 2 * _spread(free32, s["r64"])
    bad_free, _ = _faulted(free32["grads"], "channel_zeroed")
    worst = max(norm_rel(bad_free[k], g) for k, g in s["r64"]["grads"].items())
    print(f"channel zeroed in {name}: unpinned error {worst:.2e}, old envelope {old:.2e}, pinned "
          f"bar {s['bar']['w_norm']:.2e}")
    assert worst <= old
