"""The branch-pinned fp64 method of tests/masked.py, checked on the CPU: the hooks reproduce a
run from its own recorded decisions bit for bit, pinning removes the ReLU-flip slack from the
fp32-vs-fp64 spread, and the comparison the GPU tests use fails gradients with one seeded fault
each that the unpinned bars (floor 1e-2; 2x the unpinned bf16 spread) let through.  For the bf16
residual network the faults are those one wrong tile edge produces: a lost K chunk of a weight
gradient, a lost image column, a residual add from the neighbouring row."""
import os

import pytest
import torch

import masked as MK
import res_bf16_ref as RB
from _helpers import inputs, norm_rel
from oracle import mod_ref_cpu as MO
from oracle import unet_ref_cpu as O


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


# ---- the bf16 residual network: faults of the size one wrong tile edge produces.  ResUNet(64, 4)
# at 2x32x64: 2 x 16 x 32 = 1024 pixels at level 1, 2 x 8 x 16 = 256 at level 2.
RESBF = _case("res", "bf16", 64, 4, (2, 32, 64))
CHUNK_CONV = (5, "encoders.2.conv.3.weight")  # MO._conv3 call 2 b + 1 of block b = 2: level 2
COLUMN_SKIP = (7, 0, 5)                       # RB._skip call of block 7 (decoders.2, level 1), sample, column
RESID_BLOCK = ("decoders.2", 256)             # the block whose add is faulted, first row of the group


def _rows(t):
    """NCHW as the [pixels][channels] rows the GEMM kernels walk (n, h, w raster): a view."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


class _DropColumn(torch.autograd.Function):
    """Identity whose backward loses image column `col` of sample `n`."""

    @staticmethod
    def forward(ctx, x, n, col):
        ctx.at = (n, col)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        g = g.clone()
        g[ctx.at[0], :, :, ctx.at[1]] = 0
        return g, None, None


def _seeded_res_bf16(s, fault, monkeypatch):
    """The fp32 bf16-operand oracle's step on s's branches with one fault seeded:
    "chunk": 64 consecutive pixels (one K chunk of the tap-row kernel) left out of the weight-
        gradient sum of CHUNK_CONV, the products on the operands the oracle rounds;
    "column": one image column of one sample zero in the output gradient COLUMN_SKIP's 1x1 GEMM
        reads in backward (both its weight and its input gradient lose it);
    "resid": the residual add of RESID_BLOCK takes the BN output of pixel p + 1 for the 128
        GEMM rows p = first .. first + 127 (the forward value only: the backward of a kernel
        with that fault knows nothing of it)."""
    seen, calls = {}, dict(conv=0, skip=0)
    conv3, skip, bn = MO._conv3, RB._skip, O._bn

    def conv3_(x, w, bf16):
        y = conv3(x, w, bf16)
        if calls["conv"] == CHUNK_CONV[0]:
            seen["x"], seen["shape"] = x.detach(), w.shape
            y.register_hook(lambda g: seen.__setitem__("g", g.detach()))
        calls["conv"] += 1
        return y

    def skip_(x, w, bf16):
        y = skip(x, w, bf16)
        if calls["skip"] == COLUMN_SKIP[0]:
            y = _DropColumn.apply(y, *COLUMN_SKIP[1:])
        calls["skip"] += 1
        return y

    def bn_(x, P, B, name, training):
        y = bn(x, P, B, name, training)
        if name == f"{RESID_BLOCK[0]}.conv.4":
            rows = _rows(y.detach())
            d = torch.zeros_like(rows)
            p0 = RESID_BLOCK[1]
            d[p0:p0 + 128] = rows[p0 + 1:p0 + 129] - rows[p0:p0 + 128]
            N, C, H, W = y.shape
            y = y + d.reshape(N, H, W, C).permute(0, 3, 1, 2)
        return y

    if fault == "chunk":
        monkeypatch.setattr(MO, "_conv3", conv3_)
    elif fault == "column":
        monkeypatch.setattr(RB, "_skip", skip_)
    else:
        monkeypatch.setattr(O, "_bn", bn_)
    r = MK.step(RESBF, s["P"], s["x"], s["t"], False, s["br"])
    monkeypatch.undo()
    if fault == "chunk":
        g = MO._rnd(seen["g"])
        keep = torch.zeros(g.shape[0] * g.shape[2] * g.shape[3], 1)
        keep[128:192] = 1
        N, C, H, W = g.shape
        g = g * keep.reshape(N, H, W, 1).permute(0, 3, 1, 2)
        lost = torch.nn.grad.conv2d_weight(MO._rnd(seen["x"]), seen["shape"], g, padding=1)
        assert float(lost.norm()) > 0
        r["grads"][CHUNK_CONV[1]] = r["grads"][CHUNK_CONV[1]] - lost
    return r


@pytest.mark.parametrize("fault", ["chunk", "column", "resid"])
def test_seeded_res_bf16_tile_edge_fault_fails_the_pinned_bars(fault, monkeypatch):
    """ResUNet(64, 4), bf16 operands, 2x32x64, reference: the pinned fp64 step.  The fp32
    oracle's own result passes masked.check at the bars of masked.bars; the same result with one
    fault of the size a wrong tile edge produces fails it -- a 64-pixel chunk missing from a
    level-2 3x3 weight gradient (of 256 pixels), one image column of one sample missing from a
    level-1 skip GEMM's output gradient (of 64 columns), the residual add of one 128-row group
    taken from the neighbouring pixel (of 1024 rows).  A fault that passed would mean the shape
    is too large for its bars: shrink the shape, the bars are masked.bars' own."""
    s = _shared(RESBF)
    MK.check(s["r32"]["grads"], s["r32"]["logits"], s["r64"], s["bar"], "cpu_res_bf16")
    bad = _seeded_res_bf16(s, fault, monkeypatch)
    with pytest.raises(AssertionError, match="bar"):
        MK.check(bad["grads"], bad["logits"], s["r64"], s["bar"], f"cpu_res_bf16_{fault}")
