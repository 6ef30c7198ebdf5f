"""tests/eval_ref.py itself: the traced eval oracle is the plain oracle, the trained-like buffers
give every eval small case a meaningful input, and the per-layer bars of
tests/test_gpu_eval_coverage.py bite -- an oracle that normalises with batch statistics, or that
takes one 16-pixel row from the neighbouring sample, misses them by orders of magnitude.  No GPU.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import eval_ref as ER
import kernel_cases as KC
from _helpers import inputs, norm_rel, rel_max
from oracle import unet_ref_cpu as O

_CACHE = {}


def _case(cid):
    """(c, P, B, x, fp64 trace) of an eval small case, computed once: do not modify."""
    if cid not in _CACHE:
        c = KC.by_id(KC.SMALL_EVAL)[cid]
        P = ER.fns(c)[0](c["pseed"])
        x, _ = inputs(c["xseed"], *c["shape"])
        B = ER.trained_buffers(c, P, x)
        _CACHE[cid] = (c, P, B, x, ER.eval_trace(c, P, B, x, torch.float64, c["math"] == "bf16"))
    return _CACHE[cid]


@pytest.mark.parametrize("case", [c["id"] for c in KC.SMALL_EVAL])
def test_meaningful_input(case):
    """Parameters seed 7, inputs seed 33 (or the table's), trained_buffers: every BN output
    10 % .. 90 % positive, no stored layer all zero, max|logits| >= 1e-2."""
    c, P, B, x, tr = _case(case)
    assert (c["pseed"], c["xseed"]) == (7, 33) or "seed" in c["note"]
    assert ER.meaningful(tr) == []
    assert len(tr["out"]) == ((2 * c["depth"] + 1) if c["net"] == "res" else 0)


@pytest.mark.parametrize("case,dtype", [("unet_onetap256", torch.float32), ("mod128_onetap256", torch.float64),
                                        ("res48_default", torch.float32), ("mod128_bf16_512x128", torch.float32),
                                        ("res64_bf16_512x128", torch.float64)])
def test_trace_logits_are_the_plain_oracle(case, dtype):
    c, P, B, x, _ = _case(case)
    bf16 = c["math"] == "bf16"
    tr = ER.eval_trace(c, P, B, x, dtype, bf16)
    Pd = {k: v.to(dtype) for k, v in P.items()}
    Bd = {k: v.to(dtype) if v.is_floating_point() else v.clone() for k, v in B.items()}
    with torch.no_grad():
        ref = ER.fns(c, bf16)[2](x.to(dtype), Pd, Bd, False)
    assert torch.equal(tr["logits"], ref)
    for k, v in Bd.items():  # eval touches no buffer
        assert torch.equal(v, B[k].to(dtype) if v.is_floating_point() else B[k])
    # the stored layers are what the next op reads: BN of conv i is its recorded output
    i = 3
    name = ER.bn_names(c)[i]
    y = F.batch_norm(tr["conv"][i], Bd[f"{name}.running_mean"], Bd[f"{name}.running_var"], Pd[f"{name}.weight"],
                     Pd[f"{name}.bias"], False, 0.1, O.BN_EPS)
    assert torch.equal(y, tr["bn"][i])


def test_trained_buffers_are_near_not_equal():
    c, P, B, x, _ = _case("res16_default")
    st = ER.batch_stats(c, P, x)
    for name in ER.bn_names(c):
        m, v = (a.numpy() for a in st[name])
        rm, rv = B[f"{name}.running_mean"].numpy(), B[f"{name}.running_var"].numpy()
        assert rm.dtype == np.float32 and rv.dtype == np.float32
        d = np.abs(rm - m) / np.sqrt(v)
        assert d.max() <= 0.25 * (1 + 1e-6) and np.median(d) > 0.05
        r = np.log2(rv / v)
        assert np.abs(r).max() <= 1 + 1e-6 and np.median(np.abs(r)) > 0.2
    # deterministic
    B2 = ER.trained_buffers(c, P, x)
    assert all(torch.equal(B[k], B2[k]) for k in B)


def _f32_bars(c, P, B, x, tr64, factor=4.0):
    """{layer: (rel_max bar, norm_rel bar)}: factor x the fp32 CPU oracle's worst deviation from
    the fp64 trace over x, x (1 +- 1e-7) -- the rule of tests/test_gpu_eval_coverage.py."""
    bars = {}
    for eps in (0.0, 1e-7, -1e-7):
        tr = ER.eval_trace(c, P, B, x * (1 + eps) if eps else x, torch.float32)
        for (tag, a), (_, r) in zip(ER.layers(tr), ER.layers(tr64)):
            e = (rel_max(a, r), norm_rel(a, r))
            bars[tag] = tuple(max(p, factor * q) for p, q in zip(bars.get(tag, (0, 0)), e))
    return bars


def _worst_miss(tr, tr64, bars, tags=None):
    worst = (0.0, "")
    for (tag, a), (_, r) in zip(ER.layers(tr), ER.layers(tr64)):
        if tags is None or tag in tags:
            k = max(rel_max(a, r) / bars[tag][0], norm_rel(a, r) / bars[tag][1])
            worst = max(worst, (k, tag))
    return worst


def test_mutation_batch_statistics_miss_the_bars():
    """The fp64 oracle with batch statistics in place of the running ones, on the trained_buffers
    inputs, against the per-layer bars (4x the fp32 oracle's deviation): conv0 is untouched (no
    BN ahead of it), every later layer misses, the worst by >= 1e4 x its bar."""
    c, P, B, x, tr64 = _case("mod128_halo256_n3")

    def batch_bn(z, P_, B_, name):
        return F.batch_norm(z, None, None, P_[f"{name}.weight"], P_[f"{name}.bias"], True, 0.1, O.BN_EPS)

    mut = ER.eval_trace(c, P, B, x, torch.float64, bn_hook=batch_bn)
    bars = _f32_bars(c, P, B, x, tr64)
    assert _worst_miss(mut, tr64, bars, {"conv0"})[0] == 0.0
    later = [t for t, _ in ER.layers(tr64) if t != "conv0"]
    least = min(_worst_miss(mut, tr64, bars, {t}) for t in later)
    worst = _worst_miss(mut, tr64, bars)
    print(f"batch statistics: least miss {least[0]:.1e}x ({least[1]}), worst {worst[0]:.1e}x ({worst[1]})")
    assert least[0] >= 1e3 and worst[0] >= 1e4


def test_mutation_row_from_the_neighbouring_sample_misses_the_bars():
    """One 16-pixel row of a level-2 conv output (conv 4 of mod128_halo256_n3: 3 samples of 8 x 32
    pixels) taken from the neighbouring sample, as a halo tile reading across a sample border
    would leave it: that layer misses its bar, and so do the logits."""
    c, P, B, x, tr64 = _case("mod128_halo256_n3")

    def swap(i, z):
        if i != 4:
            return z
        z = z.clone()
        z[1, :, 0, :16] = z[0, :, 0, :16]
        return z

    mut = ER.eval_trace(c, P, B, x, torch.float64, conv_hook=swap)
    bars = _f32_bars(c, P, B, x, tr64)
    assert _worst_miss(mut, tr64, bars, {f"conv{i}" for i in range(4)})[0] == 0.0
    at, logit = _worst_miss(mut, tr64, bars, {"conv4"}), _worst_miss(mut, tr64, bars, {"logits"})
    print(f"neighbour's row: conv4 {at[0]:.1e}x its bar, logits {logit[0]:.1e}x")
    assert at[0] >= 1e4 and logit[0] >= 1e2


@pytest.mark.parametrize("case", [c["id"] for c in ER.EDGE_CASES])
def test_planted_buffers_keep_the_network_in_range(case):
    """The planted edge channels (var 0 / 1e-12 / 1e6, mean +-1e4, gamma 0 / < 0, beta +-10) in
    every BN layer: fp64 and fp32 eval traces finite, float32 affine inside `affine_bounds` when
    evaluated as the kernel does (the bound accepts a faithful emulation and refuses a scale
    formed from var without eps)."""
    c = next(c for c in ER.EDGE_CASES if c["id"] == case)
    P = ER.plant_params(c, ER.fns(c)[0](7))
    x, _ = inputs(33, *c["shape"])
    B = ER.planted_buffers(c, P, x)
    for dt in (torch.float64, torch.float32):
        tr = ER.eval_trace(c, P, B, x, dt, c["math"] == "bf16")
        assert all(np.isfinite(r).all() for _, r in ER.layers(tr))
    f32 = np.float32
    for name in ER.bn_names(c):
        g, b = P[f"{name}.weight"].numpy(), P[f"{name}.bias"].numpy()
        m, v = B[f"{name}.running_mean"].numpy(), B[f"{name}.running_var"].numpy()
        assert v[ER.PLANTED["var=0"]] == 0 and m[ER.PLANTED["mean=-1e4"]] == -1e4 and g[ER.PLANTED["gamma=0"]] == 0
        sc = g * (f32(1) / np.sqrt(v + ER.BN_EPS32))
        ER.check_affine(sc, b - m * sc, g, b, m, v, name)
        fused = (b.astype(np.float64) - m.astype(np.float64) * sc.astype(np.float64)).astype(f32)
        ER.check_affine(sc, fused, g, b, m, v, name)
        with pytest.raises(AssertionError):
            ER.check_affine(sc * f32(1 + 2e-6), b - m * sc, g, b, m, v, name)
        with pytest.raises(AssertionError):
            ER.check_affine(sc, (b - m * sc) * f32(1 + 4e-6) + f32(1e-5), g, b, m, v, name)
