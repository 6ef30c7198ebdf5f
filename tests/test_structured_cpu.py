"""tests/structured_inputs.py on the CPU: the families are deterministic and have the structure
they promise; run through the fp32 oracles they deliver the exact-tie windows the GPU tests
(tests/test_gpu_structured.py) require; the checkers accept a faithful CPU emulation of the
device (winners by torch's rule, statistics by the device formula) and reject one planted fault
each."""
import hashlib
import os

import numpy as np
import pytest
import torch

import structured_inputs as S


@pytest.fixture(autouse=True, scope="module")
def _threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


DIGESTS = {
    "margins": "33b1591ef9169123",
    "blocks": "a73c9c27c1d68bbe",
    "ddti_like": "06ef30d9c0c08694",
    "black_sample": "b10a95207028f6f6",
    "offset0.9": "c9b9dc6039e42e29",
}


def _digest(x, t):
    return hashlib.sha256(x.numpy().tobytes() + t.numpy().tobytes()).hexdigest()[:16]


@pytest.mark.parametrize("fam", sorted(DIGESTS))
def test_families_are_deterministic(fam):
    c = S.at_shape(S.SHAPED[1], S.BLACK_SHAPE) if fam == "black_sample" else S.SHAPED[1]
    x, t = S.family(fam, c)
    assert x.dtype == t.dtype == torch.float32 and tuple(x.shape) == (c["shape"][0], 1) + c["shape"][1:]
    assert t.shape == x.shape and set(np.unique(t.numpy())) <= {0.0, 1.0}
    assert _digest(x, t) == _digest(*S.family(fam, c)) == DIGESTS[fam]


def test_margins_structure():
    for c in S.SHAPED:
        N, H, W = c["shape"]
        x = S.family("margins", c)[0].numpy()
        top, bot, left, right = S.margin_box(H, W, c["depth"])
        assert bot % 2 == 1 and right % 2 == 1 and min(H - top - bot, W - left - right) >= 8
        assert not x[:, :, :top].any() and not x[:, :, H - bot:].any()
        assert not x[..., :left].any() and not x[..., W - right:].any()
        inner = x[:, :, top:H - bot, left:W - right]
        assert (inner > 0).all() and inner.max() < 1
    # the full leading margin where the image has room for it
    assert S.margin_box(64, 64, 3) == (44, 3, 44, 5)


def test_blocks_structure():
    x = S.blocks(33, 2, 64, 64)[0].numpy()
    cuts = S.block_cuts(64)
    assert any(c % 2 for c in cuts[1:-1]) and any(c % 2 == 0 for c in cuts[1:-1])
    k = x * 255
    assert np.array_equal(k, np.round(k)) and len(np.unique(k)) > 16
    for i in range(len(cuts) - 1):
        for j in range(len(cuts) - 1):
            blk = x[:, 0, cuts[i]:cuts[i + 1], cuts[j]:cuts[j + 1]]
            assert (blk == blk[:, :1, :1]).all()


def test_ddti_like_structure():
    x = S.ddti_like(33, 2, 64, 64)[0].numpy()
    k = x.astype(np.float64) * 255
    assert np.abs(k - np.round(k)).max() < 1e-4 and np.array_equal(x, (np.round(k) / 255).astype(np.float32))
    assert 0.27 <= (x == 0).mean() <= 0.33 and 0.04 <= (x == 1).mean() <= 0.06
    speckle = x[(x > 0) & (x < 1)]
    assert 0.33 <= speckle.mean() <= 0.37


def test_black_sample_and_offset_structure():
    x, t = S.black_sample(33, 32, 64, 3)
    m = S.margins(33, 2, 32, 64, 3)[0]
    assert x.shape[0] == 3 and not x[1].any() and not t[1].any()
    assert torch.equal(x[0], m[0]) and torch.equal(x[2], m[1])
    for a in (0.0, 0.9, 0.99):
        xo = S.offset(a, 33, 2, 64, 64)[0]
        assert a <= float(xo.min()) and float(xo.max()) <= 1.0


# ------------------------------------------------------------------ the oracles deliver the ties
_TRACES = {}


def _trace(c, fam):
    """(P, x, trace of the fp32 oracle) of case c on family fam, computed once.  Do not modify."""
    key = (c["id"], fam)
    if key not in _TRACES:
        P = S.oracle_of(c)[0](7)
        x, _ = S.family(fam, c)
        _TRACES[key] = (P, x, S.trace_oracle(c, P, x))
    return _TRACES[key]


def _emulated(c, tr, lvl, P):
    """Pooled level lvl of the trace as the device would have it: operands, and winners by torch's
    rule on the float32 values torch pools (after the ReLU where the network has one there)."""
    y4, sc, sh, relu = S.pool_operands(c, tr, lvl, P)
    v = y4.astype(np.float64)
    if sc is not None:
        v = (v * sc.astype(np.float64)[:, None] + sh.astype(np.float64)[:, None]).astype(np.float32)
    return y4, sc, sh, relu, S.torch_winners(np.maximum(v, 0) if relu else v)


TIE_CASES = [(c, fam) for c in S.SHAPED for fam in ("margins", "blocks")] + \
            [(S.at_shape(c, S.BLACK_SHAPE), "black_sample") for c in S.SHAPED]


@pytest.mark.parametrize("c,fam", TIE_CASES, ids=[f"{c['id']}-{f}" for c, f in TIE_CASES])
def test_oracle_delivers_the_tie_windows(c, fam):
    """What tests/test_gpu_structured.py requires of the device's workspace, established on the
    fp32 oracle's own activations: at least 16 four-way exact-tie windows at every pooled level
    that can hold one (`four_way_reachable`) and exactly none at the others, at least 16 two-way windows with first member 1 and
    16 with first member 2 at level 0 of `blocks`; and the checker accepts torch's winners."""
    P, x, tr = _trace(c, fam)
    assert len(tr["pools"]) == c["depth"]
    for lvl in range(c["depth"]):
        n = S.check_winners(*_emulated(c, tr, lvl, P))
        print(f"{c['id']} {fam} level {lvl}: {n}")
        if S.four_way_reachable(c, fam, lvl):
            assert n["four"] >= S.MIN_FOUR, (lvl, n)
        else:   # the receptive-field argument, established: the oracle has not one such window
            assert n["four"] == 0, (lvl, n)
        if fam == "blocks" and lvl == 0:
            assert min(n["first1"], n["first2"]) >= S.MIN_TWO, n


def test_unreachable_levels_are_few_and_only_mod():
    """The waiver of `four_way_reachable` covers the BN -> ReLU network alone: its deepest level
    at 32 rows, and the levels below 0 of `blocks`."""
    off = [(c["id"], fam, lvl) for c, fam in TIE_CASES for lvl in range(c["depth"])
           if not S.four_way_reachable(c, fam, lvl)]
    assert all(i.startswith("mod") for i, _, _ in off)
    assert all(f == "blocks" or (i.endswith("x32x64") and lvl == 2) for i, f, lvl in off), off


# ------------------------------------------------------------------------ winners: planted faults
MOD = S.SHAPED[1]


def test_winner_checker_rejects_last_of_ties():
    """Last instead of first winner among ties: rule (b)."""
    P, x, tr = _trace(MOD, "blocks")
    y4, sc, sh, relu, idx = _emulated(MOD, tr, 0, P)
    v = y4.astype(np.float64) * sc.astype(np.float64)[:, None] + sh.astype(np.float64)[:, None]
    last = (3 - np.argmax(v.astype(np.float32)[..., ::-1], -1)).astype(np.uint8)
    assert (last != idx).sum() >= S.MIN_FOUR
    with pytest.raises(AssertionError, match=r"\(b\)"):
        S.check_winners(y4, sc, sh, relu, last)
    # a two-way tie alone: winner 3 where the pair (1, 3) or (2, 3) ties
    b = y4.view(np.uint32)
    for first in (1, 2):
        two = idx.copy()
        pair = (idx == first) & (b[..., first] == b[..., 3]) & ((b == b[..., first:first + 1]).sum(-1) == 2)
        assert pair.sum() >= S.MIN_TWO
        two[pair] = 3
        with pytest.raises(AssertionError, match=r"\(b\)"):
            S.check_winners(y4, sc, sh, relu, two)


@pytest.mark.parametrize("relu", [0, 1])
def test_winner_checker_rejects_winner_chosen_before_the_affine(relu):
    """Winner chosen on y before an affine with gamma < 0 (the arg max of y is the arg min of v):
    rules (a) / (c); with the ReLU, only live windows count."""
    P, x, tr = _trace(MOD, "margins")
    y4, sc, sh, _, _ = _emulated(MOD, tr, 0, P)
    sc = -sc
    v = (y4.astype(np.float64) * sc.astype(np.float64)[:, None] + sh.astype(np.float64)[:, None]).astype(np.float32)
    S.check_winners(y4, sc, sh, relu, S.torch_winners(np.maximum(v, 0) if relu else v))
    with pytest.raises(AssertionError, match=r"\((a|c)\)"):
        S.check_winners(y4, sc, sh, relu, S.torch_winners(y4))


def test_winner_checker_exempts_dead_windows_from_value_rules_only():
    y4 = np.array([[[-3.0, -1.0, -2.0, -1.0]]], np.float32)      # one channel, one window
    one, zero = np.ones(1, np.float32), np.zeros(1, np.float32)
    S.check_winners(y4, one, zero, 1, np.array([[0]], np.uint8))     # torch: ReLU first, index 0
    S.check_winners(y4, one, zero, 1, np.array([[1]], np.uint8))     # the kernel: max before ReLU
    with pytest.raises(AssertionError, match=r"\(b\)"):
        S.check_winners(y4, one, zero, 1, np.array([[3]], np.uint8))
    with pytest.raises(AssertionError, match=r"\(a\)"):
        S.check_winners(y4, one, zero, 0, np.array([[0]], np.uint8))


# --------------------------------------------------------------------- statistics: planted faults
def _bn_layer(c, fam, i):
    P, x, tr = _trace(c, fam)
    name, z = tr["bn"][i]
    before = (np.zeros(z.shape[1], np.float32), np.ones(z.shape[1], np.float32), 0)
    return S.rows(z), P[name + ".weight"].numpy(), P[name + ".bias"].numpy(), before


def _run_checks(y, gamma, beta, before, mean, invstd, var, n_fin=None, **fin):
    n = y.shape[0]
    var64, bv = S.check_stats(y, n, mean, invstd, 1e-5)
    sc, sh, rm, rv, nbt = S.finalize(mean.astype(np.float64), var, gamma, beta, before, n_fin or n, **fin)
    S.check_affine_and_running(sc, sh, mean, invstd, gamma, beta, before, (rm, rv, nbt), n, var64, bv)
    return sc, sh, rm, rv, nbt, var64, bv


LAYERS = [(c, fam, i) for c in (S.UNET, MOD, S.SHAPED[2]) for fam in ("ddti_like", "offset0.99") for i in (0, 1, 5)]


@pytest.mark.parametrize("c,fam,i", LAYERS, ids=[f"{c['id']}-{f}-bn{i}" for c, f, i in LAYERS])
def test_stat_checkers_accept_the_device_formula(c, fam, i):
    y, gamma, beta, before = _bn_layer(c, fam, i)
    _run_checks(y, gamma, beta, before, *S.device_stats(y))


def test_stat_checkers_accept_a_constant_channel():
    y = np.zeros((256, 4), np.float32)
    y[:, 1] = 0.75
    mean, invstd, var = S.device_stats(y)
    assert var[0] == 0 and invstd[0] == np.float32(1 / np.sqrt(1e-5))
    _run_checks(y, np.ones(4, np.float32), np.zeros(4, np.float32), (np.zeros(4), np.ones(4), 0), mean, invstd, var)


def test_stat_checkers_reject_planted_faults():
    """Level 0 of mod.UNet(64, 3) on the ddti-like image (8192 rows): biased running_var, count
    off by one, a dropped 128-row group, a shift from a mean 4 ulp away, and a counter that stays."""
    y, gamma, beta, before = _bn_layer(MOD, "ddti_like", 1)
    n = y.shape[0]
    mean, invstd, var = S.device_stats(y)
    sc, sh, rm, rv, nbt, var64, bv = _run_checks(y, gamma, beta, before, mean, invstd, var)
    ok = (sc, sh, mean, invstd, gamma, beta, before)

    with pytest.raises(AssertionError, match="running_var"):
        _run_checks(y, gamma, beta, before, mean, invstd, var, unbiased=False)
    with pytest.raises(AssertionError, match="count"):
        S.check_stats(y, n - 1, *S.device_stats(y, count=n - 1)[:2], 1e-5)
    with pytest.raises(AssertionError, match="mean|var"):       # the statistics of n - 1 rows
        S.check_stats(y, n, *S.device_stats(y, count=n - 1)[:2], 1e-5)
    with pytest.raises(AssertionError, match="mean|var"):
        S.check_stats(y, n, *S.device_stats(y, drop=n // 128 - 1)[:2], 1e-5)
    mean4 = mean.astype(np.float64) + 4 * np.spacing(np.abs(mean)).astype(np.float64)
    with pytest.raises(AssertionError, match="shift"):
        S.check_affine_and_running(sc, (beta.astype(np.float64) - mean4 * sc).astype(np.float32), *ok[2:],
                                   (rm, rv, nbt), n, var64, bv)
    with pytest.raises(AssertionError, match="num_batches_tracked"):
        S.check_affine_and_running(*ok, (rm, rv, nbt - 1), n, var64, bv)
    with pytest.raises(AssertionError, match="scale"):
        S.check_affine_and_running(sc * np.float32(1 + 2.0 ** -21), *ok[1:], (rm, rv, nbt), n, var64, bv)
    with pytest.raises(AssertionError, match="running_mean"):
        S.check_affine_and_running(*ok, (rm * np.float32(1 + 2.0 ** -20), rv, nbt), n, var64, bv)
