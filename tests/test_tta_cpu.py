"""CPU: the host twins unet_tta_views_host / unet_tta_merge_host (csrc/tta.h compiled for the host,
the same source the kernels of csrc/kernels_tta.hip use) against the NumPy definition of
tests/tta_ref.py.  Views, the mode-0 merge and the round trips are compared bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import tta_ref as R

CASES = R.cases()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def t(a):
    return torch.from_numpy(np.array(a, order="C"))  # a copy: the shared inputs are read-only


@pytest.mark.parametrize("case", CASES, ids=R.case_id)
def test_views_are_the_numpy_views(case):
    import unet_hip
    shape, mask = case
    x = R.ramp(shape)
    assert len(np.unique(x)) == x.size
    got = unet_hip.tta_views_host(t(x), mask).numpy()
    want = R.views(x, mask)
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(bits(got), bits(want))
    ks = R.numbers(mask)
    if x[0, 0].size > 1:  # no view is a symmetry of the content: the K views differ pairwise
        n = shape[0]
        for a in range(len(ks)):
            for b in range(a):
                assert not np.array_equal(got[a * n:(a + 1) * n], got[b * n:(b + 1) * n]), (ks[a], ks[b])


@pytest.mark.parametrize("case", CASES, ids=R.case_id)
def test_merge_logit_is_the_definition(case):
    import unet_hip
    shape, mask = case
    K = len(R.numbers(mask))
    logits = R.ramp(shape, K)
    got = unet_hip.tta_merge_host(t(logits), shape[0], mask, "logit")
    score, m, v = R.merge_logit(logits, shape[0], mask)
    assert got["score"].dtype == torch.float32 and got["mask"].dtype == torch.uint8 and got["votes"].dtype == torch.uint8
    assert tuple(got["score"].shape) == tuple(shape)
    assert np.array_equal(bits(got["score"].numpy()), bits(score))
    assert np.array_equal(got["mask"].numpy(), m)
    assert np.array_equal(got["votes"].numpy(), v)
    assert v.max() <= K


def test_named_sets():
    import unet_hip
    from unet_hip import functional as F
    assert F.TTA_SETS == R.SETS
    assert [F.tta_view_numbers(s) for s in ("hflip", "flips", "d4")] == [[0, 1], [0, 1, 2, 3], list(range(8))]
    x = R.ramp((2, 2, 70, 70))
    for name, mask in R.SETS.items():
        assert np.array_equal(bits(unet_hip.tta_views_host(t(x), name).numpy()), bits(R.views(x, mask)))
    assert np.array_equal(unet_hip.tta_views_host(t(x), [6, 1]).numpy(), R.views(x, 0x42))
    with pytest.raises(ValueError):
        unet_hip.tta_views_host(t(x), "d8")
    with pytest.raises(ValueError):
        unet_hip.tta_merge_host(t(x), 2, "hflip", "mean")
    with pytest.raises(ValueError):  # 2 planes are not 2 views of 2 samples
        unet_hip.tta_merge_host(t(x), 2, "hflip")


ROUND_TRIPS = [1 << k for k in range(8)] + [0x03, 0x60, 0x0F, 0x96, 0xFF]  # K = 1, 2, 4, 8


@pytest.mark.parametrize("mask", ROUND_TRIPS, ids=lambda m: f"0x{m:02x}")
def test_round_trip_returns_the_input(mask):
    """merge(views(f)) == f bit for bit: every view is undone by ITS inverse (k = 5 and k = 6 are
    each other's inverses, so swapping them passes every test that only looks at one direction).
    f has 16 significant bits, so the sum of K <= 8 equal values and its division by K, a power
    of two, are exact and the comparison is about the index maps alone."""
    import unet_hip
    K = len(R.numbers(mask))
    assert K in (1, 2, 4, 8)
    shapes = [(2, 2, 70, 70), (1, 1, 64, 64), (1, 1, 1, 1)] + ([(2, 2, 3, 5), (1, 2, 130, 67)] if mask < 16 else [])
    for shape in shapes:
        f = R.short_random(shape, seed=mask)
        stack = unet_hip.tta_views_host(t(f), mask)
        assert np.array_equal(bits(stack.numpy()), bits(R.views(f, mask)))
        got = unet_hip.tta_merge_host(stack, shape[0], mask, "logit")
        assert np.array_equal(bits(got["score"].numpy()), bits(f)), shape
        assert np.array_equal(got["votes"].numpy(), K * R.surf_pred(f).astype(np.uint8))


@pytest.mark.parametrize("case", CASES, ids=R.case_id)
def test_merge_prob_against_float64(case):
    """mode 1: score = (p_0 + ... + p_{K-1}) / K in float32 against the float64 mean.

    The bound, with u = 2^-24 the unit roundoff of float32 and every p_q in (0, 1]:
      * one sigmoid p = fl(1 / fl(1 + e)), e = expf(-x) with a relative error of at most one ulp,
        2u: d sigma / sigma = -(1 - sigma) de / e, so e contributes at most 2u relative, the add
        and the division u each: |p - sigma(x)| <= 4u sigma <= 4u (an overflowing e gives p = 0
        where sigma < 2^-126);
      * the K - 1 adds: the partial sum after adding term m (m = 2..K) is at most m, its rounding
        at most m u: u (K (K + 1) / 2 - 1) in all, on top of the K 4u carried in by the terms;
      * the division by K is exact up to one rounding of a value <= 1: u.
    |score - ref| <= (4 K u + u (K (K + 1) / 2 - 1)) / K + u <= u (5 + (K + 1) / 2): 9.5 u = 5.7e-7
    at K = 8.  tta_ref.prob_bound adds 1 % for the second-order terms (below 1e-13).

    The inputs (tta_ref.prob_inputs: N(0, 3^2), fixed seeds) are asserted, on the reference alone,
    to have no mean probability within that bound of 0.5, so the mask must agree on every pixel."""
    import unet_hip
    shape, mask = case
    K = len(R.numbers(mask))
    logits, ref, ref_mask = R.prob_inputs(shape, mask)  # asserts the margin before the code runs
    got = unet_hip.tta_merge_host(t(logits), shape[0], mask, "prob")
    diff = np.abs(got["score"].numpy().astype(np.float64) - ref).max()
    print(f"{R.case_id(case)}: K {K}, worst |score - float64| {diff:.3e}, bound {R.prob_bound(K):.3e}, "
          f"closest reference to 0.5: {np.abs(ref - 0.5).min():.3e}")
    assert diff <= R.prob_bound(K)
    assert np.array_equal(got["mask"].numpy(), ref_mask)
    assert np.array_equal(got["votes"].numpy(), R.votes(logits, shape[0], mask))


def _raw(name):
    from unet_hip import _lib
    return getattr(_lib.load(), name)


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def test_errors():
    INVALID, SHAPE = -1, -2
    x = np.zeros((8, 1, 4, 6), np.float32)
    out = np.zeros((8, 1, 4, 6), np.float32)
    u8 = np.zeros((1, 1, 4, 6), np.uint8)
    views, merge = _raw("unet_tta_views_host"), _raw("unet_tta_merge_host")
    assert views(_p(x), 1, 1, 4, 6, 0x0F, _p(out)) == 0
    for k in range(4, 8):  # a transposed view of a non-square plane
        assert views(_p(x), 1, 1, 4, 6, 1 << k, _p(out)) == SHAPE
        assert merge(_p(x), 1, 1, 4, 6, 1 << k, 0, _p(out), _p(u8), _p(u8)) == SHAPE
    assert views(_p(x), 1, 1, 4, 6, 0xFF, _p(out)) == SHAPE
    for bad in (0, 0x100, 0x101):
        assert views(_p(x), 1, 1, 4, 6, bad, _p(out)) == INVALID
        assert merge(_p(x), 1, 1, 4, 6, bad, 0, _p(out), _p(u8), _p(u8)) == INVALID
    assert merge(_p(x), 1, 1, 4, 6, 0x03, 0, None, _p(u8), _p(u8)) == INVALID  # null score
    assert merge(None, 1, 1, 4, 6, 0x03, 0, _p(out), _p(u8), _p(u8)) == INVALID
    assert views(_p(x), 1, 1, 4, 6, 0x03, None) == INVALID
    assert merge(_p(x), 1, 1, 4, 6, 0x03, 2, _p(out), _p(u8), _p(u8)) == INVALID  # unknown mode
    assert merge(_p(x), 1, 1, 4, 6, 0x03, 0, _p(x), _p(u8), _p(u8)) == INVALID  # score aliases logits
    assert merge(_p(x), 0, 1, 4, 6, 0x03, 0, _p(out), _p(u8), _p(u8)) == INVALID
    # null mask / votes are fine
    assert merge(_p(x), 1, 1, 4, 6, 0x03, 0, _p(out), None, None) == 0
    import unet_hip
    with pytest.raises(unet_hip.HipError, match="UNET_ERR_SHAPE"):
        unet_hip.tta_views_host(torch.zeros(1, 1, 4, 6), "d4")
