"""CPU: the Lovasz hinge loss without a GPU -- the NumPy restatement (tests/lovasz_ref.py) against
Berman's published formula in float64 torch, the library's host twin (unet_lovasz_host: csrc/lovasz.h,
the device kernels' rules) against the restatement, the key transform, and the wiring that needs no
device (the main.py flag, CompositeLoss's defaults)."""
import ctypes

import numpy as np
import pytest
import torch

import lovasz_ref as R

SHAPES = [(1, 1, 5, 7), (2, 1, 97, 101), (3, 2, 64, 64), (1, 1, 1, 4099)]
EXACT_SHAPES = [(1, 1, 5, 7), (2, 2, 37, 41), (1, 1, 1, 4099)]


def _host(x, t, want_perm=True):
    import unet_hip
    out = unet_hip.lovasz_hinge_host(torch.from_numpy(np.array(x)), torch.from_numpy(np.array(t)), want_perm)
    return {k: (None if v is None else v.numpy()) for k, v in out.items()}


@pytest.mark.parametrize("shape", EXACT_SHAPES)
def test_restatement_is_bermans_formula(shape):
    """Tie-free inputs whose errors are exact in float32 and float64 alike: the restatement's loss
    is the published formula's within the float64 rounding of a sum of M products, M 2^-52 sum
    |terms| (derived, not measured), and so is its gradient -s g / (N C), element by element
    within 4 ulp of float64 (one division, two subtractions, one division by N C)."""
    x, t, ref = R.case(shape, "exact")
    M = shape[2] * shape[3]
    loss, xd = R.berman_torch(x, t)
    loss.backward()
    planes = shape[0] * shape[1]
    bar = R.sum_bar(ref, M) / planes
    print(f"{shape}: loss {loss.item():.17g} vs {ref['sum'] / planes:.17g}, bar {bar:.3e}")
    assert abs(loss.item() - ref["sum"] / planes) <= bar
    # the restatement's float64 gradient, from g in rank order
    g64 = np.zeros((planes, M))
    for p in range(planes):
        g64[p, ref["perm"][p]] = ref["g"][p]
    e = ref["e"].reshape(planes, M)
    s = np.where(np.asarray(t).reshape(planes, M) >= 0.5, 1.0, -1.0)
    want = np.where(e > 0, -s * g64 / planes, 0.0)
    got = xd.grad.numpy().reshape(planes, M)
    assert np.all(np.abs(got - want) <= 4 * 2.0 ** -52 * np.abs(want))
    # and the float32 dlogits is that gradient rounded twice (gmap, then the division)
    d = ref["dlogits"].reshape(planes, M).astype(np.float64)
    assert np.all(np.abs(d - want) <= 2.0 ** -23 * np.abs(want))


@pytest.mark.parametrize("kind", R.KINDS + ("exact",))
@pytest.mark.parametrize("shape", SHAPES)
def test_host_twin_matches_restatement(shape, kind):
    """perm equal exactly, gmap bit-equal, sum within the derived float64 bar."""
    x, t, ref = R.case(shape, kind)
    got = _host(x, t)
    planes, M = shape[0] * shape[1], shape[2] * shape[3]
    assert np.array_equal(got["perm"].reshape(planes, M), ref["perm"])
    assert np.array_equal(got["gmap"].view(np.uint32), ref["gmap"].view(np.uint32))
    if np.isfinite(ref["sum"]):
        assert abs(got["sum"][0] - ref["sum"]) <= R.sum_bar(ref, M), (got["sum"][0], ref["sum"])
        assert abs(float(got["loss"]) - float(ref["loss"])) <= np.spacing(np.float32(abs(ref["loss"])))
    else:  # the inf kind: +inf errors with positive weights
        assert got["sum"][0] == ref["sum"] and float(got["loss"]) == float(ref["loss"])
    # without the permutation output: the same numbers
    again = _host(x, t, want_perm=False)
    assert again["perm"] is None and np.array_equal(again["gmap"].view(np.uint32), got["gmap"].view(np.uint32))
    assert again["sum"][0] == got["sum"][0] or (np.isnan(again["sum"][0]) and np.isnan(got["sum"][0]))


def test_constant_logits_keep_raster_order_within_each_class():
    x, t, ref = R.case((2, 1, 97, 101), "constant")
    perm = _host(x, t)["perm"].reshape(2, -1)
    y = np.asarray(t).reshape(2, -1) >= 0.5
    for p in range(2):
        # x = 0.3: the negatives' e = 1.3 sorts before the positives' 0.7
        want = np.concatenate([np.flatnonzero(~y[p]), np.flatnonzero(y[p])])
        assert np.array_equal(perm[p], want)


def test_nan_logit_gives_nan_loss_and_a_permutation():
    x, t = (a.copy() for a in R.make_case((2, 1, 97, 101), "random"))
    x[1, 0, 40, 50] = np.nan
    got = _host(x, t)
    assert np.isnan(got["sum"][0]) and np.isnan(got["loss"])
    M = 97 * 101
    for p in got["perm"].reshape(2, M):
        assert np.array_equal(np.sort(p), np.arange(M))


def test_soft_targets_binarise_at_one_half():
    x = np.full((1, 1, 1, 4), 0.25, np.float32)
    t = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(0)), 1.0, 0.0], np.float32).reshape(1, 1, 1, 4)
    got = _host(x, t)
    # positives (t >= 0.5): pixels 0 and 2, e = 0.75; negatives: 1 and 3, e = 1.25, first
    assert got["perm"].ravel().tolist() == [1, 3, 0, 2]


def _key(v):
    """csrc/lovasz.h lovasz_key in NumPy: -0 reads as +0; positive floats flip their low 31 bits."""
    v = np.asarray(v, np.float32)
    b = np.where(v == 0, np.uint32(0), v.view(np.uint32))
    return np.where(b & np.uint32(0x80000000), b, b ^ np.uint32(0x7FFFFFFF)).astype(np.uint32)


def _unkey(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k, k ^ np.uint32(0x7FFFFFFF)).astype(np.uint32).view(np.float32)


def test_key_transform_orders_and_round_trips():
    """-inf < ... < -0 = +0 < ... < +inf in e is +inf first in ascending keys; the transform is its
    own inverse on everything but -0.  The host twin sorts by exactly this key: its permutation of
    the ladder is the ladder reversed, the two zeros in raster order."""
    tiny = np.float32(1e-45)
    ladder = np.array([-np.inf, -3.4e38, -2.5, -1.0, -1e-38, -tiny, -0.0, 0.0, tiny, 1e-38, 1.0, 2.5, 3.4e38,
                       np.inf], np.float32)
    k = _key(ladder).astype(np.int64)
    assert k[6] == k[7]
    strict = np.delete(k, 7)
    assert np.all(np.diff(strict) < 0)
    back = _unkey(_key(ladder))
    keep = np.arange(ladder.size) != 6
    assert np.array_equal(back[keep].view(np.uint32), ladder[keep].view(np.uint32))
    assert back[6].view(np.uint32) == 0  # -0 comes back as +0
    r = np.random.default_rng(0).integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    r = r[np.isfinite(r) & (r != 0)]
    assert np.array_equal(_unkey(_key(r)).view(np.uint32), r.view(np.uint32))
    assert np.array_equal(np.argsort(_key(r), kind="stable"), np.argsort(-r, kind="stable"))
    # through the library: negatives (t = 0) with x = e - 1 have e = the ladder value where that is exact
    e = np.array([-np.inf, -2.5, -1.0, -0.0, 0.0, 1.0, 2.5, np.inf], np.float32)
    x = (e - np.float32(1)).reshape(1, 1, 1, -1)
    got = _host(x, np.zeros_like(x))
    assert got["perm"].ravel().tolist() == [7, 6, 5, 3, 4, 2, 1, 0]


def test_refusals_by_shape_alone():
    """H W > 2^24 is UNET_ERR_SHAPE before any access (a 4-float dummy is never read); null
    pointers are UNET_ERR_INVALID."""
    from unet_hip import _lib
    lib = _lib.load()
    a = np.zeros(4, np.float32)
    d = np.zeros(1, np.float64)
    p = lambda v: v.ctypes.data_as(ctypes.c_void_p)
    assert lib.unet_lovasz_host(p(a), p(a), 1, 1, 4097, 4096, p(a), None, p(d), p(a)) == -2
    assert lib.unet_lovasz_host(p(a), p(a), 1, 1, 0, 4, p(a), None, p(d), p(a)) == -2
    assert lib.unet_lovasz_host(None, p(a), 1, 1, 1, 4, p(a), None, p(d), p(a)) == -1
    assert lib.unet_lovasz_host(p(a), p(a), 1, 1, 1, 4, p(a), None, p(d), p(a)) == 0


def test_cpu_tensors_are_refused_by_the_device_entries():
    import unet_hip
    from models.loss import LovaszHingeLoss
    x = torch.zeros(1, 1, 4, 4)
    with pytest.raises(unet_hip.HipUnavailable):
        unet_hip.lovasz_hinge(x, x)
    with pytest.raises(unet_hip.HipUnavailable):
        unet_hip.lovasz_hinge_parts(x, x)
    with pytest.raises(unet_hip.HipUnavailable):
        LovaszHingeLoss()(x, x)


def test_main_flag_and_composite_defaults():
    import inspect

    import main
    from models.loss import CompositeLoss
    assert main.get_parser([]).lovasz_ratio == 0
    assert main.get_parser(["--lovasz_ratio", "0.5"]).lovasz_ratio == 0.5
    c = CompositeLoss()
    assert (c.λ_ft, c.λ_b, c.λ_bce, c.λ_dice, c.λ_lovasz) == (1.0, 0.5, 0.0, 0.0, 0.0)
    assert list(inspect.signature(CompositeLoss.__init__).parameters)[1:5] == ["λ_ft", "λ_b", "λ_bce", "λ_dice"]
