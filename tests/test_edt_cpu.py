"""CPU: the exact Euclidean distance transform behind BoundaryLoss (csrc/edt.h through the host
hook unet_edt_host, the source the device kernels share) against scipy, bit for bit, and the
CPU behaviour of the public boundary-loss surface."""
import ctypes
import os

import numpy as np
import pytest
import scipy.ndimage as nd
import torch

SHAPES = [(1, 7), (7, 1), (16, 16), (32, 48), (48, 32), (40, 333)]


def edt_host(t):
    from unet_hip import _lib
    t = np.ascontiguousarray(t, np.float32)
    N, C, H, W = t.shape
    out = np.full((N, 1, H, W), -1.0, np.float32)
    rc = _lib.load().unet_edt_host(t.ctypes.data_as(ctypes.c_void_p), N, C, H, W,
                                   out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, rc
    return out


def scipy_dist(t):
    """models/loss.py:55-61 of the reference, cast to float32."""
    g = np.asarray(t).astype(np.uint8)
    return np.stack([nd.distance_transform_edt(1 - g[b, 0]) for b in range(g.shape[0])])[:, None] \
        .astype(np.float32)


def masks(H, W, seed):
    """N = 7: density 0.5, an EMPTY sample, density 0.03, then a single site in each corner."""
    r = np.random.default_rng(seed)
    t = np.zeros((7, 1, H, W), np.float32)
    t[0, 0] = r.random((H, W)) < 0.5
    t[2, 0] = r.random((H, W)) < 0.03
    t[2, 0, r.integers(H), r.integers(W)] = 1  # never empty
    for k, (i, j) in enumerate([(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]):
        t[3 + k, 0, i, j] = 1
    return t


@pytest.mark.parametrize("shape", SHAPES)
def test_edt_host_bit_equal_to_scipy(shape):
    t = masks(*shape, seed=shape[0] * 1000 + shape[1])
    assert not t[1].any() and t[0].any() and t[2].any()
    assert np.array_equal(edt_host(t), scipy_dist(t))


def test_edt_host_512():
    t = masks(512, 512, seed=5)[:4]  # dense, empty, sparse, one corner site (the longest scans)
    assert np.array_equal(edt_host(t), scipy_dist(t))


def test_all_ones_is_all_zero():
    t = np.ones((2, 1, 16, 24), np.float32)
    assert np.array_equal(edt_host(t), np.zeros((2, 1, 16, 24), np.float32))


def test_only_channel_0_is_read():
    r = np.random.default_rng(2)
    t = (r.random((3, 2, 24, 40)) < 0.1).astype(np.float32)
    t[1, 0] = 0  # empty channel 0 next to a busy channel 1
    assert t[1, 1].any()
    assert np.array_equal(edt_host(t), scipy_dist(t))


def test_site_rule_is_the_uint8_cast():
    """A site is (uint8)t == 1: 0.5 and 0.9999999 are not, 1.0 and 1.5 are, 2.0 and 255.0 are not."""
    vals = [0.5, 0.9999999, 1.0, 1.5, 2.0, 255.0]
    assert np.float32(0.9999999) < 1
    for k, v in enumerate(vals):
        t = np.zeros((1, 1, 9, 13), np.float32)
        t[0, 0, 4, 2 * k + 1] = v
        want = scipy_dist(t)
        assert np.array_equal(edt_host(t), want), v
        assert (want[0, 0, 4, 2 * k + 1] == 0) == (v in (1.0, 1.5)), v
    t = np.zeros((1, 1, 9, 13), np.float32)
    for k, v in enumerate(vals):
        t[0, 0, 4, 2 * k + 1] = v
    assert np.array_equal(edt_host(t), scipy_dist(t))


def test_fixture_dist_reproduced(golden_dir):
    z = np.load(os.path.join(golden_dir, "boundary_32.npz"))
    assert z["x"].shape == (3, 1, 32, 48) and not z["t"][1].any()
    assert (z["t"][2] == 1).any() and ((z["t"][2] > 0) & (z["t"][2] < 1)).any()
    assert np.array_equal(edt_host(z["t"]), z["dist"])


def test_size_limit():
    from unet_hip import _lib
    lib = _lib.load()
    t = np.zeros((1, 1, 1, 2049), np.float32)
    out = np.zeros_like(t)
    args = (t.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    assert lib.unet_edt_host(args[0], 1, 1, 1, 2049, args[1]) == -2  # UNET_ERR_SHAPE
    assert lib.unet_edt_host(args[0], 1, 1, 2049, 1, args[1]) == -2
    t = np.zeros((1, 1, 1, 2048), np.float32)
    t[0, 0, 0, 2047] = 1
    assert np.array_equal(edt_host(t), scipy_dist(t))
    # the device entry point refuses the shape before any launch (no device work here)
    from unet_hip.runtime import UNetRuntime
    rt = UNetRuntime("cuda:0")
    d = ctypes.c_void_p(256)
    assert rt.lib.unet_edt(rt.ctx, d, 1, 1, 1, 2049, d, None) == -2
    assert rt.lib.unet_edt(rt.ctx, d, 1, 1, 2049, 8, d, None) == -2


def test_no_cpu_fallback():
    import unet_hip
    x, t = torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8)
    with pytest.raises(unet_hip.HipUnavailable):
        unet_hip.boundary_loss(x, t)
    with pytest.raises(unet_hip.HipUnavailable):
        unet_hip.distance_maps(t)


def test_module_on_cpu_keeps_the_scipy_path(golden_dir):
    from models.loss import BoundaryLoss, _distance_maps
    z = np.load(os.path.join(golden_dir, "boundary_32.npz"))
    x, t = torch.from_numpy(z["x"]).requires_grad_(True), torch.from_numpy(z["t"])
    assert np.array_equal(_distance_maps(t).numpy(), z["dist"])
    loss = BoundaryLoss()(x, t)
    loss.backward()
    assert abs(loss.item() - float(z["loss"])) <= 1e-6 + 1e-5 * abs(float(z["loss"]))
    assert np.allclose(x.grad.numpy(), z["dlogits"], rtol=1e-5, atol=1e-9)
