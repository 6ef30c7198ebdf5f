"""GPU: the context-owned scratch buffers (csrc/runtime_internal.h: Scratch, grow) grow with work
in flight.  Each of the six entry points that own one runs three times on one fresh context and
one non-default stream with no host synchronisation in between: a small shape, a shape whose
scratch need is strictly larger (the buffer is replaced while the first call may still be
running, and the outgrown one must stay allocated), the small shape again.  All three results
must be bit-equal to the host twin of the entry point (the loss has none: to the same call made
alone on a fresh context; tests/test_gpu_loss_edges.py holds its values to the fp64 definition),
and the small result the same before and after the growth."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SMALL, LARGE = (1, 16, 16), (3, 64, 64)  # (N, H, W)


def fresh():
    from unet_hip.runtime import UNetRuntime
    return UNetRuntime(DEV)  # not the cached one: its scratch buffers start empty


def grown(call, cases):
    """[call(rt, *case) for the three cases] as numpy, enqueued back to back on a side stream."""
    rt = fresh()
    ins = [[torch.from_numpy(a).to(DEV) if isinstance(a, np.ndarray) else a for a in c] for c in cases]
    torch.cuda.synchronize()  # the uploads; nothing below waits until all three calls are enqueued
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        outs = [call(rt, *i) for i in ins]
    s.synchronize()
    return [[o.cpu().numpy() for o in out] for out in outs]


def check(call, want, small, large):
    cases = [small, large, small]
    got = grown(call, cases)
    for k, (g, c) in enumerate(zip(got, cases)):
        for a, b in zip(g, want(*c)):
            assert a.dtype == b.dtype and a.shape == b.shape, k
            assert a.tobytes() == b.tobytes(), f"call {k} differs from its reference"
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[0], got[2]))


def vp(a):
    return ctypes.c_void_p(a.ctypes.data)


def host_check(rc, what):
    from unet_hip import _lib
    _lib.check(rc, None, what)


def test_loss_stats():
    # 4 N loss_groups(C H W) partials: 4 at 1 x 16 x 16, 48 at 3 x 128 x 128 (loss_groups = 4)
    def case(n, h, w, seed):
        rng = np.random.default_rng(seed)
        return (rng.standard_normal((n, 1, h, w)).astype(np.float32),
                (rng.random((n, 1, h, w)) < 0.3).astype(np.float32))

    def call(rt, x, t):
        return rt.loss_stats(x, t)

    def alone(x, t):
        rt = fresh()
        out = call(rt, torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV))
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in out]

    check(call, alone, case(1, 16, 16, 0), case(3, 128, 128, 1))


def test_edt():
    def case(shape, seed):
        n, h, w = shape
        return ((np.random.default_rng(seed).random((n, 1, h, w)) < 0.1).astype(np.float32),)

    def host(t):
        from unet_hip import _lib
        n, c, h, w = t.shape
        dist = np.empty((n, 1, h, w), np.float32)
        host_check(_lib.load().unet_edt_host(vp(t), n, c, h, w, vp(dist)), "unet_edt_host")
        return [dist]

    check(lambda rt, t: [rt.edt(t)], host, case(SMALL, 2), case(LARGE, 3))


def test_clahe():
    # gx gy tile histograms and tables: 2 x 2 tiles, then 8 x 8
    def case(h, w, gx, gy, seed):
        return (np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8), 2.0, gx, gy)

    def call(rt, src, clip, gx, gy):
        from unet_hip import _lib
        dst = torch.empty_like(src)
        _lib.check(rt.lib.unet_clahe_u8(rt.ctx, _lib.ptr(src), *src.shape, _lib.ptr(dst), clip, gx, gy,
                                        _lib.stream_ptr(DEV)), rt.ctx, "unet_clahe_u8")
        return [dst]

    def host(src, clip, gx, gy):
        from unet_hip import _lib
        dst = np.empty_like(src)
        host_check(_lib.load().unet_clahe_u8_host(vp(src), *src.shape, vp(dst), clip, gx, gy),
                   "unet_clahe_u8_host")
        return [dst]

    check(call, host, case(16, 16, 2, 2, 4), case(64, 64, 8, 8, 5))


def test_elastic():
    from unet_hip import _lib
    params = _lib.ElasticParams()
    taps = np.exp(-0.5 * (np.arange(17) - 8.0) ** 2 / 36.0)
    params.ksize, params.alpha = 17, 30.0
    params.k[:17] = [float(k) for k in taps / taps.sum()]

    def case(h, w, seed):  # image, mask and the two random fields: 2 h w doubles of scratch
        rng = np.random.default_rng(seed)
        return (rng.integers(0, 256, (h, w), dtype=np.uint8),
                (rng.random((h, w)) < 0.5).astype(np.uint8) * 255, rng.random((h, w)), rng.random((h, w)))

    def call(rt, img, mask, rx, ry):
        di, dm = torch.empty_like(img), torch.empty_like(mask)
        _lib.check(rt.lib.unet_elastic_u8(rt.ctx, _lib.ptr(img), _lib.ptr(mask), *img.shape, _lib.ptr(di),
                                          _lib.ptr(dm), _lib.ptr(rx), _lib.ptr(ry), ctypes.byref(params),
                                          _lib.stream_ptr(DEV)), rt.ctx, "unet_elastic_u8")
        return di, dm

    def host(img, mask, rx, ry):
        di, dm = np.empty_like(img), np.empty_like(mask)
        host_check(_lib.load().unet_elastic_u8_host(vp(img), vp(mask), *img.shape, vp(di), vp(dm), vp(rx),
                                                    vp(ry), ctypes.byref(params)), "unet_elastic_u8_host")
        return di, dm

    check(call, host, case(16, 16, 6), case(64, 64, 7))


def test_surface_stats():
    # Full-width bands: the nearest border pixel of the other mask is always in the same column, so
    # every surface distance is an integer, the float64 sums are exact in any order and the device
    # result is bit-equal to the host twin's raster-order sums (tests/test_gpu_surface.py bounds
    # the order dependence of general masks).
    def case(shape):
        n, h, w = shape
        x = np.full((n, 1, h, w), -1.0, np.float32)
        t = np.zeros((n, 1, h, w), np.float32)
        for i in range(n):
            x[i, 0, h // 8 + i:h // 2 + i] = 1.0
            t[i, 0, h // 3 + 2 * i:3 * h // 4 + i] = 1.0
        return x, t

    def host(x, t):
        from unet_hip import _lib
        n, c, h, w = x.shape
        oi, of = np.empty((n, 6), np.int64), np.empty((n, 2), np.float64)
        host_check(_lib.load().unet_surface_stats_host(vp(x), vp(t), n, c, h, w, vp(oi), vp(of)),
                   "unet_surface_stats_host")
        assert oi[:, 0].all() and (of > 0).all()  # every sample defined, with non-zero distances
        return oi, of

    check(lambda rt, x, t: rt.surface_stats(x, t), host, case(SMALL), case(LARGE))


def test_components():
    def case(shape, seed):
        n, h, w = shape
        return ((np.random.default_rng(seed).random((n, 1, h, w)) < 0.55).astype(np.uint8),)

    def host(m):
        from unet_hip import _lib
        n, c, h, w = m.shape
        labels, count = np.empty((n, h, w), np.int32), np.empty(n, np.int32)
        host_check(_lib.load().unet_components_host(vp(m), 0, n, c, h, w, 1, vp(labels), vp(count)),
                   "unet_components_host")
        return labels, count

    check(lambda rt, m: rt.components(m, 0, 1), host, case(SMALL, 8), case(LARGE, 9))
