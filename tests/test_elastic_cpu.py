"""CPU: ElasticDeform and SpeckleNoise of the device path (csrc/elastic.h and csrc/aug.h through
the host hooks unet_elastic_u8_host / unet_augment_noise_u8_host, the source the device kernels
share) against the NumPy of utils/transforms.py, bit for bit; build_train_transform's
device_augment="all" chain against the host chain, RNG states included; its fallbacks; the
record's trip through pickling; the refusals."""
import ctypes
import pickle
import random
import types

import numpy as np
import pytest
from PIL import Image

SHAPES = [(9, 9), (9, 40), (17, 16), (33, 48), (40, 333)]
INVALID, SHAPE = -1, -2


def plane(h, w, seed=0):
    return np.random.default_rng(seed + 1000 * h + w).integers(0, 256, (h, w), dtype=np.uint8)


def disc(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    m = ((yy - h / 2) ** 2 + (xx - w / 3) ** 2) < (min(h, w) / 3) ** 2
    return m.astype(np.uint8) * 255


def elastic_params(taps, alpha):
    from unet_hip import _lib
    p = _lib.ElasticParams()
    p.ksize, p.alpha = len(taps), alpha
    p.k[:len(taps)] = [float(k) for k in taps]
    return p


def elastic_host(img, mask, rx, ry, p):
    """unet_elastic_u8_host; img or mask may be None.  (status, img_dst, mask_dst)"""
    from unet_hip import _lib
    h, w = rx.shape
    di = None if img is None else np.full_like(img, 7)
    dm = None if mask is None else np.full_like(mask, 7)
    a = [None if v is None else ctypes.c_void_p(v.ctypes.data) for v in (img, mask, di, dm)]
    rc = _lib.load().unet_elastic_u8_host(a[0], a[1], h, w, a[2], a[3], rx.ctypes.data,
                                          ry.ctypes.data, ctypes.byref(p))
    return rc, di, dm


def numpy_elastic(img, mask, rx, ry, sigma, alpha):
    """ElasticDeform.__call__'s arithmetic on given draws."""
    from utils.transforms import gaussian_blur, remap_linear_u8, remap_nearest
    h, w = rx.shape
    dx = gaussian_blur(rx * 2 - 1, 17, sigma) * alpha
    dy = gaussian_blur(ry * 2 - 1, 17, sigma) * alpha
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    map_x = (x + dx).astype(np.float32)
    map_y = (y + dy).astype(np.float32)
    return remap_linear_u8(img, map_x, map_y), remap_nearest(mask, map_x, map_y), map_x, map_y


@pytest.mark.parametrize("shape", SHAPES)
def test_elastic_bit_equal_to_numpy(shape):
    from utils.transforms import gaussian_kernel
    h, w = shape
    rng = np.random.RandomState(h * 1000 + w)
    outside = False
    for k, (sigma, alpha) in enumerate([(s, a) for s in (6, 10) for a in (20, 40, 2000)]):
        img = plane(h, w, k)
        mask = disc(h, w) if k % 2 else plane(h, w, 50 + k)
        rx, ry = rng.rand(h, w), rng.rand(h, w)
        want_i, want_m, map_x, map_y = numpy_elastic(img, mask, rx, ry, sigma, alpha)
        p = elastic_params(gaussian_kernel(17, sigma), float(alpha))
        rc, gi, gm = elastic_host(img, mask, rx, ry, p)
        assert rc == 0
        assert np.array_equal(gi, want_i), (sigma, alpha)
        assert np.array_equal(gm, want_m), (sigma, alpha)
        # each plane alone, the other pointer null
        rc, gi, none = elastic_host(img, None, rx, ry, p)
        assert rc == 0 and none is None and np.array_equal(gi, want_i)
        rc, none, gm = elastic_host(None, mask, rx, ry, p)
        assert rc == 0 and none is None and np.array_equal(gm, want_m)
        if alpha == 2000:  # more than one reflect period (2 n) outside the plane
            outside |= bool((map_x < -2 * w).any() or (map_x > 3 * w).any() or
                            (map_y < -2 * h).any() or (map_y > 3 * h).any())
    assert outside


def test_elastic_hand_made_map_with_ties():
    """ksize 1, tap 1, alpha 1: blur = r * 2 - 1 itself, so the map is chosen freely.  Fields in
    steps of 1/128 put map * 32 on exact .5 ties (rounded to even) and the nearest coordinate on
    .5 as well."""
    from utils.transforms import remap_linear_u8, remap_nearest
    h, w = 12, 20
    img, mask = plane(h, w, 3), disc(h, w)
    yy, xx = np.mgrid[0:h, 0:w]
    dx = ((xx * 7 + yy * 3) % 64 - 32) / 64.0    # multiples of 1/64: ties of map * 32
    dy = ((xx * 5 + yy * 11) % 128 - 64) / 128.0
    dy[::2] = 0.5 * np.sign(dy[::2] + 0.001)     # nearest: y +- 0.5 exactly
    rx, ry = (dx + 1) / 2, (dy + 1) / 2          # exact: r * 2 - 1 == d
    assert np.array_equal(rx * 2 - 1, dx) and np.array_equal(ry * 2 - 1, dy)
    map_x = (xx + dx).astype(np.float32)
    map_y = (yy + dy).astype(np.float32)
    fx = map_x * np.float32(32)
    assert (np.abs(fx - np.floor(fx)) == 0.5).sum() >= 10
    assert (np.abs(map_y - np.floor(map_y)) == 0.5).sum() >= 10
    rc, gi, gm = elastic_host(img, mask, rx, ry, elastic_params([1.0], 1.0))
    assert rc == 0
    assert np.array_equal(gi, remap_linear_u8(img, map_x, map_y))
    assert np.array_equal(gm, remap_nearest(mask, map_x, map_y))


def noise_host(a, p, noise):
    from unet_hip import _lib
    dst = np.full_like(a, 7)
    rc = _lib.load().unet_augment_noise_u8_host(
        a.ctypes.data, a.shape[0], a.shape[1], dst.ctypes.data, ctypes.byref(p),
        None if noise is None else ctypes.c_void_p(noise.ctypes.data))
    assert rc == 0
    return dst


def numpy_speckle(a, noise):
    """SpeckleNoise.__call__'s arithmetic on a given draw."""
    f = a.astype(np.float32) / 255.
    f = f + f * noise
    return np.clip(f * 255., 0, 255).astype(np.uint8)


@pytest.mark.parametrize("shape", [(1, 256), (33, 48), (40, 333)])
def test_speckle_bit_equal_to_numpy(shape):
    from unet_hip.data import AugRecord, apply_augment_host
    h, w = shape
    a = plane(h, w, 2)
    if h == 1:
        a = np.arange(256, dtype=np.uint8)[None, :]  # every value
    rng = np.random.RandomState(h + w)
    for sigma in (0.05, 0.15, 3.0):  # 3.0: many pixels clamp at 0 and at 255
        noise = rng.normal(0, sigma, (h, w))
        noise.flat[0:4] = [-1.0, -2.5, 0.0, 1e-17]
        want = numpy_speckle(a, noise)
        got = np.asarray(apply_augment_host(a, AugRecord(speckle=noise)))
        assert np.array_equal(got, want), sigma
        if sigma == 3.0:
            f = (a.astype(np.float32) / 255.).astype(np.float64)
            raw = (f + f * noise) * 255.
            assert (raw < 0).sum() > 10 and (raw > 255).sum() > 10
    # whole values: (v / 255) * 255 in mixed precision must truncate as NumPy does
    zero = np.zeros((h, w))
    assert np.array_equal(np.asarray(apply_augment_host(a, AugRecord(speckle=zero))),
                          numpy_speckle(a, zero))


def test_speckle_sits_between_brightness_and_tgc():
    """The chain's order: gather, brightness table, speckle at the OUTPUT pixel, TGC."""
    from unet_hip.data import AugRecord, apply_augment_host, brightness_lut
    from utils.transforms import TGCAugment
    a = plane(33, 48, 4)
    noise = np.random.RandomState(1).normal(0, 0.15, a.shape)
    gains = tuple(0.8 + 0.04 * i for i in range(10))
    rec = AugRecord(flip_h=True, angle=180, brightness=1.3, tgc=gains, speckle=noise)
    want = numpy_speckle(brightness_lut(1.3)[a[::-1, ::-1][:, ::-1]], noise)
    f = want.astype(np.float32)
    for i, g in enumerate(gains):
        f[i * 3:(i + 1) * 3] *= g
    want = np.clip(f, 0, 255).astype(np.uint8)
    assert TGCAugment().num_bins == 10
    assert np.array_equal(np.asarray(apply_augment_host(a, rec)), want)
    # the mask takes the geometry only
    assert np.array_equal(np.asarray(apply_augment_host(a, rec, is_mask=True)), a[::-1])


def test_noise_null_equals_plain_augment():
    from unet_hip import _lib
    from unet_hip.data import AugRecord
    a = plane(40, 333, 5)
    rec = AugRecord(flip_v=True, angle=33.3, brightness=0.7, tgc=tuple([1.1] * 10))
    p = rec.params(40, 333, False)
    plain = np.empty_like(a)
    assert _lib.load().unet_augment_u8_host(a.ctypes.data, 40, 333, plain.ctypes.data,
                                            ctypes.byref(p)) == 0
    assert np.array_equal(noise_host(a, p, None), plain)


FLAG_SETS = [dict(use_elastic=True), dict(use_speckle=True),
             dict(use_elastic=True, use_speckle=True, use_tgc=True, use_clahe=True)]
SEED0 = 300


@pytest.mark.parametrize("flags", FLAG_SETS, ids=["elastic", "speckle", "all-four"])
@pytest.mark.parametrize("shape", [(33, 48), (40, 333)])
def test_whole_chain_all_matches_host_chain(flags, shape):
    """build_train_transform(device_augment="all") + the host hooks == the host chain +
    DecodeU8, sample by sample, and both leave the RNGs in the same state."""
    from data.data_loader import DecodeU8
    from unet_hip.data import apply_augment_host
    from utils.transforms import RecordAugment, build_train_transform
    cfg = types.SimpleNamespace(**flags)
    host_tf = build_train_transform(cfg, tail=[DecodeU8()])
    dev_tf = build_train_transform(cfg, device_augment="all")
    assert len(dev_tf.transforms) == 1 and isinstance(dev_tf.transforms[0], RecordAugment)
    assert len(dev_tf.transforms[0].transforms) == len(host_tf.transforms) - 1
    mask = disc(*shape)
    fired = dict(elastic=0, speckle=0)
    for k in range(32):
        a = plane(*shape, seed=k)
        random.seed(SEED0 + k)
        np.random.seed(SEED0 + k)
        wi, wm = host_tf(Image.fromarray(a, "L"), Image.fromarray(mask, "L"))
        st_host = (random.getstate(), np.random.get_state())
        random.seed(SEED0 + k)
        np.random.seed(SEED0 + k)
        pi, pm = dev_tf(Image.fromarray(a, "L"), Image.fromarray(mask, "L"))
        st_dev = (random.getstate(), np.random.get_state())
        assert pi.aug is pm.aug and pi.aug is not None
        assert np.array_equal(np.asarray(pi), a) and np.array_equal(np.asarray(pm), mask)
        gi = apply_augment_host(pi, pi.aug)
        gm = apply_augment_host(pm, pm.aug, is_mask=True)
        assert np.array_equal(np.asarray(gi), np.asarray(wi)), k
        assert np.array_equal(np.asarray(gm), np.asarray(wm)), k
        assert st_host[0] == st_dev[0], k
        assert all(np.array_equal(x, y) for x, y in zip(st_host[1], st_dev[1])), k
        fired["elastic"] += pi.aug.elastic is not None
        fired["speckle"] += pi.aug.speckle is not None
    for name in ("elastic", "speckle"):
        assert fired[name] >= 4 if flags.get("use_" + name) else fired[name] == 0, fired


def _chain_pair(flags, img, mask, seed):
    from data.data_loader import DecodeU8
    from utils.transforms import build_train_transform
    cfg = types.SimpleNamespace(**flags)
    out = []
    for tf in (build_train_transform(cfg, tail=[DecodeU8()]),
               build_train_transform(cfg, device_augment="all")):
        random.seed(seed)
        np.random.seed(seed)
        try:
            pi, pm = tf(img, mask)
        except ValueError:  # ImageEnhance.Brightness refuses a palette image, on either chain
            pi = pm = None
        out.append((pi, pm, random.getstate(), np.random.get_state()))
    return out


@pytest.mark.parametrize("kind", ["palette", "bilevel-mask", "8x40", "40x8"])
def test_fallback_runs_the_host_chain(kind):
    """A pair the device cannot reproduce exactly goes through the host classes: an empty
    record, the host chain's planes (resample tag included) and the host chain's RNG state."""
    from unet_hip.data import AugRecord
    from utils.transforms import ElasticDeform, SpeckleNoise
    flags = FLAG_SETS[2]
    if kind == "palette":
        img = Image.fromarray(plane(33, 48), "P")
        mask = Image.fromarray(disc(33, 48), "P")
    elif kind == "bilevel-mask":
        img = Image.fromarray(plane(33, 48), "L")
        mask = Image.fromarray(disc(33, 48), "L").convert("1")
    else:
        h, w = (8, 40) if kind == "8x40" else (40, 8)
        img, mask = Image.fromarray(plane(h, w), "L"), Image.fromarray(disc(h, w), "L")
    fired = done = 0
    for seed in range(40, 52):
        (wi, wm, wr, wn), (gi, gm, gr, gn) = _chain_pair(flags, img, mask, seed)
        assert wr == gr and all(np.array_equal(x, y) for x, y in zip(wn, gn))
        if wi is None:  # the host chain itself refuses this sample: so does the fallback
            assert kind == "palette" and gi is None
            continue
        done += 1
        assert gi.aug == AugRecord() and gi.aug.elastic is None and gi.aug.speckle is None
        assert np.array_equal(np.asarray(gi), np.asarray(wi))
        assert np.array_equal(np.asarray(gm), np.asarray(wm))
        assert gi.resample == wi.resample and gm.resample == wm.resample
        assert wr == gr and all(np.array_equal(x, y) for x, y in zip(wn, gn))
        random.seed(seed)
        fired += ElasticDeform(p=0.25).draw(2, 2) is not None
    assert fired >= 2 and done >= 4  # the host ElasticDeform did run on some of them
    assert SpeckleNoise(p=1.0).draw((2, 3)).shape == (2, 3)
    # a 9-pixel side is the device's again
    img, mask = Image.fromarray(plane(9, 40), "L"), Image.fromarray(disc(9, 40), "L")
    assert any(_chain_pair(dict(use_elastic=True), img, mask, s)[1][0].aug.elastic is not None
               for s in range(40, 52))


def test_call_and_draw_make_the_same_calls():
    """ElasticDeform / SpeckleNoise.__call__ go through draw(): same values, same RNG state."""
    from utils.transforms import ElasticDeform, SpeckleNoise
    img, mask = Image.fromarray(plane(20, 30), "L"), Image.fromarray(disc(20, 30), "L")
    for seed in range(3):
        for t, args in ((ElasticDeform(p=1.0), (20, 30)), (SpeckleNoise(p=1.0), ((20, 30),))):
            random.seed(seed)
            np.random.seed(seed)
            t(img, mask)
            st = (random.getstate(), np.random.get_state())
            random.seed(seed)
            np.random.seed(seed)
            assert t.draw(*args) is not None
            assert st[0] == random.getstate()
            assert all(np.array_equal(x, y) for x, y in zip(st[1], np.random.get_state()))
    random.seed(0)
    np.random.seed(0)
    st = np.random.get_state()
    assert ElasticDeform(p=0.0).draw(20, 30) is None and SpeckleNoise(p=0.0).draw((20, 30)) is None
    assert all(np.array_equal(x, y) for x, y in zip(st, np.random.get_state()))


def test_record_with_fields_survives_pickle_and_collate():
    from data.data_loader import U8Plane, u8_collate
    from unet_hip.data import AugRecord, apply_augment_host
    from utils.transforms import gaussian_kernel
    rng = np.random.RandomState(0)
    h, w = 12, 17
    rec = AugRecord(flip_h=True, angle=12.5,
                    elastic=(30.0, tuple(gaussian_kernel(17, 8.0)), rng.rand(h, w), rng.rand(h, w)),
                    speckle=rng.normal(0, 0.1, (h, w)))
    assert rec == AugRecord(flip_h=True, angle=12.5)  # == leaves the fields out, and does not raise
    assert rec != AugRecord(flip_h=True)
    assert AugRecord().elastic is None and AugRecord().speckle is None
    pi, pm = U8Plane.of(plane(h, w), "bilinear"), U8Plane.of(disc(h, w), "bilinear")
    pi.aug = pm.aug = rec
    images, masks = pickle.loads(pickle.dumps(u8_collate([(pi, pm)])))
    q = images[0].aug
    assert q == rec and q.elastic[:2] == rec.elastic[:2]
    assert all(np.array_equal(x, y) for x, y in zip(q.elastic[2:], rec.elastic[2:]))
    assert np.array_equal(q.speckle, rec.speckle) and q.speckle.dtype == np.float64
    assert masks[0].aug.elastic is not None
    for is_mask, (got, src) in enumerate(((images[0], pi), (masks[0], pm))):
        assert np.array_equal(np.asarray(apply_augment_host(got, got.aug, bool(is_mask))),
                              np.asarray(apply_augment_host(src, rec, bool(is_mask))))


def test_refusals():
    taps17 = [1.0 / 17] * 17

    def rc(h, w, taps=taps17, alpha=30.0, **kw):
        img = np.zeros((h, w), np.uint8)
        r = np.zeros((h, w))
        return elastic_host(kw.get("img", img), kw.get("mask", img.copy()), r, r,
                            elastic_params(taps, alpha))[0]

    assert rc(9, 9) == 0
    assert rc(16, 16, [1.0 / 16] * 16) == INVALID          # even ksize
    p33 = elastic_params([0.0] * 31, 30.0)
    p33.ksize = 33
    z, r = np.zeros((40, 40), np.uint8), np.zeros((40, 40))
    assert elastic_host(z, z.copy(), r, r, p33)[0] == INVALID
    p33.ksize = 0
    assert elastic_host(z, z.copy(), r, r, p33)[0] == INVALID
    assert rc(40, 40, [1.0 / 31] * 31) == 0
    assert rc(8, 40) == SHAPE and rc(40, 8) == SHAPE        # a side of 8: nothing to reflect
    assert rc(8193, 9) == SHAPE and rc(9, 8193) == SHAPE
    assert rc(9, 9, alpha=float("nan")) == INVALID and rc(9, 9, alpha=float("inf")) == INVALID
    assert rc(9, 9, img=None, mask=None) == INVALID         # no plane at all
    # a destination must differ from its source
    from unet_hip import _lib
    a = np.zeros((9, 9), np.uint8)
    q = ctypes.c_void_p(a.ctypes.data)
    f = np.zeros((9, 9))
    assert _lib.load().unet_elastic_u8_host(q, None, 9, 9, q, None, f.ctypes.data, f.ctypes.data,
                                            ctypes.byref(elastic_params(taps17, 1.0))) == INVALID


def test_modes_of_build_train_transform():
    from utils.transforms import (ALL_DEVICE_AUGMENTS, ElasticDeform, RecordAugment,
                                  build_train_transform)
    every = types.SimpleNamespace(use_elastic=True, use_speckle=True, use_tgc=True, use_clahe=True)
    # device_augment=True keeps its split
    tf = build_train_transform(types.SimpleNamespace(use_elastic=True), device_augment=True)
    assert [type(t) for t in tf.transforms] == [ElasticDeform, RecordAugment]
    tf = build_train_transform(every, device_augment=True)
    assert [type(t).__name__ for t in tf.transforms] == [
        "ElasticDeform", "Flip", "Rotate", "AdjustBrightness", "SpeckleNoise", "RecordAugment"]
    tf = build_train_transform(every, device_augment="all")
    assert [type(t) for t in tf.transforms] == [RecordAugment]
    assert tuple(type(t) for t in tf.transforms[0].transforms) == ALL_DEVICE_AUGMENTS
    with pytest.raises(ValueError):
        build_train_transform(every, tail=[], device_augment="all")
    with pytest.raises(ValueError):  # out of order
        RecordAugment(list(reversed(tf.transforms[0].transforms)), ALL_DEVICE_AUGMENTS)
    with pytest.raises(ValueError):  # not capable without the "all" set
        RecordAugment([ElasticDeform()])


def test_main_parser_flag():
    import main
    args = main.get_parser(["--gpu_augment_all"])
    assert args.gpu_augment_all and not main.get_parser([]).gpu_augment_all
