"""CPU: the training augmentations of the device path (csrc/aug.h through the host hooks
unet_augment_u8_host / unet_clahe_u8_host, the source the device kernels share) against Pillow
and the NumPy classes of utils/transforms.py, bit for bit; the split of the transform chain into
a host prefix and recorded device draws; the record's trip through pickling."""
import ctypes
import pickle
import random
import types

import numpy as np
import pytest
from PIL import Image, ImageEnhance

SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (7, 5), (16, 16), (33, 48), (40, 333)]
_rng = random.Random(2024)
ANGLES = [0, 90, 180, 270, -90, -180, 45, -45, 1e-9, -1e-9, 179.999999, 89.9999, 360 - 1e-12, 0.5,
          30] + [_rng.uniform(-180, 180) for _ in range(40)]
CLAHE_SHAPES = [(4, 4), (5, 4), (7, 5), (16, 16), (33, 48), (40, 333)]


def plane(h, w, seed=0):
    return np.random.default_rng(seed + 1000 * h + w).integers(0, 256, (h, w), dtype=np.uint8)


def host(a, rec, is_mask=False):
    from unet_hip.data import apply_augment_host
    return np.asarray(apply_augment_host(a, rec, is_mask))


def record(**kw):
    from unet_hip.data import AugRecord
    return AugRecord(**kw)


@pytest.mark.parametrize("shape", SHAPES)
def test_rotate_bit_equal_to_pillow(shape):
    a = plane(*shape)
    img = Image.fromarray(a, "L")
    for angle in ANGLES:
        want = np.asarray(img.rotate(angle, Image.NEAREST, expand=False, fillcolor=0))
        assert np.array_equal(host(a, record(angle=angle)), want), angle
        # the mask takes the same geometry
        assert np.array_equal(host(a, record(angle=angle, brightness=0.7), is_mask=True), want), angle


def test_rotate_plan_modes():
    from unet_hip import _lib
    from unet_hip.data import rotate_plan
    assert rotate_plan(5, 7, 0.0)[0] == _lib.ROT_NONE
    assert rotate_plan(5, 7, 360.0)[0] == _lib.ROT_NONE
    assert rotate_plan(5, 7, -180)[0] == _lib.ROT_180
    assert rotate_plan(7, 7, 90)[0] == _lib.ROT_90 and rotate_plan(7, 7, -90)[0] == _lib.ROT_270
    mode, a = rotate_plan(5, 7, 90)  # not square: Pillow takes the affine path
    assert mode == _lib.ROT_AFFINE and a[0] == 0 and a[4] == 0 and abs(a[1]) == 65536


@pytest.mark.parametrize("fh", [False, True])
@pytest.mark.parametrize("fv", [False, True])
def test_flip_and_rotate_together(fh, fv):
    a = plane(33, 48, 3)
    img = Image.fromarray(a, "L")
    if fh:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    if fv:
        img = img.transpose(Image.FLIP_TOP_BOTTOM)
    assert np.array_equal(host(a, record(flip_h=fh, flip_v=fv)), np.asarray(img))
    for angle in (0, 180, 30, -45, 179.999999, 90, -117.3):
        want = np.asarray(img.rotate(angle, Image.NEAREST, expand=False, fillcolor=0))
        assert np.array_equal(host(a, record(flip_h=fh, flip_v=fv, angle=angle)), want), angle
    sq = plane(16, 16, 4)
    im = Image.fromarray(sq, "L")
    if fh:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    if fv:
        im = im.transpose(Image.FLIP_TOP_BOTTOM)
    for angle in (90, 270):
        want = np.asarray(im.rotate(angle, Image.NEAREST, expand=False, fillcolor=0))
        assert np.array_equal(host(sq, record(flip_h=fh, flip_v=fv, angle=angle)), want), angle


def test_brightness_bit_equal_to_pillow():
    from unet_hip.data import brightness_lut
    ramp = np.arange(256, dtype=np.uint8)[None, :]
    img = Image.fromarray(ramp, "L")
    r = random.Random(7)
    for f in [0.5, 1.0, 1.5] + [r.uniform(0.5, 1.5) for _ in range(200)]:
        want = np.asarray(ImageEnhance.Brightness(img).enhance(f))
        assert np.array_equal(brightness_lut(f)[None, :], want), f
        assert np.array_equal(host(ramp, record(brightness=f)), want), f
        assert np.array_equal(host(ramp, record(brightness=f), is_mask=True), ramp), f


@pytest.mark.parametrize("shape", [(33, 48), (7, 5), (40, 333)])
def test_tgc_bit_equal_to_numpy_class(shape):
    from utils.transforms import TGCAugment
    a = plane(*shape, seed=5)
    for seed in range(10):
        random.seed(seed)
        want = np.asarray(TGCAugment(p=1.0)(Image.fromarray(a, "L"), None)[0])
        random.seed(seed)
        gains = TGCAugment(p=1.0).draw()
        got = host(a, record(tgc=tuple(gains)))
        assert np.array_equal(got, want), seed
    if shape == (33, 48):  # bin_h = 3: rows 30..32 are past the last whole band
        assert np.array_equal(got[30:], a[30:]) and not np.array_equal(got[:30], a[:30])
    if shape == (7, 5):  # bin_h == 0
        assert np.array_equal(got, a)


@pytest.mark.parametrize("clip", [2.0, 40.0, 0.0])
@pytest.mark.parametrize("shape", CLAHE_SHAPES)
def test_clahe_bit_equal_to_restatement(shape, clip):
    from utils.transforms import clahe_u8
    for seed in (0, 1):
        a = plane(*shape, seed=seed)
        if seed:  # a smooth, low-contrast plane: many bins over the clip limit
            yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
            a = (100 + 20 * np.sin(yy / 5.0) + 10 * np.cos(xx / 7.0) + a % 4).astype(np.uint8)
        assert np.array_equal(host(a, record(clahe=(clip, (4, 4)))), clahe_u8(a, clip, (4, 4)))


def test_clahe_constant_image_and_other_grid():
    from utils.transforms import clahe_u8
    c = np.full((33, 48), 77, np.uint8)
    assert np.array_equal(host(c, record(clahe=(2.0, (4, 4)))), clahe_u8(c, 2.0, (4, 4)))
    a = plane(33, 48, 9)
    assert np.array_equal(host(a, record(clahe=(2.0, (2, 3)))), clahe_u8(a, 2.0, (2, 3)))


FLAG_SETS = [dict(), dict(use_tgc=True, use_clahe=True), dict(use_speckle=True, use_tgc=True)]


@pytest.mark.parametrize("flags", FLAG_SETS, ids=["defaults", "tgc+clahe", "speckle+tgc"])
@pytest.mark.parametrize("shape", [(33, 48), (40, 333)])
def test_whole_chain_matches_host_chain(flags, shape):
    """build_train_transform(device_augment=True) + the host hooks == the host chain +
    DecodeU8, sample by sample, and both leave the RNGs in the same state."""
    from data.data_loader import DecodeU8
    from unet_hip.data import apply_augment_host
    from utils.transforms import RecordAugment, build_train_transform
    cfg = types.SimpleNamespace(**flags)
    host_tf = build_train_transform(cfg, tail=[DecodeU8()])
    dev_tf = build_train_transform(cfg, device_augment=True)
    assert isinstance(dev_tf.transforms[-1], RecordAugment)
    n_host_side = len(dev_tf.transforms) - 1
    assert n_host_side == (4 if flags.get("use_speckle") else 0)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    mask = (((yy - shape[0] / 2) ** 2 + (xx - shape[1] / 3) ** 2) < (min(shape) / 3) ** 2)
    mask = mask.astype(np.uint8) * 255
    seen = set()
    for k in range(32):
        a = plane(*shape, seed=k)
        random.seed(100 + k)
        np.random.seed(100 + k)
        wi, wm = host_tf(Image.fromarray(a, "L"), Image.fromarray(mask, "L"))
        st_host = (random.getstate(), np.random.get_state())
        random.seed(100 + k)
        np.random.seed(100 + k)
        pi, pm = dev_tf(Image.fromarray(a, "L"), Image.fromarray(mask, "L"))
        st_dev = (random.getstate(), np.random.get_state())
        assert pi.aug is pm.aug and pi.aug is not None
        gi = apply_augment_host(pi, pi.aug)
        gm = apply_augment_host(pm, pm.aug, is_mask=True)
        assert np.array_equal(np.asarray(gi), np.asarray(wi)), k
        assert np.array_equal(np.asarray(gm), np.asarray(wm)), k
        assert st_host[0] == st_dev[0], k
        assert all(np.array_equal(x, y) for x, y in zip(st_host[1], st_dev[1])), k
        r = pi.aug
        seen |= {n for n in ("flip_h", "flip_v", "angle", "brightness", "tgc", "clahe")
                 if getattr(r, n) not in (None, False)}
    if flags.get("use_speckle"):  # Flip .. SpeckleNoise stay on the host
        assert seen == {"tgc"}
    else:
        assert seen == {"flip_h", "flip_v", "angle", "brightness"} | \
            ({"tgc", "clahe"} if flags else set())


def test_elastic_stays_on_the_host():
    from utils.transforms import ElasticDeform, RecordAugment, build_train_transform
    tf = build_train_transform(types.SimpleNamespace(use_elastic=True), device_augment=True)
    assert [type(t) for t in tf.transforms] == [ElasticDeform, RecordAugment]
    assert len(tf.transforms[1].transforms) == 3


def test_default_transform_unchanged():
    from utils.transforms import Resize, ToTensor, build_train_transform
    tf = build_train_transform(types.SimpleNamespace())
    assert [type(t).__name__ for t in tf.transforms] == ["Flip", "Rotate", "AdjustBrightness",
                                                         "Resize", "ToTensor"]
    assert isinstance(tf.transforms[-2], Resize) and isinstance(tf.transforms[-1], ToTensor)


def test_record_and_resample_tag_survive_pickling():
    from data.data_loader import DecodeU8, U8Plane, u8_collate
    from unet_hip.data import AugRecord, apply_augment_host
    rec = AugRecord(flip_h=True, angle=12.5, brightness=0.8, tgc=(0.9, 1.1), clahe=(2.0, (4, 4)))
    p = U8Plane.of(plane(7, 5), "nearest")
    p.aug = rec
    q = pickle.loads(pickle.dumps(p))
    assert type(q) is U8Plane and q.resample == "nearest" and q.aug == rec
    assert np.array_equal(q, p)
    plain = pickle.loads(pickle.dumps(U8Plane.of(plane(7, 5), "bilinear")))
    assert plain.resample == "bilinear" and plain.aug is None
    # the tag of a palette plane survives the augmentation and the collate
    pal = Image.fromarray(plane(16, 16), "P")
    pi, pm = DecodeU8()(pal, pal)
    pi.aug = pm.aug = AugRecord(flip_v=True, angle=33.0)
    out = apply_augment_host(pm, pm.aug, is_mask=True)
    assert out.resample == "nearest"
    images, masks = pickle.loads(pickle.dumps(u8_collate([(pi, pm)])))
    assert images[0].aug == pi.aug and masks[0].resample == "nearest"


def _raw_augment(h, w, **fields):
    from unet_hip import _lib
    p = _lib.AugParams()
    for k, v in fields.items():
        setattr(p, k, v)
    src, dst = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    return _lib.load().unet_augment_u8_host(src.ctypes.data, h, w, dst.ctypes.data, ctypes.byref(p))


def _raw_clahe(h, w, gx, gy):
    from unet_hip import _lib
    src, dst = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    return _lib.load().unet_clahe_u8_host(src.ctypes.data, h, w, dst.ctypes.data, 2.0, gx, gy)


def test_refusals():
    UNSUPPORTED, SHAPE, INVALID = -5, -2, -1
    assert _raw_augment(8, 8, num_bins=64) == 0
    assert _raw_augment(8, 8, num_bins=65) == UNSUPPORTED
    assert _raw_augment(8, 9, mode=3) == SHAPE and _raw_augment(8, 8, mode=3) == 0
    assert _raw_augment(8, 8, mode=7) == INVALID
    assert _raw_clahe(64, 64, 16, 16) == 0
    assert _raw_clahe(64, 64, 16, 17) == UNSUPPORTED
    assert _raw_clahe(1, 8, 4, 4) == SHAPE   # 3 rows of padding, nothing to reflect
    assert _raw_clahe(8, 2, 4, 4) == SHAPE   # 2 columns of padding from 2 columns
    assert _raw_clahe(8, 3, 4, 4) == 0       # 1 column of padding from 3
    from unet_hip import _lib
    with pytest.raises(_lib.HipError, match="UNSUPPORTED"):
        host(plane(8, 8), record(tgc=tuple([1.0] * 65)))
