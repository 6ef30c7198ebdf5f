"""Device-side ElasticDeform and SpeckleNoise (unet_elastic_u8 / unet_augment_noise_u8 through
unet_hip.GpuResizeToTensor) against the host hooks of the same source (which
tests/test_elastic_cpu.py pins to the NumPy classes), and the pipeline, the loader and main.py in
device_augment="all" mode against the host transform chain.  Bit-equal everywhere."""
import os
import random
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(9, 9), (9, 40), (17, 16), (33, 48), (40, 333)]
EVERY = dict(use_elastic=True, use_speckle=True, use_tgc=True, use_clahe=True)


def plane(h, w, seed=0):
    return np.random.default_rng(seed + 1000 * h + w).integers(0, 256, (h, w), dtype=np.uint8)


def disc(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    m = ((yy - h / 2) ** 2 + (xx - w / 3) ** 2) < (min(h, w) / 3) ** 2
    return m.astype(np.uint8) * 255


@pytest.fixture(scope="module")
def pipe():
    import unet_hip
    return unet_hip.GpuResizeToTensor((32, 32), device="cuda:0")


def host(a, rec, is_mask=False):
    from unet_hip.data import apply_augment_host
    return np.asarray(apply_augment_host(a, rec, is_mask))


def elastic_record(h, w, sigma, alpha, rng, ksize=17):
    from unet_hip.data import AugRecord
    from utils.transforms import gaussian_kernel
    return AugRecord(elastic=(float(alpha), tuple(gaussian_kernel(ksize, sigma)), rng.rand(h, w),
                              rng.rand(h, w)))


def check_elastic(pipe, img, mask, rec):
    """The pair in one call, and each plane alone (the other pointer null), against the hook."""
    ti, tm = torch.from_numpy(img).to(pipe.device), torch.from_numpy(mask).to(pipe.device)
    want_i, want_m = host(img, rec), host(mask, rec, True)
    di, dm = pipe.elastic(ti, tm, rec)
    assert np.array_equal(di.cpu().numpy(), want_i) and np.array_equal(dm.cpu().numpy(), want_m)
    di, none = pipe.elastic(ti, None, rec)
    assert none is None and np.array_equal(di.cpu().numpy(), want_i)
    none, dm = pipe.elastic(None, tm, rec)
    assert none is None and np.array_equal(dm.cpu().numpy(), want_m)
    assert np.array_equal(pipe.augment(ti, rec, False).cpu().numpy(), want_i)
    assert np.array_equal(pipe.augment(tm, rec, True).cpu().numpy(), want_m)


@pytest.mark.parametrize("shape", SHAPES)
def test_elastic_kernels_match_host_hook(pipe, shape):
    h, w = shape
    rng = np.random.RandomState(h * 1000 + w)
    for k, (sigma, alpha) in enumerate([(s, a) for s in (6, 10) for a in (20, 40, 2000)]):
        mask = disc(h, w) if k % 2 else plane(h, w, 50 + k)
        check_elastic(pipe, plane(h, w, k), mask, elastic_record(h, w, sigma, alpha, rng))


def test_elastic_one_large_plane_crosses_many_blocks(pipe):
    """360 x 560: three LDS segments per row (the last one partial), 788 remap blocks."""
    h, w = 360, 560
    rng = np.random.RandomState(1)
    check_elastic(pipe, plane(h, w, 1), disc(h, w), elastic_record(h, w, 8.0, 30.0, rng))


def test_elastic_other_window_sizes(pipe):
    rng = np.random.RandomState(2)
    for ksize, shape in ((1, (5, 7)), (3, (2, 300)), (31, (16, 16)), (31, (40, 333))):
        rec = elastic_record(*shape, 5.0, 25.0, rng, ksize)
        check_elastic(pipe, plane(*shape, 3), disc(*shape), rec)


@pytest.mark.parametrize("shape", [(1, 256)] + SHAPES + [(360, 560)])
def test_noise_kernel_matches_host_hook(pipe, shape):
    from unet_hip.data import AugRecord
    h, w = shape
    a = np.arange(256, dtype=np.uint8)[None, :] if h == 1 else plane(h, w, 2)
    t = torch.from_numpy(a).to(pipe.device)
    rng = np.random.RandomState(h + w)
    for k, sigma in enumerate((0.05, 0.15, 3.0)):  # 3.0: many pixels clamp at 0 and at 255
        noise = rng.normal(0, sigma, (h, w))
        noise.flat[0:4] = [-1.0, -2.5, 0.0, 1e-17]
        rec = AugRecord(speckle=noise)
        assert np.array_equal(pipe.augment(t, rec, False).cpu().numpy(), host(a, rec)), sigma
        if h > 1:
            rec = AugRecord(flip_h=bool(k % 2), angle=33.3 * k, brightness=0.7 + 0.3 * k,
                            tgc=tuple(0.8 + 0.04 * i for i in range(10)), speckle=noise)
            assert np.array_equal(pipe.augment(t, rec, False).cpu().numpy(), host(a, rec)), sigma
            # the mask takes the geometry only
            assert np.array_equal(pipe.augment(t, rec, True).cpu().numpy(), host(a, rec, True))


def test_noise_null_is_the_plain_kernel(pipe):
    import ctypes
    from unet_hip import _lib
    from unet_hip.data import AugRecord
    a = plane(40, 333, 5)
    rec = AugRecord(flip_v=True, angle=33.3, brightness=0.7, tgc=tuple([1.1] * 10))
    t = torch.from_numpy(a).to(pipe.device)
    d = torch.empty_like(t)
    _lib.check(pipe.rt.lib.unet_augment_noise_u8(
        pipe.rt.ctx, _lib.ptr(t), 40, 333, _lib.ptr(d), ctypes.byref(rec.params(40, 333, False)),
        None, _lib.stream_ptr(pipe.device)), pipe.rt.ctx, "unet_augment_noise_u8")
    assert torch.equal(d, pipe.augment(t, rec, False))


def test_refusals_on_the_device_entry(pipe):
    from unet_hip import _lib
    rng = np.random.RandomState(0)
    t = torch.zeros((8, 40), dtype=torch.uint8, device=pipe.device)
    with pytest.raises(_lib.HipError, match="UNET_ERR_SHAPE"):
        pipe.elastic(t, None, elastic_record(8, 40, 8.0, 30.0, rng))
    t = torch.zeros((20, 20), dtype=torch.uint8, device=pipe.device)
    with pytest.raises(_lib.HipError, match="UNET_ERR_INVALID"):
        pipe.elastic(t, None, elastic_record(20, 20, 8.0, 30.0, rng, ksize=16))


def _samples(n):
    """n seeded (image, mask) PIL pairs of mixed sizes."""
    from PIL import Image
    sizes = [(33, 48), (40, 333), (64, 64), (100, 37), (57, 80), (48, 33), (90, 90), (36, 56)]
    out = []
    for k in range(n):
        h, w = sizes[k % len(sizes)]
        out.append((Image.fromarray(plane(h, w, k), "L"), Image.fromarray(disc(h, w), "L")))
    return out


def test_pipeline_all_matches_host_chain(pipe):
    """GpuResizeToTensor(images, masks, aug=records) == host chain + Resize + ToTensor, with
    every augmentation of the chain on the device."""
    from utils.transforms import build_train_transform
    cfg = types.SimpleNamespace(**EVERY)
    host_tf = build_train_transform(cfg, (32, 32))
    dev_tf = build_train_transform(cfg, device_augment="all")
    want_x, want_t, images, masks = [], [], [], []
    for k, (img, m) in enumerate(_samples(16)):
        random.seed(700 + k)
        np.random.seed(700 + k)
        x, t = host_tf(img, m)
        want_x.append(x)
        want_t.append(t)
        random.seed(700 + k)
        np.random.seed(700 + k)
        pi, pm = dev_tf(img, m)
        images.append(pi)
        masks.append(pm)
    records = [p.aug for p in images]
    assert sum(r.elastic is not None for r in records) >= 2
    assert sum(r.speckle is not None for r in records) >= 2
    assert any(r.elastic is not None and r.speckle is not None for r in records)
    assert any(r.clahe for r in records) and any(r.tgc for r in records)
    x, t = pipe(images, masks, aug=records)
    assert torch.equal(x.cpu(), torch.stack(want_x)) and torch.equal(t.cpu(), torch.stack(want_t))
    # images alone: the elastic call with a null mask
    assert torch.equal(pipe(images, aug=records), x)


def _jpeg_dir(root, n=6):
    os.makedirs(root / "train")
    os.makedirs(root / "train_mask")
    for k, (img, m) in enumerate(_samples(n)):
        img.save(root / "train" / f"{k}.jpg")
        m.save(root / "train_mask" / f"{k}_mask.jpg")
    return str(root / "train"), str(root / "train_mask")


@pytest.mark.parametrize("workers", [0, 2])
def test_device_loader_all_matches_host_chain_loader(tmp_path, workers):
    """DeviceResizeLoader over the all-recording transform == the host-chain DataLoader, batch by
    batch, under the same seed: the fields cross the worker pickle with the planes."""
    from data.data_loader import DeviceResizeLoader, MedicalDataset, u8_collate
    from utils.transforms import build_train_transform
    d, md = _jpeg_dir(tmp_path, 12)
    cfg = types.SimpleNamespace(**EVERY)
    fired = []

    def batches(device_side):
        random.seed(13)
        np.random.seed(13)
        g = torch.Generator().manual_seed(13)
        if device_side:
            ds = MedicalDataset(d, md, build_train_transform(cfg, device_augment="all"))
            dl = torch.utils.data.DataLoader(ds, batch_size=4, num_workers=workers,
                                             collate_fn=u8_collate, generator=g)
            fired.extend((im.aug.elastic is not None, im.aug.speckle is not None)
                         for images, _ in dl for im in images)
            random.seed(13)
            np.random.seed(13)
            g.manual_seed(13)
            dl = DeviceResizeLoader(dl, (32, 32), "cuda:0")
        else:
            ds = MedicalDataset(d, md, build_train_transform(cfg, (32, 32)))
            dl = torch.utils.data.DataLoader(ds, batch_size=4, num_workers=workers, generator=g)
        return [(x.cpu(), t.cpu()) for x, t in dl]

    want, got = batches(False), batches(True)
    assert len(want) == len(got) == 3
    for (wx, wt), (gx, gt) in zip(want, got):
        assert torch.equal(wx, gx) and torch.equal(wt, gt)
    assert any(e for e, _ in fired) and any(s for _, s in fired)


def test_main_cli_gpu_augment_all(tmp_path, monkeypatch):
    import main
    for split in ("train", "val", "test"):
        os.makedirs(tmp_path / "ddti" / split)
        os.makedirs(tmp_path / "ddti" / (split + "_mask"))
        for k, (img, m) in enumerate(_samples(4)):
            img.save(tmp_path / "ddti" / split / f"{k}.jpg")
            m.save(tmp_path / "ddti" / (split + "_mask") / f"{k}_mask.jpg")
    monkeypatch.chdir(tmp_path)
    args = main.get_parser(["--mode", "both", "--dataset_path", str(tmp_path / "ddti"), "--epochs",
                            "1", "--batch_size", "2", "--image_size", "64", "--num_workers", "0",
                            "--dice_ratio", "1", "--gpu_augment_all", "--use_elastic",
                            "--use_speckle", "--use_tgc", "--use_clahe"])
    main.main(args)
    assert len(os.listdir(tmp_path / "experiments")) == 1
