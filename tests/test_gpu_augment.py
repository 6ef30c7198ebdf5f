"""Device-side training augmentations (unet_augment_u8 / unet_clahe_u8 through
unet_hip.GpuResizeToTensor) against the host hooks of the same source (which
tests/test_aug_cpu.py pins to Pillow and the NumPy classes), and the whole loader against the
host transform chain.  Bit-equal everywhere."""
import os
import random
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (7, 5), (16, 16), (33, 48), (40, 333)]
ANGLES = [0, 90, 180, -90, 45, -1e-9, 179.999999, 30, -117.3]
ALL_ON = dict(use_tgc=True, use_clahe=True)


def plane(h, w, seed=0):
    return np.random.default_rng(seed + 1000 * h + w).integers(0, 256, (h, w), dtype=np.uint8)


@pytest.fixture(scope="module")
def pipe():
    import unet_hip
    return unet_hip.GpuResizeToTensor((32, 32), device="cuda:0")


def device(pipe, a, rec, is_mask=False):
    t = torch.from_numpy(a).to(pipe.device)
    return pipe.augment(t, rec, is_mask).cpu().numpy()


def host(a, rec, is_mask=False):
    from unet_hip.data import apply_augment_host
    return np.asarray(apply_augment_host(a, rec, is_mask))


@pytest.mark.parametrize("shape", SHAPES)
def test_augment_kernel_matches_host_hook(pipe, shape):
    from unet_hip.data import AugRecord
    a = plane(*shape)
    r = random.Random(shape[0] * 7 + shape[1])
    for k, angle in enumerate(ANGLES):
        for fh in (False, True):
            for fv in (False, True):
                rec = AugRecord(flip_h=fh, flip_v=fv, angle=angle,
                                brightness=r.uniform(0.5, 1.5) if k % 2 else None,
                                tgc=tuple(r.uniform(0.8, 1.2) for _ in range(10)) if k % 3 else None)
                assert np.array_equal(device(pipe, a, rec), host(a, rec)), rec
                assert np.array_equal(device(pipe, a, rec, True), host(a, rec, True)), rec


@pytest.mark.parametrize("shape", [(4, 4), (5, 4), (7, 5), (16, 16), (33, 48), (40, 333)])
def test_clahe_kernels_match_host_hook(pipe, shape):
    from unet_hip.data import AugRecord
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    smooth = (100 + 20 * np.sin(yy / 5.0) + 10 * np.cos(xx / 7.0) + plane(*shape) % 4).astype(np.uint8)
    for a in (plane(*shape), smooth, np.full(shape, 77, np.uint8)):
        for clip in (2.0, 40.0, 0.0):
            rec = AugRecord(clahe=(clip, (4, 4)))
            assert np.array_equal(device(pipe, a, rec), host(a, rec)), clip
    if shape == (33, 48):
        rec = AugRecord(clahe=(2.0, (2, 3)))
        assert np.array_equal(device(pipe, plane(*shape), rec), host(plane(*shape), rec))


def test_one_large_plane_crosses_many_blocks(pipe):
    from unet_hip.data import AugRecord
    a = plane(512, 512, 1)
    for angle in (90, 33.3):
        rec = AugRecord(flip_h=True, angle=angle, brightness=1.3,
                        tgc=tuple(0.8 + 0.04 * i for i in range(10)), clahe=(2.0, (4, 4)))
        assert np.array_equal(device(pipe, a, rec), host(a, rec)), angle
        assert np.array_equal(device(pipe, a, rec, True), host(a, rec, True)), angle


def test_refusals_on_the_device_entry(pipe):
    from unet_hip import _lib
    from unet_hip.data import AugRecord
    t = torch.zeros((1, 8), dtype=torch.uint8, device=pipe.device)
    with pytest.raises(_lib.HipError, match="UNET_ERR_SHAPE"):
        pipe.augment(t, AugRecord(clahe=(2.0, (4, 4))), False)
    with pytest.raises(_lib.HipError, match="UNET_ERR_UNSUPPORTED"):
        pipe.augment(t, AugRecord(clahe=(2.0, (16, 17))), False)


def _samples(n):
    """n seeded (image, mask) PIL pairs of mixed sizes."""
    from PIL import Image
    sizes = [(33, 48), (40, 333), (64, 64), (100, 37), (57, 80), (48, 33), (90, 90), (36, 56)]
    out = []
    for k in range(n):
        h, w = sizes[k % len(sizes)]
        yy, xx = np.mgrid[0:h, 0:w]
        m = (((yy - h / 2) ** 2 + (xx - w / 3) ** 2) < (min(h, w) / 3) ** 2).astype(np.uint8) * 255
        out.append((Image.fromarray(plane(h, w, k), "L"), Image.fromarray(m, "L")))
    return out


def test_pipeline_matches_host_chain(pipe):
    """GpuResizeToTensor(images, masks, aug=records) == host chain + Resize + ToTensor."""
    from utils.transforms import build_train_transform
    cfg = types.SimpleNamespace(**ALL_ON)
    host_tf = build_train_transform(cfg, (32, 32))
    dev_tf = build_train_transform(cfg, device_augment=True)
    want_x, want_t, images, masks = [], [], [], []
    for k, (img, m) in enumerate(_samples(8)):
        random.seed(500 + k)
        np.random.seed(500 + k)
        x, t = host_tf(img, m)
        want_x.append(x)
        want_t.append(t)
        random.seed(500 + k)
        np.random.seed(500 + k)
        pi, pm = dev_tf(img, m)
        images.append(pi)
        masks.append(pm)
    records = [p.aug for p in images]
    assert any(r.clahe for r in records) and any(r.tgc for r in records)
    assert any(r.angle is not None for r in records)
    x, t = pipe(images, masks, aug=records)
    assert torch.equal(x.cpu(), torch.stack(want_x)) and torch.equal(t.cpu(), torch.stack(want_t))


def test_aug_none_is_the_plain_resize(pipe):
    from utils.transforms import Resize, ToTensor
    pairs = _samples(4)
    images = [np.asarray(i) for i, _ in pairs]
    masks = [np.asarray(m) for _, m in pairs]
    x0, t0 = pipe(images, masks)
    x1, t1 = pipe(images, masks, aug=None)
    x2, t2 = pipe(images, masks, aug=[None] * 4)
    assert torch.equal(x0, x1) and torch.equal(t0, t1) and torch.equal(x0, x2) and torch.equal(t0, t2)
    for k, (img, m) in enumerate(pairs):
        hx, ht = ToTensor()(*Resize((32, 32))(img, m))
        assert torch.equal(x0[k].cpu(), hx) and torch.equal(t0[k].cpu(), ht)


def _jpeg_dir(root):
    os.makedirs(root / "train")
    os.makedirs(root / "train_mask")
    for k, (img, m) in enumerate(_samples(6)):
        img.save(root / "train" / f"{k}.jpg")
        m.save(root / "train_mask" / f"{k}_mask.jpg")
    return str(root / "train"), str(root / "train_mask")


@pytest.mark.parametrize("workers", [0, 2])
def test_device_loader_matches_host_chain_loader(tmp_path, workers):
    """DeviceResizeLoader over the recording transform == the host-chain DataLoader, batch by
    batch, under the same seed (the workers take identical decisions)."""
    from data.data_loader import DeviceResizeLoader, MedicalDataset, u8_collate
    from utils.transforms import build_train_transform
    d, md = _jpeg_dir(tmp_path)
    cfg = types.SimpleNamespace(**ALL_ON)

    def batches(device_side):
        random.seed(11)
        np.random.seed(11)
        g = torch.Generator().manual_seed(11)
        if device_side:
            ds = MedicalDataset(d, md, build_train_transform(cfg, device_augment=True))
            dl = torch.utils.data.DataLoader(ds, batch_size=3, num_workers=workers,
                                             collate_fn=u8_collate, generator=g)
            dl = DeviceResizeLoader(dl, (32, 32), "cuda:0")
        else:
            ds = MedicalDataset(d, md, build_train_transform(cfg, (32, 32)))
            dl = torch.utils.data.DataLoader(ds, batch_size=3, num_workers=workers, generator=g)
        return [(x.cpu(), t.cpu()) for x, t in dl]

    want, got = batches(False), batches(True)
    assert len(want) == len(got) == 2
    for (wx, wt), (gx, gt) in zip(want, got):
        assert torch.equal(wx, gx) and torch.equal(wt, gt)


def test_main_cli_gpu_augment(tmp_path, monkeypatch):
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
                            "--dice_ratio", "1", "--gpu_augment", "--use_tgc", "--use_clahe"])
    main.main(args)
    assert len(os.listdir(tmp_path / "experiments")) == 1
