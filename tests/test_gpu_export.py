"""GPU: the predict-mode export kernels (csrc/kernels_export.hip) against Pillow for the resized
float32 plane (uint32 bit patterns) and against the NumPy restatement export_ref for the masks, the
RGB bytes and the statistics; then the scratch growth, the Predictor against the composition of
the public functions, main.py --mode predict in a child process and Trainer.test(save_overlays)."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import export_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "thyroid-nodule-image-segmentation-unet-ddti_amd")
TILE_H, TILE_W = 16, 64  # overlay_kernel's tile


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pillow(a, oh, ow):
    return np.asarray(Image.fromarray(a, "F").resize((ow, oh), Image.BILINEAR))


def host_pred(x):
    """surf_pred evaluated by the host (the reference of tests/test_gpu_mask_counts.py)."""
    import unet_hip
    labels, _ = unet_hip.connected_components_host(torch.from_numpy(x.reshape(1, 1, 1, -1).copy()), kind="logits")
    return labels.numpy().reshape(-1) != 0


def check_sigmoid_mask(mask, x):
    """The rule of test_gpu_mask_counts._check_mask: x > 0 outside the 0.5 band; inside it the
    float32 sigmoid legitimately rounds to 0.5, so the host's readout or x > 0."""
    mask, x = mask.reshape(-1).astype(bool), x.reshape(-1)
    far = np.abs(x) >= 2.0 ** -20
    assert np.array_equal(mask[far], x[far] > 0)
    near = ~far
    if near.any():
        ok = (mask[near] == host_pred(x[near])) | (mask[near] == (x[near] > 0))
        assert ok.all()


@pytest.mark.parametrize("h,w,oh,ow", R.RESIZE_SHAPES)
def test_resize_back(h, w, oh, ow):
    import unet_hip
    a = R.score_plane(h, w, h * 1000 + ow)
    a[0, :6] = [0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 1e-40, 2.0 ** -21]  # the sigmoid's band
    want = pillow(a, oh, ow)
    ad = torch.from_numpy(a).to(DEV)
    for thr in (0.25, -3.0):
        mask, plane = unet_hip.resize_back(ad, (oh, ow), "greater", thr, return_plane=True)
        assert np.array_equal(bits(plane.cpu().numpy()), bits(want)), "plane differs from Pillow"
        assert np.array_equal(mask.cpu().numpy(), (want > np.float32(thr)).astype(np.uint8))
        assert torch.equal(unet_hip.resize_back(ad, (oh, ow), "greater", thr), mask)
    mask, plane = unet_hip.resize_back(ad, (oh, ow), "sigmoid", return_plane=True)
    assert np.array_equal(bits(plane.cpu().numpy()), bits(want))
    m = mask.cpu().numpy()
    assert set(np.unique(m)) <= {0, 1}
    check_sigmoid_mask(m, want)
    assert torch.equal(unet_hip.resize_back(ad, (oh, ow), "sigmoid"), mask)


def test_resize_back_unaligned_views():
    """A plane that starts 4 bytes into its buffer: the scalar store path."""
    import unet_hip
    a = R.score_plane(16, 16, 3)
    buf = torch.zeros(16 * 16 + 1, dtype=torch.float32, device=DEV)
    buf[1:] = torch.from_numpy(a.reshape(-1)).to(DEV)
    mask, plane = unet_hip.resize_back(buf[1:].view(16, 16), (24, 40), "greater", 0.0, return_plane=True)
    want = pillow(a, 24, 40)
    assert np.array_equal(bits(plane.cpu().numpy()), bits(want))
    assert np.array_equal(mask.cpu().numpy(), (want > 0).astype(np.uint8))


def test_scratch_grows_with_work_in_flight():
    """tests/test_gpu_scratch.py's growth case for the resize intermediate: small, large, small on a
    fresh context and a side stream without a synchronisation in between."""
    from unet_hip.runtime import UNetRuntime
    rt = UNetRuntime(DEV)
    cases = [(R.score_plane(16, 16, 1), 23, 37), (R.score_plane(48, 48, 2), 360, 560), (R.score_plane(16, 16, 1), 23, 37)]
    ins = [torch.from_numpy(a).to(DEV) for a, _, _ in cases]
    plans = [(rt.export_plan(a.shape[1], ow), rt.export_plan(a.shape[0], oh)) for a, oh, ow in cases]
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        outs = [rt.resize_f32_mask(x, oh, ow, ph, pv, 1, 0.0, True) for x, (ph, pv), (_, oh, ow) in zip(ins, plans, cases)]
    s.synchronize()
    for (mask, plane), (a, oh, ow) in zip(outs, cases):
        want = pillow(a, oh, ow)
        assert np.array_equal(bits(plane.cpu().numpy()), bits(want))
        assert np.array_equal(mask.cpu().numpy(), (want > 0).astype(np.uint8))
    assert torch.equal(outs[0][1], outs[2][1])


CASES = R.overlay_cases(TILE_H, TILE_W)
_REF = {}


def overlay_ref(name, r, alpha, with_gt):
    key = (name, r, alpha, with_gt)
    if key not in _REF:
        gray, pred, gt = CASES[name]
        _REF[key] = R.overlay(gray, pred, gt if with_gt else None, r, alpha)
    return _REF[key]


@pytest.mark.parametrize("name", sorted(CASES))
def test_overlay(name):
    import unet_hip
    gray, pred, gt = (torch.from_numpy(a).to(DEV) for a in CASES[name])
    for r in (1, 2, 3):
        for alpha in (0, 96, 256):
            for with_gt in (False, True):
                rgb, st = unet_hip.overlay(gray, pred, gt if with_gt else None, r, alpha)
                want, wst = overlay_ref(name, r, alpha, with_gt)
                assert rgb.cpu().numpy().tobytes() == want.tobytes(), (name, r, alpha, with_gt)
                assert st.cpu().tolist() == wst, (name, r, alpha, with_gt)


def test_overlay_odd_width_rows_start_unaligned():
    """W = 7 and 65: the rows of the RGB plane start at every byte alignment."""
    import unet_hip
    rng = np.random.default_rng(11)
    for h, w in ((9, 7), (18, 65), (17, 130)):
        gray = rng.integers(0, 256, (h, w), dtype=np.uint8)
        pred = (rng.random((h, w)) < 0.6).astype(np.uint8)
        gt = (rng.random((h, w)) < 0.5).astype(np.uint8)
        rgb, st = unet_hip.overlay(*(torch.from_numpy(a).to(DEV) for a in (gray, pred, gt)), 2, 77)
        want, wst = R.overlay(gray, pred, gt, 2, 77)
        assert rgb.cpu().numpy().tobytes() == want.tobytes() and st.cpu().tolist() == wst


def test_device_refusals():
    import unet_hip
    from unet_hip import _lib
    rt = unet_hip.UNetRuntime.get(DEV)
    u = torch.zeros((4, 4), dtype=torch.uint8, device=DEV)
    for r, alpha in ((0, 0), (4, 0), (1, -1), (1, 257)):
        with pytest.raises(unet_hip.HipError, match="UNET_ERR_INVALID"):
            rt.overlay_u8(u, u, None, r, alpha)
    a = torch.zeros((4, 4), dtype=torch.float32, device=DEV)
    with pytest.raises(unet_hip.HipError, match="UNET_ERR_INVALID.*kind"):
        rt.resize_f32_mask(a, 4, 4, None, None, 7, 0.5, False)
    rc = rt.lib.unet_resize_f32_mask(rt.ctx, _lib.ptr(a), 4, 0, 4, 4, None, None, 0, None, None, 0, 0, 0.5, None,
                                     _lib.ptr(u), _lib.stream_ptr(DEV))
    assert rc == -1 and b">= 1" in rt.lib.unet_last_error(rt.ctx)


# ---------------------------------------------------------------- Predictor
def small_model():
    from models.mod import ResUNet
    torch.manual_seed(3)
    return ResUNet(base_filters=16, depth=3)


def frames():
    rng = np.random.default_rng(5)
    out = []
    for h, w in ((40, 56), (64, 64), (33, 80)):
        yy, xx = np.mgrid[0:h, 0:w]
        f = rng.integers(0, 120, (h, w)).astype(np.int64)
        f[(yy - h / 2) ** 2 + (xx - w / 3) ** 2 < (h / 4) ** 2] += 120
        out.append(f.astype(np.uint8))
    return out


@pytest.mark.parametrize("tta,largest", [("flips", True), ("none", False)])
def test_predictor_equals_the_composition(tta, largest):
    import unet_hip
    model = small_model()
    planes = frames()
    pred = unet_hip.Predictor(model, 32, DEV, tta=tta, tta_merge="prob", pp=dict(keep_largest=largest), width=2,
                              alpha=96)
    out = pred(planes, return_scores=True)
    pipe = unet_hip.GpuResizeToTensor(32, DEV)
    x = pipe(planes)
    with torch.no_grad():
        if tta == "none":
            score, kind = model.to(DEV).eval()(x)[:, 0].contiguous(), "sigmoid"
        else:
            score, kind = unet_hip.tta_predict(model, x, tta, "prob")["score"][:, 0].contiguous(), "greater"
    for i, f in enumerate(planes):
        h, w = f.shape
        mask, plane = unet_hip.resize_back(score[i], (h, w), kind, 0.5, return_plane=True)
        if largest:
            mask = unet_hip.postprocess_mask(mask, keep_largest=True)[0][0]
        gray = torch.from_numpy(f).to(DEV)
        rgb, st = unet_hip.overlay(gray, mask, None, 2, 96)
        _, count = unet_hip.connected_components(mask)
        assert torch.equal(out["masks"][i], mask) and torch.equal(out["overlays"][i], rgb)
        assert torch.equal(out["scores"][i], plane)
        row = out["rows"][i]
        assert [row[k] for k in ("area", "contour", "x0", "y0", "x1", "y1")] == st.cpu().tolist()
        assert (row["h"], row["w"], row["components"]) == (h, w, int(count.item()))
        if largest:
            assert row["components"] <= 1


def test_main_predict_end_to_end(tmp_path):
    """main.py --mode predict in a fresh child process on three small PNGs."""
    import unet_hip
    from unet_hip.predict import csv_row
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    planes = frames()
    names = ["a.png", "b.png", "c.png"]
    for n, f in zip(names, planes):
        Image.fromarray(f, "L").save(src / n)
    model = small_model()
    ckpt = tmp_path / "m.pth"
    torch.save({k: v.detach().clone().cpu() for k, v in model.state_dict().items()}, ckpt)
    cmd = [sys.executable, os.path.join(PKG, "main.py"), "--mode", "predict", "--input_dir", str(src), "--output_dir",
           str(dst), "--model_type", "ResUNet", "--base_filters", "16", "--depth", "3", "--image_size", "32",
           "--checkpoint_path", str(ckpt), "--batch_size", "2", "--contour_width", "2", "--overlay_alpha", "96",
           "--save_prob"]
    done = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout + done.stderr
    out = unet_hip.Predictor(model, 32, DEV, width=2, alpha=96)(planes, return_scores=True)
    lines = (dst / "predictions.csv").read_text().splitlines()
    assert lines[0].split(",")[:4] == ["name", "h", "w", "area"] and len(lines) == 4
    for i, n in enumerate(names):
        stem = n[:-4]
        mask = np.asarray(Image.open(dst / f"{stem}_mask.png"))
        assert mask.dtype == np.uint8 and set(np.unique(mask)) <= {0, 255}
        assert np.array_equal(mask, out["masks"][i].cpu().numpy() * 255)
        rgb = np.asarray(Image.open(dst / f"{stem}_overlay.png"))
        assert np.array_equal(rgb, out["overlays"][i].cpu().numpy())
        assert np.array_equal(bits(np.load(dst / f"{stem}_score.npy")), bits(out["scores"][i].cpu().numpy()))
        assert lines[i + 1] == csv_row(n, out["rows"][i])
        assert int(lines[i + 1].split(",")[3]) == int(out["masks"][i].sum().item())


def test_trainer_save_overlays(tmp_path):
    import unet_hip
    from data.data_loader import SyntheticSegmentation, create_dataloader
    from unet_hip.predict import gray_u8
    from utils.trainer import Trainer
    from utils.utils import Config, create_logger
    ns = argparse.Namespace(model_type="ResUNet", lr=1e-4, bce_ratio=1.0, dice_ratio=1.0, focal_ratio=0.5,
                            boundary_ratio=0.0, use_mixup=False, mixup_prob=0.0, mixup_alpha=0.2, epochs=1,
                            early_stop_patience=5, batch_size=2, num_workers=0, contour_width=2, overlay_alpha=64)
    cfg = Config(ns, base_dir=str(tmp_path))
    cfg.device = DEV
    loaders = tuple(create_dataloader(SyntheticSegmentation(4, 32, seed=s), cfg, shuffle=False) for s in range(3))
    tr = Trainer(cfg, loaders, create_logger(os.path.join(cfg.log_dir, "t.log")), small_model())
    plain = tr.test()
    assert not [f for f in os.listdir(cfg.result_dir) if f.startswith("test_overlay_")]
    with_png = tr.test(save_overlays=True)
    assert with_png == plain
    files = sorted(f for f in os.listdir(cfg.result_dir) if f.startswith("test_overlay_"))
    assert files == [f"test_overlay_{i}.png" for i in range(4)]
    assert not hasattr(tr, "kept")  # the test set is not pinned on the trainer
    idx = 0
    tr.model.eval()
    with torch.no_grad():
        for images, masks in loaders[2]:  # the samples in the loader's order, read as Trainer.test reads them
            images, masks = images.to(DEV).float(), masks.to(DEV).float()
            logits = tr.model(images)
            mask = torch.empty(logits.shape, dtype=torch.uint8, device=DEV)
            tr.rt.mask_counts(logits, masks, torch.zeros(6, dtype=torch.int64, device=DEV), mask)
            gray = gray_u8(images)
            for n in range(images.shape[0]):
                gt = (masks[n, 0].to(torch.uint8) == 1).to(torch.uint8)
                rgb, _ = unet_hip.overlay(gray[n], mask[n, 0], gt, 2, 64)
                got = np.asarray(Image.open(os.path.join(cfg.result_dir, f"test_overlay_{idx}.png")))
                assert np.array_equal(got, rgb.cpu().numpy())
                idx += 1
    assert idx == 4
