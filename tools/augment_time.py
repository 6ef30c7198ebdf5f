#!/usr/bin/env python3
"""Time the training augmentations per sample: the host chain (Pillow / NumPy in one worker
process, utils/transforms.py) against the device chain (--gpu_augment: unet_augment_u8 +
unet_clahe_u8 in front of the resize).

64 synthetic 360 x 560 image / mask pairs -> 512 x 512, with the default flags (Flip, Rotate,
AdjustBrightness) and with TGC + CLAHE switched on.  Per sample, in ms:

  host chain            Flip ... CLAHE + DecodeU8 on the host: what one worker does per sample
                        under --gpu_transforms (wall clock)
  host chain + resize   the same followed by Resize + ToTensor on the host: the reference's worker
  host left             what stays on the host with --gpu_augment: the draws + DecodeU8 (wall)
  device, events        upload + augment + CLAHE + resize of image and mask between two HIP events
  device, wall          the same by a host clock around the batch, ending in a synchronise (the
                        per-plane launches are driven from Python)
  resize only           the device path without augmentations (--gpu_transforms), same two clocks

The synthetic planes are PIL images in memory, so no JPEG decoding is timed on either side.
Median of --runs passes over the 64 samples after --warmup warm-up passes (a device window holds
--reps batches of the 64); every pass re-seeds, so both sides take the same 64 sets of
decisions.

    python tools/augment_time.py --out profiles/augment_time.txt
"""
import argparse
import os
import random
import statistics
import sys
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "thyroid-nodule-image-segmentation-unet-ddti_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

N, H, W, S = 64, 360, 560, 512


def samples():
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for _ in range(N):
        # speckled ultrasound-like texture and a disc mask
        img = np.clip(rng.normal(90, 40, (H, W)), 0, 255).astype(np.uint8)
        cy, cx, r = rng.uniform(100, 260), rng.uniform(150, 400), rng.uniform(30, 90)
        m = (((yy - cy) ** 2 + (xx - cx) ** 2) < r * r).astype(np.uint8) * 255
        out.append((Image.fromarray(img, "L"), Image.fromarray(m, "L")))
    return out


def seed():
    random.seed(0)
    np.random.seed(0)


def host_pass(tf, data):
    seed()
    t0 = time.perf_counter()
    out = [tf(i, m) for i, m in data]
    return (time.perf_counter() - t0) * 1e3 / N, out


def device_pass(pipe, planes, with_aug, reps):
    """`reps` batches of the 64 samples in one timed window."""
    images = [p[0] for p in planes]
    masks = [p[1] for p in planes]
    aug = [p[0].aug for p in planes] if with_aug else None
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        out = pipe(images, masks, aug=aug)
    b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / (N * reps)
    return a.elapsed_time(b) / (N * reps), wall, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=16, help="device batches per timed window")
    a = ap.parse_args()
    import unet_hip
    from data.data_loader import DecodeU8
    from utils.transforms import build_train_transform
    if not torch.cuda.is_available():
        sys.exit("augment_time.py needs the GPU: nothing is measured without it")
    pipe = unet_hip.GpuResizeToTensor((S, S), device="cuda:0")
    data = samples()
    med = statistics.median
    lines = [f"Training augmentations per sample, {N} synthetic {H}x{W} pairs -> {S}^2, median of "
             f"{a.runs} passes after {a.warmup} warm-up ({torch.cuda.get_device_name(0)}); ms/sample",
             f"{'flags':<14}{'host chain':>12}{'+ resize':>10}{'host left':>11}{'dev events':>12}"
             f"{'dev wall':>10}{'resize ev':>11}{'resize wall':>12}{'bit-equal':>11}"]
    beats = True
    for name, flags in (("default", {}), ("tgc+clahe", dict(use_tgc=True, use_clahe=True))):
        cfg = types.SimpleNamespace(**flags)
        host_u8 = build_train_transform(cfg, tail=[DecodeU8()])
        host_full = build_train_transform(cfg, (S, S))
        dev_tf = build_train_transform(cfg, device_augment=True)
        r = {k: [] for k in ("u8", "full", "left", "ev", "wall", "rev", "rwall")}
        equal = True
        for k in range(a.warmup + a.runs):
            t_u8, _ = host_pass(host_u8, data)
            t_full, want = host_pass(host_full, data)
            t_left, planes = host_pass(dev_tf, data)
            ev, wall, (x, t) = device_pass(pipe, planes, True, a.reps)
            rev, rwall, _ = device_pass(pipe, planes, False, a.reps)
            if k == 0:
                equal = (torch.equal(x.cpu(), torch.stack([w[0] for w in want])) and
                         torch.equal(t.cpu(), torch.stack([w[1] for w in want])))
            if k >= a.warmup:
                for key, v in zip(r, (t_u8, t_full, t_left, ev, wall, rev, rwall)):
                    r[key].append(v)
        m = {k: med(v) for k, v in r.items()}
        lines.append(f"{name:<14}{m['u8']:>12.3f}{m['full']:>10.3f}{m['left']:>11.3f}{m['ev']:>12.3f}"
                     f"{m['wall']:>10.3f}{m['rev']:>11.3f}{m['rwall']:>12.3f}{'yes' if equal else 'NO':>11}")
        # one worker's work per sample before and after: host chain vs what is left on the host,
        # and the device's own added time must not eat the difference
        beats = beats and (m["left"] + (m["wall"] - m["rwall"])) < m["u8"] and equal
    lines.append("host left + (device wall - resize-only wall) < host chain in every configuration: "
                 + ("yes" if beats else "NO"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
