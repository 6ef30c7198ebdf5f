#!/usr/bin/env python3
"""Time connected-component labelling and the mask post-processing per sample: the device calls
(unet_hip.connected_components and unet_hip.postprocess_mask: tile, seam, flatten and rank /
select / write / fill kernels) against the host route a user takes without them (copy the masks
back, then scipy.ndimage.label + bincount + binary_fill_holes; one thread), in one process.

Input: a 16 x 1 x 512 x 512 uint8 batch on the device, an ellipse with a hole per sample plus
salt-and-pepper noise (islands outside, pinholes inside).  The device side is timed with HIP
events around each call (median of --runs after --warmup calls) for each tile shape (option
cc_tile); the per-phase kernel times come from the context's per-launch events in a separate
pass.  Both routes' outputs are compared in the same run, exactly.

    python tools/cc_time.py --out profiles/cc_time.txt
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "thyroid-nodule-image-segmentation-unet-ddti_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import scipy.ndimage as nd  # noqa: E402
import torch  # noqa: E402

TILES = {0: "64x16", 1: "64x32", 2: "64x64"}


def make_masks(n, size, noise, seed=7):
    r = np.random.default_rng(seed)
    i, j = np.mgrid[:size, :size]
    out = []
    for _ in range(n):
        cy, cx = size * (0.35 + 0.3 * r.random(2))
        ry, rx = size * (0.15 + 0.2 * r.random(2))
        m = ((i - cy) / ry) ** 2 + ((j - cx) / rx) ** 2 <= 1.0
        m &= ~(((i - cy) / (ry / 4)) ** 2 + ((j - cx) / (rx / 4)) ** 2 <= 1.0)
        out.append(m ^ (r.random((size, size)) < noise))
    return np.stack(out).astype(np.uint8)


def host_route(masks_dev):
    """What a user does without the device path: labels, largest component, filled holes."""
    masks = masks_dev.cpu().numpy()
    labs, outs = [], []
    for m in masks:
        lab, k = nd.label(m)
        keep = lab == np.argmax(np.bincount(lab.ravel())[1:]) + 1 if k else lab != 0
        labs.append(lab)
        outs.append(nd.binary_fill_holes(keep))
    return np.stack(labs), np.stack(outs)


def event_ms(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--noise", type=float, default=0.02)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--host_runs", type=int, default=3)
    a = ap.parse_args()
    import unet_hip
    from unet_hip.runtime import UNetRuntime
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    rt = UNetRuntime.get(dev)
    x = torch.from_numpy(make_masks(a.batch, a.size, a.noise)).to(dev)
    N = a.batch

    host_ms, want = [], None
    for k in range(a.host_runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = host_route(x)
        if k:
            host_ms.append((time.perf_counter() - t0) * 1e3 / N)
    h = statistics.median(host_ms)

    calls = {"label": lambda: unet_hip.connected_components(x),
             "keep-largest": lambda: unet_hip.postprocess_mask(x, keep_largest=True),
             "keep-largest + fill-holes": lambda: unet_hip.postprocess_mask(x, keep_largest=True, fill_holes=True)}
    default = rt.get_option("cc_tile")
    rows, same = [], True
    for tile, name in TILES.items():
        rt.set_option("cc_tile", tile)
        lab, cnt = unet_hip.connected_components(x)
        out, info = unet_hip.postprocess_mask(x, keep_largest=True, fill_holes=True)
        same &= np.array_equal(lab.cpu().numpy(), want[0]) and np.array_equal(out.cpu().numpy().astype(bool), want[1])
        t = {k: event_ms(f, a.warmup, a.runs) / N for k, f in calls.items()}
        wall0 = time.perf_counter()
        for _ in range(a.runs):
            unet_hip.connected_components(x)
            unet_hip.postprocess_mask(x, keep_largest=True, fill_holes=True)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - wall0) * 1e3 / a.runs / N
        rows.append((tile, name, t, wall))
    rt.set_option("cc_tile", default)

    phases = {}
    rt.timing(True, "cc/")
    for _ in range(a.warmup):
        unet_hip.connected_components(x)
        unet_hip.postprocess_mask(x, keep_largest=True, fill_holes=True)
    rt.timing_records()
    for _ in range(a.runs):
        unet_hip.connected_components(x)
        unet_hip.postprocess_mask(x, keep_largest=True, fill_holes=True)
        for fam, ms, _ in rt.timing_records():
            phases.setdefault(fam, []).append(ms)
    rt.timing(False)

    comps = float(np.mean([w.max() for w in want[0]]))
    lines = [f"Connected components and mask post-processing per sample: {N} x 1 x {a.size} x {a.size} uint8 masks "
             f"(ellipse with a hole, {a.noise:.0%} salt-and-pepper noise, {comps:.0f} components per sample on "
             f"average, connectivity 1), HIP events, median of {a.runs} calls after {a.warmup} warm-up "
             f"({torch.cuda.get_device_name(0)}); ms/sample",
             f"host route (copy back + scipy label + bincount + binary_fill_holes, 1 thread): {h:.3f}",
             f"{'tile':>8}{'label':>10}{'largest':>10}{'largest+fill':>14}{'label & largest+fill wall':>27}"
             f"{'host / device wall':>20}"]
    for tile, name, t, wall in rows:
        lines.append(f"{name + ('*' if tile == default else ''):>8}{t['label']:>10.4f}{t['keep-largest']:>10.4f}"
                     f"{t['keep-largest + fill-holes']:>14.4f}{wall:>27.4f}{h / wall:>20.1f}")
    lines.append(f"(* the default tile)   labels and masks equal to scipy for every tile: {'yes' if same else 'NO'}")
    lines.append(f"per-phase kernel times, default tile, ms per launch over the batch of {N} (median):")
    for fam, v in phases.items():
        lines.append(f"  {fam:<28}{statistics.median(v):>9.4f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
