#!/usr/bin/env python3
"""Time BoundaryLoss forward + backward: the host path (scipy's distance transform of the
targets copied to the host, torch ops on the device -- models/loss.py before the device path)
against the device path (unet_hip.boundary_loss: distance transform, loss and dlogits kernels).

Each configuration is timed with HIP events (device time between the first and the last
enqueued operation) and with a host wall clock around the call plus a device synchronisation
(the host path's cost is mostly CPU time and the synchronising copies, which events alone do
not show).  Median of --runs runs after --warmup warm-up runs.  Masks: `blob` =
SyntheticSegmentation's discs, `empty` = an all-background batch (every sample takes the
empty-mask rule), `corner` = a single site in one corner of every sample (the longest row
scans).  The distance transform alone is listed as well.

    python tools/boundary_time.py --out profiles/boundary_time.txt
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


def host_distance_maps(targets):
    t = targets.detach().cpu().numpy().astype(np.uint8)
    out = np.stack([nd.distance_transform_edt(1 - t[b, 0]) for b in range(t.shape[0])])
    return torch.from_numpy(out[:, None].astype(np.float32)).to(targets.device)


def host_path(x, t):
    dist = host_distance_maps(t)
    loss = (torch.abs(torch.sigmoid(x) - t) * dist).flatten(1).mean(1).mean()
    loss.backward()
    return loss


def device_path(x, t):
    import unet_hip
    loss = unet_hip.boundary_loss(x, t)
    loss.backward()
    return loss


def device_edt(x, t):
    import unet_hip
    return unet_hip.distance_maps(t)


def host_edt(x, t):
    return host_distance_maps(t)


def measure(fn, x, t, warmup, runs):
    ev, wall = [], []
    for k in range(warmup + runs):
        x.grad = None
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn(x, t)
        b.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if k >= warmup:
            ev.append(a.elapsed_time(b))
            wall.append((t1 - t0) * 1e3)
    return statistics.median(ev), statistics.median(wall)


def make_masks(kind, bs, size):
    from data.data_loader import SyntheticSegmentation
    if kind == "blob":
        ds = SyntheticSegmentation(bs, size, seed=3)
        return torch.stack([ds[i][1] for i in range(bs)])
    t = torch.zeros(bs, 1, size, size)
    if kind == "corner":
        t[:, 0, size - 1, size - 1] = 1
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"BoundaryLoss forward + backward, median of {a.runs} runs after {a.warmup} warm-up "
             f"({torch.cuda.get_device_name(0)}); ms",
             f"{'config':<18}{'path':<8}{'events':>10}{'wall':>10}   {'edt events':>11}{'edt wall':>10}"]
    ok = True
    for bs, size in ((32, 256), (16, 512)):
        for kind in ("blob", "empty", "corner"):
            t = make_masks(kind, bs, size).to(dev)
            g = torch.Generator().manual_seed(1)
            x = torch.randn(bs, 1, size, size, generator=g).to(dev).requires_grad_(True)
            res = {}
            for name, full, edt in (("host", host_path, host_edt), ("device", device_path, device_edt)):
                res[name] = measure(full, x, t, a.warmup, a.runs) + measure(edt, x, t, a.warmup, a.runs)
                e, w, ee, ew = res[name]
                lines.append(f"{f'bs{bs} {size}^2 {kind}':<18}{name:<8}{e:>10.3f}{w:>10.3f}   "
                             f"{ee:>11.3f}{ew:>10.3f}")
            ok = ok and res["device"][1] < res["host"][1]
    lines.append("device wall < host wall in every configuration: " + ("yes" if ok else "NO"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
