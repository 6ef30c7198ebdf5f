#!/usr/bin/env python3
"""Time the surface-distance metrics (HD95, HD, ASSD) per sample: the host implementation of the
definition (scipy's binary_erosion and distance_transform_edt, numpy's percentile; one thread)
against the device call (unet_hip.surface_metrics: border, distance-transform, gather and
radix-select kernels plus the torch finalize).

Input: 64 synthetic 512x512 pairs, an ellipse as the target and a perturbed copy (shifted,
rescaled, with a ragged rim) as the prediction.  The device side is timed in batches of --batch
with HIP events (device time between the first and the last enqueued operation) and with a host
wall clock around the call plus a device synchronisation; the host side with the wall clock.
Median of --runs passes over all pairs after one warm-up pass; both sides' outputs are compared
in the same run (integer fields exactly, the three metrics within 1e-9 relative).

    python tools/surface_time.py --out profiles/surface_time.txt
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

FIELDS = ("defined", "n_pg", "n_gp", "max_d2", "d2_lo", "d2_hi")


def make_pairs(n, size, seed=7):
    r = np.random.default_rng(seed)
    i, j = np.mgrid[:size, :size]
    P, G = [], []
    for _ in range(n):
        cy, cx = size * (0.35 + 0.3 * r.random(2))
        ry, rx = size * (0.12 + 0.2 * r.random(2))
        g = ((i - cy) / ry) ** 2 + ((j - cx) / rx) ** 2 <= 1.0
        dy, dx = r.normal(0, 0.02 * size, 2)
        s = 1.0 + r.normal(0, 0.08, 2)
        ang = np.arctan2(i - cy - dy, j - cx - dx)
        rim = 1.0 + 0.06 * np.sin(7 * ang + r.random() * 6.28) + 0.03 * np.sin(23 * ang)
        p = ((i - cy - dy) / (ry * s[0])) ** 2 + ((j - cx - dx) / (rx * s[1])) ** 2 <= rim ** 2
        P.append(p)
        G.append(g)
    return np.stack(P), np.stack(G)


def host_metrics(p, g):
    """The definition (MedPy's hd / hd95 / assd at connectivity 1) on one pair of bool masks."""
    st = nd.generate_binary_structure(2, 1)
    bp, bg = p & ~nd.binary_erosion(p, st), g & ~nd.binary_erosion(g, st)
    d_pg = nd.distance_transform_edt(~bg)[bp]
    d_gp = nd.distance_transform_edt(~bp)[bg]
    both = np.hstack([d_pg, d_gp])
    s = np.sort(np.rint(both ** 2).astype(np.int64))
    pos = 0.95 * (s.size - 1)
    return dict(defined=1, n_pg=d_pg.size, n_gp=d_gp.size, max_d2=int(s[-1]),
                d2_lo=int(s[int(np.floor(pos))]), d2_hi=int(s[int(np.ceil(pos))]),
                hd=float(both.max()), hd95=float(np.percentile(both, 95)),
                assd=float((d_pg.mean() + d_gp.mean()) / 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    import unet_hip
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    P, G = make_pairs(a.pairs, a.size)
    x = torch.from_numpy(np.where(P, 3.0, -3.0).astype(np.float32))[:, None].to(dev)
    t = torch.from_numpy(G.astype(np.float32))[:, None].to(dev)

    host_ms, want = [], None
    for k in range(a.runs + 1):
        t0 = time.perf_counter()
        want = [host_metrics(p, g) for p, g in zip(P, G)]
        if k:
            host_ms.append((time.perf_counter() - t0) * 1e3 / a.pairs)

    ev_ms, wall_ms, got = [], [], None
    for k in range(a.runs + 1):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        got = [unet_hip.surface_metrics(x[b:b + a.batch], t[b:b + a.batch])
               for b in range(0, a.pairs, a.batch)]
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if k:
            ev_ms.append(e0.elapsed_time(e1) / a.pairs)
            wall_ms.append((t1 - t0) * 1e3 / a.pairs)
    got = {k: torch.cat([g[k] for g in got]).cpu().numpy() for k in got[0]}

    same = all(int(got[k][n]) == want[n][k] for n in range(a.pairs) for k in FIELDS)
    worst = max(abs(got[k][n] - want[n][k]) / max(abs(want[n][k]), 1e-300)
                for n in range(a.pairs) for k in ("hd", "hd95", "assd"))
    ok = same and worst <= 1e-9
    h, e, w = (statistics.median(v) for v in (host_ms, ev_ms, wall_ms))
    border = float(np.mean([wn["n_pg"] + wn["n_gp"] for wn in want]))
    lines = [f"Surface metrics (HD95, HD, ASSD) per sample, {a.pairs} synthetic {a.size}x{a.size} pairs "
             f"(ellipse vs perturbed copy, {border:.0f} surface pixels per pair on average), device in "
             f"batches of {a.batch}, median of {a.runs} passes after 1 warm-up "
             f"({torch.cuda.get_device_name(0)}); ms/sample",
             f"{'host scipy+numpy (1 thread)':>28}{'dev events':>12}{'dev wall':>10}{'host/dev wall':>15}"
             f"{'integer fields equal':>22}{'worst metric rel diff':>23}",
             f"{h:>28.3f}{e:>12.4f}{w:>10.4f}{h / w:>15.1f}{'yes' if same else 'NO':>22}{worst:>23.2e}",
             f"mean HD95 {np.mean([wn['hd95'] for wn in want]):.4f}, HD "
             f"{np.mean([wn['hd'] for wn in want]):.4f}, ASSD {np.mean([wn['assd'] for wn in want]):.4f} px"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
