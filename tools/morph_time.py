#!/usr/bin/env python3
"""Time the lesion-morphometry table per sample: the device call (unet_hip.morphometry_table: reduce,
extent and feret kernels, on labels already on the device) against two routes a user takes without
it, in one process:

* a torch composition on the device: ``bincount`` with weights for the six sums, ``scatter_reduce``
  (amin / amax) for the box, ``cdist`` over the contour of the largest component for the Feret
  diameter (no bit quads, no per-component Feret: less than the table holds), on the one-ellipse
  input only: on the many-component input (table rows in the tens of thousands) these torch calls
  did not come back within minutes on the MI355X, so that input has no torch column;
* scipy on the host after copying the labels back: ``sum_labels``, ``find_objects`` and ``pdist`` over
  the largest component's contour (one thread).

Inputs: 32 x 1 x 512 x 512 label planes of (a) one ellipse per plane and (b) a many-small-component
plane (30 % noise).  The reduce pass is also reported as achieved bytes/s of the label planes it
reads, against a device copy of the same planes timed in the same run, and with the block's LDS
table switched off (option morph_lds = 0: every run straight to global atomics).  HIP events, median
of --runs calls after --warmup.  No ratio is fixed in advance: the file records what was measured.

    python tools/morph_time.py --out profiles/morph_time.txt
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
from scipy.spatial.distance import pdist  # noqa: E402


def make_masks(kind, n, size, seed=11):
    r = np.random.default_rng(seed)
    i, j = np.mgrid[:size, :size]
    out = []
    for _ in range(n):
        if kind == "ellipse":
            cy, cx = size * (0.4 + 0.2 * r.random(2))
            ry, rx = size * (0.15 + 0.2 * r.random(2))
            out.append(((i - cy) / ry) ** 2 + ((j - cx) / rx) ** 2 <= 1.0)
        else:
            out.append(r.random((size, size)) < 0.3)
    return np.stack(out).astype(np.uint8)


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


def torch_route(lab, rows):
    """Sums, boxes and the largest component's Feret diameter of int32 (N, H, W) labels, in torch."""
    N, H, W = lab.shape
    yi = torch.arange(H, device=lab.device, dtype=torch.int32)[:, None].expand(H, W).reshape(-1)
    xi = torch.arange(W, device=lab.device, dtype=torch.int32)[None, :].expand(H, W).reshape(-1)
    ys, xs = yi.double(), xi.double()
    out = []
    for n in range(N):
        l = lab[n].reshape(-1).long()
        sums = [torch.bincount(l, weights=w, minlength=rows + 1) for w in (torch.ones_like(xs), xs, ys, xs * xs, xs * ys, ys * ys)]
        fg = l > 0  # (integer coordinates: float64 amin / amax is a compare-and-swap loop per colliding pixel)
        box = [torch.full((rows + 1,), v, dtype=torch.int32, device=lab.device).scatter_reduce(0, l[fg], w[fg], r)
               for v, w, r in ((1 << 30, xi, "amin"), (1 << 30, yi, "amin"), (-1, xi, "amax"), (-1, yi, "amax"))]
        big = int(torch.argmax(sums[0][1:])) + 1
        m = torch.nn.functional.pad(lab[n] == big, (1, 1, 1, 1))
        inner = m[:-2, 1:-1] & m[2:, 1:-1] & m[1:-1, :-2] & m[1:-1, 2:]
        pts = torch.nonzero(m[1:-1, 1:-1] & ~inner).double()
        out.append((sums, box, torch.cdist(pts, pts).max() ** 2))
    return out


def host_route(lab_dev, rows):
    lab = lab_dev.cpu().numpy()
    N, H, W = lab.shape
    i, j = np.mgrid[:H, :W]
    out = []
    for n in range(N):
        idx = np.arange(1, rows + 1)
        sums = [nd.sum_labels(w, lab[n], idx) for w in (np.ones((H, W)), j, i, j * j, i * j, i * i)]
        boxes = nd.find_objects(lab[n])
        big = int(np.argmax(sums[0])) + 1
        m = np.pad(lab[n] == big, 1)
        inner = m[:-2, 1:-1] & m[2:, 1:-1] & m[1:-1, :-2] & m[1:-1, 2:]
        pts = np.argwhere(m[1:-1, 1:-1] & ~inner).astype(np.float64)
        out.append((sums, boxes, pdist(pts, "sqeuclidean").max() if len(pts) > 1 else 0.0, big))
    return out


T0 = time.perf_counter()


def stage(what):
    print(f"[{time.perf_counter() - T0:7.1f} s] {what}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--host_runs", type=int, default=2)
    a = ap.parse_args()
    import unet_hip
    from unet_hip.runtime import UNetRuntime
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    rt = UNetRuntime.get(dev)
    N = a.batch
    lines = [f"Lesion morphometry table per sample: {N} x 1 x {a.size} x {a.size} int32 label planes (connectivity 1), "
             f"HIP events, median of {a.runs} calls after {a.warmup} warm-up ({torch.cuda.get_device_name(0)}); "
             f"ms/sample unless noted"]
    ok = True
    for kind in ("ellipse", "noise"):
        x = torch.from_numpy(make_masks(kind, N, a.size)).to(dev)
        lab, cnt = unet_hip.connected_components(x)
        rows = max(int(cnt.max()), 1)
        table = unet_hip.morphometry_table(lab, cnt, rows)
        want = unet_hip.morphometry_table_host(lab.cpu(), cnt.cpu(), rows)
        same = torch.equal(table.cpu(), want)
        host_ms, href = [], None
        for k in range(a.host_runs + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            href = host_route(lab, rows)
            if k:
                host_ms.append((time.perf_counter() - t0) * 1e3 / N)
        tab = table.cpu().numpy()
        for n, (sums, boxes, d2, big) in enumerate(href):  # the routes measure the same thing
            k = int(cnt[n])
            same &= all(np.array_equal(tab[n, :k, f], np.asarray(s[:k]).astype(np.int64)) for f, s in enumerate(sums))
            same &= int(tab[n, big - 1, 14]) == int(round(d2))
        T = min(N, 4)  # the torch composition runs sample by sample: a few samples time it
        stage("baselines on the host done")
        with_torch = kind == "ellipse"
        if with_torch:
            for n, (sums, box, d2) in enumerate(torch_route(lab[:T], rows)):
                same &= bool(torch.equal(sums[0][1:].long().cpu(), table[n, :, 0].cpu()))
                same &= int(round(float(d2))) == int(table[n, int(torch.argmax(table[n, :, 0])), 14])
            stage("torch composition checked")
        ok &= same
        t_dev = event_ms(lambda: unet_hip.morphometry_table(lab, cnt, rows), a.warmup, a.runs) / N
        stage("device table timed")
        t_torch = event_ms(lambda: torch_route(lab[:T], rows), 1, 3) / T if with_torch else None
        stage("torch composition timed")
        t_copy = event_ms(lambda: lab.clone(), a.warmup, a.runs)
        phases = {}
        for lds in (1, 0):
            rt.set_option("morph_lds", lds)
            rt.timing(True, "morph/")
            for _ in range(a.warmup):
                unet_hip.morphometry_table(lab, cnt, rows)
            rt.timing_records()
            for _ in range(a.runs):
                unet_hip.morphometry_table(lab, cnt, rows)
                for fam, ms, _ in rt.timing_records():
                    phases.setdefault((lds, fam), []).append(ms)
            rt.timing(False)
        rt.set_option("morph_lds", 1)
        med = {k: statistics.median(v) for k, v in phases.items()}
        nbytes = lab.numel() * 4
        h = statistics.median(host_ms)
        lines += [f"--- {kind}: {float(cnt.float().mean()):.0f} components per sample on average, table rows {rows}; "
                  f"device table equal to the host twin and to the baselines' sums and Feret: {'yes' if same else 'NO'}",
                  f"  device table (3 phases)                       {t_dev:9.4f}",
                  (f"  torch composition (bincount/scatter_reduce/cdist, {T} samples) {t_torch:9.4f}   "
                   f"({t_torch / t_dev:.1f} x the table)" if with_torch else
                   "  torch composition: not measured on this input (see the tool's header)"),
                  f"  scipy on the host (copy + sum_labels/find_objects/pdist, 1 thread) {h:9.4f}   ({h / t_dev:.1f} x the table)",
                  f"  per-phase, ms per launch over the batch of {N} (median):"]
        for fam in ("morph/reduce", "morph/extent", "morph/feret"):
            lines.append(f"    {fam:<16} LDS table {med[(1, fam)]:9.4f}    direct global atomics {med[(0, fam)]:9.4f}")
        r1, r0 = med[(1, "morph/reduce")], med[(0, "morph/reduce")]
        lines += [f"  reduce pass (table init + one read of the label planes, {nbytes / 1e6:.1f} MB): "
                  f"{nbytes / r1 / 1e6:.1f} GB/s read; device copy of the same planes {t_copy:.4f} ms = "
                  f"{nbytes / t_copy / 1e6:.1f} GB/s read (+ as much written)",
                  f"  LDS aggregation against direct global atomics on this input: {r0 / r1:.2f} x "
                  f"({'faster' if r1 < r0 else 'NOT faster'})"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
