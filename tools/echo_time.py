#!/usr/bin/env python3
"""Time the lesion echo table per sample: the device call (unet_hip.echo_table: a memset and the count
kernel, on grey planes and labels already on the device) against two routes a user takes without it,
in one process:

* a torch composition on the device, sample by sample: ``bincount`` on label * 256 + grey for the
  lesion histogram, a ``max_pool2d`` of the negated positive labels for the ring's ownership and a
  second ``bincount``, ``bincount`` over the four shifted slices for the co-occurrence pairs.  It is
  checked equal to the kernel's table before it is timed;
* the library's host twin (one thread) on planes already on the host.

Inputs: 32 x 1 x 512 x 512 planes of (a) one ellipse per plane and (b) many small components (30 %
noise), grey values a speckled background with darker lesions, and (c) the ellipses again under
nearly flat grey (two levels of noise), where the lanes of a wave do share histogram bins; levels 16,
ring 8.  Everything outside the A/B runs under the library's default options.  The count kernel is
also reported as achieved bytes/s over the ideal 5 bytes per pixel (one grey byte, one label) at the
default options, against a device copy of the same bytes timed in the same run, and under both values
of option echo_agg (0, the default: one LDS atomic per lane and count; 1: every add first aggregated
over the lanes that share the first active lane's label and column).  HIP events, median of --runs
calls after --warmup.  No ratio is fixed in advance: the file records what was measured.

    python tools/echo_time.py --out profiles/echo_time.txt
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
import torch  # noqa: E402

from morph_time import event_ms, make_masks  # noqa: E402

OFFSETS = ((0, 1), (1, 1), (1, 0), (1, -1))


def make_gray(masks, smooth=False, seed=12):
    """Speckle: background around 120, the lesions around 60; smooth: the same means with two grey
    levels of noise."""
    r = np.random.default_rng(seed)
    if smooth:
        g = np.where(masks > 0, 60, 120) + r.integers(0, 2, masks.shape)
    else:
        g = np.where(masks > 0, r.normal(60, 20, masks.shape), r.normal(120, 35, masks.shape))
    return np.clip(g, 0, 255).astype(np.uint8)


def torch_route(gray, lab, rows, G, w):
    """int64 (N, rows, 512 + G G): the echo table of gray uint8 / lab int32 (N, H, W), in torch."""
    N, H, W = lab.shape
    big = float(1 << 24)
    out = []
    for n in range(N):
        l, g = lab[n].long(), gray[n].long()
        pos = l > 0
        hist = torch.bincount(l[pos] * 256 + g[pos], minlength=(rows + 1) * 256).reshape(rows + 1, 256)[1:]
        neg = torch.where(pos, -l.float(), torch.full_like(l, -big, dtype=torch.float32))
        own = (-torch.nn.functional.max_pool2d(neg[None, None], 2 * w + 1, 1, w)[0, 0]).long()  # padding: -inf
        sel = ~pos & (own < (1 << 24))
        ring = torch.bincount(own[sel] * 256 + g[sel], minlength=(rows + 1) * 256).reshape(rows + 1, 256)[1:]
        q = (g * G) >> 8
        acc = torch.zeros((rows + 1) * G * G, dtype=torch.int64, device=lab.device)
        for dy, dx in OFFSETS:
            ys, xs = slice(0, H - dy), slice(max(0, -dx), W - max(0, dx))
            yt, xt = slice(dy, H), slice(max(0, dx), W + min(0, dx))
            a = l[ys, xs]
            same = (a == l[yt, xt]) & (a > 0)
            acc += torch.bincount(a[same] * G * G + q[ys, xs][same] * G + q[yt, xt][same], minlength=acc.numel())
        out.append(torch.cat([hist, ring, acc.reshape(rows + 1, G * G)[1:]], 1))
    return torch.stack(out)


T0 = time.perf_counter()


def stage(what):
    print(f"[{time.perf_counter() - T0:7.1f} s] {what}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--ring", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--host_runs", type=int, default=2)
    a = ap.parse_args()
    import unet_hip
    from unet_hip.runtime import UNetRuntime
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    rt = UNetRuntime.get(dev)
    N, G, w = a.batch, a.levels, a.ring
    lines = [f"Lesion echo table per sample: {N} x 1 x {a.size} x {a.size} uint8 grey planes and int32 label planes "
             f"(connectivity 1), levels {G}, ring {w}, HIP events, median of {a.runs} calls after {a.warmup} warm-up "
             f"({torch.cuda.get_device_name(0)}); ms/sample unless noted"]
    ok = True
    default = rt.get_option("echo_agg")
    lines.append(f"default options: echo_agg = {default}")
    for kind in ("ellipse", "noise", "ellipse, smooth grey"):
        masks = make_masks(kind.split(",")[0], N, a.size)
        gray = torch.from_numpy(make_gray(masks, "smooth" in kind)).to(dev)
        lab, cnt = unet_hip.connected_components(torch.from_numpy(masks).to(dev))
        rows = max(int(cnt.max()), 1)
        table = unet_hip.echo_table(gray, lab, cnt, rows, G, w)
        gh, lh, ch = gray.cpu(), lab.cpu(), cnt.cpu()
        host_ms, want = [], None
        for k in range(a.host_runs + 1):
            t0 = time.perf_counter()
            want = unet_hip.echo_table_host(gh, lh, ch, rows, G, w)
            if k:
                host_ms.append((time.perf_counter() - t0) * 1e3 / N)
        same = torch.equal(table.cpu(), want)
        stage(f"{kind}: host twin done")
        T = min(N, 4)  # the torch composition runs sample by sample: a few samples time it
        same_t = torch.equal(torch_route(gray[:T], lab[:T], rows, G, w), table[:T].long())
        stage(f"{kind}: torch composition checked")
        ok &= same and same_t
        t_dev = event_ms(lambda: unet_hip.echo_table(gray, lab, cnt, rows, G, w), a.warmup, a.runs) / N
        t_torch = event_ms(lambda: torch_route(gray[:T], lab[:T], rows, G, w), 1, 3) / T
        t_copy = event_ms(lambda: (lab.clone(), gray.clone()), a.warmup, a.runs)
        stage(f"{kind}: timed")
        phases = {}
        for agg in (1, 0):
            rt.set_option("echo_agg", agg)
            ok &= torch.equal(unet_hip.echo_table(gray, lab, cnt, rows, G, w).cpu(), want)
            rt.timing(True, "echo/")
            for _ in range(a.warmup):
                unet_hip.echo_table(gray, lab, cnt, rows, G, w)
            rt.timing_records()
            for _ in range(a.runs):
                unet_hip.echo_table(gray, lab, cnt, rows, G, w)
                for fam, ms, _ in rt.timing_records():
                    phases.setdefault((agg, fam), []).append(ms)
            rt.timing(False)
        rt.set_option("echo_agg", default)
        med = {k: statistics.median(v) for k, v in phases.items()}
        nbytes = lab.numel() * 5
        h = statistics.median(host_ms)
        c1, c0 = med[(1, "echo/count")], med[(0, "echo/count")]
        cd = med[(default, "echo/count")]
        lines += [f"--- {kind}: {float(cnt.float().mean()):.0f} components per sample on average, table rows {rows} "
                  f"({table.numel() * 4 / 1e6:.1f} MB of table); device table equal to the host twin: "
                  f"{'yes' if same else 'NO'}, to the torch composition ({T} samples): {'yes' if same_t else 'NO'}",
                  f"  device table (memset + count kernel, default options) {t_dev:9.4f}",
                  f"  torch composition (bincount / max_pool2d / shifted bincount, {T} samples) {t_torch:9.4f}   "
                  f"({t_torch / t_dev:.1f} x the table{'' if t_torch > t_dev else ': the kernel LOSES'})",
                  f"  host twin (1 thread, planes on the host)           {h:9.4f}   ({h / t_dev:.1f} x the table)",
                  f"  per-phase, ms per launch over the batch of {N} (median):"]
        for fam in ("echo/clear", "echo/count"):
            lines.append(f"    {fam:<12} wave-aggregated adds {med[(1, fam)]:9.4f}    plain LDS atomics {med[(0, fam)]:9.4f}")
        lines += [f"  count kernel (echo_agg = {default}) over the ideal 5 bytes per pixel ({nbytes / 1e6:.1f} MB): "
                  f"{nbytes / cd / 1e6:.1f} GB/s read; "
                  f"device copy of the same planes {t_copy:.4f} ms = {nbytes / t_copy / 1e6:.1f} GB/s read (+ as much "
                  f"written)",
                  f"  wave-aggregated against plain LDS atomics on this input: {c0 / c1:.2f} x "
                  f"({'faster' if c1 < c0 else 'NOT faster'})"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
