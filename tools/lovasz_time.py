#!/usr/bin/env python3
"""Time the Lovasz hinge loss per sample, forward and backward, against the torch composition a user
writes without it and against the library's host twin, on the same inputs and in one process.

Input: --batch x 1 x 512 x 512 float32 logits and {0, 1} blob targets on the device, two logit fields:
  fresh      randn logits, as a freshly initialised network gives: about all margins are active (e > 0);
  confident  95 % of the pixels on the right side of the margin (e <= 0), the rest as above.
  device   unet_hip.lovasz_hinge (forward: the segmented radix sort and the plane kernels, 15 launches
           per batch; backward: one streaming kernel).
  torch    per plane torch.sort(errors, descending=True, stable=True) + cumsum + the Jaccard
           increments + dot, in float32, autograd backward (Berman's published code).  NOT bit-equal
           to the device: its cumsums and Jaccard weights are float32 where the library's are exact
           integers and float64; the two losses are compared in the same run.
  host     unet_hip.lovasz_hinge_host on the CPU copies (forward only; a wall clock).
The device sides are timed with HIP events around --calls back-to-back calls (median of --runs after
--warmup), so a call shorter than the host's launch sequence is not timed as that sequence.  Achieved
bytes/s counts the bytes the ALGORITHM needs once -- forward 8 read + 4 written (gmap) per pixel, backward
12 read + 4 written -- over the time, set against a copy of the same tensor measured here and the 8.0 TB/s
HBM peak; the forward's four sort passes move about 100 bytes per pixel, so its share says how far the
sort is from a single streaming pass, not how well each pass streams.

    python tools/lovasz_time.py --out profiles/lovasz_time.txt
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

import torch  # noqa: E402

HBM_PEAK = 8.0e12


def torch_lovasz(x, t):
    """Berman's lovasz_hinge(per_image=True) over the (n, c) planes, float32 torch ops."""
    N, C, H, W = x.shape
    losses = []
    for logit, label in zip(x.reshape(N * C, -1), (t >= 0.5).float().reshape(N * C, -1)):
        signs = 2.0 * label - 1.0
        errors = 1.0 - logit * signs
        errors_sorted, perm = torch.sort(errors, dim=0, descending=True, stable=True)
        gt_sorted = label[perm]
        gts = gt_sorted.sum()
        intersection = gts - gt_sorted.cumsum(0)
        union = gts + (1.0 - gt_sorted).cumsum(0)
        jaccard = 1.0 - intersection / union
        jaccard = torch.cat([jaccard[:1], jaccard[1:] - jaccard[:-1]])
        losses.append(torch.dot(torch.relu(errors_sorted), jaccard))
    return torch.stack(losses).mean()


def event_ms(fn, warmup, runs, calls):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--label", default="", help="a note for the header (which build is measured)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lovasz_time.py measures on the GPU; none is visible")
    import unet_hip
    dev = torch.device("cuda:0")
    n, s = a.batch, a.size
    elems = n * s * s
    g = torch.Generator(device="cpu").manual_seed(13)
    yy, xx = torch.meshgrid(torch.arange(s), torch.arange(s), indexing="ij")
    c = torch.rand((n, 2), generator=g) * 0.5 + 0.25
    r = torch.rand((n, 1), generator=g) * 0.15 + 0.1
    t = (((yy[None] / s - c[:, :1, None]) ** 2 + (xx[None] / s - c[:, 1:, None]) ** 2) <= r[:, :, None] ** 2)
    t = t.float()[:, None].contiguous()
    fresh = torch.randn((n, 1, s, s), generator=g)
    sign = t * 2 - 1
    sure = torch.rand((n, 1, s, s), generator=g) < 0.95
    confident = torch.where(sure, sign * (1 + fresh.abs() * 3), fresh)
    td = t.to(dev)
    dst, src = torch.empty_like(td), fresh.to(dev)
    copy_ms = event_ms(lambda: dst.copy_(src), a.warmup, a.runs, a.calls)
    copy_rate = 8 * elems / (copy_ms * 1e-3)
    lines = [f"Lovasz hinge loss, {n} x 1 x {s} x {s} float32, median of {a.runs} runs of {a.calls} calls after "
             f"{a.warmup}; ms per sample; bytes/s = the algorithm's bytes per pixel (forward 12, backward 16) / time"
             + (f"; {a.label}" if a.label else ""),
             f"copy of the same tensor: {copy_ms / n:.5f} ms/sample, {copy_rate / 1e12:.3f} TB/s; HBM peak "
             f"{HBM_PEAK / 1e12:.1f} TB/s ({torch.cuda.get_device_name(0)})", ""]

    def row(name, ms, bytes_per_px):
        bw = bytes_per_px * elems / (ms * 1e-3)
        lines.append(f"  {name:<40s} {ms / n:9.5f} ms/sample  {bw / 1e12:6.3f} TB/s  "
                     f"{100 * bw / copy_rate:5.1f} % of copy rate, {100 * bw / HBM_PEAK:5.1f} % of peak")
        return ms

    slower = []
    for name, x in (("fresh", fresh), ("confident", confident)):
        xd = x.to(dev)
        active = ((1 - sign * x) > 0).float().mean().item()
        lines.append(f"{name}: {100 * active:.1f} % of the margins active (e > 0)")

        def fwd_bwd(fn):
            xr = xd.clone().requires_grad_(True)
            loss = fn(xr, td)
            go = torch.ones_like(loss)
            return xr, loss, lambda: torch.autograd.grad(loss, xr, go, retain_graph=True)

        with torch.no_grad():
            kf = row("device forward  unet_hip.lovasz_hinge", event_ms(lambda: unet_hip.lovasz_hinge(xd, td), a.warmup, a.runs, a.calls), 12)
            tf = row("torch  forward  sort + cumsum + dot", event_ms(lambda: torch_lovasz(xd, td), 2, 5, 2), 12)
        _, kl, kb = fwd_bwd(unet_hip.lovasz_hinge)
        _, tl, tb = fwd_bwd(torch_lovasz)
        kbt = row("device backward (one kernel)", event_ms(kb, a.warmup, a.runs, a.calls), 16)
        tbt = row("torch  backward (autograd)", event_ms(tb, 2, 5, 2), 16)
        xc, tc = x.contiguous(), t
        unet_hip.lovasz_hinge_host(xc[:1], tc[:1])
        t0 = time.perf_counter()
        host = unet_hip.lovasz_hinge_host(xc, tc)
        ht = (time.perf_counter() - t0) * 1e3
        lines.append(f"  {'host   forward  unet_lovasz_host (CPU)':<40s} {ht / n:9.5f} ms/sample (wall clock, one call)")
        lines.append(f"  forward device / torch time = {kf / tf:.4f} ({tf / kf:.1f}x faster); backward {kbt / tbt:.4f} "
                     f"({tbt / kbt:.1f}x faster)")
        lines.append(f"  loss: device {kl.item():.9g}, host twin {host['loss'].item():.9g}, torch float32 {tl.item():.9g} "
                     f"(the torch composition is not bit-equal: float32 cumsums and weights)")
        lines.append("")
        if kf >= tf or kbt >= tbt:
            slower.append(name)
    lines.append("the kernel path is faster than the torch composition in this run" if not slower else
                 f"THE KERNEL PATH IS NOT FASTER than the torch composition on: {', '.join(slower)}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
