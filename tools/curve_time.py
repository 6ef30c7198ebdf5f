#!/usr/bin/env python3
"""Time the threshold-sweep histogram per sample against the torch composition a user writes without
it, on the same inputs and in one process.

Input: --batch x 1 x 512 x 512 float32 logits and {0, 1} targets (10 % positives) on the device,
B = --bins operating points, for two logit distributions:
  uniform  logit(u), u uniform in (0, 1): every bin equally likely;
  skewed   95 % of the pixels at -9 (one bin: confident background), the rest as above.  This is the
           realistic case and the worst one for a histogram: the lanes of a wave add to one word.
  device   unet_hip.curve_hist (+ unet_hip.curve_stats, timed on its own): 8 bytes read per pixel.
  torch    torch.bucketize + torch.bincount over (plane, class, bin) keys (torch ops only).
Each side is timed with HIP events around 20 back-to-back calls (median of --runs after --warmup
calls), so that a call shorter than the host's launch sequence is not timed as that sequence.  The
achieved bytes/s is the ideal 8 bytes per pixel over that time, set against the rate of a float4
copy of the same tensor measured here (4 bytes read + 4 written per element) and the 8.0 TB/s HBM
peak of the MI355X.  The two routes' histograms are compared in the same run.

    python tools/curve_time.py --out profiles/curve_time.txt
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "thyroid-nodule-image-segmentation-unet-ddti_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

HBM_PEAK = 8.0e12


def torch_hist(x, t, edges):
    planes, B = x.shape[0], edges.numel() + 1
    b = torch.bucketize(x, edges)  # the number of edges below x
    u = t.to(torch.int64)
    key = (torch.arange(planes, device=x.device)[:, None] * 2 + u) * B + b
    ok = (u == 0) | (u == 1)
    return torch.bincount(key[ok], minlength=planes * 2 * B).view(planes, 2, B)


CALLS = 20  # back-to-back calls inside one pair of events: the queue hides the host's launch time


def event_ms(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / CALLS)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--label", default="", help="a note for the header (which build is measured)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("curve_time.py measures on the GPU; none is visible")
    import unet_hip
    dev = torch.device("cuda:0")
    n, s, B = a.batch, a.size, a.bins
    g = torch.Generator(device="cpu").manual_seed(11)
    elems = n * s * s
    edges = unet_hip.curve_edges(B).to(dev)
    u = torch.rand((n, s * s), generator=g).clamp(1e-6, 1 - 1e-6)
    uniform = torch.log(u / (1 - u))
    skewed = torch.where(torch.rand((n, s * s), generator=g) < 0.95, torch.full_like(uniform, -9.0), uniform)
    t = (torch.rand((n, s * s), generator=g) < 0.1).float().to(dev)
    dst = torch.empty((n, s * s), device=dev)
    src = uniform.to(dev)
    copy_ms = event_ms(lambda: dst.copy_(src), a.warmup, a.runs)
    copy_rate = 8 * elems / (copy_ms * 1e-3)
    lines = [f"threshold-sweep histogram, {n} x 1 x {s} x {s} float32, B = {B}, median of {a.runs} runs of {CALLS} "
             f"calls after {a.warmup}; ms per sample; bytes/s = 8 bytes per pixel / time"
             + (f"; {a.label}" if a.label else ""),
             f"float4 copy of the same tensor: {copy_ms / n:.5f} ms/sample, {copy_rate / 1e12:.3f} TB/s; HBM peak "
             f"{HBM_PEAK / 1e12:.1f} TB/s ({torch.cuda.get_device_name(0)})", ""]

    def row(name, ms):
        bw = 8 * elems / (ms * 1e-3)
        lines.append(f"  {name:<36s} {ms / n:9.5f} ms/sample  {bw / 1e12:6.3f} TB/s  "
                     f"{100 * bw / copy_rate:5.1f} % of copy rate, {100 * bw / HBM_PEAK:5.1f} % of peak")
        return ms

    res = {}
    for name, x in (("uniform", uniform), ("skewed", skewed)):
        x = x.to(dev)
        total = torch.zeros(2 * B + 1, dtype=torch.int64, device=dev)
        ph, _ = unet_hip.curve_hist(x, t, edges, total)
        ds = torch.zeros(B + 1, dtype=torch.float64, device=dev)
        top = ph.sum((0, 1)).max().item() / elems
        lines.append(f"{name}: fullest bin holds {100 * top:.1f} % of the pixels")
        tt = row("torch  bucketize + bincount", event_ms(lambda: torch_hist(x, t, edges), a.warmup, a.runs))
        kt = row("device unet_hip.curve_hist", event_ms(lambda: unet_hip.curve_hist(x, t, edges, total), a.warmup, a.runs))
        st = event_ms(lambda: unet_hip.curve_stats(ph, ds), a.warmup, a.runs)
        lines.append(f"  device unet_hip.curve_stats             {st / n:9.5f} ms/sample ({1e3 * st:.1f} us per call)")
        same = torch.equal(ph.long(), torch_hist(x, t, edges))
        lines.append(f"  curve_hist / torch time = {kt / tt:.4f} ({tt / kt:.1f}x faster); histograms "
                     f"{'bit-equal' if same else 'DIFFER'}")
        lines.append("")
        res[name] = kt
    r = res["skewed"] / res["uniform"]
    lines.append(f"skewed / uniform time of curve_hist = {r:.2f}"
                 + ("  (the skewed case is MORE than 2x slower than the uniform one)" if r > 2 else ""))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
