#!/usr/bin/env python3
"""Time the test-time-augmentation kernels per sample against the torch composition a user writes
without them, on the same inputs and in one process.

Input: a --batch x 1 x 512 x 512 float32 image batch and K such batches of N(0, 3^2) logits on
the device, for the view sets "flips" (K = 4) and "d4" (K = 8).
  views   torch: torch.cat of flip / transpose(...).contiguous() per view (torch ops only);
          kernel: unet_hip.tta_views.  Ideal traffic 4 + 4 K bytes per input element.
  merge   torch: un-flip / un-transpose each view, sigmoid, stack, mean, > 0.5, and the votes as
          a sum of (sigmoid > 0.5) (torch ops only); kernel: unet_hip.tta_merge, mode "prob" and
          "logit".  Ideal traffic 4 K + 4 + 2 bytes per output element.
Each side is timed with HIP events around the call (median of --runs after --warmup calls).  The
achieved bytes/s is the ideal traffic over that time, set against the HBM figure of the MI355X:
8.0 TB/s peak, 6.3 TB/s achieved by a float4 copy.  The outputs of both routes are compared in the
same run (the torch mean sums in another order, so scores differ in the last bits).

    python tools/tta_time.py --out profiles/tta_time.txt
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

HBM_PEAK, HBM_COPY = 8.0e12, 6.3e12


def view(x, k):
    y = x
    if k & 4:
        y = y.transpose(-1, -2)
    if k & 2:
        y = torch.flip(y, (-2,))
    if k & 1:
        y = torch.flip(y, (-1,))
    return y


def unview(y, k):
    x = y
    if k & 1:
        x = torch.flip(x, (-1,))
    if k & 2:
        x = torch.flip(x, (-2,))
    if k & 4:
        x = x.transpose(-1, -2)
    return x


def torch_views(x, ks):
    return torch.cat([view(x, k).contiguous() for k in ks])


def torch_merge(logits, n, ks, mode):
    xs = torch.stack([unview(logits[q * n:(q + 1) * n], k) for q, k in enumerate(ks)])
    p = torch.sigmoid(xs)
    votes = (p > 0.5).sum(0, dtype=torch.uint8)
    if mode == "prob":
        score = p.mean(0)
        return score, (score > 0.5).to(torch.uint8), votes
    score = xs.mean(0)
    return score, (torch.sigmoid(score) > 0.5).to(torch.uint8), votes


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
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tta_time.py measures on the GPU; none is visible")
    import unet_hip
    from unet_hip.functional import tta_view_numbers
    dev = torch.device("cuda:0")
    n, s = a.batch, a.size
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn((n, 1, s, s), generator=g).to(dev)
    elems = n * s * s
    lines = [f"test-time augmentation, {n} x 1 x {s} x {s} float32 per view, median of {a.runs} runs "
             f"after {a.warmup}; ms per sample; bytes/s = ideal traffic / time",
             f"HBM: {HBM_PEAK / 1e12:.1f} TB/s peak, {HBM_COPY / 1e12:.1f} TB/s float4 copy "
             f"({torch.cuda.get_device_name(0)})", ""]

    def row(name, ms, nbytes):
        bw = nbytes / (ms * 1e-3)
        lines.append(f"  {name:<34s} {ms / n:9.5f} ms/sample  {bw / 1e12:6.3f} TB/s  "
                     f"{100 * bw / HBM_COPY:5.1f} % of copy rate, {100 * bw / HBM_PEAK:5.1f} % of peak")
        return ms

    for name in ("flips", "d4"):
        ks = tta_view_numbers(name)
        K = len(ks)
        logits = (3.0 * torch.randn((K * n, 1, s, s), generator=g)).to(dev)
        lines.append(f"{name} (K = {K})")
        vb = (4 + 4 * K) * elems
        tv = row("views  torch composition", event_ms(lambda: torch_views(x, ks), a.warmup, a.runs), vb)
        kv = row("views  unet_hip.tta_views", event_ms(lambda: unet_hip.tta_views(x, name), a.warmup, a.runs), vb)
        assert torch.equal(torch_views(x, ks), unet_hip.tta_views(x, name))
        lines.append(f"  views: kernel / torch time = {kv / tv:.3f}; outputs bit-equal")
        mb = (4 * K + 4 + 2) * elems
        for mode in ("prob", "logit"):
            tm = row(f"merge {mode:<5s} torch composition",
                     event_ms(lambda: torch_merge(logits, n, ks, mode), a.warmup, a.runs), mb)
            km = row(f"merge {mode:<5s} unet_hip.tta_merge",
                     event_ms(lambda: unet_hip.tta_merge(logits, n, name, mode), a.warmup, a.runs), mb)
            ts, tmask, tvotes = torch_merge(logits, n, ks, mode)
            got = unet_hip.tta_merge(logits, n, name, mode)
            lines.append(f"  merge {mode}: kernel / torch time = {km / tm:.3f}"
                         f"{'' if km < tm else '  (the fused merge is NOT faster here)'}; "
                         f"max |score diff| {(got['score'] - ts).abs().max().item():.2e}, "
                         f"mask differs on {(got['mask'] != tmask).sum().item()} of {elems} pixels, "
                         f"votes on {(got['votes'] != tvotes).sum().item()}")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
