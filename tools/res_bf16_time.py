#!/usr/bin/env python3
"""Time one training step of models/mod.py:ResUNet in fp32 and in bf16 math.

A step is forward, seg_losses (BCE + Dice), backward and HipAdamW, on synthetic data:
ResUNet(64, 4) and ResUNet(64, 5) at 512^2, bs 16, each with mfma_dtype "fp32" and "bf16", all
in one process.  Every step is timed with HIP events (device time between the first and the
last enqueued operation) and with a host wall clock around the step plus a device
synchronisation.  Reported: the median of --runs (>= 7) timed steps after --warmup warm-up
steps and the min-max over the timed steps.  bf16 counts as faster only where its median lies
below the fp32 median by more than both min-max spreads.

    python tools/res_bf16_time.py --out profiles/res_bf16_time.txt
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


def measure(depth, mfma, bs, size, warmup, runs, dev):
    import unet_hip
    from data.data_loader import SyntheticSegmentation
    torch.manual_seed(42)
    m = unet_hip.ResUNet(1, 1, base_filters=64, depth=depth, mfma_dtype=mfma).to(dev).train()
    opt = unet_hip.HipAdamW(m.parameters(), lr=1e-5)
    ds = SyntheticSegmentation(bs, size, seed=3)
    x = torch.stack([ds[i][0] for i in range(bs)]).to(dev)
    t = torch.stack([ds[i][1] for i in range(bs)]).to(dev)
    ev, wall = [], []
    for k in range(warmup + runs):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        opt.zero_grad()
        losses = unet_hip.seg_losses(m(x), t)
        (losses[0] + losses[1]).backward()
        opt.step()
        b.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if k >= warmup:
            ev.append(a.elapsed_time(b))
            wall.append((t1 - t0) * 1e3)
    del m, opt
    torch.cuda.empty_cache()
    return ev, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    a = ap.parse_args()
    if a.runs < 7:
        ap.error("--runs must be at least 7")
    dev = torch.device("cuda:0")
    lines = [f"ResUNet training step (forward, seg_losses, backward, HipAdamW), bs {a.batch} at "
             f"{a.size}^2, median of {a.runs} steps after {a.warmup} warm-up "
             f"({torch.cuda.get_device_name(0)}); ms",
             f"{'network':<16}{'math':<6}{'events':>9}{'min':>9}{'max':>9}{'wall':>9}{'min':>9}"
             f"{'max':>9}{'img/s':>9}"]
    ok = True
    for depth in (4, 5):
        res = {}
        for mfma in ("fp32", "bf16"):
            ev, wall = measure(depth, mfma, a.batch, a.size, a.warmup, a.runs, dev)
            res[mfma] = ev
            me, mw = statistics.median(ev), statistics.median(wall)
            lines.append(f"{f'ResUNet(64, {depth})':<16}{mfma:<6}{me:>9.2f}{min(ev):>9.2f}{max(ev):>9.2f}"
                         f"{mw:>9.2f}{min(wall):>9.2f}{max(wall):>9.2f}{a.batch / mw * 1e3:>9.1f}")
        f32, b16 = res["fp32"], res["bf16"]
        gain = statistics.median(f32) - statistics.median(b16)
        spread = max(max(f32) - min(f32), max(b16) - min(b16))
        faster = gain > spread
        ok = ok and faster
        lines.append(f"  bf16 vs fp32: {statistics.median(f32) / statistics.median(b16):.2f}x "
                     f"({gain:+.2f} ms against a min-max spread of {spread:.2f} ms): "
                     + ("faster" if faster else "NOT faster"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
