#!/usr/bin/env python3
"""Time the predict-mode export per image -- the score plane resized back to the frame
(unet_hip.resize_back) and the contour overlay (unet_hip.overlay), the device-side successor of the
reference's plot (utils/trainer.py:262-299) -- against two ways to do it without them, on the same
inputs and in one process.

Input: --batch score planes of --size x --size N(0, 3^2) logits, each resized to --out_h x --out_w
(360 x 560, a DDTI frame) and thresholded, then overlaid on a gray frame of that size.
  kernels   unet_hip.resize_back (mask only; and with the plane), unet_hip.overlay at width 2,
            alpha 96, with a ground-truth mask.
  torch     on the device: F.interpolate(bilinear, antialias) + compare for the resize; max_pool2d
            of the inverted mask for the border + where for the overlay.  NOT bit-equal to Pillow (float32
            arithmetic, a square neighbourhood): a time baseline only.
  host      Pillow Image.resize on a mode "F" image + NumPy compare; NumPy shifts for the contour.
Each device side is timed with HIP events around the whole batch (median of --runs after --warmup).
The achieved bytes/s is the ideal traffic over that time, set beside a float4-sized copy
(torch.Tensor.copy_ of 256 MiB) timed in the same run.  Ideal traffic per image: resize, mask only
4 S^2 + h w; with the plane + 4 h w; overlay with ground truth 3 h w in, 3 h w out.

    python tools/export_time.py --out profiles/export_time.txt
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "thyroid-nodule-image-segmentation-unet-ddti_amd")
for p in (REPO, PKG, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as TF  # noqa: E402


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


def torch_resize(score, oh, ow):
    plane = TF.interpolate(score[None, None], size=(oh, ow), mode="bilinear", antialias=True, align_corners=False)[0, 0]
    return (plane > 0).to(torch.uint8)


def torch_border(m, r):
    inv = 1.0 - m[None, None].float()
    near_bg = TF.max_pool2d(TF.pad(inv, (r, r, r, r), value=1.0), 2 * r + 1, stride=1)[0, 0]
    return (m != 0) & (near_bg > 0)


def torch_overlay(gray, pred, gt, r, alpha):
    g = gray.to(torch.int32)
    cp, cg = torch_border(pred, r), torch_border(gt, r)
    interior = (pred != 0) & ~cp
    red = torch.where(interior, (g * (256 - alpha) + 255 * alpha + 128) >> 8, g)
    oth = torch.where(interior, (g * (256 - alpha) + 128) >> 8, g)
    rgb = torch.stack([red, oth, oth], -1)
    rgb = torch.where(cg[..., None], torch.tensor([0, 0, 255], device=g.device, dtype=torch.int32), rgb)
    rgb = torch.where(cp[..., None], torch.tensor([255, 0, 0], device=g.device, dtype=torch.int32), rgb)
    return rgb.to(torch.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out_h", type=int, default=360)
    ap.add_argument("--out_w", type=int, default=560)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("export_time.py measures on the GPU; none is visible")
    from PIL import Image

    import export_ref
    import unet_hip
    dev = torch.device("cuda:0")
    n, s, oh, ow = a.batch, a.size, a.out_h, a.out_w
    g = torch.Generator(device="cpu").manual_seed(13)
    # smooth planes, so that the masks are regions and not noise
    low = 3.0 * torch.randn((n, 1, 16, 16), generator=g)
    score_h = TF.interpolate(low, size=(s, s), mode="bicubic", align_corners=False)[:, 0].contiguous()
    score = score_h.to(dev)
    gray_h = torch.randint(0, 256, (n, oh, ow), generator=g, dtype=torch.uint8)
    gray = gray_h.to(dev)
    masks = [unet_hip.resize_back(score[i], (oh, ow), "greater", 0.0) for i in range(n)]
    gts = [torch.roll(m, (3, 5), (0, 1)) for m in masks]

    big = torch.empty(64 << 20, dtype=torch.float32, device=dev)
    dst = torch.empty_like(big)
    copy_ms = event_ms(lambda: dst.copy_(big), a.warmup, a.runs)
    copy_bw = 2 * big.numel() * 4 / (copy_ms * 1e-3)
    lines = [f"predict-mode export, {n} planes of {s} x {s} float32 -> {oh} x {ow}; median of {a.runs} runs after "
             f"{a.warmup}; ms per image; bytes/s = ideal traffic / time",
             f"device copy of 256 MiB (read + write) in this run: {copy_bw / 1e12:.3f} TB/s "
             f"({torch.cuda.get_device_name(0)})", ""]

    def row(name, ms, nbytes=None):
        t = f"  {name:<44s} {ms / n:9.5f} ms/image"
        if nbytes:
            bw = nbytes / (ms * 1e-3)
            t += f"  {bw / 1e12:6.3f} TB/s  {100 * bw / copy_bw:5.1f} % of the copy rate"
        lines.append(t)
        return ms

    rb = n * (4 * s * s + oh * ow)
    k1 = row("resize  unet_hip.resize_back (mask)",
             event_ms(lambda: [unet_hip.resize_back(score[i], (oh, ow), "greater", 0.0) for i in range(n)],
                      a.warmup, a.runs), rb)
    row("resize  unet_hip.resize_back (mask + plane)",
        event_ms(lambda: [unet_hip.resize_back(score[i], (oh, ow), "greater", 0.0, return_plane=True)
                          for i in range(n)], a.warmup, a.runs), rb + n * 4 * oh * ow)
    t1 = row("resize  torch interpolate + compare",
             event_ms(lambda: [torch_resize(score[i], oh, ow) for i in range(n)], a.warmup, a.runs), rb)
    t0 = time.perf_counter()
    host_planes = [np.asarray(Image.fromarray(score_h[i].numpy(), "F").resize((ow, oh), Image.BILINEAR)) for i in range(n)]
    host_masks = [(p > 0).astype(np.uint8) for p in host_planes]
    h1 = row("resize  Pillow + NumPy on the host", (time.perf_counter() - t0) * 1e3)
    same = all(np.array_equal(m.cpu().numpy(), hm) for m, hm in zip(masks, host_masks))
    tdiff = sum(int((torch_resize(score[i], oh, ow).cpu().numpy() != host_masks[i]).sum()) for i in range(n))
    lines.append(f"  resize: kernel / torch time = {k1 / t1:.3f}"
                 f"{'' if k1 < t1 else '  (the kernels do NOT beat the torch composition here)'}, kernel / host = "
                 f"{k1 / h1:.4f}; kernel masks equal Pillow's: {same}; torch's differ on {tdiff} of {n * oh * ow} pixels")
    lines.append("")
    ob = n * 6 * oh * ow
    k2 = row("overlay unet_hip.overlay (width 2, alpha 96, gt)",
             event_ms(lambda: [unet_hip.overlay(gray[i], masks[i], gts[i], 2, 96) for i in range(n)], a.warmup, a.runs),
             ob)
    t2 = row("overlay torch max_pool2d border + where",
             event_ms(lambda: [torch_overlay(gray[i], masks[i], gts[i], 2, 96) for i in range(n)], a.warmup, a.runs), ob)
    t0 = time.perf_counter()
    host_rgb = [export_ref.overlay(gray_h[i].numpy(), host_masks[i], gts[i].cpu().numpy(), 2, 96)[0] for i in range(n)]
    h2 = row("overlay NumPy on the host", (time.perf_counter() - t0) * 1e3)
    same = all(np.array_equal(unet_hip.overlay(gray[i], masks[i], gts[i], 2, 96)[0].cpu().numpy(), host_rgb[i])
               for i in range(n))
    lines.append(f"  overlay: kernel / torch time = {k2 / t2:.3f}"
                 f"{'' if k2 < t2 else '  (the kernel does NOT beat the torch composition here)'}, kernel / host = "
                 f"{k2 / h2:.4f}; kernel RGB equals the NumPy rules: {same} (torch's border is a square, not a diamond)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
