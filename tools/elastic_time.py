#!/usr/bin/env python3
"""Time ElasticDeform and SpeckleNoise per sample: the host chain (NumPy in one worker process,
utils/transforms.py) against the device chain of --gpu_augment_all (the host draws the float64
fields; unet_elastic_u8 + unet_augment_noise_u8 + unet_clahe_u8 run in front of the resize).

64 synthetic 360 x 560 image / mask pairs -> 512 x 512 (the pairs of tools/augment_time.py), three
flag sets: ElasticDeform alone and SpeckleNoise alone with their probability forced to 1 (every
sample pays), and the real chain with all four optional flags at the reference's probabilities.
Per sample, in ms:

  host chain     ElasticDeform ... CLAHE + DecodeU8 on the host: what one worker does per sample
                 under --gpu_transforms (wall clock)
  host left      what stays on the host with --gpu_augment_all: the draws (the np.random fields
                 among them) + DecodeU8 (wall)
  dev events     upload of planes and fields + elastic + augment + CLAHE + resize of image and mask
                 between two HIP events
  dev wall       the same by a host clock around the batch, ending in a synchronise (the per-plane
                 launches and the pageable uploads are driven from Python)
  resize wall    the device path without augmentations (--gpu_transforms), host clock
  upload B       bytes sent to the device per sample: 2 planes of 1 B/pixel, plus 16 B/pixel when
                 ElasticDeform fired and 8 B/pixel when SpeckleNoise fired (mean over the 64)

The synthetic planes are PIL images in memory, so no JPEG decoding is timed on either side.
Median of --runs passes over the 64 samples after --warmup warm-up passes (a device window holds
--reps batches of the 64); every pass re-seeds, so both sides take the same 64 sets of
decisions, and the device tensors of the first pass are compared with the host chain's + Resize +
ToTensor.

    python tools/elastic_time.py --out profiles/elastic_time.txt
"""
import argparse
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from augment_time import N, H, W, S, device_pass, host_pass, samples  # noqa: E402  (sets sys.path)

import torch  # noqa: E402

FLAG_SETS = (("elastic p=1", dict(use_elastic=True), True),
             ("speckle p=1", dict(use_speckle=True), True),
             ("all four", dict(use_elastic=True, use_speckle=True, use_tgc=True, use_clahe=True),
              False))


def chains(flags, force):
    """(host chain -> planes, host chain -> tensors, recording chain) of one flag set."""
    from data.data_loader import DecodeU8
    from utils.transforms import ElasticDeform, SpeckleNoise, build_train_transform
    cfg = types.SimpleNamespace(**flags)
    out = (build_train_transform(cfg, tail=[DecodeU8()]), build_train_transform(cfg, (S, S)),
           build_train_transform(cfg, device_augment="all"))
    if force:
        for tf in out:
            for t in tf.transforms + getattr(tf.transforms[0], "transforms", []):
                if isinstance(t, (ElasticDeform, SpeckleNoise)):
                    t.p = 1.0
    return out


def upload_bytes(planes):
    total = 0
    for pi, pm in planes:
        total += pi.nbytes + pm.nbytes
        if pi.aug.elastic is not None:
            total += sum(f.nbytes for f in pi.aug.elastic[2:])
        if pi.aug.speckle is not None:
            total += pi.aug.speckle.nbytes
    return total / len(planes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=4, help="device batches per timed window")
    a = ap.parse_args()
    import unet_hip
    if not torch.cuda.is_available():
        sys.exit("elastic_time.py needs the GPU: nothing is measured without it")
    pipe = unet_hip.GpuResizeToTensor((S, S), device="cuda:0")
    data = samples()
    med = statistics.median
    lines = [f"ElasticDeform / SpeckleNoise per sample, {N} synthetic {H}x{W} pairs -> {S}^2, median "
             f"of {a.runs} passes after {a.warmup} warm-up ({torch.cuda.get_device_name(0)}); "
             f"ms/sample",
             f"{'flags':<14}{'host chain':>12}{'host left':>11}{'dev events':>12}{'dev wall':>10}"
             f"{'resize wall':>13}{'upload B':>12}{'fired e/s':>11}{'bit-equal':>11}"]
    for name, flags, force in FLAG_SETS:
        host_u8, host_full, dev_tf = chains(flags, force)
        r = {k: [] for k in ("u8", "left", "ev", "wall", "rwall")}
        for k in range(a.warmup + a.runs):
            t_u8, _ = host_pass(host_u8, data)
            t_left, planes = host_pass(dev_tf, data)
            ev, wall, (x, t) = device_pass(pipe, planes, True, a.reps)
            _, rwall, _ = device_pass(pipe, planes, False, a.reps)
            if k == 0:
                _, want = host_pass(host_full, data)
                equal = (torch.equal(x.cpu(), torch.stack([w[0] for w in want])) and
                         torch.equal(t.cpu(), torch.stack([w[1] for w in want])))
                nbytes = upload_bytes(planes)
                fired = (sum(p[0].aug.elastic is not None for p in planes),
                         sum(p[0].aug.speckle is not None for p in planes))
            if k >= a.warmup:
                for key, v in zip(r, (t_u8, t_left, ev, wall, rwall)):
                    r[key].append(v)
        m = {k: med(v) for k, v in r.items()}
        lines.append(f"{name:<14}{m['u8']:>12.3f}{m['left']:>11.3f}{m['ev']:>12.3f}{m['wall']:>10.3f}"
                     f"{m['rwall']:>13.3f}{nbytes:>12.0f}{'%d/%d' % fired:>11}"
                     f"{'yes' if equal else 'NO':>11}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
