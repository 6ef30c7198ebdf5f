"""The code that joins the metric, loss and checkpoint paths across ranks, on a real GPU: two ranks
(gloo, both on cuda:0, the harness of test_gpu_dist.py) drive ``utils.trainer.Trainer`` with the
switches ``main.py --mode test`` offers and with a boundary term in training.

* ``Trainer.test()``: every rank walks its own shard of the test split once more in eval mode (the
  batch shapes of ``test()``, so the logits are the same bits) and restates every per-sample
  quantity with the references of the single-process tests (surface_ref, cc_ref, the torch views
  merged by the host twin, the curve host twins, curve_ref).  The parent alone combines the two
  ranks' records -- integer sums, float64 means in dataset order -- and compares the dict ``test()``
  returned: integers and functions of integers exactly, means of float64 per-sample values at the
  1e-9 relative bar of the single-process tests (only the summation order differs).
* the contour gather: batch by batch, rank 0's shard before rank 1's, to rank 0 alone.
* ``Trainer._losses`` with a boundary term on leaf logits against the fp64 composite of the
  CONCATENATED batch, value and this rank's slice of the gradient, on 2 + 1, 2 + 2 and 1 + empty.
* ``Trainer.train()``: the same epochs, scheduler and early-stopping state on both ranks, the
  checkpoints written by rank 0 alone, ``_last.pth`` reproducing rank 0's eval logits.

Splits: test 7 samples at global batch 3 (shards 2 + 1, 2 + 1, 1 + empty), validation 5 samples at
global batch 3 (2 + 1, 1 + 1), training 6 samples at global batch 3.  One test sample's mask is
blanked, so that the surface blocks count an undefined sample (on rank 1)."""
import os
import time
import traceback
from datetime import timedelta

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_gpu_dist import PKG, REPO, _free_port

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BINS = 256
EPOCHS = 20  # 40 steps: the BN running statistics the eval forwards read have settled
# (samples, seed[, the sample whose mask is blanked]).  Test sample 5 -- rank 1's shard of the second
# batch -- has no foreground: surface-undefined, so that k != total and u != 0 in the surface blocks
# (the synthetic masks are never empty and this model never predicts an empty one).  Validation seed
# 36: the first of 1..60 at which the gathered split's operating point differs from what either
# rank's shard alone chooses, under both criteria (gathered 246 / 246, shards 247 / 247 and 244 / 244).
TRAIN, VAL, TEST = (6, 0), (5, 36), (7, 2, 5)
BASE = ["TP", "FP", "FN", "TN", "ACC", "Precision", "Recall", "F1", "IoU"]
MEANS = {"HD95", "HD", "ASSD", "PP_HD95", "PP_HD", "PP_ASSD", "Curve_BestImageDice", "Curve_ImageDice"}
PP = dict(pp_largest=True, pp_min_area=8, pp_fill_holes=True)


# ---------------------------------------------------------------- the two-rank harness
def _guarded(body, rank, world, port, q, *args):
    import sys
    for p in (REPO, PKG, os.path.join(REPO, "tests")):
        sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    # a collective the other rank never joins raises here instead of hanging the worker
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    try:
        torch.cuda.set_device(0)
        q.put((rank, body(rank, world, *args)))
    except Exception:
        q.put((rank, ("error", traceback.format_exc())))
        raise
    finally:
        dist.destroy_process_group()


def _spawn(body, *args):
    """body(rank, world, *args) on two ranks -> (rank 0's result, rank 1's); both exit 0."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_guarded, args=(body, r, 2, port, q) + args) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    deadline = time.monotonic() + 240  # a worker left alone in a collective raises after 120 s
    try:
        for _ in procs:
            rank, out = q.get(timeout=max(deadline - time.monotonic(), 1))
            assert not (isinstance(out, tuple) and len(out) == 2 and out[0] == "error"), f"rank {rank}:\n{out[1]}"
            res[rank] = out
        for p in procs:
            p.join(120)
            assert p.exitcode == 0, p.exitcode
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
                p.join(10)
    return res[0], res[1]


def _dataset(n, seed, blank=None):
    """SyntheticSegmentation(n, 64, seed); sample `blank`, if given, with an empty mask."""
    from data.data_loader import SyntheticSegmentation

    class Blanked(SyntheticSegmentation):
        def __getitem__(self, idx):
            img, m = super().__getitem__(idx)
            return img, (torch.zeros_like(m) if idx == blank else m)
    return Blanked(n, 64, seed=seed)


def _trainer(rank, world, tmp, splits, bs, **kw):
    """The small ResUNet of the single-process end-to-end tests over DataParallel shards; one log
    file for both ranks, as main.py has it."""
    import argparse
    from data.data_loader import DataParallelShardSampler, dp_collate
    from models.mod import ResUNet
    from utils.trainer import Trainer
    from utils.utils import Config, create_logger
    args = dict(model_type="ResUNet", lr=1e-3, bce_ratio=1.0, dice_ratio=1.0, focal_ratio=0.0, boundary_ratio=0.0,
                use_mixup=False, mixup_prob=0.0, mixup_alpha=0.2, epochs=1, early_stop_patience=5, batch_size=bs,
                num_workers=0)
    args.update(kw)
    cfg = Config(argparse.Namespace(**args), base_dir=os.path.join(tmp, f"r{rank}"))
    cfg.device = DEV
    loaders = tuple(torch.utils.data.DataLoader(
        _dataset(*s), batch_sampler=DataParallelShardSampler(s[0], bs, False, rank, world), collate_fn=dp_collate())
        for s in splits)
    torch.manual_seed(0)
    model = ResUNet(base_filters=16, depth=3)
    return Trainer(cfg, loaders, create_logger(os.path.join(tmp, "shared.log")), model), loaders


def _log(tmp):
    with open(os.path.join(str(tmp), "shared.log")) as f:
        return f.read()


# ---------------------------------------------------------------- 1, 2: Trainer.test()
def _confusion(P, G):
    return np.array([(P & G).sum(), (P & ~G).sum(), (~P & G).sum(), (~P & ~G).sum()], np.int64)


def _surface(P, G):
    import surface_ref
    o = surface_ref.oracle(P, G)
    return (int(o["defined"]), o["hd95"], o["hd"], o["assd"])


def _shard_records(tr, loader, tta=False, curve=False):
    """This rank's shard of `loader` once more in eval mode, batch by batch as test() forms them,
    and every per-sample quantity by the references of tests/: a list of dicts with `idx`, the
    sample's index in the split."""
    import cc_ref
    import unet_hip
    from test_gpu_tta import _torch_view
    edges = unet_hip.curve_edges(BINS)
    recs = []
    tr.model.eval()
    with torch.no_grad():
        for idx, batch in zip(loader.batch_sampler, loader):
            if batch is None:
                assert idx == []
                continue
            xb, yb = batch
            x, y = xb.to(DEV).float(), yb.to(DEV).float()
            logits = tr.model(x)
            mask = torch.empty(logits.shape, dtype=torch.uint8, device=DEV)
            tr.rt.mask_counts(logits, y, torch.zeros(6, dtype=torch.int64, device=DEV), mask)
            raw = mask.cpu().numpy()[:, 0] != 0
            src = raw
            if tta:  # the torch views through the model, merged by the host twin
                lg = torch.cat([tr.model(_torch_view(x, k)).float() for k in range(8)]).cpu()
                h = unet_hip.tta_merge_host(lg, x.shape[0], "d4", "prob")
                src = h["mask"].numpy()[:, 0] != 0
                votes = h["votes"].numpy()[:, 0]
            lc, yc = logits.float().cpu(), yb.float()
            for j, i in enumerate(idx):
                g = yb.numpy()[j, 0].astype(np.int64) == 1
                r = dict(idx=i, raw=_confusion(raw[j], g), mask=src[j], pred_pixels=int(src[j].sum()),
                         defined=bool(src[j].any() and g.any()))
                if tta:
                    r.update(tta=_confusion(src[j], g), dis=int(((votes[j] > 0) & (votes[j] < 8)).sum()))
                if curve:
                    ph, tot = unet_hip.curve_hist_host(lc[j:j + 1, :1], yc[j:j + 1, :1], edges)
                    r.update(x=lc[j, 0].reshape(-1).numpy(), t=yc[j, 0].reshape(-1).numpy(), hist=tot.numpy(),
                             dice=unet_hip.curve_stats_host(ph)["dice_sum"].numpy())
                else:
                    clean = cc_ref.postprocess(src[j], 1, True, 8, True)[0]
                    r.update(surf=_surface(src[j], g), pp=_confusion(clean, g), pp_surf=_surface(clean, g),
                             les=np.array(cc_ref.lesion(clean, g, 1), np.int64))
                recs.append(r)
    return recs


def _eval_body(rank, world, tmp, case):
    from utils.trainer import Trainer
    plots = []
    if case == "a":  # record what rank 0 would plot; no matplotlib needed
        Trainer._can_plot = staticmethod(lambda: True)
        Trainer._plot_contours = lambda self, keep: plots.append(
            [tuple(t.numpy() for t in entry) for entry in keep])
    else:
        Trainer._can_plot = staticmethod(lambda: False)
    tr, loaders = _trainer(rank, world, tmp, (TRAIN, VAL, TEST), 3)
    for ep in range(EPOCHS):
        tr.train_one_epoch(ep)
    cfg = tr.config
    out = dict(plots=plots)
    if case in "ab":
        cfg.surface_metrics = cfg.lesion_metrics = True
        for k, v in PP.items():
            setattr(cfg, k, v)
        if case == "b":
            cfg.tta, cfg.tta_merge = "d4", "prob"
        out["metrics"] = [tr.test()]
        out["test"] = _shard_records(tr, loaders[2], tta=case == "b")
    else:
        cfg.curve_metrics = True
        out["metrics"] = []
        for thr in ("val-dice", "val-image-dice", 0.3):
            cfg.threshold = thr
            out["metrics"].append(tr.test())
        out["test"] = _shard_records(tr, loaders[2], curve=True)
        out["val"] = _shard_records(tr, loaders[1], curve=True)
    return out


def _block(c, prefix=""):
    """utils/trainer.py:232-250 of the reference, from the four counts."""
    TP, FP, FN, TN = (int(v) for v in c)
    eps = 1e-8
    P = TP / (TP + FP + eps)
    R = TP / (TP + FN + eps)
    d = dict(TP=TP, FP=FP, FN=FN, TN=TN, ACC=(TP + TN) / (TP + TN + FP + FN + eps), Precision=P, Recall=R,
             F1=2 * P * R / (P + R + eps), IoU=TP / (TP + FP + FN + eps))
    return {prefix + k: v for k, v in d.items()}


def _surface_block(recs, key, prefix=""):
    """(entries, the log's count string): float64 means in dataset order over the defined samples."""
    ok = [r[key] for r in recs if r[key][0]]
    mean = [float(np.mean([s[f] for s in ok])) if ok else float("nan") for f in (1, 2, 3)]
    d = {prefix + "HD95": mean[0], prefix + "HD": mean[1], prefix + "ASSD": mean[2], prefix + "SurfaceDefined": len(ok)}
    return d, f"over {len(ok)} of {len(recs)} images ({len(recs) - len(ok)} undefined)"


def _same_dicts(a, b):
    return list(a) == list(b) and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)


def _compare(got, want):
    assert list(got) == list(want), (list(got), list(want))
    for k, w in want.items():
        g = got[k]
        if isinstance(w, float) and np.isnan(w):
            assert np.isnan(g), (k, g, w)
        elif k in MEANS:
            print(f"{k}: {g!r} vs {w!r}")
            assert abs(g - w) <= 1e-9 * max(abs(w), 1e-300), (k, g, w)
        else:
            assert g == w, (k, g, w)


def _gathered(r0, r1, split):
    """Both ranks' records in dataset order; every sample of the split exactly once."""
    recs = sorted(r0[split] + r1[split], key=lambda r: r["idx"])
    n = dict(test=TEST[0], val=VAL[0])[split]
    assert [r["idx"] for r in recs] == list(range(n))
    return recs


def _guard(recs):
    """The sensitivity guard of the single-process tests on the gathered prediction."""
    pred = sum(r["pred_pixels"] for r in recs)
    assert 0 < pred < len(recs) * 64 * 64, pred
    assert any(r["defined"] for r in recs)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", ["a", "b"], ids=["surface_pp_lesion", "tta_d4"])
def test_trainer_test_metric_blocks_dp2(tmp_path, case):
    """(a) surface + post-processing + lesion blocks, (b) the same reading the D4-merged mask plus
    the TTA block.  Case (a) also pins the contour gather: rank 0 gets the 7 samples in dataset
    order -- batch by batch, rank 0's shard (2, 2, 1 samples) before rank 1's (1, 1, none) -- and
    rank 1 plots nothing."""
    r0, r1 = _spawn(_eval_body, str(tmp_path), case)
    (m,), (m1,) = r0["metrics"], r1["metrics"]
    assert _same_dicts(m, m1), (m, m1)
    recs = _gathered(r0, r1, "test")
    _guard(recs)
    assert 1 <= sum(r["surf"][0] for r in recs) < len(recs)  # defined and undefined samples: k != total
    n = len(recs)
    tot = lambda k: sum(r[k] for r in recs)
    want = _block(tot("raw"))
    if case == "b":
        want.update(_block(tot("tta"), "TTA_"))
        want["TTA_Disagreement"] = int(tot("dis")) / int(tot("tta").sum())
    sb, s_line = _surface_block(recs, "surf")
    want.update(sb)
    want.update(_block(tot("pp"), "PP_"))
    pb, p_line = _surface_block(recs, "pp_surf", "PP_")
    want.update(pb)
    n_pred, n_gt, gt_hit, pred_hit = (int(v) for v in tot("les"))
    want.update(LesionRecall=gt_hit / n_gt if n_gt else float("nan"),
                LesionPrecision=pred_hit / n_pred if n_pred else float("nan"),
                FPComponentsPerImage=(n_pred - pred_hit) / n, PredComponents=n_pred, GTComponents=n_gt)
    print({k: m[k] for k in m if k not in BASE})
    _compare(m, want)
    text = _log(tmp_path)
    for header, times in (("Test Metrics", 1), ("Surface Metrics", 1), ("Post-processed", 1), ("Lesion Metrics", 1),
                          ("TTA (", int(case == "b")), ("Curve Metrics", 0), ("Operating point", 0)):
        assert text.count(header) == times, (header, text.count(header))
    assert "Total Images: 7\n" in text
    assert "px " + s_line in text.split("Surface Metrics")[1].split("\n")[0]
    assert "px " + p_line in text.split("Post-processed")[1]
    if case == "a":
        ds = _dataset(*TEST)
        assert len(r0["plots"]) == 1 and r1["plots"] == []
        keep = r0["plots"][0]
        assert [k[0].shape[0] for k in keep] == [2, 1, 2, 1, 1]
        images, gts, masks = (np.concatenate([k[i] for k in keep]) for i in range(3))
        assert images.shape[0] == 7
        for i in range(7):
            assert np.array_equal(images[i], ds[i][0].numpy()), i
            assert np.array_equal(gts[i], ds[i][1].numpy()), i
            assert np.array_equal(masks[i, 0] != 0, recs[i]["mask"]), i


def _curve_of(recs):
    """curve_summary of the records' host histograms (integer sums) and per-image Dice curves
    (float64, added in the order given)."""
    import unet_hip
    ds = np.zeros(BINS + 1, np.float64)
    for r in recs:
        ds = ds + r["dice"]
    return unet_hip.curve_summary(sum(r["hist"] for r in recs).tolist(), ds.tolist(), len(recs),
                                  unet_hip.curve_edges(BINS))


def _image_choice_is_order_free(recs, what):
    """The best mean per-image Dice must win by more than any summation order can move a sum of
    len(recs) values in [0, 1].  Operating points whose per-image Dice equal the winner's image for
    image (no pixel of any image in the bins between them) tie bit for bit in every order -- the
    same additions of the same values -- and the tie rule, not rounding, decides among them."""
    D = np.stack([r["dice"] for r in recs])
    s = np.zeros(BINS + 1)
    for row in D:
        s = s + row
    k = _curve_of(recs)["best_image_k"]
    others = ~(D == D[:, k:k + 1]).all(0)
    gap = float(s[k] - s[others].max())
    print(f"{what}: best_image_k {k}, gap to the next distinct operating point {gap:.3e}")
    assert gap > 1e-9 * len(recs), \
        (f"{what}: the best and second-best operating points' summed per-image Dice differ by {gap:.3e} <= "
         f"1e-9 * {len(recs)}: the choice depends on the summation order; choose another seed")


@pytest.mark.timeout(300)
def test_trainer_test_curve_and_operating_point_dp2(tmp_path):
    """(c) the curve block and the operating point: chosen on the validation split by global Dice,
    by mean per-image Dice, and given as 0.3 -- three test() calls in one pair of workers."""
    import curve_ref
    import unet_hip
    r0, r1 = _spawn(_eval_body, str(tmp_path), "c")
    for a, b in zip(r0["metrics"], r1["metrics"]):
        assert _same_dicts(a, b), (a, b)
    test, val = _gathered(r0, r1, "test"), _gathered(r0, r1, "val")
    _guard(test)
    _guard(val)
    _image_choice_is_order_free(test, "test split")
    _image_choice_is_order_free(val, "validation split")
    s, vs = _curve_of(test), _curve_of(val)
    alone = [_curve_of(sorted(r["val"], key=lambda v: v["idx"])) for r in (r0, r1)]
    print("validation best_global_k / best_image_k: gathered", vs["best_global_k"], vs["best_image_k"],
          "shards alone", [(a["best_global_k"], a["best_image_k"]) for a in alone])
    for key in ("best_global_k", "best_image_k"):
        assert all(a[key] != vs[key] for a in alone), \
            (f"{key}: a rank's validation shard alone chooses the gathered split's operating point "
             f"({vs[key]}; shards {[a[key] for a in alone]}): a missing all-reduce would not show; choose another seed")
    e = unet_hip.curve_edges(BINS).numpy()
    x, t = np.stack([r["x"] for r in test]), np.stack([r["t"] for r in test])
    for m, k in zip(r0["metrics"], (vs["best_global_k"], vs["best_image_k"], 77)):
        want = _block(sum(r["raw"] for r in test))
        want.update(Curve_AUROC=s["auroc"], Curve_AP=s["ap"], Curve_BestDice=s["best_global_dice"],
                    Curve_BestDiceThreshold=s["best_global_threshold"], Curve_Dice=s["dice_global_half"],
                    Curve_BestImageDice=s["best_image_dice"], Curve_BestImageDiceThreshold=s["best_image_threshold"],
                    Curve_ImageDice=s["dice_image_half"], Curve_Ignored=s["ignored"], Curve_Bins=BINS)
        want.update(_block(curve_ref.counts(x, t, e, k), "OPT_"))
        want["OPT_Threshold"] = k / BINS
        _compare(m, want)
    assert s["planes"] == 7 and s["ignored"] == 0
    text = _log(tmp_path)
    for header, times in (("Test Metrics", 3), ("Curve Metrics", 3), ("Operating point", 3), ("Surface Metrics", 0),
                          ("Post-processed", 0), ("Lesion Metrics", 0), ("TTA (", 0)):
        assert text.count(header) == times, (header, text.count(header))
    assert text.count("Total Images: 7\n") == 3 and text.count("over 7 images") == 3
    for how in ("chosen by val-dice)", "chosen by val-image-dice)", "snapped from 0.3)"):
        assert text.count(how) == 1, how


def _refusal_body(rank, world, tmp):
    tr, _ = _trainer(rank, world, tmp, (TRAIN, VAL, TEST), 3, threshold=0.3, tta="d4")
    try:
        tr.test()
        raised = None
    except ValueError as e:
        raised = str(e)
    # the ranks are still in step: a collective after the refusal pairs up
    v = torch.tensor([float(rank + 1)])
    dist.all_reduce(v)
    return raised, float(v)


@pytest.mark.timeout(300)
def test_threshold_with_tta_is_refused_on_both_ranks(tmp_path):
    r0, r1 = _spawn(_refusal_body, str(tmp_path))
    for raised, v in (r0, r1):
        assert raised is not None and "threshold=0.3" in raised and "tta='d4'" in raised, raised
        assert v == 3.0


# ---------------------------------------------------------------- 3: the boundary term
RATIOS = dict(bce_ratio=1.0, dice_ratio=1.0, focal_ratio=0.5, boundary_ratio=0.7)
SHARDS = {"2+1": (2, 1), "2+2": (2, 2), "1+empty": (1, 0)}
H, W = 32, 48


def _boundary_inputs(n, kind):
    """Fixed random logits; soft targets in the style of test_gpu_boundary._soft_case (sample 0 has
    sites, the others follow the empty-mask rule) or hard {0, 1} masks whose last sample (of
    three or more) is empty."""
    g = torch.Generator().manual_seed(100 * n + (kind == "hard"))
    x = torch.randn(n, 1, H, W, generator=g) * 3
    t = torch.rand(n, 1, H, W, generator=g)
    if kind == "soft":
        t[0, 0, 6:16, 10:33] = 1.0
        t[0, 0, 26:30, 2:5] = 1.5
    else:
        t = (t < torch.linspace(0.02, 0.3, n).reshape(n, 1, 1, 1)).float()
        t[0, 0, 6:16, 10:33] = 1.0
        if n >= 3:
            t[n - 1] = 0.0
    return x, t


def _boundary_body(rank, world, tmp):
    tr, _ = _trainer(rank, world, tmp, ((2, 0), (2, 1), (2, 2)), 2, **RATIOS)
    out = {}
    for name, split in SHARDS.items():
        lo, n = sum(split[:rank]), split[rank]
        for kind in ("soft", "hard"):
            x, t = _boundary_inputs(sum(split), kind)
            for grad in (False, True):
                if n == 0:  # the empty shard joins the step's collectives as _run_epoch does
                    if grad:
                        tr.optimizer.zero_grad(set_to_none=True)
                        tr.ddp.empty_step(2)
                    else:
                        tr.ddp.empty_losses(2)
                    continue
                xs = x[lo:lo + n].to(DEV).requires_grad_(grad)
                with torch.set_grad_enabled(grad):
                    loss, l, lb, total = tr._losses(xs, t[lo:lo + n].to(DEV))
                assert not total.requires_grad and not lb.requires_grad and loss.requires_grad == grad
                if grad:
                    loss.backward()
                    if 0 in split:  # the gradient buckets empty_step() sums on the other rank
                        tr.ddp.reducer.reduce(torch.zeros_like(tr.model._state.param_arena), wait_native=False)
                out[name, kind, grad] = dict(l=l.detach().double().cpu().numpy(), lb=float(lb.double()),
                                             total=float(total.double()),
                                             grad=xs.grad.cpu().numpy() if grad else None)
    return out


def _boundary_reference(x, t):
    """fp64: the three losses and their analytic gradient (loss_ref), the boundary mean over the
    FULL batch and its gradient (the reference's expression over scipy's distance maps)."""
    import loss_ref
    from test_edt_cpu import scipy_dist
    from test_gpu_boundary import _torch_boundary
    w = (RATIOS["bce_ratio"], RATIOS["dice_ratio"], RATIOS["focal_ratio"])
    l = loss_ref.losses(x.numpy(), t.numpy())
    g_seg = loss_ref.dlogits(x.numpy(), t.numpy(), w)
    xr = x.double().requires_grad_(True)
    lb = _torch_boundary(xr, t.double(), torch.from_numpy(scipy_dist(t.numpy())).double())
    lb.backward()
    total = float(np.dot(w, l) + RATIOS["boundary_ratio"] * lb.item())
    return l, lb.item(), total, g_seg, xr.grad.numpy()


@pytest.mark.timeout(300)
def test_losses_boundary_term_is_the_gathered_batch_s(tmp_path):
    """Value and gradient of Trainer._losses under data parallelism: `lb` and `total` are the
    concatenated batch's (rtol 1e-5, atol 1e-6), each rank's logits.grad is its slice of the
    gradient with respect to the gathered logits (norm_rel <= 1e-4), with and without grad; an
    empty shard pairs its collectives through empty_losses(2) / empty_step(2).  On 2 + 1 a weight of
    1 / world in place of n_local / n_global misses both bars (asserted on the host)."""
    from _helpers import norm_rel
    r0, r1 = _spawn(_boundary_body, str(tmp_path))
    rb = RATIOS["boundary_ratio"]
    for name, split in SHARDS.items():
        N = sum(split)
        for kind in ("soft", "hard"):
            l, lb, total, g_seg, g_b = _boundary_reference(*_boundary_inputs(N, kind))
            g_ref = g_seg + rb * g_b
            for grad in (False, True):
                a = r0[name, kind, grad]
                if split[1]:
                    b = r1[name, kind, grad]
                    assert np.array_equal(a["l"], b["l"]) and a["lb"] == b["lb"] and a["total"] == b["total"], (a, b)
                else:
                    assert (name, kind, grad) not in r1
                print(f"{name} {kind} grad={grad}: lb {a['lb']:.9g} vs {lb:.9g}, total {a['total']:.9g} vs {total:.9g}")
                assert np.allclose(a["lb"], lb, rtol=1e-5, atol=1e-6), (name, kind, a["lb"], lb)
                assert np.allclose(a["total"], total, rtol=1e-5, atol=1e-6), (name, kind, a["total"], total)
                assert a["lb"] == r0[name, kind, True]["lb"] and a["total"] == r0[name, kind, True]["total"]
            for rank, res in enumerate((r0, r1)):
                lo, n = sum(split[:rank]), split[rank]
                if n:
                    err = norm_rel(res[name, kind, True]["grad"], g_ref[lo:lo + n])
                    print(f"{name} {kind} rank {rank}: grad norm_rel {err:.3e}")
                    assert err <= 1e-4, (name, kind, rank, err)
            if name == "2+1":  # the local mean weighted by 1 / world: a plausible, wrong, number
                per = [g_b[lo:lo + n] * (N / n) for lo, n in ((0, 2), (2, 1))]  # gradients of the local means
                for (lo, n), gl in zip(((0, 2), (2, 1)), per):
                    assert norm_rel(g_seg[lo:lo + n] + rb * gl / 2, g_ref[lo:lo + n]) > 1e-4
                from test_edt_cpu import scipy_dist
                from test_gpu_boundary import _torch_boundary
                x, t = _boundary_inputs(N, kind)
                d = torch.from_numpy(scipy_dist(t.numpy())).double()
                wrong = sum(float(_torch_boundary(x[s].double(), t[s].double(), d[s])) / 2
                            for s in (slice(0, 2), slice(2, 3)))
                assert not np.allclose(wrong, lb, rtol=1e-5, atol=1e-6), (wrong, lb)


def _boundary_epoch_body(rank, world, tmp):
    tr, _ = _trainer(rank, world, tmp, ((5, 4), (5, 5), (5, 6)), 4, boundary_ratio=0.1)
    seen = []
    log_epoch = tr._log_epoch

    def record(tag, epoch, meters, counts):
        seen.append((tag, [m.avg for m in meters], counts.tolist()))
        return log_epoch(tag, epoch, meters, counts)
    tr._log_epoch = record
    avg = tr.train_one_epoch(0)
    val = tr.validate(0)
    st = tr.model._state
    return dict(seen=seen, avg=avg, val=val, params=st.param_arena.detach().cpu().numpy(),
                bn=st.bn_arena.detach().cpu().numpy())


@pytest.mark.timeout(300)
def test_trainer_dp2_epoch_with_boundary_term(tmp_path):
    """boundary_ratio = 0.1, 5 samples at global batch 4 (2 + 2, then 1 + empty), train then
    validate: no collective mismatch, bit-identical parameters, identical finite meters."""
    r0, r1 = _spawn(_boundary_epoch_body, str(tmp_path))
    assert np.array_equal(r0["params"], r1["params"]), "ranks diverged"
    assert np.array_equal(r0["bn"], r1["bn"]), "validate() left different BN buffers"
    assert r0["seen"] == r1["seen"] and r0["avg"] == r1["avg"] and r0["val"] == r1["val"], (r0["seen"], r1["seen"])
    assert [s[0] for s in r0["seen"]] == ["Train", "Validate"]
    for tag, meters, counts in r0["seen"]:
        assert np.isfinite(meters).all() and meters[3] > 0, (tag, meters)  # the boundary meter moved
        assert sum(counts[:4]) == 5 * 64 * 64
    assert np.isfinite(r0["params"]).all() and np.isfinite(r0["val"]).all()


# ---------------------------------------------------------------- 4: Trainer.train()
def _train_body(rank, world, tmp):
    from models.mod import ResUNet
    tr, _ = _trainer(rank, world, tmp, (TRAIN, VAL, TEST), 3, epochs=4, early_stop_patience=1)
    ran = []
    one = tr.train_one_epoch

    def counted(epoch):
        ran.append(epoch)
        return one(epoch)
    tr.train_one_epoch = counted
    tr.train()
    tr.ddp.sync_buffers()
    st = tr.model._state
    mdir = tr.config.model_dir
    out = dict(ran=ran, stop=tr.early_stopping.early_stop, counter=tr.early_stopping.counter,
               lr=tr.optimizer.param_groups[0]["lr"], files=sorted(os.listdir(mdir)),
               params=st.param_arena.detach().cpu().numpy(), bn=st.bn_arena.detach().cpu().numpy(),
               nbt=st.nbt_arena.cpu().numpy())
    if rank == 0:  # the checkpoint in a fresh module against this rank's eval logits
        x = _dataset(*TEST)[3][0][None].to(DEV)
        tr.model.eval()
        fresh = ResUNet(base_filters=16, depth=3)
        fresh.load_state_dict(torch.load(os.path.join(mdir, "ResUNet_last.pth")))
        fresh = fresh.to(DEV).eval()
        with torch.no_grad():
            own, again = tr.model(x), fresh(x)
        out["reloaded"] = bool(torch.equal(own, again)) and bool(torch.isfinite(own).all())
    return out


@pytest.mark.timeout(300)
def test_trainer_train_dp2(tmp_path):
    """epochs = 4, early_stop_patience = 1 on the ragged splits: both ranks run the same epochs
    and agree on the early-stopping state, the learning rate is the closed form of
    CosineAnnealingWarmRestarts(T_0=20, T_mult=2) after that many steps, parameters and BN buffers
    are the same bits, and rank 0 alone wrote the checkpoints."""
    import math
    r0, r1 = _spawn(_train_body, str(tmp_path))
    n = len(r0["ran"])
    print(f"epochs run {n}, early_stop {r0['stop']}, counter {r0['counter']}, lr {r0['lr']!r}")
    assert r0["ran"] == r1["ran"] == list(range(n)) and 1 <= n <= 4
    assert (r0["stop"], r0["counter"]) == (r1["stop"], r1["counter"])
    assert r0["stop"] == (r0["counter"] >= 1) and (r0["stop"] or n == 4)
    for k in ("params", "bn", "nbt"):
        assert np.array_equal(r0[k], r1[k]), k
    want_lr = 1e-3 * (1 + math.cos(math.pi * n / 20)) / 2
    assert r0["lr"] == r1["lr"] and abs(r0["lr"] - want_lr) <= 1e-12 * want_lr, (r0["lr"], want_lr)
    assert r0["files"] == ["ResUNet_best.pth", "ResUNet_last.pth"] and r1["files"] == []
    assert r0["reloaded"], "_last.pth in a fresh module does not reproduce rank 0's eval logits"
