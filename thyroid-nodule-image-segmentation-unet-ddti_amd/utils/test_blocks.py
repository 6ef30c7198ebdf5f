"""The metric blocks of ``Trainer.test``, one small class each.  A block is constructed only when it is
switched on (and allocates its accumulator on the device); ``add(batch)`` runs once per batch (device calls
only, nothing synchronises); ``finish(total)`` all-reduces, brings the result back in one transfer and
returns ``(message, entries)``: the text to report and the entries of the returned dict.  The device entry
points are looked up on the ``unet_hip`` package when they are called."""
from functools import cached_property

import torch
import torch.distributed as dist

import unet_hip
from unet_hip import functional as F
from utils.utils import global_metrics_from_counts


def distributed():
    return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


def all_reduce(t):
    if distributed():
        dist.all_reduce(t)
    return t


def report(msg, logger, rank0):
    if rank0:
        print(msg)
    logger.info(msg)


def confusion_text(header, m):
    return (f"{header}\n"
            f"  TP={m['TP']}, FP={m['FP']}, FN={m['FN']}, TN={m['TN']}\n"
            f"  ACC={m['ACC']:.4f}, Precision={m['Precision']:.4f}, "
            f"Recall={m['Recall']:.4f}, F1={m['F1']:.4f}, IoU={m['IoU']:.4f}")


def surface_sums(logits, masks):
    """float64[5] on the device: the batch's sums of the per-sample hd95, hd and assd over its
    defined samples, then how many are defined and how many are not (P or G empty)."""
    s = unet_hip.surface_metrics(logits, masks)
    ok = s["defined"] != 0
    zero = torch.zeros_like(s["hd"])
    parts = [torch.where(ok, s[k], zero).sum() for k in ("hd95", "hd", "assd")]
    return torch.stack(parts + [ok.sum().double(), (~ok).sum().double()])


def surface_means(sums, total):
    """The five sums, all-reduced and read in one transfer -> ((hd95, hd, assd, defined), their text)."""
    hd95, hd, assd, k, u = all_reduce(sums).tolist()
    k, u = int(k), int(u)
    hd95, hd, assd = ((v / k if k else float("nan")) for v in (hd95, hd, assd))
    return (hd95, hd, assd, k), (f"HD95={hd95:.4f}, HD={hd:.4f}, ASSD={assd:.4f} px "
                                 f"over {k} of {total} images ({u} undefined)")


def largest_row(x, connectivity, kind):
    """int64 (N, 16): the morphometry row of every sample's largest component (the cc_key rule of
    ``postprocess_mask``: largest area, then first in raster order; zeros for an empty mask), on the
    device with no synchronisation -- the mask of that component alone has one label, so one table
    row holds it."""
    one, _ = unet_hip.postprocess_mask(x, keep_largest=True, connectivity=connectivity, kind=kind)
    return unet_hip.lesion_morphometry(one, connectivity, max_rows=1)["table"][:, 0]


class Switches:
    """The configuration of ``Trainer.test``, read once: which blocks are on, the options more than one of
    them reads, and where they run.  A ``threshold`` with ``tta`` is refused here, before any batch is read."""

    def __init__(self, cfg, device, rt):
        self.device, self.rt = device, rt
        self.surface = bool(getattr(cfg, "surface_metrics", False))
        self.pp = dict(keep_largest=bool(getattr(cfg, "pp_largest", False)),
                       min_area=int(getattr(cfg, "pp_min_area", 0) or 0),
                       fill_holes=bool(getattr(cfg, "pp_fill_holes", False)),
                       connectivity=int(getattr(cfg, "pp_connectivity", 1) or 1))
        self.post = self.pp["keep_largest"] or self.pp["min_area"] > 0 or self.pp["fill_holes"]
        self.lesion = bool(getattr(cfg, "lesion_metrics", False))
        self.shape = bool(getattr(cfg, "lesion_shape", False))
        self.tta = str(getattr(cfg, "tta", None) or "none")
        self.tta_merge = str(getattr(cfg, "tta_merge", None) or "prob")
        self.tta_on = self.tta != "none"
        if self.tta_on:
            self.n_views = len(F.tta_view_numbers(self.tta))
            F.tta_mode(self.tta_merge)
        self.curve = bool(getattr(cfg, "curve_metrics", False))
        self.bins = int(getattr(cfg, "curve_bins", None) or 256)
        self.threshold = getattr(cfg, "threshold", None)
        # opt_k: the operating point; with a criterion the validation split decides it (Trainer.test)
        self.criterion, self.opt_k = F.parse_threshold(self.threshold, self.bins)
        self.opt = self.criterion is not None or self.opt_k is not None
        if self.opt and self.tta_on:
            raise ValueError(f"threshold={self.threshold!r} with tta={self.tta!r}: merging the views at a "
                             "threshold other than 0.5 is not supported; use one of the two")
        if self.curve or self.opt:
            self.edges = unet_hip.curve_edges(self.bins).to(device)
        # under TTA every block past the TTA block reads the merged mask; the lesion and shape blocks label
        # the components of the post-processed mask when there is one (Batch.components)
        self.src = " (TTA mask)" if self.tta_on else ""
        self.components, kind = ("clean", "post-processed") if self.post else ("mask", "raw")
        self.kind = kind + (" TTA" if self.tta_on else "") + " masks"


class Batch:
    """One test batch on the device as the blocks read it: ``images``, ``masks`` (the targets), ``raw`` (the
    plain forward's logits: the first TTA view is the identity), ``mask`` (uint8: the readout of ``raw``,
    which the plain block's ``add`` -- the first -- writes into ``readout``, or the merged TTA mask),
    ``logits`` and ``clean``, both formed when the first block asks for them, and once."""

    def __init__(self, sw, model, images, masks):
        self.sw, self.images, self.masks = sw, images, masks
        if sw.tta_on:
            self.merged = unet_hip.tta_predict(model, images, sw.tta, sw.tta_merge)
            self.raw = self.merged["logits"][:images.size(0)]
        else:
            self.raw = model(images)
        self.readout = torch.empty(self.raw.shape, dtype=torch.uint8, device=sw.device)
        self.mask = self.merged["mask"] if sw.tta_on else self.readout

    @cached_property
    def logits(self):
        """What the readouts downstream read: ``raw``, or the merged mask as +-1 logits, so that every kernel
        reads the mask the merge formed (in "prob" mode the score is a probability, not a logit)."""
        return self.mask.float() * 2 - 1 if self.sw.tta_on else self.raw

    @cached_property
    def clean(self):
        """uint8 (N, H, W): the post-processed mask, or None without a ``pp_*`` option."""
        return unet_hip.postprocess_mask(self.mask, **self.sw.pp)[0] if self.sw.post else None

    @property
    def components(self):
        return getattr(self, self.sw.components)


class Block:
    size, dtype = 6, torch.int64  # the accumulator: the six confusion counts, unless the block says otherwise

    def __init__(self, sw):
        self.sw = sw
        self.acc = torch.zeros(self.size, dtype=self.dtype, device=sw.device)

    def metrics(self):
        return global_metrics_from_counts(all_reduce(self.acc).tolist())


class Plain(Block):
    """The counts of the plain forward; its readout is the mask every block reads without TTA."""

    def add(self, b):
        self.sw.rt.mask_counts(b.raw, b.masks, self.acc, b.readout)

    def finish(self, total):
        m = self.metrics()
        return confusion_text(f"Test Metrics  —  Total Images: {total}", m), m


class TTA(Block):
    """The counts of the merged masks; the pixels the views disagree on (0 < votes < K)."""

    def __init__(self, sw):
        super().__init__(sw)
        self.dis = torch.zeros(1, dtype=torch.int64, device=sw.device)

    def add(self, b):
        self.sw.rt.mask_counts(b.logits, b.masks, self.acc)
        self.dis += ((b.merged["votes"] > 0) & (b.merged["votes"] < self.sw.n_views)).sum()

    def finish(self, total):
        sw, m = self.sw, self.metrics()
        n_dis = int(all_reduce(self.dis).item())  # the one transfer
        n_pix = m["TP"] + m["FP"] + m["FN"] + m["TN"]
        dis = n_dis / n_pix if n_pix else float("nan")
        msg = (confusion_text(f"TTA ({sw.tta}, {sw.tta_merge})", m)
               + f"\n  Disagreement={dis:.4f} ({n_dis} of {n_pix} pixels, {sw.n_views} views)")
        return msg, {**{"TTA_" + k: v for k, v in m.items()}, "TTA_Disagreement": dis}


class Surface(Block):
    size, dtype = 5, torch.float64  # sums of hd95, hd, assd over the defined samples; defined, undefined

    def add(self, b):
        self.acc += surface_sums(b.logits, b.masks)

    def finish(self, total):
        (hd95, hd, assd, k), text = surface_means(self.acc, total)
        return f"Surface Metrics{self.sw.src} — {text}", dict(HD95=hd95, HD=hd, ASSD=assd, SurfaceDefined=k)


class PostProcessed(Block):
    """The same counts and, with ``surface_metrics``, the same sums for the post-processed masks."""

    def __init__(self, sw):
        super().__init__(sw)
        self.sums = torch.zeros(5, dtype=torch.float64, device=sw.device)

    def add(self, b):
        # the cleaned mask as +-1 logits: the existing readout and surface kernels count it
        plog = b.clean[:, None].float() * 2 - 1
        masks = b.masks[:, :1].contiguous()
        self.sw.rt.mask_counts(plog, masks, self.acc)
        if self.sw.surface:
            self.sums += surface_sums(plog, masks)

    def finish(self, total):
        sw, pp, m = self.sw, self.sw.pp, self.metrics()
        msg = confusion_text(f"Post-processed (largest={int(pp['keep_largest'])}, min_area={pp['min_area']}, "
                             f"fill_holes={int(pp['fill_holes'])}, connectivity={pp['connectivity']}){sw.src}", m)
        entries = {"PP_" + k: v for k, v in m.items()}
        if sw.surface:
            (hd95, hd, assd, k), text = surface_means(self.sums, total)
            msg += f"\n  {text}"
            entries.update(PP_HD95=hd95, PP_HD=hd, PP_ASSD=assd, PP_SurfaceDefined=k)
        return msg, entries


class Lesion(Block):
    size = 4  # n_pred, n_gt, gt_hit, pred_hit over the test set

    def add(self, b):
        les = unet_hip.lesion_metrics(b.components, b.masks, self.sw.pp["connectivity"])
        self.acc += torch.stack([les[k].sum() for k in F.LESION_FIELDS])

    def finish(self, total):
        n_pred, n_gt, gt_hit, pred_hit = all_reduce(self.acc).tolist()  # the one transfer
        nan = float("nan")
        rec = gt_hit / n_gt if n_gt else nan
        prec = pred_hit / n_pred if n_pred else nan
        fpc = (n_pred - pred_hit) / total if total else nan
        msg = (f"Lesion Metrics ({self.sw.kind}, connectivity {self.sw.pp['connectivity']}) — "
               f"Recall={rec:.4f} ({gt_hit}/{n_gt}), Precision={prec:.4f} "
               f"({pred_hit}/{n_pred}), FP components/image={fpc:.4f}")
        return msg, dict(LesionRecall=rec, LesionPrecision=prec, FPComponentsPerImage=fpc,
                         PredComponents=n_pred, GTComponents=n_gt)


class Curve:
    """The threshold sweep's accumulators: the histogram rows + ignored pixels, the Dice sums, the planes."""

    def __init__(self, sw):
        self.sw, self.planes = sw, 0
        self.total = torch.zeros(2 * sw.bins + 1, dtype=torch.int64, device=sw.device)
        self.dice = torch.zeros(sw.bins + 1, dtype=torch.float64, device=sw.device)

    def add_logits(self, logits, masks):
        """One histogram and one statistics call on the batch's channel-0 planes."""
        ph, _ = unet_hip.curve_hist(logits[:, :1], masks[:, :1], self.sw.edges, self.total)
        unet_hip.curve_stats(ph, self.dice)
        self.planes += logits.shape[0]

    def add(self, b):  # (no TTA with a threshold; under TTA `raw` is the first view's logits)
        self.add_logits(b.raw, b.masks)

    def sweep(self, model, loader):
        """The sweep over a loader in eval mode (the caller has synchronised the BN buffers)."""
        for batch in loader:
            if batch is not None:  # (None: an empty DataParallel shard)
                images, masks = batch
                logits = model(images.to(self.sw.device).float())
                self.add_logits(logits, masks.to(self.sw.device).float())
        return self

    def summary(self):
        """All-reduce the accumulators, bring them back in one transfer, read the curves."""
        ints = torch.cat([self.total, torch.tensor([self.planes], dtype=torch.int64, device=self.sw.device)])
        all_reduce(ints)
        all_reduce(self.dice)
        back = torch.cat([ints, self.dice.view(torch.int64)]).cpu()  # the one transfer
        n = ints.numel()
        return unet_hip.curve_summary(back[:n - 1].tolist(), back[n:].view(torch.float64).tolist(),
                                      int(back[n - 1]), self.sw.edges)

    def finish(self, total):
        cs, bins = self.summary(), self.sw.bins
        msg = (f"Curve Metrics ({bins} bins) — AUROC={cs['auroc']:.4f}, AP={cs['ap']:.4f}\n"
               f"  Best global Dice={cs['best_global_dice']:.4f} at threshold {cs['best_global_threshold']:.4f} "
               f"(Dice at 0.5: {cs['dice_global_half']:.4f})\n"
               f"  Best mean per-image Dice={cs['best_image_dice']:.4f} at threshold "
               f"{cs['best_image_threshold']:.4f} (at 0.5: {cs['dice_image_half']:.4f}) over {cs['planes']} images\n"
               f"  Ignored pixels={cs['ignored']}")
        return msg, dict(Curve_AUROC=cs["auroc"], Curve_AP=cs["ap"], Curve_BestDice=cs["best_global_dice"],
                         Curve_BestDiceThreshold=cs["best_global_threshold"], Curve_Dice=cs["dice_global_half"],
                         Curve_BestImageDice=cs["best_image_dice"],
                         Curve_BestImageDiceThreshold=cs["best_image_threshold"],
                         Curve_ImageDice=cs["dice_image_half"], Curve_Ignored=cs["ignored"], Curve_Bins=bins)


class OperatingPoint(Block):
    """The counts of the mask of operating point ``opt_k``, as +-1 logits for the same readout."""

    def add(self, b):
        om = F.curve_predict(b.raw[:, :1], self.sw.opt_k, self.sw.edges)
        self.sw.rt.mask_counts(om.float() * 2 - 1, b.masks[:, :1].contiguous(), self.acc)

    def finish(self, total):
        sw, m = self.sw, self.metrics()
        how = f"chosen by {sw.criterion}" if sw.criterion else f"snapped from {float(sw.threshold):g}"
        msg = confusion_text(f"Operating point — threshold {sw.opt_k / sw.bins:.6f} "
                             f"(k={sw.opt_k} of {sw.bins}, {how})", m)
        return msg, {**{"OPT_" + k: v for k, v in m.items()}, "OPT_Threshold": sw.opt_k / sw.bins}


class Shape:
    """Per batch: the table rows of the largest predicted and the largest annotated component."""

    def __init__(self, sw):
        self.sw, self.rows = sw, []

    def add(self, b):
        c = self.sw.pp["connectivity"]
        self.rows.append(torch.cat([largest_row(b.components, c, None), largest_row(b.masks, c, "targets")], 1))

    def finish(self, total):
        rows = (torch.cat(self.rows) if self.rows else torch.zeros((0, 32), dtype=torch.int64)).cpu()  # the one transfer
        sums = torch.from_numpy(F.shape_agreement(rows[:, :16], rows[:, 16:]))
        if distributed():
            sums = all_reduce(sums.to(self.sw.device))
        sh = F.shape_summary(sums.tolist())
        msg = (f"SHAPE (largest component, {self.sw.kind}, connectivity {self.sw.pp['connectivity']}) — "
               f"pairs={sh['n_pairs']} of {total} images\n"
               f"  Feret MAE={sh['feret_mae']:.4f} px, area rel. error={sh['area_rel_err']:.4f}, "
               f"centroid distance={sh['centroid_dist']:.4f} px\n"
               f"  taller-than-wide (pred/gt): both={sh['ttw'][0]}, pred only={sh['ttw'][1]}, "
               f"gt only={sh['ttw'][2]}, neither={sh['ttw'][3]}, kappa={sh['kappa']:.4f}")
        return msg, dict(Shape_Pairs=sh["n_pairs"], Shape_FeretMAE=sh["feret_mae"], Shape_AreaRelErr=sh["area_rel_err"],
                         Shape_CentroidDist=sh["centroid_dist"], Shape_TTW=sh["ttw"], Shape_TTWKappa=sh["kappa"])
