"""Predict mode: frames without masks in, source-size masks and contour overlays out, all on the
device (``main.py --mode predict``; the picture side of it is what the reference plots with
matplotlib and scikit-image at utils/trainer.py:262-299).

    pred = Predictor(model, 512, "cuda", tta="flips", pp=dict(keep_largest=True))
    out = pred(planes)                  # a list of (h, w) uint8 frames of any sizes
    out["masks"][i], out["overlays"][i], out["rows"][i]

Per batch: ``GpuResizeToTensor`` to the network resolution, the forward (or ``tta_predict``), then
per frame ``resize_back`` of its score plane to the frame's own (h, w) with the threshold fused in,
the optional ``postprocess_mask`` there, ``overlay`` on the frame itself and a connected-component
count.  Nothing comes back to the host but one row of seven integers per frame, in one transfer.
With ``lesion_table=True`` the labels of that count are kept, the frames of one size share one
``morphometry_table`` call, and the sixteen integers of every component come back in a second transfer
(``out["lesions"]``, the rows of lesions.csv).  With ``lesion_echo=True`` too, the same groups go with
the frames' own grey planes through one ``echo_table`` call each, and the histograms and co-occurrence
counts of every component come back in one more transfer (``out["echo"]``, the echo columns of
lesions.csv).
"""
import numpy as np
import torch

from . import functional as F
from .data import GpuResizeToTensor

CSV_HEADER = ("name", "h", "w", "area", "area_fraction", "x0", "y0", "x1", "y1", "components")
ROW_FIELDS = F.OVERLAY_FIELDS + ("components",)


def csv_row(name, row):
    """One line of predictions.csv (no newline) for a row of ``Predictor``: the CSV_HEADER columns,
    the area fraction with six decimals, the inclusive box (-1 four times for an empty mask)."""
    frac = row["area"] / (row["h"] * row["w"])
    return ",".join([str(name), str(row["h"]), str(row["w"]), str(row["area"]), f"{frac:.6f}",
                     str(row["x0"]), str(row["y0"]), str(row["x1"]), str(row["y1"]), str(row["components"])])


def gray_u8(images):
    """The uint8 gray planes (N, H, W) of a float batch (N, C, H, W) in [0, 1] (channel 0): the bytes
    ToTensor divided by 255, recovered exactly by rounding."""
    return (images[:, 0].detach().float().clamp(0, 1) * 255 + 0.5).to(torch.uint8)


def check_predict_options(tta, threshold):
    """The combinations predict mode refuses, as ValueError: a validation-chosen threshold (there is
    no labelled split) and a threshold other than 0.5 under test-time augmentation (as
    ``Trainer.test`` refuses it).  Returns the operating point k, or None for the plain 0.5 readout."""
    if isinstance(threshold, str) and threshold in F.THRESHOLD_CRITERIA:
        raise ValueError(f"threshold={threshold!r} needs a labelled validation split; predict mode has none "
                         "(pass a number)")
    _, k = F.parse_threshold(threshold)
    if k is not None and str(tta or "none") != "none":
        raise ValueError(f"threshold={threshold!r} with tta={tta!r}: merging the views at a threshold other "
                         "than 0.5 is not supported; use one of the two")
    return k


class Predictor:
    def __init__(self, model, image_size, device, tta="none", tta_merge="prob", threshold=0.5, pp=None, width=1,
                 alpha=0, bins=256, lesion_table=False, lesion_echo=False, echo_ring=8, echo_levels=16):
        self.device = torch.device(device)
        self.model = model.to(self.device).eval()
        self.pipe = GpuResizeToTensor(image_size, self.device)
        self.tta = str(tta or "none")
        self.tta_merge = str(tta_merge or "prob")
        if self.tta != "none":
            F.tta_view_mask(self.tta)
            F._tta_mode(self.tta_merge)
        check_predict_options(self.tta, threshold)
        _, k = F.parse_threshold(threshold, bins)
        # how the score plane is read: logits through the sigmoid readout, a merged probability
        # against 0.5, or logits against the edge of operating point k (curve_predict: x > e[k - 1])
        if self.tta != "none" and self.tta_merge == "prob":
            self.kind, self.thr = "greater", 0.5
        elif k is not None:
            self.kind, self.thr = "greater", float(F.curve_edges(bins)[k - 1])
        else:
            self.kind, self.thr = "sigmoid", 0.5
        pp = dict(pp or {})
        self.pp = dict(keep_largest=bool(pp.get("keep_largest", False)), min_area=int(pp.get("min_area", 0) or 0),
                       fill_holes=bool(pp.get("fill_holes", False)), connectivity=int(pp.get("connectivity", 1) or 1))
        self.post = self.pp["keep_largest"] or self.pp["min_area"] > 0 or self.pp["fill_holes"]
        self.width, self.alpha = int(width), int(alpha)
        self.lesion_table = bool(lesion_table)
        self.lesion_echo = bool(lesion_echo)
        if self.lesion_echo and not self.lesion_table:
            raise ValueError("lesion_echo=True adds columns to the lesion table; pass lesion_table=True too")
        if echo_levels not in F.ECHO_LEVELS:
            raise ValueError(f"echo_levels must be one of {F.ECHO_LEVELS}, got {echo_levels!r}")
        if not isinstance(echo_ring, int) or isinstance(echo_ring, bool) or not 0 <= echo_ring <= F.ECHO_MAX_RING:
            raise ValueError(f"echo_ring must be an int in 0..{F.ECHO_MAX_RING}, got {echo_ring!r}")
        self.echo_ring, self.echo_levels = int(echo_ring), int(echo_levels)

    def _forward(self, gray, planes):
        """(N, S, S) float32: the score planes at the network resolution of the uploaded frames
        ``gray`` (``planes`` still carry the decoder's resample tags)."""
        x = torch.empty((len(gray), 1, self.pipe.oh, self.pipe.ow), dtype=torch.float32, device=self.device)
        for i, g in enumerate(gray):
            self.pipe.resize(g, x[i, 0], nearest=getattr(planes[i], "resample", "bilinear") == "nearest")
        if self.tta != "none":
            return F.tta_predict(self.model, x, self.tta, self.tta_merge)["score"][:, 0].contiguous()
        return self.model(x).detach().float()[:, 0].contiguous()

    def _lesions(self, labels, counts, grays=None):
        """Per frame the int64 (count, 16) table rows on the host: the frames of one size are one
        ``morphometry_table`` call (max_rows their largest count), all tables one transfer.  With the
        frames' grey planes ``grays``, a second list too: per frame the int32 (count, 512 + G^2)
        ``echo_table`` rows, the same groups one call each and all of them one more transfer."""
        groups = {}
        for i, (lab, _) in enumerate(labels):
            if counts[i] > 0:
                groups.setdefault(tuple(lab.shape[1:]), []).append(i)
        width = 512 + self.echo_levels ** 2
        flat, flat_e, where = [], [], {}
        for idx in groups.values():
            rows = max(counts[i] for i in idx)
            lab, cnt = torch.cat([labels[i][0] for i in idx]), torch.cat([labels[i][1] for i in idx])
            tab = F.morphometry_table(lab, cnt, rows)
            if grays is not None:
                etab = F.echo_table(torch.stack([grays[i] for i in idx]), lab, cnt, rows, self.echo_levels,
                                    self.echo_ring)
            for j, i in enumerate(idx):
                where[i] = (sum(t.shape[0] for t in flat), counts[i])
                flat.append(tab[j, :counts[i]])
                if grays is not None:
                    flat_e.append(etab[j, :counts[i]])
        back = torch.cat(flat).cpu() if flat else torch.zeros((0, 16), dtype=torch.int64)  # the one transfer
        empty = torch.zeros((0, 16), dtype=torch.int64)
        cut = lambda t, e: [t[where[i][0]:where[i][0] + where[i][1]] if i in where else e for i in range(len(labels))]
        if grays is None:
            return cut(back, empty)
        back_e = torch.cat(flat_e).cpu() if flat_e else torch.zeros((0, width), dtype=torch.int32)  # one more
        return cut(back, empty), cut(back_e, torch.zeros((0, width), dtype=torch.int32))

    @torch.no_grad()
    def scores(self, planes):
        """(N, S, S) float32: the score planes of the frames at the network resolution."""
        return self._forward([self.pipe.upload(im) for im in planes], planes)

    @torch.no_grad()
    def __call__(self, planes, return_scores=False):
        """planes: a list of (h, w) uint8 frames (arrays or tensors, any sizes).  Returns a dict of
        lists, one entry per frame: ``masks`` (uint8 (h, w) in {0, 1}), ``overlays`` (uint8 (h, w, 3)),
        ``scores`` (float32 (h, w), when asked), all on the device, and ``rows`` (dicts of Python ints:
        h, w, area, contour, x0, y0, x1, y1, components).  Every frame is uploaded once.  With
        ``lesion_table``, ``lesions`` too: per frame the int64 (components, 16) rows of
        ``morphometry_table`` on the host, and with ``lesion_echo`` ``echo``: per frame the int32
        (components, 512 + echo_levels^2) rows of ``echo_table`` of the frame's own grey plane and the
        labels of its final mask, on the host."""
        grays = [self.pipe.upload(im) for im in planes]
        score = self._forward(grays, planes)
        masks, overlays, planes_out, stats, labels = [], [], [], [], []
        for i, gray in enumerate(grays):
            h, w = gray.shape
            out = F.resize_back(score[i], (h, w), self.kind, self.thr, return_plane=return_scores)
            mask, sc = out if return_scores else (out, None)
            if self.post:
                mask = F.postprocess_mask(mask, **self.pp)[0][0]
            rgb, st = F.overlay(gray, mask, None, self.width, self.alpha)
            lab, count = F.connected_components(mask, self.pp["connectivity"])
            if self.lesion_table:
                labels.append((lab, count))
            masks.append(mask)
            overlays.append(rgb)
            planes_out.append(sc)
            stats.append(torch.cat([st, count.to(torch.int64)]))
        back = torch.stack(stats).cpu().tolist() if stats else []  # the one transfer
        rows = []
        for m, r in zip(masks, back):
            row = dict(h=int(m.shape[0]), w=int(m.shape[1]))
            row.update(zip(ROW_FIELDS, (int(v) for v in r)))
            rows.append(row)
        out = dict(masks=masks, overlays=overlays, rows=rows)
        if self.lesion_echo:
            out["lesions"], out["echo"] = self._lesions(labels, [r["components"] for r in rows], grays)
        elif self.lesion_table:
            out["lesions"] = self._lesions(labels, [r["components"] for r in rows])
        if return_scores:
            out["scores"] = planes_out
        return out


def lesion_lines(out, names, pixel_spacing=None, connectivity=1):
    """The lines of lesions.csv (no header) for what a ``Predictor`` with ``lesion_table`` returned for
    the frames ``names``: one per component, none for an empty mask (``F.lesion_csv_lines``); with the
    echo columns when the ``Predictor`` had ``lesion_echo``."""
    import os
    lines = []
    echo = out.get("echo") or [None] * len(names)
    for name, tab, e in zip(names, out["lesions"], echo):
        lines += F.lesion_csv_lines(os.path.basename(name), tab, tab.shape[0], pixel_spacing, connectivity, e)
    return lines


def lesion_csv_header(pixel_spacing=None, echo=False):
    return (F.LESION_COLUMNS + (F.LESION_COLUMNS_MM if pixel_spacing is not None else ())
            + (F.LESION_COLUMNS_ECHO if echo else ()))


def save_predictions(out, names, output_dir, save_scores=False):
    """Write what ``Predictor`` returned for the frames ``names``: <stem>_mask.png (mode L, 0 / 255),
    <stem>_overlay.png (RGB) and, with ``save_scores``, <stem>_score.npy.  Returns the CSV lines."""
    import os

    from PIL import Image
    lines = []
    for i, name in enumerate(names):
        stem = os.path.splitext(os.path.basename(name))[0]
        Image.fromarray(out["masks"][i].cpu().numpy() * np.uint8(255), "L").save(
            os.path.join(output_dir, f"{stem}_mask.png"))
        Image.fromarray(out["overlays"][i].cpu().numpy(), "RGB").save(os.path.join(output_dir, f"{stem}_overlay.png"))
        if save_scores:
            np.save(os.path.join(output_dir, f"{stem}_score.npy"), out["scores"][i].cpu().numpy())
        lines.append(csv_row(os.path.basename(name), out["rows"][i]))
    return lines
