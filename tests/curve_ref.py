"""The threshold sweep restated in NumPy, independently of csrc/curve.h, and the cases its tests share.

Bin: ``np.searchsorted(edges, x, side="left")`` (the number of edges below x), NaN sent to bin 0.
Class: the integer cast of the target, its low byte: 1 positive, 0 negative, anything else ignored.
Operating point k in 0..B: predicted positive iff bin >= k, counted here DIRECTLY on the raw arrays
with ``x > e[k-1]`` (everything for k = 0, nothing for k = B).  AUROC numerator: the Mann-Whitney
count on the binned scores, a tie counted once and a win twice."""
import functools

import numpy as np

BINS = (2, 16, 256, 1024)
FIELDS = ("P", "Nn", "best_k", "TP", "FP", "FN", "auc2")


def edges(B):
    """The formula of the standard edges in float64 NumPy, rounded to float32."""
    t = (np.arange(B - 1, dtype=np.float64) + 1) / B
    return np.log(t / (1 - t)).astype(np.float32)


def classes(t):
    u = t.astype(np.int64) & 0xFF
    return u == 1, u == 0


def bins_of(x, e):
    b = np.searchsorted(e, x, side="left")
    return np.where(np.isnan(x), 0, b)


def hist(x, t, e):
    """x, t (planes, hw) -> plane_hist int32 (planes, 2, B), total int64 (2 B + 1)."""
    B = e.size + 1
    pos, neg = classes(t)
    b = bins_of(x, e)
    h = np.zeros((x.shape[0], 2, B), np.int64)
    p = np.broadcast_to(np.arange(x.shape[0])[:, None], x.shape)
    np.add.at(h, (p[neg], 0, b[neg]), 1)
    np.add.at(h, (p[pos], 1, b[pos]), 1)
    total = np.concatenate([h.sum(0).reshape(-1), [x.size - pos.sum() - neg.sum()]]).astype(np.int64)
    return h.astype(np.int32), total


def predict(x, e, k):
    B = e.size + 1
    if k == 0:
        return np.ones(x.shape, bool)
    if k == B:
        return np.zeros(x.shape, bool)
    return x > e[k - 1]


def counts(x, t, e, k):
    """TP, FP, FN, TN at operating point k, counted on the raw arrays."""
    pos, neg = classes(t)
    pr = predict(x, e, k)
    return (int((pr & pos).sum()), int((pr & neg).sum()), int((~pr & pos).sum()), int((~pr & neg).sum()))


def best(values):
    B = len(values) - 1
    order = sorted(range(B + 1), key=lambda k: (-values[k], abs(k - B // 2), k))
    return order[0]


def dice_curve(x, t, e):
    """[dice_k for k in 0..B] of one plane (or of everything given) as float64, and the counts."""
    B = e.size + 1
    out, cs = [], []
    for k in range(B + 1):
        tp, fp, fn, _ = counts(x, t, e, k)
        den = 2 * tp + fp + fn
        out.append(np.float64(1.0) if den == 0 else np.float64(2 * tp) / np.float64(den))
        cs.append((tp, fp, fn))
    return out, cs


def auc2(x, t, e):
    pos, neg = classes(t)
    b = bins_of(x, e)
    nb = np.sort(b[neg])
    return int(np.searchsorted(nb, b[pos], side="left").sum() + np.searchsorted(nb, b[pos], side="right").sum())


def stats(x, t, e, dice_sum=None):
    """-> out_i64 (planes, 8) and dice_sum float64 (B + 1), the planes added in ascending order."""
    B = e.size + 1
    out = np.zeros((x.shape[0], 8), np.int64)
    ds = np.zeros(B + 1, np.float64) if dice_sum is None else dice_sum.copy()
    for p in range(x.shape[0]):
        d, cs = dice_curve(x[p], t[p], e)
        k = best(d)
        pos, neg = classes(t[p])
        out[p, :7] = (pos.sum(), neg.sum(), k, cs[k][0], cs[k][1], cs[k][2], auc2(x[p], t[p], e))
        for j in range(B + 1):
            ds[j] = ds[j] + d[j]
    return out, ds


def summary(x, t, e):
    """AUROC, AP and the two Dice curves of every plane of x together, by direct counts."""
    B = e.size + 1
    pos, neg = classes(t)
    P, Nn = int(pos.sum()), int(neg.sum())
    dg, cs = dice_curve(x, t, e)
    tp = [c[0] for c in cs] + [0]
    prec = [c[0] / (c[0] + c[1]) if c[0] + c[1] else 1.0 for c in cs]
    per = np.zeros(B + 1, np.float64)
    for p in range(x.shape[0]):
        d, _ = dice_curve(x[p], t[p], e)
        for j in range(B + 1):
            per[j] = per[j] + d[j]
    per = [float(v) / x.shape[0] for v in per]
    return dict(auroc=auc2(x, t, e) / (2 * P * Nn) if P and Nn else float("nan"),
                ap=sum((tp[k] - tp[k + 1]) / P * prec[k] for k in range(B)) if P else float("nan"),
                dice_global=[float(v) for v in dg], dice_image=per, best_global_k=best(dg), best_image_k=best(per),
                ignored=int(x.size - P - Nn))


# ---------------------------------------------------------------- cases
def _blob(h, w, cy, cx, ry, rx):
    y, x = np.mgrid[:h, :w]
    return ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1


def _scene(r, planes, h, w):
    """Logits around a blob target: confident background, a softer inside, a noisy rim."""
    t = np.stack([_blob(h, w, h * (0.3 + 0.1 * p % 0.4), w * 0.5, h * 0.2, w * (0.15 + 0.03 * p)) for p in range(planes)])
    x = np.where(t, 3.0, -7.0) + r.normal(0, 1.5, t.shape) * np.where(t, 1.5, 0.6)
    return x.reshape(planes, -1).astype(np.float32), t.reshape(planes, -1).astype(np.float32)


def small_cases(B, e):
    """name -> (x, t, offset): float32 (planes, hw) arrays; offset > 0 asks for a view taken that many
    floats into a buffer.  e: the edges in use (the values case sits on them)."""
    r = np.random.default_rng(B)
    c = {}
    c["single_pixel_1x1"] = (np.array([[0.7]], np.float32), np.array([[1.0]], np.float32), 0)
    for name, (planes, h, w) in (("scalar_tail_2x3x5", (2, 3, 5)), ("aligned_3x64x64", (3, 64, 64)),
                                 ("unaligned_2x7x333", (2, 7, 333))):
        c[name] = (*_scene(r, planes, h, w), 0)
    c["offset_view_1x130x67"] = (*_scene(r, 1, 130, 67), 1)
    x, t = _scene(r, 4, 32, 32)
    c["one_bin_4x32x32"] = (np.full_like(x, -9.0), t, 0)
    t2 = t.copy()
    t2[0], t2[1] = 0.0, 1.0
    c["one_class_planes_4x32x32"] = (x, t2, 0)
    tiny = np.float32(1e-45)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, tiny, -tiny, 1e-39, -1e-39, 5e-8, -5e-8], np.float32)
    vals = np.concatenate([e, np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf)), special])
    alt = (np.arange(vals.size) % 2).astype(np.float32)
    c["values_on_the_edges"] = (np.stack([vals, vals]), np.stack([alt, 1 - alt]), 0)
    x, _ = _scene(r, 2, 25, 40)
    c["target_values_2x25x40"] = (x, r.choice(np.array([0, 1, 0.3, 1.5, 2, 255], np.float32), x.shape), 0)
    return c


@functools.lru_cache(maxsize=None)
def big_case():
    """8 x 512 x 512: the realistic skew (most pixels confident background)."""
    return _scene(np.random.default_rng(99), 8, 512, 512)
