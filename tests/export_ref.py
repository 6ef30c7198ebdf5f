"""NumPy restatement of the predict-mode export rules (written from the rules, not from csrc/export.h):
Pillow's float BILINEAR plan and its two passes in float64 with a float32 intermediate, the two
threshold kinds, the city-block contour, the integer overlay and the mask statistics."""
import math

import numpy as np

SIGMOID, GREATER = "sigmoid", "greater"


def plan(n_in, n_out):
    """coeffs float64 (out, ksize), bounds int32 (out, 2) = {first, count}."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    ksize = 2 * int(math.ceil(support)) + 1
    inv = 1.0 / fs
    k = np.zeros((n_out, ksize), np.float64)
    b = np.zeros((n_out, 2), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * inv)) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k[xx, :xmax] = w
        b[xx] = (xmin, xmax)
    return k, b


def _pass_rows(a, n_out):
    """Resample the last axis of float32 a to n_out: float64 sums in ascending tap order (NumPy's
    float64 multiply and add round separately), stored as float32."""
    k, b = plan(a.shape[-1], n_out)
    out = np.empty(a.shape[:-1] + (n_out,), np.float32)
    a64 = a.astype(np.float64)
    for xx in range(n_out):
        first, count = b[xx]
        ss = np.zeros(a.shape[:-1], np.float64)
        for t in range(count):
            ss = ss + a64[..., first + t] * k[xx, t]
        out[..., xx] = ss.astype(np.float32)
    return out


def resize(a, oh, ow):
    """float32 (h, w) -> (oh, ow): horizontal pass first, an unchanged axis skipped."""
    a = np.ascontiguousarray(a, np.float32)
    if ow != a.shape[1]:
        a = _pass_rows(a, ow)
    if oh != a.shape[0]:
        a = np.ascontiguousarray(_pass_rows(np.ascontiguousarray(a.T), oh).T)
    return a


def threshold(plane, kind, thr=0.5):
    """uint8 {0, 1}.  The sigmoid kind is float32 1 / (1 + exp(-v)) > 0.5; within |v| < 2^-20 the
    result depends on the last bit of expf, so compare there with ``sigmoid_band``."""
    if kind == GREATER:
        return (plane > np.float32(thr)).astype(np.uint8)
    with np.errstate(over="ignore"):
        s = np.float32(1) / (np.float32(1) + np.exp(-plane.astype(np.float32)))
    return (s > np.float32(0.5)).astype(np.uint8)


def sigmoid_band(plane):
    return np.abs(plane) < 2.0 ** -20


def contour(mask, r):
    """bool: foreground pixels with a background or outside pixel at city-block distance <= r."""
    fg = mask != 0
    h, w = fg.shape
    pad = np.zeros((h + 2 * r, w + 2 * r), bool)
    pad[r:r + h, r:r + w] = fg
    inner = np.ones((h, w), bool)
    for dy in range(-r, r + 1):
        for dx in range(-(r - abs(dy)), r - abs(dy) + 1):
            inner &= pad[r + dy:r + dy + h, r + dx:r + dx + w]
    return fg & ~inner


_CONTOURS = {}


def _contour_once(mask, r):
    """contour(mask, r), computed once per (plane, r): the overlay cases ask for it at every alpha."""
    key = (id(mask), r)
    if key not in _CONTOURS or _CONTOURS[key][0] is not mask:
        _CONTOURS[key] = (mask, contour(mask, r))
    return _CONTOURS[key][1]


def overlay(gray, pred, gt=None, r=1, alpha=0):
    """(rgb uint8 (h, w, 3), stats list of 6 ints)."""
    g = gray.astype(np.int32)
    rgb = np.stack([g, g, g], -1)
    fg = pred != 0
    cp = _contour_once(pred, r)
    interior = fg & ~cp
    if alpha:
        for c, col in enumerate((255, 0, 0)):
            rgb[..., c] = np.where(interior, (g * (256 - alpha) + col * alpha + 128) >> 8, rgb[..., c])
    if gt is not None:
        rgb[_contour_once(gt, r)] = (0, 0, 255)
    rgb[cp] = (255, 0, 0)
    ys, xs = np.nonzero(fg)
    if ys.size:
        stats = [int(fg.sum()), int(cp.sum()), int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]
    else:
        stats = [0, 0, -1, -1, -1, -1]
    return rgb.astype(np.uint8), stats


# ---- shared cases ----
RESIZE_SHAPES = [(16, 16, 23, 37), (16, 16, 7, 5), (16, 16, 16, 31), (16, 16, 31, 16), (16, 16, 16, 16),
                 (48, 48, 360, 560), (16, 16, 1, 1), (16, 16, 1, 40)]  # (h, w, oh, ow)


def score_plane(h, w, seed):
    """Finite normal-distributed scores scaled by 6."""
    return (np.random.default_rng(seed).standard_normal((h, w)) * 6).astype(np.float32)


def overlay_cases(tile_h, tile_w):
    """name -> (gray, pred, gt) uint8 planes: the edge masks at 5 x 7, one tile + 1 in each direction
    and 360 x 560.  gt overlaps pred's contour (pred shifted by one pixel)."""
    rng = np.random.default_rng(7)
    cases = {}
    for h, w in ((5, 7), (tile_h + 1, tile_w + 1), (360, 560)):
        yy, xx = np.mgrid[0:h, 0:w]
        masks = {
            "empty": np.zeros((h, w), bool),
            "full": np.ones((h, w), bool),
            "corner": (yy == h - 1) & (xx == w - 1),
            "disc": (yy - h / 2) ** 2 + (xx - w / 2.5) ** 2 <= (min(h, w) / 3) ** 2,
            "vstripes": xx % 3 == 0,
            "hstripes": yy % 3 != 1,
            "line": yy == h // 2,
        }
        for name, m in masks.items():
            gray = rng.integers(0, 256, (h, w), dtype=np.uint8)
            gt = np.roll(m, 1, axis=1) | np.roll(m, 1, axis=0)  # overlapping contours
            cases[f"{name}_{h}x{w}"] = (gray, m.astype(np.uint8) * 255, gt.astype(np.uint8))
    return cases
