"""The oracle and the extra inputs of the lesion-morphometry tests (test_morph_cpu.py,
test_gpu_morph.py): a NumPy / scipy restatement of the sixteen integers per component that
``unet_morphometry`` writes (csrc/morph.h).  Every comparison against it is exact.

Per label: sums over the boolean mask of the component, the box from ``np.where``, the bit quads from
four shifted views of the zero-padded indicator, and d2max by brute force over all pixel pairs of a
small component.  A large component's farthest pair is taken with ``scipy.spatial.distance.pdist``
over its contour pixels (a farthest pair never has an interior pixel: moving it outwards along the
pair's line stays inside the component's 4-neighbourhood and lengthens the pair), thinned to the
vertices of their convex hull when the contour itself is long (the farthest pair of a point set
are hull vertices)."""
import numpy as np
import scipy.ndimage as nd
from scipy.spatial import ConvexHull, QhullError
from scipy.spatial.distance import pdist

import cc_ref

FIELDS = ("area", "sx", "sy", "sxx", "sxy", "syy", "x0", "y0", "x1", "y1", "q1", "q2", "qd", "q3", "d2max", "first")
BRUTE_PIXELS = 1500   # all pairs up to here
PDIST_POINTS = 3000   # pdist over the contour up to here, over its hull beyond


def quads(ind):
    """(q1, q2, qd, q3) of a bool (h, w) indicator: the (h + 1) (w + 1) windows of its zero padding."""
    p = np.pad(np.asarray(ind, bool), 1).astype(np.int64)
    a, b, c, d = p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:]
    s = a + b + c + d
    diag = (s == 2) & (a == d)
    return int((s == 1).sum()), int(((s == 2) & ~diag).sum()), int(diag.sum()), int((s == 3).sum())


def contour(ind):
    """The pixels of ind with a 4-neighbour outside it (the plane's border counts as outside)."""
    p = np.pad(np.asarray(ind, bool), 1)
    inner = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return ind & ~inner


def d2max(ind):
    """max dx^2 + dy^2 over the pixel pairs of a bool (h, w) indicator, exactly."""
    ys, xs = np.nonzero(ind)
    if ys.size > BRUTE_PIXELS:
        ys, xs = np.nonzero(contour(ind))
    if ys.size <= BRUTE_PIXELS:
        dx, dy = xs[:, None] - xs[None, :], ys[:, None] - ys[None, :]
        return int((dx * dx + dy * dy).max())
    pts = np.stack([xs, ys], 1).astype(np.float64)
    if len(pts) > PDIST_POINTS:
        try:
            pts = pts[ConvexHull(pts).vertices]
        except QhullError:  # collinear: the two ends
            pts = pts[[np.lexsort((ys, xs))[0], np.lexsort((ys, xs))[-1]]]
    return int(round(pdist(pts, "sqeuclidean").max()))  # integers below 2^53: exact in float64


def table(lab, max_rows=None):
    """int64 (max_rows, 16) of one int32 (H, W) label plane whose labels are 1..K (K = lab.max());
    max_rows defaults to max(K, 1).  Rows beyond K are zero, labels beyond max_rows dropped."""
    lab = np.asarray(lab)
    H, W = lab.shape
    K = int(lab.max()) if lab.size else 0
    rows = max(K, 1) if max_rows is None else int(max_rows)
    out = np.zeros((rows, 16), np.int64)
    boxes = nd.find_objects(lab)  # only to crop: the box itself comes from np.where below
    for l in range(1, min(K, rows) + 1):
        sl = boxes[l - 1]
        ind = lab[sl] == l
        ys, xs = np.where(ind)
        ys, xs = ys.astype(np.int64) + sl[0].start, xs.astype(np.int64) + sl[1].start
        out[l - 1] = [ys.size, xs.sum(), ys.sum(), (xs * xs).sum(), (xs * ys).sum(), (ys * ys).sum(),
                      xs.min(), ys.min(), xs.max(), ys.max(), *quads(ind), d2max(ind), (ys * W + xs).min()]
    return out


def tables(labels, max_rows):
    """int64 (N, max_rows, 16) of int32 (N, H, W) label planes."""
    return np.stack([table(l, max_rows) for l in labels])


def enclosed_background(ind):
    """The holes of a bool (h, w) indicator, counted: the components (connectivity 1) of its
    complement that do not touch the border of the padded plane."""
    bg, k = nd.label(~np.pad(np.asarray(ind, bool), 1))
    return k - 1  # the padding joins everything that reaches the border into one component


# ---------------------------------------------------------------- extra planes
def checkerboard16():
    return cc_ref.checkerboard(16, 16)


def diagonal_squares():
    """Two 3 x 3 squares that touch at one corner: at connectivity 1 the window at the corner holds
    two labels, at connectivity 2 one component with a diagonal quad."""
    m = np.zeros((9, 9), bool)
    m[1:4, 1:4] = True
    m[4:7, 4:7] = True
    return m


def four_borders(H=40, W=70):
    """One component that touches all four borders: a cross."""
    m = np.zeros((H, W), bool)
    m[H // 2] = True
    m[:, W // 3] = True
    return m


def rectangle(H, W, y0, x0, b, a):
    """An axis-aligned rectangle a wide and b high."""
    m = np.zeros((H, W), bool)
    m[y0:y0 + b, x0:x0 + a] = True
    return m


def rotated_ellipse(H, W, cy, cx, ra, rb, theta):
    """An ellipse with semi-axes ra (along theta, measured from the x axis towards y) and rb."""
    i, j = np.mgrid[:H, :W]
    dx, dy = j - cx, i - cy
    u = dx * np.cos(theta) + dy * np.sin(theta)
    v = -dx * np.sin(theta) + dy * np.cos(theta)
    return (u / ra) ** 2 + (v / rb) ** 2 <= 1.0


def extra_cases():
    """name -> bool (H, W): the planes of the issue that cc_ref.mask_cases() does not hold."""
    return {
        "1x1": np.ones((1, 1), bool),
        "1x130": np.ones((1, 130), bool),
        "130x1": np.ones((130, 1), bool),
        "full65": np.ones((65, 65), bool),
        "checkerboard16": checkerboard16(),
        "diagonal_squares": diagonal_squares(),
        "four_borders": four_borders(),
    }


def all_planes():
    """[(name, bool (H, W))]: every plane of cc_ref.mask_cases() and of extra_cases()."""
    out = []
    for name, batch in cc_ref.mask_cases().items():
        out += [(f"{name}/{p}", m) for p, m in zip(cc_ref.PATTERNS, batch)]
    return out + list(extra_cases().items())


def ellipse_batch():
    """bool (2, 512, 512): one ellipse per plane (the second rotated, with a hole)."""
    a = cc_ref.ellipse(512, 512, 250, 260, 150, 200)
    b = rotated_ellipse(512, 512, 270, 240, 210, 90, 0.6) & ~cc_ref.ellipse(512, 512, 270, 240, 20, 30)
    return np.stack([a, b])


# ---------------------------------------------------------------- the SHAPE block of Trainer.test
def largest_row(tab):
    """The row of the largest component of an int64 (rows, 16) table by the cc_key rule (largest
    area, then the smallest first pixel), or None for an empty table."""
    tab = np.asarray(tab)
    if not (tab[:, 0] > 0).any():
        return None
    best = max(range(len(tab)), key=lambda i: (int(tab[i, 0]), -int(tab[i, 15])) if tab[i, 0] > 0 else (-1, 0))
    return tab[best]
