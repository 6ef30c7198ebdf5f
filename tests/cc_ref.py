"""The oracle and the inputs of the connected-component tests (test_cc_cpu.py, test_gpu_cc.py).

The oracle is scipy: ``scipy.ndimage.label`` for the labels, the composition of ``label``,
``bincount``, ``argmax`` and ``binary_fill_holes`` for the post-processing, and a NumPy count over
``np.unique`` for the lesion statistics.  Every comparison against it is exact.

The cases are the smallest shapes that can break tiling (64-column tiles of 16, 32 or 64 rows),
seams, find depth or the tie rules; each is a batch of every pattern at one size."""
import itertools

import numpy as np
import scipy.ndimage as nd

CONNECTIVITIES = (1, 2)
SIZES = ((1, 1), (1, 130), (130, 1), (7, 5), (33, 65), (64, 64), (96, 160))
OPTIONS = list(itertools.product((False, True), repeat=3))  # keep_largest, small min_area, fill_holes


def structure(conn):
    return nd.generate_binary_structure(2, 1) if conn == 1 else np.ones((3, 3), int)


# ---------------------------------------------------------------- oracle
def label(m, conn):
    lab, k = nd.label(np.asarray(m, bool), structure(conn))
    return lab.astype(np.int32), k


def postprocess(m, conn, keep_largest=False, min_area=0, fill_holes=False):
    """bool (H, W) -> (bool (H, W), [components before, components kept, pixels after, pixels filled])."""
    a = np.asarray(m, bool)
    lab, k = nd.label(a, structure(conn))
    area = np.bincount(lab.ravel(), minlength=k + 1)
    keep = area >= min_area
    keep[0] = False
    a = keep[lab]
    kept = int(keep.sum())
    if keep_largest and a.any():
        lab, _ = nd.label(a, structure(conn))
        a = lab == np.argmax(np.bincount(lab.ravel())[1:]) + 1
        kept = 1
    before = int(a.sum())
    if fill_holes:
        a = nd.binary_fill_holes(a)
    return a, [k, kept, int(a.sum()), int(a.sum()) - before]


def lesion(P, G, conn):
    """[n_pred, n_gt, gt_hit, pred_hit] of bool (H, W) masks."""
    P, G = np.asarray(P, bool), np.asarray(G, bool)
    lab_p, n_p = nd.label(P, structure(conn))
    lab_g, n_g = nd.label(G, structure(conn))
    return [n_p, n_g, int(np.unique(lab_g[P & G]).size), int(np.unique(lab_p[P & G]).size)]


# ---------------------------------------------------------------- patterns
def ellipse(H, W, cy, cx, ry, rx):
    i, j = np.mgrid[:H, :W]
    return ((i - cy) / ry) ** 2 + ((j - cx) / rx) ** 2 <= 1.0


def serpentine(H, W):
    """Full even rows joined alternately at the right and left ends: one component of maximal
    path length (a single row or a single full column when there is no room)."""
    m = np.zeros((H, W), bool)
    m[::2] = True
    for k, i in enumerate(range(1, H - 1, 2)):
        m[i, W - 1 if k % 2 == 0 else 0] = True
    return m


def spiral(H, W):
    m = np.zeros((H, W), bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True

    def free(a, b):
        return 0 <= a < H and 0 <= b < W and not m[a, b]

    def can(dy, dx):
        a, b = y + dy, x + dx
        if not free(a, b):
            return False
        a2, b2 = a + dy, b + dx
        return not (0 <= a2 < H and 0 <= b2 < W and m[a2, b2])

    for _ in range(H * W):
        if not can(dy, dx):
            dy, dx = dx, -dy
            if not can(dy, dx):
                break
        y, x = y + dy, x + dx
        m[y, x] = True
    return m


def checkerboard(H, W):
    i, j = np.mgrid[:H, :W]
    return (i + j) % 2 == 0


def diagonal(H, W, anti=False):
    m = np.zeros((H, W), bool)
    n = min(H, W)
    k = np.arange(n)
    m[k, (W - 1 - k) if anti else k] = True
    return m


def comb(H, W):
    m = np.zeros((H, W), bool)
    m[0] = True
    m[:, ::2] = True
    if H > 2:
        m[H - 1, 1::2] = False
    return m


def ring(H, W, gap=False):
    m = ellipse(H, W, (H - 1) / 2, (W - 1) / 2, H / 2.2, W / 2.2) & ~ellipse(H, W, (H - 1) / 2, (W - 1) / 2,
                                                                              H / 3.5, W / 3.5)
    if gap:  # the hole opens to the border: nothing to fill
        m[: H // 2 + 1, W // 2] = False
    return m


def nested_rings(H, W):
    i, j = np.mgrid[:H, :W]
    d = np.minimum(np.minimum(i, H - 1 - i), np.minimum(j, W - 1 - j))
    return d % 4 == 1


def tie_pair(H, W, swap=False):
    """Two components; equal areas unless swap (then the later one in raster order is larger)."""
    m = np.zeros((H, W), bool)
    if H * W < 12:
        m.flat[:1] = True
        return m
    if W >= 6:
        m[0, 0:2] = True
        m[H - 1, W - (3 if swap else 2):] = True
    else:
        m[0:2, 0] = True
        m[H - (3 if swap else 2):, W - 1] = True
    return m


PATTERNS = ("empty", "full", "rand30", "rand50", "rand60", "serpentine", "spiral", "checkerboard",
            "diagonal", "antidiagonal", "comb", "ring", "nested_rings", "open_ring", "tie", "tie_swapped")


def patterns(H, W, seed=0):
    """bool (len(PATTERNS), H, W), in PATTERNS order."""
    r = np.random.default_rng([seed, H, W])
    out = [np.zeros((H, W), bool), np.ones((H, W), bool)]
    out += [r.random((H, W)) < d for d in (0.3, 0.5, 0.6)]
    out += [serpentine(H, W), spiral(H, W), checkerboard(H, W), diagonal(H, W), diagonal(H, W, True),
            comb(H, W), ring(H, W), nested_rings(H, W), ring(H, W, True), tie_pair(H, W), tie_pair(H, W, True)]
    return np.stack(out)


def mask_cases():
    """name -> bool (N, H, W): every pattern at every size (one batch per size)."""
    return {f"{H}x{W}": patterns(H, W) for H, W in SIZES}


def big_case():
    """One 512x512 batch of 2: noise at density 0.6, and a noisy ellipse with a hole."""
    r = np.random.default_rng(5)
    a = r.random((512, 512)) < 0.6
    b = (ellipse(512, 512, 250, 260, 150, 200) & ~ellipse(512, 512, 240, 250, 40, 60)) ^ (r.random((512, 512)) < 0.02)
    return np.stack([a, b])


EDGE_LOGITS = np.array([0.0, 1e-45, -1e-45, 5.9e-8, 6.0e-8, 1.19e-7, 1.2e-7, 2.4e-7, 1e-6, -1e-6, 1.0, -1.0],
                       np.float32)  # the values of test_predicate_is_the_mask_readout (1e-45: the smallest float)


def edge_logits(N=2, C=2, H=33, W=65, seed=4):
    r = np.random.default_rng(seed)
    return EDGE_LOGITS[r.integers(0, EDGE_LOGITS.size, (N, C, H, W))]


def readout(x):
    """The mask Trainer.test reads: torch.sigmoid(x) > 0.5 in float32 (utils/trainer.py)."""
    import torch
    return (torch.sigmoid(torch.from_numpy(np.asarray(x, np.float32))) > 0.5).numpy()


def to_logits(m, C=2, seed=1):
    """bool (N, H, W) -> float32 (N, C, H, W) logits (+-3 in channel 0, noise above it)."""
    m = np.asarray(m, bool)
    x = np.random.default_rng(seed).normal(size=(m.shape[0], C) + m.shape[1:]).astype(np.float32)
    x[:, 0] = np.where(m, 3.0, -3.0)
    return x


def to_targets(m, C=2, seed=2):
    """bool (N, H, W) -> float32 (N, C, H, W) targets (0 / 1 in channel 0; 0.5, 1.5 and 2 mixed in:
    (int)t == 1 is foreground, so 1.5 is and 0.5 and 2 are not)."""
    m = np.asarray(m, bool)
    r = np.random.default_rng(seed)
    t = (r.random((m.shape[0], C) + m.shape[1:]) < 0.5).astype(np.float32)
    t[:, 0] = m
    odd = r.random(m.shape) < 0.1
    t[:, 0][odd & m] = 1.5
    t[:, 0][odd & ~m] = r.choice(np.array([0.5, 2.0], np.float32), int((odd & ~m).sum()))
    return t


def min_areas(m, conn):
    """The min_area values worth checking on one mask: none, a component's area (kept), one above
    it (removed), and one above the largest (removes everything)."""
    lab, k = label(m, conn)
    if k == 0:
        return [0, 3]
    area = np.bincount(lab.ravel())[1:]
    mid = int(np.sort(area)[k // 2])
    return sorted({0, mid, mid + 1, int(area.max()) + 1})
