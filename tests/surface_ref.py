"""The oracle and the inputs of the surface-metric tests (test_surface_cpu.py,
test_gpu_surface.py).

``oracle`` is the definition itself -- MedPy's ``hd``, ``hd95`` and ``assd`` at connectivity 1,
spelled out with scipy and numpy (MedPy is not a dependency) -- and returns the integer fields of
``unet_surface_stats`` next to the three metrics."""
import numpy as np
import scipy.ndimage as nd

INT_FIELDS = ("defined", "n_pg", "n_gp", "max_d2", "d2_lo", "d2_hi")


def oracle(P, G):
    """P, G: bool (H, W).  dict of the integer fields, sum_pg, sum_gp, hd, hd95, assd."""
    P, G = np.asarray(P, bool), np.asarray(G, bool)
    if not P.any() or not G.any():  # MedPy raises here
        out = dict.fromkeys(INT_FIELDS, 0)
        out.update(sum_pg=0.0, sum_gp=0.0, hd=np.nan, hd95=np.nan, assd=np.nan)
        return out
    st = nd.generate_binary_structure(2, 1)
    bp, bg = P & ~nd.binary_erosion(P, st), G & ~nd.binary_erosion(G, st)
    dt_g, dt_p = nd.distance_transform_edt(~bg), nd.distance_transform_edt(~bp)
    d_pg, d_gp = dt_g[bp], dt_p[bg]
    d2 = []
    for d in (d_pg, d_gp):  # the squared distances are integers: the round trip is exact
        q = np.rint(d ** 2).astype(np.int64)
        assert np.array_equal(np.sqrt(q.astype(np.float64)), d)
        d2.append(q)
    both = np.sort(np.concatenate(d2))
    pos = 0.95 * (both.size - 1)
    return dict(defined=1, n_pg=d_pg.size, n_gp=d_gp.size, max_d2=int(both[-1]),
                d2_lo=int(both[int(np.floor(pos))]), d2_hi=int(both[int(np.ceil(pos))]),
                sum_pg=float(d_pg.sum()), sum_gp=float(d_gp.sum()),
                hd=float(np.sqrt(np.float64(both[-1]))),
                hd95=float(np.percentile(np.hstack([d_pg, d_gp]), 95)),
                assd=float((d_pg.mean() + d_gp.mean()) / 2))


def to_inputs(P, G, C=1, seed=0):
    """bool (N, H, W) masks -> float32 logits (+-3) and targets (0 / 1) of shape (N, C, H, W);
    channels above 0 hold values that would change every result if they were read."""
    P, G = np.asarray(P, bool), np.asarray(G, bool)
    N, H, W = P.shape
    r = np.random.default_rng(seed)
    x = r.normal(size=(N, C, H, W)).astype(np.float32)
    t = (r.random((N, C, H, W)) < 0.5).astype(np.float32)
    x[:, 0] = np.where(P, 3.0, -3.0)
    t[:, 0] = G
    return x, t


def ellipse(H, W, cy, cx, ry, rx):
    i, j = np.mgrid[:H, :W]
    return ((i - cy) / ry) ** 2 + ((j - cx) / rx) ** 2 <= 1.0


def _z(H, W):
    return np.zeros((H, W), bool)


def mask_cases():
    """name -> (P, G), bool (N, H, W) each; every sample is defined."""
    c = {}
    b = _z(8, 8)
    b[2:6, 1:5] = True
    c["identical_8x8"] = (b[None], b[None])
    p, g = _z(8, 8), _z(8, 8)
    p[1, 2] = g[6, 5] = True
    c["single_pixels_8x8_n2"] = (p[None], g[None])  # n = 1 is impossible: both masks are non-empty
    p, g = _z(33, 65), _z(33, 65)
    p[5, 3:13] = True   # one-pixel-wide lines: every pixel is a border pixel
    g[20, 30:41] = True
    c["lines_33x65_n21"] = (p[None], g[None])  # 0.95 * 20 == 19: lo == hi
    p2, g2 = _z(33, 65), _z(33, 65)
    p2[5, 3:15] = True
    g2[20, 30:38] = True
    c["lines_33x65_n20"] = (p2[None], g2[None])  # 0.95 * 19 = 18.05: lo != hi
    p, g = np.ones((40, 72), bool), _z(40, 72)
    g[:9, 60:] = True
    g[30:, :5] = True
    c["full_image_vs_edge_blobs_40x72"] = (p[None], g[None])
    p = ellipse(40, 72, 20, 36, 15, 30) & ~ellipse(40, 72, 20, 36, 7, 12)  # a hole
    g = ellipse(40, 72, 18, 30, 12, 25)
    c["hole_40x72"] = (p[None], g[None])
    p = ellipse(33, 65, 10, 12, 6, 8) | ellipse(33, 65, 22, 50, 7, 9)  # two components
    g = ellipse(33, 65, 16, 30, 10, 20)
    c["two_components_33x65"] = (p[None], g[None])
    r = np.random.default_rng(3)
    P = np.stack([ellipse(40, 72, 20, 30, 10, 18), ellipse(40, 72, 5, 60, 9, 15), r.random((40, 72)) < 0.4])
    G = np.stack([ellipse(40, 72, 22, 34, 12, 15), r.random((40, 72)) < 0.05, ellipse(40, 72, 20, 36, 19, 35)])
    c["batch3_40x72"] = (P, G)
    P = np.stack([ellipse(64, 64, 30, 30, 20, 12), r.random((64, 64)) < 0.5, ellipse(64, 64, 0, 0, 25, 40)])
    G = np.stack([ellipse(64, 64, 34, 28, 14, 18), r.random((64, 64)) < 0.5, ellipse(64, 64, 63, 63, 30, 30)])
    c["batch3_64x64"] = (P, G)
    return c


def empty_case():
    """(P, G) of 4 samples at 8x8: empty prediction, empty target, both empty, then a defined one."""
    b = _z(8, 8)
    b[2:5, 3:6] = True
    e = _z(8, 8)
    return np.stack([e, b, e, b]), np.stack([b, e, e, np.roll(b, 2, 1)])


def big_case():
    """Two 512x512 pairs: an ellipse against its perturbed copy, and a speckled region against a
    small far blob (thousands of distinct squared distances: a three-pass select)."""
    r = np.random.default_rng(11)
    p0 = ellipse(512, 512, 250, 260, 150, 200)
    g0 = ellipse(512, 512, 262, 249, 140, 215)
    p1 = ellipse(512, 512, 300, 300, 180, 190) | (r.random((512, 512)) < 0.02)
    g1 = ellipse(512, 512, 40, 50, 20, 30)
    return np.stack([p0, p1]), np.stack([g0, g1])
