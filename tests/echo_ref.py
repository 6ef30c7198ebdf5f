"""NumPy / scipy restatement of the lesion echo table (the columns unet_lesion_echo documents), written
from the rules and not from csrc/echo.h: ``np.bincount`` on label * 256 + grey for the histograms,
``scipy.ndimage.minimum_filter`` for the ring's ownership, ``np.bincount`` over shifted slices for the
co-occurrence pairs.  Also the case list the CPU and the GPU tests share, and the direct (pixel-list)
descriptors ``echo_descriptors`` is checked against."""
import numpy as np
import scipy.ndimage as nd
import scipy.stats as st

OFFSETS = ((0, 1), (1, 1), (1, 0), (1, -1))
BIG = np.iinfo(np.int32).max


def owners(lab, w):
    """int64 (H, W): the smallest positive label within chessboard distance w of every pixel (BIG: none)."""
    return nd.minimum_filter(np.where(lab > 0, lab, BIG).astype(np.int64), size=2 * w + 1, mode="constant", cval=BIG)


def plane_table(gray, lab, count, max_rows, G, w):
    F = 512 + G * G
    K = int(min(max(int(count), 0), max_rows))
    out = np.zeros((max_rows, F), np.int64)
    if K == 0:
        return out.astype(np.int32)
    lab = lab.astype(np.int64)
    g = gray.astype(np.int64)
    own_row = (lab > 0) & (lab <= K)
    out[:K, :256] = np.bincount(lab[own_row] * 256 + g[own_row], minlength=(K + 1) * 256).reshape(K + 1, 256)[1:]
    if w > 0:
        own = owners(lab, w)
        sel = (lab <= 0) & (own <= K)
        out[:K, 256:512] = np.bincount(own[sel] * 256 + g[sel], minlength=(K + 1) * 256).reshape(K + 1, 256)[1:]
    q = (g * G) >> 8
    H, W = lab.shape
    acc = np.zeros((K + 1) * G * G, np.int64)
    for dy, dx in OFFSETS:
        ys, xs = slice(0, H - dy), slice(max(0, -dx), W - max(0, dx))
        yt, xt = slice(dy, H), slice(max(0, dx), W + min(0, dx))
        a, b = lab[ys, xs], lab[yt, xt]
        same = (a == b) & (a > 0) & (a <= K)
        acc += np.bincount(a[same] * G * G + q[ys, xs][same] * G + q[yt, xt][same], minlength=acc.size)
    out[:K, 512:] = acc.reshape(K + 1, G * G)[1:]
    return out.astype(np.int32)


def table(gray, labels, count, max_rows, G, w):
    """int32 (N, max_rows, 512 + G G) of gray uint8 (N, H, W), labels int32 (N, H, W), count (N,)."""
    return np.stack([plane_table(gray[n], labels[n], count[n], max_rows, G, w) for n in range(len(labels))])


# ---------------------------------------------------------------- the case list
def label4(mask):
    lab, k = nd.label(mask)  # connectivity 1
    return lab.astype(np.int32), k


def grey(kind, H, W, seed=0):
    if kind == "const":
        return np.full((H, W), 93, np.uint8)
    if kind == "ramp":
        return np.broadcast_to((np.arange(W) % 256).astype(np.uint8), (H, W)).copy()
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


def blobs(H, W, seed, p=0.5, sigma=2.0):
    r = np.random.default_rng(seed)
    return nd.gaussian_filter(r.random((H, W)), sigma) > np.quantile(nd.gaussian_filter(r.random((H, W)), sigma), p)


def _case(name, gray, labels, count, G, w, max_rows=None):
    labels = np.ascontiguousarray(labels, np.int32)
    gray = np.ascontiguousarray(gray, np.uint8)
    if labels.ndim == 2:
        labels, gray = labels[None], gray[None]
    count = np.atleast_1d(np.asarray(count, np.int32))
    rows = int(max(int(count.max()), 1)) if max_rows is None else max_rows
    return dict(name=name, gray=gray, labels=labels, count=count, max_rows=rows, G=G, w=w)


def cases():
    """The planes the kernel can go wrong on (tile 64 x 32): see the comment of every entry."""
    out = []
    # the smallest planes; a ring wider than the plane
    one = np.ones((1, 1), np.int32)
    out += [_case(f"1x1 w{w}", np.full((1, 1), 7, np.uint8), one, 1, 16, w) for w in (0, 1, 16)]
    row = np.zeros((1, 70), bool)
    row[0, 58:67] = True  # a run across the seam at x = 64
    for w in (0, 1, 16):
        out.append(_case(f"1x70 w{w}", grey("random", 1, 70, 1), label4(row)[0], 1, 8, w))
        out.append(_case(f"70x1 w{w}", grey("random", 70, 1, 2), label4(row.T)[0], 1, 32, w))
    # both sides off the tile size: blobs, every G and w, every grey
    H, W = 67, 131
    lab, k = label4(blobs(H, W, 3))
    for G, w, kind in ((8, 0, "random"), (16, 1, "ramp"), (32, 16, "random"), (16, 8, "const"), (32, 1, "const"),
                       (8, 16, "ramp")):
        out.append(_case(f"67x131 blobs G{G} w{w} {kind}", grey(kind, H, W, 4), lab, k, G, w))
    # one component across every tile seam, both ways
    cross = np.zeros((H, W), bool)
    cross[30:35, :] = True
    cross[:, 62:67] = True
    cross[62:66, :] = True
    cross[:, 126:130] = True
    out.append(_case("67x131 seams", grey("random", H, W, 5), label4(cross)[0], 1, 16, 8))
    out.append(_case("67x131 seams ramp w16", grey("ramp", H, W), label4(cross)[0], 1, 32, 16))
    # a component on all four borders: ring and pairs clipped at the plane
    frame = np.ones((40, 70), bool)
    frame[3:-3, 3:-3] = False
    frame[10:20, 20:40] = True  # and an island inside, closer than 2 w to it
    lab, k = label4(frame)
    out.append(_case("40x70 frame", grey("random", 40, 70, 6), lab, k, 16, 8))
    out.append(_case("40x70 frame w16", grey("random", 40, 70, 6), lab, k, 8, 16))
    # two squares touching only diagonally (connectivity 1: two labels, no pair crosses them)
    diag = np.zeros((20, 20), bool)
    diag[4:10, 4:10] = True
    diag[10:16, 10:16] = True
    lab, k = label4(diag)
    assert k == 2
    out.append(_case("diagonal squares", grey("const", 20, 20), lab, k, 16, 1))
    out.append(_case("diagonal squares random", grey("random", 20, 20, 7), lab, k, 8, 8))
    # two bars closer than 2 w: the shared ring goes to the lower label; wider than 256 columns for the ramp
    bars = np.zeros((12, 300), bool)
    bars[2:10, 100:110] = True
    bars[2:10, 115:125] = True
    lab, k = label4(bars)
    assert k == 2
    for w in (1, 8, 16):
        out.append(_case(f"12x300 bars w{w}", grey("ramp", 12, 300), lab, k, 16, w))
    # single-pixel components with distinct labels: more labels per tile than LDS slots, no pair at all
    yy, xx = np.mgrid[:33, :70]
    board = (yy + xx) % 2 == 0
    lab = np.zeros((33, 70), np.int32)
    lab[board] = np.arange(1, board.sum() + 1)
    for G, w in ((16, 1), (32, 0), (8, 16)):
        out.append(_case(f"33x70 checkerboard G{G} w{w}", grey("random", 33, 70, 8), lab, int(board.sum()), G, w))
    # N = 3 with counts (0, 1, many)
    H, W = 67, 131
    one_blob = np.zeros((H, W), bool)
    one_blob[20:50, 40:100] = True
    noise = np.random.default_rng(9).random((H, W)) < 0.3
    labs = [np.zeros((H, W), np.int32), label4(one_blob)[0], label4(noise)[0]]
    cnt = [0, 1, int(labs[2].max())]
    g3 = np.stack([grey("random", H, W, 10), grey("ramp", H, W), grey("random", H, W, 11)])
    out.append(_case("N3 counts 0 1 many", g3, np.stack(labs), cnt, 16, 8))
    # max_rows below the largest label: the dropped labels leave the neighbouring rows alone
    out.append(_case("N3 max_rows 3", g3, np.stack(labs), cnt, 16, 8, max_rows=3))
    out.append(_case("N3 max_rows 1 w1", g3, np.stack(labs), cnt, 8, 1, max_rows=1))
    # negative background values
    neg = labs[2].copy()
    neg[(neg == 0) & (np.random.default_rng(12).random((H, W)) < 0.5)] = -7
    out.append(_case("negative background", g3[2], neg, cnt[2], 32, 8))
    return out


# ---------------------------------------------------------------- descriptors from the pixel lists
def direct_descriptors(gray, lab, l, G, w):
    """The descriptors of label l of one plane, computed on the pixel lists and a dense matrix."""
    import warnings
    v = gray[lab == l].astype(np.float64)
    with warnings.catch_warnings():  # constant grey: scipy warns and gives nan, which is what is wanted
        warnings.simplefilter("ignore")
        skew, kurt = float(st.skew(v)), float(st.kurtosis(v))
    d = dict(pixels=len(v), mean=np.mean(v), std=np.std(v), skewness=skew, kurtosis=kurt, min=v.min(), max=v.max())
    for k, p in (("median", 50), ("p10", 10), ("p90", 90)):
        d[k] = np.percentile(v, p, method="inverted_cdf")
    pr = np.bincount(v.astype(np.int64), minlength=256) / len(v)
    d["entropy"] = -(pr[pr > 0] * np.log2(pr[pr > 0])).sum()
    ring = gray[(lab <= 0) & (owners(lab, w) == l)].astype(np.float64) if w > 0 else np.zeros(0)
    d["ring_pixels"] = len(ring)
    if len(ring):
        d.update(ring_mean=np.mean(ring), ring_std=np.std(ring), ring_p25=np.percentile(ring, 25, method="inverted_cdf"),
                 ring_p75=np.percentile(ring, 75, method="inverted_cdf"))
        d["echo_ratio"] = d["mean"] / d["ring_mean"] if d["ring_mean"] > 0 else np.nan
        den = np.sqrt(d["std"] ** 2 + d["ring_std"] ** 2)
        d["echo_cnr"] = abs(d["mean"] - d["ring_mean"]) / den if den > 0 else np.nan
        d["echo_class"] = -1 if d["median"] < d["ring_p25"] else (1 if d["median"] > d["ring_p75"] else 0)
    else:
        d.update(ring_mean=np.nan, ring_std=np.nan, ring_p25=np.nan, ring_p75=np.nan, echo_ratio=np.nan,
                 echo_cnr=np.nan, echo_class=0)
    q = (gray.astype(np.int64) * G) >> 8
    C = np.zeros((G, G), np.float64)
    H, W = lab.shape
    for dy, dx in OFFSETS:
        for y in range(H - dy):
            for x in range(max(0, -dx), W - max(0, dx)):
                if lab[y, x] == l and lab[y + dy, x + dx] == l:
                    C[q[y, x], q[y + dy, x + dx]] += 1
    pairs = C.sum()
    d["glcm_pairs"] = int(pairs)
    names = ("glcm_contrast", "glcm_dissimilarity", "glcm_homogeneity", "glcm_energy", "glcm_correlation",
             "glcm_entropy")
    if pairs == 0:
        d.update({k: np.nan for k in names})
        return d
    P = (C + C.T) / (2 * pairs)
    i, j = np.mgrid[:G, :G]
    mu = (i * P).sum()
    var = ((i - mu) ** 2 * P).sum()
    d.update(glcm_contrast=((i - j) ** 2 * P).sum(), glcm_dissimilarity=(np.abs(i - j) * P).sum(),
             glcm_homogeneity=(P / (1.0 + (i - j) ** 2)).sum(), glcm_energy=np.sqrt((P * P).sum()),
             glcm_correlation=((i - mu) * (j - mu) * P).sum() / var if var > 0 else 1.0,
             glcm_entropy=-(P[P > 0] * np.log2(P[P > 0])).sum())
    return d
