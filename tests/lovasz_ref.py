"""NumPy float64 restatement of the Lovasz hinge loss as csrc/lovasz.h defines it, and the inputs
the Lovasz tests share.

Every (n, c) plane is its own binary problem over its M = H W pixels, i the raster index:
y_i = (t_i >= 0.5f), s_i = +-1, e_i = fl32(1 - s_i x_i); the order is descending e, ties by ascending
i (np.argsort(-e, kind="stable")); P = sum y, cTP_r / cFP_r the positives / negatives among the ranks
<= r; J_r = 1 - (P - cTP_r) / (P + cFP_r), J_{-1} = 0, g_r = J_r - J_{r-1} in float64;
gmap_i = fl32(g_rank(i)) where e_i > 0 and 0 elsewhere; L_plane = sum_r max(e_r, 0) g_r in float64;
loss = fl32(sum L_plane / (N C)); dlogits_i = ((w * -s_i) * gmap_i) / (N C) in float32 where e_i > 0,
0 elsewhere.
"""
import functools
import math

import numpy as np
import torch

KINDS = ("random", "ties", "constant", "all_zero", "all_one", "soft", "confident", "signed_zero", "inf")


def _blobs(N, C, H, W, rng):
    """{0, 1} float32 targets: one ellipse per plane, never empty, never the whole plane (for H W > 1)."""
    yy, xx = np.mgrid[0:H, 0:W]
    t = np.zeros((N, C, H, W), np.float32)
    for n in range(N):
        for c in range(C):
            cy, cx = rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W
            ry, rx = max(rng.uniform(0.15, 0.35) * H, 0.6), max(rng.uniform(0.15, 0.35) * W, 0.6)
            m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
            m[int(min(cy, H - 1)), int(min(cx, W - 1))] = True
            t[n, c] = m
    if H * W > 1:
        t.reshape(N, C, -1)[:, :, 0] = 0.0
    return t


def make_case(shape, kind, seed=0):
    """(logits, targets) float32 (N, C, H, W) of one kind:
    random       randn * 4 logits, blob targets
    ties         logits quantised to multiples of 0.25: thousands of equal keys
    constant     all logits equal: the order is decided by stability alone
    all_zero / all_one   targets: P = 0 and P = M
    soft         torch.rand targets with exact 0.5 among them (the 0.5 rule)
    confident    at least 95 % of the pixels with e <= 0
    signed_zero  x = s exactly on half of the pixels: e = 0, inactive
    inf          a few +-inf logits (the plane keeps finite positives below them, so that no
                 0 * inf product arises)
    exact        tie-free, and e = 1 - s x exact in float64 as in float32 (multiples of 2^-10):
                 where a float64 composition of the published formula must agree
    """
    N, C, H, W = shape
    rng = np.random.default_rng(1000 * seed + 17 * H + W + len(kind))
    x = (rng.standard_normal(shape) * 4).astype(np.float32)
    t = _blobs(N, C, H, W, rng)
    if kind == "random":
        pass
    elif kind == "ties":
        x = (np.round(x * 4) / 4).astype(np.float32)
    elif kind == "constant":
        x = np.full(shape, 0.3, np.float32)
    elif kind == "all_zero":
        t = np.zeros(shape, np.float32)
    elif kind == "all_one":
        t = np.ones(shape, np.float32)
    elif kind == "soft":
        g = torch.Generator().manual_seed(seed + 5)
        t = torch.rand(shape, generator=g).numpy()
        t.reshape(-1)[::7] = 0.5
        t.reshape(-1)[3::11] = np.nextafter(np.float32(0.5), np.float32(0))
    elif kind == "confident":
        s = np.where(t >= 0.5, 1.0, -1.0).astype(np.float32)
        sure = rng.random(shape) < 0.97
        x = np.where(sure, s * (1 + np.abs(x)), x).astype(np.float32)
    elif kind == "signed_zero":
        s = np.where(t >= 0.5, 1.0, -1.0).astype(np.float32)
        x = np.where(rng.random(shape) < 0.5, s, x).astype(np.float32)
    elif kind == "inf":
        flat, tf = x.reshape(N * C, -1), t.reshape(N * C, -1)
        for p in range(N * C):
            idx = rng.choice(H * W, size=min(4, H * W), replace=False)
            for j, i in enumerate(idx):
                flat[p, i] = np.inf if j % 2 else -np.inf
            # finite, active positives below the infinities: cTP < P at every infinite rank
            pos = np.flatnonzero((tf[p] >= 0.5) & np.isfinite(flat[p]))
            assert pos.size, "the inf kind needs a finite positive in every plane"
            flat[p, pos[0]] = -0.5
    elif kind == "exact":
        M = H * W
        assert M <= 12000
        flat = x.reshape(N * C, -1)
        s = np.where(t >= 0.5, 1.0, -1.0).reshape(N * C, -1)
        for p in range(N * C):
            k = rng.choice(np.arange(-6000, 6001), size=M, replace=False)
            flat[p] = (s[p] * (1.0 - k / 1024.0)).astype(np.float32)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(t, np.float32)


def reference(x, t, w=1.0):
    """dict: e float32 (N, C, H, W), perm int64 (N C, M), g float64 (N C, M) in RANK order, gmap
    float32 (N, C, H, W), L float64 (N C,), terms (N C,) = sum_r |max(e_r, 0) g_r|, sum float64, loss
    float32, dlogits float32 (N, C, H, W) for the incoming gradient w."""
    x, t = np.asarray(x, np.float32), np.asarray(t, np.float32)
    N, C, H, W = x.shape
    M, planes = H * W, N * C
    y = t >= np.float32(0.5)
    s = np.where(y, np.float32(1), np.float32(-1))
    with np.errstate(invalid="ignore", over="ignore"):
        e = (np.float32(1) - s * x).astype(np.float32)
    ef, yf = e.reshape(planes, M), y.reshape(planes, M)
    perm = np.empty((planes, M), np.int64)
    g = np.empty((planes, M), np.float64)
    gmap = np.zeros((planes, M), np.float32)
    L, terms = np.empty(planes), np.empty(planes)
    for p in range(planes):
        perm[p] = np.argsort(-ef[p], kind="stable")
        ys = yf[p][perm[p]].astype(np.int64)
        P = int(ys.sum())
        ctp = np.cumsum(ys)
        cfp = np.arange(1, M + 1) - ctp
        J = 1.0 - (P - ctp).astype(np.float64) / (P + cfp).astype(np.float64)
        g[p] = np.diff(J, prepend=0.0)
        es = ef[p][perm[p]].astype(np.float64)
        with np.errstate(invalid="ignore"):
            prod = np.maximum(es, 0.0) * g[p]
        L[p] = math.fsum(prod) if np.all(np.isfinite(prod)) else prod.sum()
        terms[p] = np.abs(prod).sum()
        gmap[p, perm[p]] = np.where(es > 0, g[p].astype(np.float32), np.float32(0))
    total = math.fsum(L) if np.all(np.isfinite(L)) else L.sum()
    gm = gmap.reshape(x.shape)
    w32, nc = np.float32(w), np.float32(planes)
    d = np.where(e > 0, (np.where(y, -w32, w32) * gm) / nc, np.float32(0)).astype(np.float32)
    return dict(e=e, perm=perm, g=g, gmap=gm, L=L, terms=terms, sum=total,
                loss=np.float32(total / planes), dlogits=d)


@functools.lru_cache(maxsize=None)
def case(shape, kind, seed=0):
    """(x, t, reference(x, t)) of a case, computed once and never modified."""
    x, t = make_case(shape, kind, seed)
    for a in (x, t):
        a.setflags(write=False)
    return x, t, reference(x, t)


def sum_bar(ref, M):
    """The float64-rounding bar of a sum of the planes' M products each: M 2^-52 sum |terms|."""
    return M * 2.0 ** -52 * float(ref["terms"].sum())


def berman_torch(x, t):
    """Berman's published lovasz_hinge (per_image=True, one image per plane) written out in float64
    torch: (mean loss with autograd attached to the returned float64 logits, those logits)."""
    xd = torch.from_numpy(np.array(x)).double().requires_grad_(True)
    labels = (torch.from_numpy(np.array(t)) >= 0.5).double()
    N, C, H, W = xd.shape
    losses = []
    for logit, label in zip(xd.reshape(N * C, -1), labels.reshape(N * C, -1)):
        signs = 2.0 * label - 1.0
        errors = 1.0 - logit * signs
        errors_sorted, perm = torch.sort(errors, dim=0, descending=True)
        gt_sorted = label[perm]
        gts = gt_sorted.sum()
        intersection = gts - gt_sorted.cumsum(0)
        union = gts + (1.0 - gt_sorted).cumsum(0)
        jaccard = 1.0 - intersection / union
        jaccard = torch.cat([jaccard[:1], jaccard[1:] - jaccard[:-1]])
        losses.append(torch.dot(torch.relu(errors_sorted), jaccard))
    return torch.stack(losses).mean(), xd
