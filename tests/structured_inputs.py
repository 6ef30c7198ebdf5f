"""Structured input images and the rules the kernels must keep on them (helper of the tests, not
a test; importable without a GPU).

Every other network test feeds i.i.d. uniform noise (`_helpers.inputs`).  Ultrasound frames are
not noise: exact-zero margins, flat saturated areas, speckle in between.  The families below are
built from `oracle.weights.uniform` alone (no new generator) and return `(x, t)` like
`_helpers.inputs`.  The checkers are pure numpy / float64, so the rules they apply are tested on
the CPU (tests/test_structured_cpu.py) before the GPU tests apply them to the workspace.

Exact ties.  A conv output is a function of its receptive field alone, computed in one fixed
order, so two pixels whose receptive fields hold the same values in the same places carry
bit-equal outputs.  A constant region of the image therefore gives four-way ties in every pooled
window whose receptive field lies inside it and, unlike the image itself, away from the image
border (zero padding is not the constant): each 3x3 conv after the first moves that frontier one
pixel of its level inwards.  Straight edges between constant regions give the two-way ties.
"""
import numpy as np
import torch

from oracle import weights as Wt

U32 = 2.0 ** -24          # unit roundoff of float32
K_GROUP = 127             # additions of a 128-row partial sum, any order
T_NOISE, T_AUX, T_TARGET = 1000, 1001, 2000   # oracle.weights tensor indices


def _u(seed, idx, N, H, W):
    return Wt.uniform(seed, idx, N * H * W).reshape(N, 1, H, W)


def _pack(x, t):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)), torch.from_numpy(np.ascontiguousarray(t, np.float32))


def margin_box(H, W, depth):
    """(top, bottom, left, right) margins of `margins`: 11 * 2**(depth - 1) pixels on the top and
    the left, 3 and 5 pixels -- odd, so the speckle ends inside a pooling window -- on the bottom
    and the right.  3 * 2**depth would leave a 2x2 block of the deepest pooled windows over zeros
    of the IMAGE; the windows tie only where their receptive fields do (module docstring), which
    at the deepest pool d = depth - 1 ends 4 pixels of that level from the image border and 4
    from the speckle (one pixel after level 0's two convs, halved and rounded up by every pool,
    plus two per level: 1, 3, 4, 4, ...), and a window starts on an even pixel: 11 pixels of
    level d.  Where the image is too small for that and a speckle strip of 8 pixels the leading
    margin gives way; `four_way_reachable` says where ties then cannot occur at all."""
    lead = 11 * 2 ** (depth - 1)
    return min(lead, H - 3 - 8), 3, min(lead, W - 5 - 8), 5


def margins(seed, N, H, W, depth):
    """Speckle interior (the noise image times a smooth sin^2 envelope), exact-zero margins on all
    four sides (`margin_box`); the target is the disc phantom cut to the interior."""
    top, bot, left, right = margin_box(H, W, depth)
    h, w = H - top - bot, W - left - right
    env = np.outer(np.sin(np.pi * (np.arange(h) + 0.5) / h) ** 2, np.sin(np.pi * (np.arange(w) + 0.5) / w) ** 2)
    x = np.zeros((N, 1, H, W))
    x[:, :, top:H - bot, left:W - right] = _u(seed, T_NOISE, N, H, W)[:, :, top:H - bot, left:W - right] * env
    t = np.zeros((N, 1, H, W), np.float32)
    t[:, :, top:H - bot, left:W - right] = Wt.make_target(seed, N, H, W)[:, :, top:H - bot, left:W - right]
    return _pack(x, t)


def block_cuts(n):
    """Cut positions 0, 9, 20, 29, 40, ... (blocks of 9 and 11 pixels): odd and even corners."""
    cuts, step = [0], 9
    while cuts[-1] + step < n:
        cuts.append(cuts[-1] + step)
        step = 20 - step
    return cuts + [n]


def blocks(seed, N, H, W):
    """Piecewise-constant values k / 255 in rectangles between `block_cuts`: four-way ties inside
    a block, ties of the pairs (0, 2) and (1, 3) along a vertical edge and of (0, 1) and (2, 3)
    along a horizontal one.  The target is the set of blocks with k >= 128."""
    ry, rx = block_cuts(H), block_cuts(W)
    ny, nx = len(ry) - 1, len(rx) - 1
    k = np.floor(Wt.uniform(seed, T_AUX, N * ny * nx) * 256).reshape(N, ny, nx)
    x = np.zeros((N, 1, H, W))
    for i in range(ny):
        for j in range(nx):
            x[:, 0, ry[i]:ry[i + 1], rx[j]:rx[j + 1]] = (k[:, i, j] / 255.0)[:, None, None]
    return _pack(x, x >= 128 / 255.0)


def ddti_like(seed, N, H, W):
    """uint8-quantised values k / 255: the left 30 % of the columns exactly 0.0, a rectangle of
    1/4 of the rows by 1/5 of the columns (5 % of the area) exactly 1.0, speckle k = 1 .. 178
    (mean ~0.35) elsewhere."""
    k = 1 + np.floor(Wt.uniform(seed, T_NOISE, N * H * W) * 178).reshape(N, 1, H, W)
    z = int(round(0.3 * W))
    k[..., :z] = 0
    y0, x0 = H // 4, W // 2
    k[:, :, y0:y0 + H // 4, x0:x0 + W // 5] = 255
    t = Wt.make_target(seed, N, H, W)
    t[..., :z] = 0
    return _pack(k / 255.0, t)


def black_sample(seed, H, W, depth):
    """N = 3: samples 0 and 2 from `margins`, sample 1 all zeros with an empty target."""
    x, t = margins(seed, 2, H, W, depth)
    z = torch.zeros_like(x[:1])
    return torch.cat([x[:1], z, x[1:]]), torch.cat([t[:1], z, t[1:]])


def offset(a, seed, N, H, W):
    """a + (1 - a) u: the noise image squeezed towards 1 (statistics check only)."""
    x = a + (1.0 - a) * _u(seed, T_NOISE, N, H, W)
    return _pack(x, Wt.make_target(seed, N, H, W))


FAMILIES = {
    "margins": lambda seed, N, H, W, depth: margins(seed, N, H, W, depth),
    "blocks": lambda seed, N, H, W, depth: blocks(seed, N, H, W),
    "ddti_like": lambda seed, N, H, W, depth: ddti_like(seed, N, H, W),
    "black_sample": lambda seed, N, H, W, depth: black_sample(seed, H, W, depth),
    "offset0": lambda seed, N, H, W, depth: offset(0.0, seed, N, H, W),
    "offset0.9": lambda seed, N, H, W, depth: offset(0.9, seed, N, H, W),
    "offset0.99": lambda seed, N, H, W, depth: offset(0.99, seed, N, H, W),
}


# ------------------------------------------------------------------------------- pool winners
def windows(a):
    """(N, C, H, W) -> (N, C, H/2, W/2, 4): the 2x2 windows in torch's scan order (0,0), (0,1),
    (1,0), (1,1)."""
    a = np.asarray(a)
    N, C, H, W = a.shape
    return a.reshape(N, C, H // 2, 2, W // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)


def torch_winners(v):
    """torch's max_pool2d rule on window values v (..., 4): the first maximum in scan order."""
    return np.argmax(np.asarray(v), axis=-1).astype(np.uint8)


def tie_counts(y4, idx):
    """Exact ties of the recorded winner: windows whose four stored inputs are bit-equal
    ("four"), and windows in which exactly one other input is bit-equal to the winner's, by the
    first member of that pair ("first0", "first1", "first2")."""
    b = np.ascontiguousarray(y4, np.float32).view(np.uint32)
    win = np.take_along_axis(b, idx[..., None].astype(np.int64), -1)
    eq = b == win
    n = eq.sum(-1)
    first = np.argmax(eq, -1)
    out = {"four": int((n == 4).sum())}
    for k in range(3):
        out[f"first{k}"] = int(((n == 2) & (first == k)).sum())
    return out


def check_winners(y4, sc, sh, relu, idx):
    """The max-pool's winner rule on what the pass read: y4 (..., C, 4) float32, the four stored
    window inputs of every pooled element; (sc, sh) (C,) float32, the affine the pass applies, or
    None; idx (..., C) the recorded winner k*.  With v = float64(y) float64(sc) + float64(sh)
    (the product of two float32 is exact in float64, the sum is rounded once at 2^-53):

      (a) v[k*] >= max v - 1 float32 ulp of max |v|  (the kernel compares float32 roundings of v);
      (b) no k < k* has y[k] bit-equal to y[k*]      (arithmetic-free: equal inputs under one
          affine give equal outputs, and of equals the first in scan order wins);
      (c) no k < k* has v[k] > v[k*]                 (rounding is monotone: a strictly larger v
          cannot round below a smaller one, so an earlier strictly larger candidate wins).

    relu (BN -> ReLU order): the kernel takes the max before the ReLU; where max v <= 0 every
    candidate becomes 0 and the gradient is blocked, so such windows are exempt from (a) and (c).
    (b) binds everywhere.  Returns `tie_counts` of the windows judged."""
    y4 = np.ascontiguousarray(y4, np.float32)
    idx = np.asarray(idx)
    assert y4.shape[-1] == 4 and idx.shape == y4.shape[:-1], (y4.shape, idx.shape)
    assert idx.max() <= 3, "winner index outside the window"
    v = y4.astype(np.float64)
    if sc is not None:
        v = v * np.asarray(sc, np.float32).astype(np.float64)[:, None] + \
            np.asarray(sh, np.float32).astype(np.float64)[:, None]
    assert np.isfinite(v).all()
    k = idx[..., None].astype(np.int64)
    vw = np.take_along_axis(v, k, -1)[..., 0]
    vmax = v.max(-1)
    live = vmax > 0 if relu else np.ones(vmax.shape, bool)
    ulp = np.spacing(np.abs(v).max(-1).astype(np.float32)).astype(np.float64)
    bad = live & (vw < vmax - ulp)
    assert not bad.any(), f"(a) {int(bad.sum())} winners below the window maximum, first at {np.argwhere(bad)[0]}"
    before = np.arange(4) < k
    b = y4.view(np.uint32)
    bw = np.take_along_axis(b, k, -1)
    bad = (before & (b == bw)).any(-1)
    assert not bad.any(), f"(b) {int(bad.sum())} winners with a bit-equal earlier input, first at {np.argwhere(bad)[0]}"
    bad = live & (before & (v > vw[..., None])).any(-1)
    assert not bad.any(), f"(c) {int(bad.sum())} winners with a larger earlier candidate, first at {np.argwhere(bad)[0]}"
    return tie_counts(y4, idx)


# ----------------------------------------------------------------------------- BN statistics
def stats64(y):
    """float64 statistics of the stored rows y (M, C): mean, biased variance, mean |y|, mean y^2."""
    y = np.asarray(y, np.float64)
    m = y.mean(0)
    return m, ((y - m) ** 2).mean(0), np.abs(y).mean(0), (y * y).mean(0)


def var_bound(y, K=K_GROUP):
    """The bound of `check_stats` on |var_dev - var64| without its relative term, per channel."""
    m, _, ma, m2 = stats64(y)
    return K * U32 * (m2 + 2 * np.abs(m) * ma)


def check_stats(y, count, mean, invstd, eps, K=K_GROUP):
    """The batch statistics the forward finalized (debug views 3, 4) against the float64
    statistics of the rows y (M, C) it stored, per channel.  u = 2^-24.

    What the kernels do (gemm_common.h row_epilogue, conv_first_fwd_kernel, bn_train_final): every
    group of at most 128 rows is summed in float32, s_g = sum y and q_g = sum y^2 (fma(y, y, q):
    the square is not rounded); the groups are combined and divided by `count` in float64;
    var = q / count - mean^2 in float64, clamped at 0; mean and invstd = 1 / sqrt(var + eps) are
    rounded to float32.

    A float32 sum of n terms in any order is off by at most (n - 1) u sum |terms| to first order,
    and exactly so once the depth d of the sum (roundings a term passes) obeys d u / (1 - d u) <=
    (n - 1) u.  The GEMM epilogue sums 32 rows per lane, then the lane halves, then the two 64-row
    units: d = 34.  The first conv sums ceil(P / G) <= 64 pixels per block (G >= P / 64 blocks)
    with a rounded square: d <= 65.  Both are below K = 127, which therefore bounds every
    producer.  The float64 combine adds 2^-53 relative terms, which the slack between d and 127
    covers by orders of magnitude.  So, with dm the error of the float64 mean,

        |dm|               <= K u mean|y|
        |mean - mean64|    <= K u mean|y| + u |mean64|              (the float32 rounding)
        |q / n - mean(y^2)| <= K u mean(y^2)
        |mean_dev^2 - mean64^2| <= 2 |mean64| |dm| + dm^2
        |var_dev - var64|  <= K u (mean(y^2) + 2 |mean64| mean|y|) + 4 u var64 + 3 u eps

    where var_dev = 1 / invstd^2 - eps.  Rounding invstd to float32 moves 1 / invstd^2 by
    (2 u + 3 u^2) (var + eps): the 4 u var64 takes its var part, dm^2 and the rounding of mean
    twice over; the eps part, 2 u eps, is listed apart (3 u eps = 1.8e-12 at eps = 1e-5) because a
    constant channel has var64 = 0 and invstd = fl(1 / sqrt(eps)).  Returns var64 and the bound on
    var, which `check_affine_and_running` reuses."""
    y = np.asarray(y, np.float32)
    assert count == y.shape[0], f"count {count} is not the {y.shape[0]} rows stored"
    mean, invstd = np.asarray(mean, np.float64), np.asarray(invstd, np.float64)
    m, var, ma, m2 = stats64(y)
    bm = K * U32 * ma + U32 * np.abs(m)
    bad = np.abs(mean - m) > bm
    assert not bad.any(), (f"mean: {int(bad.sum())} channels off, worst {np.max(np.abs(mean - m) / bm):.2f}x "
                           f"the bound, first {np.flatnonzero(bad)[0]}")
    bv = var_bound(y, K) + 4 * U32 * var + 3 * U32 * eps
    dv = np.abs(1.0 / invstd ** 2 - eps - var)
    bad = dv > bv
    assert not bad.any(), (f"var: {int(bad.sum())} channels off, worst {np.max(dv / bv):.2f}x the bound, "
                           f"first {np.flatnonzero(bad)[0]}")
    lo, hi = 1 / np.sqrt(var + bv + eps), 1 / np.sqrt(np.maximum(var - bv, 0) + eps)
    assert np.all((invstd >= lo * (1 - 2 * U32)) & (invstd <= hi * (1 + 2 * U32))), "invstd"
    return var, bv


def _ulp(a):
    return np.spacing(np.abs(np.asarray(a, np.float32))).astype(np.float64)


def check_affine_and_running(scale, shift, mean, invstd, gamma, beta, before, after, n, var64, bv):
    """The rest of the finalize pass, per channel, from the float32 values it stored (views 1-4),
    gamma, beta and the buffers (running_mean, running_var, num_batches_tracked) `before` and
    `after` the step; n rows; (var64, bv) from `check_stats`.

      scale = gamma invstd                   to 1 ulp
      shift = beta - mean scale              to 1 ulp of either evaluation: the product rounded
                                             before the subtraction, or one fma
      running_mean = 0.9 old + 0.1 mean      to 2 ulp
      running_var = 0.9 old + 0.1 var n / (n - 1)   to 2 ulp plus 0.1 n / (n - 1) times the
                                             variance bound
      num_batches_tracked = old + 1"""
    f32 = np.float32
    scale, shift, mean, invstd = (np.asarray(a, f32) for a in (scale, shift, mean, invstd))
    gamma, beta = np.asarray(gamma, f32), np.asarray(beta, f32)
    want = gamma * invstd
    bad = np.abs(scale.astype(np.float64) - want) > _ulp(want)
    assert not bad.any(), f"scale: {int(bad.sum())} channels, first {np.flatnonzero(bad)[0]}"
    plain = beta - mean * scale
    fused = (beta.astype(np.float64) - mean.astype(np.float64) * scale.astype(np.float64)).astype(f32)
    s64 = shift.astype(np.float64)
    bad = (np.abs(s64 - plain) > _ulp(plain)) & (np.abs(s64 - fused) > _ulp(fused))
    assert not bad.any(), f"shift: {int(bad.sum())} channels, first {np.flatnonzero(bad)[0]}"
    rm0, rv0, nbt0 = (np.asarray(a, np.float64) for a in before)
    rm1, rv1, nbt1 = (np.asarray(a, np.float64) for a in after)
    want = 0.9 * rm0 + 0.1 * mean.astype(np.float64)
    bad = np.abs(rm1 - want) > 2 * _ulp(want)
    assert not bad.any(), f"running_mean: {int(bad.sum())} channels, first {np.flatnonzero(bad)[0]}"
    unb = n / (n - 1.0) if n > 1 else 1.0
    want = 0.9 * rv0 + 0.1 * var64 * unb
    bad = np.abs(rv1 - want) > 2 * _ulp(want) + 0.1 * unb * bv
    assert not bad.any(), (f"running_var: {int(bad.sum())} channels, worst "
                           f"{np.max(np.abs(rv1 - want) / (2 * _ulp(want) + 0.1 * unb * bv)):.2f}x, first "
                           f"{np.flatnonzero(bad)[0]}")
    assert int(nbt1) == int(nbt0) + 1, f"num_batches_tracked {int(nbt0)} -> {int(nbt1)}"


def device_stats(y, count=None, group=128, drop=None):
    """The device formula on the CPU (a faithful emulation the checkers must accept): float32
    sums per `group` rows, float64 combine, var = q / count - mean^2 clamped at 0, float32 mean
    and invstd (eps 1e-5).  `drop`: a group left out (a planted fault).  Returns mean, invstd
    (float32) and the float64 variance before the rounding."""
    y = np.asarray(y, np.float32)
    M = y.shape[0]
    s = np.zeros(y.shape[1])
    q = np.zeros(y.shape[1])
    for g, r in enumerate(range(0, M, group)):
        if g == drop:
            continue
        blk = y[r:r + group]
        s += blk.sum(0, dtype=np.float32)
        q += (blk.astype(np.float64) ** 2).astype(np.float32).sum(0, dtype=np.float32)
    n = float(M if count is None else count)
    mean = s / n
    var = np.maximum(q / n - mean * mean, 0)
    return mean.astype(np.float32), (1 / np.sqrt(var + 1e-5)).astype(np.float32), var


def finalize(mean64, var, gamma, beta, before, n, unbiased=True, bump=1):
    """bn_train_final on the CPU from the float64 mean and variance: (scale, shift, running_mean,
    running_var, num_batches_tracked) in float32 arithmetic."""
    f32 = np.float32
    mean, invstd = mean64.astype(f32), (1 / np.sqrt(var + 1e-5)).astype(f32)
    scale = np.asarray(gamma, f32) * invstd
    shift = np.asarray(beta, f32) - mean * scale
    unb = var * n / (n - 1) if unbiased and n > 1 else var
    rm = (f32(1) - f32(0.1)) * np.asarray(before[0], f32) + f32(0.1) * mean
    rv = (f32(1) - f32(0.1)) * np.asarray(before[1], f32) + f32(0.1) * unb.astype(f32)
    return scale, shift, rm, rv, int(before[2]) + bump


# --------------------------------------------------------------------- the oracles, traced
def case(net, base, depth, shape, math="fp32"):
    tag = f"{net}{base}" + ("_bf16" if math == "bf16" else "")
    return dict(id=f"{tag}_{shape[0]}x{shape[1]}x{shape[2]}", net=net, base=base, depth=depth, shape=shape,
                math=math)


UNET = case("unet", 64, 4, (2, 64, 64))
SHAPED = [UNET, case("mod", 64, 3, (2, 64, 64)), case("res", 64, 3, (2, 64, 64)),
          case("mod", 16, 3, (1, 32, 64)), case("res", 16, 3, (1, 32, 64))]
BLACK_SHAPE = (3, 32, 64)


def at_shape(c, shape):
    return case(c["net"], c["base"], c["depth"], shape, c["math"])


def oracle_of(c):
    """(make_params(seed), init_buffers(), forward(x, P, B, training)) of case c's fp32 oracle."""
    from oracle import mod_ref_cpu as MO
    from oracle import unet_ref_cpu as O
    if c["net"] == "unet":
        return O.make_params, O.init_buffers, O.forward
    b, d = c["base"], c["depth"]
    if c["net"] == "mod":
        return (lambda s: MO.make_params(s, b, d)), (lambda: MO.init_buffers(b, d)), MO.make_forward(d)
    return (lambda s: MO.res_make_params(s, b, d)), (lambda: MO.res_init_buffers(b, d)), MO.make_res_forward(d)


def family(name, c, seed=33):
    """Family `name` at case c's shape and depth."""
    return FAMILIES[name](seed, *c["shape"], c["depth"])


def trace_oracle(c, P, x, dtype=torch.float32):
    """One training forward of case c's oracle with every BatchNorm input and every max-pool
    input recorded: {"bn": [(name, z)], "pools": [(X, name of the BN before it, its z)], "buffers"}
    (NCHW tensors).  What a pool's pass reads on the device: z and that BN's affine without ReLU
    ("unet", ReLU before BN), z, the affine and ReLU ("mod"), X alone ("res")."""
    from oracle import mod_ref_cpu as MO
    from oracle import unet_ref_cpu as O
    _, init_buffers, forward = oracle_of(c)
    out = {"bn": [], "pools": []}
    bn0, mp0, mp1 = O._bn, O._maxpool, MO._maxpool

    def bn(z, P_, B_, name, training):
        out["bn"].append((name, z.detach()))
        return bn0(z, P_, B_, name, training)

    def pool(orig):
        def f(X):
            out["pools"].append((X.detach(),) + out["bn"][-1])
            return orig(X)
        return f

    O._bn, O._maxpool, MO._maxpool = bn, pool(mp0), pool(mp1)
    try:
        B = {k: v.to(dtype) if v.is_floating_point() else v.clone() for k, v in init_buffers().items()}
        with torch.no_grad():
            out["logits"] = forward(x.to(dtype), {k: v.to(dtype) for k, v in P.items()}, B, True)
        out["buffers"] = B
    finally:
        O._bn, O._maxpool, MO._maxpool = bn0, mp0, mp1
    return out


def rows(z):
    """NCHW tensor -> (N H W, C) float array, the rows the device stores."""
    return z.permute(0, 2, 3, 1).reshape(-1, z.shape[1]).numpy()


def pool_operands(c, tr, lvl, P):
    """(y4 (N, Ho, Wo, C, 4), sc, sh, relu) of pooled level lvl as the oracle's trace tr has them,
    the affine finalized by the device formula (`device_stats`, `finalize`)."""
    X, name, z = tr["pools"][lvl]
    if c["net"] == "res":
        return windows(X.float().numpy()).transpose(0, 2, 3, 1, 4), None, None, 0
    zr = rows(z.float())
    m, _, var = device_stats(zr)
    sc, sh = finalize(m.astype(np.float64), var, P[name + ".weight"].numpy(), P[name + ".bias"].numpy(),
                      (0 * m, 0 * m + 1, 0), zr.shape[0])[:2]
    return windows(z.float().numpy()).transpose(0, 2, 3, 1, 4), sc, sh, int(c["net"] == "mod")


MIN_FOUR, MIN_TWO = 16, 16


def four_way_reachable(c, fam, lvl):
    """Whether ANY pooled window of level lvl can hold four bit-equal inputs on family fam.  The
    pools of "unet" and "res" read post-ReLU values, whose exact zeros tie at every level.  The
    "mod" pool reads conv outputs ahead of BN -> ReLU, which tie only over a flat receptive
    field: the flat span of a region shrinks by 1, 3, 4, 4 pixels of level 0, 1, 2, 3 from the
    image border (zero padding) and by 2, 3, 4, 4 from a neighbouring region.  So a 32-row image
    has no flat row left at level 2 (8 rows, 4 lost from either border) whatever it shows, and
    the 9- and 11-pixel rectangles of `blocks` have none left at level 1 (11 pixels are 5 of level
    1, 3 lost from either side)."""
    if c["net"] != "mod":
        return True
    if fam == "blocks":
        return lvl == 0
    edge = (1, 3, 4, 4)[lvl]
    span = (min(c["shape"][1:]) >> lvl) - 2 * edge
    if fam == "ddti_like":     # the zero columns: 30 % of the width, speckle on one side
        span = min(span, (int(round(0.3 * c["shape"][2])) >> lvl) - edge - (2, 3, 4, 4)[lvl])
    return span >= 3
