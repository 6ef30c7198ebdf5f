"""Eval-mode oracles of the small cases (helper of the tests, not a test; importable without a
GPU): running buffers as a trained network carries them, and the oracle's eval forward traced
layer by layer (tests/test_gpu_eval_coverage.py, tests/test_eval_ref_cpu.py).

`trained_buffers`: per BN layer, the fp64 batch statistics of the case's own input moved by a
deterministic per-channel amount -- near them, so eval activations are scaled as in a trained
network (fresh buffers, mean 0 / var 1, leave BN a near-identity on activations of another
scale); not equal to them, so a forward that used batch statistics, or another layer's buffers,
misses the bars.

`eval_trace`: what the device stores per conv (debug view 0: post-ReLU and ahead of BN for
models/model.py, the conv output ahead of BN for models/mod.py), per residual block (view 9)
and the logits.
"""
import numpy as np
import torch

import res_bf16_ref as RB
from _helpers import _to64
from oracle import mod_ref_cpu as MO
from oracle import unet_ref_cpu as O
from oracle import weights as Wt

T_MEAN, T_VAR = 3000, 3500      # oracle.weights tensor indices of u_c, v_c (+ BN layer index)
BUF_SEED = 91
MEAN_SHIFT = 0.25               # running_mean = mean + MEAN_SHIFT sqrt(var) u_c


def fns(c, bf16=False):
    """(make_params(seed), init_buffers(), forward(x, P, B, training)) of case c's oracle; bf16:
    the bf16-operand oracle (mod / res)."""
    b, d = c["base"], c["depth"]
    if c["net"] == "unet":
        assert not bf16
        return O.make_params, O.init_buffers, O.forward
    if c["net"] == "mod":
        return (lambda s: MO.make_params(s, b, d)), (lambda: MO.init_buffers(b, d)), MO.make_forward(d, bf16)
    fwd = RB.make_res_forward(d, True) if bf16 else MO.make_res_forward(d)
    return (lambda s: MO.res_make_params(s, b, d)), (lambda: MO.res_init_buffers(b, d)), fwd


def bn_names(c):
    if c["net"] == "unet":
        return list(O.BN_LAYERS)
    layers = MO.bn_layers if c["net"] == "mod" else MO.res_bn_layers
    return [n for n, _ in layers(c["base"], c["depth"])]


def batch_stats(c, P, x, bf16=None):
    """{BN layer: (mean, biased variance)} (fp64, per channel) of one training-mode fp64 forward
    of case c's oracle on x."""
    bf16 = (c["math"] == "bf16") if bf16 is None else bf16
    _, init_buffers, forward = fns(c, bf16)
    stats = {}
    bn0 = O._bn

    def bn(z, P_, B_, name, training):
        stats[name] = (z.detach().mean((0, 2, 3)), z.detach().var((0, 2, 3), unbiased=False))
        return bn0(z, P_, B_, name, training)

    O._bn = bn
    try:
        with torch.no_grad():
            forward(x.double(), _to64(P), _to64(init_buffers()), True)
    finally:
        O._bn = bn0
    return stats


def trained_buffers(c, P, x):
    """Running buffers near, not equal to, the batch statistics of x (module docstring):
    running_mean = mean + 0.25 sqrt(var) u_c, running_var = var 2^(v_c), u_c, v_c in [-1, 1)
    from oracle.weights.uniform per layer and channel; float32; num_batches_tracked = 1."""
    stats = batch_stats(c, P, x)
    names = bn_names(c)
    assert set(names) == set(stats), "a BN layer the training forward did not reach"
    B = {}
    for i, name in enumerate(names):
        m, v = (a.numpy() for a in stats[name])
        u = 2 * Wt.uniform(BUF_SEED, T_MEAN + i, m.size) - 1
        w = 2 * Wt.uniform(BUF_SEED, T_VAR + i, m.size) - 1
        B[f"{name}.running_mean"] = torch.from_numpy((m + MEAN_SHIFT * np.sqrt(v) * u).astype(np.float32))
        B[f"{name}.running_var"] = torch.from_numpy((v * 2.0 ** w).astype(np.float32))
        B[f"{name}.num_batches_tracked"] = torch.tensor(1, dtype=torch.long)
    return B


def eval_trace(c, P, B, x, dtype, bf16=False, bn_hook=None, conv_hook=None):
    """Case c's oracle in eval mode on x, evaluated in `dtype`: {"conv": the stored output of
    every conv (NCHW, forward order = conv index), "bn": every BN layer's output, "out": every
    residual block's output (ResUNet; else empty), "logits"}.  bn_hook(z, P, B, name) -> BN(z)
    replaces the eval BatchNorm, conv_hook(i, z) -> z' a conv's stored output ahead of its BN
    (the mutations of tests/test_eval_ref_cpu.py); neither is set in a reference run."""
    _, _, forward = fns(c, bf16)
    out = {"conv": [], "bn": [], "out": []}
    unet = c["net"] == "unet"
    bn0, relu0 = O._bn, MO._relu
    calls = [0]

    def bn(z, P_, B_, name, training):
        assert not training
        if conv_hook is not None:
            z = conv_hook(len(out["bn"]), z)
        if not unet:
            out["conv"].append(z.detach())
        y = bn0(z, P_, B_, name, False) if bn_hook is None else bn_hook(z, P_, B_, name)
        out["bn"].append(y.detach())
        return y

    def relu(v):
        r = relu0(v)
        calls[0] += 1
        if c["net"] == "res" and calls[0] % 2 == 0:
            out["out"].append(r.detach())
        return r

    O._bn, MO._relu = bn, relu
    try:
        Pd = {k: v.to(dtype) for k, v in P.items()}
        Bd = {k: v.to(dtype) if v.is_floating_point() else v.clone() for k, v in B.items()}
        with torch.no_grad():
            if unet:
                out["logits"] = forward(x.to(dtype), Pd, Bd, False, record=out["conv"])
            else:
                out["logits"] = forward(x.to(dtype), Pd, Bd, False)
    finally:
        O._bn, MO._relu = bn0, relu0
    n = 2 * (2 * c["depth"] + 1)
    assert len(out["conv"]) == len(out["bn"]) == n and len(out["out"]) in (0, n // 2)
    return out


def rows(z):
    """NCHW tensor -> (N H W, C) float64 array, the rows the device stores."""
    return z.permute(0, 2, 3, 1).reshape(-1, z.shape[1]).double().numpy()


def layers(tr):
    """[(tag, rows)] of a trace: conv0 .. , out0 .. , logits."""
    return ([(f"conv{i}", rows(z)) for i, z in enumerate(tr["conv"])] +
            [(f"out{b}", rows(z)) for b, z in enumerate(tr["out"])] + [("logits", rows(tr["logits"]))])


def meaningful(tr):
    """The meaningful-input condition on an fp64 eval trace: every BN layer's output between 10 %
    and 90 % positive, no stored layer all zero, max|logits| >= 1e-2.  Returns the failures."""
    bad = []
    for i, y in enumerate(tr["bn"]):
        f = float((y > 0).double().mean())
        if not 0.1 <= f <= 0.9:
            bad.append(f"bn{i}: {100 * f:.1f} % positive")
    for tag, r in layers(tr):
        if not np.any(r):
            bad.append(f"{tag}: all zero")
    if float(tr["logits"].abs().max()) < 1e-2:
        bad.append(f"max|logits| {float(tr['logits'].abs().max()):.2e}")
    return bad


def level_of_conv(c, i):
    b = i // 2
    return b if b <= c["depth"] else 2 * c["depth"] - b


# ------------------------------------------------------------------ the eval finalize's bound
U32 = 2.0 ** -24
BN_EPS32 = np.float32(1e-5)


def affine64(gamma, beta, mean, var):
    """scale = gamma / sqrt(var + eps), shift = beta - mean scale in float64 from the float32
    parameters and buffers (eps: the float32 1e-5 the kernel is given)."""
    g, b, m, v = (np.asarray(a, np.float32).astype(np.float64) for a in (gamma, beta, mean, var))
    sc = g / np.sqrt(v + np.float64(BN_EPS32))
    return sc, b - m * sc


def affine_bounds(gamma, beta, mean, var):
    """Bounds on |scale_dev - scale64| and |shift_dev - shift64| per channel, from
    bn_finalize_eval_kernel's arithmetic (u = 2^-24):

        invstd = 1.f / sqrtf(rvar + eps);  sc = gamma * invstd;  shift = beta - rmean * sc

    The library is built without fast-math and without turning off correctly rounded float32
    division and square root (hipcc's default), so every operation is one rounding, relative u:
    the sum rvar + eps (halved by the square root: u / 2), sqrtf (u), the division (u), the
    product (u) -- |d scale| <= 3.5 u |scale| to first order, taken as 4 u |scale|.  The shift is
    compiled either as a rounded product and a subtraction or, under the default fp-contract, as
    one fma; the wider of the two: |rmean| |d scale| (4 u) + the product's rounding (u), both of
    |rmean scale|, + the final rounding u |shift| -- (5 u |rmean scale| + u |shift|), the second
    order terms (<= 20 u^2) under the 6 taken.  A float32 subnormal is far below every value
    here (scale >= |gamma| 1e-3 at var = 1e6)."""
    sc, sh = affine64(gamma, beta, mean, var)
    m = np.abs(np.asarray(mean, np.float32).astype(np.float64))
    return 4 * U32 * np.abs(sc), 6 * U32 * m * np.abs(sc) + U32 * np.abs(sh)


def check_affine(scale, shift, gamma, beta, mean, var, tag=""):
    """Views 1 / 2 of an eval forward against float64 at `affine_bounds`, and the shift against
    either evaluation from the float32 scale the device stored: the rounded product, or one fma
    (to one ulp: the float64 stand-in for the fma rounds twice).  Returns the worst ratios to
    the bounds (scale, shift)."""
    f32 = np.float32
    scale, shift = np.asarray(scale, f32), np.asarray(shift, f32)
    gamma, beta, mean = (np.asarray(a, f32) for a in (gamma, beta, mean))
    assert np.isfinite(scale).all() and np.isfinite(shift).all(), f"{tag}: non-finite affine"
    sc, sh = affine64(gamma, beta, mean, var)
    bs, bh = affine_bounds(gamma, beta, mean, var)
    es, eh = np.abs(scale - sc), np.abs(shift - sh)
    bad = es > bs
    assert not bad.any(), f"{tag} scale: {int(bad.sum())} channels, first {np.flatnonzero(bad)[0]}"
    bad = eh > bh
    assert not bad.any(), f"{tag} shift: {int(bad.sum())} channels, first {np.flatnonzero(bad)[0]}"
    plain = beta - mean * scale
    fused = (beta.astype(np.float64) - mean.astype(np.float64) * scale.astype(np.float64)).astype(f32)
    ulp = lambda a: np.spacing(np.abs(a)).astype(np.float64)
    s64 = shift.astype(np.float64)
    bad = (np.abs(s64 - plain) > ulp(plain)) & (np.abs(s64 - fused) > ulp(fused))
    assert not bad.any(), f"{tag} shift is neither evaluation: {int(bad.sum())} channels"
    tiny = 1e-300
    return float(np.max(es / np.maximum(bs, tiny))), float(np.max(eh / np.maximum(bh, tiny)))


# ------------------------------------------------------------------ planted buffers (edges)
# kind -> channel of every BN layer (the narrowest layer has 16 channels)
PLANTED = {"var=0": 0, "var=1e-12": 1, "var=1e6": 2, "mean=+1e4": 3, "mean=-1e4": 4, "gamma=0": 5,
           "gamma<0": 6, "beta=+10": 7, "beta=-10": 8}


def plant_params(c, P):
    """A copy of P with the planted gamma / beta channels in every BN layer."""
    P = {k: v.clone() for k, v in P.items()}
    for name in bn_names(c):
        g, b = P[f"{name}.weight"], P[f"{name}.bias"]
        g[PLANTED["gamma=0"]] = 0.0
        g[PLANTED["gamma<0"]] = -g[PLANTED["gamma<0"]].abs()
        b[PLANTED["beta=+10"]], b[PLANTED["beta=-10"]] = 10.0, -10.0
    return P


def planted_buffers(c, P, x):
    """`trained_buffers` with the planted running_var / running_mean channels, built in one fp64
    pass in which every BN layer already normalises with its own planted buffers: the next
    layer's buffers are near the statistics of what the planted network feeds it, so its
    activations stay in range however a planted channel scales (var = 0: x 316)."""
    bf16 = c["math"] == "bf16"
    _, init_buffers, forward = fns(c, bf16)
    names = bn_names(c)
    B = {}

    def bn(z, P_, B_, name, training):
        i = names.index(name)
        m, v = z.mean((0, 2, 3)).numpy(), z.var((0, 2, 3), unbiased=False).numpy()
        u = 2 * Wt.uniform(BUF_SEED, T_MEAN + i, m.size) - 1
        w = 2 * Wt.uniform(BUF_SEED, T_VAR + i, m.size) - 1
        rm, rv = m + MEAN_SHIFT * np.sqrt(v) * u, v * 2.0 ** w
        rv[PLANTED["var=0"]], rv[PLANTED["var=1e-12"]], rv[PLANTED["var=1e6"]] = 0.0, 1e-12, 1e6
        rm[PLANTED["mean=+1e4"]], rm[PLANTED["mean=-1e4"]] = 1e4, -1e4
        B[f"{name}.running_mean"] = torch.from_numpy(rm.astype(np.float32))
        B[f"{name}.running_var"] = torch.from_numpy(rv.astype(np.float32))
        B[f"{name}.num_batches_tracked"] = torch.tensor(1, dtype=torch.long)
        return torch.nn.functional.batch_norm(z, B[f"{name}.running_mean"].double(), B[f"{name}.running_var"].double(),
                                              P_[f"{name}.weight"], P_[f"{name}.bias"], False, 0.1, O.BN_EPS)

    bn0 = O._bn
    O._bn = bn
    try:
        with torch.no_grad():
            forward(x.double(), _to64(P), _to64(init_buffers()), True)
    finally:
        O._bn = bn0
    return {k: B[k] for n in names for k in (f"{n}.running_mean", f"{n}.running_var", f"{n}.num_batches_tracked")}


EDGE_SHAPE = (1, 32, 64)
EDGE_CASES = [dict(id="unet", net="unet", base=64, depth=4, math="fp32", shape=EDGE_SHAPE, opts={}),
              dict(id="mod64", net="mod", base=64, depth=3, math="fp32", shape=EDGE_SHAPE, opts={}),
              dict(id="res64", net="res", base=64, depth=3, math="fp32", shape=EDGE_SHAPE, opts={}),
              dict(id="res16", net="res", base=16, depth=3, math="fp32", shape=EDGE_SHAPE, opts={}),
              dict(id="res64_bf16", net="res", base=64, depth=3, math="bf16", shape=EDGE_SHAPE, opts={})]


def torch_bn_rows(tr64, tr32, P, B, c):
    """{kind: worst over the BN layers of max|y32 - y64| / max|y64| on the planted channel}: torch's
    own float32 CPU batch_norm(training=False) on the float32 oracle's layer input against the
    float64 BatchNorm of the same (float32) input."""
    out = dict.fromkeys(PLANTED, 0.0)
    for i, name in enumerate(bn_names(c)):
        z = tr32["conv"][i]
        for kind, ch in PLANTED.items():
            y64 = bn64(z[:, ch].double().numpy(), P, B, name, ch)
            y32 = tr32["bn"][i][:, ch].double().numpy()
            out[kind] = max(out[kind], float(np.abs(y32 - y64).max() / max(np.abs(y64).max(), 1e-30)))
    return out


def bn64(z, P, B, name, ch):
    sc, sh = affine64(P[f"{name}.weight"][ch], P[f"{name}.bias"][ch], B[f"{name}.running_mean"][ch],
                      B[f"{name}.running_var"][ch])
    return z * sc + sh
