"""The networks on structured images (tests/structured_inputs.py): exact-zero margins, flat
blocks, uint8-quantised speckle, an all-black sample, and images squeezed towards 1.

Winners: on every pooled level of the training forward's workspace the recorded max-pool winners
keep torch's rule on the inputs the pass read (`check_winners`: first of bit-equal inputs, never
below the window maximum, never after a larger candidate), with at least 16 four-way exact-tie
windows per level that can hold one and 16 two-way windows of either kind at level 0 of
`blocks` -- the counts tests/test_structured_cpu.py establishes on the fp32 oracle -- and agree
with the fp32 oracle's own max_pool2d indices wherever the oracle sees an exact tie.

Statistics: on every BatchNorm layer the finalized mean / invstd (debug views 3, 4) stay within
the worst case of the documented arithmetic against the float64 statistics of the stored rows
(`check_stats`), the affine and the running buffers follow from them to the ulp
(`check_affine_and_running`); measured against torch's fp32 CPU BatchNorm on the oracle's rows
in profiles/structured_stats.txt.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import structured_inputs as S
from _helpers import hip_model, options

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(REPO, "profiles", "structured_stats.txt")
EPS = 1e-5
SEED = 7


@pytest.fixture(autouse=True, scope="module")
def _threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def _arm(c, **opts):
    return (c, opts)


BF16 = [S.case(net, 64, 3, (2, 64, 64), "bf16") for net in ("mod", "res")]
F32_ARMS = [_arm(c, x3=x3) for c in S.SHAPED for x3 in (1, 0)]
# pool_fuse / head_fuse are on by default: flipped for one case per network
ARMS = F32_ARMS + [_arm(c) for c in BF16] + [_arm(c, pool_fuse=0, head_fuse=0) for c in S.SHAPED[:3]]


def _arm_id(a):
    return a[0]["id"] + "".join(f"/{k}={v}" for k, v in a[1].items())


def _model(c, P):
    if c["net"] == "unet":
        return hip_model(P, DEV)
    import unet_hip
    from oracle import mod_ref_cpu as MO
    cls = unet_hip.ModUNet if c["net"] == "mod" else unet_hip.ResUNet
    m = cls(1, 1, base_filters=c["base"], depth=c["depth"], mfma_dtype=c["math"])
    sd = m.state_dict()
    init = MO.init_buffers if c["net"] == "mod" else MO.res_init_buffers
    for k, v in list(P.items()) + list(init(c["base"], c["depth"]).items()):
        sd[k] = v.clone()
    m.load_state_dict(sd)
    return m.to(DEV).train()


def _bn_names(c):
    from oracle import mod_ref_cpu as MO
    from oracle import unet_ref_cpu as O
    if c["net"] == "unet":
        return list(zip(O.BN_LAYERS, O.BN_CHANNELS))
    return (MO.bn_layers if c["net"] == "mod" else MO.res_bn_layers)(c["base"], c["depth"])


def _forward_views(m, x, c):
    """The workspace of one training forward on x (running buffers untouched: clones), read back:
    per BN layer the stored rows and views 1-4 sliced to the real channels, per pooled level the
    operands of the pass (see `S.trace_oracle`) and its winners."""
    st = m.flatten_()
    N, _, H, W = x.shape
    with torch.no_grad():
        _, ws = st.rt.forward(st.param_arena, st.bn_arena.clone(), st.nbt_arena.clone(), x.to(DEV),
                              training=True)
        torch.cuda.synchronize()
    view = lambda kind, i: st.rt.debug_view(ws, N, H, W, True, kind, i)
    bn = []
    for i, (name, C) in enumerate(_bn_names(c)):
        z, off = view(0, i)
        bn.append(dict(name=name, y=z[:, off:off + C].cpu().numpy(),
                       **{k: view(kind, i)[:C].cpu().numpy()
                          for kind, k in ((1, "scale"), (2, "shift"), (3, "mean"), (4, "invstd"))}))
    pools = []
    for lvl in range(c["depth"]):
        C, h, w = c["base"] << lvl, H >> lvl, W >> lvl
        idx = view(8, lvl)[0][:, :C].cpu().numpy().reshape(N, h // 2, w // 2, C)
        if c["net"] == "res":
            v, off = view(9, lvl)
            y, sc, sh = v[:, off:off + C].cpu().numpy(), None, None
        else:
            b = bn[2 * lvl + 1]
            y, sc, sh = b["y"], b["scale"], b["shift"]
        assert y.shape == (N * h * w, C)
        y4 = y.reshape(N, h // 2, 2, w // 2, 2, C).transpose(0, 1, 3, 5, 2, 4).reshape(N, h // 2, w // 2, C, 4)
        pools.append((np.ascontiguousarray(y4), sc, sh, int(c["net"] == "mod"), idx))
    del ws
    return bn, pools


_ORACLE = {}


def _oracle(c, fam):
    """(P, x, t, fp32 trace, fp64 trace) of case c's oracle on family fam, computed once and shared
    by the arms.  Do not modify."""
    key = (c["net"], c["base"], c["shape"], fam)
    if key not in _ORACLE:
        P = S.oracle_of(c)[0](SEED)
        x, t = S.family(fam, c)
        _ORACLE[key] = (P, x, t, S.trace_oracle(c, P, x), S.trace_oracle(c, P, x, torch.float64))
    return _ORACLE[key]


def _oracle_ties(c, tr, lvl, y4):
    """The fp32 oracle's own max_pool2d winners (N, Ho, Wo, C) of level lvl, and the windows it
    sees as an exact tie that the device must see too: two or more inputs bit-equal to the maximum,
    every other input below it by more than 1e-3 of the level's largest value (ten times the
    forward bar of 1e-4, so a device value cannot climb over it), the tied inputs bit-equal among
    the device's stored inputs y4 too (a ReLU input within rounding of zero is 0 in one evaluation
    and 1e-8 in the other: arithmetic, not the tie rule), and not a dead window of a ReLU the
    device applies after the max (every input 0: `check_winners` exempts it the same way)."""
    X = tr["pools"][lvl][0].float()
    _, flat = F.max_pool2d(X, 2, 2, return_indices=True)
    Wl = X.shape[3]
    k = (((flat // Wl) % 2) * 2 + (flat % Wl) % 2).numpy().transpose(0, 2, 3, 1)
    w = S.windows(X.numpy()).transpose(0, 2, 3, 1, 4)
    top = w.max(-1, keepdims=True)
    tied = w == top
    clear = (tied | (w < top - 1e-3 * np.abs(w).max())).all(-1)
    b = y4.view(np.uint32)
    on_device = ((b == np.take_along_axis(b, k[..., None].astype(np.int64), -1)) | ~tied).all(-1)
    sure = (tied.sum(-1) >= 2) & clear & on_device
    if c["net"] == "mod":
        sure &= top[..., 0] > 0
    return k, sure


WIN_CASES = [(a, fam) for a in ARMS for fam in ("margins", "blocks", "black_sample")]


@pytest.mark.parametrize("arm,fam", WIN_CASES, ids=[f"{_arm_id(a)}-{f}" for a, f in WIN_CASES])
def test_pool_winners_keep_torchs_rule_on_ties(arm, fam):
    c0, opts = arm
    c = S.at_shape(c0, S.BLACK_SHAPE) if fam == "black_sample" else c0
    P, x, t, tr, _ = _oracle(c, fam)
    m = _model(c, P)
    with options(m.flatten_().rt, **opts):
        _, pools = _forward_views(m, x, c)
    del m
    for lvl, (y4, sc, sh, relu, idx) in enumerate(pools):
        n = S.check_winners(y4, sc, sh, relu, idx)
        k, sure = _oracle_ties(c, tr, lvl, y4)
        same = bool((idx[sure] == k[sure]).all()) if c["math"] == "fp32" else None
        print(f"{_arm_id(arm)} {fam} level {lvl}: ties {n}; oracle exact-tie windows {int(sure.sum())}, "
              f"same winner: {same}")
        if S.four_way_reachable(c, fam, lvl):
            assert n["four"] >= S.MIN_FOUR, (lvl, n)
        if fam == "blocks" and lvl == 0:
            assert min(n["first1"], n["first2"]) >= S.MIN_TWO, n
        if c["math"] == "fp32":      # (the bf16 path's values are not the fp32 oracle's)
            assert sure.sum() >= S.MIN_FOUR or not S.four_way_reachable(c, fam, lvl)
            assert same, (lvl, int((idx[sure] != k[sure]).sum()))


# ----------------------------------------------------------------------------------- statistics
STAT_FAMILIES = ("offset0", "offset0.9", "offset0.99", "ddti_like", "black_sample")
STAT_CASES = [(a, fam) for a in F32_ARMS for fam in STAT_FAMILIES]
_ROWS = {}


@pytest.fixture(autouse=True, scope="module")
def _stats_table():
    """profiles/structured_stats.txt, rewritten whole from the statistics cases of this run: per
    arm, family and BN layer the conditioning of the stored rows and the relative variance error
    of the device and of torch's fp32 CPU BatchNorm, each against float64 on its own rows."""
    yield
    if not _ROWS:
        return
    head = ["# Written by tests/test_gpu_structured.py (the statistics cases of one run).",
            "# Per arm, input family and BatchNorm layer (forward order): rows n, the worst channel's",
            "# |mean| / std of the stored rows, and the worst channel's relative error of the batch variance",
            "# over the channels with var64 >= eps = 1e-5 (`lo`: channels below that, left out -- there the",
            "# error relative to var64 measures the rows' own rounding, not the reduction): the device's",
            "# (1 / invstd^2 - eps of debug view 4) against float64 on the rows it stored, and torch's fp32",
            "# CPU BatchNorm on the fp32 oracle's rows against float64 on those."]
    with open(TABLE, "w") as f:
        f.write("\n".join(head + [_ROWS[k] for k in sorted(_ROWS)]) + "\n")


def _rel_var_err(var, var64):
    ok = var64 >= EPS
    return float(np.max(np.abs(var - var64)[ok] / var64[ok])) if ok.any() else 0.0


@pytest.mark.parametrize("arm,fam", STAT_CASES, ids=[f"{_arm_id(a)}-{f}" for a, f in STAT_CASES])
def test_bn_statistics_within_the_derived_bound(arm, fam):
    c0, opts = arm
    c = S.at_shape(c0, S.BLACK_SHAPE) if fam == "black_sample" else c0
    P, x, t, tr32, tr64 = _oracle(c, fam)
    m = _model(c, P)
    with options(m.flatten_().rt, **opts):
        bn, _ = _forward_views(m, x, c)
        before = {k: v.detach().cpu().numpy().copy() for k, v in m.named_buffers()}
        m(x.to(DEV))
        torch.cuda.synchronize()
        after = {k: v.detach().cpu().numpy().copy() for k, v in m.named_buffers()}
    del m
    failures = []
    for i, b in enumerate(bn):
        name, y = b["name"], b["y"]
        n = y.shape[0]
        m64, v64, _, _ = S.stats64(y)
        dev_err = _rel_var_err(1.0 / b["invstd"].astype(np.float64) ** 2 - EPS, v64)
        cond = float(np.max(np.abs(m64) / np.sqrt(v64 + EPS)))
        lo = int((v64 < EPS).sum())
        # torch's fp32 CPU BatchNorm on the fp32 oracle's rows, against float64 on the same rows
        z32 = tr32["bn"][i][1]
        _, _, inv = torch.native_batch_norm(z32, None, None, None, None, True, 0.1, EPS)
        ref_err = _rel_var_err(1.0 / inv.double().numpy() ** 2 - EPS, S.stats64(S.rows(z32))[1])
        line = (f"{_arm_id(arm):28s} {fam:12s} {i:2d} {name:18s} n {n:5d} lo {lo:3d}  |mean|/std {cond:9.2e}  "
                f"var err device {dev_err:.2e}  torch fp32 {ref_err:.2e}")
        print("stats:", line)
        _ROWS[(_arm_id(arm), fam, i)] = line
        try:
            var64, bv = S.check_stats(y, n, b["mean"], b["invstd"], EPS)
            S.check_affine_and_running(
                b["scale"], b["shift"], b["mean"], b["invstd"], P[name + ".weight"].numpy(),
                P[name + ".bias"].numpy(),
                *[tuple(d[f"{name}.{k}"] for k in ("running_mean", "running_var", "num_batches_tracked"))
                  for d in (before, after)], n, var64, bv)
        except AssertionError as e:
            failures.append(f"{name}: {e}")
    assert not failures, failures


# ------------------------------------------------------------------- network bars, dead channels
def _train_step(m, x, t):
    import unet_hip
    logits = m(x.to(DEV))
    losses = unet_hip.seg_losses(logits, t.to(DEV))
    (losses[0] + losses[1]).backward()
    torch.cuda.synchronize()
    return logits.detach().cpu().double()


def _eval_forward(c):
    """(forward_fn, bf16) for `_helpers.check_eval`: the case's oracle, bf16 operands where its
    math is bf16."""
    from oracle import mod_ref_cpu as MO
    import res_bf16_ref as RB
    if c["math"] != "bf16":
        return S.oracle_of(c)[2], False
    return (MO.make_forward(c["depth"], bf16=True) if c["net"] == "mod"
            else RB.make_res_forward(c["depth"], bf16=True)), True


def _check_eval(m, c, x, t):
    """`_helpers.check_eval` after the step: at its own bar (1e-4) in f32; in bf16 at the bar of
    tests/test_gpu_res_bf16.py::test_res_bf16_eval_and_bn_buffers, 1e-4 plus twice the bf16
    oracle's own fp32-vs-fp64 spread in eval mode from this path's parameters and buffers."""
    from _helpers import _to64, check_eval, rel_max
    fwd, bf16 = _eval_forward(c)
    tol = 1e-4
    if bf16:
        Pc = {k: v.detach().cpu().clone() for k, v in m.named_parameters()}
        Bc = {k: v.detach().cpu().clone() for k, v in m.named_buffers()}
        with torch.no_grad():
            tol += 2 * rel_max(fwd(x, Pc, Bc, False).numpy(), fwd(x.double(), _to64(Pc), _to64(Bc), False).numpy())
    check_eval(m, fwd, x, t, tol)


def _pinned_step(c, opts, P, x, t, tag):
    """One training step of case c under opts on (x, t), held to the pinned fp64 bars as the noise
    tests hold theirs: tests/masked.py (step, bars, check: what check_on_branches runs, without
    adding rows to its table) for the models/mod.py networks, tests/test_gpu_x3.py for the
    models/model.py network.  Returns the model (gradients in place) and the forward's BN views."""
    import masked as MK
    import test_gpu_x3 as X3
    m = _model(c, P)
    with options(m.flatten_().rt, **opts):
        bn, _ = _forward_views(m, x, c)
        br = X3._relu_masks(m, x) if c["net"] == "unet" else MK.device_branches(m, x, c)
        logits = _train_step(m, x, t)
    grads = MK.grads_of(m)
    assert all(torch.isfinite(g).all() for g in grads.values()) and torch.isfinite(logits).all()
    if c["net"] == "unet":
        X3._check_masked(grads, X3._masked_fp64_step(P, x, t, br), tag)
    else:
        assert (len(br[0]), len(br[1])) == MK.n_decisions(c)
        ref = MK.step(c, P, x, t, True, br)
        MK.check(grads, logits, ref, MK.bars(c, P, x, t, br, ref, opts.get("x3", 1)), tag)
    return m, bn, grads


# The model.py network (depth 4) at 64 x 64 keeps 11 x 13 pixels of speckle inside the margins, and
# the 32 rows of its bottleneck are nearly flat.  There the forward's variance, q / n - mean^2 from
# f32 partial sums, is the limit: measured on the device, middle.1.0.weight 1.15e-3 (margins) and
# 4.3e-4 (black_sample) against the bar of 1e-4, the same with x3 off and with the fused passes
# off; the fp32 CPU oracle on the same branches has 2.5e-5, and 5.0e-3 once its batch variance is
# replaced by that formula (`structured_inputs.device_stats`), so the cancellation alone accounts
# for it.  Frames with three quarters of black margin are not what the workload shows (`ddti_like`:
# 30 %), so this network's bars run on `ddti_like`; its winners and statistics run on every family.
BAR_CASES = [(a, fam) for a in ARMS for fam in ("margins", "ddti_like", "black_sample")
             if a[0]["net"] != "unet" or fam == "ddti_like"]


@pytest.mark.parametrize("arm,fam", BAR_CASES, ids=[f"{_arm_id(a)}-{f}" for a, f in BAR_CASES])
def test_step_on_structured_image_vs_pinned_fp64(arm, fam):
    """Logits and every gradient of one training step on a structured image against the fp64
    oracle on this path's own branches, at the bars of the noise tests (4x / 12x the pinned fp32
    oracle's own error, 2x the pinned bf16 oracle's spread; the model.py network's absolute
    bars), then the eval-mode forward from the updated running statistics."""
    c0, opts = arm
    c = S.at_shape(c0, S.BLACK_SHAPE) if fam == "black_sample" else c0
    P, x, t, _, _ = _oracle(c, fam)
    m, _, _ = _pinned_step(c, opts, P, x, t, f"{_arm_id(arm)}-{fam}")
    with options(m.flatten_().rt, **opts):
        _check_eval(m, c, x, t)


# fl(1 / sqrt(eps)) with eps the float32 1e-5 the runtime (and torch's float BatchNorm) holds
INVSTD_EPS = np.float32(1.0 / np.sqrt(np.float64(np.float32(EPS))))
DEAD = 5  # the planted channel


def test_dead_channel_model_network():
    """models/model.py network on the ddti-like image with encoder1.0.bias[5] = -10: the ReLU
    output of that channel is 0 at every pixel, its batch variance exactly 0.  mean 0, invstd
    fl(1 / sqrt(eps)), and the BN output fma(0, scale, shift) = shift equals beta bit for bit;
    dgamma and the conv's weight and bias gradients of the channel are exactly 0 (the ReLU passes
    nothing); everything is finite and every tensor stays at the pinned bars."""
    c = S.UNET
    P = {k: v.clone() for k, v in S.oracle_of(c)[0](SEED).items()}
    P["encoder1.0.bias"][DEAD] = -10.0
    x, t = S.family("ddti_like", c)
    m, bn, g = _pinned_step(c, {}, P, x, t, "unet64-dead-channel")
    b = bn[0]
    assert not b["y"][:, DEAD].any()
    assert b["mean"][DEAD] == 0 and b["invstd"][DEAD] == INVSTD_EPS
    beta = P["encoder1.2.bias"].numpy()
    assert b["shift"][DEAD].view(np.uint32) == beta[DEAD].view(np.uint32)
    assert b["scale"][DEAD] == P["encoder1.2.weight"].numpy()[DEAD] * INVSTD_EPS
    assert g["encoder1.2.weight"][DEAD] == 0
    assert not g["encoder1.0.weight"][DEAD].any() and g["encoder1.0.bias"][DEAD] == 0
    sd = m.state_dict()
    assert float(sd["encoder1.2.running_mean"][DEAD]) == 0
    assert float(sd["encoder1.2.running_var"][DEAD]) == float(np.float32(1) - np.float32(0.1))


@pytest.mark.parametrize("c", [S.SHAPED[1], S.SHAPED[2]] + BF16, ids=lambda c: c["id"])
def test_constant_channel_mod_networks(c):
    """models/mod.py networks on the ddti-like image with every weight of output channel 5 of the
    first conv and of the bottleneck's second 3x3 conv zeroed: z = 0 there, so views 3 and 4 are
    exactly (0, fl(1 / sqrt(eps))) and dgamma exactly 0; that channel's weight gradient, which the
    backward amplifies by gamma / sqrt(eps), and every other tensor stay at the pinned bars."""
    res = c["net"] == "res"
    first, deep = ("encoders.0.conv.0", "bottleneck.conv.3") if res else ("encoders.0.0", "bottleneck.3")
    P = {k: v.clone() for k, v in S.oracle_of(c)[0](SEED).items()}
    P[first + ".weight"][DEAD] = 0.0
    P[deep + ".weight"][DEAD] = 0.0
    x, t = S.family("ddti_like", c)
    m, bn, g = _pinned_step(c, {}, P, x, t, f"{c['id']}-constant-channel")
    for i, conv in ((0, first), (2 * c["depth"] + 1, deep)):
        b = bn[i]
        assert conv[:-1] + str(int(conv[-1]) + 1) == b["name"]
        assert not b["y"][:, DEAD].any()
        assert b["mean"][DEAD] == 0 and b["invstd"][DEAD] == INVSTD_EPS, (conv, b["mean"][DEAD], b["invstd"][DEAD])
        assert g[b["name"] + ".weight"][DEAD] == 0, (conv, float(g[b["name"] + ".weight"][DEAD]))
