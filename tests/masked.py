"""Branch-pinned fp64 checks of the models/mod.py networks (helper of the tests, not a test;
importable without a GPU).

Every network is judged on its own branches: the ReLU and max-pool decisions of THIS path's
training forward are read back from its workspace (`device_branches`), the fp64 oracle follows
them through the relu_masks / pool_idx hooks of oracle/mod_ref_cpu.py and tests/res_bf16_ref.py
(`step`), and what is left between the two is arithmetic, not a pre-activation within ~1e-6 of
zero that lands on the other side in another evaluation.

Measures (`measure`), per tensor, worst over a class -- "w": conv / ConvT weights (4-d), "o":
every other tensor:
    norm   |a - ref| / |ref|                (Frobenius)
    elem   max|a - ref| / max|ref|
and the logits, norm-relative.

Bars (`bars`), computed from the reference alone, never from the code under test:
  f32 math: the fp32 CPU oracle pinned to the same branches, on x, x (1 + 1e-7) and
      x (1 - 1e-7); each class and each measure gets `margin` x that oracle's worst error against
      the pinned fp64 step on x.  margin 4: what tests/test_gpu_loss_edges.py gives the device
      over "the same formulas in torch CPU float32" (another summation order); 12 for an arm
      that forces x3 = 0 (profiles/r05_x3_masked_bars.txt: the f32-MFMA path at ~2.7x the x3
      path's error on the same footing).  Logits: 1e-5, the pinned bar of tests/test_gpu_x3.py.
  bf16 math: 2x the pinned bf16-operand oracle's own fp32-vs-fp64 spread over the same three
      inputs (the margin the bf16 tests give already), and that 2x spread may not exceed CAP_BF16
      (norm measures): a case whose own spread exceeds it needs another seed, not a wider cap.
"""
import os

import torch

from _helpers import _to64, norm_rel
from oracle import mod_ref_cpu as MO
import res_bf16_ref as RB

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(REPO, "profiles", "masked_bars.txt")
LOGIT_BAR_F32 = 1e-5
CAP_BF16 = 5e-2
MARGIN_X3, MARGIN_F32_MFMA, MARGIN_BF16 = 4.0, 12.0, 2.0
EPS = (0.0, 1e-7, -1e-7)
OLD_FLOOR = 1e-2       # the unpinned f32 floor these bars replace (seeded-fault tests)
MEASURES = ("w_norm", "o_norm", "w_elem", "o_elem")


def make_params(c, seed, gamma=(0.5, 1.5)):
    mk = MO.make_params if c["net"] == "mod" else MO.res_make_params
    return mk(seed, c["base"], c["depth"], *gamma)


def init_buffers(c):
    return (MO.init_buffers if c["net"] == "mod" else MO.res_init_buffers)(c["base"], c["depth"])


def step(c, P, x, t, f64, branches=None, record=None, bf16=None):
    """One oracle training step of case c's network in fp64 or fp32, bf16 operands where the
    case's math is bf16 (or as `bf16` says), on `branches` = (relu_masks, pool_idx) if given."""
    bf16 = (c["math"] == "bf16") if bf16 is None else bf16
    masks, pools = branches if branches is not None else (None, None)
    B = init_buffers(c)
    if f64:
        P, B, x, t = _to64(P), _to64(B), x.double(), t.double()
    kw = dict(depth=c["depth"], relu_masks=masks, pool_idx=pools, record=record)
    if c["net"] == "mod":
        return MO.train_step(P, B, None, x, t, bf16=bf16, **kw)
    if bf16:
        return RB.res_train_step(P, B, None, x, t, bf16=True, **kw)
    return MO.res_train_step(P, B, None, x, t, **kw)


def n_decisions(c):
    """(ReLU decisions, pools) of case c's network: two per block either way."""
    return 2 * (2 * c["depth"] + 1), c["depth"]


def device_branches(m, x, c):
    """The ReLU decisions (boolean NCHW, forward order) and max-pool winner indices of this
    path's training forward on x, under the options in force (the forward is deterministic, so
    they are the ones m(x) takes).

    Inner ReLUs: the kernels decide fmaf(z, scale, shift) > 0 on the stored conv output z (debug
    view 0) and the finalized BN affine (views 1, 2).  An f32 x f32 product is exact in float64,
    so double(z) * double(scale) + double(shift) has the sign of the fma (one rounding of the
    exact value either way); a float32 multiply-then-add rounds the product first and does not.
    ResUNet's outer ReLU: out > 0 of the stored block output (view 9).  Pools: view 8.  Padded
    widths (base 16 / 24 / 48) are sliced back to the real channels."""
    dev = next(m.parameters()).device
    st = m.flatten_()
    N, _, H, W = x.shape
    D, base, res = c["depth"], c["base"], c["net"] == "res"
    with torch.no_grad():
        _, ws = st.rt.forward(st.param_arena, st.bn_arena.clone(), st.nbt_arena.clone(),
                              x.to(dev), training=True)
        torch.cuda.synchronize()

    def nchw(v, lvl, C):
        return v.reshape(N, H >> lvl, W >> lvl, C).permute(0, 3, 1, 2).contiguous().cpu()

    masks = []
    for b in range(2 * D + 1):
        lvl = b if b <= D else 2 * D - b
        C = base << lvl
        for i in (2 * b, 2 * b + 1):
            if res and i == 2 * b + 1:
                v, off = st.rt.debug_view(ws, N, H, W, True, 9, b)
                masks.append(nchw(v[:, off:off + C] > 0, lvl, C))
                continue
            z, off = st.rt.debug_view(ws, N, H, W, True, 0, i)
            sc = st.rt.debug_view(ws, N, H, W, True, 1, i)[:C].double()
            sh = st.rt.debug_view(ws, N, H, W, True, 2, i)[:C].double()
            masks.append(nchw(z[:, off:off + C].double() * sc + sh > 0, lvl, C))
    pools = []
    for lvl in range(D):
        v, _ = st.rt.debug_view(ws, N, H, W, True, 8, lvl)
        C = base << lvl
        pools.append(nchw(v[:, :C], lvl + 1, C))
    del ws
    return masks, pools


def measure(grads, ref_grads):
    """{measure: (worst value, tensor name)} of `grads` against `ref_grads` (see the module
    docstring)."""
    out = {}
    for cls in "wo":
        keys = [k for k, g in ref_grads.items() if (g.dim() == 4) == (cls == "w")]
        en = {k: norm_rel(grads[k], ref_grads[k]) for k in keys}
        ee = {k: float((grads[k].double() - ref_grads[k].double()).abs().max()
                       / max(float(ref_grads[k].abs().max()), 1e-30)) for k in keys}
        kn, ke = max(en, key=en.get), max(ee, key=ee.get)
        out[f"{cls}_norm"], out[f"{cls}_elem"] = (en[kn], kn), (ee[ke], ke)
    return out


def bars(c, P, x, t, branches, ref, x3=1):
    """The bars of case c on `branches`; `ref` is step(c, P, x, t, True, branches)."""
    bf16 = c["math"] == "bf16"
    worst = dict.fromkeys(MEASURES + ("logits",), 0.0)
    for eps in EPS:
        r = step(c, P, x * (1 + eps) if eps else x, t, False, branches)
        for k, (v, _) in measure(r["grads"], ref["grads"]).items():
            worst[k] = max(worst[k], v)
        worst["logits"] = max(worst["logits"], norm_rel(r["logits"], ref["logits"]))
    margin = MARGIN_BF16 if bf16 else MARGIN_X3 if x3 else MARGIN_F32_MFMA
    out = {k: margin * worst[k] for k in MEASURES}
    out["logits"] = MARGIN_BF16 * worst["logits"] if bf16 else LOGIT_BAR_F32
    if bf16:
        assert max(out["w_norm"], out["o_norm"]) <= CAP_BF16, \
            f"{c['id']}: the bf16 oracle's own 2x spread {out} exceeds {CAP_BF16}: change the seed"
    return out


ROWS = {}  # tag -> table line of the checks that ran in this session


def check(grads, logits, ref, bar, tag, rows=None):
    """The pinned comparison: `grads` / `logits` of the path under test against the pinned fp64
    step `ref` at `bar`.  Prints every figure (and keeps the line in `rows`), then asserts."""
    got = measure(grads, ref["grads"])
    e_l = norm_rel(logits, ref["logits"])
    line = (f"{tag:34s} logits {e_l:.2e} / {bar['logits']:.2e}  " +
            "  ".join(f"{k} {got[k][0]:.2e} / {bar[k]:.2e}" for k in MEASURES))
    print("pinned:", line)
    if rows is not None:
        rows[tag] = line
    for k in MEASURES:
        assert got[k][0] <= bar[k], f"{tag} {k} {got[k][1]}: {got[k][0]:.3e} > bar {bar[k]:.3e}"
    assert e_l <= bar["logits"], f"{tag} logits: {e_l:.3e} > bar {bar['logits']:.3e}"
    return got


def check_on_branches(c, P, x, t, br, logits, grads, tag=None, x3=1):
    """Hold one training step of the path under test (logits, gradients: name -> tensor), taken
    under the options `br` = device_branches(m, x, c) was read under, to the pinned bars."""
    assert (len(br[0]), len(br[1])) == n_decisions(c)
    ref = step(c, P, x, t, True, br)
    return check(grads, logits, ref, bars(c, P, x, t, br, ref, x3), tag or c["id"], ROWS)


def grads_of(m):
    return {k: p.grad.detach().cpu().double() for k, p in m.named_parameters()}


def write_table():
    """profiles/masked_bars.txt: measured / bar per check; lines of checks that did not run in
    this session are kept."""
    head = ["# Written by tests/test_gpu_masked.py::test_bars_table_written.",
            "# Pinned fp64 checks (tests/masked.py): device error / bar per case; w = conv and ConvT",
            "# weights, o = every other tensor; norm = |a - ref| / |ref|, elem = max|a - ref| / max|ref|,",
            "# worst tensor of the class.  Bars: f32 4x (x3 = 0 arms 12x) the pinned fp32 CPU oracle's",
            "# worst error over x, x (1 +- 1e-7); bf16 2x the pinned bf16 oracle's fp32-vs-fp64 spread."]
    rows = {}
    if os.path.exists(TABLE):
        for line in open(TABLE):
            if line.strip() and not line.startswith("#"):
                rows[line.split()[0]] = line.rstrip("\n")
    rows.update({k.split()[0]: v for k, v in ROWS.items()})
    with open(TABLE, "w") as f:
        f.write("\n".join(head + [rows[k] for k in sorted(rows)]) + "\n")
    return len(rows)
