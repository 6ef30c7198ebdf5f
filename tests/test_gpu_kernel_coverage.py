"""Every GEMM kernel and tile a production configuration launches -- the bench.py
configurations and the bf16 ResUNet steps main.py trains -- is tied to a small case that is
checked against the fp64 oracle (tests/kernel_cases.py: PRODUCTION, SMALL, key).

test_small_case_vs_fp64 runs one training step per small case with per-launch timing on and
judges it against the fp64 oracle by the project's methods and bars (the masked-fp64
step of tests/test_gpu_x3.py for models/model.py UNet; the fp32-oracle envelope of
test_mod_narrow_full_grads_vs_fp64 / test_res_full_grads_vs_oracle for the f32 mod.py networks;
the bf16-operand oracle and envelope of test_mod_bf16_matches_bf16_oracle for bf16, with
tests/res_bf16_ref.py as the residual network's bf16-operand oracle; for every
mod.py case also the branch-pinned fp64 check of tests/masked.py, whose bars are ~100x / ~10x
below those envelopes).  Only a
case that passed lends its launch keys to the coverage; agreement between two tiles counts for
nothing here.

test_production_kernels_are_covered then runs one step of each production configuration with
default options, takes the launch labels only, and fails for every GEMM key no passed small
case launched -- so a kernel or tile that becomes a default without an fp64-checked small case
fails the suite.  test_coverage_table_written records the table in
profiles/kernel_coverage.txt.  The three run in file order; the later ones fail (not skip) if
the small cases did not run.
"""
import gc
import os
import time

import pytest
import torch

import kernel_cases as KC
import masked as MK
import res_bf16_ref as RB
import test_gpu_x3 as TX
from _helpers import grad_errors, hip_mod_model, hip_model, inputs, norm_rel, options, rel_max
from oracle import mod_ref_cpu as MO
from oracle import unet_ref_cpu as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(REPO, "profiles", "kernel_coverage.txt")
LOGIT_TOL = 1e-4   # tests/test_gpu_mod.py, tests/test_gpu_res.py
GRAD_TOL = 1e-2

_RAN = set()           # small cases that ran
_COVERED = {}          # key -> ids of the small cases that launched it AND passed their check
_SMALL_FAMILIES = set()  # every family (GEMM or not) a passed small case launched
_PROD = {}             # configuration id -> {key: [labels]}
_PROD_FAMILIES = {}    # configuration id -> families


@pytest.fixture(autouse=True, scope="module")
def _threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def _to64(d):
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in d.items()}


def _load(m, P, B):
    sd = m.state_dict()
    for k, v in list(P.items()) + list(B.items()):
        sd[k] = v.clone()
    m.load_state_dict(sd)
    return m.to(DEV).train()


def _oracle_fns(c):
    """(make_params(seed), init_buffers(), train_step(P, B, x, t, bf16)) of a case's network."""
    b, d = c["base"], c["depth"]
    if c["net"] == "unet":
        return (O.make_params, O.init_buffers,
                lambda P, B, x, t, bf16=False: O.train_step(P, B, None, x, t))
    if c["net"] == "mod":
        return (lambda s: MO.make_params(s, b, d), lambda: MO.init_buffers(b, d),
                lambda P, B, x, t, bf16=False: MO.train_step(P, B, None, x, t, depth=d, bf16=bf16))
    assert c["net"] == "res" and c["math"] in ("fp32", "bf16"), (c["net"], c["math"])
    if c["math"] == "bf16":  # with bf16=False the helper is MO.res_train_step op for op
        return (lambda s: MO.res_make_params(s, b, d), lambda: MO.res_init_buffers(b, d),
                lambda P, B, x, t, bf16=False: RB.res_train_step(P, B, None, x, t, depth=d, bf16=bf16))
    return (lambda s: MO.res_make_params(s, b, d), lambda: MO.res_init_buffers(b, d),
            lambda P, B, x, t, bf16=False: MO.res_train_step(P, B, None, x, t, depth=d))


def _model(c, P=None, B=None):
    """The HIP network of a case / configuration; with P (and B) the oracle's parameters."""
    import unet_hip
    b, d = c["base"], c["depth"]
    if c["net"] == "unet":
        if P is not None:
            return hip_model(P, DEV, B)
        return unet_hip.UNet(1, 1).to(DEV).train()
    if c["net"] == "mod":
        if P is not None and c["math"] == "fp32":
            return hip_mod_model(P, DEV, b, d, B)
        m = unet_hip.ModUNet(1, 1, base_filters=b, depth=d, mfma_dtype=c["math"])
    else:
        m = unet_hip.ResUNet(1, 1, base_filters=b, depth=d, mfma_dtype=c["math"])
    return _load(m, P or {}, B or {})


def _timed_step(m, x, t):
    """One training step (forward, BCE + Dice, backward) with per-launch timing on: logits,
    loss, gradients (CPU, fp64) and the launch labels."""
    import unet_hip
    rt = m.flatten_().rt
    rt.timing(True)
    try:
        logits = m(x.to(DEV))
        losses = unet_hip.seg_losses(logits, t.to(DEV))
        loss = losses[0] + losses[1]
        loss.backward()
        torch.cuda.synchronize()
        labels = [lab for lab, _, _ in rt.timing_records()]
    finally:
        rt.timing(False)
    return logits.detach().cpu(), float(loss.item()), labels


def _check_unet(c, m, P, x, t, step):
    """tests/test_gpu_x3.py: gradients against the fp64 step on this path's own ReLU / max-pool
    branches at W_BAR / B_BAR / ALL_BAR, logits 1e-5 norm-relative against the fp64 step."""
    masks = TX._relu_masks(m, x)
    logits, _, labels = step()
    ref = O.train_step(_to64(P), _to64(O.init_buffers()), None, x.double(), t.double())
    e_l = norm_rel(logits.double(), ref["logits"])
    print(f"{c['id']}: logits vs fp64 {e_l:.2e}")
    grads = {k: p.grad.detach().cpu().double() for k, p in m.named_parameters()}
    TX._check_masked(grads, TX._masked_fp64_step(P, x, t, masks), c["id"])
    assert e_l <= 1e-5, (c["id"], e_l)
    return labels


def _check_f32(c, m, P, x, t, step):
    """test_mod_narrow_full_grads_vs_fp64 / test_res_full_grads_vs_oracle: logits within 1e-4
    of max|ref| of the fp32 oracle; every gradient against the fp64 oracle within 2x the fp32
    oracle's own worst deviation over x and x (1 + 1e-7), floor 1e-2.  Then the pinned check of
    tests/masked.py: the same step against the fp64 oracle on this path's own ReLU / max-pool
    branches, at 4x the pinned fp32 CPU oracle's own error (12x under x3 = 0)."""
    _, bufs, ts = _oracle_fns(c)
    br = MK.device_branches(m, x, c)
    ref = ts(P, bufs(), x, t)
    refp = ts(P, bufs(), x * (1 + 1e-7), t)
    r64 = ts(_to64(P), _to64(bufs()), x.double(), t.double())
    logits, _, labels = step()
    e_l = rel_max(logits.numpy(), ref["logits"].numpy())
    e32 = {k: max(norm_rel(g, r64["grads"][k]), norm_rel(refp["grads"][k], r64["grads"][k]))
           for k, g in ref["grads"].items()}
    env = max(2 * max(e32.values()), GRAD_TOL)
    errs = grad_errors(m, r64["grads"])
    worst = max(errs, key=errs.get)
    print(f"{c['id']}: logits {e_l:.2e}; worst grad {worst} {errs[worst]:.2e} (fp32 oracle "
          f"{e32[worst]:.2e}, envelope {env:.2e})")
    assert e_l <= LOGIT_TOL, (c["id"], e_l)
    assert errs[worst] <= env, f"{c['id']} {worst}: {errs[worst]:.3e} (fp32 oracle {e32[worst]:.3e})"
    MK.check_on_branches(c, P, x, t, br, logits.double(), MK.grads_of(m), c["id"],
                         c["opts"].get("x3", 1))
    return labels


def _check_bf16(c, m, P, x, t, step):
    """test_mod_bf16_matches_bf16_oracle: against the oracle that rounds the operands the HIP
    bf16 kernels round -- logits 2x the oracle's own fp32-vs-fp64 spread + 1e-4, loss 1e-3,
    every gradient 2x the largest spread; distance to the fp32 oracle 5e-2, or twice the bf16
    oracle's own where that exceeds it (tests/test_gpu_res_bf16.py _fp32_bar).  Then the pinned
    check of tests/masked.py: against the bf16-operand oracle in fp64 on this path's own
    branches, at 2x that oracle's pinned fp32-vs-fp64 spread (at most 5e-2)."""
    _, bufs, ts = _oracle_fns(c)
    br = MK.device_branches(m, x, c)
    ref = ts(P, bufs(), x, t, bf16=True)
    r64 = ts(_to64(P), _to64(bufs()), x.double(), t.double(), bf16=True)
    ref32 = ts(P, bufs(), x, t)
    spread_l = rel_max(ref["logits"].numpy(), r64["logits"].numpy())
    spread = {k: norm_rel(ref["grads"][k], r64["grads"][k]) for k in ref["grads"]}
    own32 = rel_max(ref["logits"].numpy(), ref32["logits"].numpy())
    bar32 = 5e-2 if own32 < 5e-2 else 2 * own32
    logits, loss, labels = step()
    e_l = rel_max(logits.numpy(), ref["logits"].numpy())
    e_l32 = rel_max(logits.numpy(), ref32["logits"].numpy())
    errs = grad_errors(m, ref["grads"])
    worst = max(errs, key=errs.get)
    env = 2 * max(spread.values())
    print(f"{c['id']}: logits vs bf16 oracle {e_l:.2e} (spread {spread_l:.2e}), vs fp32 oracle "
          f"{e_l32:.2e} (oracle's own {own32:.2e}); worst grad {worst} {errs[worst]:.2e} "
          f"(envelope {env:.2e}); loss {loss:.6f} vs {ref['loss'].item():.6f}")
    assert e_l <= 2 * spread_l + 1e-4, (c["id"], e_l, spread_l)
    assert abs(loss - ref["loss"].item()) <= 1e-3
    assert errs[worst] <= env, f"{c['id']} {worst}: {errs[worst]:.3e} (envelope {env:.3e})"
    assert e_l32 <= bar32, (c["id"], e_l32, bar32)
    MK.check_on_branches(c, P, x, t, br, logits.double(), MK.grads_of(m), c["id"])
    return labels


def _keys(labels, c):
    """{key: [labels]} over the GEMM families, and every family launched."""
    out, fams = {}, set()
    for lab in labels:
        fam = lab.partition("/")[0]
        fams.add(fam)
        if fam in KC.GEMM_FAMILIES:
            out.setdefault(KC.key(lab, c["depth"], c["shape"][2]), []).append(lab)
    return out, fams


@pytest.mark.parametrize("case", [c["id"] for c in KC.SMALL])
def test_small_case_vs_fp64(case):
    """One training step of a small case under the options that force its kernels, against
    the fp64 oracle (method and bars by network, see the module docstring)."""
    c = KC.by_id(KC.SMALL)[case]
    _RAN.add(case)
    t0 = time.perf_counter()
    mk, bufs, _ = _oracle_fns(c)
    P = mk(7)
    x, t = inputs(33, *c["shape"])
    m = _model(c, P, bufs())
    check = _check_unet if c["net"] == "unet" else _check_bf16 if c["math"] == "bf16" else _check_f32
    with options(m.flatten_().rt, **c["opts"]):
        labels = check(c, m, P, x, t, lambda: _timed_step(m, x, t))
    keys, fams = _keys(labels, c)
    assert keys, f"{case}: no GEMM launch was recorded"
    for k in keys:  # reached only if the fp64 check passed
        _COVERED.setdefault(k, []).append(case)
    _SMALL_FAMILIES.update(fams)
    print(f"{case}: {len(keys)} keys, {time.perf_counter() - t0:.1f} s")


def _require_small_cases():
    missing = [c["id"] for c in KC.SMALL if c["id"] not in _RAN]
    assert not missing, ("the small cases must run before this test (run the whole file); "
                         f"not run: {missing}")


@pytest.mark.parametrize("config", [c["id"] for c in KC.PRODUCTION])
def test_production_kernels_are_covered(config):
    """One default-option training step of a production configuration at its own batch and
    image size (bench.py's, main.py's for the bf16 residual network); labels only.  Every GEMM
    key it launches must have been launched by a small case that passed its fp64 check, and so
    must every elementwise family."""
    _require_small_cases()
    import unet_hip.runtime as RT
    c = KC.by_id(KC.PRODUCTION)[config]
    before = set(RT._RUNTIMES)
    torch.manual_seed(42)
    m = _model(c)
    N, H, W = c["shape"]
    g = torch.Generator(device="cpu").manual_seed(1000)
    x = torch.rand(N, 1, H, W, generator=g)
    t = (torch.rand(N, 1, H, W, generator=g) > 0.5).float()
    try:
        _, loss, labels = _timed_step(m, x, t)
    finally:
        # the model, its workspace, the context this configuration created, the allocator's cache
        m.zero_grad(set_to_none=True)
        del m
        for k in set(RT._RUNTIMES) - before:
            del RT._RUNTIMES[k]
        gc.collect()
        torch.cuda.empty_cache()
    keys, fams = _keys(labels, c)
    _PROD[config], _PROD_FAMILIES[config] = keys, fams
    assert keys, f"{config}: no GEMM launch was recorded"
    uncovered = {k: v for k, v in keys.items() if k not in _COVERED}
    for k, labs in sorted(uncovered.items()):
        print(f"{config}: UNCOVERED {k} launched by {sorted(set(labs))}")
    elementwise = sorted(f for f in fams if f not in KC.GEMM_FAMILIES and f not in _SMALL_FAMILIES)
    if elementwise:
        print(f"{config}: elementwise families no small case launches: {elementwise}")
    assert not uncovered, (f"{config}: no fp64-checked small case in tests/kernel_cases.py launches "
                           f"{sorted(uncovered)} (launched by "
                           f"{sorted({l for v in uncovered.values() for l in v})})")
    assert not elementwise, f"{config}: families no small case launches: {elementwise}"


def test_coverage_table_written():
    """profiles/kernel_coverage.txt: every production key, the configurations that launch it
    and the small cases that check it."""
    _require_small_cases()
    missing = [c["id"] for c in KC.PRODUCTION if c["id"] not in _PROD]
    assert not missing, f"production configurations that did not run: {missing}"
    rows = {}
    for cfg in (c["id"] for c in KC.PRODUCTION):
        for k in _PROD[cfg]:
            rows.setdefault(k, []).append(cfg)
    lines = ["# Written by tests/test_gpu_kernel_coverage.py::test_coverage_table_written.",
             "# GEMM launch keys (family, kernel_tile, row class: tests/kernel_cases.py key) of one",
             "# default-option training step of every production configuration, and the small",
             "# fp64-checked cases (tests/kernel_cases.py SMALL) that launch the same key.",
             f"# {'family':12s} {'kernel_tile':24s} {'rows':4s}  configurations <- small cases"]
    for k in sorted(rows):
        lines.append(f"{k[0]:14s} {k[1]:24s} {k[2]:4s}  {','.join(rows[k])} <- "
                     f"{','.join(_COVERED.get(k, [])) or 'NONE'}")
    with open(TABLE, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert all(k in _COVERED for k in rows)
