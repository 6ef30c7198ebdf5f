"""Every GEMM kernel and tile an eval-mode forward of production launches -- Trainer.validate /
Trainer.test, main.py --mode test, unet_hip.tta_predict -- is tied to a small eval case that is
checked layer by layer against the fp64 oracle (tests/kernel_cases.py: INFERENCE, SMALL_EVAL;
tests/eval_ref.py: trained-like running buffers, the traced eval oracle).  The eval forward has
its own routes (no kept images: every operand image is written by prep16 / prep_x3 into one
scratch image), its own plan and bn_finalize_eval_kernel; coverage lent by the training small
cases of tests/test_gpu_kernel_coverage.py does not count here.

test_small_eval_case_vs_fp64: one eval forward per small case under the options that force its
kernels, on a workspace of exactly workspace_bytes(..., False); every conv's stored rows (debug
view 0), every residual block's output (view 9) and the logits against the fp64 trace.
  f32: rel_max and norm_rel per layer within FACTOR x the fp32 CPU oracle's own deviation from
       fp64 at that layer (worst over x, x (1 +- 1e-7); 4x, 12x for a case that sets x3 = 0 or
       a level named in KC.NARROW_12X: the factors of tests/masked.py), capped at LOGIT_TOL =
       1e-4 (rel_max), the models/model.py logits at 1e-5 norm-relative.
  bf16: against the bf16-operand oracle in fp32; per layer 2x that oracle's own fp32-vs-fp64
       rel_max spread + 1e-4 (the eval bar of test_res_bf16_eval_and_bn_buffers); the logits'
       distance to the plain fp32 oracle at 5e-2, or twice the bf16 oracle's own where that
       exceeds it (_fp32_bar's rule).
  views 1 / 2: eval scale / shift per channel against float64 at eval_ref.affine_bounds.
  The buffers are bit-equal after the call; a second forward on a NaN-filled workspace gives
  bit-equal logits.
Only a case that passed lends its keys.  test_eval_bn_finalize_edges plants extreme channels in
the running buffers; test_eval_samples_are_independent holds sample n alone to sample n in the
batch bit for bit; test_inference_kernels_are_covered runs every INFERENCE entry with default
options, labels only; test_eval_coverage_table_written records profiles/eval_coverage.txt.  They
run in file order; the later ones fail (not skip) if the small cases did not run.
"""
import gc
import os
import time

import numpy as np
import pytest
import torch

import eval_ref as ER
import kernel_cases as KC
from _helpers import inputs, norm_rel, options, rel_max
from test_gpu_kernel_coverage import DEV, LOGIT_TOL, REPO, _keys, _model

pytestmark = pytest.mark.gpu

TABLE = os.path.join(REPO, "profiles", "eval_coverage.txt")
STATS = os.path.join(REPO, "profiles", "eval_stats.txt")
EPS = (0.0, 1e-7, -1e-7)       # tests/masked.py
FACTOR_X3, FACTOR_F32_MFMA = 4.0, 12.0

_RAN = set()
_COVERED = {}
_SMALL_FAMILIES = set()
_INF = {}
_T0 = [None]


@pytest.fixture(autouse=True, scope="module")
def _threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    _T0[0] = time.perf_counter()


def _eval_forward(m, x, opts, timed=True, fill=None):
    """One rt.forward(..., training=False) of m on x under `opts` on a fresh workspace of exactly
    workspace_bytes(N, H, W, False) (filled with NaN if `fill`): logits, workspace, labels."""
    st = m.flatten_()
    rt = st.rt
    N, _, H, W = x.shape
    with options(rt, **opts), torch.no_grad():
        ws = torch.empty(rt.workspace_bytes(N, H, W, False), dtype=torch.uint8, device=DEV)
        if fill:
            ws[:ws.numel() // 4 * 4].view(torch.float32).fill_(float("nan"))
        st.sync_params()
        rt.timing(timed)
        try:
            logits, ws2 = rt.forward(st.param_arena, st.bn_arena, st.nbt_arena, x.to(DEV), training=False,
                                     workspace=ws)
            torch.cuda.synchronize()
            labels = [lab for lab, _, _ in rt.timing_records()] if timed else []
        finally:
            rt.timing(False)
    assert ws2.data_ptr() == ws.data_ptr() and ws2.numel() == ws.numel()
    return logits, ws, labels


def _device_layers(m, c, ws, logits):
    """[(tag, rows)] as eval_ref.layers gives them: view 0 of every conv sliced to the real
    channels, view 9 of every residual block, the logits."""
    rt = m.flatten_().rt
    N, H, W = c["shape"]
    D = c["depth"]
    out = []
    for i in range(2 * (2 * D + 1)):
        C = c["base"] << ER.level_of_conv(c, i)
        z, off = rt.debug_view(ws, N, H, W, False, 0, i)
        out.append((f"conv{i}", z[:, off:off + C].double().cpu().numpy()))
    for b in range(2 * D + 1 if c["net"] == "res" else 0):
        C = c["base"] << (b if b <= D else 2 * D - b)
        v, off = rt.debug_view(ws, N, H, W, False, 9, b)
        out.append((f"out{b}", v[:, off:off + C].double().cpu().numpy()))
    out.append(("logits", ER.rows(logits.cpu())))
    return out


def _check_affine(m, c, ws, P, B, tag):
    """Views 1 / 2 of every BN layer against float64 from P and the buffers."""
    rt = m.flatten_().rt
    N, H, W = c["shape"]
    worst = (0.0, 0.0)
    for i, name in enumerate(ER.bn_names(c)):
        C = c["base"] << ER.level_of_conv(c, i)
        sc = rt.debug_view(ws, N, H, W, False, 1, i)[:C].cpu().numpy()
        sh = rt.debug_view(ws, N, H, W, False, 2, i)[:C].cpu().numpy()
        r = ER.check_affine(sc, sh, P[f"{name}.weight"].numpy(), P[f"{name}.bias"].numpy(),
                            B[f"{name}.running_mean"].numpy(), B[f"{name}.running_var"].numpy(), f"{tag} {name}")
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    print(f"{tag}: eval scale {worst[0]:.2f} x its bound, shift {worst[1]:.2f} x")
    return sc, sh


def _level(c, tag):
    if tag == "logits":
        return 0
    if tag.startswith("conv"):
        return ER.level_of_conv(c, int(tag[4:]))
    b = int(tag[3:])
    return b if b <= c["depth"] else 2 * c["depth"] - b


def _bars(c, P, B, x):
    """{tag: {measure: bar}}, the reference rows per tag, and the logits bar against the plain
    fp32 oracle (bf16) -- from the oracles alone (module docstring)."""
    bf16 = c["math"] == "bf16"
    tr64 = ER.eval_trace(c, P, B, x, torch.float64, bf16)
    l64 = ER.layers(tr64)
    assert ER.meaningful(tr64) == [] or c.get("planted"), ER.meaningful(tr64)
    bars = {}
    if bf16:
        tr32 = ER.eval_trace(c, P, B, x, torch.float32, True)
        l32 = ER.layers(tr32)
        for (tag, a), (_, r) in zip(l32, l64):
            bars[tag] = {"rel_max": 2 * rel_max(a, r) + 1e-4}
        plain = ER.rows(ER.eval_trace(c, P, B, x, torch.float32, False)["logits"])
        own = rel_max(l32[-1][1], plain)
        return bars, dict(l32), (plain, 5e-2 if own < 5e-2 else 2 * own)
    dev = dict.fromkeys((t for t, _ in l64), (0.0, 0.0))
    for eps in EPS:
        tr = ER.eval_trace(c, P, B, x * (1 + eps) if eps else x, torch.float32)
        for (tag, a), (_, r) in zip(ER.layers(tr), l64):
            dev[tag] = (max(dev[tag][0], rel_max(a, r)), max(dev[tag][1], norm_rel(a, r)))
    for tag, (em, en) in dev.items():
        narrow = (c["id"], _level(c, tag)) in KC.NARROW_12X
        f = FACTOR_F32_MFMA if c["opts"].get("x3", 1) == 0 or narrow else FACTOR_X3
        bars[tag] = {"rel_max": _cap(c, f * em, em, LOGIT_TOL), "norm_rel": f * en}
    if c["net"] == "unet":
        bars["logits"]["norm_rel"] = _cap(c, bars["logits"]["norm_rel"], dev["logits"][1], 1e-5)
    return bars, dict(l64), None


def _cap(c, bar, own, cap):
    """min(bar, cap) -- always for a small case.  A planted network (test_eval_bn_finalize_edges)
    keeps a cap only where the fp32 CPU oracle's own deviation `own` is inside it: |mean| = 1e4
    against activations of unit spread costs every float32 evaluation four digits of the stored
    rows, torch's own included, so a cap below the reference's own float32 error is no statement
    about a kernel; the factor rule alone holds there."""
    return bar if c.get("planted") and own > cap else min(bar, cap)


def _compare(c, got, bars, ref, plain, tag):
    """Print every per-layer error next to its bar, then assert them all."""
    fails, worst = [], (0.0, "")
    for t, a in got:
        assert np.isfinite(a).all(), f"{tag} {t}: non-finite"
        err = {"rel_max": rel_max(a, ref[t]), "norm_rel": norm_rel(a, ref[t])}
        line = "  ".join(f"{k} {err[k]:.2e} / {b:.2e}" for k, b in bars[t].items())
        print(f"{tag} {t:8s} {line}")
        for k, b in bars[t].items():
            worst = max(worst, (err[k] / b, f"{t} {k} {err[k]:.2e} / {b:.2e}"))
            if err[k] > b:
                fails.append(f"{t} {k} {err[k]:.3e} > {b:.3e}")
    if plain is not None:
        e = rel_max(got[-1][1], plain[0])
        print(f"{tag} logits vs the plain fp32 oracle {e:.2e} / {plain[1]:.2e}")
        if e > plain[1]:
            fails.append(f"logits vs fp32 oracle {e:.3e} > {plain[1]:.3e}")
    print(f"{tag}: worst {worst[0]:.2f} x its bar ({worst[1]})")
    assert not fails, f"{tag}: {fails}"


def _setup(c, P, B):
    m = _model(c, P, B).eval()
    st = m.flatten_()
    return m, st, st.bn_arena.clone(), st.nbt_arena.clone()


@pytest.mark.parametrize("case", [c["id"] for c in KC.SMALL_EVAL])
def test_small_eval_case_vs_fp64(case):
    c = KC.by_id(KC.SMALL_EVAL)[case]
    _RAN.add(case)
    t0 = time.perf_counter()
    P = ER.fns(c)[0](c["pseed"])
    x, _ = inputs(c["xseed"], *c["shape"])
    B = ER.trained_buffers(c, P, x)
    m, st, bn0, nbt0 = _setup(c, P, B)
    logits, ws, labels = _eval_forward(m, x, c["opts"])
    got = _device_layers(m, c, ws, logits)
    bars, ref, plain = _bars(c, P, B, x)
    _compare(c, got, bars, ref, plain, case)
    _check_affine(m, c, ws, P, B, case)
    assert torch.equal(st.bn_arena, bn0) and torch.equal(st.nbt_arena, nbt0), "eval wrote the buffers"
    again, _, _ = _eval_forward(m, x, c["opts"], timed=False, fill=True)
    assert torch.equal(again, logits), "second forward on a NaN-filled workspace differs"
    keys, fams = _keys(labels, c)
    assert keys, f"{case}: no GEMM launch was recorded"
    back = sorted(f for f in fams if f in KC.BACKWARD_FAMILIES)
    assert not back, f"{case}: backward families in an eval forward: {back}"
    for k in keys:  # reached only if every check passed
        _COVERED.setdefault(k, []).append(case)
    _SMALL_FAMILIES.update(fams)
    print(f"{case}: {len(keys)} keys, {time.perf_counter() - t0:.1f} s")


def test_eval_bn_finalize_edges():
    """One network per variant at (1, 32, 64) with planted channels in every BN layer's
    parameters and running buffers (eval_ref.PLANTED): views 1 / 2 against float64 at
    eval_ref.affine_bounds, every stored value finite, every layer and the logits inside the
    case's bars (the 1e-4 / 1e-5 caps where the fp32 CPU oracle itself is inside them: `_cap`;
    measured on models/model.py's logits, norm-relative: device 1.09e-5, torch fp32 1.54e-5, 4x
    bar 6.2e-5).  profiles/eval_stats.txt: per planted kind, the error of BN's output on that
    channel relative to max|BN64| -- torch's float32 CPU batch_norm(training=False), the device's
    stored affine applied in float64, and the derived bound -- worst over the BN layers."""
    rows = {k: [0.0, 0.0, 0.0] for k in ER.PLANTED}
    failed = []
    for c in ER.EDGE_CASES:
        c = dict(c, planted=True)
        P = ER.plant_params(c, ER.fns(c)[0](7))
        x, _ = inputs(33, *c["shape"])
        B = ER.planted_buffers(c, P, x)
        m, st, bn0, nbt0 = _setup(c, P, B)
        logits, ws, _ = _eval_forward(m, x, {}, timed=False)
        got = _device_layers(m, c, ws, logits)
        bars, ref, plain = _bars(c, P, B, x)
        tag = f"edges {c['id']}"
        try:
            _compare(c, got, bars, ref, plain, tag)
        except AssertionError as e:  # every network's figures are printed before the test fails
            failed.append(str(e))
        _check_affine(m, c, ws, P, B, tag)
        assert torch.equal(st.bn_arena, bn0) and torch.equal(st.nbt_arena, nbt0)
        bf16 = c["math"] == "bf16"
        tr32 = ER.eval_trace(c, P, B, x, torch.float32, bf16)
        tch = ER.torch_bn_rows(None, tr32, P, B, c)
        rt = st.rt
        N, H, W = c["shape"]
        for i, name in enumerate(ER.bn_names(c)):
            sc = rt.debug_view(ws, N, H, W, False, 1, i).cpu().numpy().astype(np.float64)
            sh = rt.debug_view(ws, N, H, W, False, 2, i).cpu().numpy().astype(np.float64)
            g, b = P[f"{name}.weight"].numpy(), P[f"{name}.bias"].numpy()
            rm, rv = B[f"{name}.running_mean"].numpy(), B[f"{name}.running_var"].numpy()
            bs, bh = ER.affine_bounds(g, b, rm, rv)
            for kind, ch in ER.PLANTED.items():
                z = tr32["conv"][i][:, ch].double().numpy()
                y64 = ER.bn64(z, P, B, name, ch)
                den = max(np.abs(y64).max(), 1e-30)
                rows[kind][1] = max(rows[kind][1], float(np.abs(z * sc[ch] + sh[ch] - y64).max() / den))
                rows[kind][2] = max(rows[kind][2], float((np.abs(z).max() * bs[ch] + bh[ch]) / den))
        for kind in ER.PLANTED:
            rows[kind][0] = max(rows[kind][0], tch[kind])
    lines = ["# Written by tests/test_gpu_eval_coverage.py::test_eval_bn_finalize_edges.",
             "# Eval BatchNorm on the planted channels of every BN layer (tests/eval_ref.py PLANTED,",
             "# EDGE_CASES at (1, 32, 64)): max|y - y64| / max|y64| of the layer's output on that channel,",
             "# worst over the layers and networks.  torch fp32: torch's CPU batch_norm(training=False);",
             "# device: the affine bn_finalize_eval_kernel stored (views 1, 2) applied in float64; bound:",
             "# eval_ref.affine_bounds (4 u |scale|, 6 u |mean scale| + u |shift|) on the same input.",
             f"# {'kind':12s} {'torch fp32':>12s} {'device':>12s} {'bound':>12s}"]
    for kind, (t, d, b) in rows.items():
        lines.append(f"{kind:14s} {t:12.3e} {d:12.3e} {b:12.3e}")
        assert d <= b, (kind, d, b)
    with open(STATS, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    assert not failed, failed


N3 = [c["id"] for c in KC.SMALL_EVAL if c["shape"][0] == 3]


@pytest.mark.parametrize("case", N3)
def test_eval_samples_are_independent(case):
    """Sample n run alone gives the logits it gives inside the batch of three, bit for bit, under
    the case's forced tile: in eval nothing couples samples, and every GEMM sums one output
    pixel's K in an order that does not depend on where the pixel's tile starts."""
    assert case in _RAN, "the small cases must run before this test (run the whole file)"
    c = KC.by_id(KC.SMALL_EVAL)[case]
    P = ER.fns(c)[0](c["pseed"])
    x, _ = inputs(c["xseed"], *c["shape"])
    m, _, _, _ = _setup(c, P, ER.trained_buffers(c, P, x))
    batch, _, _ = _eval_forward(m, x, c["opts"], timed=False)
    for n in range(3):
        alone, _, _ = _eval_forward(m, x[n:n + 1], c["opts"], timed=False)
        d = (alone[0] - batch[n]).abs().max().item()
        print(f"{case}: sample {n} alone vs in the batch: max|d| {d:.2e}")
        assert torch.equal(alone[0], batch[n]), f"{case}: sample {n} differs by {d:.3e}"


def _require_small_cases():
    missing = [c["id"] for c in KC.SMALL_EVAL if c["id"] not in _RAN]
    assert not missing, f"the small eval cases must run before this test (run the whole file); not run: {missing}"


@pytest.mark.parametrize("config", [c["id"] for c in KC.INFERENCE])
def test_inference_kernels_are_covered(config):
    """One default-option eval forward of an INFERENCE entry at its own shape, labels only: every
    GEMM key and every other family must have been launched by an eval small case that passed,
    and no backward family may appear."""
    _require_small_cases()
    import unet_hip.runtime as RT
    c = KC.by_id(KC.INFERENCE)[config]
    before = set(RT._RUNTIMES)
    torch.manual_seed(42)
    m = _model(c).eval()
    N, H, W = c["shape"]
    x = torch.rand(N, 1, H, W, generator=torch.Generator(device="cpu").manual_seed(1000))
    try:
        logits, ws, labels = _eval_forward(m, x, {})
        finite = bool(torch.isfinite(logits).all())
    finally:
        del m
        logits = ws = None
        for k in set(RT._RUNTIMES) - before:
            del RT._RUNTIMES[k]
        gc.collect()
        torch.cuda.empty_cache()
    keys, fams = _keys(labels, c)
    _INF[config] = keys
    assert keys and finite
    back = sorted(f for f in fams if f in KC.BACKWARD_FAMILIES)
    assert not back, f"{config}: backward families in an eval forward: {back}"
    uncovered = {k: v for k, v in keys.items() if k not in _COVERED}
    for k, labs in sorted(uncovered.items()):
        print(f"{config}: UNCOVERED {k} launched by {sorted(set(labs))}")
    other = sorted(f for f in fams if f not in KC.GEMM_FAMILIES and f not in _SMALL_FAMILIES)
    assert not uncovered, (f"{config}: no fp64-checked eval case in tests/kernel_cases.py SMALL_EVAL launches "
                           f"{sorted(uncovered)}")
    assert not other, f"{config}: families no eval small case launches: {other}"


def test_eval_coverage_table_written():
    """profiles/eval_coverage.txt: every inference key, the entries that launch it and the eval
    small cases that check it."""
    _require_small_cases()
    missing = [c["id"] for c in KC.INFERENCE if c["id"] not in _INF]
    assert not missing, f"inference entries that did not run: {missing}"
    rows = {}
    for cfg in (c["id"] for c in KC.INFERENCE):
        for k in _INF[cfg]:
            rows.setdefault(k, []).append(cfg)
    lines = ["# Written by tests/test_gpu_eval_coverage.py::test_eval_coverage_table_written.",
             "# GEMM launch keys (family, kernel_tile, row class: tests/kernel_cases.py key) of one",
             "# default-option eval forward of every inference entry (tests/kernel_cases.py INFERENCE),",
             "# and the small fp64-checked eval cases (SMALL_EVAL) that launch the same key.",
             f"# {'family':12s} {'kernel_tile':24s} {'rows':4s}  entries <- small eval cases"]
    for k in sorted(rows):
        lines.append(f"{k[0]:14s} {k[1]:24s} {k[2]:4s}  {','.join(rows[k])} <- "
                     f"{','.join(_COVERED.get(k, [])) or 'NONE'}")
    with open(TABLE, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"tests/test_gpu_eval_coverage.py: {time.perf_counter() - _T0[0]:.0f} s since the first test")
    assert all(k in _COVERED for k in rows)
