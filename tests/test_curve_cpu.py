"""CPU: the threshold sweep through the host twins unet_curve_hist_host / unet_curve_stats_host --
csrc/curve.h, the source the device kernels share -- against its NumPy restatement (curve_ref:
searchsorted bins, operating points counted directly on the raw arrays), bit for bit: everything is
float comparisons, integer sums and one correctly rounded float64 division per Dice value, added in
ascending plane order.  Then the pure-Python summary, the k = B/2 operating point against the 0.5
readout, the refusals, the host-only build of curve.h under the sanitizers, the flags, and
Trainer.test with the device ops replaced by the host twins."""
import ctypes
import logging
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import curve_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "thyroid-nodule-image-segmentation-unet-ddti_amd", "csrc")


def lib_edges(B):
    import unet_hip
    return unet_hip.curve_edges(B).numpy()


def as_torch(x, off):
    """The array as a tensor, taken `off` floats into a buffer when off > 0."""
    if not off:
        return torch.from_numpy(np.ascontiguousarray(x))
    buf = torch.zeros(x.size + off, dtype=torch.float32)
    buf[off:] = torch.from_numpy(x.reshape(-1))
    return buf[off:].view(x.shape)


def host_hist(x, t, e, off=0, total=None):
    import unet_hip
    ph, tot = unet_hip.curve_hist_host(as_torch(x, off), as_torch(t, off), torch.from_numpy(e), total)
    return ph, tot


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


# ---------------------------------------------------------------- edges
@pytest.mark.parametrize("B", [2 ** i for i in range(1, 11)])
def test_edges_are_monotone_antisymmetric_and_the_formula(B):
    e = lib_edges(B)
    assert e.dtype == np.float32 and e.shape == (B - 1,)
    assert (np.diff(e) > 0).all()
    assert np.array_equal(e, -e[::-1])
    assert e[B // 2 - 1] == 0.0 and not np.signbit(e[B // 2 - 1])
    want = R.edges(B)  # NumPy's log may differ from libm's in the last place of the double
    assert (np.abs(e - want) <= np.spacing(np.abs(want))).all()


def test_edges_refuse_bad_bin_counts():
    import unet_hip
    from unet_hip import _lib
    for B in (0, 1, 3, 12, 2048, -4):
        with pytest.raises(ValueError):
            unet_hip.curve_edges(B)
    buf = (ctypes.c_float * 4096)()
    lib = _lib.load()
    assert lib.unet_curve_edges(3, buf) == -1 and lib.unet_curve_edges(2048, buf) == -1
    assert lib.unet_curve_edges(256, None) == -1 and lib.unet_curve_edges(2, buf) == 0 and buf[0] == 0.0


# ---------------------------------------------------------------- host twins against the restatement
def _case_ids():
    return [(B, name) for B in R.BINS for name in sorted(R.small_cases(B, R.edges(B)))]


@pytest.mark.parametrize("B,name", _case_ids())
def test_host_twins_match_the_restatement(B, name):
    import unet_hip
    e = lib_edges(B)
    x, t, off = R.small_cases(B, e)[name]
    ph, tot = host_hist(x, t, e, off)
    want_h, want_tot = R.hist(x, t, e)
    assert np.array_equal(ph.numpy(), want_h)
    assert np.array_equal(tot.numpy(), want_tot)
    assert int(tot.sum()) == x.size
    got = unet_hip.curve_stats_host(ph)
    want_o, want_d = R.stats(x, t, e)
    for i, k in enumerate(R.FIELDS):
        assert np.array_equal(got[k].numpy(), want_o[:, i]), k
    assert np.array_equal(bits(got["dice_sum"].numpy()), bits(want_d))


def test_big_case_histogram_and_coarse_statistics():
    import unet_hip
    x, t = R.big_case()
    e = lib_edges(256)
    ph, tot = host_hist(x, t, e)
    want_h, want_tot = R.hist(x, t, e)
    assert np.array_equal(ph.numpy(), want_h) and np.array_equal(tot.numpy(), want_tot)
    assert want_h[:, 0, :2].sum() > 0.8 * x.size  # the skew: most pixels in the two lowest bins
    e = lib_edges(16)
    got = unet_hip.curve_stats_host(host_hist(x, t, e)[0])
    want_o, want_d = R.stats(x, t, e)
    for i, k in enumerate(R.FIELDS):
        assert np.array_equal(got[k].numpy(), want_o[:, i]), k
    assert np.array_equal(bits(got["dice_sum"].numpy()), bits(want_d))


def test_value_case_properties():
    """The bins of the special values are what curve.h says."""
    B = 16
    e = lib_edges(B)
    v = np.array([[np.nan, -np.inf, np.inf, 0.0, -0.0, 1e-45, e[3], np.nextafter(e[3], np.float32(9))]], np.float32)
    ph, _ = host_hist(v, np.zeros_like(v), e)
    h = ph.numpy()[0, 0]
    want = np.zeros(B, np.int32)
    for b in (0, 0, B - 1, B // 2 - 1, B // 2 - 1, B // 2, 3, 4):
        want[b] += 1
    assert np.array_equal(h, want)


def test_total_and_dice_sum_accumulate_over_two_calls():
    import unet_hip
    B = 16
    e = lib_edges(B)
    cs = R.small_cases(B, e)
    xa, ta, _ = cs["target_values_2x25x40"]
    xb, tb, _ = cs["aligned_3x64x64"]
    pa, tot = host_hist(xa, ta, e)
    assert tot[2 * B] > 0  # ignored pixels
    pb, tot2 = host_hist(xb, tb, e, total=tot)
    assert tot2 is tot
    assert np.array_equal(tot.numpy(), R.hist(xa, ta, e)[1] + R.hist(xb, tb, e)[1])
    assert np.array_equal(pb.numpy(), R.hist(xb, tb, e)[0])  # plane_hist is overwritten, not added to
    ds = unet_hip.curve_stats_host(pa)["dice_sum"]
    got = unet_hip.curve_stats_host(pb, ds)["dice_sum"]
    assert got is ds
    _, first = R.stats(xa, ta, e)
    _, both = R.stats(xb, tb, e, first)
    assert np.array_equal(bits(got.numpy()), bits(both))


def test_tie_break_nearest_to_the_middle_then_the_smaller():
    """One positive in bin B/2 - 1 and one in the last bin, two negatives in bin B/2: Dice is 2/3
    at every k <= B/2 - 1 and every k in B/2 + 1 .. B - 1, and 0.4 at B/2."""
    import unet_hip
    B = 16
    h = np.zeros((2, 2, B), np.int32)
    h[0, 1, B // 2 - 1] = h[0, 1, B - 1] = 1
    h[0, 0, B // 2] = 2
    h[1, 0, 3] = 5  # no positive at all: Dice 1 wherever nothing is predicted, k = 4 .. B
    got = unet_hip.curve_stats_host(torch.from_numpy(h))
    d0 = [2 / 3] * (B // 2) + [0.4] + [2 / 3] * (B // 2 - 1) + [0.0]
    d1 = [0.0] * 4 + [1.0] * (B - 3)
    assert got["best_k"].tolist() == [B // 2 - 1, B // 2] == [R.best(d0), R.best(d1)]
    assert got["TP"].tolist() == [2, 0] and got["FP"].tolist() == [2, 0] and got["FN"].tolist() == [0, 0]
    assert np.array_equal(bits(got["dice_sum"].numpy()), bits(np.array(d0) + np.array(d1)))
    assert got["auc2"].tolist() == [1 * 0 + 1 * 4, 0]


# ---------------------------------------------------------------- the summary
@pytest.mark.parametrize("B", [2, 16, 256])
def test_summary_matches_brute_force_counts(B):
    import unet_hip
    e = lib_edges(B)
    for name in ("aligned_3x64x64", "target_values_2x25x40", "one_class_planes_4x32x32", "one_bin_4x32x32"):
        x, t, _ = R.small_cases(B, e)[name]
        ph, tot = host_hist(x, t, e)
        ds = unet_hip.curve_stats_host(ph)["dice_sum"]
        got = unet_hip.curve_summary(tot.tolist(), ds.tolist(), x.shape[0], e)
        want = R.summary(x, t, e)
        assert got["dice_global"] == want["dice_global"] and got["dice_image"] == want["dice_image"]
        for k in ("auroc", "ap", "best_global_k", "best_image_k", "ignored"):
            assert got[k] == want[k] or (got[k] != got[k] and want[k] != want[k]), (name, k, got[k], want[k])
        assert got["best_global_threshold"] == want["best_global_k"] / B
        assert got["dice_global_half"] == want["dice_global"][B // 2]
        assert got["dice_image_half"] == want["dice_image"][B // 2]
        assert got["best_image_dice"] == max(want["dice_image"])


def test_middle_operating_point_is_the_half_readout():
    """k = B/2 counts what the 1 / (1 + exp(-x)) > 0.5 float32 readout counts, away from (0, ~2^-24]."""
    r = np.random.default_rng(3)
    x = (r.normal(0, 3, (2, 5000))).astype(np.float32)
    x[np.abs(x) < 1e-3] = 0.0
    x[0, :6] = (0.0, -0.0, 1e-3, -1e-3, np.inf, -np.inf)
    t = (r.random(x.shape) < 0.3).astype(np.float32)
    assert ((x == 0) | (np.abs(x) >= 1e-3)).all()  # before any code under test runs
    with np.errstate(over="ignore"):
        pr = np.float32(1) / (np.float32(1) + np.exp(-x, dtype=np.float32)) > np.float32(0.5)
    pos = t == 1
    want = [int((pr & pos).sum()), int((pr & ~pos).sum()), int((~pr & pos).sum()), int((~pr & ~pos).sum())]
    for B in (2, 256):
        e = lib_edges(B)
        _, tot = host_hist(x, t, e)
        neg_h, pos_h = tot.numpy()[:B], tot.numpy()[B:2 * B]
        got = [int(pos_h[B // 2:].sum()), int(neg_h[B // 2:].sum()), int(pos_h[:B // 2].sum()), int(neg_h[:B // 2].sum())]
        assert got == want and got == list(R.counts(x, t, e, B // 2))


# ---------------------------------------------------------------- refusals
def test_error_codes():
    import unet_hip
    from unet_hip import _lib
    from unet_hip.runtime import UNetRuntime
    lib = _lib.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    x = np.zeros(16, np.float32)
    e = lib_edges(16)
    ph, tot = np.zeros(2 * 2 * 16, np.int32), np.zeros(33, np.int64)
    oi, ds = np.zeros(2 * 8, np.int64), np.zeros(17, np.float64)
    H = lib.unet_curve_hist_host
    assert H(p(x), p(x), 2, 8, p(e), 16, p(ph), p(tot)) == 0
    for bad in ((None, p(x), 2, 8, p(e), 16, p(ph), p(tot)), (p(x), None, 2, 8, p(e), 16, p(ph), p(tot)),
                (p(x), p(x), 2, 8, None, 16, p(ph), p(tot)), (p(x), p(x), 2, 8, p(e), 16, None, p(tot)),
                (p(x), p(x), 2, 8, p(e), 16, p(ph), None), (p(x), p(x), 0, 8, p(e), 16, p(ph), p(tot)),
                (p(x), p(x), 2, 0, p(e), 16, p(ph), p(tot)), (p(x), p(x), 2, 8, p(e), 12, p(ph), p(tot)),
                (p(x), p(x), 2, 8, p(e), 1, p(ph), p(tot)), (p(x), p(x), 2, 8, p(e), 2048, p(ph), p(tot))):
        assert H(*bad) == -1, bad
    assert H(p(x), p(x), 1, 2 ** 31, p(e), 16, p(ph), p(tot)) == -2  # refused before anything is read
    S = lib.unet_curve_stats_host
    assert S(p(ph), 2, 16, p(oi), p(ds)) == 0
    for bad in ((None, 2, 16, p(oi), p(ds)), (p(ph), 2, 16, None, p(ds)), (p(ph), 2, 16, p(oi), None),
                (p(ph), 0, 16, p(oi), p(ds)), (p(ph), 2, 24, p(oi), p(ds))):
        assert S(*bad) == -1, bad
    # the device entries refuse before they touch the device
    rt = UNetRuntime("cuda:0")  # creating a context performs no device work
    d = ctypes.c_void_p(256)
    assert lib.unet_curve_hist(rt.ctx, d, d, 1, 2 ** 31, d, 16, d, d, None) == -2
    assert b"2^31" in lib.unet_last_error(rt.ctx)
    assert lib.unet_curve_hist(rt.ctx, d, d, 1, 8, d, 48, d, d, None) == -1
    assert lib.unet_curve_hist(rt.ctx, d, None, 1, 8, d, 16, d, d, None) == -1
    assert lib.unet_curve_stats(rt.ctx, d, 0, 16, d, d, None) == -1
    assert lib.unet_curve_stats(rt.ctx, d, 1, 16, None, d, None) == -1
    with pytest.raises(unet_hip.HipUnavailable):
        unet_hip.curve_hist(torch.zeros(1, 8), torch.zeros(1, 8), unet_hip.curve_edges(16))
    with pytest.raises(ValueError):
        unet_hip.curve_hist_host(torch.zeros(1, 8), torch.zeros(1, 9), unet_hip.curve_edges(16))
    with pytest.raises(ValueError):
        unet_hip.curve_stats_host(torch.zeros((1, 2, 12), dtype=torch.int32))


# ---------------------------------------------------------------- curve.h alone, under the sanitizers
def test_curve_header_builds_for_the_host_alone_and_runs_clean(tmp_path):
    """tools/curve_host_check.cpp includes curve.h with no HIP header, runs the two host twins on the
    shapes of the shared cases against a linear-count restatement, and is built with
    -fsanitize=address,undefined: a stand-alone program, run as its own process."""
    exe = str(tmp_path / "curve_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-DCURVE_HOST_ONLY", "-I", CSRC,
                           os.path.join(REPO, "tools", "curve_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env={"PATH": os.environ.get("PATH", "")})
    assert out.returncode == 0, out.stdout + out.stderr
    assert "curve_host_check ok" in out.stdout


# ---------------------------------------------------------------- flags
def test_flags_parse():
    import main
    a = main.get_parser([])
    assert a.curve_metrics is False and a.curve_bins == 256 and a.threshold == 0.5
    a = main.get_parser(["--curve_metrics", "--curve_bins", "64", "--threshold", "0.3"])
    assert a.curve_metrics is True and a.curve_bins == 64 and a.threshold == 0.3
    assert main.get_parser(["--threshold", "val-dice"]).threshold == "val-dice"
    assert main.get_parser(["--threshold", "val-image-dice"]).threshold == "val-image-dice"
    for bad in ("0", "1", "1.5", "val-iou"):
        with pytest.raises(SystemExit):
            main.get_parser(["--threshold", bad])


def test_threshold_snapping():
    from unet_hip.functional import parse_threshold
    assert parse_threshold(None) == (None, None) and parse_threshold(0.5) == (None, None)
    assert parse_threshold(0.3, 256) == (None, 77)  # 76.8 -> 77
    assert parse_threshold(0.3, 16) == (None, 5)
    assert parse_threshold(0.001, 256) == (None, 1) and parse_threshold(0.9999, 256) == (None, 255)
    assert parse_threshold(0.501, 256) == (None, 128)  # snaps to the middle: x > 0
    assert parse_threshold("val-dice") == ("val-dice", None)
    for bad in (0.0, 1.0, -0.2, "best", float("nan")):
        with pytest.raises(ValueError):
            parse_threshold(bad)


# ---------------------------------------------------------------- Trainer.test on the CPU
class _StubRuntime:
    """unet_mask_counts restated in torch for the CPU (away from logits in (0, 2^-24])."""

    def mask_counts(self, logits, targets, counts, mask=None):
        pr = logits > 0
        tu = targets.to(torch.int64)
        if mask is not None:
            mask.copy_(pr)
        counts += torch.stack([(pr & (tu == 1)).sum(), (pr & (tu == 0)).sum(), (~pr & (tu == 1)).sum(),
                               (~pr & (tu == 0)).sum(), (pr & (targets != 0)).sum(),
                               (pr | (targets != 0)).sum()])


class _StubModel:
    def eval(self):
        return self

    def __call__(self, images):
        return images  # the "image" is the logit plane


def _cpu_trainer(tmp_path, test_batches, val_batches, **cfg):
    from utils.trainer import Trainer
    tr = object.__new__(Trainer)
    tr.config = types.SimpleNamespace(result_dir=str(tmp_path), **cfg)
    tr.logger = logging.getLogger("curve_cpu")
    tr.rank0, tr.ddp, tr.device = True, None, torch.device("cpu")
    tr.model, tr.rt = _StubModel(), _StubRuntime()
    tr.test_loader, tr.val_loader = test_batches, val_batches
    tr._plot_contours = lambda keep: None
    return tr


def _loader(seed, bias):
    r = np.random.default_rng(seed)
    out = []
    for n in (3, 2):
        x, t = R._scene(r, n, 32, 48)
        x = x + np.float32(bias)
        x[np.abs(x) < 1e-3] = 0.0
        out.append((torch.from_numpy(x.reshape(n, 1, 32, 48)), torch.from_numpy(t.reshape(n, 1, 32, 48))))
    return out


def _flat(batches):
    return (np.concatenate([b[0].numpy().reshape(b[0].shape[0], -1) for b in batches]),
            np.concatenate([b[1].numpy().reshape(b[1].shape[0], -1) for b in batches]))


BASE_KEYS = ["TP", "FP", "FN", "TN", "ACC", "Precision", "Recall", "F1", "IoU"]
CURVE_KEYS = ["Curve_AUROC", "Curve_AP", "Curve_BestDice", "Curve_BestDiceThreshold", "Curve_Dice",
              "Curve_BestImageDice", "Curve_BestImageDiceThreshold", "Curve_ImageDice", "Curve_Ignored", "Curve_Bins"]
OPT_KEYS = ["OPT_" + k for k in BASE_KEYS] + ["OPT_Threshold"]


@pytest.fixture
def host_ops(monkeypatch):
    import unet_hip
    monkeypatch.setattr(unet_hip, "curve_hist", unet_hip.curve_hist_host)
    monkeypatch.setattr(unet_hip, "curve_stats", unet_hip.curve_stats_host)


def test_trainer_with_the_switches_off_runs_no_curve_code(tmp_path, monkeypatch, capsys):
    import unet_hip

    def boom(*a, **k):
        raise AssertionError("curve code called with the switches off")

    for f in ("curve_hist", "curve_stats", "curve_edges", "curve_summary"):
        monkeypatch.setattr(unet_hip, f, boom)
    test, val = _loader(1, 0.0), _loader(2, 0.0)
    want = None
    for cfg in ({}, {"curve_metrics": False, "curve_bins": 256, "threshold": 0.5}, {"threshold": None}):
        m = _cpu_trainer(tmp_path, test, val, **cfg).test()
        assert list(m) == BASE_KEYS
        want = want or m
        assert m == want
    out = capsys.readouterr().out
    assert "Curve" not in out and "Operating point" not in out


def test_trainer_curve_metrics_block(tmp_path, host_ops, capsys):
    test, val = _loader(1, -2.0), _loader(2, -2.0)  # a bias: the best threshold is not 0.5
    base = _cpu_trainer(tmp_path, test, val).test()
    m = _cpu_trainer(tmp_path, test, val, curve_metrics=True, curve_bins=64).test()
    assert list(m) == BASE_KEYS + CURVE_KEYS
    assert {k: m[k] for k in BASE_KEYS} == base
    x, t = _flat(test)
    e = lib_edges(64)
    want = R.summary(x, t, e)
    assert m["Curve_AUROC"] == want["auroc"] and m["Curve_AP"] == want["ap"] and m["Curve_Bins"] == 64
    assert m["Curve_BestDice"] == max(want["dice_global"]) and m["Curve_BestDiceThreshold"] == want["best_global_k"] / 64
    assert m["Curve_BestImageDice"] == max(want["dice_image"])
    assert m["Curve_BestImageDiceThreshold"] == want["best_image_k"] / 64
    assert m["Curve_Dice"] == want["dice_global"][32] and m["Curve_ImageDice"] == want["dice_image"][32]
    assert m["Curve_Ignored"] == 0 and m["Curve_BestDiceThreshold"] != 0.5
    out = capsys.readouterr().out
    assert "Curve Metrics (64 bins) — AUROC=" in out and "over 5 images" in out


def test_trainer_float_threshold_is_snapped_and_reported(tmp_path, host_ops, capsys):
    test, val = _loader(1, -2.0), _loader(2, -2.0)
    base = _cpu_trainer(tmp_path, test, val).test()
    m = _cpu_trainer(tmp_path, test, val, threshold=0.3, curve_bins=16).test()
    assert list(m) == BASE_KEYS + OPT_KEYS
    assert {k: m[k] for k in BASE_KEYS} == base
    assert m["OPT_Threshold"] == 5 / 16
    x, t = _flat(test)
    assert (m["OPT_TP"], m["OPT_FP"], m["OPT_FN"], m["OPT_TN"]) == R.counts(x, t, lib_edges(16), 5)
    assert "threshold 0.312500 (k=5 of 16, snapped from 0.3)" in capsys.readouterr().out


@pytest.mark.parametrize("criterion,key", [("val-dice", "best_global_k"), ("val-image-dice", "best_image_k")])
def test_trainer_threshold_from_the_validation_split(tmp_path, host_ops, criterion, key):
    test, val = _loader(1, -2.0), _loader(2, -2.0)
    m = _cpu_trainer(tmp_path, test, val, threshold=criterion, curve_metrics=True).test()
    assert list(m) == BASE_KEYS + CURVE_KEYS + OPT_KEYS
    e = lib_edges(256)
    k = R.summary(*_flat(val), e)[key]
    assert m["OPT_Threshold"] == k / 256 and k != 128
    x, t = _flat(test)
    assert (m["OPT_TP"], m["OPT_FP"], m["OPT_FN"], m["OPT_TN"]) == R.counts(x, t, e, k)


def test_trainer_refuses_a_threshold_with_tta(tmp_path, host_ops):
    test, val = _loader(1, 0.0), _loader(2, 0.0)
    for thr in (0.3, "val-dice"):
        with pytest.raises(ValueError, match="tta"):
            _cpu_trainer(tmp_path, test, val, threshold=thr, tta="hflip").test()
    with pytest.raises(ValueError, match="threshold"):
        _cpu_trainer(tmp_path, test, val, threshold=1.5).test()
