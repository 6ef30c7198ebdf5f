"""CPU: the surface-distance metrics (HD, HD95, ASSD) through the host hook
unet_surface_stats_host -- csrc/surf.h, the source the device kernels share -- against the
definition (surface_ref.oracle: scipy's erosion and distance transform, numpy's percentile), and
the CPU behaviour of the public surface: refusals, the --surface_metrics flag, and Trainer.test
with the metrics off and on.

Bounds.  The integer fields and hd (a correctly rounded sqrt of an integer) are exact.  hd95 and
assd are float64 sums of at most 2 H W non-negative terms (n eps < 6e-11 at 512^2) and an
interpolation of a few ulps: 1e-9 relative."""
import ctypes
import logging
import math
import types

import numpy as np
import pytest
import torch

import surface_ref as R

REL = 1e-9


def host(x, t):
    import unet_hip
    return {k: v.numpy() for k, v in unet_hip.surface_metrics_host(torch.from_numpy(x), torch.from_numpy(t)).items()}


def check_against_oracle(got, P, G):
    for n in range(P.shape[0]):
        want = R.oracle(P[n], G[n])
        for k in R.INT_FIELDS:
            assert int(got[k][n]) == want[k], (n, k, int(got[k][n]), want[k])
        if not want["defined"]:
            assert all(math.isnan(got[k][n]) for k in ("hd", "hd95", "assd"))
            assert got["sum_pg"][n] == 0 and got["sum_gp"][n] == 0
            continue
        assert got["hd"][n] == want["hd"], (n, got["hd"][n], want["hd"])
        for k in ("hd95", "assd", "sum_pg", "sum_gp"):
            assert abs(got[k][n] - want[k]) <= REL * abs(want[k]), (n, k, got[k][n], want[k])


CASES = R.mask_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_hook_matches_definition(name):
    P, G = CASES[name]
    got = host(*R.to_inputs(P, G))
    assert got["defined"].all()
    check_against_oracle(got, P, G)


def test_case_properties():
    """The cases are what their names say."""
    o = R.oracle(*(m[0] for m in CASES["identical_8x8"]))
    assert o["max_d2"] == 0 and o["hd95"] == 0 and o["assd"] == 0 and o["n_pg"] == o["n_gp"] == 12
    o = R.oracle(*(m[0] for m in CASES["single_pixels_8x8_n2"]))
    assert o["n_pg"] == o["n_gp"] == 1 and o["max_d2"] == 25 + 9 == o["d2_lo"] == o["d2_hi"]
    o = R.oracle(*(m[0] for m in CASES["lines_33x65_n21"]))
    assert o["n_pg"] + o["n_gp"] == 21 and 0.95 * 20 == 19.0
    o = R.oracle(*(m[0] for m in CASES["lines_33x65_n20"]))
    assert o["n_pg"] + o["n_gp"] == 20 and o["d2_lo"] != o["d2_hi"]
    o = R.oracle(*(m[0] for m in CASES["full_image_vs_edge_blobs_40x72"]))
    assert o["n_pg"] == 2 * (40 + 72) - 4  # the border of a full image is its frame


def test_channels_above_zero_are_ignored():
    P, G = CASES["batch3_40x72"]
    a = host(*R.to_inputs(P, G, C=1))
    b = host(*R.to_inputs(P, G, C=2, seed=5))
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    check_against_oracle(b, P, G)


def test_logits_at_the_threshold():
    """sigmoid(x) > 0.5 in float32, as unet_mask_counts forms it (surf_pred is its source): 0 and
    the smallest positive float32 both give exp(-x) == 1, sigmoid == 0.5, background."""
    tiny = np.float32(np.nextafter(np.float32(0), np.float32(1)))
    x = np.full((1, 1, 8, 8), tiny, np.float32)
    x[0, 0, :, 4:] = 0.0
    x[0, 0, 2:5, 2:6] = 1.0
    t = np.zeros((1, 1, 8, 8), np.float32)
    t[0, 0, 3:7, 1:4] = 1.0
    got = host(x, t)
    check_against_oracle(got, x[:, 0] == 1.0, t[:, 0] == 1.0)
    assert (torch.sigmoid(torch.from_numpy(x)) > 0.5).numpy()[0, 0].sum() == 12
    # and the target's integer cast: 0.5 and 1.5 truncate to 0 and 1, 2 is not foreground
    t2 = t.copy()
    t2[0, 0, 0, 0], t2[0, 0, 0, 7], t2[0, 0, 7, 7] = 0.5, 1.5, 2.0
    g = (t2[:, 0].astype(np.int64) == 1)
    assert g[0, 0, 7] and not g[0, 0, 0] and not g[0, 7, 7]
    check_against_oracle(host(x, t2), x[:, 0] == 1.0, g)


def test_undefined_samples_are_flagged_and_zero():
    P, G = R.empty_case()
    got = host(*R.to_inputs(P, G))
    assert got["defined"].tolist() == [0, 0, 0, 1]
    check_against_oracle(got, P, G)
    for k in R.INT_FIELDS:
        assert not got[k][:3].any()


def test_refusals():
    import unet_hip
    from unet_hip import _lib
    from unet_hip.runtime import UNetRuntime
    lib = _lib.load()
    x = np.zeros((1, 1, 1, 2049), np.float32)
    oi, of = np.zeros(6, np.int64), np.zeros(2, np.float64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.unet_surface_stats_host(p(x), p(x), 1, 1, 1, 2049, p(oi), p(of)) == -2
    assert lib.unet_surface_stats_host(p(x), p(x), 1, 1, 2049, 1, p(oi), p(of)) == -2
    assert lib.unet_surface_stats_host(p(x), p(x), 1, 1, 1, 2048, p(oi), p(of)) == 0
    assert lib.unet_surface_stats_host(None, p(x), 1, 1, 1, 8, p(oi), p(of)) == -1
    assert lib.unet_surface_stats_host(p(x), p(x), 1, 1, 1, 8, None, p(of)) == -1
    assert lib.unet_surface_stats_host(p(x), p(x), 1, 1, 1, 8, p(oi), None) == -1
    with pytest.raises(_lib.HipError, match="UNET_ERR_SHAPE"):
        unet_hip.surface_metrics_host(torch.zeros(1, 1, 2049, 2), torch.zeros(1, 1, 2049, 2))
    # the device entry refuses before it touches the device
    rt = UNetRuntime("cuda:0")  # creating a context performs no device work
    d = ctypes.c_void_p(256)
    assert lib.unet_surface_stats(rt.ctx, d, d, 1, 1, 2049, 8, d, d, None) == -2
    assert b"2048" in lib.unet_last_error(rt.ctx)
    assert lib.unet_surface_stats(rt.ctx, None, d, 1, 1, 8, 8, d, d, None) == -1
    assert lib.unet_surface_stats(rt.ctx, d, d, 1, 1, 8, 8, None, d, None) == -1
    with pytest.raises(unet_hip.HipUnavailable):
        unet_hip.surface_metrics(torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8))


def test_flag_parses():
    import main
    assert main.get_parser(["--surface_metrics"]).surface_metrics is True
    assert main.get_parser([]).surface_metrics is False


# ---------------------------------------------------------------- Trainer.test on the CPU
class _StubRuntime:
    """unet_mask_counts restated in torch for the CPU (the trainer's only other device call)."""

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
        return images * 6 - 3  # the "image" is the predicted mask


def _cpu_trainer(tmp_path, batches, **cfg):
    from utils.trainer import Trainer
    tr = object.__new__(Trainer)
    tr.config = types.SimpleNamespace(result_dir=str(tmp_path), **cfg)
    tr.logger = logging.getLogger("surface_cpu")
    tr.rank0, tr.ddp, tr.device = True, None, torch.device("cpu")
    tr.model, tr.rt, tr.test_loader = _StubModel(), _StubRuntime(), batches
    tr._plot_contours = lambda keep: None
    return tr


def _batches():
    P, G = CASES["batch3_64x64"]
    Pe, Ge = R.empty_case()
    out = []
    for p, g in ((P, G), (np.kron(Pe, np.ones((8, 8), bool)), np.kron(Ge, np.ones((8, 8), bool)))):
        out.append((torch.from_numpy(p[:, None].astype(np.float32)), torch.from_numpy(g[:, None].astype(np.float32))))
    return out, np.concatenate([P, np.kron(Pe, np.ones((8, 8), bool))]), \
        np.concatenate([G, np.kron(Ge, np.ones((8, 8), bool))])


def test_trainer_test_without_the_flag_runs_no_surface_code(tmp_path, monkeypatch, capsys):
    import unet_hip

    def boom(*a, **k):
        raise AssertionError("surface_metrics called with the flag off")

    monkeypatch.setattr(unet_hip, "surface_metrics", boom)
    batches, _, _ = _batches()
    for cfg in ({}, {"surface_metrics": False}):
        m = _cpu_trainer(tmp_path, batches, **cfg).test()
        assert list(m) == ["TP", "FP", "FN", "TN", "ACC", "Precision", "Recall", "F1", "IoU"]
    assert "Surface" not in capsys.readouterr().out


def test_trainer_test_with_the_flag(tmp_path, monkeypatch, capsys):
    import unet_hip
    monkeypatch.setattr(unet_hip, "surface_metrics", unet_hip.surface_metrics_host)
    batches, P, G = _batches()
    m = _cpu_trainer(tmp_path, batches, surface_metrics=True).test()
    assert list(m) == ["TP", "FP", "FN", "TN", "ACC", "Precision", "Recall", "F1", "IoU",
                       "HD95", "HD", "ASSD", "SurfaceDefined"]
    want = [R.oracle(p, g) for p, g in zip(P, G)]
    ok = [w for w in want if w["defined"]]
    assert m["SurfaceDefined"] == len(ok) == 4 and len(want) == 7
    for k, f in (("HD95", "hd95"), ("HD", "hd"), ("ASSD", "assd")):
        ref = float(np.mean([w[f] for w in ok]))
        assert abs(m[k] - ref) <= REL * ref, (k, m[k], ref)
    out = capsys.readouterr().out.splitlines()
    assert out[-1] == (f"Surface Metrics — HD95={m['HD95']:.4f}, HD={m['HD']:.4f}, ASSD={m['ASSD']:.4f} px "
                       f"over 4 of 7 images (3 undefined)")
    assert out[-4].startswith("Test Metrics  —  Total Images: 7")
