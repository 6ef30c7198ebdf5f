"""GPU: unet_surface_stats (csrc/kernels_surf.hip) against the host hook that shares its source
(csrc/surf.h; the hook against the definition: test_surface_cpu.py), and Trainer.test with
config.surface_metrics end to end.

Bounds.  Every integer field is exact (integer atomics, int32 distances).  The float64 sums may
differ from the hook's raster-order sum by their order alone: 1e-12 relative (at most 2 H W
terms of one sign; the observed figure is printed before it is asserted)."""
import argparse
import os

import numpy as np
import pytest
import scipy.ndimage as nd
import torch

import surface_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SUM_REL = 1e-12
CASES = R.mask_cases()


def device(x, t):
    import unet_hip
    out = unet_hip.surface_metrics(torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV))
    assert all(v.device.type == "cuda" for v in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


def host(x, t):
    import unet_hip
    return {k: v.numpy() for k, v in unet_hip.surface_metrics_host(torch.from_numpy(x), torch.from_numpy(t)).items()}


def check_device_against_host(x, t):
    got, want = device(x, t), host(x, t)
    for k in R.INT_FIELDS:
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    for k in ("sum_pg", "sum_gp"):
        rel = np.abs(got[k] - want[k]) / np.maximum(np.abs(want[k]), 1e-300)
        print(f"{k}: worst relative difference {rel.max():.3e}")
        assert (rel <= SUM_REL).all(), (k, got[k], want[k])
    for k in ("hd", "hd95", "assd"):
        assert np.allclose(got[k], want[k], rtol=1e-12, atol=0, equal_nan=True), (k, got[k], want[k])
    return got


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_matches_host_hook(name):
    got = check_device_against_host(*R.to_inputs(*CASES[name]))
    assert got["defined"].all()


def test_undefined_samples_and_extra_channels():
    got = check_device_against_host(*R.to_inputs(*R.empty_case(), C=2))
    assert got["defined"].tolist() == [0, 0, 0, 1]
    assert np.isnan(got["hd95"][:3]).all() and not got["max_d2"][:3].any()


def test_512_batch2_three_pass_select():
    P, G = R.big_case()
    o = R.oracle(P[1], G[1])
    st = nd
    bp = P[1] & ~st.binary_erosion(P[1], st.generate_binary_structure(2, 1))
    bg = G[1] & ~st.binary_erosion(G[1], st.generate_binary_structure(2, 1))
    keys = np.concatenate([np.rint(st.distance_transform_edt(~bg)[bp] ** 2),
                           np.rint(st.distance_transform_edt(~bp)[bg] ** 2)])
    assert np.unique(keys).size > 2 ** 11 and o["max_d2"] >= 2 ** 16  # three 8-bit digits
    got = check_device_against_host(*R.to_inputs(P, G))
    for n in range(2):
        want = R.oracle(P[n], G[n])
        assert all(int(got[k][n]) == want[k] for k in R.INT_FIELDS)


def test_two_runs_are_bit_identical():
    P, G = R.big_case()
    x, t = R.to_inputs(P, G)
    a, b = device(x, t), device(x, t)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    x, t = R.to_inputs(*CASES["batch3_64x64"])
    a, b = device(x, t), device(x, t)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_scratch_grows_and_is_reused():
    """A fresh context: a small call, a 700x300 call that outgrows its scratch, then the small
    call again in the grown scratch -- each equal to the host hook."""
    from unet_hip.functional import _surface_finalize
    from unet_hip.runtime import UNetRuntime
    rt = UNetRuntime(DEV)
    r = np.random.default_rng(2)
    big = (R.ellipse(700, 300, 350, 150, 300, 120)[None] | (r.random((1, 700, 300)) < 0.01),
           R.ellipse(700, 300, 300, 170, 250, 100)[None])
    small = CASES["hole_40x72"]
    for P, G in (small, big, small):
        x, t = R.to_inputs(P, G)
        got = _surface_finalize(*rt.surface_stats(torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)))
        want = host(x, t)
        for k in R.INT_FIELDS:
            assert np.array_equal(got[k].cpu().numpy(), want[k]), k
        for k in ("sum_pg", "sum_gp"):
            assert np.allclose(got[k].cpu().numpy(), want[k], rtol=SUM_REL, atol=0), k


def test_predicate_is_the_mask_readout():
    """The surfaces are those of unet_mask_counts's mask: logits around the float32 threshold of
    sigmoid(x) > 0.5 (0, the smallest positive float, the ulps around 2^-23 .. 2^-22) give the
    statistics of the mask the readout writes."""
    import unet_hip
    from unet_hip.runtime import UNetRuntime
    r = np.random.default_rng(4)
    tiny = np.nextafter(np.float32(0), np.float32(1))
    vals = np.array([0.0, tiny, -tiny, 5.9e-8, 6.0e-8, 1.19e-7, 1.2e-7, 2.4e-7, 1e-6, -1e-6, 1.0, -1.0], np.float32)
    x = vals[r.integers(0, vals.size, (2, 1, 33, 65))]
    t = R.ellipse(33, 65, 16, 30, 10, 20)[None, None].repeat(2, 0).astype(np.float32)
    xd, td = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
    mask = torch.empty(x.shape, dtype=torch.uint8, device=DEV)
    UNetRuntime.get(DEV).mask_counts(xd, td, torch.zeros(6, dtype=torch.int64, device=DEV), mask)
    m = mask.cpu().numpy()[:, 0].astype(bool)
    assert not m[x[:, 0] == 0].any() and not m[x[:, 0] == tiny].any() and m[x[:, 0] == 1].all()
    got = {k: v.cpu().numpy() for k, v in unet_hip.surface_metrics(xd, td).items()}
    for n in range(2):
        want = R.oracle(m[n], t[n, 0] == 1)
        assert all(int(got[k][n]) == want[k] for k in R.INT_FIELDS), (n, want)


# ---------------------------------------------------------------- Trainer.test end to end
def _trainer(tmp, **kw):
    from data.data_loader import SyntheticSegmentation, create_dataloader
    from models.mod import ResUNet
    from utils.trainer import Trainer
    from utils.utils import Config, create_logger
    ns = argparse.Namespace(model_type="ResUNet", lr=1e-3, bce_ratio=1.0, dice_ratio=1.0, focal_ratio=0.0,
                            boundary_ratio=0.0, use_mixup=False, mixup_prob=0.0, mixup_alpha=0.2,
                            epochs=1, early_stop_patience=5, batch_size=3, num_workers=0, **kw)
    cfg = Config(ns, base_dir=str(tmp))
    cfg.device = DEV
    loaders = tuple(create_dataloader(SyntheticSegmentation(6, 64, seed=s), cfg, shuffle=False)
                    for s in range(3))
    torch.manual_seed(0)
    model = ResUNet(base_filters=16, depth=3)
    return Trainer(cfg, loaders, create_logger(os.path.join(cfg.log_dir, "t.log")), model), loaders


def test_trainer_test_reports_surface_metrics(tmp_path, capsys):
    tr, loaders = _trainer(tmp_path, surface_metrics=True)
    for e in range(3):  # enough for non-trivial masks
        tr.train_one_epoch(e)
    m = tr.test()
    assert list(m) == ["TP", "FP", "FN", "TN", "ACC", "Precision", "Recall", "F1", "IoU",
                       "HD95", "HD", "ASSD", "SurfaceDefined"]
    want = []
    tr.model.eval()
    with torch.no_grad():
        for xb, yb in loaders[2]:
            logits = tr.model(xb.to(DEV).float())
            mask = torch.empty(logits.shape, dtype=torch.uint8, device=DEV)
            tr.rt.mask_counts(logits, yb.to(DEV).float(), torch.zeros(6, dtype=torch.int64, device=DEV), mask)
            want += [R.oracle(p[0] != 0, g[0].astype(np.int64) == 1)
                     for p, g in zip(mask.cpu().numpy(), yb.numpy())]
    ok = [w for w in want if w["defined"]]
    print(f"defined {len(ok)} of {len(want)}: HD95 {m['HD95']}, HD {m['HD']}, ASSD {m['ASSD']}")
    assert len(want) == 6 and m["SurfaceDefined"] == len(ok) >= 1
    for k, f in (("HD95", "hd95"), ("HD", "hd"), ("ASSD", "assd")):
        ref = float(np.mean([w[f] for w in ok]))
        assert abs(m[k] - ref) <= 1e-9 * max(ref, 1e-300), (k, m[k], ref)
    assert (f"over {len(ok)} of 6 images ({6 - len(ok)} undefined)") in capsys.readouterr().out


def test_trainer_test_default_keys_unchanged(tmp_path, capsys):
    tr, _ = _trainer(tmp_path)
    m = tr.test()
    assert list(m) == ["TP", "FP", "FN", "TN", "ACC", "Precision", "Recall", "F1", "IoU"]
    assert "Surface" not in capsys.readouterr().out
