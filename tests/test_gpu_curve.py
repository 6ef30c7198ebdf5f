"""GPU: unet_curve_hist / unet_curve_stats (csrc/kernels_curve.hip) against the host twins that share
their source (csrc/curve.h; the twins against the NumPy restatement: test_curve_cpu.py), bit for
bit -- integer atomics are exact and the Dice sums are added in ascending plane order on both sides
-- and Trainer.test with the new switches end to end."""
import numpy as np
import pytest
import torch

import curve_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def edges(B):
    import unet_hip
    return unet_hip.curve_edges(B)


def placed(x, off, device):
    """The array as a tensor on `device`, taken `off` floats into a buffer when off > 0."""
    if not off:
        return torch.from_numpy(np.ascontiguousarray(x)).to(device)
    buf = torch.zeros(x.size + off, dtype=torch.float32, device=device)
    buf[off:] = torch.from_numpy(x.reshape(-1)).to(device)
    v = buf[off:].view(x.shape)
    assert v.data_ptr() % 16 == 4 * off % 16
    return v


def both(x, t, e, off=0):
    """(device, host) results: plane_hist, total, out_i64 fields, dice_sum as numpy arrays."""
    import unet_hip
    out = []
    for dev, hist, stats in ((DEV, unet_hip.curve_hist, unet_hip.curve_stats),
                             ("cpu", unet_hip.curve_hist_host, unet_hip.curve_stats_host)):
        ph, tot = hist(placed(x, off, dev), placed(t, off, dev), e)
        st = stats(ph)
        assert ph.device.type == tot.device.type == st["dice_sum"].device.type == torch.device(dev).type
        out.append(dict(plane_hist=ph.cpu().numpy(), total=tot.cpu().numpy(),
                        dice_sum=st["dice_sum"].cpu().numpy().view(np.uint64),
                        **{k: st[k].cpu().numpy() for k in R.FIELDS}))
    return out


def assert_same(got, want):
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def _case_ids():
    return [(B, name) for B in R.BINS for name in sorted(R.small_cases(B, R.edges(B)))]


@pytest.mark.parametrize("B,name", _case_ids())
def test_device_matches_host_twin(B, name):
    e = edges(B)
    x, t, off = R.small_cases(B, e.numpy())[name]
    got, want = both(x, t, e, off)
    assert_same(got, want)
    assert int(got["total"].sum()) == x.size


@pytest.mark.parametrize("B", R.BINS)
def test_big_case_and_two_runs_agree(B):
    x, t = R.big_case()
    e = edges(B)
    got, want = both(x, t, e)
    assert_same(got, want)
    again, _ = both(x, t, e)
    assert_same(again, got)
    if B == 256:
        assert got["plane_hist"][:, 0, :2].sum() > 0.8 * x.size  # the contended bins


def test_sliced_pointers_take_the_scalar_path():
    """Every 4-byte alignment of the logits and of the targets, hw a multiple of 4 and not."""
    import unet_hip
    e = edges(16)
    r = np.random.default_rng(8)
    for hw in (4096, 4097):
        x, t = r.normal(-2, 4, (2, hw)).astype(np.float32), (r.random((2, hw)) < 0.3).astype(np.float32)
        want_h, want_tot = R.hist(x, t, e.numpy())
        for ox in range(4):
            for ot in (0, 3):
                ph, tot = unet_hip.curve_hist(placed(x, ox, DEV), placed(t, ot, DEV), e)
                assert np.array_equal(ph.cpu().numpy(), want_h) and np.array_equal(tot.cpu().numpy(), want_tot)


def test_accumulates_into_non_zero_total_and_dice_sum():
    import unet_hip
    B = 256
    e = edges(B)
    cs = R.small_cases(B, e.numpy())
    r = np.random.default_rng(5)
    tot0 = r.integers(1, 10 ** 12, 2 * B + 1)
    ds0 = r.random(B + 1)
    res = []
    for dev, hist, stats in ((DEV, unet_hip.curve_hist, unet_hip.curve_stats),
                             ("cpu", unet_hip.curve_hist_host, unet_hip.curve_stats_host)):
        tot, ds = torch.from_numpy(tot0.copy()).to(dev), torch.from_numpy(ds0.copy()).to(dev)
        for name in ("target_values_2x25x40", "aligned_3x64x64", "unaligned_2x7x333"):
            x, t, _ = cs[name]
            ph, tot_out = hist(placed(x, 0, dev), placed(t, 0, dev), e, tot)
            assert tot_out is tot
            assert stats(ph, ds)["dice_sum"] is ds
        res.append((tot.cpu().numpy(), ds.cpu().numpy().view(np.uint64)))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    want = tot0 + sum(R.hist(*cs[n][:2], e.numpy())[1] for n in ("target_values_2x25x40", "aligned_3x64x64",
                                                                 "unaligned_2x7x333"))
    assert np.array_equal(res[0][0], want)


def test_outputs_stay_inside_their_buffers():
    """Poisoned margins either side of every output are untouched."""
    from unet_hip.runtime import UNetRuntime
    rt = UNetRuntime.get(DEV)
    G = 512
    for B, name in ((2, "unaligned_2x7x333"), (1024, "aligned_3x64x64"), (256, "values_on_the_edges")):
        e = edges(B)
        x, t, _ = R.small_cases(B, e.numpy())[name]
        planes = x.shape[0]
        ph = torch.full((G + planes * 2 * B + G,), -7, dtype=torch.int32, device=DEV)
        tot = torch.full((G + 2 * B + 1 + G,), -7, dtype=torch.int64, device=DEV)
        oi = torch.full((G + planes * 8 + G,), -7, dtype=torch.int64, device=DEV)
        ds = torch.full((G + B + 1 + G,), -7.0, dtype=torch.float64, device=DEV)
        tot[G:G + 2 * B + 1] = 0
        ds[G:G + B + 1] = 0
        xd, td, ed = placed(x, 0, DEV), placed(t, 0, DEV), e.to(DEV)
        from unet_hip import _lib
        s = _lib.stream_ptr(DEV)
        p = lambda a, off: _lib.ptr(a[off:])
        _lib.check(rt.lib.unet_curve_hist(rt.ctx, _lib.ptr(xd), _lib.ptr(td), planes, x.shape[1], _lib.ptr(ed), B,
                                          p(ph, G), p(tot, G), s), rt.ctx, "hist")
        _lib.check(rt.lib.unet_curve_stats(rt.ctx, p(ph, G), planes, B, p(oi, G), p(ds, G), s), rt.ctx, "stats")
        for buf, n in ((ph, planes * 2 * B), (tot, 2 * B + 1), (oi, planes * 8), (ds, B + 1)):
            assert (buf[:G] == -7).all() and (buf[G + n:] == -7).all()
        want_h, want_tot = R.hist(x, t, e.numpy())
        assert np.array_equal(ph[G:G + planes * 2 * B].cpu().numpy(), want_h.reshape(-1))
        assert np.array_equal(tot[G:G + 2 * B + 1].cpu().numpy(), want_tot)


@pytest.mark.parametrize("B", [2, 256, 1024])
def test_reversed_edges_still_count_every_pixel(B):
    """Range safety: with unsorted edges the bins mean nothing, but each lies inside the histogram."""
    import unet_hip
    x, t = R.big_case()
    x, t = x[:2], t[:2]
    ph, tot = unet_hip.curve_hist(torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV), edges(B).flip(0))
    ph, tot = ph.cpu().numpy(), tot.cpu().numpy()
    assert (ph >= 0).all() and ph.sum() == x.size and tot[:2 * B].sum() == x.size and tot[2 * B] == 0
    assert np.array_equal(ph.sum(2), np.stack([(t == 0).sum(1), (t == 1).sum(1)], 1))


# ---------------------------------------------------------------- Trainer.test end to end
BASE_KEYS = ["TP", "FP", "FN", "TN", "ACC", "Precision", "Recall", "F1", "IoU"]


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    from test_gpu_surface import _trainer
    tr, loaders = _trainer(tmp_path_factory.mktemp("curve"))
    for ep in range(3):  # enough for non-trivial masks
        tr.train_one_epoch(ep)
    base = tr.test()
    assert list(base) == BASE_KEYS
    tr.model.eval()
    got = []
    with torch.no_grad():
        for loader in loaders[1:]:  # val, test
            xs, ts = [], []
            for xb, yb in loader:
                xs.append(tr.model(xb.to(DEV).float()).cpu())
                ts.append(yb.float())
            got.append((xs, ts))
    return tr, base, got[0], got[1]


def _host_summary(batches, B):
    import unet_hip
    e = unet_hip.curve_edges(B)
    tot = ds = None
    n = 0
    for x, t in zip(*batches):
        ph, tot = unet_hip.curve_hist_host(x[:, :1], t[:, :1], e, tot)
        ds = unet_hip.curve_stats_host(ph, ds)["dice_sum"]
        n += x.shape[0]
    return unet_hip.curve_summary(tot.tolist(), ds.tolist(), n, e)


def _flat(batches):
    return (torch.cat(batches[0])[:, 0].reshape(-1, 64 * 64).numpy(), torch.cat(batches[1])[:, 0].reshape(-1, 64 * 64).numpy())


@pytest.mark.parametrize("setting", [dict(curve_metrics=True), dict(threshold=0.3), dict(threshold="val-dice")],
                         ids=["curve_metrics", "threshold_0.3", "threshold_val_dice"])
def test_trainer_test_with_the_switches(trained, setting, capsys):
    tr, base, val, test = trained
    B = 256
    for k in ("curve_metrics", "threshold"):
        if hasattr(tr.config, k):
            delattr(tr.config, k)
    for k, v in setting.items():
        setattr(tr.config, k, v)
    try:
        m = tr.test()
    finally:
        for k in setting:
            delattr(tr.config, k)
    assert {k: m[k] for k in BASE_KEYS} == base and list(m)[:len(BASE_KEYS)] == BASE_KEYS
    out = capsys.readouterr().out
    if "curve_metrics" in setting:
        s = _host_summary(test, B)
        print(f"AUROC {s['auroc']}, AP {s['ap']}, best Dice {s['best_global_dice']} at {s['best_global_threshold']}")
        want = dict(Curve_AUROC=s["auroc"], Curve_AP=s["ap"], Curve_BestDice=s["best_global_dice"],
                    Curve_BestDiceThreshold=s["best_global_threshold"], Curve_Dice=s["dice_global_half"],
                    Curve_BestImageDice=s["best_image_dice"], Curve_BestImageDiceThreshold=s["best_image_threshold"],
                    Curve_ImageDice=s["dice_image_half"], Curve_Ignored=s["ignored"], Curve_Bins=B)
        assert {k: v for k, v in m.items() if k.startswith("Curve_")} == want
        assert s["planes"] == 6 and "Curve Metrics (256 bins)" in out
        assert not any(k.startswith("OPT_") for k in m)
    else:
        assert not any(k.startswith("Curve_") for k in m) and "Curve Metrics" not in out
        k = 77 if setting["threshold"] == 0.3 else _host_summary(val, B)["best_global_k"]
        assert m["OPT_Threshold"] == k / B
        x, t = _flat(test)
        assert (m["OPT_TP"], m["OPT_FP"], m["OPT_FN"], m["OPT_TN"]) == R.counts(x, t, edges(B).numpy(), k)
        assert f"(k={k} of {B}" in out
