"""GPU: the connected-component kernels (csrc/kernels_cc.hip) against the host twins that share
their rules (csrc/cc.h; the twins against scipy: test_cc_cpu.py), against scipy directly on the
512x512 batch, and Trainer.test with the post-processing and lesion options end to end.  Every
comparison of labels, masks and counts is exact."""
import numpy as np
import pytest
import torch

import cc_ref as R
import surface_ref as S
from test_gpu_surface import _trainer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = R.mask_cases()


def u8(m):
    return torch.from_numpy(np.ascontiguousarray(m).astype(np.uint8))


def check_all(x, conn, kind=None, rt=None):
    """labels, every post-processing combination and (against a shifted copy) the lesion counts
    of x: device == host twin, bit for bit.  Returns the device labels."""
    import unet_hip
    xd = x.to(DEV)
    lab, cnt = unet_hip.connected_components(xd, conn, kind)
    assert lab.device.type == "cuda" and lab.dtype == torch.int32 and cnt.dtype == torch.int32
    hl, hc = unet_hip.connected_components_host(x, conn, kind)
    assert np.array_equal(cnt.cpu().numpy(), hc.numpy()), (cnt, hc)
    assert np.array_equal(lab.cpu().numpy(), hl.numpy())
    for kl, small, fh in R.OPTIONS:
        out, info = unet_hip.postprocess_mask(xd, kl, 8 if small else 0, fh, conn, kind)
        ho, hi = unet_hip.postprocess_mask_host(x, kl, 8 if small else 0, fh, conn, kind)
        assert out.dtype == torch.uint8 and info.dtype == torch.int64
        assert np.array_equal(info.cpu().numpy(), hi.numpy()), (kl, small, fh, info, hi)
        assert np.array_equal(out.cpu().numpy(), ho.numpy()), (kl, small, fh)
    t = torch.from_numpy(R.to_targets(np.roll((hl != 0).numpy(), 3, axis=1)[::-1].copy(), C=x.shape[1] if x.dim() == 4 else 1))
    got = unet_hip.lesion_metrics(xd, t.to(DEV), conn, kind)
    want = unet_hip.lesion_metrics_host(x, t, conn, kind)
    for k in want:
        assert np.array_equal(got[k].cpu().numpy(), want[k].numpy()), k
    return lab.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("conn", R.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(CASES))
def test_device_matches_host_twin(name, conn):
    check_all(u8(CASES[name]), conn)


@pytest.mark.parametrize("conn", R.CONNECTIVITIES)
def test_min_area_edges_and_ties(conn):
    import unet_hip
    m = CASES["33x65"]
    for n in (2, 11, 14, 15):  # noise, ring, the tie pairs
        x = u8(m[n][None])
        for ma in R.min_areas(m[n], conn):
            for kl in (False, True):
                out, info = unet_hip.postprocess_mask(x.to(DEV), kl, ma, True, conn)
                want, winfo = R.postprocess(m[n], conn, kl, ma, True)
                assert info[0].tolist() == winfo and np.array_equal(out[0].cpu().numpy().astype(bool), want)


@pytest.mark.parametrize("tile", (0, 1, 2))
def test_every_tile_shape_gives_the_same_labels(tile):
    import unet_hip
    from unet_hip.runtime import UNetRuntime
    UNetRuntime.get(DEV).set_option("cc_tile", tile)  # restored after the test (conftest)
    for name in ("33x65", "96x160"):
        for conn in R.CONNECTIVITIES:
            lab, cnt = unet_hip.connected_components(u8(CASES[name]).to(DEV), conn)
            hl, hc = unet_hip.connected_components_host(u8(CASES[name]), conn)
            assert np.array_equal(lab.cpu().numpy(), hl.numpy()) and np.array_equal(cnt.cpu().numpy(), hc.numpy())


def test_512_batch_against_scipy_and_two_runs_identical():
    """The 512x512 batch against scipy directly, and twice: byte-identical results show that the
    order of the atomics does not matter.  The same twice for the 0.6-density 96x160 sample."""
    import unet_hip
    m = R.big_case()
    for conn in R.CONNECTIVITIES:
        x = u8(m).to(DEV)
        runs = [unet_hip.connected_components(x, conn) + unet_hip.postprocess_mask(x, True, 8, True, conn)
                for _ in range(2)]
        for a, b in zip(*runs):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        lab, cnt, out, info = (v.cpu().numpy() for v in runs[0])
        for n in range(2):
            want, k = R.label(m[n], conn)
            assert cnt[n] == k and np.array_equal(lab[n], want)
            wo, wi = R.postprocess(m[n], conn, True, 8, True)
            assert info[n].tolist() == wi and np.array_equal(out[n].astype(bool), wo)
        x = u8(CASES["96x160"][4:5]).to(DEV)
        a, b = unet_hip.connected_components(x, conn), unet_hip.connected_components(x, conn)
        assert all(p.cpu().numpy().tobytes() == q.cpu().numpy().tobytes() for p, q in zip(a, b))


def test_scratch_grows_and_is_reused():
    """A fresh context: a small call, a 700x300 call that outgrows its scratch, then the small
    call again in the grown scratch -- each equal to the host twin."""
    import unet_hip
    from unet_hip.runtime import UNetRuntime
    rt = UNetRuntime(DEV)
    r = np.random.default_rng(2)
    big = (R.ellipse(700, 300, 350, 150, 300, 120) ^ (r.random((700, 300)) < 0.05))[None]
    small = CASES["33x65"][[4, 11]]
    for m in (small, big, small):
        x = u8(m)[:, None]
        lab, cnt = rt.components(x.to(DEV), 0, 2)
        hl, hc = unet_hip.connected_components_host(x, 2)
        assert np.array_equal(lab.cpu().numpy(), hl.numpy()) and np.array_equal(cnt.cpu().numpy(), hc.numpy())
        out, info = rt.postprocess(x.to(DEV), 0, 1, True, 8, True)
        ho, hi = unet_hip.postprocess_mask_host(x, True, 8, True, 1)
        assert np.array_equal(out.cpu().numpy(), ho.numpy()) and np.array_equal(info.cpu().numpy(), hi.numpy())
        t = torch.from_numpy(R.to_targets(np.roll(m, 5, axis=2), C=1))
        got = rt.lesion_stats(x.to(DEV), 0, t.to(DEV), 1)
        want = unet_hip.lesion_metrics_host(x, t, 1)
        assert np.array_equal(got.cpu().numpy(), torch.stack(list(want.values()), 1).numpy())


def test_kinds_read_the_mask_readout():
    """Kind 1 on the threshold-edge logits (C = 2) gives the components of the mask that
    unet_mask_counts writes; logits and targets of the patterns give the patterns' components."""
    import unet_hip
    from unet_hip.runtime import UNetRuntime
    x = R.edge_logits()
    xd = torch.from_numpy(x).to(DEV)
    mask = torch.empty(x.shape, dtype=torch.uint8, device=DEV)
    UNetRuntime.get(DEV).mask_counts(xd, torch.zeros_like(xd), torch.zeros(6, dtype=torch.int64, device=DEV), mask)
    m = mask.cpu().numpy()[:, 0].astype(bool)
    assert not m[x[:, 0] == 0].any() and m[x[:, 0] == 1].all()
    for conn in R.CONNECTIVITIES:
        lab, cnt = unet_hip.connected_components(xd, conn)
        for n in range(2):
            want, k = R.label(m[n], conn)
            assert cnt[n].item() == k and np.array_equal(lab[n].cpu().numpy(), want)
        check_all(torch.from_numpy(x), conn)
        p = CASES["33x65"]
        lab, cnt = check_all(torch.from_numpy(R.to_logits(p)), conn)
        for n in range(len(p)):
            assert np.array_equal(lab[n], R.label(p[n], conn)[0])
        t = R.to_targets(p)
        lab, cnt = check_all(torch.from_numpy(t), conn, "targets")
        for n in range(len(p)):
            assert np.array_equal(lab[n], R.label(t[n, 0].astype(np.uint8) == 1, conn)[0])


def test_trainer_test_postprocess_and_lesion_metrics(tmp_path, capsys):
    tr, loaders = _trainer(tmp_path, surface_metrics=True, pp_largest=True, pp_min_area=8, pp_fill_holes=True,
                           lesion_metrics=True)
    for e in range(3):  # enough for non-trivial masks
        tr.train_one_epoch(e)
    m = tr.test()
    base = ["TP", "FP", "FN", "TN", "ACC", "Precision", "Recall", "F1", "IoU"]
    assert list(m) == (base + ["HD95", "HD", "ASSD", "SurfaceDefined"] + ["PP_" + k for k in base] +
                       ["PP_HD95", "PP_HD", "PP_ASSD", "PP_SurfaceDefined"] +
                       ["LesionRecall", "LesionPrecision", "FPComponentsPerImage", "PredComponents", "GTComponents"])
    pp, gt = [], []
    tr.model.eval()
    with torch.no_grad():
        for xb, yb in loaders[2]:
            logits = tr.model(xb.to(DEV).float())
            mask = torch.empty(logits.shape, dtype=torch.uint8, device=DEV)
            tr.rt.mask_counts(logits, yb.to(DEV).float(), torch.zeros(6, dtype=torch.int64, device=DEV), mask)
            pp += [R.postprocess(p[0] != 0, 1, True, 8, True)[0] for p in mask.cpu().numpy()]
            gt += [g[0].astype(np.int64) == 1 for g in yb.numpy()]
    assert len(pp) == 6
    P, G = np.stack(pp), np.stack(gt)
    assert all(R.label(p, 1)[1] <= 1 for p in pp)  # every post-processed mask: at most one component
    want = dict(PP_TP=int((P & G).sum()), PP_FP=int((P & ~G).sum()), PP_FN=int((~P & G).sum()),
                PP_TN=int((~P & ~G).sum()))
    print({k: m[k] for k in m if k.startswith(("PP_", "Lesion", "FP", "Pred", "GT"))})
    for k, v in want.items():
        assert m[k] == v, (k, m[k], v)
    les = np.array([R.lesion(p, g, 1) for p, g in zip(pp, gt)]).sum(0)
    assert m["PredComponents"] == les[0] and m["GTComponents"] == les[1]
    assert m["LesionRecall"] == (les[2] / les[1] if les[1] else float("nan")) or (les[1] == 0 and np.isnan(m["LesionRecall"]))
    assert m["LesionPrecision"] == (les[3] / les[0] if les[0] else float("nan")) or (les[0] == 0 and np.isnan(m["LesionPrecision"]))
    assert m["FPComponentsPerImage"] == (les[0] - les[3]) / 6
    surf = [S.oracle(p, g) for p, g in zip(pp, gt)]
    ok = [w for w in surf if w["defined"]]
    assert m["PP_SurfaceDefined"] == len(ok)
    for k, f in (("PP_HD95", "hd95"), ("PP_HD", "hd"), ("PP_ASSD", "assd")):
        if ok:
            ref = float(np.mean([w[f] for w in ok]))
            assert abs(m[k] - ref) <= 1e-9 * max(ref, 1e-300), (k, m[k], ref)
        else:
            assert np.isnan(m[k])
    out = capsys.readouterr().out
    assert "Post-processed" in out and "Lesion Metrics" in out
