"""GPU: the test-time-augmentation kernels (csrc/kernels_tta.hip) against the host twins that share
their rules (csrc/tta.h; the twins against NumPy: test_tta_cpu.py), the unaligned / scalar
paths, the sample and channel strides, and Trainer.test with config.tta end to end.  Views, the
mode-0 merge and every vote count are compared bit for bit."""
import numpy as np
import pytest
import torch

import cc_ref
import surface_ref
import tta_ref as R
from test_gpu_surface import _trainer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = R.cases() + [R.BIG]


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def t(a):
    return torch.from_numpy(np.array(a, order="C"))  # a copy: the shared inputs are read-only


def same_merge(got, want):
    assert got["score"].device.type == "cuda" and got["mask"].dtype == torch.uint8 and got["votes"].dtype == torch.uint8
    assert np.array_equal(bits(got["score"]), bits(want["score"]))
    assert np.array_equal(got["mask"].cpu().numpy(), want["mask"].numpy())
    assert np.array_equal(got["votes"].cpu().numpy(), want["votes"].numpy())


@pytest.mark.parametrize("case", CASES, ids=R.case_id)
def test_device_matches_host_twin(case):
    """views, mode-0 score / mask / votes and mode-1 votes bit for bit; the mode-1 score within
    the bound test_tta_cpu.test_merge_prob_against_float64 derives (expf differs between libm and
    the device) and the mode-1 mask equal on inputs whose reference keeps clear of 0.5."""
    import unet_hip
    shape, mask = case
    n, K = shape[0], len(R.numbers(mask))
    logits, ref, ref_mask = R.prob_inputs(shape, mask)  # asserts the margin before any code runs
    x = t(logits[:n])
    assert np.array_equal(bits(unet_hip.tta_views(x.to(DEV), mask)), bits(unet_hip.tta_views_host(x, mask)))
    for lg in ([t(logits)] if case == R.BIG else [t(logits), t(R.ramp(shape, K))]):
        same_merge(unet_hip.tta_merge(lg.to(DEV), n, mask, "logit"), unet_hip.tta_merge_host(lg, n, mask, "logit"))
    got = unet_hip.tta_merge(t(logits).to(DEV), n, mask, "prob")
    want = unet_hip.tta_merge_host(t(logits), n, mask, "prob")
    assert np.array_equal(got["votes"].cpu().numpy(), want["votes"].numpy())
    diff = (got["score"].cpu().double() - want["score"].double()).abs().max().item()
    dref = np.abs(got["score"].cpu().numpy().astype(np.float64) - ref).max()
    print(f"{R.case_id(case)}: K {K}, worst |device - host| {diff:.3e}, |device - float64| {dref:.3e}, "
          f"bound {R.prob_bound(K):.3e}")
    assert diff <= R.prob_bound(K)
    assert np.array_equal(got["mask"].cpu().numpy(), ref_mask)


@pytest.mark.parametrize("shape,mask", [((1, 2, 130, 67), 0x0F), ((1, 1, 64, 64), 0xFF), ((1, 2, 8, 12), 0x0F)],
                         ids=["w67-flips", "64-d4", "w12-flips"])
def test_slice_one_float_into_a_buffer(shape, mask):
    """A base pointer that is only 4-byte aligned (and W = 67, no multiple of 4): the scalar
    paths, for rows of every alignment."""
    import unet_hip
    K = len(R.numbers(mask))
    x = R.ramp(shape)
    buf = torch.zeros(x.size + 1, device=DEV)
    buf[1:] = t(x).to(DEV).flatten()
    xd = buf[1:].view(shape)
    assert xd.data_ptr() % 16 == 4 and xd.is_contiguous()
    assert np.array_equal(bits(unet_hip.tta_views(xd, mask)), bits(R.views(x, mask)))
    lg = R.ramp(shape, K)
    buf = torch.zeros(lg.size + 1, device=DEV)
    buf[1:] = t(lg).to(DEV).flatten()
    ld = buf[1:].view(lg.shape)
    assert ld.data_ptr() % 16 == 4
    for mode in ("logit", "prob"):
        got = unet_hip.tta_merge(ld, shape[0], mask, mode)
        aligned = unet_hip.tta_merge(t(lg).to(DEV), shape[0], mask, mode)
        for k in got:  # the path must not change a bit
            assert torch.equal(got[k], aligned[k]), (mode, k)
    same_merge(unet_hip.tta_merge(ld, shape[0], mask, "logit"), unet_hip.tta_merge_host(t(lg), shape[0], mask, "logit"))


@pytest.mark.parametrize("shape,mask", [((3, 2, 70, 70), 0xFF), ((3, 2, 8, 12), 0x0F), ((3, 2, 5, 7), 0x0A)],
                         ids=["70-d4", "8x12-flips", "5x7-0x0a"])
def test_sample_and_channel_strides(shape, mask):
    """N = 3 and C = 2 against the NumPy definition itself: a wrong sample, channel or view
    stride moves a plane."""
    import unet_hip
    K = len(R.numbers(mask))
    x = R.ramp(shape)
    assert np.array_equal(bits(unet_hip.tta_views(t(x).to(DEV), mask)), bits(R.views(x, mask)))
    lg = R.ramp(shape, K)
    got = unet_hip.tta_merge(t(lg).to(DEV), shape[0], mask, "logit")
    score, m, v = R.merge_logit(lg, shape[0], mask)
    assert np.array_equal(bits(got["score"]), bits(score))
    assert np.array_equal(got["mask"].cpu().numpy(), m)
    assert np.array_equal(got["votes"].cpu().numpy(), v)


def test_two_runs_identical_and_null_outputs():
    import unet_hip
    from unet_hip.runtime import UNetRuntime
    shape, mask = (2, 2, 70, 70), 0xFF
    logits = t(R.prob_inputs(shape, mask)[0]).to(DEV)
    rt = UNetRuntime.get(DEV)
    for mode in (0, 1):
        a = rt.tta_merge(logits, 2, mask, mode)
        b = rt.tta_merge(logits, 2, mask, mode)
        assert all(torch.equal(p, q) for p, q in zip(a, b))
        for wm, wv in ((False, True), (True, False), (False, False)):
            s, m, v = rt.tta_merge(logits, 2, mask, mode, want_mask=wm, want_votes=wv)
            assert torch.equal(s, a[0]) and (m is None) == (not wm) and (v is None) == (not wv)
            assert m is None or torch.equal(m, a[1])
            assert v is None or torch.equal(v, a[2])
    x = logits[:2]
    assert torch.equal(unet_hip.tta_views(x, mask), unet_hip.tta_views(x, mask))
    with pytest.raises(unet_hip.HipError, match="UNET_ERR_SHAPE"):
        unet_hip.tta_views(torch.zeros(1, 1, 4, 6, device=DEV), "d4")
    with pytest.raises(unet_hip.HipError, match="UNET_ERR_INVALID"):
        unet_hip.tta_views(x, 0x100)
    torch.cuda.synchronize()


def _torch_view(x, k):
    y = x
    if k & 4:
        y = y.transpose(-1, -2)
    if k & 2:
        y = torch.flip(y, (-2,))
    if k & 1:
        y = torch.flip(y, (-1,))
    return y.contiguous()


def test_trainer_test_with_tta(tmp_path, capsys):
    """tta="none" leaves the report as it is; tta="d4" keeps the raw block and adds the TTA block,
    whose counts equal an independent route (torch.flip / transpose views through the model,
    merged by the host twin); the surface and post-processing blocks then read the TTA mask."""
    import unet_hip
    tr, loaders = _trainer(tmp_path)
    for e in range(20):  # 40 steps: the BN running statistics Trainer.test evaluates with have settled
        tr.train_one_epoch(e)
    base = ["TP", "FP", "FN", "TN", "ACC", "Precision", "Recall", "F1", "IoU"]
    plain = tr.test()
    assert list(plain) == base and not any(k.startswith("TTA_") for k in plain)
    tr.config.tta, tr.config.tta_merge = "none", "prob"
    again = tr.test()
    assert again == plain
    assert "TTA" not in capsys.readouterr().out

    tr.config.tta = "d4"
    m = tr.test()
    out = capsys.readouterr().out
    assert "TTA (d4, prob)" in out and "Test Metrics" in out
    assert list(m) == base + ["TTA_" + k for k in base] + ["TTA_Disagreement"]
    assert {k: m[k] for k in base} == plain  # the raw block is the plain forward's

    masks, gts, n_dis = [], [], 0
    tr.model.eval()
    with torch.no_grad():
        for xb, yb in loaders[2]:
            x = xb.to(DEV).float()
            logits = torch.cat([tr.model(_torch_view(x, k)).float() for k in range(8)]).cpu()
            h = unet_hip.tta_merge_host(logits, x.shape[0], "d4", "prob")
            masks += [p[0] != 0 for p in h["mask"].numpy()]
            gts += [g[0].astype(np.int64) == 1 for g in yb.numpy()]
            v = h["votes"].numpy()
            n_dis += int(((v > 0) & (v < 8)).sum())
    P, G = np.stack(masks), np.stack(gts)
    want = dict(TTA_TP=int((P & G).sum()), TTA_FP=int((P & ~G).sum()), TTA_FN=int((~P & G).sum()),
                TTA_TN=int((~P & ~G).sum()))
    print({k: m[k] for k in m if k.startswith("TTA_")}, "raw", {k: m[k] for k in base[:4]}, "disagree", n_dis)
    for k, w in want.items():
        assert m[k] == w, (k, m[k], w)
    assert m["TTA_Disagreement"] == n_dis / P.size
    assert 0 < P.sum() < P.size

    tr.config.surface_metrics, tr.config.pp_largest = True, True
    m2 = tr.test()
    out = capsys.readouterr().out
    assert "Surface Metrics (TTA mask)" in out and "(TTA mask)\n" in out.split("Post-processed")[1]
    assert {k: m2[k] for k in m} == m
    surf = [surface_ref.oracle(p, g) for p, g in zip(masks, gts)]
    ok = [w for w in surf if w["defined"]]
    assert m2["SurfaceDefined"] == len(ok)
    for k, f in (("HD95", "hd95"), ("HD", "hd"), ("ASSD", "assd")):
        if ok:
            ref = float(np.mean([w[f] for w in ok]))
            assert abs(m2[k] - ref) <= 1e-9 * max(ref, 1e-300), (k, m2[k], ref)
        else:
            assert np.isnan(m2[k])
    PP = np.stack([cc_ref.postprocess(p, 1, True, 0, False)[0] for p in masks]).astype(bool)
    want = dict(PP_TP=int((PP & G).sum()), PP_FP=int((PP & ~G).sum()), PP_FN=int((~PP & G).sum()),
                PP_TN=int((~PP & ~G).sum()))
    for k, w in want.items():
        assert m2[k] == w, (k, m2[k], w)
