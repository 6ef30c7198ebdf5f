"""The loss kernels (loss_stats / loss_sums / loss_finalize / loss_bwd, kernels_misc.hip) element
by element against the fp64 reference of tests/loss_ref.py, through rt.loss_fwd / rt.loss_bwd.

Bar (measured, not fixed): the same formulas through torch CPU ops and autograd in float32 are
the yardstick.  With err = max |a - ref| / max |ref| per sample for dlogits and |a - ref| for the
three losses, the kernel must stay within max(4 x the yardstick's err, 16 x 2^-24): 4 for the
device's 1-ulp expf / log1pf and its chunked float sums, the floor so that a case where torch
fp32 happens to be exact does not ask for bit-equality.  The worst values are tabulated in
DESIGN.md (section 3, "Loss statistics over 64 chunks per sample").

Shapes: the smallest that reach each path of loss_stats_kernel --
(3, 1, 16, 16) one chunk, vector path; (2, 3, 17, 19) scalar path, several classes;
(2, 1, 4, 4099) per % 4 == 0 with G = 4 chunks of 4099: the scalar fall-back; (2, 1, 128, 128)
G = 4 on the vector path; and the first on views one float off a 16-byte boundary."""
import numpy as np
import pytest
import torch

import loss_ref as L

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FLOOR = 16 * 2.0 ** -24
SHAPES = [((3, 1, 16, 16), 0), ((2, 3, 17, 19), 0), ((2, 1, 4, 4099), 0), ((2, 1, 128, 128), 0),
          ((3, 1, 16, 16), 1)]


def _rt():
    import unet_hip
    return unet_hip.UNetRuntime.get(DEV)


def _dev(a, offset=0):
    """`a` on the device; offset = 1: in a view that starts one float past a 16-byte boundary."""
    a = torch.from_numpy(np.ascontiguousarray(a))
    if not offset:
        d = a.to(DEV)
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.empty(a.numel() + 8, dtype=a.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    d = buf[offset:offset + a.numel()].view(a.shape)
    d.copy_(a)
    assert d.data_ptr() % 16 == 4 * offset and d.is_contiguous()
    return d


def _bar(yard):
    return max(4 * yard, FLOOR)


def _check(tag, got_l, got_g, x, t, w, abg, worst):
    """Losses and every element of dlogits vs the fp64 reference at the measured bar; the two
    elements at every sample boundary individually."""
    ref_l, ref_g = L.losses(x, t, *abg), L.dlogits(x, t, w, *abg)
    y_l, y_g = L.torch_losses_and_grad(x, t, w, *abg, dtype=torch.float32)
    e_l, ey_l = np.abs(got_l - ref_l), np.abs(y_l - ref_l)
    e_g, ey_g = L.sample_rel_err(got_g, ref_g), L.sample_rel_err(y_g, ref_g)
    print(f"{tag} abg {abg} w {w}: losses dev {e_l.max():.2e} / torch32 {ey_l.max():.2e}; "
          f"dlogits dev {e_g.max():.2e} / torch32 {ey_g.max():.2e}")
    worst["dl"], worst["yl"] = max(worst["dl"], e_l.max()), max(worst["yl"], ey_l.max())
    worst["dg"], worst["yg"] = max(worst["dg"], e_g.max()), max(worst["yg"], ey_g.max())
    assert np.all(np.isfinite(got_l)) and np.all(np.isfinite(got_g)), tag
    for k, name in enumerate(("bce", "dice", "focal")):
        assert e_l[k] <= _bar(ey_l[k]), f"{tag} {abg}: {name} {e_l[k]:.3e} (torch fp32 {ey_l[k]:.3e})"
    N = x.shape[0]
    per = x[0].size
    for n in range(N):
        assert e_g[n] <= _bar(ey_g[n]), \
            f"{tag} {abg} {w}: sample {n} dlogits {e_g[n]:.3e} (torch fp32 {ey_g[n]:.3e})"
    gf, rf = np.asarray(got_g, np.float64).reshape(-1), ref_g.reshape(-1)
    scale = np.abs(ref_g).reshape(N, -1).max(1)
    for n in range(1, N):  # elements per - 1 and per of the flattened batch, at every boundary
        for i in (n * per - 1, n * per):
            s = i // per
            assert abs(gf[i] - rf[i]) / scale[s] <= _bar(ey_g[s]), f"{tag}: boundary element {i}"


@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("shape,offset", SHAPES)
def test_loss_kernels_vs_fp64(shape, offset, kind):
    rt = _rt()
    x, t = L.make_case(shape, kind)
    xd, td = _dev(x, offset), _dev(t, offset)
    stats, sums = rt.loss_stats(xd, td)
    stats2, sums2 = rt.loss_stats(xd, td)
    assert torch.equal(stats, stats2) and torch.equal(sums, sums2), "loss_stats is not repeatable"
    worst = dict(dl=0.0, yl=0.0, dg=0.0, yg=0.0)
    tag = f"{shape}{'+4B' if offset else ''} {kind}"
    for abg in L.ABG:
        losses = rt.loss_finalize(sums, *abg).cpu().double().numpy()
        for w in L.WEIGHTS:
            wd = torch.tensor(w, dtype=torch.float32, device=DEV)
            d = rt.loss_bwd(xd, td, stats, sums, wd, *abg)
            _check(tag, losses, d.cpu().numpy(), x, t, w, abg, worst)
    print(f"WORST {tag}: losses dev {worst['dl']:.2e} torch32 {worst['yl']:.2e}; dlogits dev "
          f"{worst['dg']:.2e} torch32 {worst['yg']:.2e}")


@pytest.mark.parametrize("shape", [(5, 1, 128, 128), (5, 3, 17, 19)])
def test_two_phase_shards_on_one_gpu(shape):
    """unet_loss_stats per shard -> sum of `sums` -> unet_loss_finalize -> unet_loss_bwd per shard
    (what two ranks do around their all-reduce), on a batch of 5 split 2 + 3: the per-sample
    statistics are bit-equal to the whole batch's (the chunk count depends on the sample size
    only), and losses and dlogits are those of the whole batch."""
    rt = _rt()
    x, t = L.make_case(shape, "soft", seed=2)
    xd, td = _dev(x), _dev(t)
    stats, sums = rt.loss_stats(xd, td)
    parts = [(xd[:2].contiguous(), td[:2].contiguous()), (xd[2:].contiguous(), td[2:].contiguous())]
    sh = [rt.loss_stats(a, b) for a, b in parts]
    assert torch.equal(torch.cat([s[0] for s in sh]), stats), "per-sample stats depend on the batch"
    tot = sh[0][1] + sh[1][1]  # the all-reduce, on the device
    assert tot[5].item() == 5 and tot[6].item() == x.size
    worst = dict(dl=0.0, yl=0.0, dg=0.0, yg=0.0)
    for abg in (L.ABG[0], L.ABG[1]):
        w = L.WEIGHTS[0]
        wd = torch.tensor(w, dtype=torch.float32, device=DEV)
        whole_l = rt.loss_finalize(sums, *abg).cpu().double().numpy()
        whole_g = rt.loss_bwd(xd, td, stats, sums, wd, *abg).cpu().numpy()
        got_l = rt.loss_finalize(tot, *abg).cpu().double().numpy()
        got_g = torch.cat([rt.loss_bwd(a, b, s[0], tot, wd, *abg) for (a, b), s in zip(parts, sh)])
        got_g = got_g.cpu().numpy()
        _check(f"{shape} shards", got_l, got_g, x, t, w, abg, worst)
        _check(f"{shape} whole", whole_l, whole_g, x, t, w, abg, worst)
        # shards vs whole batch: the double sums associate differently, so not bit-equal
        y_g = L.torch_losses_and_grad(x, t, w, *abg, dtype=torch.float32)[1]
        ey = L.sample_rel_err(y_g, L.dlogits(x, t, w, *abg))
        e = L.sample_rel_err(got_g, whole_g.astype(np.float64))
        for n in range(shape[0]):
            assert e[n] <= _bar(ey[n]), f"sample {n}: shards vs whole {e[n]:.3e}"
