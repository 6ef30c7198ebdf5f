"""GPU: BoundaryLoss on the device -- the distance transform kernels bit for bit against scipy
and the host hook, the loss / dlogits kernels against torch fp32 ops over scipy's distance maps
(the bars of test_gpu_parity.py::test_losses_and_grads_vs_torch), and the module / trainer
wiring with scipy's transform patched out."""
import functools
import os

import numpy as np
import pytest
import scipy.ndimage as nd
import torch

from _helpers import norm_rel
from test_edt_cpu import SHAPES, edt_host, masks, scipy_dist

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(targets, scipy's dist) of a shape, computed once and never modified."""
    t = masks(*shape, seed=shape[0] * 1000 + shape[1])
    if shape == (512, 512):
        t = t[:4]
    return t, scipy_dist(t)


def _torch_boundary(x, t, dist):
    """The reference's expression (models/loss.py:52-66) in torch fp32 ops."""
    per = (torch.abs(torch.sigmoid(x[:, 0]) - t[:, 0]) * dist[:, 0]).flatten(1).mean(1)
    return per.mean()


def _no_scipy(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("scipy.ndimage.distance_transform_edt called on the device path")
    monkeypatch.setattr(nd, "distance_transform_edt", boom)


def _soft_case(seed=7, shape=(2, 1, 97, 101)):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g) * 3
    t = torch.rand(*shape, generator=g)  # soft targets: no site by themselves
    t[0, 0, 20:50, 30:70] = 1.0  # sample 0 has sites, sample 1 follows the empty-mask rule
    t[0, 0, 80:90, 5:9] = 1.5
    return x, t


# (333 > the row pass's 256-thread block: its threads loop)
@pytest.mark.parametrize("shape", SHAPES + [(512, 512)])
def test_distance_maps_bit_equal(shape):
    import unet_hip
    t, want = _case(shape)
    got = unet_hip.distance_maps(torch.from_numpy(t).to(DEV)).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(got, want)
    assert np.array_equal(got, edt_host(t))


def test_distance_maps_channels_site_rule_and_all_ones():
    import unet_hip
    r = np.random.default_rng(2)
    t = (r.random((3, 2, 24, 40)) < 0.1).astype(np.float32)
    t[1, 0] = 0
    t[2, 0, 3, :6] = [0.5, 0.9999999, 1.0, 1.5, 2.0, 255.0]
    got = unet_hip.distance_maps(torch.from_numpy(t).to(DEV)).cpu().numpy()
    assert np.array_equal(got, scipy_dist(t))
    ones = torch.ones(2, 1, 16, 24, device=DEV)
    assert not unet_hip.distance_maps(ones).any()


def test_size_limit_on_device():
    import unet_hip
    with pytest.raises(unet_hip.HipError):
        unet_hip.distance_maps(torch.zeros(1, 1, 1, 2049, device=DEV))


def _check(x, t, dist, want_loss=None, want_grad=None):
    import unet_hip
    xd, td, dd = x.to(DEV), t.to(DEV), torch.as_tensor(dist).to(DEV)
    xr = xd.clone().requires_grad_(True)
    ref = _torch_boundary(xr, td, dd)
    (1.7 * ref).backward()
    xh = xd.clone().requires_grad_(True)
    loss = unet_hip.boundary_loss(xh, td)
    (1.7 * loss).backward()
    print(f"loss {loss.item():.9g} vs torch {ref.item():.9g}; grad norm_rel "
          f"{norm_rel(xh.grad.cpu(), xr.grad.cpu()):.3e}")
    assert loss.shape == ()
    assert torch.allclose(loss.detach(), ref.detach(), rtol=1e-5, atol=1e-6), (loss, ref)
    assert norm_rel(xh.grad.cpu(), xr.grad.cpu()) <= 1e-4
    if want_loss is not None:
        assert np.allclose(loss.item(), want_loss, rtol=1e-5, atol=1e-6), (loss.item(), want_loss)
        assert norm_rel(xh.grad.cpu() / 1.7, want_grad) <= 1e-4
    return xh.grad


def test_loss_and_grad_vs_torch_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "boundary_32.npz"))
    x, t = torch.from_numpy(z["x"]), torch.from_numpy(z["t"])
    _check(x, t, scipy_dist(z["t"]), float(z["loss"]), torch.from_numpy(z["dlogits"]))


def test_loss_and_grad_vs_torch_soft_odd():
    x, t = _soft_case()
    _check(x, t, scipy_dist(t.numpy()))


def test_sign_zero_and_other_channels():
    """p == t exactly -> gradient 0 (torch's abs backward); channels 1.. get zero gradient."""
    import unet_hip
    x = torch.zeros(2, 3, 8, 12, device=DEV)
    t = torch.full((2, 3, 8, 12), 0.5, device=DEV)
    t[0, 0, 2, 3] = 1.0
    x[0, 0, 5, 5] = 2.0
    xh = x.clone().requires_grad_(True)
    unet_hip.boundary_loss(xh, t).backward()
    g = xh.grad
    assert not g[:, 1:].any()
    assert g[0, 0, 5, 5] > 0 and g[0, 0, 2, 3] == 0 and g[0, 0, 0, 0] == 0
    xr = x.clone().requires_grad_(True)
    _torch_boundary(xr, t, torch.from_numpy(scipy_dist(t.cpu().numpy())).to(DEV)).backward()
    assert norm_rel(g.cpu(), xr.grad.cpu()) <= 1e-4


def test_module_uses_the_device_path(monkeypatch):
    from models.loss import BoundaryLoss, _distance_maps
    x, t = _soft_case()
    dist = scipy_dist(t.numpy())
    xd, td = x.to(DEV), t.to(DEV)
    want = _torch_boundary(xd, td, torch.from_numpy(dist).to(DEV))
    _no_scipy(monkeypatch)
    got = BoundaryLoss()(xd, td)
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-6), (got, want)
    assert np.array_equal(_distance_maps(td).cpu().numpy(), dist)


def test_composite_loss_backward(monkeypatch):
    from models.loss import CompositeLoss
    x, t = _soft_case(seed=9)
    dist = torch.from_numpy(scipy_dist(t.numpy())).to(DEV)
    xd, td = x.to(DEV), t.to(DEV)
    xr = xd.clone().requires_grad_(True)
    pr = torch.sigmoid(xr)
    TP, FP, FN = (pr * td).sum(), (pr * (1 - td)).sum(), ((1 - pr) * td).sum()
    ti = (TP + 1e-6) / (TP + 0.3 * FP + 0.7 * FN + 1e-6)
    ref = 1.0 * (1 - ti) ** 0.75 + 0.5 * _torch_boundary(xr, td, dist)
    ref.backward()
    _no_scipy(monkeypatch)
    xh = xd.clone().requires_grad_(True)
    loss = CompositeLoss()(xh, td)
    loss.backward()
    print(f"composite {loss.item():.9g} vs {ref.item():.9g}; grad "
          f"{norm_rel(xh.grad.cpu(), xr.grad.cpu()):.3e}")
    assert torch.allclose(loss.detach(), ref.detach(), rtol=1e-5, atol=1e-6), (loss, ref)
    assert norm_rel(xh.grad.cpu(), xr.grad.cpu()) <= 1e-4


def _run(x, t, dist=None):
    import unet_hip
    xh = x.clone().requires_grad_(True)
    loss = unet_hip.boundary_loss(xh, t, dist=dist)
    loss.backward()
    return loss.detach(), xh.grad


def test_deterministic_stream_and_precomputed_dist():
    import unet_hip
    x, t = (a.to(DEV) for a in _soft_case(seed=11))
    l0, g0 = _run(x, t)
    l1, g1 = _run(x, t)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    # a precomputed distance map skips the transform and changes no bit
    l2, g2 = _run(x, t, dist=unet_hip.distance_maps(t))
    assert torch.equal(l0, l2) and torch.equal(g0, g2)
    # a non-default stream
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        l3, g3 = _run(x, t)
    torch.cuda.current_stream(DEV).wait_stream(s)
    assert torch.equal(l0, l3) and torch.equal(g0, g3)


class _HostBoundary(torch.nn.Module):
    """The reference's host path: scipy's transform, torch ops (models/loss.py:48-66)."""

    def forward(self, logits, targets):
        dist = torch.from_numpy(scipy_dist(targets.detach().cpu().numpy())).to(logits.device)
        return _torch_boundary(logits, targets, dist)


def test_trainer_step_with_boundary_term(tmp_path, monkeypatch):
    """One Trainer step with boundary_ratio = 0.5 on the device path (scipy patched out) == the
    same step of a second Trainer whose boundary term is the host path, on a copy of the model
    (loss and updated parameters, the bars of test_trainer_step_matches_oracle)."""
    from _helpers import inputs
    from models.model import UNet
    from oracle import unet_ref_cpu as O
    from test_gpu_trainer import _config
    from utils.trainer import Trainer
    from utils.utils import create_logger
    x, t = inputs(1, 2, 64, 64)
    P = O.make_params(42)

    def step(name, host):
        cfg = _config(tmp_path / name, use_mixup=False, focal_ratio=0.0, lr=1e-5, boundary_ratio=0.5)
        model = UNet()
        model.load_state_dict({**P, **O.init_buffers()})
        tr = Trainer(cfg, ([(x, t)], [(x, t)], [(x, t)]),
                     create_logger(os.path.join(cfg.log_dir, "s.log")), model)
        if host:
            tr.criterion_boundary = _HostBoundary()
        loss = tr.train_one_epoch(0)
        return loss, {k: v.detach().cpu().clone() for k, v in tr.model.named_parameters()}

    loss_h, p_h = step("host", True)
    _no_scipy(monkeypatch)
    loss_d, p_d = step("dev", False)
    worst = max(float((p_d[k] - v).abs().max()) for k, v in p_h.items())
    print(f"loss {loss_d:.9g} vs host path {loss_h:.9g}; worst parameter difference {worst:.3e}")
    assert abs(loss_d - loss_h) < 1e-5
    assert worst <= 4e-5
    moved = max(float((p_d[k] - v).abs().max()) for k, v in P.items())
    assert moved > 0
