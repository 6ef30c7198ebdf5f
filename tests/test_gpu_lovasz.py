"""GPU: the Lovasz hinge loss on the device -- the stable segmented radix sort's permutation exactly
against the NumPy restatement (tests/lovasz_ref.py), gmap bit for bit against the restatement and the
host twin, the loss within the float64 bar derived there, dlogits bit for bit, and the wiring: autograd,
the refusals, scratch growth, the Trainer term and two data-parallel ranks."""
import ctypes
import os

import numpy as np
import pytest
import torch

import lovasz_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# a plane smaller than one wave; odd, five tiles with a ragged last one; C > 1 and exact multiples of
# the 2048-element tile; one long row of prime length
SHAPES = [(1, 1, 5, 7), (2, 1, 97, 101), (3, 2, 64, 64), (1, 1, 1, 4099)]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _parts(x, t, want_perm=True):
    import unet_hip
    out = unet_hip.lovasz_hinge_parts(_dev(x), _dev(t), want_perm)
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_loss(got, ref, shape):
    """The device's float64 sum is within M 2^-52 sum |terms| of the restatement's (both are sums of
    the same correctly rounded products in different orders), and its float32 loss is that sum over
    N C rounded once: equal to the restatement's, or one float32 ulp off where the two double sums
    straddle a rounding boundary -- the assertion allows that one ulp and no more."""
    planes, M = shape[0] * shape[1], shape[2] * shape[3]
    if not np.isfinite(ref["sum"]):  # the inf kind: +inf errors with positive weights
        assert got["sum"][0] == ref["sum"] and float(got["loss"]) == float(ref["loss"])
        return
    bar = R.sum_bar(ref, M)
    print(f"sum {got['sum'][0]:.17g} vs {ref['sum']:.17g} (bar {bar:.3e}); loss {float(got['loss']):.9g} "
          f"vs {float(ref['loss']):.9g}")
    assert abs(got["sum"][0] - ref["sum"]) <= bar
    assert np.float32(got["loss"]) == np.float32(got["sum"][0] / planes)
    assert abs(float(got["loss"]) - float(ref["loss"])) <= np.spacing(np.float32(abs(ref["loss"])))


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_sort_weights_loss_and_gradient(shape, kind):
    import unet_hip
    x, t, ref = R.case(shape, kind)
    planes, M = shape[0] * shape[1], shape[2] * shape[3]
    got = _parts(x, t)
    # the permutation: `constant` and `ties` are the kinds an unstable scatter fails
    assert np.array_equal(got["perm"].reshape(planes, M).astype(np.int64), ref["perm"])
    assert np.array_equal(_bits(got["gmap"]), _bits(ref["gmap"]))
    host = unet_hip.lovasz_hinge_host(torch.from_numpy(np.array(x)), torch.from_numpy(np.array(t)), True)
    assert np.array_equal(_bits(got["gmap"]), _bits(host["gmap"].numpy()))
    assert np.array_equal(got["perm"], host["perm"].numpy())
    _check_loss(got, ref, shape)
    # without the permutation output: the same bits
    again = _parts(x, t, want_perm=False)
    assert again["perm"] is None
    assert np.array_equal(_bits(again["gmap"]), _bits(got["gmap"]))
    assert again["sum"].tobytes() == got["sum"].tobytes() and again["loss"].tobytes() == got["loss"].tobytes()
    # dlogits: ((w * -s) * gmap) / (N C) in float32, in this order, bit for bit
    w = 1.7
    rt = unet_hip.UNetRuntime.get(DEV)
    d = rt.lovasz_bwd(_dev(x), _dev(t), _dev(got["gmap"]), torch.tensor([w], device=DEV)).cpu().numpy()
    want = R.reference(x, t, w)["dlogits"]
    assert np.array_equal(_bits(d), _bits(want))
    if kind == "signed_zero":  # e == 0 is inactive: relu'(0) = 0
        assert not d[ref["e"] == 0].any() and (ref["e"] == 0).sum() > x.size // 4
    if kind == "confident":
        assert (ref["e"] <= 0).mean() >= 0.95


def test_two_shapes_in_a_row_grow_the_scratch_and_runs_repeat():
    """A small call, then a larger one on the same context with the first still in flight (the
    scratch is outgrown and retired, not freed), then the small one again; nothing is read back until
    all three are enqueued.  The repeated call gives the same bits: every sum has a fixed order."""
    import unet_hip
    small, large = (1, 1, 5, 7), (4, 2, 97, 101)
    xs, ts, rs = R.case(small, "ties")
    xl, tl, rl = R.case(large, "ties")
    a = unet_hip.lovasz_hinge_parts(_dev(xs), _dev(ts), True)
    b = unet_hip.lovasz_hinge_parts(_dev(xl), _dev(tl), True)
    c = unet_hip.lovasz_hinge_parts(_dev(xs), _dev(ts), True)
    d = unet_hip.lovasz_hinge_parts(_dev(xl), _dev(tl), True)
    torch.cuda.synchronize()
    for got, ref, shape in ((a, rs, small), (b, rl, large)):
        assert np.array_equal(got["perm"].cpu().numpy().reshape(ref["perm"].shape), ref["perm"])
        assert np.array_equal(_bits(got["gmap"].cpu().numpy()), _bits(ref["gmap"]))
    for p, q in ((a, c), (b, d)):
        for k in ("perm", "gmap", "sum", "loss"):
            assert torch.equal(p[k].reshape(-1).view(torch.uint8), q[k].reshape(-1).view(torch.uint8)), k


def test_nan_logit_gives_nan_loss_and_indices_stay_inside():
    x, t = (a.copy() for a in R.make_case((2, 1, 97, 101), "random"))
    x[1, 0, 40, 50] = np.nan
    x[0, 0, 3, 3] = -np.nan
    got = _parts(x, t)
    M = 97 * 101
    assert np.isnan(got["loss"]) and np.isnan(got["sum"][0])
    perm = got["perm"].reshape(2, M)
    assert perm.min() >= 0 and perm.max() < M
    for p in perm:  # still a permutation of the plane
        assert np.array_equal(np.sort(p), np.arange(M))


def test_autograd_against_the_float64_composition():
    """lovasz_hinge and its backward against Berman's formula in float64 torch on tie-free input whose
    errors are exact in float32: the loss within the float64 bar plus one float32 rounding, the
    gradient within 2^-23 |g| per element (gmap's rounding to float32 and the division by N C)."""
    import unet_hip
    shape = (2, 2, 37, 41)
    x, t, ref = R.case(shape, "exact")
    want, xd = R.berman_torch(x, t)
    want.backward()
    xh = _dev(x).requires_grad_(True)
    loss = unet_hip.lovasz_hinge(xh, _dev(t))
    assert loss.shape == () and loss.dtype == torch.float32
    loss.backward()
    bar = R.sum_bar(ref, 37 * 41) / 4 + 2.0 ** -24 * abs(want.item())
    print(f"loss {loss.item():.9g} vs float64 {want.item():.17g} (bar {bar:.3e})")
    assert abs(loss.item() - want.item()) <= bar
    g, gw = xh.grad.cpu().numpy().astype(np.float64), xd.grad.numpy()
    assert np.all(np.abs(g - gw) <= 2.0 ** -23 * np.abs(gw))
    assert (gw != 0).mean() > 0.3
    # the module and the composite term ride the same function
    from models.loss import CompositeLoss, LovaszHingeLoss
    assert torch.equal(LovaszHingeLoss()(_dev(x), _dev(t)), loss.detach())
    td = _dev(t)
    base, with_l = CompositeLoss()(_dev(x), td), CompositeLoss(λ_lovasz=0.25)(_dev(x), td)
    assert abs((with_l - base).item() - 0.25 * loss.item()) <= 4 * 2.0 ** -24 * (abs(with_l.item()) + abs(base.item()))


def test_cpu_tensor_is_refused():
    import unet_hip
    x = torch.zeros(1, 1, 4, 4)
    with pytest.raises(unet_hip.HipUnavailable):
        unet_hip.lovasz_hinge(x, x)
    with pytest.raises(ValueError):
        unet_hip.lovasz_hinge(x.to(DEV), torch.zeros(1, 1, 4, 5, device=DEV))


def test_plane_above_2_24_is_refused_by_shape_alone():
    """The shape check precedes every access and the scratch: a 4-float dummy passes for a
    4097 x 4096 plane through the raw binding, forward and backward; nothing large is allocated."""
    import unet_hip
    from unet_hip import _lib
    rt = unet_hip.UNetRuntime.get(DEV)
    a = torch.zeros(4, device=DEV)
    s = torch.zeros(1, dtype=torch.float64, device=DEV)
    before = torch.cuda.memory_allocated(DEV)
    rc = rt.lib.unet_lovasz_fwd(rt.ctx, _lib.ptr(a), _lib.ptr(a), 1, 1, 4097, 4096, _lib.ptr(a), None,
                                _lib.ptr(s), _lib.ptr(a), _lib.stream_ptr(DEV))
    assert rc == -2 and b"2^24" in rt.lib.unet_last_error(rt.ctx)
    rc = rt.lib.unet_lovasz_bwd(rt.ctx, _lib.ptr(a), _lib.ptr(a), _lib.ptr(a), 1, 1, 4097, 4096, _lib.ptr(a),
                                _lib.ptr(a), _lib.stream_ptr(DEV))
    assert rc == -2
    assert torch.cuda.memory_allocated(DEV) == before
    h = np.zeros(4, np.float32)
    p = h.ctypes.data_as(ctypes.c_void_p)
    assert rt.lib.unet_lovasz_host(p, p, 1, 1, 4097, 4096, p, None, p, p) == -2


# ---------------------------------------------------------------- Trainer
def _epoch(tmp, name, ratio):
    """One epoch over one synthetic 64^2 batch from fixed parameters -> (meter averages, parameters, log)."""
    from _helpers import inputs
    from models.model import UNet
    from oracle import unet_ref_cpu as O
    from test_gpu_trainer import _config
    from utils.trainer import Trainer
    from utils.utils import create_logger
    x, t = inputs(1, 2, 64, 64)
    kw = dict(use_mixup=False, focal_ratio=0.0, lr=1e-5)
    if ratio is not None:
        kw["lovasz_ratio"] = ratio
    cfg = _config(tmp / name, **kw)
    model = UNet()
    model.load_state_dict({**O.make_params(42), **O.init_buffers()})
    log = os.path.join(cfg.log_dir, "s.log")
    tr = Trainer(cfg, ([(x, t)], [(x, t)], [(x, t)]), create_logger(log), model)
    seen = []
    log_epoch = tr._log_epoch
    tr._log_epoch = lambda tag, epoch, meters, counts: (seen.append([m.avg for m in meters]),
                                                       log_epoch(tag, epoch, meters, counts))[1]
    tr.train_one_epoch(0)
    tr.validate(0)
    with open(log) as f:
        text = f.read()
    return seen, {k: v.detach().cpu().clone() for k, v in tr.model.named_parameters()}, text


def test_trainer_epoch_with_the_lovasz_term(tmp_path):
    """lovasz_ratio = 0.5: a sixth meter, the logged total = sum ratio * loss (float32 sums of at most
    four terms: 8 float32 ulps of the terms' magnitudes), "Lovasz Loss" in the log, parameters that
    differ from the ratio-0 run; ratio 0 and a config without the field log the same lines."""
    on, p_on, log_on = _epoch(tmp_path, "on", 0.5)
    off, p_off, log_off = _epoch(tmp_path, "off", 0.0)
    none, p_none, log_none = _epoch(tmp_path, "none", None)
    for bce, dice, focal, bnd, tot, lov in on:  # train, validate
        mag = abs(bce) + abs(dice) + 0.5 * abs(lov)
        print(f"total {tot:.9g} vs {bce + dice + 0.5 * lov:.9g}; lovasz {lov:.6g}")
        assert lov > 0 and abs(tot - (bce + dice + 0.5 * lov)) <= 8 * 2.0 ** -24 * mag
    assert all(len(m) == 5 for m in off + none)
    assert log_on.count("Lovasz Loss: ") == 2 and "Lovasz Loss" not in log_off + log_none
    strip = lambda text: [ln.split(" - ", 1)[-1] for ln in text.splitlines() if "Loss" in ln or "IoU" in ln]
    assert strip(log_off) == strip(log_none)
    assert all(torch.equal(p_off[k], p_none[k]) for k in p_off)
    assert max(float((p_on[k] - p_off[k]).abs().max()) for k in p_on) > 0


# ---------------------------------------------------------------- two data-parallel ranks
DP_SHARDS = {"3+1": (3, 1), "1+empty": (1, 0)}
DP_RATIOS = dict(bce_ratio=0.0, dice_ratio=0.0, focal_ratio=0.0, boundary_ratio=0.0, lovasz_ratio=1.0)
DP_SHAPE = (37, 41)


def _dp_body(rank, world, tmp):
    from test_gpu_dist_eval import _trainer
    tr, _ = _trainer(rank, world, tmp, ((2, 0), (2, 1), (2, 2)), 2, **DP_RATIOS)
    assert tr._extra_reduces() == 2
    out = {}
    for name, split in DP_SHARDS.items():
        lo, n = sum(split[:rank]), split[rank]
        x, t, _ = R.case((sum(split), 1) + DP_SHAPE, "random")
        for grad in (False, True):
            if n == 0:  # the empty shard joins the step's collectives as _run_epoch does
                if grad:
                    tr.optimizer.zero_grad(set_to_none=True)
                    tr.ddp.empty_step(tr._extra_reduces())
                else:
                    tr.ddp.empty_losses(tr._extra_reduces())
                continue
            xs = torch.from_numpy(np.array(x[lo:lo + n])).to(DEV).requires_grad_(grad)
            with torch.set_grad_enabled(grad):
                loss, l, lb, total = tr._losses(xs, torch.from_numpy(np.array(t[lo:lo + n])).to(DEV))
            if grad:
                loss.backward()
                if 0 in split:  # the gradient buckets empty_step() sums on the other rank
                    tr.ddp.reducer.reduce(torch.zeros_like(tr.model._state.param_arena), wait_native=False)
            out[name, grad] = dict(lovasz=float(tr._lovasz.double()), total=float(total.double()),
                                   grad=xs.grad.cpu().numpy() if grad else None)
    return out


@pytest.mark.timeout(300)
def test_two_ranks_sum_to_the_gathered_batch(tmp_path):
    """Trainer._losses with lovasz_ratio = 1 and the other ratios 0 on two ranks (gloo, both on one
    GPU): on a ragged 3 + 1 split each rank's logits.grad is its slice of the 4-sample batch's
    gradient (the restatement's dlogits; the device forms (w n_local / n_global) g / (n_local C) where
    the restatement forms w g / (n_global C): at most three float32 roundings against one, 2^-22 |g|
    per element), the reported value is the gathered batch's on both ranks, and a rank with an empty
    shard joins the same collectives (the workers' process group times out instead of hanging)."""
    from test_gpu_dist_eval import _spawn
    r0, r1 = _spawn(_dp_body, str(tmp_path))
    for name, split in DP_SHARDS.items():
        N = sum(split)
        x, t, ref = R.case((N, 1) + DP_SHAPE, "random")
        for grad in (False, True):
            a = r0[name, grad]
            if split[1]:
                assert a["lovasz"] == r1[name, grad]["lovasz"] and a["total"] == r1[name, grad]["total"]
            else:
                assert (name, grad) not in r1
            print(f"{name} grad={grad}: lovasz {a['lovasz']:.9g} vs {float(ref['loss']):.9g}")
            # each rank's float32 mean times its float32 share, added in float32, against one rounding
            # of the restatement's: four roundings of positive terms, 2^-22 of the loss
            assert abs(a["lovasz"] - float(ref["loss"])) <= 2.0 ** -22 * abs(float(ref["loss"]))
            assert a["total"] == a["lovasz"]
        for rank, res in enumerate((r0, r1)):
            lo, n = sum(split[:rank]), split[rank]
            if n:
                got, want = res[name, True]["grad"].astype(np.float64), ref["dlogits"][lo:lo + n].astype(np.float64)
                assert np.all(np.abs(got - want) <= 2.0 ** -22 * np.abs(want)), (name, rank)
                assert (want != 0).any()
