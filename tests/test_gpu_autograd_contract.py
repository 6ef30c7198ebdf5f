"""The autograd contract of the HIP modules (unet_hip.UNet / ModUNet / ResUNet) beyond the
Trainer's one pattern: the model applied twice in one graph, gradient accumulation, both
zero_grad forms, kept .grad references, a retained graph, no-grad and eval forwards in between,
non-contiguous and float64 inputs, non-contiguous incoming gradients, partly used seg_losses,
inputs that require grad, and copies (copy.deepcopy, pickle) of a model that has run.

Two judges:

* bit for bit against the HIP path's own plain steps.  BN running buffers do not enter a
  training forward, so with the same parameters the gradient of loss(m(x1)) + loss(m(x2)) is
  exactly g1 + g2 in torch float32, g1 and g2 from two one-forward steps (computed once per
  network, _singles);
* once per network against the fp64 oracle: the joint gradient against the sum of the oracle's
  fp64 gradients over x1 and x2, by the method and bars of
  tests/test_gpu_kernel_coverage.py::_check_f32 (2x the fp32 oracle's own deviation over x and
  x (1 + 1e-7), floor GRAD_TOL); running statistics at the bars of
  tests/test_gpu_mod.py::test_mod_narrow_full_grads_vs_fp64.

Networks: models/model.py UNet (unpadded: HipAdamW's fused unet_adamw_repack) and ResUNet(16, 3)
(channels padded to 32 inside the library: the plain unet_adamw).  x1 is 2x64x64, x2 1x32x96:
two workspaces and plans.  The oracle runs before the first GPU call of a network's tests.
"""
import copy
import os
import pickle

import numpy as np
import pytest
import torch

import loss_ref as L
import test_gpu_loss_edges as TL
from _helpers import hip_model, inputs, norm_rel
from oracle import mod_ref_cpu as MO
from oracle import unet_ref_cpu as O
from test_gpu_kernel_coverage import GRAD_TOL

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NETS = ["unet", "res16"]
LR = 1e-3
_REF = {}
_SINGLES = {}


@pytest.fixture(autouse=True, scope="module")
def _threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def _to64(d):
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in d.items()}


def _oracle(net):
    if net == "unet":
        return (O.make_params(7), O.init_buffers,
                lambda P, B, x, t: O.train_step(P, B, None, x, t))
    return (MO.res_make_params(7, 16, 3), lambda: MO.res_init_buffers(16, 3),
            lambda P, B, x, t: MO.res_train_step(P, B, None, x, t, depth=3))


def _batches():
    return [inputs(33, 2, 64, 64), inputs(34, 1, 32, 96)]


def _ref(net):
    """Once per network, on the CPU: the parameters, the fp64 gradient sum over x1 and x2, the
    fp32 oracle's own deviation from it (over x and x (1 + 1e-7)) and the BN buffers after the
    train-mode forwards of x1 then x2."""
    if net not in _REF:
        P, bufs, ts = _oracle(net)
        B32 = bufs()
        g64, g32, g32p = {}, {}, {}
        for x, t in _batches():
            r32 = ts(P, B32, x, t)  # B32 advances over x1, then x2
            r32p = ts(P, bufs(), x * (1 + 1e-7), t)
            r64 = ts(_to64(P), _to64(bufs()), x.double(), t.double())
            for acc, r in ((g64, r64), (g32, r32), (g32p, r32p)):
                for k, g in r["grads"].items():
                    acc[k] = g.clone() if k not in acc else acc[k] + g
        e32 = {k: max(norm_rel(g32[k], g64[k]), norm_rel(g32p[k], g64[k])) for k in g64}
        _REF[net] = dict(P=P, bufs=bufs, g64=g64, e32=e32, B=B32)
    return _REF[net]


def _model(net):
    import unet_hip
    r = _ref(net)
    if net == "unet":
        return hip_model(r["P"], DEV, r["bufs"]())
    m = unet_hip.ResUNet(1, 1, base_filters=16, depth=3)
    sd = m.state_dict()
    for k, v in list(r["P"].items()) + list(r["bufs"]().items()):
        sd[k] = v.clone()
    m.load_state_dict(sd)
    return m.to(DEV).train()


def _dev_batches():
    return [(x.to(DEV), t.to(DEV)) for x, t in _batches()]


def _loss(m, x, t):
    import unet_hip
    logits = m(x)
    l = unet_hip.seg_losses(logits, t)
    return logits, l[0] + l[1]


def _zero(m, set_to_none=True):
    for p in m.parameters():
        if set_to_none:
            p.grad = None
        elif p.grad is not None:
            p.grad.zero_()


def _flat(m):
    return torch.cat([p.grad.detach().reshape(-1) for p in m.parameters()]).clone()


def _params(m):
    return torch.cat([p.detach().reshape(-1) for p in m.parameters()]).clone()


def _plain_step(m, x, t):
    """zero_grad(set_to_none=True) -> forward -> backward: (logits, flat gradient)."""
    _zero(m)
    logits, loss = _loss(m, x, t)
    loss.backward()
    return logits.detach().clone(), _flat(m)


def _singles(net):
    """Once per network: logits and gradients of the plain one-forward steps of x1 and x2 on a
    fresh model -- the bit-for-bit reference of every case (no optimizer step: the parameters
    are those of every other fresh model)."""
    if net not in _SINGLES:
        m = _model(net)
        _SINGLES[net] = [_plain_step(m, x, t) for x, t in _dev_batches()]
    return _SINGLES[net]


def _check_buffers(m, net, steps):
    Bref = _ref(net)["B"]
    for k, v in m.named_buffers():
        if v.is_floating_point():
            np.testing.assert_allclose(v.cpu().numpy(), Bref[k].numpy(), rtol=1e-4, atol=1e-5, err_msg=k)
        else:
            assert int(v) == steps == int(Bref[k]), k


def _assert_flat(m, at_state_arena):
    from unet_hip.optim import _flat_base
    st = m.flatten_()
    flat = _flat_base([p.grad for p in m.parameters()])
    assert flat is not None, "the .grad tensors are not one flat arena"
    assert flat.numel() == st.param_arena.numel()
    for p, off, shape in st.params:
        assert p.grad.data_ptr() == flat.data_ptr() + 4 * off and p.grad.shape == p.shape
    if at_state_arena:
        assert flat.data_ptr() == st.grad_arena.data_ptr()


# ------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("net", NETS)
def test_two_forwards_one_backward(net):
    """(a) loss(m(x1)) + loss(m(x2)), one backward: bit-equal to g1 + g2 of the plain steps, and
    within the fp32 oracle's envelope of the fp64 oracle's gradient sum; the running statistics
    after the two forwards are the oracle's over x1 then x2."""
    r = _ref(net)
    (l1, g1), (l2, g2) = _singles(net)
    (x1, t1), (x2, t2) = _dev_batches()
    m = _model(net)
    a1, loss1 = _loss(m, x1, t1)
    a2, loss2 = _loss(m, x2, t2)
    (loss1 + loss2).backward()
    _check_buffers(m, net, 2)
    got = _flat(m)
    assert torch.equal(a1.detach(), l1) and torch.equal(a2.detach(), l2)
    d = float((got - (g1 + g2)).double().norm() / (g1 + g2).double().norm())
    named = dict(m.named_parameters())
    errs = {k: norm_rel(named[k].grad.detach().cpu(), v) for k, v in r["g64"].items()}
    worst = max(errs, key=errs.get)
    env = max(2 * max(r["e32"].values()), GRAD_TOL)
    print(f"{net}: joint vs g1 + g2 norm-rel {d:.2e}; vs fp64 sum worst grad {worst} "
          f"{errs[worst]:.2e} (fp32 oracle {r['e32'][worst]:.2e}, envelope {env:.2e})")
    assert torch.equal(got, g1 + g2), f"joint gradient off g1 + g2 by {d:.2e} (norm-rel)"
    assert errs[worst] <= env, f"{net} {worst}: {errs[worst]:.3e} (fp32 oracle {r['e32'][worst]:.3e})"


# ------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("net", NETS)
def test_accumulate_three_micro_batches_then_step(net):
    """(b) three backward() calls without zero_grad accumulate ((g1 + g2) + g1, bit for bit) into
    one flat arena (f); a HipAdamW step from it equals, in parameters, moments and the next
    forward, the step of a fresh model whose .grad holds the same sum."""
    import unet_hip
    (_, g1), (_, g2) = _singles(net)
    b = _dev_batches()
    m = _model(net)
    for x, t in (b[0], b[1], b[0]):
        _loss(m, x, t)[1].backward()
    want = (g1 + g2) + g1
    assert torch.equal(_flat(m), want)
    _assert_flat(m, at_state_arena=False)
    ref = _model(net)
    st = ref.flatten_()
    arena = want.clone()
    assert arena.numel() == st.param_arena.numel()
    for (p, _, _), g in zip(st.params, st.grad_views(arena)):
        p.grad = g
    start = _params(ref)
    out = []
    for mod in (m, ref):
        opt = unet_hip.HipAdamW(mod.parameters(), lr=LR)
        opt.step()
        mom = [torch.cat([opt.state[p][k].reshape(-1) for p in mod.parameters()]) for k in
               ("exp_avg", "exp_avg_sq")]
        with torch.no_grad():
            nxt = mod(b[0][0])
        out.append((_params(mod), mom[0], mom[1], nxt))
    assert not torch.equal(out[0][0], start)
    for got, exp, what in zip(out[0], out[1], ("parameters", "exp_avg", "exp_avg_sq", "next logits")):
        assert torch.equal(got, exp), what


# ------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("net", NETS)
def test_zero_grad_in_place_between_steps(net):
    """(c) zero_grad(set_to_none=False) between steps: the gradients of the set_to_none=True
    path."""
    (_, g1), (_, g2) = _singles(net)
    (x1, t1), (x2, t2) = _dev_batches()
    m = _model(net)
    _loss(m, x1, t1)[1].backward()
    assert torch.equal(_flat(m), g1)
    _zero(m, set_to_none=False)
    _loss(m, x2, t2)[1].backward()
    assert torch.equal(_flat(m), g2)


# ------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("net", NETS)
def test_kept_grad_survives_the_next_step(net):
    """(d) references to last step's .grad kept over zero_grad(set_to_none=True) still hold that
    step's values after the next backward."""
    (_, g1), (_, g2) = _singles(net)
    (x1, t1), (x2, t2) = _dev_batches()
    m = _model(net)
    _loss(m, x1, t1)[1].backward()
    kept = [p.grad for p in m.parameters()]
    _zero(m)
    _loss(m, x2, t2)[1].backward()
    torch.cuda.synchronize()
    assert torch.equal(_flat(m), g2)
    assert torch.equal(torch.cat([g.reshape(-1) for g in kept]), g1)


# ------------------------------------------------------------------------------ (e)
@pytest.mark.parametrize("net", NETS)
def test_second_backward_is_refused(net, monkeypatch):
    """(e) a second backward through a retained graph raises in Python, before the library."""
    (_, g1), _ = _singles(net)
    x1, t1 = _dev_batches()[0]
    m = _model(net)
    rt = m.flatten_().rt
    calls, native = [], rt.backward
    monkeypatch.setattr(rt, "backward", lambda *a, **k: (calls.append(1), native(*a, **k))[1])
    loss = _loss(m, x1, t1)[1]
    loss.backward(retain_graph=True)
    assert len(calls) == 1
    with pytest.raises(RuntimeError, match="workspace of a training forward is consumed by its backward"):
        loss.backward()
    assert len(calls) == 1
    assert torch.equal(_flat(m), g1)


# ------------------------------------------------------------------------------ (f)
@pytest.mark.parametrize("net", NETS)
def test_trainer_pattern_grads_are_the_state_arena(net):
    """(f) zero_grad(set_to_none=True) -> forward -> backward -> HipAdamW.step: after every
    backward the .grad tensors are contiguous views of the state's one flat arena, laid out like
    the parameter arena, and a steady step allocates nothing the one before did not."""
    import unet_hip
    x1, t1 = _dev_batches()[0]
    m = _model(net)
    opt = unet_hip.HipAdamW(m.parameters(), lr=LR)
    mem = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        loss = _loss(m, x1, t1)[1]
        loss.backward()
        _assert_flat(m, at_state_arena=True)
        opt.step()
        del loss
        mem.append(torch.cuda.memory_allocated(DEV))
    assert mem[1] == mem[2], mem


# ------------------------------------------------------------------------------ no-grad / eval
@pytest.mark.parametrize("net", NETS)
def test_train_mode_forward_under_no_grad(net):
    """Train-mode forwards under torch.no_grad(): no grad_fn, the plain steps' logits, and the
    BN buffers the oracle has after x1 then x2."""
    (l1, _), (l2, _) = _singles(net)
    (x1, _), (x2, _) = _dev_batches()
    m = _model(net)
    with torch.no_grad():
        a1, a2 = m(x1), m(x2)
    assert a1.grad_fn is None and a2.grad_fn is None and not a1.requires_grad
    assert torch.equal(a1, l1) and torch.equal(a2, l2)
    _check_buffers(m, net, 2)


@pytest.mark.parametrize("net", NETS)
def test_eval_forward_between_forward_and_backward(net):
    """A no-grad eval() forward of the same model on another shape between a training forward
    and its backward leaves the gradients bit-equal to the undisturbed step."""
    (l1, g1), _ = _singles(net)
    (x1, t1), (x2, _) = _dev_batches()
    m = _model(net)
    logits, loss = _loss(m, x1, t1)
    m.eval()
    with torch.no_grad():
        e = m(x2)
    m.train()
    loss.backward()
    assert e.grad_fn is None and torch.isfinite(e).all()
    assert torch.equal(logits.detach(), l1) and torch.equal(_flat(m), g1)


# ------------------------------------------------------------------------------ input forms
@pytest.mark.parametrize("form", ["crop_view", "float64"])
@pytest.mark.parametrize("net", NETS)
def test_input_forms(net, form):
    """A non-contiguous crop view and a float64 x: logits and gradients bit-equal to the
    contiguous float32 call."""
    (l1, g1), _ = _singles(net)
    x1, t1 = _dev_batches()[0]
    if form == "crop_view":
        big = torch.full((2, 1, 80, 77), 9.0, device=DEV)
        big[:, :, 8:72, 5:69] = x1
        x = big[:, :, 8:72, 5:69]
        assert not x.is_contiguous()
    else:
        x = x1.double()
    assert torch.equal(x.float(), x1)
    m = _model(net)
    logits, g = _plain_step(m, x, t1)
    assert logits.dtype == torch.float32
    assert torch.equal(logits, l1) and torch.equal(g, g1)


@pytest.mark.parametrize("form", ["stride0", "strided", "transposed"])
@pytest.mark.parametrize("net", NETS)
def test_incoming_gradient_forms(net, form):
    """logits.sum() (a stride-0 dlogits), a squared every-other-pixel slice, a product with a
    transposed weight map: each bit-equal to logits.backward(gradient=d.contiguous()) of the same
    values."""
    x1, _ = _dev_batches()[0]
    m = _model(net)
    logits = m(x1)
    lg = logits.detach()
    if form == "stride0":
        loss, d = logits.sum(), torch.ones_like(lg)
    elif form == "strided":
        loss = logits[:, :, ::2, ::2].square().sum()
        d = torch.zeros_like(lg)
        d[:, :, ::2, ::2] = 2 * lg[:, :, ::2, ::2]
    else:
        g = torch.Generator(device="cpu").manual_seed(5)
        w = torch.rand(2, 1, 64, 64, generator=g).to(DEV).transpose(2, 3)
        assert not w.is_contiguous()
        loss, d = (logits * w).sum(), w.contiguous()
    _zero(m)
    loss.backward()
    got = _flat(m)
    _zero(m)
    again = m(x1)
    assert torch.equal(again.detach(), lg)
    again.backward(gradient=d.contiguous())
    want = _flat(m)
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------ seg_losses
@pytest.mark.parametrize("use", ["bce", "dice", "focal", "sum"])
def test_seg_losses_partly_used(use):
    """seg_losses with only one of its three outputs used, and with losses.sum(): the values and
    dlogits against tests/loss_ref.py at the bars of tests/test_gpu_loss_edges.py."""
    import unet_hip
    x, t = L.make_case((2, 1, 32, 32), "soft")
    w = {"bce": (1.0, 0.0, 0.0), "dice": (0.0, 1.0, 0.0), "focal": (0.0, 0.0, 1.0),
         "sum": (1.0, 1.0, 1.0)}[use]
    xd = torch.from_numpy(x).to(DEV).requires_grad_(True)
    losses = unet_hip.seg_losses(xd, torch.from_numpy(t).to(DEV))
    (losses.sum() if use == "sum" else losses[("bce", "dice", "focal").index(use)]).backward()
    abg = L.ABG[0]
    ref_l, ref_g = L.losses(x, t, *abg), L.dlogits(x, t, w, *abg)
    y_l, y_g = L.torch_losses_and_grad(x, t, w, *abg, dtype=torch.float32)
    e_l, ey_l = np.abs(losses.detach().cpu().double().numpy() - ref_l), np.abs(y_l - ref_l)
    e_g = L.sample_rel_err(xd.grad.cpu().numpy(), ref_g)
    ey_g = L.sample_rel_err(y_g, ref_g)
    print(f"{use}: losses dev {e_l.max():.2e} / torch32 {ey_l.max():.2e}; dlogits dev "
          f"{e_g.max():.2e} / torch32 {ey_g.max():.2e}")
    for k in range(3):
        assert e_l[k] <= TL._bar(ey_l[k]), (use, k, e_l[k], ey_l[k])
    for n in range(x.shape[0]):
        assert e_g[n] <= TL._bar(ey_g[n]), (use, n, e_g[n], ey_g[n])


# ------------------------------------------------------------------------------ refused input
@pytest.mark.parametrize("net", NETS)
def test_input_that_requires_grad_is_refused(net, monkeypatch):
    """x.requires_grad_(True) in a grad-enabled training forward: ValueError before the library
    (the native path has no input gradient), instead of an x.grad that silently stays None."""
    x1, _ = _dev_batches()[0]
    m = _model(net)
    rt = m.flatten_().rt
    calls, native = [], rt.forward
    monkeypatch.setattr(rt, "forward", lambda *a, **k: (calls.append(1), native(*a, **k))[1])
    with pytest.raises(ValueError, match="computes no input gradient"):
        m(x1.clone().requires_grad_(True))
    assert not calls
    with torch.no_grad():  # nothing to differentiate: allowed
        m(x1.clone().requires_grad_(True))
    assert len(calls) == 1


# ------------------------------------------------------------------------------ copies
def _spans(m):
    st = m._state
    return [(a.data_ptr(), a.numel() * a.element_size()) for a in (st.param_arena, st.bn_arena, st.nbt_arena)]


def _adam_step(m, opt, x, t):
    opt.zero_grad(set_to_none=True)
    logits, loss = _loss(m, x, t)
    loss.backward()
    opt.step()
    return logits.detach().clone()


def _eval_logits(m, x):
    m.eval()
    with torch.no_grad():
        out = m(x)
    m.train()
    return out


@pytest.mark.parametrize("how", ["deepcopy", "pickle"])
@pytest.mark.parametrize("net", NETS)
def test_copy_after_a_training_step(net, how):
    """copy.deepcopy(model) / pickle.loads(pickle.dumps(model)) after a HipAdamW step: the copy
    shares no storage with the source, has its parameters and buffers, its eval logits and its
    gradients on a batch; stepping the copy leaves the source (parameters, next forward) where an
    uncopied twin is, and the source stepped again stays bit-equal to that twin."""
    import unet_hip
    (x1, t1), (x2, t2) = _dev_batches()
    src, twin = _model(net), _model(net)
    osrc = unet_hip.HipAdamW(src.parameters(), lr=LR)
    otwin = unet_hip.HipAdamW(twin.parameters(), lr=LR)
    assert torch.equal(_adam_step(src, osrc, x1, t1), _adam_step(twin, otwin, x1, t1))
    c = copy.deepcopy(src) if how == "deepcopy" else pickle.loads(pickle.dumps(src))
    assert type(c) is type(src) and c._state is None and c.training
    spans = _spans(src)
    a, b = src.state_dict(), c.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert b[k].device == a[k].device and torch.equal(a[k], b[k]), k
        assert not any(lo <= b[k].data_ptr() < lo + n for lo, n in spans), k
    assert torch.equal(_eval_logits(c, x2), _eval_logits(src, x2))
    assert c._state is not None and c._state.rt is src._state.rt  # the shared runtime, found again
    lo, n = _spans(c)[0]
    assert lo + n <= spans[0][0] or spans[0][0] + spans[0][1] <= lo
    _eval_logits(twin, x2)
    (lc, gc), (ls, gs), (lt, gt) = (_plain_step(mod, x2, t2) for mod in (c, src, twin))
    assert torch.equal(lc, ls) and torch.equal(gc, gs)
    assert torch.equal(ls, lt) and torch.equal(gs, gt)
    # one step of the copy (its weight images are now the shared context's)
    before = _params(c)
    unet_hip.HipAdamW(c.parameters(), lr=LR).step()
    assert not torch.equal(_params(c), before)
    assert torch.equal(_params(src), _params(twin))
    for k, v in src.named_buffers():
        assert torch.equal(v, dict(twin.named_buffers())[k]), k
    # the source goes on (the step of the x2 gradients, then a whole step) like its twin
    osrc.step()
    otwin.step()
    assert torch.equal(_params(src), _params(twin))
    assert torch.equal(_adam_step(src, osrc, x1, t1), _adam_step(twin, otwin, x1, t1))
    assert torch.equal(_params(src), _params(twin))
    for p, q in zip(src.parameters(), twin.parameters()):
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(osrc.state[p][k], otwin.state[q][k]), k
