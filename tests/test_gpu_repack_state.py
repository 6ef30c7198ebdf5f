"""The state behind the fused AdamW + weight repack (unet_adamw_repack), driven the way callers
can drive it: several models of one configuration on one device share ONE native context, and
with it one set of GEMM weight images (those of the arena whose fused step ran last).  Which
forward read them, whether they still match the parameters, and which backward may read them
must come out right whatever the models, options and optimizers do in between.

Two references, used together where both apply:

* sharp: bit-identical to the same computation with the fused images out of play -- for
  gradients the same model state after ``params_changed()`` (its forward then packs into its own
  workspace), run alone; for logits a fresh model loaded from the current parameters and
  buffers.  tests/test_gpu_parity.py::test_adamw_repack_bit_identical holds the fused path
  bit-identical to the unfused one, which licenses this reference.
* independent: for models/model.py UNet (f32) every gradient tensor against the CPU oracle from
  that model's current parameters at the project's bars (gradients 1e-2 norm-relative per
  tensor, logits 1e-4 of max|ref|).  The bf16 variant has no f32 oracle by construction.

Models that share a context start from different seeds, and lr is 1e-3, so a mix-up of two
models' images or an image one step stale is an error of percents, not of a last bit.
Shapes: B = 2 at 32x32, the smallest at which every level runs on the images end to end."""
import copy
import gc

import pytest
import torch

from _helpers import grad_errors, hip_model, inputs, options, rel_max
from oracle import mod_ref_cpu as MO
from oracle import unet_ref_cpu as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LR = 1e-3
GRAD_TOL = 1e-2
LOGIT_TOL = 1e-4
VARIANTS = ["model", "mod_bf16"]


def _build(variant, seed=None, like=None):
    """A model of `variant` from make_params(seed), or from the current parameters and buffers
    of the model `like`."""
    import unet_hip
    if like is not None:
        P = {k: v.detach().cpu().clone() for k, v in like.named_parameters()}
        B = {k: v.detach().cpu().clone() for k, v in like.named_buffers()}
    elif variant == "model":
        P, B = O.make_params(seed), O.init_buffers()
    else:
        P, B = MO.make_params(seed, 64, 3), MO.init_buffers(64, 3)
    if variant == "model":
        return hip_model(P, DEV, B)
    m = unet_hip.ModUNet(1, 1, base_filters=64, depth=3, mfma_dtype="bf16")
    sd = m.state_dict()
    sd.update({k: v.clone() for k, v in P.items()})
    sd.update({k: v.clone() for k, v in B.items()})
    m.load_state_dict(sd)
    return m.to(DEV).train()


def _batch(seed):
    x, t = inputs(seed, 2, 32, 32)
    return x.to(DEV), t.to(DEV)


def _loss(m, x, t):
    import unet_hip
    logits = m(x)
    l = unet_hip.seg_losses(logits, t)
    return logits, l[0] + l[1]


def _step(m, opt, x, t):
    opt.zero_grad()
    logits, loss = _loss(m, x, t)
    loss.backward()
    opt.step()
    return logits.detach().clone()


def _grad_arena(m):
    return torch.cat([p.grad.detach().reshape(-1) for p in m.parameters()]).clone()


def _param_arena(m):
    return torch.cat([p.detach().reshape(-1) for p in m.parameters()]).clone()


def _check_grads(tag, variant, m, x, t, logits):
    """m holds the gradients of loss(m(x), t) computed in the situation under test, and `logits`
    that forward's output: both bit-equal to the same model run alone on its own repack and,
    for the f32 model, within the project's bars of the CPU oracle."""
    got_g, got_l = _grad_arena(m), logits.detach().clone()
    e_l = e_g = 0.0
    if variant == "model":
        P = {k: v.detach().cpu().clone() for k, v in m.named_parameters()}
        B = {k: v.detach().cpu().clone() for k, v in m.named_buffers()}
        ref = O.train_step(P, B, None, x.cpu(), t.cpu())
        e_l = rel_max(got_l.cpu().numpy(), ref["logits"].numpy())
        errs = grad_errors(m, ref["grads"])
        k_w = max(errs, key=errs.get)
        e_g = errs[k_w]
        print(f"{tag}: oracle logits {e_l:.2e}, worst grad {k_w} {e_g:.2e}")
    m.params_changed()
    for p in m.parameters():
        p.grad = None
    want_l, loss = _loss(m, x, t)
    loss.backward()
    want_g = _grad_arena(m)
    d_l = (got_l - want_l.detach()).abs().max().item()
    d_g = float((got_g - want_g).double().norm() / want_g.double().norm())
    print(f"{tag}: vs alone on its own repack: logits max diff {d_l:.2e}, grads norm-rel {d_g:.2e}")
    assert torch.equal(got_l, want_l.detach()), f"{tag}: logits differ by {d_l:.2e}"
    assert torch.equal(got_g, want_g), f"{tag}: gradient arena off by {d_g:.2e} (norm-rel)"
    assert e_l <= LOGIT_TOL, f"{tag}: logits vs oracle {e_l:.2e}"
    assert e_g <= GRAD_TOL, f"{tag}: worst gradient tensor vs oracle {e_g:.2e}"


def _check_logits_fresh(tag, variant, m, x, oracle=False):
    """m's next training forward of x is bit-equal to that of a fresh model loaded from m's
    current parameters and buffers.  Returns the fresh model."""
    got = m(x).detach().clone()  # before the fresh model exists
    e = 0.0
    ref = _build(variant, like=m)
    if oracle:
        P = {k: v.detach().cpu().clone() for k, v in ref.named_parameters()}
        B = {k: v.detach().cpu().clone() for k, v in ref.named_buffers()}
        with torch.no_grad():
            rl = O.forward(x.cpu(), P, B, True)
        e = rel_max(got.cpu().numpy(), rl.numpy())
        print(f"{tag}: oracle logits {e:.2e}")
    want = ref(x).detach()
    d = (got - want).abs().max().item() / want.abs().max().item()
    print(f"{tag}: logits vs a fresh model: max diff {d:.2e} of max|ref|")
    assert torch.equal(got, want), f"{tag}: logits off by {d:.2e} of max|ref|"
    assert e <= LOGIT_TOL, f"{tag}: logits vs oracle {e:.2e}"
    return ref


@pytest.mark.parametrize("order", ["AB", "BA"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_joint_backward_of_two_models(variant, order):
    """Two models of one configuration, one fused step each (the context's images are B's), then
    both training forwards in either order and ONE backward of loss_A + loss_B: each model's
    backward must read the images its own forward read -- A its workspace's, B the context's."""
    import unet_hip
    M = {"A": _build(variant, 42), "B": _build(variant, 7)}
    opt = {k: unet_hip.HipAdamW(m.parameters(), lr=LR) for k, m in M.items()}
    data = {"A": _batch(101), "B": _batch(102)}
    for k in "AB":
        _step(M[k], opt[k], *data[k])
    for k in "AB":
        opt[k].zero_grad()
    logits, total = {}, 0
    for k in order:
        logits[k], loss = _loss(M[k], *data[k])
        total = total + loss
    total.backward()
    bad = []
    for k in "AB":  # both models' figures before failing on either
        try:
            _check_grads(f"{variant} {order} model {k}", variant, M[k], *data[k], logits[k])
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, bad


@pytest.mark.parametrize("variant", VARIANTS)
def test_backward_after_another_models_fused_step(variant):
    """B takes a fused step (rewriting the context's images) between A's forward and A's
    backward.  A forward that packed into its own workspace is untouched by that: its backward
    succeeds and is right.  A forward that read the context's images must still refuse."""
    import unet_hip
    from unet_hip._lib import HipError
    A, B = _build(variant, 42), _build(variant, 7)
    oA, oB = unet_hip.HipAdamW(A.parameters(), lr=LR), unet_hip.HipAdamW(B.parameters(), lr=LR)
    (xa, ta), (xb, tb) = _batch(101), _batch(102)
    _step(A, oA, xa, ta)
    _step(B, oB, xb, tb)      # the images are B's: A's forward packs into its own workspace
    oA.zero_grad()
    logits, loss = _loss(A, xa, ta)
    oB.step()                 # B's gradients are still there: a fused repack
    loss.backward()
    _check_grads(f"{variant} own workspace", variant, A, xa, ta, logits)
    _step(A, oA, xa, ta)      # the images are A's: A's forward reads them
    oA.zero_grad()
    logits, loss = _loss(A, xa, ta)
    oB.step()
    with pytest.raises(HipError):
        loss.backward()


@pytest.mark.parametrize("variant", VARIANTS)
def test_teacher_forward_between_student_forward_and_backward(variant):
    """Student S trains on the fused images; teacher T (same configuration, so the same
    context) is updated in place under no_grad, EMA style, and evaluated between S's forward
    and S's backward.  T's parameter change is T's alone: S's images were never rewritten, so
    S's backward runs and is right -- on the iteration where T's update is noticed and on the
    next, where T is quiet."""
    import unet_hip
    S, T = _build(variant, 42), _build(variant, 7)
    opt = unet_hip.HipAdamW(S.parameters(), lr=LR)
    x, t = _batch(103)
    _step(S, opt, x, t)
    T.eval()
    for it in range(2):
        if it == 0:
            with torch.no_grad():
                for pt, ps in zip(T.parameters(), S.parameters()):
                    pt.mul_(0.99).add_(ps.detach(), alpha=0.01)
        opt.zero_grad()
        logits, loss = _loss(S, x, t)
        with torch.no_grad():
            T(x)
        loss.backward()
        _check_grads(f"{variant} iteration {it}", variant, S, x, t, logits)
        opt.step()


def test_option_round_trip_leaves_no_stale_x3_images():
    """A fused step under x3=0 rewrites the f32 images only; back under x3=1 the x3 images are
    those of a step earlier and must not be read."""
    import unet_hip
    x, t = _batch(104)
    m = _build("model", 42)
    opt = unet_hip.HipAdamW(m.parameters(), lr=LR)
    _step(m, opt, x, t)
    rt = m.flatten_().rt
    assert rt.get_option("x3") == 1
    with options(rt, x3=0):
        _step(m, opt, x, t)
    ref = _check_logits_fresh("after x3 1 -> 0 -> 1", "model", m, x, oracle=True)
    # one further full step of both: logits and parameters
    ropt = unet_hip.HipAdamW(ref.parameters(), lr=LR)
    ropt.load_state_dict(copy.deepcopy(opt.state_dict()))
    got, want = _step(m, opt, x, t), _step(ref, ropt, x, t)
    assert torch.equal(got, want), (got - want).abs().max().item()
    pa, pr = _param_arena(m), _param_arena(ref)
    assert torch.equal(pa, pr), (pa - pr).abs().max().item()
    _check_logits_fresh("one step later", "model", m, x)


@pytest.mark.parametrize("how", ["frozen", "two_groups", "raw_abi"])
def test_plain_adamw_after_a_fused_step(how):
    """After fused steps, a step that cannot be fused -- one 3x3 weight frozen (per-tensor
    launches), an optimizer with two parameter groups (one launch per group), unet_adamw called
    on the arena directly -- writes the parameters without packing: the next forward must not
    read the images of the step before."""
    import unet_hip
    x, t = _batch(105)
    m = _build("model", 42)
    opt = unet_hip.HipAdamW(m.parameters(), lr=LR)
    _step(m, opt, x, t)
    if how == "frozen":
        m.encoder2[3].weight.requires_grad_(False)
        _step(m, opt, x, t)
    elif how == "two_groups":
        enc = [p for n, p in m.named_parameters() if n.startswith("encoder")]
        dec = [p for n, p in m.named_parameters() if not n.startswith("encoder")]
        opt2 = unet_hip.HipAdamW([{"params": enc}, {"params": dec}], lr=LR)
        _step(m, opt2, x, t)
    else:
        opt.zero_grad()
        _, loss = _loss(m, x, t)
        loss.backward()
        st = m.flatten_()
        g = st.grad_arena
        assert g.data_ptr() == next(m.parameters()).grad.data_ptr()
        st.rt.adamw(st.param_arena, g, torch.zeros_like(g), torch.zeros_like(g), 1, LR, 0.9, 0.999,
                    1e-8, 1e-2)
    _check_logits_fresh(how, "model", m, x, oracle=True)


def test_arena_address_reuse():
    """A model trained one fused step dies; the next model of its configuration usually gets its
    arena's address back from the caching allocator, and must not inherit its images."""
    import unet_hip
    x, t = _batch(106)
    m = _build("model", 42)
    opt = unet_hip.HipAdamW(m.parameters(), lr=LR)
    _step(m, opt, x, t)
    addr = m.flatten_().param_arena.data_ptr()
    del m, opt
    gc.collect()
    m2 = _build("model", 7)
    print("arena address reused:", m2.flatten_().param_arena.data_ptr() == addr)
    _check_logits_fresh("second model", "model", m2, x, oracle=True)


def _pack_launches(m, x):
    """The weight-repack launches of one training forward of m (per-launch timing records)."""
    rt = m.flatten_().rt
    rt.timing(True)
    try:
        m(x)
        torch.cuda.synchronize()
        return [lab for lab, _, _ in rt.timing_records() if lab.partition("/")[0] == "pack"]
    finally:
        rt.timing(False)


@pytest.mark.parametrize("variant", VARIANTS)
def test_fused_images_outlive_another_models_update(variant):
    """What the fused step is for: the forward after it launches no repack -- also when another
    model of the configuration was updated and evaluated in between (its invalidation is scoped
    to its own arena) -- and does again once this model's own parameters are declared changed."""
    import unet_hip
    S, T = _build(variant, 42), _build(variant, 7)
    opt = unet_hip.HipAdamW(S.parameters(), lr=LR)
    x, t = _batch(107)
    _step(S, opt, x, t)
    assert _pack_launches(S, x) == []
    with torch.no_grad():
        for pt in T.parameters():
            pt.mul_(0.5)
        T(x)
    assert _pack_launches(S, x) == []
    S.params_changed()
    assert _pack_launches(S, x) != []
