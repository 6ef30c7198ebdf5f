"""The autograd bridge (unet_hip.functional.UNetFunction + unet_hip.module._ArenaState) driven
the ways a PyTorch user drives a module, with a stub in place of the native runtime.

The stub network is logits = x * s(theta), s = sum_i C_i theta_i with C_i = i + 1 over the
parameter arena, so for an incoming dlogits d the gradient of theta_i is C_i * sum(d * x): the
position in the arena is part of the value.  Its backward writes that into the arena it is handed
with '=' semantics, as unet_backward does, and counts its calls.  x, theta and the loss weights are
small integers, so every expected value is an exact float32 sum and the comparisons are
torch.equal.
"""
import pytest
import torch

from unet_hip.functional import UNetFunction
from unet_hip.module import _ArenaState
from unet_hip.optim import _flat_base

SHAPES = [(3,), (2, 2), (1,), (2, 1, 3)]
N_FLOATS = sum(torch.Size(s).numel() for s in SHAPES)
COEF = torch.arange(1, N_FLOATS + 1, dtype=torch.float32)


class StubRuntime:
    """What UNetFunction and _ArenaState call on a UNetRuntime."""

    def __init__(self):
        self.forwards = self.backwards = 0

    def arena_changed(self, arena):
        pass

    def forward(self, params, bn_running, bn_count, x, training, workspace=None):
        self.forwards += 1
        return x * (COEF * params).sum(), x.clone()  # the workspace: what the backward needs

    def backward(self, params, dlogits, grads, workspace):
        self.backwards += 1
        assert dlogits.is_contiguous() and grads.is_contiguous() and workspace.numel() > 0
        grads.copy_(COEF * (dlogits * workspace).sum())  # '=': whatever was there is gone


def _state():
    """(_ArenaState over the stub, its parameters): theta_i = i - 4."""
    arena = torch.arange(N_FLOATS, dtype=torch.float32) - 4
    plist, off = [], 0
    for shape in SHAPES:
        n = torch.Size(shape).numel()
        p = torch.nn.Parameter(torch.empty(0))
        p.data = arena[off:off + n].view(shape)
        plist.append((p, off, shape))
        off += n
    st = _ArenaState(StubRuntime(), plist, arena, torch.zeros(1), torch.zeros(1, dtype=torch.int64))
    return st, [p for p, _, _ in plist]


def _x(k, shape=(2, 1, 2, 2)):
    n = torch.Size(shape).numel()
    return ((torch.arange(n, dtype=torch.float32) * (k + 1)) % 7 - k).view(shape)  # sums differ


def _apply(st, x):
    return UNetFunction.apply(x, st, *[p for p, _, _ in st.params])


def _g(x, w=1.0):
    """The closed form of d(w * logits.sum()) / d theta, as the flat arena."""
    return COEF * (w * x.sum())


def _flat_grad(params):
    return torch.cat([p.grad.reshape(-1) for p in params])


def _zero(params, set_to_none):
    for p in params:
        if set_to_none:
            p.grad = None
        elif p.grad is not None:
            p.grad.zero_()


def test_two_applications_in_one_graph():
    """(a) loss(m(x1)) + loss(m(x2)), one backward: p.grad = g(x1) + g(x2), different shapes."""
    st, params = _state()
    x1, x2 = _x(0), _x(1, (1, 1, 2, 4))
    (2 * _apply(st, x1).sum() + 3 * _apply(st, x2).sum()).backward()
    assert st.rt.forwards == 2 and st.rt.backwards == 2
    want = _g(x1, 2.0) + _g(x2, 3.0)
    assert not torch.equal(want, 2 * _g(x1, 2.0)) and not torch.equal(want, 2 * _g(x2, 3.0))
    assert torch.equal(_flat_grad(params), want)


def test_three_backwards_accumulate():
    """(b) three backward() calls without zero_grad add up, and (f) the sum is still one flat
    arena laid out like the parameter arena."""
    st, params = _state()
    xs = [_x(k) for k in range(3)]
    for x in xs:
        _apply(st, x).sum().backward()
    assert torch.equal(_flat_grad(params), _g(xs[0]) + _g(xs[1]) + _g(xs[2]))
    flat = _flat_base([p.grad for p in params])
    assert flat is not None and flat.numel() == N_FLOATS
    assert torch.equal(flat, _flat_grad(params))


def test_zero_grad_in_place_equals_set_to_none():
    """(c) zero_grad(set_to_none=False) between steps gives the gradients of the set_to_none=True
    path."""
    got = {}
    for set_to_none in (True, False):
        st, params = _state()
        for k in range(3):
            _zero(params, set_to_none)
            _apply(st, _x(k)).sum().backward()
        got[set_to_none] = _flat_grad(params).clone()
    assert torch.equal(got[True], _g(_x(2)))
    assert torch.equal(got[False], got[True])


def test_kept_grad_survives_the_next_step():
    """(d) a reference to last step's .grad kept over zero_grad(set_to_none=True) holds the old
    values after the next backward."""
    st, params = _state()
    _apply(st, _x(0)).sum().backward()
    kept = [p.grad for p in params]
    old = [g.clone() for g in kept]
    _zero(params, True)
    _apply(st, _x(1)).sum().backward()
    assert not torch.equal(_g(_x(0)), _g(_x(1)))
    assert torch.equal(_flat_grad(params), _g(_x(1)))
    for g, o in zip(kept, old):
        assert torch.equal(g, o)
    assert torch.equal(torch.cat([g.reshape(-1) for g in kept]), _g(_x(0)))


def test_second_backward_is_refused():
    """(e) a second backward through a retained graph states the limit and enters the runtime no
    second time."""
    st, params = _state()
    loss = _apply(st, _x(0)).sum()
    loss.backward(retain_graph=True)
    assert st.rt.backwards == 1
    with pytest.raises(RuntimeError, match="workspace of a training forward is consumed by its backward"):
        loss.backward()
    assert st.rt.backwards == 1
    assert torch.equal(_flat_grad(params), _g(_x(0)))


@pytest.mark.parametrize("how", ["deepcopy", "pickle"])
def test_copy_of_a_flattened_model_drops_the_arenas(how):
    """A model whose tensors are views of flat arenas and whose state holds a native handle (what
    the first forward leaves behind; laid out by hand here, there is no device) copies and
    pickles: the copy has no state, equal values, and compact tensors of its own."""
    import copy
    import ctypes
    import pickle

    import unet_hip
    torch.manual_seed(3)
    m = unet_hip.ModUNet(1, 1, base_filters=8, depth=1)
    plist, off = [], 0
    arena = torch.empty(sum(p.numel() for p in m.parameters()))
    for p in m.parameters():
        arena[off:off + p.numel()] = p.detach().reshape(-1)
        p.data = arena[off:off + p.numel()].view(p.shape)
        plist.append((p, off, tuple(p.shape)))
        off += p.numel()
    bns = [b for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)]
    bn_arena = torch.arange(sum(2 * b.num_features for b in bns), dtype=torch.float32)
    nbt = torch.arange(len(bns), dtype=torch.int64) + 5
    off = 0
    for i, b in enumerate(bns):
        ch = b.num_features
        b.running_mean, b.running_var = bn_arena[off:off + ch], bn_arena[off + ch:off + 2 * ch]
        b.num_batches_tracked = nbt[i]
        off += 2 * ch
    rt = StubRuntime()
    rt.ctx = ctypes.c_void_p(1234)  # copy.deepcopy and pickle refuse this
    m._state = _ArenaState(rt, plist, arena, bn_arena, nbt)
    c = copy.deepcopy(m) if how == "deepcopy" else pickle.loads(pickle.dumps(m))
    assert type(c) is type(m) and c._state is None and m._state is not None
    assert c.training == m.training and (c.base_filters, c.depth) == (8, 1)
    src, dst = m.state_dict(), c.state_dict()
    assert list(src) == list(dst)
    spans = [(arena.data_ptr(), arena.numel() * 4), (bn_arena.data_ptr(), bn_arena.numel() * 4),
             (nbt.data_ptr(), nbt.numel() * 8)]
    for k in src:
        assert torch.equal(src[k], dst[k]) and dst[k].dtype == src[k].dtype, k
        assert dst[k].untyped_storage().nbytes() == dst[k].numel() * dst[k].element_size(), k
        assert not any(lo <= dst[k].data_ptr() < lo + n for lo, n in spans), k
    for (n, p), (_, q) in zip(m.named_parameters(), c.named_parameters()):
        assert isinstance(q, torch.nn.Parameter) and q.requires_grad == p.requires_grad, n
        assert p.data_ptr() == arena.data_ptr() + 4 * dict((id(a), o) for a, o, _ in plist)[id(p)]


def test_trainer_pattern_grads_are_one_flat_arena():
    """(f) zero_grad(set_to_none=True) -> forward -> backward: every p.grad is a contiguous view
    of the state's one flat arena, laid out like the parameter arena (HipAdamW's one-launch step
    and DistributedUNet's bucket reduce read it as such), step after step."""
    st, params = _state()
    for k in range(3):
        _zero(params, True)
        _apply(st, _x(k)).sum().backward()
        flat = _flat_base([p.grad for p in params])
        assert flat is not None and flat.numel() == N_FLOATS
        assert flat.data_ptr() == st.grad_arena.data_ptr()
        assert params[0].grad.data_ptr() == st.grad_arena.data_ptr()  # what dist.py asks
        for (p, off, shape) in st.params:
            assert p.grad.data_ptr() == st.grad_arena.data_ptr() + 4 * off
            assert tuple(p.grad.shape) == tuple(shape)
        assert torch.equal(st.grad_arena, _g(_x(k)))
