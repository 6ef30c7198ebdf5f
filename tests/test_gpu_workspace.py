"""The memory contract under unet_forward / unet_backward (include/unet_hip.h, "The workspace
contract"): the caller's workspace may hold anything on entry, nothing outside the plan and the
named outputs is written, the parameters are read-only, and every entry of `grads` is overwritten.

The parity tests take their workspace from torch.empty: zeros in a fresh process, the previous
step's almost-right values afterwards.  A kernel that reads a lane, a halo row, a padded channel or
a split-K slab entry nobody wrote this step passes all of them.  Here every buffer the library sees
lies between two 4 MiB guard bands of a fixed byte pattern (4 MiB: a fixed condition, larger than
any row tile of these shapes, so an overrun of that size stays inside memory the test owns), and
the workspace interior is filled before the step with

  zero   0x00;
  ones   0xFF: NaN as f32 and as bf16, 255 as a max-pool winner index;
  huge   0x7F7F7F7F: a large finite f32 / bf16, so garbage times zero shows as inf or NaN and a
         read under a max (pool, ReLU) survives;
  stale  a complete training step (forward, loss gradient, backward) of another input and target
         in the same workspace.

One step = training forward, dlogits of BCE + Dice (unet_loss_bwd), backward, then an eval forward
in a workspace of its own size and fill.  After each call every guard band and the parameter arena
must be bit-unchanged; logits, the BN running arena, num_batches_tracked, the whole grads arena
(pre-filled with NaN) and the eval logits must equal, bit for bit, those of the ordinary path: the
same step through unet_hip.UNet / ModUNet / ResUNet and autograd, workspaces from torch.empty.
The paths are deterministic (test_determinism_full_size, test_res_bf16_deterministic), so bit
equality is the bar and there is no tolerance.

Cases: tests/workspace_cases.py.  Each runs under the default schedule options and under every
single-option setting that changes its plan's size (probed on the host; the settings are the
test ids), the f32 cases also under x3 = 0, dz_in_wgrad, convt16, rg16, head_fuse, pool_fuse
toggled and wgrad_row3 = 0.

What this cannot see: two live regions of the plan that overlap.  Both paths run the same plan, so
they agree with each other; that shows against the oracles (the parity tests), and only at a shape
where the mis-sized term is the larger one: at these shapes `stats` and `part` are sized by their
RED_G floor (512 rows of 2 * cmax), not by the pixel count ((P + 63) / 64 and P / 64 + 1 rows).

Checked against two mutations of make_plan / forward_impl (not kept): without the memset of the
zero page, 12 of the 13 default cases fail (NaN gradients under the 0xFF fill; the base-16 depth-1
network runs no LDS-DMA GEMM); with the last region of the inference plan (s3) 4 KiB short, the
guard band behind the eval workspace is written and the check after the eval forward fails."""
import numpy as np
import pytest
import torch

import workspace_cases as WC
from _helpers import options
from oracle import mod_ref_cpu as MO
from oracle import unet_ref_cpu as O
from oracle import weights as Wt

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 4 << 20
FILLS = ("zero", "ones", "huge", "stale")
FILL_BYTE = {"zero": 0x00, "ones": 0xFF, "huge": 0x7F}

_PATTERN = None


def _pattern():
    global _PATTERN
    if _PATTERN is None:
        i = torch.arange(GUARD, dtype=torch.int64, device=DEV)
        _PATTERN = ((i * 37 + (i >> 8) * 11 + 0x5A) & 0xFF).to(torch.uint8)
    return _PATTERN


class Guarded:
    """One uint8 allocation guard | part 0 | part 1 | ... | guard; every part starts 256-byte
    aligned and directly after the one before it (rounded up to 256 bytes)."""

    def __init__(self, *sizes):
        offs, pos = [], GUARD
        for n in sizes:
            offs.append(pos)
            pos += (n + 255) & ~255
        self.buf = torch.empty(pos + GUARD, dtype=torch.uint8, device=DEV)
        assert self.buf.data_ptr() % 256 == 0, "torch allocation is not 256-byte aligned"
        self.parts = [self.buf[o:o + n] for o, n in zip(offs, sizes)]
        self.lo, self.hi = self.buf[:GUARD], self.buf[pos:]
        self.lo.copy_(_pattern())
        self.hi.copy_(_pattern())

    @property
    def mid(self):
        return self.parts[0]

    def intact(self):
        return torch.equal(self.lo, _pattern()) and torch.equal(self.hi, _pattern())


def _guarded_like(t):
    g = Guarded(t.numel() * t.element_size())
    v = g.mid.view(t.dtype).view(t.shape)
    v.copy_(t)
    return g, v


def _fill(ws, kind):
    ws.fill_(FILL_BYTE[kind])


# ---------------------------------------------------------------- parameters, data, models
def _splitmix64(z):
    """oracle.weights.splitmix64 on int64 tensors (wrapping arithmetic, logical shifts)."""
    def shr(v, k):
        return (v >> k) & ((1 << (64 - k)) - 1)

    def s64(v):
        v &= (1 << 64) - 1
        return v - (1 << 64) if v >> 63 else v

    z = z + s64(0x9E3779B97F4A7C15)
    z = (z ^ shr(z, 30)) * s64(0xBF58476D1CE4E5B9)
    z = (z ^ shr(z, 27)) * s64(0x94D049BB133111EB)
    return z ^ shr(z, 31)


def _device_params(spec, seed, dev=DEV):
    """oracle.weights.make_params(spec, seed), evaluated on `dev`: the same counter hash and the
    same float64 formulas (the deep narrow network has 2.8e8 parameters: seconds on the host)."""
    out = {}
    for t, item in enumerate(spec):
        name, shape, kind = item[0], tuple(item[1]), item[2]
        n = int(np.prod(shape))
        base = (seed * 0x9E3779B97F4A7C15 + (t << 36)) & ((1 << 64) - 1)
        base = base - (1 << 64) if base >> 63 else base
        h = _splitmix64(torch.arange(n, dtype=torch.int64, device=dev) + base)
        u = ((h >> 11) & ((1 << 53) - 1)).double() * (2.0 ** -53)
        if kind == "conv_w":
            v = (2 * u - 1) / np.sqrt(Wt.fan_in(shape))
        elif kind == "convT_w":
            v = (2 * u - 1) / np.sqrt(Wt.fan_in(shape, transposed=True))
        elif kind in ("conv_b", "convT_b"):
            v = (2 * u - 1) / np.sqrt(item[3])
        elif kind == "bn_w":
            v = 0.5 + u
        elif kind == "bn_b":
            v = 0.1 * (2 * u - 1)
        else:
            raise ValueError(kind)
        out[name] = v.float().reshape(shape)
    return out


def test_device_init_is_oracle_weights():
    """_device_params is oracle.weights.make_params bit for bit (the smallest network)."""
    spec = MO.param_spec(1, 2, 16, 1)
    want = Wt.make_params(spec, 11)
    got = _device_params(spec, 11)
    for k, v in want.items():
        assert np.array_equal(got[k].cpu().numpy(), v), k


def _spec(c):
    if c.net == "model":
        return O.param_spec(1, c.out_ch)
    if c.net == "res":
        return MO.res_param_spec(1, c.out_ch, c.base, c.depth)
    return MO.param_spec(1, c.out_ch, c.base, c.depth)


def _data(c, seed):
    x = torch.from_numpy(Wt.make_input(seed, c.N, 1, c.H, c.W))
    if c.out_ch == 1:
        t = torch.from_numpy(Wt.make_target(seed, c.N, c.H, c.W))
    else:  # hard targets that differ per class (tests/test_gpu_head_classes.py)
        g = torch.Generator().manual_seed(seed)
        t = (torch.rand(c.N, c.out_ch, c.H, c.W, generator=g) > 0.7).float()
    return x.to(DEV), t.to(DEV)


_MODEL = {}


def _model(c):
    """The module of case c on the device with oracle.weights parameters (seed 42) and fresh BN
    buffers; one case is kept at a time (the cases run one after the other)."""
    import unet_hip
    if c not in _MODEL:
        _MODEL.clear()
        torch.cuda.empty_cache()
        with torch.device(DEV):
            if c.net == "model":
                m = unet_hip.UNet(1, c.out_ch)
            else:
                cls = unet_hip.ResUNet if c.net == "res" else unet_hip.ModUNet
                m = cls(1, c.out_ch, base_filters=c.base, depth=c.depth, mfma_dtype=c.math)
        with torch.no_grad():
            named = dict(m.named_parameters())
            for k, v in _device_params(_spec(c), 42).items():
                named[k].copy_(v)
        m.train()
        st = m.flatten_()
        _MODEL[c] = (m, st.bn_arena.clone(), st.nbt_arena.clone())
    return _MODEL[c]


def _loss_grad(logits, t):
    """d(BCE + Dice)/d(logits), the call seg_losses' backward makes for loss = l[0] + l[1]."""
    from unet_hip.runtime import UNetRuntime
    lrt = UNetRuntime.get(DEV)
    stats, sums = lrt.loss_stats(logits, t)
    w = torch.tensor([1.0, 1.0, 0.0], device=DEV)
    return lrt.loss_bwd(logits, t, stats, sums, w)


def _ordinary(c, x, t):
    """One step on the ordinary path (module + autograd, torch.empty workspaces), from fresh BN
    buffers: logits, BN arena, num_batches_tracked, flat grads, eval logits.  The caller holds
    the options."""
    import unet_hip
    m, bn0, nbt0 = _model(c)
    st = m.flatten_()
    st.bn_arena.copy_(bn0)
    st.nbt_arena.copy_(nbt0)
    m.train()
    m.zero_grad(set_to_none=True)
    logits = m(x)
    losses = unet_hip.seg_losses(logits, t)
    (losses[0] + losses[1]).backward()
    grads = torch.cat([p.grad.reshape(-1) for p in m.parameters()]).clone()
    bn, nbt = st.bn_arena.clone(), st.nbt_arena.clone()
    m.eval()
    with torch.no_grad():
        ev = m(x).clone()
    m.train()
    m.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    return dict(logits=logits.detach().clone(), bn=bn, nbt=nbt, grads=grads, eval=ev)


# ---------------------------------------------------------------- the guarded raw path
def _forward(rt, params, bn, nbt, x, logits, ws, training, ws_bytes=None):
    """unet_forward as UNetRuntime.forward calls it, into the caller's logits; returns the status."""
    from unet_hip import _lib
    N, _, H, W = x.shape
    return rt.lib.unet_forward(rt.ctx, _lib.ptr(params), _lib.ptr(bn), _lib.ptr(nbt), _lib.ptr(x),
                               _lib.ptr(logits), _lib.ptr(ws),
                               ws.numel() if ws_bytes is None else ws_bytes, N, H, W,
                               int(training), _lib.stream_ptr(x.device))


def _ok(rt, rc, what):
    from unet_hip import _lib
    _lib.check(rc, rt.ctx, what)


class Harness:
    """The guarded buffers of one case under one option setting (sizes depend on both)."""

    def __init__(self, c, rt):
        m, bn0, nbt0 = _model(c)
        st = m.flatten_()
        self.c, self.rt, self.bn0, self.nbt0 = c, rt, bn0, nbt0
        self.params0 = st.param_arena
        shape = (c.N, c.out_ch, c.H, c.W)
        like = torch.empty(shape, dtype=torch.float32, device=DEV)
        self.nb = rt.workspace_bytes(c.N, c.H, c.W, True)
        self.nb_eval = rt.workspace_bytes(c.N, c.H, c.W, False)
        self.g_ws, self.g_ews = Guarded(self.nb), Guarded(self.nb_eval)
        self.g_par, self.params = _guarded_like(st.param_arena)
        self.g_bn, self.bn = _guarded_like(bn0)
        self.g_nbt, self.nbt = _guarded_like(nbt0)
        self.g_lg, self.logits = _guarded_like(like)
        self.g_dl, self.dlogits = _guarded_like(like)
        self.g_ev, self.ev = _guarded_like(like)
        self.g_gr, self.grads = _guarded_like(torch.empty(rt.n_param_floats, device=DEV))
        assert self.grads.numel() == rt.n_param_floats == st.param_arena.numel()
        # the stale fill's step runs on buffers of its own: the BN arenas must not see it twice
        self.s_bn, self.s_nbt = bn0.clone(), nbt0.clone()
        self.s_logits, self.s_grads = torch.empty_like(like), torch.empty_like(st.param_arena)

    def guards(self):
        return [g for g in (self.g_ws, self.g_ews, self.g_par, self.g_bn, self.g_nbt, self.g_lg,
                            self.g_dl, self.g_ev, self.g_gr)]

    def check_untouched(self, when):
        torch.cuda.synchronize()
        names = ("workspace", "eval workspace", "params", "bn", "nbt", "logits", "dlogits",
                 "eval logits", "grads")
        for name, g in zip(names, self.guards()):
            assert g.intact(), f"{when}: a guard band of the {name} buffer was written"
        assert torch.equal(self.params, self.params0), f"{when}: the parameter arena changed"

    def reset(self):
        self.bn.copy_(self.bn0)
        self.nbt.copy_(self.nbt0)
        for t in (self.logits, self.ev, self.grads):
            t.fill_(float("nan"))

    def stale_step(self, xs, ts):
        rt, ws = self.rt, self.g_ws.mid
        self.s_bn.copy_(self.bn0)
        self.s_nbt.copy_(self.nbt0)
        _ok(rt, _forward(rt, self.params, self.s_bn, self.s_nbt, xs, self.s_logits, ws, True), "stale forward")
        rt.backward(self.params, _loss_grad(self.s_logits, ts), self.s_grads, ws)
        _ok(rt, _forward(rt, self.params, self.s_bn, self.s_nbt, xs, self.s_logits, self.g_ews.mid, False),
            "stale eval forward")

    def step(self, fill, x, t, xs, ts):
        """The step under test after `fill`; returns clones of what it produced."""
        rt, ws, ews = self.rt, self.g_ws.mid, self.g_ews.mid
        self.reset()
        if fill == "stale":
            self.stale_step(xs, ts)
        else:
            _fill(ws, fill)
            _fill(ews, fill)
        self.check_untouched(f"{fill}: before the step")
        _ok(rt, _forward(rt, self.params, self.bn, self.nbt, x, self.logits, ws, True), "unet_forward")
        self.check_untouched(f"{fill}: after the training forward")
        out = dict(logits=self.logits.clone(), bn=self.bn.clone(), nbt=self.nbt.clone())
        assert torch.isfinite(out["logits"]).all(), f"{fill}: logits are not finite"
        self.dlogits.copy_(_loss_grad(self.logits, t))
        dl = self.dlogits.clone()
        rt.backward(self.params, self.dlogits, self.grads, ws)
        self.check_untouched(f"{fill}: after the backward")
        assert _same(self.dlogits, dl), f"{fill}: the backward wrote dlogits"
        assert _same(self.logits, out["logits"]), f"{fill}: the backward wrote logits"
        assert _same(self.bn, out["bn"]) and _same(self.nbt, out["nbt"]), \
            f"{fill}: the backward wrote the BN buffers"
        out["grads"] = self.grads.clone()
        bad = torch.isnan(out["grads"]).nonzero()
        assert bad.numel() == 0, (f"{fill}: {bad.numel()} entries of grads are NaN (not overwritten, "
                                  f"or computed from workspace garbage), first at {int(bad[0])}")
        _ok(rt, _forward(rt, self.params, self.bn, self.nbt, x, self.ev, ews, False), "eval forward")
        self.check_untouched(f"{fill}: after the eval forward")
        assert _same(self.bn, out["bn"]) and _same(self.nbt, out["nbt"]), \
            f"{fill}: the eval forward wrote the BN buffers"
        out["eval"] = self.ev.clone()
        return out


def _diff(a, b):
    if a.dtype.is_floating_point:
        # bit comparison: NaN == NaN, and +0 != -0
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    ne = (a != b).reshape(-1)
    n = int(ne.sum())
    return n, (int(ne.nonzero()[0]) if n else -1)


def _same(a, b):
    return _diff(a, b)[0] == 0


def _assert_same(got, want, what):
    for k in ("logits", "bn", "nbt", "grads", "eval"):
        n, first = _diff(got[k], want[k])
        assert n == 0, f"{what}: {k} differs in {n} of {want[k].numel()} entries, first at {first}"


def _matrix():
    out = []
    for c in WC.CASES:
        for kv in WC.option_settings(c):
            out.append(pytest.param(c, kv, id=f"{WC.case_id(c)}-{WC.settings_id(kv)}"))
    return out


@pytest.mark.parametrize("c,kv", _matrix())
def test_workspace_contents_do_not_matter(c, kv):
    """Every fill gives the ordinary path's bits, inside the guards (module docstring)."""
    rt = WC.runtime(c)
    x, t = _data(c, 3)
    xs, ts = _data(c, 8)
    _model(c)
    with options(rt, **kv):
        want = _ordinary(c, x, t)
        h = Harness(c, rt)
        first = None
        for fill in FILLS:
            got = h.step(fill, x, t, xs, ts)
            _assert_same(got, want, f"{fill} fill against the ordinary path")
            if first is None:
                first = got
            _assert_same(got, first, f"{fill} fill against the {FILLS[0]} fill")


INTERLEAVED = [c for i, c in enumerate(WC.CASES)
               if c.net not in {d.net for d in WC.CASES[:i]}]


@pytest.mark.parametrize("c", INTERLEAVED, ids=WC.case_id)
def test_interleaved_workspaces(c):
    """A training forward in workspace A, an eval forward of another shape in workspace B laid
    directly after A in the same allocation (both filled 0xFF), then the backward in A: the bits
    of the uninterleaved step, so neither call reaches into its neighbour."""
    rt = WC.runtime(c)
    x, t = _data(c, 3)
    q = 1 << max(c.depth, 4)
    c2 = c._replace(N=c.N + 1, H=c.H + q)
    x2, _ = _data(c2, 5)
    m, bn0, nbt0 = _model(c)
    want = _ordinary(c, x, t)
    params0 = m.flatten_().param_arena
    nb, nb2 = rt.workspace_bytes(c.N, c.H, c.W, True), rt.workspace_bytes(c2.N, c2.H, c2.W, False)
    g = Guarded(nb, nb2)
    a, b = g.parts
    assert b.data_ptr() == a.data_ptr() + ((nb + 255) & ~255)
    a.fill_(0xFF)
    b.fill_(0xFF)
    g_par, params = _guarded_like(params0)
    bn, nbt = bn0.clone(), nbt0.clone()
    g_lg, logits = _guarded_like(torch.full((c.N, c.out_ch, c.H, c.W), float("nan"), device=DEV))
    g_l2, logits2 = _guarded_like(torch.full((c2.N, c2.out_ch, c2.H, c2.W), float("nan"), device=DEV))
    g_gr, grads = _guarded_like(torch.full((rt.n_param_floats,), float("nan"), device=DEV))
    _ok(rt, _forward(rt, params, bn, nbt, x, logits, a, True), "forward in A")
    _ok(rt, _forward(rt, params, bn, nbt, x2, logits2, b, False), "eval forward in B")
    rt.backward(params, _loss_grad(logits, t), grads, a)
    torch.cuda.synchronize()
    for name, gd in (("workspace", g), ("params", g_par), ("logits", g_lg), ("logits B", g_l2),
                     ("grads", g_gr)):
        assert gd.intact(), f"a guard band of the {name} buffer was written"
    assert torch.equal(params, params0)
    assert torch.isfinite(logits2).all()
    got = dict(logits=logits, bn=bn, nbt=nbt, grads=grads, eval=want["eval"])
    _assert_same(got, want, "interleaved against the ordinary path")
    # B alone, in a workspace of its own: the same eval logits
    g_b = Guarded(nb2)
    g_b.mid.fill_(0xFF)
    alone = torch.full_like(logits2, float("nan"))
    _ok(rt, _forward(rt, params, bn, nbt, x2, alone, g_b.mid, False), "eval forward alone")
    torch.cuda.synchronize()
    assert g_b.intact() and _diff(alone, logits2)[0] == 0


@pytest.mark.parametrize("c", INTERLEAVED, ids=WC.case_id)
def test_short_workspace_is_refused_untouched(c):
    """ws_bytes = unet_workspace_size - 1 is UNET_ERR_WORKSPACE from unet_forward and from
    unet_backward, and nothing is launched: logits, grads and the workspace keep their bytes."""
    rt = WC.runtime(c)
    x, t = _data(c, 3)
    m, bn0, nbt0 = _model(c)
    params = m.flatten_().param_arena
    nb = rt.workspace_bytes(c.N, c.H, c.W, True)
    g = Guarded(nb)
    ws = g.mid
    ws.copy_(_pattern().repeat((nb + GUARD - 1) // GUARD)[:nb])
    ws0 = ws.clone()
    g_lg, logits = _guarded_like(torch.full((c.N, c.out_ch, c.H, c.W), float("nan"), device=DEV))
    g_gr, grads = _guarded_like(torch.full((rt.n_param_floats,), float("nan"), device=DEV))
    bn, nbt = bn0.clone(), nbt0.clone()

    def untouched(what):
        torch.cuda.synchronize()
        assert g.intact() and g_lg.intact() and g_gr.intact(), what
        assert torch.equal(ws, ws0), f"{what}: the workspace was written"
        assert torch.isnan(logits).all() and torch.isnan(grads).all(), f"{what}: an output was written"
        assert torch.equal(bn, bn0) and torch.equal(nbt, nbt0), f"{what}: the BN buffers were written"

    for training in (True, False):
        need = rt.workspace_bytes(c.N, c.H, c.W, training)
        rc = _forward(rt, params, bn, nbt, x, logits, ws, training, ws_bytes=need - 1)
        assert rc == -4, rc
        msg = rt.lib.unet_last_error(rt.ctx).decode()
        assert str(need - 1) in msg and str(need) in msg, msg
        untouched(f"refused forward (training={training})")
    # an eval-sized workspace handed to a training forward
    rc = _forward(rt, params, bn, nbt, x, logits, ws, True, ws_bytes=rt.workspace_bytes(c.N, c.H, c.W, False))
    assert rc == -4, rc
    untouched("training forward in an eval-sized workspace")
    # a good forward, then a backward told the workspace is one byte short
    from unet_hip import _lib
    lg = torch.empty_like(logits)
    _ok(rt, _forward(rt, params, bn.clone(), nbt.clone(), x, lg, ws, True), "unet_forward")
    torch.cuda.synchronize()
    ws1 = ws.clone()
    dl = _loss_grad(lg, t)
    rc = rt.lib.unet_backward(rt.ctx, _lib.ptr(params), _lib.ptr(dl), _lib.ptr(grads), _lib.ptr(ws),
                              nb - 1, c.N, c.H, c.W, _lib.stream_ptr(DEV))
    assert rc == -4, rc
    torch.cuda.synchronize()
    assert torch.equal(ws, ws1) and torch.isnan(grads).all() and g.intact() and g_gr.intact()
    rt.backward(params, dl, grads, ws)  # and the same workspace still serves the real backward
    torch.cuda.synchronize()
    assert not torch.isnan(grads).any() and g.intact() and g_gr.intact()
