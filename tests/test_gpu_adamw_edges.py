"""AdamW at its edges, by the method of test_gpu_parity.py::test_adamw_bitwise_vs_oracle (same
oracle classes, same assertions, identical state going in at every step): the 16-B-vectorised
adamw4_kernel every real training step runs, the scalar kernel taken for alignment, tiny and
grid-stride-sized arenas, eps / step / weight_decay / grad_scale away from the defaults, and the
fused unet_adamw_repack with a gradient scale."""
import numpy as np
import pytest
import torch

from adamw_ref import assert_step_matches, oracle_step

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
# (n, byte offset of the four views from a 16-byte boundary)
VEC = (1 << 16, 0)          # n % 4 == 0, aligned: adamw4_kernel
OFFSET = ((1 << 16) + 4, 4)  # n % 4 == 0, views 4 bytes off: adamw_kernel by alignment
BIG = (16384 * 256 * 4 + 1024, 0)  # adamw4_kernel's grid-stride loop takes a second trip


def _rt():
    import unet_hip
    return unet_hip.UNetRuntime.get(DEV)


def _dev(a, off_bytes):
    buf = torch.empty(a.numel() + 8, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    k = off_bytes // 4
    d = buf[k:k + a.numel()]
    d.copy_(a)
    assert d.data_ptr() % 16 == off_bytes
    return d


def _grad(n, gen):
    scale = 10.0 ** torch.empty(n).uniform_(-7, -1, generator=gen)
    return torch.randn(n, generator=gen) * scale


def _state(n, gen, step):
    """Host (p, m, v) going into step number `step`: zero moments before the first step,
    otherwise moments of the size a run of such gradients leaves."""
    p = (torch.randn(n, generator=gen) * 0.05).float()
    if step == 1:
        return p, torch.zeros(n), torch.zeros(n)
    return p, _grad(n, gen) * 0.5, _grad(n, gen) ** 2 * 0.3


def _one_step(rt, p, g, m, v, step, off_bytes, lr, betas, eps, wd, gs, tag):
    pd, gd, md, vd = (_dev(a, off_bytes) for a in (p, g, m, v))
    rt.adamw(pd, gd, md, vd, step, lr, betas[0], betas[1], eps, wd, gs)
    torch.cuda.synchronize()
    p_ref, p_ieee, m_ref, v_ref = oracle_step(p, g, m, v, step, lr, betas, eps, wd, gs)
    nd = assert_step_matches(pd.cpu(), md.cpu(), vd.cpu(), p, p_ref, p_ieee, m_ref, v_ref, lr, wd, tag)
    return p_ieee, m_ref, v_ref, nd


@pytest.mark.parametrize("lr,wd,betas", [(1e-5, 1e-2, (0.9, 0.999)), (1e-3, 1e-2, (0.9, 0.999)),
                                         (3e-4, 0.1, (0.8, 0.99)), (1e-3, 0.0, (0.3, 0.9))])
@pytest.mark.parametrize("n,off", [VEC, OFFSET, (1, 0), (3, 0), (5, 0)])
def test_adamw_arenas_bitwise_vs_oracle(n, off, lr, wd, betas):
    """Four steps from identical state, as the scalar test, on the vector kernel (n = 2^16), on
    views 4 bytes off a 16-byte boundary (scalar kernel by alignment) and on n = 1, 3, 5."""
    rt = _rt()
    gen = torch.Generator().manual_seed(int(lr * 1e6) + int(wd * 100) + n)
    p, m, v = _state(n, gen, 1)
    for s in range(4):
        g = _grad(n, gen)
        p, m, v, nd = _one_step(rt, p, g, m, v, s + 1, off, lr, betas, 1e-8, wd, 1.0, f"step {s}")
        print(f"n {n} +{off}B step {s}: {nd} params differ from the torch-CPU oracle")


def test_adamw_vector_kernel_second_grid_trip():
    """n = 16384 * 256 * 4 + 1024 floats: adamw4_kernel's grid is capped at 16384 blocks, so its
    last 256 float4 are a second trip of the grid-stride loop.  One step."""
    n, off = BIG
    gen = torch.Generator().manual_seed(17)
    p, m, v = _state(n, gen, 3)
    g = _grad(n, gen)
    _one_step(_rt(), p, g, m, v, 3, off, 1e-3, (0.9, 0.999), 1e-8, 1e-2, 1.0, "big")


@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("eps", [1e-8, 1e-6, 1e-3])
@pytest.mark.parametrize("n,off", [VEC, OFFSET])
def test_adamw_eps_step_weight_decay(n, off, eps, wd):
    """Raw unet_adamw calls at step 1, 10, 1000 and 100000 (the bias corrections from
    pow(beta, step) in double), eps up to 1e-3 (where it dominates sqrt(v) for most elements)
    and weight_decay 0 (decay == 1) / 0.1."""
    rt = _rt()
    gen = torch.Generator().manual_seed(int(eps * 1e9) + int(wd * 10) + n)
    for step in (1, 10, 1000, 100000):
        p, m, v = _state(n, gen, step)
        g = _grad(n, gen)
        _one_step(rt, p, g, m, v, step, off, 1e-3, (0.9, 0.999), eps, wd, 1.0, f"step {step}")


@pytest.mark.parametrize("gs", [0.5, 1.0 / 3.0, 1.0 / 8.0])
@pytest.mark.parametrize("n,off", [VEC, OFFSET, (5, 0)])
def test_adamw_grad_scale(n, off, gs):
    """grad_scale (1 / world after an RCCL sum): the oracle takes g * float32(grad_scale),
    rounded once in fp32, as adamw_elem does; the same bit-level assertions."""
    rt = _rt()
    gen = torch.Generator().manual_seed(int(gs * 1000) + n)
    p, m, v = _state(n, gen, 1)
    for s in range(3):
        g = _grad(n, gen)
        p, m, v, _ = _one_step(rt, p, g, m, v, s + 1, off, 1e-3, (0.9, 0.999), 1e-6, 1e-2, gs,
                               f"gs {gs} step {s}")


def _net(variant):
    import unet_hip
    from oracle import mod_ref_cpu as MO
    from oracle import unet_ref_cpu as O
    if variant == "model":
        m = unet_hip.UNet(1, 1)
        P = O.make_params(42)
    else:
        m = unet_hip.ModUNet(1, 1, base_filters=64, depth=3, mfma_dtype="bf16")
        P = MO.make_params(61, 64, 3)
    sd = m.state_dict()
    sd.update({k: v.clone() for k, v in P.items()})
    m.load_state_dict(sd)
    return m.to(DEV).train()


@pytest.mark.parametrize("variant", ["model", "mod_bf16"])
def test_adamw_repack_grad_scale_bit_identical(variant):
    """unet_adamw_repack (pack_all_kernel's fused update + adamw_ranges_kernel) with
    grad_scale = 1/3 and eps = 1e-6 against unet_adamw on cloned arenas: p, m, v bit-identical,
    and the next forward's logits on the repacked weight images bit-identical to a forward that
    repacks from the updated arena, so the images were made from the scaled update.  N = 1,
    32 x 32: the smallest legal input."""
    import unet_hip
    from _helpers import inputs
    x, t = inputs(97, 1, 32, 32)
    xd, td = x.to(DEV), t.to(DEV)
    m = _net(variant)
    logits = m(xd)
    losses = unet_hip.seg_losses(logits, td)
    (losses[0] + losses[1]).backward()
    st = m.flatten_()
    fp, fg = st.param_arena, st.grad_arena
    assert next(m.parameters()).grad.data_ptr() == fg.data_ptr()
    gen = torch.Generator().manual_seed(3)
    n = fp.numel()
    mo = (_grad(n, gen) * 0.5).to(DEV)
    vo = (_grad(n, gen) ** 2 * 0.3).to(DEV)
    p0, m0, v0 = fp.detach().clone(), mo.clone(), vo.clone()
    p2, g2, m2, v2 = p0.clone(), fg.clone(), m0.clone(), v0.clone()
    hyper = (3, 1e-3, 0.9, 0.999, 1e-6, 1e-2, 1.0 / 3.0)
    st.rt.adamw_repack(fp.detach(), fg, mo, vo, *hyper)
    st.native_version = st.version()  # (as HipAdamW.step: the images match the parameters)
    st.rt.adamw(p2, g2, m2, v2, *hyper)
    torch.cuda.synchronize()
    assert torch.equal(fp.detach(), p2), f"{(fp.detach() != p2).sum().item()} params differ"
    assert torch.equal(mo, m2) and torch.equal(vo, v2)
    # the scale reached the kernels: the unscaled update of the same state is another one
    p3, m3, v3 = p0.clone(), m0.clone(), v0.clone()
    st.rt.adamw(p3, g2, m3, v3, *hyper[:-1], 1.0)
    assert not torch.equal(m3, m2) and not torch.equal(p3, p2)
    with torch.no_grad():
        fused = m(xd).clone()      # reads the images the fused step packed
        st.images_stale()
        repacked = m(xd).clone()   # repacks from the arena
    assert torch.equal(fused, repacked), (fused - repacked).abs().max().item()
