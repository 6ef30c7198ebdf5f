"""GPU tests of models/mod.py:ResUNet in bf16 math (``ResUNet(mfma_dtype="bf16")``): every 3x3
conv, 1x1 skip and ConvTranspose GEMM on bf16 operands with f32 accumulation, the Cin = 1 first
block in f32.  Oracle: tests/res_bf16_ref.py, which rounds exactly what the HIP kernels round.
"""
import os

import pytest
import torch

import res_bf16_ref as R
from _helpers import grad_errors, inputs, norm_rel, options, rel_max
from oracle import mod_ref_cpu as MO

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CONFIGS = [(64, 3, 64), (64, 5, 64), (128, 3, 64), (256, 2, 32)]


@pytest.fixture(autouse=True, scope="module")
def _threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def _model(P, base, depth, mfma="bf16"):
    import unet_hip
    m = unet_hip.ResUNet(1, 1, base_filters=base, depth=depth, mfma_dtype=mfma)
    sd = m.state_dict()
    for k, v in P.items():
        sd[k] = v.clone()
    for k, v in MO.res_init_buffers(base, depth).items():
        sd[k] = v.clone()
    m.load_state_dict(sd)
    return m.to(DEV).train()


def _step(m, x, t):
    import unet_hip
    m.zero_grad()
    logits = m(x.to(DEV))
    losses = unet_hip.seg_losses(logits, t.to(DEV))
    loss = losses[0] + losses[1]
    loss.backward()
    torch.cuda.synchronize()
    return (logits.detach().clone(),
            {k: p.grad.detach().clone() for k, p in m.named_parameters()},
            {k: b.detach().clone() for k, b in m.named_buffers()}, loss.item())


def _assert_same(a, b, what):
    assert torch.equal(a[0], b[0]), f"{what}: logits"
    for k, g0 in a[1].items():
        assert torch.equal(g0, b[1][k]), f"{what}: grad {k}"
    for k, b0 in a[2].items():
        assert torch.equal(b0, b[2][k]), f"{what}: buffer {k}"


def _distances(cfg):
    """(spread of the helper against itself fp32 / fp64: logits, worst gradient; the helper's
    distance from the fp32 oracle: logits, worst gradient) -- all on the CPU."""
    r32, r64, plain = R.oracles(*cfg)[:3]
    sl = rel_max(r32["logits"].numpy(), r64["logits"].numpy())
    sg = max(norm_rel(r32["grads"][k], r64["grads"][k]) for k in r32["grads"])
    dl = rel_max(r32["logits"].numpy(), plain["logits"].numpy())
    dg = max(norm_rel(r32["grads"][k], plain["grads"][k]) for k in r32["grads"])
    return sl, sg, dl, dg


def _fp32_bar(cfg):
    """Bar on the logits' distance to the fp32 oracle: the project's 5e-2 where the helper
    itself stays below it, else twice the helper's own distance (measured on the CPU)."""
    dl = _distances(cfg)[2]
    return 5e-2 if dl < 5e-2 else 2 * dl


@pytest.mark.parametrize("base,depth,size", CONFIGS)
def test_res_bf16_matches_bf16_oracle(base, depth, size):
    """One step (BCE + Dice) at B = 2 against the helper, by the method of
    test_gpu_mod.py::test_mod_bf16_matches_bf16_oracle: rounding to bf16 is discontinuous, so the
    bars are twice the helper's own fp32-vs-fp64 spread (logits 2 spread + 1e-4, every gradient
    2 max spread, loss 1e-3).  (64, 3): 64-output register-staged tiles next to the LDS-DMA
    ones; (64, 5): W < 16 one-tap fallback and a 2x2 bottleneck; (128, 3): every GEMM but block
    0's on the LDS-DMA kernels; (256, 2) at 32^2: the widest documented base, 256 .. 1024
    channels on 8 x 8 .. 32 x 32 pixels, every operand a multiple of 256.  Distance to the fp32
    oracle: 5e-2, or twice the helper's own where that exceeds it -- measured on the CPU for
    these four configurations the helper's logits lie 6.9e-3, 1.3e-2, 1.0e-2 and 7.4e-3 from the
    fp32 oracle, so 5e-2 holds for all four (base 256's distances, gradients 2.0e-1 by norm, lie
    below (64, 5)'s 4.2e-1, so the bars test_res_bf16_default_tiles_at_size takes as the largest
    over CONFIGS are what they were)."""
    cfg = (base, depth, size)
    r32, r64, plain, _, P, x, t = R.oracles(*cfg)
    sl, sg, dl, dg = _distances(cfg)
    bar32 = _fp32_bar(cfg)  # before the GPU is used
    m = _model(P, base, depth)
    lg, grads, _, loss = _step(m, x, t)
    e_l = rel_max(lg.cpu().numpy(), r32["logits"].numpy())
    e_l32 = rel_max(lg.cpu().numpy(), plain["logits"].numpy())
    errs = grad_errors(m, r32["grads"])
    worst = max(errs, key=errs.get)
    print(f"res bf16 {cfg}: logits vs helper {e_l:.2e} (spread {sl:.2e}), vs fp32 oracle "
          f"{e_l32:.2e} (helper {dl:.2e}, bar {bar32:.2e}); worst grad {worst} {errs[worst]:.2e} "
          f"(envelope {2 * sg:.2e}); loss {loss:.6f} vs {r32['loss'].item():.6f}")
    assert e_l <= 2 * sl + 1e-4
    assert abs(loss - r32["loss"].item()) <= 1e-3
    assert errs[worst] <= 2 * sg, f"{worst}: {errs[worst]:.3e}"
    assert e_l32 <= bar32


def test_res_bf16_deterministic():
    """Two bf16 steps from the same state: bit-identical logits, gradients and buffers."""
    P, x, t = R.oracles(64, 3, 64)[4:]
    outs = [_step(_model(P, 64, 3), x, t) for _ in range(2)]
    _assert_same(outs[0], outs[1], "repeat")


def test_res_bf16_tile_choice_is_invisible():
    """ResUNet(128, 3) at 64^2: the 1x1 skip GEMMs (E_RESID forward, E_STORE input gradient) and
    conv1's E_ADD input gradient on each one-tap LDS-DMA tile they can take (0 = 128x128,
    2 = 256x128, 4 = 256x256 where N divides 256, 6 = 512x128) and on the runtime's own choice:
    one training step is bit-identical (the epilogues are those of gemm_common.h, the K order is
    shared).  The tap-row halo tile sums K in another order and is off here, as in
    test_gpu_mod.py::test_rg16_tile_choice_is_numerically_invisible."""
    P, x, t = R.oracles(128, 3, 64)[4:]
    outs = {}
    for tile in (0, 2, 4, 6, -1):
        m = _model(P, 128, 3)
        with options(m.flatten_().rt, rg16_tile=tile, rg16_r3=0):
            outs[tile] = _step(m, x, t)
        del m
    for tile in (2, 4, 6, -1):
        _assert_same(outs[0], outs[tile], f"tile {tile} vs 0")


def test_res_bf16_default_tiles_at_size():
    """ResUNet(64, 4), bs 2, at 512^2: by the per-GEMM rule (runtime.hip rg16_tile) the network
    takes tiles {2, 4, 6, 19, 20} at 512^2, bs 16; at bs 2 no smaller H = W takes all five (384:
    {0, 2, 4, 6}, 256: {0, 2, 6, 20}; the 256x256 halo tile 19 needs 256 blocks of a 256-output
    3x3 GEMM, i.e. level 2 at 512^2), and 512^2 takes {0, 2, 4, 6, 19, 20}.  Logits and gradients
    must stay within bf16 distance of the same network in fp32 on the device: twice the largest
    fp32-vs-bf16 distance the helper shows over the oracle test's configurations (logits;
    gradients by norm).  Wrong large-M index arithmetic shows as O(1) errors."""
    bars = [_distances(c) for c in CONFIGS]
    bar_l, bar_g = 2 * max(b[2] for b in bars), 2 * max(b[3] for b in bars)
    x, t = inputs(7, 2, 512, 512)
    P = MO.res_make_params(11, 64, 4)
    a = _step(_model(P, 64, 4, "bf16"), x, t)
    b = _step(_model(P, 64, 4, "fp32"), x, t)
    e_l = rel_max(a[0].cpu().numpy(), b[0].cpu().numpy())
    errs = {k: norm_rel(a[1][k].cpu(), b[1][k].cpu()) for k in a[1]}
    worst = max(errs, key=errs.get)
    print(f"ResUNet(64, 4) 512^2 bf16 vs fp32: logits {e_l:.2e} (bar {bar_l:.2e}); worst grad "
          f"{worst} {errs[worst]:.2e} (bar {bar_g:.2e})")
    assert torch.isfinite(a[0]).all()
    assert e_l <= bar_l
    assert errs[worst] <= bar_g, f"{worst}: {errs[worst]:.3e}"


def test_res_bf16_eval_and_bn_buffers():
    """After one bf16 training step: running_mean / running_var against the helper at the f32
    tests' 1e-4 (rtol = atol) widened by the helper's own spread on the logits (the batch
    statistics carry the same bf16 rounding flips), num_batches_tracked, and the eval-mode
    forward against the helper in eval mode from this path's parameters and buffers (bar: twice
    the helper's fp32-vs-fp64 spread in eval mode + 1e-4)."""
    cfg = (64, 3, 64)
    r32, r64, _, B32, P, x, t = R.oracles(*cfg)
    sl = _distances(cfg)[0]
    m = _model(P, 64, 3)
    _step(m, x, t)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    tol = 1e-4 + 2 * sl
    for name, _ in MO.res_bn_layers(64, 3):
        for s in ("running_mean", "running_var"):
            ref = B32[f"{name}.{s}"]
            err = (sd[f"{name}.{s}"] - ref).abs().max().item()
            assert err <= tol * (1 + ref.abs().max().item()), (name, s, err)
        assert int(sd[f"{name}.num_batches_tracked"]) == 1
    Pc = {k: v.detach().cpu().clone() for k, v in m.named_parameters()}
    Bc = {k: v.detach().cpu().clone() for k, v in m.named_buffers()}
    fwd = R.make_res_forward(3, bf16=True)
    with torch.no_grad():
        e32 = fwd(x, Pc, Bc, False)
        e64 = fwd(x.double(), R.to64(Pc), R.to64(Bc), False)
    m.eval()
    with torch.no_grad():
        lg = m(x.to(DEV)).cpu()
    m.train()
    spread = rel_max(e32.numpy(), e64.numpy())
    err = rel_max(lg.numpy(), e32.numpy())
    print(f"eval: logits vs helper {err:.2e} (helper spread {spread:.2e})")
    assert err <= 2 * spread + 1e-4


def test_res_bf16_fused_adamw_repack_state():
    """Two HipAdamW steps on ResUNet(64, 3, bf16).  Path A: the fused AdamW + repack, the next
    forward reading the context's weight images.  Path B: the arena declared changed after each
    step, so the forward rebuilds every image.  The second-step logits are bit-identical: no
    skip weight image (plain or transposed) is stale on either path."""
    import unet_hip
    P, x, t = R.oracles(64, 3, 64)[4:]
    out = {}
    for path in "AB":
        m = _model(P, 64, 3)
        opt = unet_hip.HipAdamW(m.parameters(), lr=1e-3)
        for s in range(2):
            r = _step(m, x, t)
            opt.step()
            if path == "B":
                m.flatten_().images_stale()
        out[path] = (_step(m, x, t), r)
        del m, opt
    assert torch.equal(out["A"][1][0], out["B"][1][0]), "second-step logits"
    _assert_same(out["A"][0], out["B"][0], "third forward / backward")


def test_res_fp32_untouched_by_bf16_in_process():
    """ResUNet(64, 3) in fp32, one step, before and after a bf16 ResUNet of the same width ran
    in the same process: bit-identical."""
    P, x, t = R.oracles(64, 3, 64)[4:]
    a = _step(_model(P, 64, 3, "fp32"), x, t)
    _step(_model(P, 64, 3, "bf16"), x, t)
    b = _step(_model(P, 64, 3, "fp32"), x, t)
    _assert_same(a, b, "fp32 before / after bf16")
