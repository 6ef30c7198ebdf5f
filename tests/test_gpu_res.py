"""GPU parity of models/mod.py:ResUNet (mod.py:71-131, the network the reference's
main.py:122 builds): residual blocks ReLU(Conv-BN-ReLU-Conv-BN(x) + Conv1x1(x)), closed by
the skip GEMM's E_RESID epilogue, with the skip's input gradient added to conv1's (E_ADD).
Oracle: oracle/mod_ref_cpu.py (make_res_forward), pinned by tests/golden/res_d3_64.npz
from the reference module.  Bars as tests/test_gpu_parity.py."""
import os

import numpy as np
import pytest
import torch

from _helpers import check_eval, grad_errors, inputs, masks_agree, norm_rel, rel_max, strict_resync_steps
from oracle import mod_ref_cpu as MO
from oracle import weights as Wt

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LOGIT_TOL = 1e-4
GRAD_TOL = 1e-2


@pytest.fixture(autouse=True, scope="module")
def _threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def _model(P, base, depth):
    import unet_hip
    m = unet_hip.ResUNet(1, 1, base_filters=base, depth=depth)
    sd = m.state_dict()
    for k, v in P.items():
        sd[k] = v.clone()
    for k, v in MO.res_init_buffers(base, depth).items():
        sd[k] = v.clone()
    m.load_state_dict(sd)
    return m.to(DEV).train()


def test_res_train_steps_match_golden(golden_dir):
    import unet_hip
    f = np.load(os.path.join(golden_dir, "res_d3_64.npz"), allow_pickle=False)
    m = _model(MO.res_make_params(42, 64, 3), 64, 3)
    opt = unet_hip.HipAdamW(m.parameters(), lr=1e-4)
    x = torch.from_numpy(Wt.make_input(13, 2, 1, 64, 64)).to(DEV)
    t = torch.from_numpy(Wt.make_target(13, 2, 64, 64)).to(DEV)
    spec = MO.res_param_spec(1, 1, 64, 3)
    names = [n for n, _ in MO.res_bn_layers(64, 3)]
    for s in range(2):
        p = f"s{s}_"
        tol = LOGIT_TOL if s == 0 else 2e-3
        opt.zero_grad()
        logits = m(x)
        losses = unet_hip.seg_losses(logits, t)
        (losses[0] + losses[1]).backward()
        opt.step()
        ref = f[p + "logits"]
        lg = logits.detach().cpu().numpy()
        assert rel_max(lg, ref) <= tol, f"{p} logits {rel_max(lg, ref):.2e}"
        ok, nd = masks_agree((torch.sigmoid(logits) > 0.5).cpu().numpy().astype(np.uint8),
                             f[p + "mask"], ref, 10 * tol * np.abs(ref).max())
        assert ok, f"{p}: {nd} mask bits differ away from the decision boundary"
        assert abs(losses[0].item() - float(f[p + "bce"])) <= (1e-5 if s == 0 else 1e-4)
        assert abs(losses[1].item() - float(f[p + "dice"])) <= (1e-5 if s == 0 else 1e-4)
        gtol = GRAD_TOL if s == 0 else 10 * GRAD_TOL
        named = dict(m.named_parameters())
        norms, samp = f[p + "grad_norm"], f[p + "grad_samp"]
        for ti, item in enumerate(spec):
            g = named[item[0]].grad.detach().double().cpu().reshape(-1)
            idx = np.floor(Wt.uniform(7, 3000 + ti, 64) * g.numel()).astype(np.int64)
            assert abs(g.norm().item() - norms[ti]) <= gtol * norms[ti], f"{p} {item[0]} norm"
            assert np.max(np.abs(g[idx].numpy() - samp[ti])) <= gtol * norms[ti], f"{p} {item[0]}"
        sd = m.state_dict()
        rm = torch.cat([sd[f"{n}.running_mean"].cpu() for n in names]).numpy()
        rv = torch.cat([sd[f"{n}.running_var"].cpu() for n in names]).numpy()
        btol = 1e-4 if s == 0 else 1e-3
        np.testing.assert_allclose(rm, f[p + "running_mean"], rtol=btol, atol=btol)
        np.testing.assert_allclose(rv, f[p + "running_var"], rtol=btol, atol=btol)
    # eval mode (Trainer.validate / test, utils/trainer.py:130,206-250): the oracle resynced
    # from this path's parameters and running statistics, at the north-star bar
    check_eval(m, MO.make_res_forward(3), x.cpu(), t.cpu())


def test_res_train_steps_strict_resync():
    """Three AdamW steps (lr 1e-4) of ResUNet(base 64, depth 3) -- the block structure of
    the network the reference main.py:122 trains -- with the oracle restarted from this
    path's parameters, running statistics and Adam moments at every step: logits at 1e-4
    and gradients within the fp64 envelope at every step.  Later-step floor 2e-2: one ReLU
    input crossing zero moves a small residual-block BN-bias gradient by up to 1.5e-2 in
    this network (measured on the fp32 oracle alone; here step 2 moves
    decoders.0.conv.1.bias by 1.1e-2 while the median tensor stays at fp32 rounding)."""
    x, t = inputs(13, 2, 64, 64)
    m = _model(MO.res_make_params(42, 64, 3), 64, 3)
    strict_resync_steps(m, lambda P_, B_, o, x_, t_: MO.res_train_step(P_, B_, o, x_, t_, depth=3), x, t,
                        floor=2e-2)


def _to64(d):
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in d.items()}


@pytest.mark.parametrize("base,depth,size", [(64, 3, 64), (64, 5, 128), (32, 4, 64), (16, 4, 64)])
def test_res_full_grads_vs_oracle(base, depth, size):
    """Every element of every gradient vs the oracle (depth 5 = the reference default).

    Deep levels are small: at depth 5 the bottleneck's BatchNorm sees (size/32)^2 pixels x
    2 images per channel (8 values at 64x64, where two of its ReLU inputs lie within 1e-5
    of zero and a single fp32 mask flip moves that BN's bias gradient by ~1e-2), so depth 5
    runs at 128x128 and gradients are judged against the fp64 oracle, within 2x the fp32
    oracle's own worst per-tensor error, floored at the usual 1e-2.  That
    fp32 error is taken over two evaluations, of x and of x * (1 + 1e-7): a 1-ulp-scale
    input change flips such near-zero masks too (base 64 depth 3: the bottleneck's
    conv.1 bias gradient goes from 2.7e-3 to 1.5e-2 off fp64 in the oracle itself)."""
    import unet_hip
    from _helpers import options
    P = MO.res_make_params(9, base, depth)
    x, t = inputs(4, 2, size, size)
    ref = MO.res_train_step(P, MO.res_init_buffers(base, depth), None, x, t, depth=depth)
    refp = MO.res_train_step(P, MO.res_init_buffers(base, depth), None, x * (1 + 1e-7), t,
                             depth=depth)
    r64 = MO.res_train_step(_to64(P), _to64(MO.res_init_buffers(base, depth)), None, x.double(),
                            t.double(), depth=depth)
    m = _model(P, base, depth)
    with options(m.flatten_().rt):
        logits = m(x.to(DEV))
        losses = unet_hip.seg_losses(logits, t.to(DEV))
        (losses[0] + losses[1]).backward()
    assert rel_max(logits.detach().cpu().numpy(), ref["logits"].numpy()) <= LOGIT_TOL
    e32 = {k: max(norm_rel(g, r64["grads"][k]), norm_rel(refp["grads"][k], r64["grads"][k]))
           for k, g in ref["grads"].items()}
    env = max(2 * max(e32.values()), GRAD_TOL)
    errs = grad_errors(m, r64["grads"])
    worst = max(errs, key=errs.get)
    assert errs[worst] <= env, f"{worst}: {errs[worst]:.3e} (fp32 oracle {e32[worst]:.3e})"


def test_res_narrow_b16_matches_golden(golden_dir):
    """ResUNet(base 16, depth 3) -- the smallest width of the reference grid -- one step vs
    tests/golden/mod_narrow_64.npz (channels zero-padded to 64 inside the library)."""
    import unet_hip
    f = np.load(os.path.join(golden_dir, "mod_narrow_64.npz"), allow_pickle=False)
    m = _model(MO.res_make_params(42, 16, 3), 16, 3)
    x = torch.from_numpy(Wt.make_input(31, 2, 1, 64, 64)).to(DEV)
    t = torch.from_numpy(Wt.make_target(31, 2, 64, 64)).to(DEV)
    logits = m(x)
    losses = unet_hip.seg_losses(logits, t)
    (losses[0] + losses[1]).backward()
    assert rel_max(logits.detach().cpu().numpy(), f["r16_logits"]) <= LOGIT_TOL
    assert abs((losses[0] + losses[1]).item() - float(f["r16_loss"])) <= 1e-5
    for ti, (name, p) in enumerate(m.named_parameters()):
        n = p.grad.detach().double().norm().item()
        assert abs(n - f["r16_grad_norm"][ti]) <= GRAD_TOL * f["r16_grad_norm"][ti], name
    check_eval(m, MO.make_res_forward(3), x.cpu(), t.cpu())


def _f32_step(m, x, t):
    import unet_hip
    logits = m(x.to(DEV))
    losses = unet_hip.seg_losses(logits, t.to(DEV))
    (losses[0] + losses[1]).backward()
    torch.cuda.synchronize()
    return (logits.detach().clone(),
            {k: p.grad.detach().clone() for k, p in m.named_parameters()},
            {k: b.detach().clone() for k, b in m.named_buffers()})


@pytest.mark.parametrize("net,base,ref,alt", [
    ("res", 32, dict(tile_n32=14), dict(tile_n32=15)),
    ("mod", 32, dict(tile_n32=14), dict(tile_n32=15)),
    ("res", 16, dict(tile_n32=14), dict(tile_n32=15)),  # two 32-channel levels (0 padded)
])
def test_direct_tiles_bit_identical(net, base, ref, alt):
    """Row GEMMs on the direct-from-global tile (kernels_gemm.hip rowgemm_direct_kernel, tile
    15: MFMA operands straight from global memory into registers) against the LDS-staged tile
    14 (256 x 32): same K order and MFMA sequence per element, same epilogues (forward BN
    statistics, dgrad BN partials, residual add, 1x1 skip, ConvT), so one training step of a
    ResUNet / mod.py UNet at that width is bit-identical (base 16: levels 0 (padded 16 -> 32) and
    1 run 32 channels; since r06 no level runs 96: it pads to 128 for the x3 GEMMs)."""
    from _helpers import hip_mod_model, options
    x, t = inputs(61, 2, 128, 128)
    outs = []
    for opts in (ref, alt):
        if net == "res":
            m = _model(MO.res_make_params(67, base, 3), base, 3)
        else:
            m = hip_mod_model(MO.make_params(67, base, 3), DEV, base, 3)
        with options(m.flatten_().rt, **opts):
            outs.append(_f32_step(m, x, t))
        del m
    a, b = outs
    assert torch.equal(a[0], b[0]), "logits"
    for k, g in a[1].items():
        assert torch.equal(g, b[1][k]), f"grad {k}"
    for k, v in a[2].items():
        assert torch.equal(v, b[2][k]), f"buffer {k}"


@pytest.mark.parametrize("net,base", [("res", 32), ("mod", 32), ("mod", 64)])
def test_dz_in_wgrad_bn_relu_bit_identical(net, base):
    """Option dz_in_wgrad on the BN -> ReLU networks (r04; models/mod.py UNet and ResUNet,
    f32): the weight gradient's B' loader forms dz = A do + B (z - mean) + C unmasked (the
    producer of do already applied the ReLU mask), its first A'-tile blocks store it for the
    dgrad, and the bn_dz pass disappears -- the same bn_dz4 arithmetic, so one training step
    is bit-identical to the separate pass."""
    from _helpers import hip_mod_model, options
    x, t = inputs(71, 2, 128, 128)
    outs = []
    for flag in (0, 1 << 20):  # off / every layer (default: Cin <= 256)
        if net == "res":
            m = _model(MO.res_make_params(73, base, 3), base, 3)
        else:
            m = hip_mod_model(MO.make_params(73, base, 3), DEV, base, 3)
        with options(m.flatten_().rt, x3=0, dz_in_wgrad=flag):  # the f32 MFMA path's fusion
            outs.append(_f32_step(m, x, t))
        del m
    a, b = outs
    assert torch.equal(a[0], b[0]), "logits"
    for k, g in a[1].items():
        assert torch.equal(g, b[1][k]), f"grad {k}: {(g - b[1][k]).abs().max().item()}"
