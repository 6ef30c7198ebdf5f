"""The multi-class head (out_channels 2..4) of models/mod.py UNet and ResUNet on the HIP path:
head_fwd_kernel / head_bwd_kernel with O > 1 on the BN -> ReLU order (masked `do`), the ResUNet
head, the unfused `do` feeding the last conv's dz pass in bf16 math (the head fusion is off for
out_channels != 1), and the channel-padded widths (an (O, base) head weight through
pad_copy_kernel).

One training forward + backward, loss = bce + dice through unet_hip.seg_losses (the classes are
flattened per sample, models/loss.py:19-20, as oracle/unet_ref_cpu.py:dice_loss does), at
N = 3, H = 32, W = 48, depth 2: non-square (HW != P / N), several images (the NCHW index
(img * O + o) * HW + hw), and a pixel count that leaves head_bwd blocks without pixels.
Targets (N, O, H, W) are hard, ~30 % positive and differ per class.

References and bars are those of the single-class tests of the same network, unchanged:
* f32: oracle/mod_ref_cpu.py in fp32 and fp64; logits at LOGIT_TOL, loss at 1e-5, every gradient
  against fp64 within 2x the fp32 oracle's own deviation over x and x * (1 + 1e-7), floor 1e-2
  (tests/test_gpu_res.py, test_gpu_mod.py::test_mod_narrow_full_grads_vs_fp64);
* bf16: the bf16 oracles (mod_ref_cpu bf16=True, tests/res_bf16_ref.py) at the bars of
  test_mod_bf16_matches_bf16_oracle / test_res_bf16_matches_bf16_oracle: logits 2x the oracle's
  fp32-vs-fp64 spread + 1e-4, loss 1e-3, gradients 2x the largest spread, and 5e-2 from the
  fp32 oracle (ResUNet: or twice the helper's own distance where that exceeds it).
A per-tensor norm can hide one wrong class, so the same bars also judge rel_max of the logits of
each class channel (bf16: the oracle's spread on that channel), norm_rel of each row
final_conv.weight.grad[o] and each element of final_conv.bias.grad."""
import os

import numpy as np
import pytest
import torch

import res_bf16_ref as R
from _helpers import grad_errors, norm_rel, options, rel_max
from oracle import mod_ref_cpu as MO
from oracle import weights as Wt

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LOGIT_TOL = 1e-4
GRAD_TOL = 1e-2
N, H, W, DEPTH = 3, 32, 48, 2


@pytest.fixture(autouse=True, scope="module")
def _threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def _to64(d):
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in d.items()}


def _data(O):
    x = torch.from_numpy(Wt.make_input(21, N, 1, H, W))
    t = (torch.rand(N, O, H, W, generator=torch.Generator().manual_seed(40 + O)) > 0.7).float()
    return x, t


def _params(net, base, O):
    make = MO.res_make_params if net == "res" else MO.make_params
    return make(19, base, DEPTH, out_channels=O)


def _buffers(net, base):
    return (MO.res_init_buffers if net == "res" else MO.init_buffers)(base, DEPTH)


def _oracle_step(net, base, bf16, P, x, t):
    B = _buffers(net, base)
    if P["final_conv.bias"].dtype == torch.float64:
        B = _to64(B)
    if net == "res":
        return R.res_train_step(P, B, None, x, t, DEPTH, bf16=bf16)
    return MO.train_step(P, B, None, x, t, depth=DEPTH, bf16=bf16)


_ORACLES = {}


def _oracles(net, base, O, bf16):
    """The oracle evaluations of one configuration, computed once and shared: do not modify.
    f32: (fp32, fp32 of x * (1 + 1e-7), fp64); bf16: (bf16 fp32, bf16 fp64, plain fp32)."""
    key = (net, base, O, bf16)
    if key not in _ORACLES:
        P = _params(net, base, O)
        x, t = _data(O)
        if bf16:
            _ORACLES[key] = (_oracle_step(net, base, True, P, x, t),
                             _oracle_step(net, base, True, _to64(P), x.double(), t.double()),
                             _oracle_step(net, base, False, P, x, t))
        else:
            _ORACLES[key] = (_oracle_step(net, base, False, P, x, t),
                             _oracle_step(net, base, False, P, x * (1 + 1e-7), t),
                             _oracle_step(net, base, False, _to64(P), x.double(), t.double()))
    return _ORACLES[key]


def _model(net, base, O, math):
    import unet_hip
    cls = unet_hip.ResUNet if net == "res" else unet_hip.ModUNet
    m = cls(1, O, base_filters=base, depth=DEPTH, mfma_dtype=math)
    sd = m.state_dict()
    for k, v in _params(net, base, O).items():
        sd[k] = v.clone()
    for k, v in _buffers(net, base).items():
        sd[k] = v.clone()
    m.load_state_dict(sd)
    return m.to(DEV).train()


def _step(net, base, O, math, **opts):
    import unet_hip
    x, t = _data(O)
    m = _model(net, base, O, math)
    with options(m.flatten_().rt, **opts):
        logits = m(x.to(DEV))
        assert logits.shape == (N, O, H, W)
        losses = unet_hip.seg_losses(logits, t.to(DEV))
        loss = losses[0] + losses[1]
        loss.backward()
        torch.cuda.synchronize()
    return m, logits.detach().cpu(), loss.item()


def _head_errors(m, ref_grads):
    """norm_rel of each row of final_conv.weight.grad and the relative error of each element of
    final_conv.bias.grad: {name: error}."""
    gw = m.final_conv.weight.grad.detach().cpu()
    gb = m.final_conv.bias.grad.detach().cpu().double()
    rw, rb = ref_grads["final_conv.weight"], ref_grads["final_conv.bias"].double()
    out = {f"final_conv.weight[{o}]": norm_rel(gw[o], rw[o]) for o in range(gw.shape[0])}
    for o in range(gb.numel()):
        out[f"final_conv.bias[{o}]"] = abs(gb[o].item() - rb[o].item()) / max(abs(rb[o].item()), 1e-30)
    return out


F32_CASES = [("mod", 64, {}), ("mod", 64, {"x3": 0}), ("mod", 16, {}), ("mod", 48, {}),
             ("res", 64, {}), ("res", 64, {"x3": 0}), ("res", 16, {}), ("res", 48, {})]


@pytest.mark.parametrize("O", [2, 3, 4])
@pytest.mark.parametrize("net,base,opts", F32_CASES,
                         ids=[f"{n}{b}{'-x3off' if o else ''}" for n, b, o in F32_CASES])
def test_head_classes_f32(net, base, opts, O):
    ref, refp, r64 = _oracles(net, base, O, False)
    m, lg, loss = _step(net, base, O, "fp32", **opts)
    e_l = rel_max(lg.numpy(), ref["logits"].numpy())
    e_c = [rel_max(lg[:, o].numpy(), ref["logits"][:, o].numpy()) for o in range(O)]
    e32 = {k: max(norm_rel(g, r64["grads"][k]), norm_rel(refp["grads"][k], r64["grads"][k]))
           for k, g in ref["grads"].items()}
    env = max(2 * max(e32.values()), GRAD_TOL)
    errs = grad_errors(m, r64["grads"])
    worst = max(errs, key=errs.get)
    herr = _head_errors(m, r64["grads"])
    hworst = max(herr, key=herr.get)
    print(f"{net} base {base} {opts} O={O}: logits {e_l:.2e}, per class {max(e_c):.2e}; loss "
          f"{loss:.6f} vs {ref['loss'].item():.6f}; worst grad {worst} {errs[worst]:.2e}, head "
          f"{hworst} {herr[hworst]:.2e} (envelope {env:.2e})")
    assert e_l <= LOGIT_TOL
    assert max(e_c) <= LOGIT_TOL, f"class {int(np.argmax(e_c))}: {max(e_c):.3e}"
    assert abs(loss - ref["loss"].item()) <= 1e-5
    assert errs[worst] <= env, f"{worst}: {errs[worst]:.3e} (fp32 oracle {e32[worst]:.3e})"
    assert herr[hworst] <= env, f"{hworst}: {herr[hworst]:.3e}"


@pytest.mark.parametrize("O", [2, 3, 4])
@pytest.mark.parametrize("net", ["mod", "res"])
def test_head_fuse_option_is_inert_for_several_classes(net, O):
    """out_channels != 1 already turns the head fusion off, so head_fuse = 0 changes nothing:
    logits and every gradient bit-identical to the default (f32, base 64)."""
    a, la, _ = _step(net, 64, O, "fp32")
    b, lb, _ = _step(net, 64, O, "fp32", head_fuse=0)
    assert torch.equal(la, lb), "logits"
    gb = dict(b.named_parameters())
    for k, p in a.named_parameters():
        assert torch.equal(p.grad, gb[k].grad), f"grad {k}"


@pytest.mark.parametrize("O", [2, 3, 4])
@pytest.mark.parametrize("net,base", [("mod", 64), ("mod", 128), ("res", 64)])
def test_head_classes_bf16(net, base, O):
    ref, r64, plain = _oracles(net, base, O, True)
    dl = rel_max(ref["logits"].numpy(), plain["logits"].numpy())
    bar32 = 5e-2 if (net == "mod" or dl < 5e-2) else 2 * dl  # before the GPU is used
    m, lg, loss = _step(net, base, O, "bf16")
    spread_l = rel_max(ref["logits"].numpy(), r64["logits"].numpy())
    e_l = rel_max(lg.numpy(), ref["logits"].numpy())
    e_l32 = rel_max(lg.numpy(), plain["logits"].numpy())
    spread = {k: norm_rel(ref["grads"][k], r64["grads"][k]) for k in ref["grads"]}
    env = 2 * max(spread.values())
    errs = grad_errors(m, ref["grads"])
    worst = max(errs, key=errs.get)
    herr = _head_errors(m, ref["grads"])
    hworst = max(herr, key=herr.get)
    print(f"bf16 {net} base {base} O={O}: logits vs bf16 oracle {e_l:.2e} (spread {spread_l:.2e}), "
          f"vs fp32 oracle {e_l32:.2e} (oracle {dl:.2e}, bar {bar32:.2e}); worst grad {worst} "
          f"{errs[worst]:.2e}, head {hworst} {herr[hworst]:.2e} (envelope {env:.2e}); loss "
          f"{loss:.6f} vs {ref['loss'].item():.6f}")
    assert e_l <= 2 * spread_l + 1e-4
    for o in range(O):
        s_o = rel_max(ref["logits"][:, o].numpy(), r64["logits"][:, o].numpy())
        e_o = rel_max(lg[:, o].numpy(), ref["logits"][:, o].numpy())
        assert e_o <= 2 * s_o + 1e-4, f"class {o}: {e_o:.3e} (oracle spread {s_o:.3e})"
    assert abs(loss - ref["loss"].item()) <= 1e-3
    assert errs[worst] <= env, f"{worst}: {errs[worst]:.3e}"
    assert herr[hworst] <= env, f"{hworst}: {herr[hworst]:.3e}"
    assert e_l32 <= bar32
