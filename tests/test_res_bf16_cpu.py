"""ResUNet in bf16 math, host side: the test oracle (tests/res_bf16_ref.py) against
oracle/mod_ref_cpu.py, the configurations unet_create takes, and the Python / CLI surface."""
import pytest
import torch

import res_bf16_ref as R
from _helpers import inputs
from oracle import mod_ref_cpu as MO


def test_helper_without_bf16_is_the_res_oracle_bit_for_bit():
    """bf16=False: logits and every gradient equal MO.res_train_step exactly (base 64, depth 3,
    B = 2, 64x64), so the helper differs from the oracle by its roundings alone."""
    x, t = inputs(5, 2, 64, 64)
    P = MO.res_make_params(42, 64, 3)
    a = R.res_train_step(P, MO.res_init_buffers(64, 3), None, x, t, 3, bf16=False)
    b = MO.res_train_step(P, MO.res_init_buffers(64, 3), None, x, t, depth=3)
    assert torch.equal(a["logits"], b["logits"])
    assert torch.equal(a["loss"], b["loss"])
    assert set(a["grads"]) == set(b["grads"])
    for k, g in b["grads"].items():
        assert torch.equal(a["grads"][k], g), k


def test_create_res_bf16_widths():
    """unet_create(RES, BF16): real base_filters 64 / 128 / 256 are supported, with the f32
    context's parameter and BN tables; padded or narrow bases are refused."""
    from unet_hip import _lib
    from unet_hip.runtime import UNetRuntime
    for base in (64, 128, 256):
        a = UNetRuntime("cpu", 1, 1, _lib.VARIANT_RES, base, 3, _lib.MATH_BF16)
        b = UNetRuntime("cpu", 1, 1, _lib.VARIANT_RES, base, 3, _lib.MATH_F32)
        assert a.params == b.params and a.n_param_floats == b.n_param_floats
        assert a.bn == b.bn and a.n_bn_floats == b.n_bn_floats
    for base in (16, 32, 48):
        with pytest.raises(_lib.HipError, match="UNSUPPORTED"):
            UNetRuntime("cpu", 1, 1, _lib.VARIANT_RES, base, 3, _lib.MATH_BF16)


def test_res_unet_mfma_dtype_argument():
    import unet_hip
    from unet_hip import _lib
    assert unet_hip.ResUNet(depth=1).mfma_dtype == "fp32"
    assert unet_hip.ResUNet(depth=1)._native_cfg()[-1] == _lib.MATH_F32
    m = unet_hip.ResUNet(depth=1, mfma_dtype="bf16")
    assert m.mfma_dtype == "bf16" and m._native_cfg()[-1] == _lib.MATH_BF16
    assert unet_hip.ResUNet(depth=1, mfma_dtype=torch.bfloat16).mfma_dtype == "bf16"
    with pytest.raises(ValueError):
        unet_hip.ResUNet(depth=1, mfma_dtype="bogus")
    from models.mod import ResUNet
    assert ResUNet(depth=1, mfma_dtype="bf16").mfma_dtype == "bf16"


def test_main_mfma_flag():
    import main
    assert main.get_parser([]).mfma == "fp32"
    assert main.get_parser(["--mfma", "bf16"]).mfma == "bf16"
    a = main.get_parser(["--use_amp_autocast", "1"])
    assert a.use_amp_autocast and a.mfma == "fp32"
    with pytest.raises(SystemExit):
        main.get_parser(["--mfma", "fp16"])
