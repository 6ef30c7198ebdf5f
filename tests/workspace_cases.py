"""The case table of the workspace-contract tests (tests/test_gpu_workspace.py and the planner
checks of tests/test_lib_cpu.py) and the probe that finds, per case, the schedule-option settings
that change the workspace plan.  Nothing here touches a device: a context is created and
unet_workspace_size / unet_set_option / unet_get_option are host logic.

A case is the smallest shape at which one of make_plan's roundings (csrc/runtime.hip) differs:
(P + 63) / 64 against P / 64 + 1 rows, pixel counts below the 128- and 256-row tiles, channel
padding at one or several levels, the bf16 / x3 operand images, the residual blocks' extra
buffers, the multi-class head's partials."""
from collections import namedtuple

Case = namedtuple("Case", "net math base depth out_ch N H W why")

CASES = [
    Case("model", "fp32", 64, 4, 1, 3, 48, 80,
         "P = 11520, 2880, 720, 180, 45: below the 128- / 256-row tiles from level 1 on, no "
         "multiple of 64 from level 2 on, odd N"),
    Case("model", "fp32", 64, 4, 4, 2, 16, 32, "smallest legal plane; multi-class head (hpart)"),
    Case("mod", "fp32", 64, 3, 1, 1, 16, 48, "N = 1, W = 24 at level 1: no multiple of 16"),
    Case("mod", "fp32", 16, 1, 2, 2, 16, 16, "depth 1; level 0 padded to 32 (pprm, pbn, pgrad)"),
    Case("mod", "fp32", 24, 4, 1, 2, 32, 48, "24 -> 32, 64, 96, 192: padding at several levels"),
    Case("mod", "fp32", 48, 6, 1, 2, 64, 128, "depth 6, 48 -> 64, 96, ..."),
    Case("mod", "bf16", 64, 3, 1, 3, 48, 80, "s16, x16, t16, the LDS-DMA zero page"),
    Case("mod", "bf16", 128, 3, 1, 3, 48, 80, "s16, x16, t16, the LDS-DMA zero page"),
    Case("res", "fp32", 64, 3, 1, 3, 48, 80, "g[2], out[], the 1x1 skip slabs"),
    Case("res", "fp32", 32, 4, 1, 2, 32, 48, "narrow residual, x3 only on the wide levels"),
    Case("res", "fp32", 16, 4, 1, 2, 32, 48, "narrow residual, level 0 padded"),
    Case("res", "bf16", 64, 3, 1, 2, 16, 32, "r16, the skip images"),
    Case("res", "bf16", 128, 3, 1, 2, 16, 32, "r16, the skip images"),
]

# Shapes below the library's shape contract (H and W multiples of max(16, 2**depth),
# include/unet_hip.h): refused with UNET_ERR_SHAPE before the workspace is looked at.  The three
# cases above at 16 x 48 and 48 x 80 are the nearest legal shapes with the same properties
# (N = 1 and a level-1 width that is no multiple of 16; odd N and the pixel counts 2880, 720, 180).
REFUSED_SHAPES = [
    Case("mod", "fp32", 64, 3, 1, 1, 16, 24, "W = 24"),
    Case("mod", "bf16", 64, 3, 1, 3, 24, 40, "H = 24, W = 40"),
    Case("mod", "bf16", 128, 3, 1, 3, 24, 40, "H = 24, W = 40"),
    Case("res", "fp32", 64, 3, 1, 3, 24, 40, "H = 24, W = 40"),
]

# The alternative values the GPU suite runs each schedule option at (test_gpu_parity.py,
# test_gpu_mod.py, test_gpu_res.py, test_gpu_res_bf16.py, test_gpu_x3.py, test_gpu_head_classes.py):
# the values known to be legal.  An option that is not listed is probed at no other value.
OPTION_VALUES = {
    "x3": (0, 1), "x3_tile": (-1, 0, 1, 2), "x3_n64": (2, 3), "x3_r3": (0, 1), "x3_wtile": (-1, 1),
    "head_fuse": (0, 1), "pool_fuse": (0, 1), "tile_group": (0, 1), "convt16": (0, 1),
    "rg16": (0, 1), "wg16": (0, 1), "rg16_tile": (-1, 0, 2, 4, 6, 19, 20), "wg16_tile": (0, 2),
    "wg16_r3": (0, 4, 7), "rg16_r3": (0, 1), "tile_n32": (14, 15),
    "dz_in_wgrad": (0, 256, 1 << 20), "wgrad_row3": (0, 1),
    "tile_n128": (-1, 4, 18), "tile_n128_dgrad": (-1, 0, 4, 18), "tile_n64": (1, 19, 25, 26),
    "tile_n64_dgrad": (1, 19, 25, 26), "tile_convt64": (1, 19, 25, 26),
    "tile_convt_dgrad": (0, 18, 25, 26),
}

# Settings every f32 case runs whether or not they move the plan's size: they change which
# regions are written and read (x3 images, the fused dz, the bf16 ConvT / row-GEMM paths, the
# fused head and pool passes, the tap-row weight gradient).
F32_ALWAYS = ("x3=0", "dz_in_wgrad=toggle", "convt16=toggle", "rg16=toggle", "head_fuse=toggle",
              "pool_fuse=toggle", "wgrad_row3=0")


def case_id(c):
    return f"{c.net}-{c.math}-b{c.base}d{c.depth}-o{c.out_ch}-{c.N}x{c.H}x{c.W}"


def runtime(c, device="cuda:0"):
    """The cached UNetRuntime of a case's configuration (creating one does no device work)."""
    from unet_hip import _lib
    from unet_hip.runtime import UNetRuntime
    math = _lib.MATH_BF16 if c.math == "bf16" else _lib.MATH_F32
    if c.net == "model":
        return UNetRuntime.get(device, 1, c.out_ch, _lib.VARIANT_MODEL, 0, 0, math)
    variant = _lib.VARIANT_RES if c.net == "res" else _lib.VARIANT_MOD
    return UNetRuntime.get(device, 1, c.out_ch, variant, c.base, c.depth, math)


def _sizes(rt, c):
    return rt.workspace_bytes(c.N, c.H, c.W, True), rt.workspace_bytes(c.N, c.H, c.W, False)


def option_settings(c):
    """[{}, {name: value}, ...]: the default options, then every single-option setting that
    changes the training or the inference workspace size of case c (probed over every name of
    unet_option_name and its values in OPTION_VALUES), then, for an f32 case, the F32_ALWAYS
    settings not already found.  The runtime's options are left as they were."""
    from unet_hip import _lib
    rt = runtime(c)
    base = _sizes(rt, c)
    out = [{}]
    for name in _lib.option_names():
        old = rt.get_option(name)
        for v in OPTION_VALUES.get(name, ()):
            if v == old:
                continue
            rt.set_option(name, v)
            try:
                moved = _sizes(rt, c) != base
            finally:
                rt.set_option(name, old)
            if moved:
                out.append({name: v})
    if c.math == "fp32":
        for spec in F32_ALWAYS:
            name, v = spec.split("=")
            v = int(not rt.get_option(name)) if v == "toggle" else int(v)
            if {name: v} not in out and rt.get_option(name) != v:
                out.append({name: v})
    return out


def settings_id(kv):
    return ",".join(f"{k}={v}" for k, v in kv.items()) or "default"
