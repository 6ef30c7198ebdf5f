"""Which GEMM kernels the production configurations launch (what bench.py times, and the bf16
residual network main.py trains), and the small fp64-checked cases that stand for them
(tests/test_gpu_kernel_coverage.py; helper of the tests, not a test; importable without a GPU).

runtime.hip chooses the kernel and tile of every conv / ConvT / skip GEMM in the plan, from the shape
and the CU count (plan_tiles: x3_pick, x3_wgrad_cfg, rg16_pick, wgrad_cfg, pick_tile, wg16_pick;
the tiles are the rows of csrc/tiles.h), by block-count thresholds the suite's 64^2 / 128^2 inputs never reach.  The
library reports every launch as ``family/kernel_tile|layer`` (rt.timing_records()).  `key`
reduces such a label to what a small case has to reproduce to stand for it:

    (family, kernel_tile, row_class)

row_class applies to the kernels that walk whole image rows -- the tap-row halo row GEMMs
(label ``...r3_BMxBN``: BM pixels per tile) and the tap-row weight gradients (``wx3r3``,
``wg16r3`` / ``wg16r3m``, ``wgrad3``: the pixels of one K chunk, 32 for the x3 and f32 kernels
-- the f32 label carries it -- and 64 for the bf16 kernel).  It is how the layer's row width
W >> level relates to that count, because these kernels take another path for each:
"lt" several image rows per tile, "eq", "gt" several tiles per image row.  Every other
kernel gets "-".  Split-K counts, XCD block order and tile grouping are not in the label and
not in the key (the bit-identity tests hold those).

PRODUCTION: the configurations bench.py can time, at its own batch and image sizes, and the two
bf16 ResUNet steps bench.py cannot (its --config res is f32 only): what main.py --model_type
ResUNet --mfma bf16 trains and tools/res_bf16_time.py times.
SMALL: the small cases; each forces the kernels under test through schedule options (the
forcing rules of runtime.hip accept any tile that fits) at the smallest shape at which the
kernel still meets its edges.
INFERENCE / SMALL_EVAL: the same pair for the eval-mode forward (tests/test_gpu_eval_coverage.py).
"""
import re

GEMM_FAMILIES = tuple(f"{a}_{b}" for a in ("conv", "convT", "skip") for b in ("fwd", "dgrad", "wgrad"))

# bench.py: config 2 = UNet, bs 32 at 256^2; config 4 = ModUNet(128, 5), bs 8 at 512^2, --mfma
# fp32 / bf16; --config res = ResUNet(--base, --depth), bs 16 at 512^2, f32 only (--mfma is
# config 4's): the reference grid's bases at depth 4 and bench.py's own default (64, 5).
# Not from bench.py: res64_bf16 / res64_d5_bf16, ResUNet(64, 4 / 5) with mfma_dtype="bf16" at
# main.py's default batch and size (main.py --model_type ResUNet --mfma bf16; the two steps
# tools/res_bf16_time.py times)
PRODUCTION = [
    dict(id="c2", net="unet", base=64, depth=4, math="fp32", shape=(32, 256, 256)),
    dict(id="c4_fp32", net="mod", base=128, depth=5, math="fp32", shape=(8, 512, 512)),
    dict(id="c4_bf16", net="mod", base=128, depth=5, math="bf16", shape=(8, 512, 512)),
    dict(id="res16", net="res", base=16, depth=4, math="fp32", shape=(16, 512, 512)),
    dict(id="res24", net="res", base=24, depth=4, math="fp32", shape=(16, 512, 512)),
    dict(id="res32", net="res", base=32, depth=4, math="fp32", shape=(16, 512, 512)),
    dict(id="res48", net="res", base=48, depth=4, math="fp32", shape=(16, 512, 512)),
    dict(id="res64", net="res", base=64, depth=4, math="fp32", shape=(16, 512, 512)),
    dict(id="res64_d5", net="res", base=64, depth=5, math="fp32", shape=(16, 512, 512)),
    dict(id="res64_bf16", net="res", base=64, depth=4, math="bf16", shape=(16, 512, 512)),
    dict(id="res64_d5_bf16", net="res", base=64, depth=5, math="bf16", shape=(16, 512, 512)),
]


def _single(id, shape):
    c = dict(next(c for c in PRODUCTION if c["id"] == id))
    c.update(id=f"{id}_n1", shape=shape)
    return c


# The eval-mode forwards production runs (Trainer.validate / Trainer.test, main.py --mode test,
# unet_hip.tta_predict): every PRODUCTION entry at its own shape (validation and test run at the
# training batch and size), and the single-image / partial-last-batch forward at N = 1, where the
# block-count thresholds of x3_tile / rg16_tile choose other tiles.  tta_predict runs the model
# per view at the caller's batch: no shape of its own.
INFERENCE = [dict(c) for c in PRODUCTION] + [
    _single("res64", (1, 512, 512)),
    _single("res64_bf16", (1, 512, 512)),
    _single("res64_d5_bf16", (1, 512, 512)),
    _single("c2", (1, 256, 256)),
    _single("c4_bf16", (1, 512, 512)),
]

# families only a backward launches: no eval forward may show one
BACKWARD_FAMILIES = tuple(f for f in GEMM_FAMILIES if not f.endswith("_fwd")) + (
    "bn_bwd_reduce", "bn_bwd_finalize", "bn_dz", "bias_grad", "wgrad_reduce", "conv_first_wgrad",
    "pad_compact", "res_bwd_prep", "head_bwd", "head_grad", "maxpool_bwd")

MAX_PIXELS = 128 * 512  # per sample
MAX_N = 3


def level_of(family, layer, depth):
    """Level of the layer a label names: conv i belongs to block i // 2 (two 3x3 convs per
    block; blocks 0 .. depth - 1 encoders, depth the bottleneck, then the decoders back up),
    the skip GEMMs carry the block itself, ConvT 100 + k reads level depth - k."""
    if layer >= 100:
        return depth - (layer - 100)
    b = layer if family.startswith("skip") else layer // 2
    return b if b <= depth else 2 * depth - b


_ROWS = (
    (re.compile(r"^x3r3_(\d+)x\d+$"), None),          # x3 halo row GEMM: BM
    (re.compile(r"^rg16r3_(\d+)x\d+s\d+$"), None),    # bf16 halo row GEMM: BM
    (re.compile(r"^wx3r3_\d+x\d+$"), 32),             # x3 tap-row wgrad: 32-pixel chunks
    (re.compile(r"^wg16r3m?_\d+x\d+s\d+$"), 64),      # bf16 tap-row wgrad: 64-pixel chunks
    (re.compile(r"^wgrad3_\d+x\d+x(\d+)$"), None),    # f32 tap-row wgrad: the chunk it names
)


def tile_rows(kernel):
    """Pixels one tile (row GEMM) or K chunk (weight gradient) of a row-walking kernel spans,
    None for every other kernel."""
    for rx, fixed in _ROWS:
        m = rx.match(kernel)
        if m:
            return fixed if fixed is not None else int(m.group(1))
    return None


def key(label, depth, W):
    """Coverage key (family, kernel_tile, row_class) of one launch label of a network of
    `depth` levels run on images W pixels wide."""
    family, _, rest = label.partition("/")
    kernel, _, layer = rest.partition("|")
    rows = tile_rows(kernel)
    if rows is None or not layer:
        return (family, kernel, "-")
    w = W >> level_of(family, int(layer), depth)
    return (family, kernel, "lt" if w < rows else "eq" if w == rows else "gt")


def _case(id, net, base, depth, math, shape, note, **opts):
    return dict(id=id, net=net, base=base, depth=depth, math=math, shape=shape, opts=opts, note=note)


# Shapes: H, W multiples of max(16, 2^depth).  A 256-row tile is "gt" at W = 512, "eq" at W =
# 256, "lt" below; a 128-row tile at half those widths, so one (1, 16, 512) or (1, 32, 512)
# step meets all three on its way down the levels.  (1, 48, 80): tiles ending past M, rows
# that are no power of two (the one-tap kernels only).  N = 3: a tile spans the border
# between two samples.  (3, 32, 256) at depth 4 / (3, 32, 128) at depth 3: 2 x 16 / 4 x 16
# pixels at the deepest level, the W >= 16, row_w == 16 and row_w == 32 branches.
SMALL = [
    # ---- models/model.py UNet, f32 (x3): masked-fp64 step of tests/test_gpu_x3.py
    _case("unet_default", "unet", 64, 4, "fp32", (2, 128, 128),
          "the default rule at a small grid: 128x128 / 128x64 one-tap tiles, tap-row wgrad "
          "(shape of test_x3_train_step_matches_f32_mfma)"),
    _case("unet_halo256", "unet", 64, 4, "fp32", (1, 16, 512),
          "256x128 halo tile at W = 512 (gt), 256 (eq), 128 .. 32 (lt)", x3_tile=4),
    _case("unet_halo128", "unet", 64, 4, "fp32", (1, 16, 512),
          "128x64 halo tile on every 3x3 GEMM: W = 512, 256 (gt), 128 (eq), 64, 32 (lt)",
          x3_tile=6),
    _case("unet_halo256_n3", "unet", 64, 4, "fp32", (3, 32, 256),
          "256x128 halo tile over sample borders, 2 x 16 pixels at the deepest level; 16-pixel "
          "rows of the tap-row wgrad in pairs", x3_tile=4),
    _case("unet_halo128_n3", "unet", 64, 4, "fp32", (3, 32, 256),
          "128x64 halo tile over sample borders, W = 16 rows", x3_tile=6),
    _case("unet_onetap256", "unet", 64, 4, "fp32", (1, 48, 80),
          "256x128 / 256x64 one-tap tiles ending past M (shape of "
          "test_x3_row_tile_choice_bit_identical); one-tap x3 wgrad",
          x3_tile=0, x3_n64=3, x3_r3=0),
    _case("unet_wtile64", "unet", 64, 4, "fp32", (2, 32, 64),
          "64x64 tap-row wgrad on every 3x3 layer, 64x64 one-tap wgrad on the ConvTs", x3_wtile=4),
    # ---- models/mod.py UNet, f32 (x3): fp32-oracle envelope of test_mod_narrow_full_grads_vs_fp64
    _case("mod128_default", "mod", 128, 3, "fp32", (2, 64, 64),
          "config 4's widths at the default rule of a small grid"),
    _case("mod128_halo256", "mod", 128, 3, "fp32", (1, 16, 512),
          "256x128 halo tile with the BN -> ReLU epilogues: gt / eq / lt", x3_tile=4),
    _case("mod128_halo256_n3", "mod", 128, 3, "fp32", (3, 32, 128),
          "... over sample borders, 4 x 16 pixels at the deepest level", x3_tile=4),
    _case("mod128_onetap256", "mod", 128, 3, "fp32", (1, 48, 80),
          "256x128 one-tap tile ending past M", x3_tile=0, x3_r3=0),
    # ---- models/mod.py UNet, bf16: bf16-operand oracle of test_mod_bf16_matches_bf16_oracle
    _case("mod128_bf16_default", "mod", 128, 3, "bf16", (2, 64, 64),
          "128x128 LDS-DMA tile (small grid), tap-row wgrad at W = 64 (eq), 32, 16 (lt)"),
    _case("mod128_bf16_halo256", "mod", 128, 3, "bf16", (1, 16, 512),
          "256x256 halo tile: gt / eq / lt; tap-row wgrad gt", rg16_tile=19),
    _case("mod128_bf16_halo512", "mod", 128, 3, "bf16", (1, 16, 512),
          "512x128 halo tile: eq at W = 512, lt below", rg16_tile=20),
    _case("mod128_bf16_halo256_n3", "mod", 128, 3, "bf16", (3, 32, 128),
          "256x256 halo tile over sample borders, 4 x 16 pixels at the deepest level",
          rg16_tile=19),
    _case("mod128_bf16_256x128", "mod", 128, 3, "bf16", (1, 48, 80),
          "256x128 one-tap tile ending past M; one-tap 256x256 wgrad (W = 80)", rg16_tile=2),
    _case("mod128_bf16_256x256", "mod", 128, 3, "bf16", (1, 48, 80),
          "256x256 one-tap tile ending past M (128-output GEMMs: 128x128)", rg16_tile=4),
    _case("mod128_bf16_512x128", "mod", 128, 3, "bf16", (3, 16, 48),
          "512x128 one-tap tile ending past M, over sample borders", rg16_tile=6),
    # ---- models/mod.py ResUNet, f32: envelope of test_res_full_grads_vs_oracle
    _case("res16_default", "res", 16, 4, "fp32", (1, 32, 128),
          "padded 16 -> 32: 32-channel f32 MFMA tiles and tap-row wgrads (W = 128, 64: gt), skip "
          "GEMMs"),
    _case("res24_default", "res", 24, 4, "fp32", (1, 32, 128), "padded 24 / 48 / 96"),
    _case("res32_halo128", "res", 32, 4, "fp32", (1, 16, 512),
          "128x64 halo tile on the 64-channel level (W = 256: gt) next to the 32-channel level",
          x3_tile=6),
    _case("res48_default", "res", 48, 4, "fp32", (3, 16, 48), "padded 48 -> 64, odd N"),
    _case("res64_halo256", "res", 64, 4, "fp32", (1, 16, 512),
          "256x128 halo tile with the residual epilogues (E_ADD dgrad)", x3_tile=4),
    _case("res64_default", "res", 64, 3, "fp32", (2, 64, 64),
          "the default rule at a small grid (shape of test_res_full_grads_vs_oracle)"),
    # ---- models/mod.py ResUNet, bf16: bf16-operand oracle of tests/res_bf16_ref.py
    _case("res64_bf16_default", "res", 64, 3, "bf16", (2, 64, 64),
          "register-staged bf16 tiles of the 64-channel level, f32 first block, 128x128 LDS-DMA "
          "tile (small grid) with the residual epilogues (shape of test_res_bf16_matches_bf16_oracle)"),
    _case("res64_bf16_halo256", "res", 64, 4, "bf16", (1, 16, 512),
          "256x256 halo tile with the E_ADD dgrad: gt / eq / lt; tap-row wgrad gt", rg16_tile=19),
    _case("res64_bf16_halo512", "res", 64, 4, "bf16", (1, 16, 512),
          "512x128 halo tile on the 128-output level: eq at W = 512, lt below", rg16_tile=20),
    _case("res64_bf16_halo256_n3", "res", 64, 4, "bf16", (3, 32, 256),
          "256x256 halo tile over sample borders; W = 32 and W = 16 rows of the tap-row wgrad",
          rg16_tile=19),
    _case("res64_bf16_256x128", "res", 64, 3, "bf16", (1, 48, 80),
          "256x128 one-tap tile ending past M: skip forward (E_RESID), skip dgrad (E_STORE), "
          "conv1 dgrad (E_ADD)", rg16_tile=2),
    _case("res64_bf16_256x256", "res", 64, 3, "bf16", (1, 48, 80),
          "256x256 one-tap tile ending past M (128-output GEMMs: 128x128)", rg16_tile=4),
    _case("res64_bf16_512x128", "res", 64, 3, "bf16", (3, 16, 48),
          "512x128 one-tap tile ending past M, over sample borders", rg16_tile=6),
]


def by_id(cases):
    return {c["id"]: c for c in cases}


def _eval(id, note, **kw):
    """The SMALL case `id` run in eval mode (forward only): same network, shape and options,
    which reproduce its forward keys -- the tile rules (x3_pick, rg16_pick, pick_tile) read the
    shape and the options, not the mode.  pseed / xseed: parameter and input seeds (7 / 33, the
    coverage test's, unless the meaningful-input condition of tests/test_eval_ref_cpu.py asks
    for others)."""
    c = dict(by_id(SMALL)[id])
    c.update(note=note, pseed=kw.pop("pseed", 7), xseed=kw.pop("xseed", 33))
    assert not kw
    return c


# Eval-mode small cases (tests/test_gpu_eval_coverage.py), one per distinct set of forward keys
# of a network and math; where two SMALL cases launch the same forward keys the one with N = 3
# stays (it also serves the sample-independence test).  Left out for that reason: unet_wtile64
# (a weight-gradient option; forward keys of unet_default), unet_halo128 (unet_halo128_n3),
# res64_bf16_halo256 (res64_bf16_halo256_n3).  Eval chooses no tile of its own: the keys of every
# INFERENCE entry, N = 1 included (128x128 one-tap tiles below 256 blocks, the 128x64 halo tile
# of a single 512^2 image's level 0), are forward keys of these cases.  What differs in eval is
# the operand writers behind the same GEMM: every conv and ConvT reads an image prep16 / prep_x3
# wrote into the one scratch image, the whole concat included; the notes name what each case
# adds there.  Factor of the f32 bars: 4x the fp32 CPU oracle's deviation from fp64 per layer
# (no case sets x3 = 0, whose factor is 12x); NARROW_12X names the levels of the narrow
# networks (f32 MFMA kernels under x3 = 1) that take 12x instead -- none.
NARROW_12X = ()   # (case id, level)
SMALL_EVAL = [
    _eval("unet_default", "default rule, small grid; whole-concat prep_x3 ([up, skip] order, ReLU -> BN)"),
    _eval("unet_halo256", "256x128 halo tile on the scratch image: eq / lt"),
    _eval("unet_halo256_n3", "256x128 halo tile over sample borders, 2 x 16 pixels at the deepest level"),
    _eval("unet_halo128_n3", "128x64 halo tile: gt / eq / lt, over sample borders, W = 16 rows"),
    _eval("unet_onetap256", "256x128 / 256x64 one-tap tiles ending past M"),
    _eval("mod128_default", "default rule; whole-concat prep with the skip-half affine and ReLU span"),
    _eval("mod128_halo256", "256x128 halo tile: gt / eq / lt; the max-pool stores into the scratch image"),
    _eval("mod128_halo256_n3", "256x128 halo tile over sample borders, 4 x 16 pixels at the deepest level"),
    _eval("mod128_onetap256", "256x128 one-tap tile ending past M"),
    _eval("mod128_bf16_default", "128x128 LDS-DMA tile; prep16 of every image, f32 pooled tensor"),
    _eval("mod128_bf16_halo256", "256x256 halo tile on the scratch image: eq / lt"),
    _eval("mod128_bf16_halo512", "512x128 halo tile: eq / lt"),
    _eval("mod128_bf16_halo256_n3", "256x256 halo tile over sample borders"),
    _eval("mod128_bf16_256x128", "256x128 one-tap tile ending past M"),
    _eval("mod128_bf16_256x256", "256x256 one-tap tile ending past M"),
    _eval("mod128_bf16_512x128", "512x128 one-tap tile ending past M, over sample borders"),
    _eval("res16_default", "padded 16 -> 32 (pbn expansion of the running buffers), f32 MFMA tiles, skip GEMMs"),
    _eval("res24_default", "padded 24 / 48 / 96"),
    _eval("res32_halo128", "128x64 halo tile on the 64-channel level next to the 32-channel level"),
    _eval("res48_default", "padded 48 -> 64, odd N, over sample borders"),
    _eval("res64_halo256", "256x128 halo tile with the residual epilogue (E_RESID from eval scale / shift)"),
    _eval("res64_default", "default rule, small grid"),
    _eval("res64_bf16_default", "register-staged bf16 tiles, f32 first block, r16 shared by conv1 and the skip GEMM"),
    _eval("res64_bf16_halo512", "512x128 halo tile: lt"),
    _eval("res64_bf16_halo256_n3", "256x256 halo tile over sample borders"),
    _eval("res64_bf16_256x128", "256x128 one-tap tile ending past M: conv, ConvT and skip forward"),
    _eval("res64_bf16_256x256", "256x256 one-tap tile ending past M"),
    _eval("res64_bf16_512x128", "512x128 one-tap tile ending past M, over sample borders"),
]
