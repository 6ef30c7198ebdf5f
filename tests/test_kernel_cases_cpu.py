"""tests/kernel_cases.py itself: the coverage key of a launch label, and that every small case
is a shape and a set of options the library can take.  No GPU."""
import os
import re

import pytest

import kernel_cases as KC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("label,depth,W,want", [
    # xlabel: x3 row GEMMs; conv 16 of the depth-4 network is level 0
    ("conv_fwd/x3r3_256x128|16", 4, 256, ("conv_fwd", "x3r3_256x128", "eq")),
    ("conv_fwd/x3r3_256x128|10", 4, 256, ("conv_fwd", "x3r3_256x128", "lt")),   # level 3: W = 32
    ("conv_dgrad/x3r3_128x64|1", 4, 256, ("conv_dgrad", "x3r3_128x64", "gt")),
    ("conv_fwd/x3_128x128|8", 4, 256, ("conv_fwd", "x3_128x128", "-")),          # one-tap: no rows
    ("convT_fwd/x3_256x128|103", 4, 256, ("convT_fwd", "x3_256x128", "-")),
    # x3wlabel: the tap-row x3 weight gradient walks 32-pixel chunks
    ("conv_wgrad/wx3r3_64x128|8", 4, 256, ("conv_wgrad", "wx3r3_64x128", "lt")),  # W = 16
    ("conv_wgrad/wx3r3_64x128|6", 4, 256, ("conv_wgrad", "wx3r3_64x128", "eq")),  # W = 32
    ("conv_wgrad/wx3r3_64x64|17", 4, 256, ("conv_wgrad", "wx3r3_64x64", "gt")),
    ("convT_wgrad/wx3_128x128|100", 4, 256, ("convT_wgrad", "wx3_128x128", "-")),
    # tlabel / wlabel: the f32 MFMA kernels; wgrad3 names its pixel chunk
    ("skip_fwd/rowgemm_128x128x32p|3", 4, 512, ("skip_fwd", "rowgemm_128x128x32p", "-")),
    ("conv_wgrad/wgrad3_32x32x32|2", 4, 512, ("conv_wgrad", "wgrad3_32x32x32", "gt")),  # level 1
    ("conv_wgrad/wgrad3_32x32x32|2", 4, 64, ("conv_wgrad", "wgrad3_32x32x32", "eq")),
    ("skip_wgrad/wgrad_64x128x32|3", 4, 512, ("skip_wgrad", "wgrad_64x128x32", "-")),
    # the rg16 label function: conv 21 of the depth-5 network is level 0, conv 2 level 1
    ("conv_fwd/rg16r3_512x128s2|21", 5, 512, ("conv_fwd", "rg16r3_512x128s2", "eq")),
    ("conv_dgrad/rg16r3_256x256s2|20", 5, 512, ("conv_dgrad", "rg16r3_256x256s2", "gt")),
    ("conv_fwd/rg16r3_256x256s2|2", 5, 512, ("conv_fwd", "rg16r3_256x256s2", "eq")),
    ("conv_fwd/rg16_256x128s2|10", 5, 512, ("conv_fwd", "rg16_256x128s2", "-")),
    # the bf16 weight gradient's own label: 64-pixel chunks; conv 10 is the bottleneck (W = 16)
    ("conv_wgrad/wg16r3m_128x128s4|10", 5, 512, ("conv_wgrad", "wg16r3m_128x128s4", "lt")),
    ("conv_wgrad/wg16r3m_128x128s4|6", 5, 512, ("conv_wgrad", "wg16r3m_128x128s4", "eq")),
    ("conv_wgrad/wg16r3_128x128s4|1", 5, 512, ("conv_wgrad", "wg16r3_128x128s4", "gt")),
    ("convT_wgrad/wg16_256x256s2|100", 5, 512, ("convT_wgrad", "wg16_256x256s2", "-")),
    # a launch without a tile
    ("bn_dz", 4, 256, ("bn_dz", "", "-")),
])
def test_key_of_literal_labels(label, depth, W, want):
    assert KC.key(label, depth, W) == want


def test_levels():
    # models/model.py UNet (tests/test_gpu_x3.py _relu_masks: conv i -> level)
    want = {0: 0, 1: 0, 2: 1, 3: 1, 4: 2, 5: 2, 6: 3, 7: 3, 8: 4, 9: 4, 10: 3, 11: 3, 12: 2, 13: 2,
            14: 1, 15: 1, 16: 0, 17: 0}
    assert {i: KC.level_of("conv_fwd", i, 4) for i in range(18)} == want
    assert [KC.level_of("convT_fwd", 100 + k, 4) for k in range(4)] == [4, 3, 2, 1]
    assert [KC.level_of("skip_fwd", b, 3) for b in range(7)] == [0, 1, 2, 3, 2, 1, 0]


def test_ids_unique_and_known_networks():
    for cases in (KC.SMALL, KC.PRODUCTION, KC.SMALL_EVAL, KC.INFERENCE):
        ids = [c["id"] for c in cases]
        assert len(ids) == len(set(ids))
        for c in cases:
            assert c["net"] in ("unet", "mod", "res") and c["math"] in ("fp32", "bf16")
            assert c["net"] != "unet" or (c["base"], c["depth"], c["math"]) == (64, 4, "fp32")


def test_production_is_what_bench_times():
    """bench.py's batch and image sizes (read from its source, not imported: it parses argv)."""
    src = open(os.path.join(REPO, "bench.py")).read()
    assert "args.batch or (8 if c4 else 16 if cres else 32)" in src
    assert "args.size or (512 if c4 or cres else 256)" in src
    shapes = {c["id"]: c["shape"] for c in KC.PRODUCTION}
    assert shapes["c2"] == (32, 256, 256)
    assert shapes["c4_fp32"] == shapes["c4_bf16"] == (8, 512, 512)
    res = [c for c in KC.PRODUCTION if c["net"] == "res" and c["math"] == "fp32"]
    assert {(c["base"], c["depth"]) for c in res} >= {(b, 4) for b in (16, 24, 32, 48, 64)}
    assert all(c["shape"] == (16, 512, 512) for c in res)
    # bench.py's --config res is f32 only: every bf16 residual row is main.py's, not bench.py's
    assert "ResUNet(1, 1, base_filters=args.base, depth=args.depth)" in src


def test_production_has_the_bf16_residual_steps_main_trains():
    """main.py --model_type ResUNet --mfma bf16 at its defaults (base 64, depth 5, bs 16, 512^2)
    and the two steps tools/res_bf16_time.py times (read from their sources)."""
    rows = {c["id"]: c for c in KC.PRODUCTION if c["net"] == "res" and c["math"] == "bf16"}
    assert set(rows) == {"res64_bf16", "res64_d5_bf16"}
    assert (rows["res64_bf16"]["base"], rows["res64_bf16"]["depth"]) == (64, 4)
    assert (rows["res64_d5_bf16"]["base"], rows["res64_d5_bf16"]["depth"]) == (64, 5)
    assert all(c["shape"] == (16, 512, 512) for c in rows.values())
    tool = open(os.path.join(REPO, "tools", "res_bf16_time.py")).read()
    assert "base_filters=64, depth=depth, mfma_dtype=mfma" in tool and "for depth in (4, 5):" in tool
    assert 'add_argument("--batch", type=int, default=16)' in tool
    assert 'add_argument("--size", type=int, default=512)' in tool


def test_bf16_residual_small_cases():
    """The res / bf16 small cases force each LDS-DMA tile the production steps take (one-tap 2,
    4, 6; halo 19, 20), keep one on the default rule, and meet a sample border on a halo tile."""
    rb = [c for c in KC.SMALL if c["net"] == "res" and c["math"] == "bf16"]
    assert {c["opts"].get("rg16_tile", -1) for c in rb} == {-1, 2, 4, 6, 19, 20}
    assert all(c["base"] == 64 and set(c["opts"]) <= {"rg16_tile"} for c in rb)
    assert any(c["shape"][0] == 3 and c["opts"].get("rg16_tile") == 19 for c in rb)
    for tile, rows, want in ((19, 256, {"lt", "eq", "gt"}), (20, 512, {"lt", "eq"})):
        got = set()
        for c in rb:
            if c["opts"].get("rg16_tile") == tile:
                got |= {"lt" if w < rows else "eq" if w == rows else "gt"
                        for w in (c["shape"][2] >> l for l in range(c["depth"] + 1)) if w >= 16}
        assert got == want, (tile, got)


@pytest.mark.parametrize("case", [c["id"] for c in KC.SMALL] + [c["id"] + "@eval" for c in KC.SMALL_EVAL])
def test_small_shape_rules(case):
    c = KC.by_id(KC.SMALL_EVAL if case.endswith("@eval") else KC.SMALL)[case.partition("@")[0]]
    N, H, W = c["shape"]
    q = max(16, 2 ** c["depth"])
    assert H % q == 0 and W % q == 0, (H, W, q)
    assert H * W <= KC.MAX_PIXELS and 1 <= N <= KC.MAX_N


def test_small_options_are_library_options():
    text = open(os.path.join(REPO, "include", "unet_hip.h")).read()
    block = text[text.index("Names (runtime.hip OPTION_TABLE"):text.index("Set them between steps")]
    names = set(re.findall(r"[a-z][a-z0-9_]+", block.split("\n", 1)[1].replace("*", " ")))
    used = {k for c in KC.SMALL + KC.SMALL_EVAL for k in c["opts"]}
    assert used and used <= names, used - names


def _halo_classes(option, tile, rows, cases=None):
    """Row classes the levels of the small cases that force `tile` meet (3x3 levels of at
    least 16 pixels per row, as the halo kernels require)."""
    out = set()
    for c in KC.SMALL if cases is None else cases:
        if c["opts"].get(option) != tile:
            continue
        for level in range(c["depth"] + 1):
            w = c["shape"][2] >> level
            if w >= 16:
                out.add("lt" if w < rows else "eq" if w == rows else "gt")
    return out


def test_row_classes_of_both_halo_tiles():
    """lt, eq and gt each occur for a 256-row and a 128-row halo tile (x3 tiles 4 and 6), and
    for the bf16 256-row tile (19); the 512-row tile (20) cannot be "gt" within the size cap."""
    assert _halo_classes("x3_tile", 4, 256) == {"lt", "eq", "gt"}
    assert _halo_classes("x3_tile", 6, 128) == {"lt", "eq", "gt"}
    assert _halo_classes("rg16_tile", 19, 256) == {"lt", "eq", "gt"}
    assert _halo_classes("rg16_tile", 20, 512) == {"lt", "eq"}


def test_edge_classes_occur():
    shapes = [c["shape"] for c in KC.SMALL]
    assert (1, 48, 80) in shapes                       # a tile ending past M
    assert any(n == 3 for n, _, _ in shapes)           # a tile over a sample border
    assert any((w >> c["depth"]) == 16 and (h >> c["depth"]) % 2 == 0 and c["opts"]
               for c in KC.SMALL for _, h, w in [c["shape"]])  # W = 16 at the deepest level
    assert {16, 24, 48} <= {c["base"] for c in KC.SMALL}        # padded channels


def test_inference_is_production_plus_single_images():
    """Validation and test run at the training batch and size; the single-image / partial-batch
    forward at N = 1 of the networks main.py and bench.py's headline configurations run."""
    n = len(KC.PRODUCTION)
    assert KC.INFERENCE[:n] == KC.PRODUCTION
    single = {c["id"]: c for c in KC.INFERENCE[n:]}
    assert {k: v["shape"] for k, v in single.items()} == {
        "res64_n1": (1, 512, 512), "res64_bf16_n1": (1, 512, 512), "res64_d5_bf16_n1": (1, 512, 512),
        "c2_n1": (1, 256, 256), "c4_bf16_n1": (1, 512, 512)}
    prod = KC.by_id(KC.PRODUCTION)
    for cid, c in single.items():
        p = prod[cid[:-3]]
        assert all(c[k] == p[k] for k in ("net", "base", "depth", "math"))


def test_eval_cases_are_small_cases_in_eval_mode():
    """Every eval case is a SMALL case (same network, shape and options: the forward tile rules
    read nothing else), with a note of its own and the coverage test's seeds unless the table
    says otherwise; the three left out share their forward keys with one that stays."""
    small = KC.by_id(KC.SMALL)
    for c in KC.SMALL_EVAL:
        s = small[c["id"]]
        assert all(c[k] == s[k] for k in ("net", "base", "depth", "math", "shape", "opts"))
        assert c["note"] and isinstance(c["pseed"], int) and isinstance(c["xseed"], int)
    assert len(KC.SMALL_EVAL) < len(KC.SMALL)
    assert set(small) - {c["id"] for c in KC.SMALL_EVAL} == {"unet_wtile64", "unet_halo128", "res64_bf16_halo256"}
    for case, level in KC.NARROW_12X:
        c = KC.by_id(KC.SMALL_EVAL)[case]
        assert c["math"] == "fp32" and (c["base"] << level) % 64 and 0 <= level <= c["depth"]


def test_eval_edge_classes_occur():
    """gt / eq / lt of both x3 halo tiles and eq / lt of both bf16 halo tiles (level 0 of the
    128-base network takes the 128-output tile, so 256x256 is never "gt" in a forward), tiles
    ending past M, sample borders and 16-pixel rows, padded channels -- in eval mode."""
    ev = KC.SMALL_EVAL
    assert _halo_classes("x3_tile", 4, 256, ev) == {"lt", "eq", "gt"}
    assert _halo_classes("x3_tile", 6, 128, ev) == {"lt", "eq", "gt"}
    assert _halo_classes("rg16_tile", 19, 256, ev) >= {"lt", "eq"}
    assert _halo_classes("rg16_tile", 20, 512, ev) == {"lt", "eq"}
    shapes = {c["shape"] for c in ev}
    assert {(1, 16, 512), (1, 48, 80), (3, 32, 256), (3, 32, 128), (3, 16, 48)} <= shapes
    assert {16, 24, 48} <= {c["base"] for c in ev}
    for net, math in (("unet", "fp32"), ("mod", "fp32"), ("mod", "bf16"), ("res", "fp32"), ("res", "bf16")):
        mine = [c for c in ev if (c["net"], c["math"]) == (net, math)]
        assert any(c["shape"][0] == 3 for c in mine) and any(not c["opts"] for c in mine), (net, math)


def test_backward_families_are_no_forward_families():
    assert all(f.endswith(("dgrad", "wgrad")) for f in KC.BACKWARD_FAMILIES if f in KC.GEMM_FAMILIES)
    forward = {"bn_finalize", "bn_stats_reduce", "prep16", "prep_x3", "pack", "fill", "copy_x", "conv_first_fwd",
               "res_out", "maxpool_fwd", "head_fwd", "conv_fwd", "convT_fwd", "skip_fwd"}
    assert not forward & set(KC.BACKWARD_FAMILIES)
    src = open(os.path.join(REPO, "thyroid-nodule-image-segmentation-unet-ddti_amd", "csrc", "runtime.hip")).read()
    fwd_src, bwd_src = src[src.index("int forward_impl("):src.index("int backward_impl(")], src[src.index("int backward_impl("):]
    for f in KC.BACKWARD_FAMILIES:
        assert f'"{f}"' in bwd_src and f'"{f}"' not in fwd_src, f
