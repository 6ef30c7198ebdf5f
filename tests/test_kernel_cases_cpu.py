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
    for cases in (KC.SMALL, KC.PRODUCTION):
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


@pytest.mark.parametrize("case", [c["id"] for c in KC.SMALL])
def test_small_shape_rules(case):
    c = KC.by_id(KC.SMALL)[case]
    N, H, W = c["shape"]
    q = max(16, 2 ** c["depth"])
    assert H % q == 0 and W % q == 0, (H, W, q)
    assert H * W <= KC.MAX_PIXELS and 1 <= N <= KC.MAX_N


def test_small_options_are_library_options():
    text = open(os.path.join(REPO, "include", "unet_hip.h")).read()
    block = text[text.index("Names (runtime.hip OPTION_TABLE"):text.index("Set them between steps")]
    names = set(re.findall(r"[a-z][a-z0-9_]+", block.split("\n", 1)[1].replace("*", " ")))
    used = {k for c in KC.SMALL for k in c["opts"]}
    assert used and used <= names, used - names


def _halo_classes(option, tile, rows):
    """Row classes the levels of the small cases that force `tile` meet (3x3 levels of at
    least 16 pixels per row, as the halo kernels require)."""
    out = set()
    for c in KC.SMALL:
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
