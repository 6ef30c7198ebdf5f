"""CPU: the predict-mode export through the host twins unet_resize_f32_plan /
unet_resize_f32_mask_host / unet_overlay_u8_host -- csrc/export.h, the source the device kernels
share -- against Pillow (the float32 plane, as uint32 bit patterns) and the NumPy restatement
export_ref (plan, plane, masks, RGB, statistics), bit for bit.  Then the refusals, the main.py
flags and the CSV line."""
import ctypes
import os

import numpy as np
import pytest
import torch
from PIL import Image

import export_ref as R

SHAPES = R.RESIZE_SHAPES + [(32, 32, 19, 45), (33, 47, 11, 9)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pillow(a, oh, ow):
    return np.asarray(Image.fromarray(a, "F").resize((ow, oh), Image.BILINEAR))


@pytest.mark.parametrize("n_in,n_out", [(16, 23), (16, 37), (16, 7), (16, 5), (48, 360), (48, 560), (16, 1),
                                        (16, 40), (512, 360), (7, 7), (1, 9), (9, 1)])
def test_plan_equals_numpy(n_in, n_out):
    from unet_hip.functional import resize_f32_plan
    k, b = resize_f32_plan(n_in, n_out)
    wk, wb = R.plan(n_in, n_out)
    assert k.shape == wk.shape and np.array_equal(b, wb)
    assert np.array_equal(k.view(np.uint64), wk.view(np.uint64))


def test_plan_ksize_alone_and_refusals():
    from unet_hip import _lib
    lib = _lib.load()
    ks = ctypes.c_int()
    assert lib.unet_resize_f32_plan(16, 5, None, None, ctypes.byref(ks)) == 0
    assert ks.value == R.plan(16, 5)[0].shape[1] == 9
    assert lib.unet_resize_f32_plan(0, 5, None, None, ctypes.byref(ks)) == -1
    assert lib.unet_resize_f32_plan(5, 0, None, None, ctypes.byref(ks)) == -1
    assert lib.unet_resize_f32_plan(5, 5, None, None, None) == -1


@pytest.mark.parametrize("h,w,oh,ow", SHAPES)
def test_resize_back_host_equals_pillow_and_ref(h, w, oh, ow):
    import unet_hip
    a = R.score_plane(h, w, h * 1000 + ow)
    want = pillow(a, oh, ow)
    for kind, thr in (("greater", 0.25), ("greater", -3.0), ("sigmoid", 0.5)):
        mask, plane = unet_hip.resize_back_host(torch.from_numpy(a), (oh, ow), kind, thr, return_plane=True)
        assert plane.dtype == torch.float32 and tuple(plane.shape) == (oh, ow)
        assert np.array_equal(bits(plane.numpy()), bits(want)), "plane differs from Pillow"
        assert np.array_equal(bits(plane.numpy()), bits(R.resize(a, oh, ow))), "plane differs from export_ref"
        m = mask.numpy()
        assert m.dtype == np.uint8 and set(np.unique(m)) <= {0, 1}
        ref = R.threshold(want, kind, thr)
        if kind == "greater":
            assert np.array_equal(m, ref)
        else:  # inside the band the float32 sigmoid may round to 0.5 either way
            far = ~R.sigmoid_band(want)
            assert np.array_equal(m[far], ref[far]) and np.array_equal(m[far], (want > 0)[far])
        only = unet_hip.resize_back_host(torch.from_numpy(a), (oh, ow), kind, thr)
        assert torch.equal(only, mask)


def test_sigmoid_kind_is_not_a_sign_test():
    """Tiny positive logits: the float32 sigmoid rounds to exactly 0.5, background."""
    import unet_hip
    a = np.full((4, 4), 2.0 ** -30, np.float32)
    a[0, 0] = 1.0
    m = unet_hip.resize_back_host(torch.from_numpy(a), (4, 4), "sigmoid").numpy()
    assert m[0, 0] == 1 and m.sum() == 1
    g = unet_hip.resize_back_host(torch.from_numpy(a), (4, 4), "greater", 0.0).numpy()
    assert g.sum() == 16
    nan = np.full((3, 3), np.nan, np.float32)
    for kind in ("sigmoid", "greater"):
        assert unet_hip.resize_back_host(torch.from_numpy(nan), (3, 3), kind).sum() == 0


CASES = R.overlay_cases(16, 64)


@pytest.mark.parametrize("name", sorted(CASES))
def test_overlay_host_equals_ref(name):
    import unet_hip
    gray, pred, gt = CASES[name]
    for r in (1, 2, 3):
        for alpha in (0, 96, 256):
            for g in (None, gt):
                rgb, st = unet_hip.overlay_host(torch.from_numpy(gray), torch.from_numpy(pred),
                                                None if g is None else torch.from_numpy(g), r, alpha)
                want, wst = R.overlay(gray, pred, g, r, alpha)
                assert rgb.numpy().tobytes() == want.tobytes(), (name, r, alpha, g is not None)
                assert st.tolist() == wst, (name, r, alpha)


def test_overlay_host_large_and_width_one_is_the_surface_border():
    import unet_hip
    gray, pred, gt = CASES["disc_360x560"]
    rgb, st = unet_hip.overlay_host(torch.from_numpy(gray), torch.from_numpy(pred), torch.from_numpy(gt), 2, 96)
    want, wst = R.overlay(gray, pred, gt, 2, 96)
    assert rgb.numpy().tobytes() == want.tobytes() and st.tolist() == wst
    # r = 1: a foreground pixel with a 4-neighbour that is background or outside
    fg = pred != 0
    p = np.pad(fg, 1)
    inner = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    _, st1 = unet_hip.overlay_host(torch.from_numpy(gray), torch.from_numpy(pred), None, 1, 0)
    assert st1[1].item() == int((fg & ~inner).sum())


def test_prediction_contour_wins_and_gt_is_not_tinted():
    import unet_hip
    gray = np.full((9, 9), 100, np.uint8)
    pred = np.zeros((9, 9), np.uint8)
    pred[2:7, 2:7] = 1
    gt = np.zeros((9, 9), np.uint8)
    gt[2:7, 2:9] = 1  # shares pred's top, left and bottom contour; its inside extends right
    rgb, st = unet_hip.overlay_host(torch.from_numpy(gray), torch.from_numpy(pred), torch.from_numpy(gt), 1, 128)
    rgb = rgb.numpy()
    assert tuple(rgb[2, 2]) == (255, 0, 0)          # both contours: red wins
    assert tuple(rgb[2, 8]) == (0, 0, 255)          # gt contour alone
    assert tuple(rgb[4, 7]) == (100, 100, 100)      # inside gt only: no tint
    assert tuple(rgb[4, 4]) == ((100 * 128 + 255 * 128 + 128) >> 8, (100 * 128 + 128) >> 8, (100 * 128 + 128) >> 8)
    assert st.tolist() == [25, 16, 2, 2, 6, 6]


def test_refusals():
    import unet_hip
    from unet_hip import _lib
    lib = _lib.load()
    a = torch.zeros((4, 4), dtype=torch.float32)
    u = torch.zeros((4, 4), dtype=torch.uint8)
    rgb = torch.zeros((4, 4, 3), dtype=torch.uint8)
    st = torch.zeros(6, dtype=torch.int64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def resize(h, w, oh, ow, kind):
        return lib.unet_resize_f32_mask_host(p(a), h, w, oh, ow, None, None, 0, None, None, 0, kind, 0.5, None, p(u))

    assert resize(4, 4, 4, 4, 0) == 0
    for args in ((0, 4, 4, 4, 0), (4, -1, 4, 4, 0), (4, 4, 0, 4, 1), (4, 4, 4, 0, 1), (4, 4, 4, 4, 2), (4, 4, 4, 4, -1)):
        assert resize(*args) == -1, args
    assert resize(4, 4, 4, 8, 0) == -1  # a changed axis without its tables

    def ov(h, w, r, alpha):
        return lib.unet_overlay_u8_host(p(u), p(u), None, h, w, r, alpha, p(rgb), p(st))

    assert ov(4, 4, 1, 0) == 0 and ov(4, 4, 3, 256) == 0
    for args in ((0, 4, 1, 0), (4, 0, 1, 0), (4, 4, 0, 0), (4, 4, 4, 0), (4, 4, 1, -1), (4, 4, 1, 257)):
        assert ov(*args) == -1, args
    with pytest.raises(ValueError):
        unet_hip.overlay_host(u, u, None, 4, 0)
    with pytest.raises(ValueError):
        unet_hip.overlay_host(u, u, None, 1, 300)
    with pytest.raises(ValueError):
        unet_hip.resize_back_host(a, (4, 4), "nearest")
    with pytest.raises(ValueError):
        unet_hip.resize_back_host(a, (0, 4))
    # the device functions take no CPU tensor: no fallback
    with pytest.raises(unet_hip.HipUnavailable):
        unet_hip.resize_back(a, (4, 4))
    with pytest.raises(unet_hip.HipUnavailable):
        unet_hip.overlay(u, u)


def test_main_parser_predict(tmp_path, capsys):
    import main
    io = ["--input_dir", str(tmp_path), "--output_dir", str(tmp_path / "out"), "--checkpoint_path", "m.pth"]
    a = main.get_parser(["--mode", "predict"] + io + ["--contour_width", "2", "--overlay_alpha", "96", "--save_prob",
                                                     "--tta", "flips", "--pp_largest", "--threshold", "0.5"])
    assert a.mode == "predict" and a.contour_width == 2 and a.overlay_alpha == 96 and a.save_prob
    assert main.get_parser(["--mode", "predict", "--threshold", "0.3"] + io).threshold == 0.3
    for bad in (["--threshold", "val-dice"], ["--threshold", "val-image-dice"], ["--threshold", "0.3", "--tta", "hflip"],
                ["--contour_width", "4"], ["--overlay_alpha", "257"]):
        with pytest.raises(SystemExit):
            main.get_parser(["--mode", "predict"] + io + bad)
    for argv, word in ((["--mode", "predict"], "--input_dir"), (["--mode", "predict"] + io[:4], "--checkpoint_path"),
                       (["--mode", "predict", "--threshold", "val-dice"] + io, "validation split")):
        capsys.readouterr()
        with pytest.raises(SystemExit):
            main.get_parser(argv)
        assert word in capsys.readouterr().err, argv
    assert main.same_stem(["a.jpg", "a.png", "b.png"]) == ["a.jpg", "a.png"] and main.same_stem(["a.png", "b.png"]) == []
    assert main.predict_args_error(a, world=2) and main.predict_args_error(a, world=1) is None
    # the other modes are as before, and gain --save_overlays
    t = main.get_parser(["--mode", "test", "--save_overlays"])
    assert t.save_overlays and not main.get_parser([]).save_overlays
    assert main.get_parser(["--threshold", "val-dice"]).threshold == "val-dice"


def test_distributed_predict_is_refused(tmp_path, monkeypatch, capsys):
    import main
    argv = ["--mode", "predict", "--input_dir", str(tmp_path), "--output_dir", str(tmp_path), "--checkpoint_path",
            "m.pth"]
    monkeypatch.setenv("WORLD_SIZE", "1")
    assert main.get_parser(argv).mode == "predict"  # the same arguments parse in one process
    monkeypatch.setenv("WORLD_SIZE", "2")
    capsys.readouterr()
    with pytest.raises(SystemExit):
        main.get_parser(argv)
    assert "single-process" in capsys.readouterr().err


def test_export_plans_are_bounded():
    """The host plan cache is an LRU of fixed size, the device one lives on the runtime with a cap."""
    from unet_hip import functional as F
    from unet_hip.runtime import UNetRuntime
    assert F._host_plan.cache_info().maxsize == 64 and UNetRuntime.EXPORT_PLAN_CACHE == 256
    assert not hasattr(F, "_EXPORT_PLANS")


def test_csv_row():
    from unet_hip.predict import CSV_HEADER, csv_row
    assert CSV_HEADER == ("name", "h", "w", "area", "area_fraction", "x0", "y0", "x1", "y1", "components")
    row = dict(h=360, w=560, area=5040, contour=300, x0=10, y0=20, x1=99, y1=120, components=2)
    assert csv_row("a.png", row) == "a.png,360,560,5040,0.025000,10,20,99,120,2"
    empty = dict(h=5, w=7, area=0, contour=0, x0=-1, y0=-1, x1=-1, y1=-1, components=0)
    assert csv_row("e.png", empty) == "e.png,5,7,0,0.000000,-1,-1,-1,-1,0"
