"""CPU: lesion morphometry through the host twin unet_morphometry_host -- csrc/morph.h, the source the
device kernels share -- against its NumPy / scipy restatement (morph_ref), bit for bit: everything
is integer sums, minima and maxima.  Then scipy's own measurements, the hole counts, dropped rows
and guard words, the refusals, ``shape_descriptors`` on shapes with known answers, the CSV line, the
flags, and the host-only build of morph.h under the sanitizers."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import scipy.ndimage as nd
import torch

import cc_ref as R
import morph_ref as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "thyroid-nodule-image-segmentation-unet-ddti_amd", "csrc")
PLANES = M.all_planes()
GUARD = 0x5A5A5A5A5A5A5A5A


def u8(m):
    return torch.from_numpy(np.ascontiguousarray(m).astype(np.uint8))


def host(m, conn, max_rows=None):
    import unet_hip
    return unet_hip.lesion_morphometry_host(u8(m), conn, max_rows=max_rows)


@pytest.mark.parametrize("conn", R.CONNECTIVITIES)
def test_host_twin_equals_the_restatement(conn):
    for name, m in PLANES:
        out = host(m[None], conn)
        lab, k = R.label(m, conn)
        assert int(out["count"][0]) == k and np.array_equal(out["labels"][0].numpy(), lab), name
        assert np.array_equal(out["table"][0].numpy(), M.table(lab)), name


def test_the_named_edge_planes():
    """What each of the issue's planes is there for."""
    X = M.extra_cases()
    t = host(X["1x130"][None], 1)["table"][0, 0].tolist()  # one run across three tiles
    assert t[0] == 130 and t[1] == 129 * 130 // 2 and t[6:10] == [0, 0, 129, 0] and t[14] == 129 ** 2
    assert t[10:14] == [4, 2 * 129, 0, 0]
    t = host(X["130x1"][None], 1)["table"][0, 0].tolist()
    assert t[0] == 130 and t[2] == 129 * 130 // 2 and t[6:10] == [0, 0, 0, 129] and t[14] == 129 ** 2
    assert host(X["1x1"][None], 2)["table"][0, 0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 0, 0, 0, 0, 0]
    t = host(X["full65"][None], 1)["table"][0, 0].tolist()
    assert t[0] == 65 * 65 and t[10:14] == [4, 4 * 64, 0, 0] and t[14] == 2 * 64 ** 2
    out = host(X["checkerboard16"][None], 1)
    assert int(out["count"][0]) == 128 and (out["table"][0, :, 0] == 1).all() and (out["table"][0, :, 10] == 4).all()
    out = host(X["checkerboard16"][None], 2)
    t = out["table"][0, 0].tolist()
    assert int(out["count"][0]) == 1 and t[0] == 128 and t[12] == 15 * 15 and t[11] == 0 and t[13] == 0
    out = host(X["diagonal_squares"][None], 1)  # the window at the shared corner holds two labels: a q1 each
    assert int(out["count"][0]) == 2 and out["table"][0, :, 10].tolist() == [4, 4] and out["table"][0, :, 12].tolist() == [0, 0]
    out = host(X["diagonal_squares"][None], 2)
    assert int(out["count"][0]) == 1 and out["table"][0, 0, 12] == 1 and out["table"][0, 0, 10] == 6
    t = host(X["four_borders"][None], 1)["table"][0, 0].tolist()
    assert t[6:10] == [0, 0, 69, 39]


@pytest.mark.parametrize("conn", R.CONNECTIVITIES)
def test_against_scipy_measurements(conn):
    for name in ("33x65", "96x160"):
        for m in R.mask_cases()[name]:
            lab, k = R.label(m, conn)
            if k == 0:
                continue
            tab = host(m[None], conn)["table"][0].numpy()
            idx = np.arange(1, k + 1)
            i, j = np.mgrid[:m.shape[0], :m.shape[1]]
            assert np.array_equal(tab[:, 0], nd.sum_labels(np.ones_like(lab), lab, idx).astype(np.int64))
            assert np.array_equal(tab[:, 1], nd.sum_labels(j, lab, idx).astype(np.int64))
            assert np.array_equal(tab[:, 2], nd.sum_labels(i, lab, idx).astype(np.int64))
            assert np.array_equal(tab[:, 4], nd.sum_labels(i * j, lab, idx).astype(np.int64))
            boxes = [[s[1].start, s[0].start, s[1].stop - 1, s[0].stop - 1] for s in nd.find_objects(lab)]
            assert np.array_equal(tab[:, 6:10], np.array(boxes))


@pytest.mark.parametrize("pattern", ["ring", "nested_rings", "spiral", "open_ring", "full"])
def test_holes_are_the_enclosed_background_components(pattern):
    import unet_hip
    for name in ("33x65", "64x64", "96x160"):
        m = R.mask_cases()[name][R.PATTERNS.index(pattern)]
        for conn in R.CONNECTIVITIES:
            out = host(m[None], conn)
            lab = out["labels"][0].numpy()
            d = unet_hip.shape_descriptors(out["table"][0], connectivity=conn)
            # the foreground connectivity's dual: holes of an 8-connected component are 4-connected
            want = []
            for l in range(1, int(out["count"][0]) + 1):
                bg, k = nd.label(~np.pad(lab == l, 1), R.structure(3 - conn))
                want.append(k - 1)
            assert d["holes"].tolist() == want, (name, conn)
            if conn == 2:
                assert want == [M.enclosed_background(lab == l) for l in range(1, len(want) + 1)]


@pytest.mark.parametrize("conn", R.CONNECTIVITIES)
def test_rows_beyond_max_rows_are_dropped_and_guards_stay(conn):
    import unet_hip
    from unet_hip import _lib
    x = u8(R.mask_cases()["33x65"][[2, 14]])
    lab, cnt = unet_hip.connected_components_host(x, conn)
    full = unet_hip.morphometry_table_host(lab, cnt).numpy()
    K = int(cnt.max())
    assert K > 3 and full.shape == (2, K, 16)
    assert not full[1, int(cnt[1]):].any()  # rows beyond the sample's own count are zero
    for rows in (1, K - 1, K + 5):
        buf = torch.full((2 * rows * 16 + 64,), GUARD, dtype=torch.int64)
        rc = _lib.load().unet_morphometry_host(ctypes.c_void_p(lab.data_ptr()), ctypes.c_void_p(cnt.data_ptr()), 2, 33,
                                               65, rows, ctypes.c_void_p(buf.data_ptr()))
        assert rc == 0
        assert (buf[2 * rows * 16:] == GUARD).all()
        got = buf[:2 * rows * 16].reshape(2, rows, 16).numpy()
        assert np.array_equal(got[:, :min(rows, K)], full[:, :rows]) and not got[:, K:].any()
        assert cnt.tolist() == [R.label(m, conn)[1] for m in x.numpy()]  # count still says how many there are


def test_refusals():
    import unet_hip
    from unet_hip import _lib
    lib = _lib.load()
    lab, cnt, tab = torch.zeros((1, 4, 4), dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.zeros(16, dtype=torch.int64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.unet_morphometry_host(p(lab), p(cnt), 1, 4, 4, 1, p(tab)) == 0
    assert lib.unet_morphometry_host(None, p(cnt), 1, 4, 4, 1, p(tab)) == -1
    assert lib.unet_morphometry_host(p(lab), None, 1, 4, 4, 1, p(tab)) == -1
    assert lib.unet_morphometry_host(p(lab), p(cnt), 1, 4, 4, 1, None) == -1
    for N, H, W, rows in ((0, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (1, 4, 4, 0), (1, 1 << 16, 1 << 15, 1)):
        assert lib.unet_morphometry_host(p(lab), p(cnt), N, H, W, rows, p(tab)) == -1
    assert lib.unet_morphometry_host(p(lab), p(cnt), 1, 4097, 1, 1, p(tab)) == -2
    assert lib.unet_morphometry_host(p(lab), p(cnt), 1, 1, 4097, 1, p(tab)) == -2
    assert lib.unet_morphometry(None, p(lab), p(cnt), 1, 4, 4, 1, p(tab), None) == -1
    with pytest.raises(unet_hip.HipUnavailable):
        unet_hip.morphometry_table(lab, cnt)
    with pytest.raises(ValueError):
        unet_hip.morphometry_table_host(lab.long(), cnt)
    with pytest.raises(ValueError):
        unet_hip.morphometry_table_host(lab, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError):
        unet_hip.shape_descriptors(tab.reshape(1, 16), spacing=0.0)
    with pytest.raises(ValueError):
        unet_hip.shape_descriptors(tab.reshape(1, 16), connectivity=3)


# ---------------------------------------------------------------- shape_descriptors
@pytest.mark.parametrize("a,b", [(1, 1), (7, 3), (3, 7), (40, 12), (5, 5)])
def test_rectangle_descriptors(a, b):
    import unet_hip
    m = M.rectangle(50, 60, 4, 9, b, a)
    d = unet_hip.shape_descriptors(host(m[None], 1)["table"][0])
    assert d["mu20"][0] == (a * a - 1) / 12 and d["mu02"][0] == (b * b - 1) / 12 and d["mu11"][0] == 0
    assert d["extent"][0] == 1 and d["holes"][0] == 0 and d["euler"][0] == 1
    assert d["perimeter_crack"][0] == 2 * (a + b)
    assert d["box_w"][0] == a and d["box_h"][0] == b and bool(d["taller_than_wide"][0]) == (b > a)
    assert d["centroid_x"][0] == 9 + (a - 1) / 2 and d["centroid_y"][0] == 4 + (b - 1) / 2
    assert d["feret_max"][0] == math.sqrt((a - 1) ** 2 + (b - 1) ** 2)
    assert abs(d["major_axis"][0] - 4 * math.sqrt((max(a, b) ** 2 - 1) / 12)) < 1e-12
    s = unet_hip.shape_descriptors(host(m[None], 1)["table"][0], spacing=0.25)
    assert s["area"][0] == a * b * 0.0625 and s["feret_max"][0] == d["feret_max"][0] * 0.25
    assert s["extent"][0] == 1 and s["circularity"][0] == d["circularity"][0]


@pytest.mark.parametrize("theta", [0.0, 0.4, 1.2, -0.7, math.pi / 2])
def test_ellipse_orientation_and_axes(theta):
    """An ellipse with semi-axes 60 and 25: the moment ellipse has the same axes and angle up to the
    discretisation (the pixel grid moves the boundary by at most half a pixel: 1 / 25 rad over the
    minor semi-axis bounds the angle, one pixel each axis length)."""
    import unet_hip
    m = M.rotated_ellipse(200, 200, 99.5, 99.5, 60, 25, theta)
    d = unet_hip.shape_descriptors(host(m[None], 2)["table"][0])
    got = d["orientation"][0]
    diff = abs((got - theta + math.pi / 2) % math.pi - math.pi / 2)
    assert diff < 1 / 25, (got, theta)
    assert abs(d["major_axis"][0] - 120) < 1 and abs(d["minor_axis"][0] - 50) < 1
    assert abs(d["eccentricity"][0] - math.sqrt(1 - (25 / 60) ** 2)) < 0.01
    assert abs(d["feret_max"][0] - 120) < 2 and 0.6 < d["circularity"][0] < 1.0
    assert abs(d["centroid_x"][0] - 99.5) < 1e-9 and abs(d["centroid_y"][0] - 99.5) < 1e-9


def test_empty_rows_and_batches_of_tables():
    import unet_hip
    out = host(R.mask_cases()["33x65"][[0, 11]], 1, max_rows=3)
    d = unet_hip.shape_descriptors(out["table"])
    assert d["area"].shape == (2, 3) and not d["area"][0].any() and d["holes"][1, 0] == 1
    assert d["area"][1, 1] == 0 and d["circularity"][1, 1] == 0


def test_shape_agreement_and_kappa():
    from unet_hip import functional as F
    tall, wide = M.rectangle(40, 40, 2, 3, 20, 6), M.rectangle(40, 40, 5, 3, 6, 20)
    rows = lambda ms: torch.stack([host(m[None], 1, max_rows=1)["table"][0, 0] for m in ms])
    empty = np.zeros((40, 40), bool)
    s = F.shape_agreement(rows([tall, wide, tall, empty, wide]), rows([tall, wide, wide, tall, empty]))
    assert s.tolist()[0] == 3 and s.tolist()[4:] == [1, 1, 0, 1]
    assert s[1] == 0 and s[2] == 0 and abs(s[3] - math.hypot(7, 4)) < 1e-12  # the third pair's centroids
    out = F.shape_summary(s)
    assert out["n_pairs"] == 3 and out["ttw"] == [1, 1, 0, 1]
    po, pe = 2 / 3, (2 * 1 + 1 * 2) / 9
    assert abs(out["kappa"] - (po - pe) / (1 - pe)) < 1e-15
    assert math.isnan(F.shape_summary(np.zeros(8))["kappa"]) and math.isnan(F.shape_summary(np.zeros(8))["feret_mae"])
    assert math.isnan(F.shape_summary([2, 0, 0, 0, 2, 0, 0, 0])["kappa"])  # chance agreement 1


# ---------------------------------------------------------------- lesions.csv and the flags
def test_csv_line_format():
    from unet_hip import functional as F
    from unet_hip.predict import lesion_csv_header
    m = M.rectangle(50, 60, 4, 9, 7, 3) | M.rectangle(50, 60, 30, 20, 1, 1)
    out = host(m[None], 1)
    lines = F.lesion_csv_lines("a.png", out["table"][0], out["count"][0])
    # the 3 x 7 rectangle: feret sqrt(2^2 + 6^2), axes 4 sqrt(48 / 12) and 4 sqrt(8 / 12), upright, eccentricity
    # sqrt(1 - 1 / 6), perimeter 16 + 4 / sqrt(2), circularity 4 pi 21 / perimeter^2
    assert lesion_csv_header() == F.LESION_COLUMNS and len(F.LESION_COLUMNS) == 18
    assert lines[0] == "a.png,1,21,10.0000,7.0000,9,4,11,10,6.3246,8.0000,3.2660,1.5708,0.9129,18.8284,0.7444,0,1"
    assert lines[1].split(",")[:9] == ["a.png", "2", "1", "20.0000", "30.0000", "20", "30", "20", "30"]
    assert lines[1].split(",")[-2:] == ["0", "0"] and len(lines) == 2
    mm = F.lesion_csv_lines("a.png", out["table"][0], 2, pixel_spacing=0.5)
    assert lesion_csv_header(0.5) == F.LESION_COLUMNS + ("feret_max_mm", "area_mm2")
    assert mm[0] == lines[0] + ",3.1623,5.2500" and all(len(l.split(",")) == 20 for l in mm)
    assert F.lesion_csv_lines("e.png", out["table"][0][:0], 0) == []


def test_flags_parse_and_refusals(capsys):
    import main
    a = main.get_parser([])
    assert a.lesion_table is False and a.pixel_spacing is None and a.lesion_shape is False
    assert main.get_parser(["--mode", "test", "--lesion_shape"]).lesion_shape is True
    ok = ["--mode", "predict", "--input_dir", "i", "--output_dir", "o", "--checkpoint_path", "c"]
    a = main.get_parser(ok + ["--lesion_table", "--pixel_spacing", "0.2"])
    assert a.lesion_table is True and a.pixel_spacing == 0.2
    for bad, word in ((["--mode", "test", "--lesion_table"], "predict only"),
                      (ok + ["--lesion_table", "--pixel_spacing", "0"], "positive"),
                      (ok + ["--lesion_table", "--pixel_spacing", "-1"], "positive"),
                      (ok + ["--pixel_spacing", "0.2"], "--lesion_table")):
        with pytest.raises(SystemExit):
            main.get_parser(bad)
        assert word in capsys.readouterr().err


# ---------------------------------------------------------------- morph.h alone, under the sanitizers
def test_morph_header_builds_for_the_host_alone_and_runs_clean(tmp_path):
    """tools/morph_host_check.cpp includes morph.h with no HIP header, runs the host twin on the edge
    planes with exactly sized buffers and guard words against a brute-force restatement, and is
    built with -fsanitize=address,undefined: a stand-alone program, run as its own process."""
    exe = str(tmp_path / "morph_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-DMORPH_HOST_ONLY", "-I", CSRC,
                           os.path.join(REPO, "tools", "morph_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env={"PATH": os.environ.get("PATH", "")})
    assert out.returncode == 0, out.stdout + out.stderr
    assert "morph_host_check ok" in out.stdout
