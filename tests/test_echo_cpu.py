"""CPU: the lesion echo table through the host twin unet_lesion_echo_host -- csrc/echo.h, the source
the device kernel shares -- against its NumPy / scipy restatement (echo_ref), bit for bit: everything
is an integer count.  Then ``echo_descriptors`` against direct computation on the pixel lists, the
refusals, the CSV columns, the flags, and the host-only build of echo.h under the sanitizers."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import echo_ref as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "thyroid-nodule-image-segmentation-unet-ddti_amd", "csrc")
CASES = E.cases()
IDS = [c["name"] for c in CASES]
GUARD = 0x5A5A5A5A


def host_table(c, max_rows=None):
    from unet_hip import echo_table_host
    return echo_table_host(torch.from_numpy(c["gray"]), torch.from_numpy(c["labels"]), torch.from_numpy(c["count"]),
                           c["max_rows"] if max_rows is None else max_rows, c["G"], c["w"])


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_host_twin_equals_the_restatement(c):
    got = host_table(c)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(c["labels"]), c["max_rows"], 512 + c["G"] ** 2)
    want = E.table(c["gray"], c["labels"], c["count"], c["max_rows"], c["G"], c["w"])
    assert np.array_equal(got.numpy(), want)


def by_name(name):
    return CASES[IDS.index(name)]


def test_what_the_named_cases_are_there_for():
    t = host_table(by_name("1x1 w16"))[0, 0]
    assert t[7] == 1 and int(t.sum()) == 1  # one pixel: no ring inside the plane, no pair
    t = host_table(by_name("33x70 checkerboard G16 w1")).numpy()[0]
    assert (t[:, :256].sum(1) == 1).all() and not t[:, 512:].any()  # single pixels: glcm_pairs all 0
    assert t[:, 256:512].sum() == 33 * 70 - len(t)  # every background pixel has a neighbour: all owned
    t = host_table(by_name("12x300 bars w8")).numpy()[0]
    # bars at columns 100..109 and 115..124, rows 2..9 of 12: label 1 owns everything it reaches (columns
    # 92..117, the gap and the tie columns included) but the pixels of the bars, label 2 only columns 118..132
    lo, hi = t[0, 256:512].sum(), t[1, 256:512].sum()
    assert lo == 26 * 12 - 80 - 3 * 8 and hi == 15 * 12 - 7 * 8
    assert not host_table(by_name("1x70 w0"))[0, 0, 256:512].any()  # ring 0: no ring histogram
    t = host_table(by_name("diagonal squares")).numpy()[0]
    q = (93 * 16) >> 8
    assert t[0, 512 + q * 16 + q] == t[1, 512 + q * 16 + q] == 2 * 6 * 5 + 2 * 5 * 5 == t[0, 512:].sum()
    t3 = host_table(by_name("N3 counts 0 1 many")).numpy()
    assert not t3[0].any() and t3[1, 0, :256].sum() == 30 * 60 and not t3[1, 1:].any() and t3[2, -1, :256].sum() >= 1
    few = host_table(by_name("N3 max_rows 3")).numpy()
    assert np.array_equal(few, t3[:, :3])  # dropped labels leave the rows that stay untouched


@pytest.mark.parametrize("name", ["N3 counts 0 1 many", "33x70 checkerboard G8 w16", "1x1 w0"])
def test_guard_words_and_uninitialised_tables(name):
    from unet_hip import _lib
    c = by_name(name)
    N, H, W = c["labels"].shape
    want = E.table(c["gray"], c["labels"], c["count"], c["max_rows"], c["G"], c["w"])
    buf = torch.full((want.size + 64,), GUARD, dtype=torch.int32)  # the call clears the table itself
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    rc = _lib.load().unet_lesion_echo_host(p(c["gray"]), p(c["labels"]), p(c["count"]), N, H, W, c["max_rows"], c["G"],
                                          c["w"], ctypes.c_void_p(buf.data_ptr()))
    assert rc == 0
    assert (buf[want.size:] == GUARD).all()
    assert np.array_equal(buf[:want.size].numpy().reshape(want.shape), want)


# ---------------------------------------------------------------- echo_descriptors
DESCRIBED = ["67x131 blobs G8 w0 random", "67x131 blobs G32 w16 random", "67x131 blobs G16 w1 ramp",
             "67x131 blobs G16 w8 const", "40x70 frame", "12x300 bars w8", "diagonal squares random",
             "67x131 seams", "negative background", "1x1 w16"]


def close(got, want, rel=1e-12):
    if isinstance(want, float) and math.isnan(want) or isinstance(want, np.floating) and np.isnan(want):
        return math.isnan(got)
    return abs(got - want) <= rel * abs(want)


@pytest.mark.parametrize("name", DESCRIBED)
def test_descriptors_against_the_pixel_lists(name):
    """Both sides are float64 formulas over the same integers: 1e-12 relative.  Two quantities get a
    different bound, for a reason on the direct side, not in echo_descriptors (which forms the integer
    numerators exactly): scipy's skewness and excess kurtosis and the dense-matrix correlation subtract
    nearly equal float sums (the third central moment of a near-symmetric histogram; sum (i - mu)(j -
    mu) P), so the direct value itself carries an absolute error of about 1e-13 and the bound for
    these three is 1e-12 relative or 1e-12 absolute, whichever is larger."""
    from unet_hip import echo_descriptors
    c = by_name(name)
    n = len(c["labels"]) - 1
    tab = host_table(c)
    d = echo_descriptors(tab, c["G"])
    assert all(v.shape == tuple(tab.shape[:-1]) for v in d.values())
    K = min(int(c["count"][n]), c["max_rows"])
    for l in list(range(1, K + 1))[:6]:
        want = E.direct_descriptors(c["gray"][n], c["labels"][n], l, c["G"], c["w"])
        assert set(want) == set(d)
        for k, v in want.items():
            got = d[k][n, l - 1]
            if k in ("skewness", "kurtosis", "glcm_correlation"):
                ok = close(got, v) or abs(got - v) <= 1e-12
            else:
                ok = close(got, v)
            assert ok, (name, l, k, got, v)


def test_descriptors_of_known_histograms():
    from unet_hip import echo_descriptors
    G = 8
    t = np.zeros((3, 512 + G * G), np.int32)
    t[0, 10], t[0, 20] = 3, 1                      # lesion 10, 10, 10, 20
    t[0, 256 + 40], t[0, 256 + 60] = 2, 2          # ring 40, 40, 60, 60
    t[0, 512 + 0 * G + 0], t[0, 512 + 0 * G + 1] = 2, 2  # pairs (0, 0) twice, (0, 1) twice
    t[1, 200] = 5                                  # constant grey, no ring, no pair
    d = echo_descriptors(t)
    assert d["pixels"].tolist() == [4, 5, 0] and d["mean"][0] == 12.5 and d["std"][0] == math.sqrt(18.75)
    assert (d["min"][0], d["max"][0], d["median"][0], d["p10"][0], d["p90"][0]) == (10, 20, 10, 10, 20)
    assert abs(d["entropy"][0] - (-(0.75 * math.log2(0.75) + 0.25 * math.log2(0.25)))) < 1e-15
    assert d["ring_pixels"].tolist() == [4, 0, 0] and d["ring_mean"][0] == 50 and d["ring_std"][0] == 10
    assert (d["ring_p25"][0], d["ring_p75"][0]) == (40, 60)
    assert d["echo_ratio"][0] == 0.25 and d["echo_class"].tolist() == [-1, 0, 0]
    assert abs(d["echo_cnr"][0] - 37.5 / math.sqrt(118.75)) < 1e-15
    # P = [[1/2, 1/4], [1/4, 0]]
    assert d["glcm_pairs"].tolist() == [4, 0, 0] and d["glcm_contrast"][0] == 0.5 and d["glcm_dissimilarity"][0] == 0.5
    assert d["glcm_homogeneity"][0] == 0.75 and d["glcm_energy"][0] == math.sqrt(0.375)
    assert abs(d["glcm_correlation"][0] - (0 - 1 / 16) / (1 / 4 - 1 / 16)) < 1e-15
    assert d["glcm_entropy"][0] == 1.5
    # constant grey: zero spread (skewness undefined), empty ring (class 0), no pair (nan)
    assert d["std"][1] == 0 and math.isnan(d["skewness"][1]) and math.isnan(d["kurtosis"][1]) and d["entropy"][1] == 0
    for k in ("ring_mean", "ring_std", "ring_p25", "ring_p75", "echo_ratio", "echo_cnr", "glcm_contrast",
              "glcm_energy", "glcm_correlation", "glcm_entropy"):
        assert math.isnan(d[k][1]), k
    assert all(v[2] == 0 for v in d.values())  # a row without pixels: zeros
    t[2, 30] = 2
    t[2, 512 + 3 * G + 3] = 1  # one level only: correlation 1
    assert echo_descriptors(t, G)["glcm_correlation"][2] == 1.0
    assert echo_descriptors(torch.from_numpy(t).reshape(3, 1, -1))["mean"].shape == (3, 1)


# ---------------------------------------------------------------- refusals
def test_refusals():
    import unet_hip
    from unet_hip import _lib
    lib = _lib.load()
    g, lab = torch.zeros((1, 4, 4), dtype=torch.uint8), torch.zeros((1, 4, 4), dtype=torch.int32)
    cnt, tab = torch.zeros(1, dtype=torch.int32), torch.zeros(512 + 32 * 32, dtype=torch.int32)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    call = lambda *a: lib.unet_lesion_echo_host(*a)
    assert call(p(g), p(lab), p(cnt), 1, 4, 4, 1, 16, 8, p(tab)) == 0
    assert call(None, p(lab), p(cnt), 1, 4, 4, 1, 16, 8, p(tab)) == -1
    assert call(p(g), None, p(cnt), 1, 4, 4, 1, 16, 8, p(tab)) == -1
    assert call(p(g), p(lab), None, 1, 4, 4, 1, 16, 8, p(tab)) == -1
    assert call(p(g), p(lab), p(cnt), 1, 4, 4, 1, 16, 8, None) == -1
    for N, H, W, rows in ((0, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (1, 4, 4, 0), (1, 1 << 16, 1 << 15, 1)):
        assert call(p(g), p(lab), p(cnt), N, H, W, rows, 16, 8, p(tab)) == -1
    for G in (0, 4, 15, 17, 64, -16):
        assert call(p(g), p(lab), p(cnt), 1, 4, 4, 1, G, 8, p(tab)) == -1
    for w in (-1, 17, 1 << 20):
        assert call(p(g), p(lab), p(cnt), 1, 4, 4, 1, 16, w, p(tab)) == -1
    assert call(p(g), p(lab), p(cnt), 1, 4097, 1, 1, 16, 8, p(tab)) == -2
    assert call(p(g), p(lab), p(cnt), 1, 1, 4097, 1, 16, 8, p(tab)) == -2
    assert lib.unet_lesion_echo(None, p(g), p(lab), p(cnt), 1, 4, 4, 1, 16, 8, p(tab), None) == -1
    with pytest.raises(unet_hip.HipUnavailable):
        unet_hip.echo_table(g, lab, cnt)
    for bad in (lambda: unet_hip.echo_table_host(g.float(), lab, cnt),
                lambda: unet_hip.echo_table_host(g[:, :3], lab, cnt),
                lambda: unet_hip.echo_table_host(g, lab.long(), cnt),
                lambda: unet_hip.echo_table_host(g, lab, torch.zeros(2, dtype=torch.int32)),
                lambda: unet_hip.echo_table_host(g, lab, cnt, levels=12),
                lambda: unet_hip.echo_table_host(g, lab, cnt, ring=17),
                lambda: unet_hip.echo_table_host(g, lab, cnt, ring=-1),
                lambda: unet_hip.echo_descriptors(tab.reshape(1, -1)[:, :600]),
                lambda: unet_hip.echo_descriptors(tab.reshape(1, -1), 16),
                lambda: unet_hip.echo_descriptors(tab.reshape(1, -1).long())):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError, match=r"torch\.float32 \(1, 4, 4\)"):
        unet_hip.echo_table_host(g.float(), lab, cnt)
    from unet_hip.predict import Predictor
    with pytest.raises(ValueError, match="lesion_table"):
        Predictor(torch.nn.Identity(), 32, "cpu", lesion_echo=True)
    with pytest.raises(ValueError, match="echo_levels"):
        Predictor(torch.nn.Identity(), 32, "cpu", lesion_table=True, lesion_echo=True, echo_levels=12)
    with pytest.raises(ValueError, match="echo_ring"):
        Predictor(torch.nn.Identity(), 32, "cpu", lesion_table=True, lesion_echo=True, echo_ring=17)


# ---------------------------------------------------------------- lesions.csv and the flags
def test_csv_lines_with_and_without_the_echo_rows():
    import unet_hip
    from unet_hip import functional as F
    from unet_hip.predict import lesion_csv_header, lesion_lines
    m = np.zeros((50, 60), np.uint8)
    m[4:11, 9:12] = 1
    m[30, 20] = 1
    gray = torch.from_numpy(E.grey("ramp", 50, 60))[None]
    out = unet_hip.lesion_morphometry_host(torch.from_numpy(m)[None], 1)
    echo = unet_hip.echo_table_host(gray, out["labels"], out["count"], levels=8, ring=2)[0]
    plain = F.lesion_csv_lines("a.png", out["table"][0], out["count"][0])
    # without the echo rows: today's bytes (the line test_morph_cpu pins) and today's header
    assert plain[0] == "a.png,1,21,10.0000,7.0000,9,4,11,10,6.3246,8.0000,3.2660,1.5708,0.9129,18.8284,0.7444,0,1"
    assert plain == F.lesion_csv_lines("a.png", out["table"][0], out["count"][0], None, 1, None)
    assert lesion_csv_header() == F.LESION_COLUMNS and lesion_csv_header(0.5) == F.LESION_COLUMNS + F.LESION_COLUMNS_MM
    assert lesion_csv_header(0.5, echo=True) == F.LESION_COLUMNS + F.LESION_COLUMNS_MM + F.LESION_COLUMNS_ECHO
    assert F.LESION_COLUMNS_ECHO == (
        "echo_mean", "echo_std", "echo_median", "echo_p10", "echo_p90", "echo_entropy", "ring_pixels", "ring_mean",
        "ring_std", "echo_ratio", "echo_cnr", "echo_class", "glcm_contrast", "glcm_homogeneity", "glcm_energy",
        "glcm_correlation", "glcm_entropy")
    with_mm = F.lesion_csv_lines("a.png", out["table"][0], 2, 0.5, 1, echo)
    assert [l.split(",")[:20] for l in with_mm] == [l.split(",") for l in F.lesion_csv_lines("a.png", out["table"][0], 2, 0.5)]
    assert all(len(l.split(",")) == 37 for l in with_mm)
    # the rectangle: columns 9..11 of the ramp, 7 rows each; the ring of width 2 around it
    d = unet_hip.echo_descriptors(echo, 8)
    f = with_mm[0].split(",")[20:]
    assert f[:6] == ["10.0000", "0.8165", "10", "9", "11", f"{math.log2(3):.4f}"]
    assert f[6] == str((7 + 4) * (3 + 4) - 21) == str(int(d["ring_pixels"][0]))
    assert f[7] == "10.0000" and f[9] == "1.0000" and f[10] == "0.0000" and f[11] == "0"
    assert f[12:] == [f"{d[k][0]:.4f}" for k in ("glcm_contrast", "glcm_homogeneity", "glcm_energy",
                                                 "glcm_correlation", "glcm_entropy")]
    g = with_mm[1].split(",")[20:]  # the single pixel: no spread, no pair
    assert g[:6] == ["20.0000", "0.0000", "20", "20", "20", "0.0000"] and g[6] == "24" and g[12:] == ["nan"] * 5
    # lesion_lines: with and without out["echo"]
    res = dict(lesions=[out["table"][0][:2], out["table"][0][:0]])
    assert lesion_lines(res, ["x/a.png", "b.png"]) == plain
    res["echo"] = [echo[:2], echo[:0]]
    assert lesion_lines(res, ["x/a.png", "b.png"], 0.5) == with_mm
    with pytest.raises(ValueError):
        F.lesion_csv_lines("a.png", out["table"][0], 2, None, 1, echo[:1])


def test_flags_parse_and_refusals(capsys):
    import main
    a = main.get_parser([])
    assert a.lesion_echo is False and a.echo_ring == 8 and a.echo_levels == 16
    ok = ["--mode", "predict", "--input_dir", "i", "--output_dir", "o", "--checkpoint_path", "c"]
    a = main.get_parser(ok + ["--lesion_table", "--lesion_echo", "--echo_ring", "0", "--echo_levels", "32"])
    assert a.lesion_echo is True and a.echo_ring == 0 and a.echo_levels == 32
    assert main.get_parser(ok + ["--lesion_table", "--lesion_echo", "--echo_ring", "16"]).echo_ring == 16
    for bad, word in ((ok + ["--lesion_echo"], "--lesion_table"),
                      (["--mode", "test", "--lesion_echo"], "--lesion_table"),
                      (["--mode", "test", "--lesion_table", "--lesion_echo"], "predict only"),
                      (ok + ["--lesion_table", "--echo_ring", "4"], "--lesion_echo"),
                      (ok + ["--lesion_table", "--echo_ring", "8"], "--lesion_echo"),  # the default value, given
                      (ok + ["--lesion_table", "--echo_levels", "16"], "--lesion_echo"),
                      (ok + ["--lesion_table", "--echo_levels", "8"], "--lesion_echo"),
                      (ok + ["--lesion_table", "--lesion_echo", "--echo_ring", "17"], "0..16"),
                      (ok + ["--lesion_table", "--lesion_echo", "--echo_ring", "-1"], "0..16"),
                      (ok + ["--lesion_table", "--lesion_echo", "--echo_levels", "12"], "invalid choice")):
        with pytest.raises(SystemExit):
            main.get_parser(bad)
        assert word in capsys.readouterr().err, bad


# ---------------------------------------------------------------- echo.h alone, under the sanitizers
def test_echo_header_builds_for_the_host_alone_and_runs_clean(tmp_path):
    """tools/echo_host_check.cpp includes echo.h with no HIP header, runs the host twin over the case
    list's shapes with exactly sized buffers and guard words against a brute-force restatement, and is
    built with -fsanitize=address,undefined: a stand-alone program, run as its own process."""
    exe = str(tmp_path / "echo_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-DECHO_HOST_ONLY", "-I", CSRC,
                           os.path.join(REPO, "tools", "echo_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env={"PATH": os.environ.get("PATH", "")})
    assert out.returncode == 0, out.stdout + out.stderr
    assert "echo_host_check ok" in out.stdout
