"""GPU: the lesion echo kernel (csrc/kernels_echo.hip) against the host twin that shares its rules
(csrc/echo.h) and against the NumPy / scipy restatement (echo_ref; the twin against it without a GPU:
test_echo_cpu.py), over the shared case list, into poisoned tables with guard words, with and
without the wave-aggregated adds; then ``Predictor(lesion_echo=True)`` and ``--mode predict
--lesion_echo`` end to end.  Every comparison of table rows is exact."""
import numpy as np
import pytest
import torch

import echo_ref as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = E.cases()
IDS = [c["name"] for c in CASES]
POISON = 0x5A5A5A5B


def dev(c):
    return [torch.from_numpy(c[k]).to(DEV) for k in ("gray", "labels", "count")]


def want_of(c):
    """The restatement's table, and the host twin's: equal (test_echo_cpu), asserted here once more."""
    import unet_hip
    ref = E.table(c["gray"], c["labels"], c["count"], c["max_rows"], c["G"], c["w"])
    host = unet_hip.echo_table_host(torch.from_numpy(c["gray"]), torch.from_numpy(c["labels"]),
                                    torch.from_numpy(c["count"]), c["max_rows"], c["G"], c["w"]).numpy()
    assert np.array_equal(host, ref), c["name"]
    return ref


def poisoned_call(c):
    """unet_lesion_echo into a table pre-filled with a poison pattern, guard words behind it."""
    from unet_hip import _lib
    from unet_hip.runtime import UNetRuntime
    rt = UNetRuntime.get(DEV)
    g, lab, cnt = dev(c)
    N, H, W = lab.shape
    words = N * c["max_rows"] * (512 + c["G"] ** 2)
    buf = torch.full((words + 64,), POISON, dtype=torch.int32, device=DEV)
    rc = rt.lib.unet_lesion_echo(rt.ctx, _lib.ptr(g), _lib.ptr(lab), _lib.ptr(cnt), N, H, W, c["max_rows"], c["G"],
                                 c["w"], _lib.ptr(buf), _lib.stream_ptr(DEV))
    _lib.check(rc, rt.ctx, "unet_lesion_echo")
    out = buf.cpu().numpy()
    assert (out[words:] == POISON).all(), c["name"]
    return out[:words].reshape(N, c["max_rows"], -1)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_device_equals_host_twin_and_restatement(c):
    import unet_hip
    want = want_of(c)
    assert np.array_equal(poisoned_call(c), want)
    g, lab, cnt = dev(c)
    got = unet_hip.echo_table(g, lab, cnt, c["max_rows"], c["G"], c["w"])
    assert got.dtype == torch.int32 and got.device.type == "cuda"
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("agg", (1, 0))
def test_aggregated_and_plain_lds_adds_agree(agg):
    """Option echo_agg: every add aggregated over the wave first, or one LDS atomic per lane."""
    from unet_hip.runtime import UNetRuntime
    UNetRuntime.get(DEV).set_option("echo_agg", agg)  # restored after the test (conftest)
    for name in ("67x131 blobs G16 w8 const", "67x131 blobs G32 w16 random", "33x70 checkerboard G16 w1",
                 "N3 counts 0 1 many", "N3 max_rows 3", "40x70 frame", "12x300 bars w16"):
        c = CASES[IDS.index(name)]
        assert np.array_equal(poisoned_call(c), want_of(c)), name


def test_more_labels_than_slots_take_the_overflow_path():
    """The checkerboard puts hundreds of labels into every tile and the LDS table has 5 slots at most:
    nearly every count goes straight to global memory.  No pair anywhere."""
    import unet_hip
    for name in ("33x70 checkerboard G16 w1", "33x70 checkerboard G32 w0", "33x70 checkerboard G8 w16"):
        c = CASES[IDS.index(name)]
        got = poisoned_call(c)
        assert np.array_equal(got, want_of(c))
        assert got.shape[1] == 33 * 35 and (unet_hip.echo_descriptors(got)["glcm_pairs"] == 0).all()


def test_lesion_echo_labels_then_counts_and_run_to_run():
    """Components and table in one call; a large shape, a small one and the large one again on one
    context give the same tables every time."""
    import unet_hip
    big, small = E.blobs(96, 160, 21), E.blobs(33, 65, 22)
    gb, gs = E.grey("random", 96, 160, 23), E.grey("ramp", 33, 65)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint8))[None]
    for conn in (1, 2):
        want_b = unet_hip.lesion_echo_host(t(big), t(gb), conn, levels=32, ring=16)
        want_s = unet_hip.lesion_echo_host(t(small), t(gs), conn, levels=8, ring=3)
        for _ in range(2):
            got = unet_hip.lesion_echo(t(big).to(DEV), t(gb).to(DEV), conn, levels=32, ring=16)
            assert torch.equal(got["count"].cpu(), want_b["count"]) and torch.equal(got["labels"].cpu(), want_b["labels"])
            assert torch.equal(got["table"].cpu(), want_b["table"])
            got = unet_hip.lesion_echo(t(small).to(DEV), t(gs).to(DEV), conn, levels=8, ring=3)
            assert torch.equal(got["table"].cpu(), want_s["table"])
        lab = want_b["labels"][0].numpy()
        assert np.array_equal(want_b["table"].numpy(),
                              E.table(gb[None], lab[None], want_b["count"].numpy(), int(want_b["count"][0]), 32, 16))


def test_refusals_on_the_device():
    import unet_hip
    g = torch.zeros((1, 4, 4), dtype=torch.uint8, device=DEV)
    lab = torch.zeros((1, 4, 4), dtype=torch.int32, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(unet_hip.HipError, match="UNET_ERR_INVALID"):
        unet_hip.echo_table(g, lab, cnt, 0)
    wide = torch.zeros((1, 1, 4097), dtype=torch.int32, device=DEV)
    with pytest.raises(unet_hip.HipError, match="UNET_ERR_SHAPE"):
        unet_hip.echo_table(wide.to(torch.uint8), wide, cnt, 1)
    with pytest.raises(ValueError):
        unet_hip.echo_table(g.cpu(), lab, cnt)
    with pytest.raises(ValueError):
        unet_hip.echo_table(g, lab, cnt, levels=64)
    assert not unet_hip.echo_table(g, lab, cnt, 2).any()


# ---------------------------------------------------------------- Predictor(lesion_echo=True)
class _Gated(torch.nn.Module):
    """The tiny random-weight network, with an all-black frame sent far below the threshold so that
    one frame of the test has an empty mask whatever the weights say."""

    def __init__(self):
        super().__init__()
        from test_gpu_export import small_model
        self.net = small_model()

    def forward(self, x):
        return self.net(x) - 1e4 * (x.amax(dim=(1, 2, 3), keepdim=True) == 0)


def test_predictor_echo_rows_equal_the_host_twin_of_the_masks():
    """Three frames of two sizes, one black (an empty mask): out["echo"] is echo_table_host of each
    returned mask's components and the frame itself, and the other outputs do not notice the flag."""
    import unet_hip
    from test_gpu_export import frames
    a, b, _ = frames()
    planes = [a, b, np.zeros_like(a)]
    model = _Gated()
    plain = unet_hip.Predictor(model, 32, DEV, pp=dict(connectivity=2), lesion_table=True)(planes)
    out = unet_hip.Predictor(model, 32, DEV, pp=dict(connectivity=2), lesion_table=True, lesion_echo=True,
                             echo_ring=5, echo_levels=8)(planes)
    assert "echo" not in plain and len(out["echo"]) == 3
    comps = [r["components"] for r in out["rows"]]
    print("components per frame:", comps)
    assert comps[2] == 0 and sum(comps) >= 1
    for i, f in enumerate(planes):
        assert torch.equal(out["masks"][i], plain["masks"][i]) and torch.equal(out["lesions"][i], plain["lesions"][i])
        e = out["echo"][i]
        assert e.dtype == torch.int32 and e.device.type == "cpu" and tuple(e.shape) == (comps[i], 512 + 64)
        if comps[i]:
            want = unet_hip.lesion_echo_host(out["masks"][i].cpu()[None], torch.from_numpy(f)[None], 2, levels=8, ring=5)
            assert int(want["count"][0]) == comps[i]
            assert torch.equal(e, want["table"][0])


# ---------------------------------------------------------------- --mode predict --lesion_echo
def test_main_predict_lesion_echo(tmp_path):
    """lesions.csv without --lesion_echo is what it was; with it every line gains the seventeen columns
    of echo_descriptors(echo_table_host(...)) of the written mask and the frame."""
    import scipy.ndimage as nd
    import unet_hip
    from PIL import Image
    from test_gpu_export import frames, small_model
    from test_gpu_morph import _predict
    from unet_hip import functional as F
    src = tmp_path / "in"
    src.mkdir()
    names = ["a.png", "b.png", "c.png"]
    for n, f in zip(names, frames()):
        Image.fromarray(f, "L").save(src / n)
    ckpt = tmp_path / "m.pth"
    torch.save({k: v.detach().clone().cpu() for k, v in small_model().state_dict().items()}, ckpt)
    table = _predict(tmp_path, src, ckpt, "table", ["--lesion_table"])
    echo = _predict(tmp_path, src, ckpt, "echo", ["--lesion_table", "--lesion_echo", "--echo_ring", "4"])
    assert (table / "predictions.csv").read_bytes() == (echo / "predictions.csv").read_bytes()
    old, new = (table / "lesions.csv").read_text().splitlines(), (echo / "lesions.csv").read_text().splitlines()
    assert old[0] == ",".join(F.LESION_COLUMNS) and new[0] == ",".join(F.LESION_COLUMNS + F.LESION_COLUMNS_ECHO)
    assert len(old) == len(new) >= 2
    assert [l.split(",")[:18] for l in new] == [l.split(",") for l in old]
    want = []
    for n, f in zip(names, frames()):
        mask = np.asarray(Image.open(echo / f"{n[:-4]}_mask.png")) != 0
        lab, k = nd.label(mask, np.ones((3, 3)))  # _predict runs at --pp_connectivity 2
        if k == 0:
            continue
        tab = unet_hip.echo_table_host(torch.from_numpy(f)[None], torch.from_numpy(lab.astype(np.int32))[None],
                                       torch.tensor([k], dtype=torch.int32), k, 16, 4)[0]
        morph = unet_hip.morphometry_table_host(torch.from_numpy(lab.astype(np.int32))[None],
                                                torch.tensor([k], dtype=torch.int32))[0]
        want += F.lesion_csv_lines(n, morph, k, None, 2, tab)
    assert new[1:] == want
