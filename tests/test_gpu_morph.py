"""GPU: the lesion-morphometry kernels (csrc/kernels_morph.hip) against the host twin that shares
their rules (csrc/morph.h; the twin against NumPy / scipy: test_morph_cpu.py), against the NumPy
restatement directly on the 512 x 512 batches, and the two command-line paths built on them
(``--mode predict --lesion_table``, ``--mode test --lesion_shape``) end to end.  Every comparison of
table rows is exact."""
import numpy as np
import pytest
import torch

import cc_ref as R
import morph_ref as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PLANES = M.all_planes()
CASES = R.mask_cases()
GUARD = -0x5A5A5A5A5A5A5A5B


def u8(m):
    return torch.from_numpy(np.ascontiguousarray(m).astype(np.uint8))


def by_size():
    """(H, W) -> bool (n, H, W): the planes of PLANES grouped into one batch per size."""
    groups = {}
    for _, m in PLANES:
        groups.setdefault(m.shape, []).append(m)
    return {k: np.stack(v) for k, v in groups.items()}


@pytest.mark.parametrize("conn", R.CONNECTIVITIES)
def test_device_matches_host_twin_plane_by_plane(conn):
    import unet_hip
    for name, m in PLANES:
        x = u8(m[None])
        got = unet_hip.lesion_morphometry(x.to(DEV), conn)
        want = unet_hip.lesion_morphometry_host(x, conn)
        assert got["table"].dtype == torch.int64 and got["table"].device.type == "cuda"
        assert np.array_equal(got["count"].cpu().numpy(), want["count"].numpy()), name
        assert np.array_equal(got["table"].cpu().numpy(), want["table"].numpy()), name


@pytest.mark.parametrize("conn", R.CONNECTIVITIES)
def test_device_matches_host_twin_in_batches(conn):
    """Every size as one batch (mixed planes, mixed counts): sample offsets of the table, of the
    offsets and of the extents."""
    import unet_hip
    for shape, batch in by_size().items():
        x = u8(batch)
        got = unet_hip.lesion_morphometry(x.to(DEV), conn)
        want = unet_hip.lesion_morphometry_host(x, conn)
        assert np.array_equal(got["table"].cpu().numpy(), want["table"].numpy()), shape
    x = u8(CASES["33x65"][[2, 11, 0]])
    got = unet_hip.lesion_morphometry(x.to(DEV), conn)  # N = 3: noise, a ring, an empty plane
    want = unet_hip.lesion_morphometry_host(x, conn)
    assert np.array_equal(got["table"].cpu().numpy(), want["table"].numpy())
    assert not got["table"][2].any()


@pytest.mark.parametrize("lds", (1, 0))
def test_lds_table_and_direct_atomics_agree(lds):
    """Option morph_lds: the block's LDS table, or every contribution straight to global memory."""
    import unet_hip
    from unet_hip.runtime import UNetRuntime
    UNetRuntime.get(DEV).set_option("morph_lds", lds)  # restored after the test (conftest)
    for conn in R.CONNECTIVITIES:
        x = u8(CASES["96x160"])
        got = unet_hip.lesion_morphometry(x.to(DEV), conn)
        want = unet_hip.lesion_morphometry_host(x, conn)
        assert np.array_equal(got["table"].cpu().numpy(), want["table"].numpy())


def test_big_case_and_ellipses_against_the_restatement():
    import unet_hip
    for batch in (R.big_case(), M.ellipse_batch()):
        for conn in R.CONNECTIVITIES:
            got = unet_hip.lesion_morphometry(u8(batch).to(DEV), conn)
            tab, cnt = got["table"].cpu().numpy(), got["count"].cpu().numpy()
            for n, m in enumerate(batch):
                lab, k = R.label(m, conn)
                assert cnt[n] == k
                assert np.array_equal(tab[n, :k], M.table(lab)[:k])
                assert not tab[n, k:].any()


@pytest.mark.parametrize("conn", R.CONNECTIVITIES)
def test_overflow_rows_are_dropped_and_guards_stay(conn):
    import unet_hip
    from unet_hip import _lib
    from unet_hip.runtime import UNetRuntime
    rt = UNetRuntime.get(DEV)
    x = u8(CASES["33x65"][[2, 14]])  # noise (many components) and the tie pair (two)
    lab, cnt = unet_hip.connected_components(x.to(DEV), conn)
    full = unet_hip.morphometry_table_host(lab.cpu(), cnt.cpu()).numpy()
    K = int(cnt.max())
    assert K > 3
    for rows in (1, K - 1):
        buf = torch.full((2 * rows * 16 + 64,), GUARD, dtype=torch.int64, device=DEV)
        rc = rt.lib.unet_morphometry(rt.ctx, _lib.ptr(lab), _lib.ptr(cnt), 2, 33, 65, rows, _lib.ptr(buf),
                                     _lib.stream_ptr(DEV))
        _lib.check(rc, rt.ctx, "unet_morphometry")
        out = buf.cpu().numpy()
        assert (out[2 * rows * 16:] == GUARD).all()
        assert np.array_equal(out[:2 * rows * 16].reshape(2, rows, 16), full[:, :rows])
        assert np.array_equal(cnt.cpu().numpy(), [R.label(m, conn)[1] for m in x.numpy()])  # count stays true


def test_scratch_reuse_and_run_to_run():
    """A large call, then a smaller batch on the same context (its scratch is reused, not regrown),
    then the large one again: every result equals the host twin's, and repeated calls are identical."""
    import unet_hip
    big, small = u8(CASES["96x160"]), u8(CASES["33x65"][:3])
    want_big = unet_hip.lesion_morphometry_host(big, 2)["table"].numpy()
    want_small = unet_hip.lesion_morphometry_host(small, 2)["table"].numpy()
    first = unet_hip.lesion_morphometry(big.to(DEV), 2)["table"].cpu().numpy()
    assert np.array_equal(first, want_big)
    assert np.array_equal(unet_hip.lesion_morphometry(small.to(DEV), 2)["table"].cpu().numpy(), want_small)
    for _ in range(3):
        assert np.array_equal(unet_hip.lesion_morphometry(big.to(DEV), 2)["table"].cpu().numpy(), first)


def test_refusals_on_the_device():
    import unet_hip
    lab = torch.zeros((1, 4, 4), dtype=torch.int32, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(unet_hip.HipError, match="UNET_ERR_INVALID"):
        unet_hip.morphometry_table(lab, cnt, 0)
    wide = torch.zeros((1, 1, 4097), dtype=torch.int32, device=DEV)
    with pytest.raises(unet_hip.HipError, match="UNET_ERR_SHAPE"):
        unet_hip.morphometry_table(wide, cnt, 1)


# ---------------------------------------------------------------- --mode predict --lesion_table
def _predict(tmp, src, ckpt, name, extra):
    import main
    dst = tmp / name
    argv = ["--mode", "predict", "--input_dir", str(src), "--output_dir", str(dst), "--model_type", "ResUNet",
            "--base_filters", "16", "--depth", "3", "--image_size", "32", "--checkpoint_path", str(ckpt),
            "--batch_size", "2", "--pp_connectivity", "2"] + extra
    main.main(main.get_parser(argv))
    return dst


def test_main_predict_lesion_table(tmp_path):
    """Three frames of different sizes (two batches): lesions.csv equals the descriptors of the written
    mask files labelled by scipy and measured by morph_ref; predictions.csv does not notice the flag."""
    import unet_hip
    from PIL import Image
    from test_gpu_export import frames, small_model
    from unet_hip import functional as F
    src = tmp_path / "in"
    src.mkdir()
    names = ["a.png", "b.png", "c.png"]
    for n, f in zip(names, frames()):
        Image.fromarray(f, "L").save(src / n)
    ckpt = tmp_path / "m.pth"
    torch.save({k: v.detach().clone().cpu() for k, v in small_model().state_dict().items()}, ckpt)
    plain = _predict(tmp_path, src, ckpt, "plain", [])
    table = _predict(tmp_path, src, ckpt, "table", ["--lesion_table", "--pixel_spacing", "0.125"])
    assert (plain / "predictions.csv").read_bytes() == (table / "predictions.csv").read_bytes()
    assert not (plain / "lesions.csv").exists()
    lines = (table / "lesions.csv").read_text().splitlines()
    assert lines[0] == ",".join(F.LESION_COLUMNS + F.LESION_COLUMNS_MM)
    want, comps = [], []
    for n in names:
        mask = np.asarray(Image.open(table / f"{n[:-4]}_mask.png")) != 0
        lab, k = R.label(mask, 2)
        comps.append(k)
        if k:
            want += F.lesion_csv_lines(n, M.table(lab), k, 0.125, 2)
    print("components per frame:", comps)
    assert sum(comps) >= 1
    assert lines[1:] == want
    csv = (table / "predictions.csv").read_text().splitlines()[1:]
    assert [int(l.split(",")[-1]) for l in csv] == comps


# ---------------------------------------------------------------- --mode test --lesion_shape
def _shape_block(keep, conn=1):
    """The SHAPE sums from kept (images, targets, predicted mask) batches, on the host: scipy labels,
    morph_ref rows, the largest component of each, and the issue's formulas."""
    n = 0
    fe = ar = ce = 0.0
    ttw = [0, 0, 0, 0]
    for _, targets, mask in keep:
        for g, p in zip(targets.numpy(), mask.numpy()):
            rp = M.largest_row(M.table(R.label(p[0] != 0, conn)[0]))
            rg = M.largest_row(M.table(R.label(g[0].astype(np.int64) == 1, conn)[0]))
            if rp is None or rg is None:
                continue
            n += 1
            fe += abs(np.sqrt(float(rp[14])) - np.sqrt(float(rg[14])))
            ar += abs(int(rp[0]) - int(rg[0])) / int(rg[0])
            ce += np.hypot(rp[1] / rp[0] - rg[1] / rg[0], rp[2] / rp[0] - rg[2] / rg[0])
            tp, tg = rp[9] - rp[7] > rp[8] - rp[6], rg[9] - rg[7] > rg[8] - rg[6]
            ttw[0 if tp and tg else 1 if tp else 2 if tg else 3] += 1
    return n, fe, ar, ce, ttw


def _check_shape(m, block, rel=1e-12):
    n, fe, ar, ce, ttw = block
    assert m["Shape_Pairs"] == n and m["Shape_TTW"] == ttw
    for key, s in (("Shape_FeretMAE", fe), ("Shape_AreaRelErr", ar), ("Shape_CentroidDist", ce)):
        assert n and abs(m[key] - s / n) <= rel * max(s / n, 1e-300), (key, m[key], s / n)
    a, b, c, d = ttw
    pe = ((a + b) * (a + c) + (c + d) * (b + d)) / (n * n)
    if pe == 1:
        assert np.isnan(m["Shape_TTWKappa"])
    else:
        assert abs(m["Shape_TTWKappa"] - ((a + d) / n - pe) / (1 - pe)) <= 1e-12


def test_trainer_test_shape_block(tmp_path, capsys, monkeypatch):
    from test_gpu_surface import _trainer
    from utils.trainer import Trainer
    kept = []
    monkeypatch.setattr(Trainer, "_can_plot", staticmethod(lambda: True))
    monkeypatch.setattr(Trainer, "_plot_contours", lambda self, keep: kept.append(keep))
    tr, _ = _trainer(tmp_path, lesion_metrics=True, lesion_shape=True)
    for e in range(3):  # enough for non-trivial masks
        tr.train_one_epoch(e)
    m = tr.test()
    out = capsys.readouterr().out
    tr.config.lesion_shape = False
    before = tr.test()
    earlier = capsys.readouterr().out
    assert list(m)[:len(before)] == list(before) and all(m[k] == before[k] or m[k] != m[k] for k in before)
    assert list(m)[len(before):] == ["Shape_Pairs", "Shape_FeretMAE", "Shape_AreaRelErr", "Shape_CentroidDist",
                                     "Shape_TTW", "Shape_TTWKappa"]
    assert out.count("SHAPE (largest component, raw masks, connectivity 1)") >= 1 and "SHAPE" not in earlier
    assert "Lesion Metrics" in out.split("SHAPE (")[0]  # the block comes after the existing ones
    print({k: m[k] for k in m if k.startswith("Shape_")})
    assert len(kept) == 2 and sum(len(k[0]) for k in kept[0]) == 6
    _check_shape(m, _shape_block(kept[0]))


def _shape_body(rank, world, tmp, ckpt):
    import test_gpu_dist_eval as D
    from utils.trainer import Trainer
    Trainer._can_plot = staticmethod(lambda: False)
    tr, _ = D._trainer(rank, world, tmp, (D.TRAIN, D.VAL, D.TEST), 3, lesion_shape=True, pp_largest=True)
    tr.model.load_state_dict(torch.load(ckpt, weights_only=True))
    m = tr.test()
    return {k: v for k, v in m.items() if k.startswith("Shape_")}


def test_shape_block_dp2_equals_single_process(tmp_path):
    """Two ranks (gloo, both on cuda:0) over DataParallel shards of the 7-sample test split (2 + 1,
    2 + 1, 1 + empty) against one process that walks the same shards in turn: the counts exactly, the
    means to the rounding of a different summation order."""
    import test_gpu_dist_eval as D
    from data.data_loader import DataParallelShardSampler, dp_collate
    from test_gpu_surface import _trainer
    tr, _ = _trainer(tmp_path / "single", lesion_shape=True, pp_largest=True)
    for e in range(3):
        tr.train_one_epoch(e)
    ckpt = str(tmp_path / "m.pth")
    torch.save({k: v.detach().clone().cpu() for k, v in tr.model.state_dict().items()}, ckpt)
    shards = [list(DataParallelShardSampler(D.TEST[0], 3, False, r, 2)) for r in range(2)]
    batches = [b for pair in zip(*shards) for b in pair if b]
    assert [len(b) for b in batches] == [2, 1, 2, 1, 1]
    tr.test_loader = torch.utils.data.DataLoader(D._dataset(*D.TEST), batch_sampler=batches, collate_fn=dp_collate())
    single = {k: v for k, v in tr.test().items() if k.startswith("Shape_")}
    r0, r1 = D._spawn(_shape_body, str(tmp_path), ckpt)
    print(single, r0)
    same = lambda a, b: a == b or (a != a and b != b)  # nan: no kappa when chance agreement is 1
    assert list(r0) == list(r1) == list(single) and all(same(r0[k], r1[k]) for k in r0)
    assert 1 <= single["Shape_Pairs"] <= 6  # the blanked target is no pair
    for k, v in single.items():
        if isinstance(v, float):
            assert abs(r0[k] - v) <= 1e-12 * max(abs(v), 1e-300) or (v != v and r0[k] != r0[k]), (k, r0[k], v)
        else:
            assert r0[k] == v, (k, r0[k], v)
