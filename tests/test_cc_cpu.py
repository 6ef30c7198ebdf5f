"""CPU: the host twins of the connected-component entry points (unet_components_host,
unet_postprocess_host, unet_lesion_stats_host: csrc/cc.h compiled for the host) against scipy on
every case of cc_ref.py.  All integer, all exact (np.array_equal, no tolerance)."""
import ctypes

import numpy as np
import pytest
import torch

import cc_ref as R

CASES = R.mask_cases()


def u8(m):
    return torch.from_numpy(np.ascontiguousarray(m).astype(np.uint8))


def host_label(m, conn, **kw):
    import unet_hip
    lab, cnt = unet_hip.connected_components_host(m if isinstance(m, torch.Tensor) else u8(m), conn, **kw)
    assert lab.dtype == torch.int32 and cnt.dtype == torch.int32
    return lab.numpy(), cnt.numpy()


def check_labels(masks, lab, cnt, conn):
    for n, m in enumerate(masks):
        want, k = R.label(m, conn)
        assert cnt[n] == k, (n, cnt[n], k)
        assert np.array_equal(lab[n], want), (n, R.PATTERNS[n] if len(masks) == len(R.PATTERNS) else "")


@pytest.mark.parametrize("conn", R.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(CASES))
def test_labels_match_scipy(name, conn):
    lab, cnt = host_label(CASES[name], conn)
    check_labels(CASES[name], lab, cnt, conn)


def test_known_component_counts():
    """The counts the patterns are built for (scipy agrees: cc_ref.label)."""
    for (H, W), conn in [((33, 65), 1), ((33, 65), 2), ((96, 160), 1)]:
        P = dict(zip(R.PATTERNS, R.patterns(H, W)))
        count = {k: R.label(v, conn)[1] for k, v in P.items()}
        assert count["serpentine"] == 1 and count["spiral"] == 1 and count["full"] == 1 and count["empty"] == 0
        assert count["checkerboard"] == ((H * W + 1) // 2 if conn == 1 else 1)
        assert count["diagonal"] == count["antidiagonal"] == (min(H, W) if conn == 1 else 1)
        assert count["comb"] == 1 and count["tie"] == 2


def test_big_batch_matches_scipy():
    m = R.big_case()
    for conn in R.CONNECTIVITIES:
        lab, cnt = host_label(m, conn)
        check_labels(m, lab, cnt, conn)


def test_kinds_and_extra_channels():
    """Logits and targets go through the mask readout of unet_mask_counts; channels above 0 are
    not read; the threshold-edge logits give the components of sigmoid(x) > 0.5 in float32."""
    m = R.patterns(33, 65)
    for conn in R.CONNECTIVITIES:
        lab, cnt = host_label(torch.from_numpy(R.to_logits(m)), conn)
        check_labels(m, lab, cnt, conn)
        t = R.to_targets(m)
        lab, cnt = host_label(torch.from_numpy(t), conn, kind="targets")
        check_labels(t[:, 0].astype(np.uint8) == 1, lab, cnt, conn)
        x = R.edge_logits()
        lab, cnt = host_label(torch.from_numpy(x), conn)
        pr = R.readout(x[:, 0])
        assert not pr[x[:, 0] == 0].any() and not pr[x[:, 0] == R.EDGE_LOGITS[1]].any() and pr[x[:, 0] == 1].all()
        check_labels(pr, lab, cnt, conn)
    # a (H, W) bool mask is one sample
    lab, cnt = host_label(torch.from_numpy(m[5]), 1)
    assert lab.shape == (1, 33, 65) and np.array_equal(lab[0], R.label(m[5], 1)[0])


def check_postprocess(masks, conn, kl, ma, fh):
    import unet_hip
    out, info = unet_hip.postprocess_mask_host(u8(masks), keep_largest=kl, min_area=ma, fill_holes=fh,
                                               connectivity=conn)
    assert out.dtype == torch.uint8 and info.dtype == torch.int64 and int(out.max()) <= 1
    for n, m in enumerate(masks):
        want, winfo = R.postprocess(m, conn, kl, ma, fh)
        assert np.array_equal(out[n].numpy().astype(bool), want), (n, conn, kl, ma, fh)
        assert info[n].tolist() == winfo, (n, conn, kl, ma, fh, info[n].tolist(), winfo)


@pytest.mark.parametrize("conn", R.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(CASES))
def test_postprocess_matches_scipy_composition(name, conn):
    """The three options in every combination (min_area 0 or 8) on every pattern: rings, nested
    rings, the open ring and the noise among them."""
    for kl, small, fh in R.OPTIONS:
        check_postprocess(CASES[name], conn, kl, 8 if small else 0, fh)


@pytest.mark.parametrize("conn", R.CONNECTIVITIES)
def test_min_area_edges_and_ties(conn):
    """min_area equal to a component's area keeps it, one above removes it, above the largest
    removes everything; of two equal components the later one in raster order loses, and wins
    once it is larger."""
    for name in ("33x65", "7x5", "1x130"):
        for n, m in enumerate(CASES[name]):
            for ma in R.min_areas(m, conn):
                for kl in (False, True):
                    check_postprocess(m[None], conn, kl, ma, True)
    import unet_hip
    for size in ((33, 65), (130, 1)):
        P = dict(zip(R.PATTERNS, R.patterns(*size)))
        for key, first in (("tie", True), ("tie_swapped", False)):
            out, info = unet_hip.postprocess_mask_host(u8(P[key][None]), keep_largest=True, connectivity=conn)
            lab, k = R.label(P[key], conn)
            assert k == 2 and info[0].tolist()[:2] == [2, 1]
            assert np.array_equal(out[0].numpy().astype(bool), lab == (1 if first else 2))
    e = np.zeros((1, 7, 5), bool)
    for kl, small, fh in R.OPTIONS:
        out, info = unet_hip.postprocess_mask_host(u8(e), kl, 8 if small else 0, fh, conn)
        assert not out.any() and info[0].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("conn", R.CONNECTIVITIES)
def test_lesion_stats_match_numpy(conn):
    import unet_hip
    for name in ("33x65", "96x160", "7x5", "1x1"):
        P = CASES[name]
        G = np.roll(P, 3, axis=0)[:, ::-1].copy()  # another pattern against each one
        for pred, kind in ((u8(P), None), (torch.from_numpy(R.to_logits(P)), None)):
            got = unet_hip.lesion_metrics_host(pred, torch.from_numpy(R.to_targets(G)), conn, kind)
            assert list(got) == ["n_pred", "n_gt", "gt_hit", "pred_hit"]
            g = R.to_targets(G)[:, 0].astype(np.uint8) == 1
            for n in range(len(P)):
                assert [int(got[k][n]) for k in got] == R.lesion(P[n], g[n], conn), (name, n)


def test_invalid_arguments_are_refused():
    import unet_hip
    from unet_hip import _lib
    lib = _lib.load()
    m = np.ones((1, 1, 4, 4), np.uint8)
    lab, cnt = np.zeros((1, 4, 4), np.int32), np.zeros(1, np.int32)
    out, info = np.zeros((1, 4, 4), np.uint8), np.zeros(4, np.int64)
    t = np.ones((1, 1, 4, 4), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert lib.unet_components_host(p(m), 0, 1, 1, 4, 4, 1, p(lab), p(cnt)) == 0
    bad = [(0, 1, 1, 4, 4, 0), (0, 1, 1, 4, 4, 3), (3, 1, 1, 4, 4, 1), (-1, 1, 1, 4, 4, 1), (0, 0, 1, 4, 4, 1),
           (0, 1, 1, 0, 4, 1), (0, 1, 1, 4, 0, 1), (0, 1, 1, 1 << 16, 1 << 15, 1)]
    for kind, N, C, H, W, conn in bad:
        assert lib.unet_components_host(p(m), kind, N, C, H, W, conn, p(lab), p(cnt)) == -1
        assert lib.unet_postprocess_host(p(m), kind, N, C, H, W, conn, 1, 0, 1, p(out), p(info)) == -1
        assert lib.unet_lesion_stats_host(p(m), kind, p(t), N, C, H, W, conn, p(info)) == -1
    assert lib.unet_components_host(None, 0, 1, 1, 4, 4, 1, p(lab), p(cnt)) == -1
    # the device entry points refuse the same before touching the device, with a message
    from unet_hip.runtime import UNetRuntime
    rt = UNetRuntime("cuda:0")  # creating a context performs no device work
    d = ctypes.c_void_p(256)
    for kind, N, C, H, W, conn in bad:
        assert rt.lib.unet_components(rt.ctx, d, kind, N, C, H, W, conn, d, d, None) == -1
        assert rt.lib.unet_last_error(rt.ctx).startswith(b"components: ")
        assert rt.lib.unet_postprocess(rt.ctx, d, kind, N, C, H, W, conn, 1, 0, 1, ctypes.c_void_p(512), d, None) == -1
        assert rt.lib.unet_lesion_stats(rt.ctx, d, kind, d, N, C, H, W, conn, d, None) == -1
    assert b"connectivity" in (rt.lib.unet_components(rt.ctx, d, 0, 1, 1, 4, 4, 5, d, d, None),
                               rt.lib.unet_last_error(rt.ctx))[1]
    with pytest.raises(ValueError):
        unet_hip.connected_components_host(torch.zeros(4, 4), kind="nope")
    with pytest.raises(unet_hip.HipUnavailable):
        unet_hip.connected_components(torch.zeros(4, 4, dtype=torch.uint8))
