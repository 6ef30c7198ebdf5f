"""unet_mask_counts (mask_counts_kernel, kernels_misc.hip) at the edges of its contract:
counts are accumulated (+=), `mask` may be null, a target is positive where (int)t == 1 and
negative where (int)t == 0, the IoU pair counts t != 0, and the prediction is
sigmoid(x) > 0.5 in float32.

Targets stay inside [-1, 255): the device casts (uint8_t)(int)t and NumPy astype(int64); both
are defined and agree on == 0 / == 1 there (a target of 256 would wrap to 0 on the device)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BAND = 2.0 ** -20  # below it the float32 sigmoid may round to exactly 0.5
TARGETS = np.array([0, 1, 0.5, 0.999, 1.5, 2, -0.5, -1], np.float32)
LOGITS = np.array([0.0, -0.0, 1e-40, -1e-40, 1e-3, -1e-3, 100.0, -100.0, 1e-7, -1e-7, 3e-8, -3e-8,
                   2.0 ** -24, -2.0 ** -24, 2.0 ** -21, -2.0 ** -21, 2.0 ** -20, -2.0 ** -20], np.float32)
START = [7, 11, 13, 17, 19, 23]


def _rt():
    import unet_hip
    return unet_hip.UNetRuntime.get(DEV)


def _inputs(n, seed):
    """Logits: the special values, tiled, then N(0, 3); targets drawn from TARGETS so that every
    (special logit, target value) pair occurs when n allows."""
    g = np.random.default_rng(seed)
    x = (g.standard_normal(n) * 3).astype(np.float32)
    k = min(n, 8 * LOGITS.size)
    i = np.arange(k)
    x[:k] = LOGITS[i % LOGITS.size]
    t = g.choice(TARGETS, size=n).astype(np.float32)
    t[:k] = TARGETS[(i + i // 72) % 8]  # (18 logits x 8 targets: lcm 72, then the other parity)
    if n == 1:
        x[0], t[0] = 0.7, 1.0
    return x, t


def _host_pred(x):
    """surf_pred (surf.h) evaluated by the host: the library's host twin of the connected
    components reads its logits through it."""
    import unet_hip
    labels, _ = unet_hip.connected_components_host(torch.from_numpy(x.reshape(1, 1, 1, -1).copy()),
                                                   kind="logits")
    return labels.numpy().reshape(-1) != 0


def _want(pr, t):
    ti = t.astype(np.int64)  # targets in [-1, 255): see the module docstring
    pos, neg, nz = ti == 1, ti == 0, t != 0
    return [int((pr & pos).sum()), int((pr & neg).sum()), int((~pr & pos).sum()),
            int((~pr & neg).sum()), int((pr & nz).sum()), int((pr | nz).sum())]


def _check_mask(mask, x):
    far = np.abs(x) >= BAND
    assert np.array_equal(mask[far], x[far] > 0), "mask differs from x > 0 outside the 0.5 band"
    near = ~far
    if near.any():  # there the float32 sigmoid legitimately rounds to 0.5
        ok = (mask[near] == _host_pred(x[near])) | (mask[near] == (x[near] > 0))
        assert ok.all(), x[near][~ok]


@pytest.mark.parametrize("n", [1, 63, 64, 257, 2048 * 256 + 77])
def test_mask_counts_contract(n):
    """n = 2048 * 256 + 77 runs the grid-stride loop twice (grid_for(n, 256, 2048))."""
    rt = _rt()
    x, t = _inputs(n, n)
    assert t.min() >= -1 and t.max() < 255
    xd, td = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
    counts = torch.tensor(START, dtype=torch.int64, device=DEV)
    mask = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
    rt.mask_counts(xd, td, counts, mask)
    mk = mask.cpu().numpy()
    assert set(np.unique(mk)) <= {0, 1}
    pr = mk.astype(bool)
    _check_mask(pr, x)
    want = _want(pr, t)  # the counts agree with the mask the kernel itself wrote
    assert counts.cpu().tolist() == [a + b for a, b in zip(START, want)]
    if n >= 63:  # every class of target occurs, so a wrong predicate shows in a count
        ti = t.astype(np.int64)
        assert ((ti == 0) & (t != 0)).any() and ((ti != 0) & (ti != 1)).any()
    rt.mask_counts(xd, td, counts, mask)  # a second call accumulates
    assert counts.cpu().tolist() == [a + 2 * b for a, b in zip(START, want)]
    assert np.array_equal(mask.cpu().numpy(), mk)
    c2 = torch.tensor(START, dtype=torch.int64, device=DEV)
    rt.mask_counts(xd, td, c2, None)  # no mask wanted: the same counts
    assert c2.cpu().tolist() == [a + b for a, b in zip(START, want)]


def test_three_readouts_agree():
    """One batch read three ways gives one foreground set: the mask of unet_mask_counts, the
    non-zero labels of connected_components on the logits, and surface_stats' `defined` flag,
    0 exactly for the sample without a foreground pixel."""
    import unet_hip
    rt = _rt()
    N, H, W = 3, 16, 24
    g = np.random.default_rng(5)
    x = (g.standard_normal((N, 1, H, W)) * 2).astype(np.float32)
    x[0].reshape(-1)[:LOGITS.size] = LOGITS
    x[2] = -np.abs(x[2]) - 2.0 ** -19  # all negative, outside the band
    t = (g.random((N, 1, H, W)) < 0.3).astype(np.float32)
    xd, td = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
    counts = torch.zeros(6, dtype=torch.int64, device=DEV)
    mask = torch.empty((N, 1, H, W), dtype=torch.uint8, device=DEV)
    rt.mask_counts(xd, td, counts, mask)
    mk = mask.cpu().numpy().astype(bool)
    _check_mask(mk.reshape(-1), x.reshape(-1))
    labels, cnt = unet_hip.connected_components(xd, kind="logits")
    assert np.array_equal(labels.cpu().numpy() != 0, mk[:, 0])
    oi, _ = rt.surface_stats(xd, td)
    defined = oi[:, 0].cpu().numpy()
    fg = mk.reshape(N, -1).any(1)
    assert fg.tolist() == [True, True, False] and t.reshape(N, -1).any(1).all()
    assert defined.tolist() == [1, 1, 0]
    assert cnt.cpu().numpy()[2] == 0
    assert counts.cpu().tolist() == _want(mk.reshape(-1), t.reshape(-1))
