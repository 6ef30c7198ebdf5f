"""tests/loss_ref.py (the fp64 NumPy losses and analytic gradients the device loss kernels are
judged against) vs torch autograd in float64 on the same formulas.  No GPU."""
import numpy as np
import pytest
import torch

import loss_ref as L

# the shapes of tests/test_gpu_loss_edges.py (every path of loss_stats_kernel) and its two-phase batches
GPU_SHAPES = [(3, 1, 16, 16), (2, 3, 17, 19), (2, 1, 4, 4099), (2, 1, 128, 128), (5, 1, 128, 128),
              (5, 3, 17, 19)]


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("kind", L.KINDS)
def test_reference_matches_torch_float64(C, kind):
    """Soft and hard targets, saturating logits, all-zero and all-one targets, C in {1, 3},
    every (alpha, beta, gamma) and weight set: the losses and every element of the gradient
    agree with float64 autograd to a few ulp of float64 (1e-12 of the gradient's largest
    element: both sum ~4k float64 terms in different orders)."""
    x, t = L.make_case((4, C, 24, 40), kind, seed=C)
    for abg in L.ABG:
        for w in L.WEIGHTS:
            want_l, want_g = L.torch_losses_and_grad(x, t, w, *abg, dtype=torch.float64)
            got_l = L.losses(x, t, *abg)
            got_g = L.dlogits(x, t, w, *abg)
            assert np.all(np.isfinite(got_l)) and np.all(np.isfinite(got_g))
            assert np.max(np.abs(got_l - want_l)) <= 1e-12, (kind, abg, got_l, want_l)
            e = L.sample_rel_err(got_g, want_g).max()
            assert e <= 1e-12, (kind, abg, w, e)


@pytest.mark.parametrize("shape", GPU_SHAPES)
def test_gpu_cases_have_a_finite_reference(shape):
    """No input of the GPU test makes the reference non-finite (gamma < 1 needs ti < 1), and
    none leaves a sample's gradient identically zero (the relative metric's denominator)."""
    for kind in L.KINDS:
        x, t = L.make_case(shape, kind)
        for abg in L.ABG:
            for w in L.WEIGHTS:
                assert np.all(np.isfinite(L.losses(x, t, *abg)))
                g = L.dlogits(x, t, w, *abg)
                assert np.all(np.isfinite(g))
                assert np.abs(g).reshape(shape[0], -1).max(1).min() > 0


def test_gradient_is_the_derivative():
    """Central differences in float64 on a few elements, the sample boundaries included."""
    x, t = L.make_case((3, 2, 5, 7), "soft", seed=9)
    x = x.astype(np.float64)
    w, abg = L.WEIGHTS[0], L.ABG[1]
    g = L.dlogits(x, t, w, *abg).reshape(-1)
    per = 2 * 5 * 7
    for i in (0, per - 1, per, 2 * per - 1, 2 * per, 3 * per - 1):
        h = 1e-6
        xp, xm = x.reshape(-1).copy(), x.reshape(-1).copy()
        xp[i] += h
        xm[i] -= h
        fd = (np.dot(w, L.losses(xp.reshape(x.shape), t, *abg)) -
              np.dot(w, L.losses(xm.reshape(x.shape), t, *abg))) / (2 * h)
        assert abs(fd - g[i]) <= 1e-8 * max(1.0, np.abs(g).max() / 1e-3), (i, fd, g[i])


def test_sample_statistics_matter():
    """The inputs make a wrong sample index visible: the gradient formed with sample 0's dice
    statistics for every sample is off by far more than any bar of the GPU test."""
    x, t = L.make_case((3, 1, 16, 16), "soft")
    w = L.WEIGHTS[0]
    good = L.dlogits(x, t, w)
    x0 = np.broadcast_to(x[:1], x.shape)
    t0 = np.broadcast_to(t[:1], t.shape)
    # dice term evaluated with sample 0's I and U everywhere (what n = 0 would compute)
    p = L.sigmoid(x.astype(np.float64))
    inter = (L.sigmoid(x0[0].astype(np.float64)) * t0[0]).sum()
    u1 = L.sigmoid(x0[0].astype(np.float64)).sum() + t0[0].sum() + 1.0
    wrong_dice = (-w[1] / 3) * (2.0 * t * u1 - (2.0 * inter + 1.0)) / (u1 * u1) * p * (1 - p)
    right_dice = good - L.dlogits(x, t, (w[0], 0.0, w[2]))
    bad = good - right_dice + wrong_dice
    assert L.sample_rel_err(bad, good)[1:].min() > 1e-2
