"""fp64 NumPy restatement of models/loss.py with analytic gradients (helper of the tests, not a
test), the torch restatement of the same formulas in a chosen dtype (float64 to check this file,
float32 as the yardstick of the device kernels), and the inputs the loss-edge tests share.

* BCE: ``nn.BCEWithLogitsLoss()`` mean over every element (utils/trainer.py:37),
  elem = max(x, 0) - x t + log1p(exp(-|x|)).
* Dice (models/loss.py:13-24): per sample over all classes, smooth 1,
  dice_n = (2 I_n + 1) / (Sp_n + St_n + 1), loss = 1 - mean_n dice_n.
* FocalTversky (models/loss.py:26-46): TP / FP / FN over the whole batch, smooth 1e-6,
  ti = (TP + s) / (TP + a FP + b FN + s), loss = (1 - ti)^gamma.
"""
import numpy as np
import torch

ABG = [(0.4, 0.6, 2.0), (0.7, 0.3, 0.75), (0.5, 0.5, 1.0), (0.3, 0.7, 3.0)]
# (bce, dice, focal) weights: all three, the wf == 0 branch of loss_bwd_kernel, no dice
WEIGHTS = [(0.7, 1.3, 0.5), (1.0, 1.0, 0.0), (0.6, 0.0, 1.1)]
SAT_LOGITS = [100.0, -100.0, 88.0, -88.0, 20.0, -20.0, 0.0, 1e-6, -1e-6]
KINDS = ["soft", "saturated", "all_zero", "all_one"]


def sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def losses(x, t, alpha=0.4, beta=0.6, gamma=2.0):
    """(bce, dice, focal) of logits x and targets t, both (N, C, H, W), in float64."""
    x = np.asarray(x, np.float64)
    t = np.asarray(t, np.float64)
    N = x.shape[0]
    p = sigmoid(x)
    bce = np.mean(np.maximum(x, 0.0) - x * t + np.log1p(np.exp(-np.abs(x))))
    pf, tf = p.reshape(N, -1), t.reshape(N, -1)
    inter = (pf * tf).sum(1)
    union = pf.sum(1) + tf.sum(1)
    dice = 1.0 - np.mean((2.0 * inter + 1.0) / (union + 1.0))
    TP = (p * t).sum()
    FP = (p * (1.0 - t)).sum()
    FN = ((1.0 - p) * t).sum()
    ti = (TP + 1e-6) / (TP + alpha * FP + beta * FN + 1e-6)
    return np.array([bce, dice, (1.0 - ti) ** gamma])


def dlogits(x, t, w, alpha=0.4, beta=0.6, gamma=2.0):
    """d(w[0] bce + w[1] dice + w[2] focal) / dx in float64, analytic."""
    x = np.asarray(x, np.float64)
    t = np.asarray(t, np.float64)
    N = x.shape[0]
    p = sigmoid(x)
    g = w[0] * (p - t) / x.size
    pf, tf = p.reshape(N, -1), t.reshape(N, -1)
    inter = (pf * tf).sum(1)[:, None]
    u1 = (pf.sum(1) + tf.sum(1))[:, None] + 1.0
    ddice = (2.0 * tf * u1 - (2.0 * inter + 1.0)) / (u1 * u1)  # d dice_n / d p
    gp = (-w[1] / N) * ddice.reshape(x.shape)
    if w[2] != 0:
        TP = (p * t).sum()
        FP = (p * (1.0 - t)).sum()
        FN = ((1.0 - p) * t).sum()
        A = TP + 1e-6
        B = TP + alpha * FP + beta * FN + 1e-6
        ti = A / B
        dL = -gamma * (1.0 - ti) ** (gamma - 1.0)
        dti = (t * B - A * (t + alpha * (1.0 - t) - beta * t)) / (B * B)
        gp = gp + w[2] * dL * dti
    return g + gp * p * (1.0 - p)


def torch_losses_and_grad(x, t, w, alpha, beta, gamma, dtype):
    """The same formulas through torch CPU ops and autograd in `dtype`:
    (losses (3,), dlogits) as float64 NumPy arrays."""
    xr = torch.as_tensor(np.asarray(x)).to(dtype).clone().requires_grad_(True)
    tt = torch.as_tensor(np.asarray(t)).to(dtype)
    N = xr.shape[0]
    pr = torch.sigmoid(xr)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(xr, tt)
    pf, tf = pr.reshape(N, -1), tt.reshape(N, -1)
    dice = 1 - ((2 * (pf * tf).sum(1) + 1) / (pf.sum(1) + tf.sum(1) + 1)).mean()
    TP = (pr * tt).sum()
    FP = (pr * (1 - tt)).sum()
    FN = ((1 - pr) * tt).sum()
    ti = (TP + 1e-6) / (TP + alpha * FP + beta * FN + 1e-6)
    focal = (1 - ti) ** gamma
    loss = w[0] * bce + w[1] * dice
    if w[2] != 0:  # (the device skips the focal term's scalars for a zero weight too)
        loss = loss + w[2] * focal
    loss.backward()
    return (torch.stack([bce, dice, focal]).detach().double().numpy(),
            xr.grad.detach().double().numpy())


def make_case(shape, kind, seed=0):
    """float32 (logits, targets) of one input kind.  The samples' foreground fractions differ
    widely (2 % .. 90 %), so the per-sample dice statistics do: a gradient formed with another
    sample's statistics is wrong at first order."""
    g = np.random.default_rng(1000 * seed + sum(shape) + 7 * KINDS.index(kind))
    N = shape[0]
    frac = np.linspace(0.02, 0.9, N).reshape(N, 1, 1, 1) if N > 1 else np.full((1, 1, 1, 1), 0.3)
    if kind == "soft":
        x = g.standard_normal(shape) * 4
        t = np.clip(g.random(shape) * 2 * frac, 0.0, 1.0)
    elif kind == "saturated":
        x = g.choice(np.array(SAT_LOGITS), size=shape)
        t = (g.random(shape) < frac).astype(np.float64)
    elif kind == "all_zero":
        x = g.standard_normal(shape) * 4
        t = np.zeros(shape)
    elif kind == "all_one":
        x = g.standard_normal(shape) * 4
        t = np.ones(shape)
    else:
        raise ValueError(kind)
    return x.astype(np.float32), t.astype(np.float32)


def sample_rel_err(a, ref):
    """max |a - ref| / max |ref| of every sample: (N,)."""
    N = ref.shape[0]
    d = np.abs(np.asarray(a, np.float64) - ref).reshape(N, -1).max(1)
    return d / np.maximum(np.abs(ref).reshape(N, -1).max(1), 1e-300)
