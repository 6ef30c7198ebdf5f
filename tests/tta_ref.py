"""NumPy definition of the test-time-augmentation views and merge (csrc/tta.h restated without
it), the case table and the inputs shared by test_tta_cpu.py and test_gpu_tta.py.

View k in 0..7: h = k & 1, v = k >> 1 & 1, t = k >> 2 & 1 and
    T_k(x): y = x;  if t: y = y.swapaxes(-1, -2);  if v: y = y[..., ::-1, :];  if h: y = y[..., ::-1]
The inverse undoes h, then v, then t.  A set is a bit mask, its views taken in ascending k, the
stack view-major.  Sums are float32, sequential in ascending view order, via np.float32
arithmetic (NumPy rounds every float32 operation on its own)."""
import functools

import numpy as np

SETS = {"hflip": 0x03, "flips": 0x0F, "d4": 0xFF}
U = 2.0 ** -24  # unit roundoff of float32


def numbers(mask):
    return [k for k in range(8) if mask >> k & 1]


def view(x, k):
    y = x
    if k & 4:
        y = y.swapaxes(-1, -2)
    if k & 2:
        y = y[..., ::-1, :]
    if k & 1:
        y = y[..., ::-1]
    return np.ascontiguousarray(y)


def unview(y, k):
    x = y
    if k & 1:
        x = x[..., ::-1]
    if k & 2:
        x = x[..., ::-1, :]
    if k & 4:
        x = x.swapaxes(-1, -2)
    return np.ascontiguousarray(x)


def views(x, mask):
    """(K N, C, H, W), view-major."""
    return np.concatenate([view(x, k) for k in numbers(mask)])


def unwarped(logits, n, mask):
    """[x_0, ..., x_{K-1}], each (n, C, H, W): the per-view logits in the frame of the input."""
    return [unview(logits[q * n:(q + 1) * n], k) for q, k in enumerate(numbers(mask))]


def surf_pred(x):
    """sigmoid(x) > 0.5 in float32, the mask readout of Trainer.test (csrc/surf.h)."""
    x = x.astype(np.float32)
    with np.errstate(over="ignore"):
        return np.float32(1) / (np.float32(1) + np.exp(-x)) > np.float32(0.5)


def votes(logits, n, mask):
    return sum(surf_pred(x).astype(np.uint8) for x in unwarped(logits, n, mask))


def merge_logit(logits, n, mask):
    """mode 0: (score float32, mask uint8, votes uint8)."""
    xs = unwarped(logits.astype(np.float32), n, mask)
    s = xs[0]
    for x in xs[1:]:
        s = (s + x).astype(np.float32)
    score = (s / np.float32(len(xs))).astype(np.float32)
    return score, surf_pred(score).astype(np.uint8), votes(logits, n, mask)


def merge_prob64(logits, n, mask):
    """mode 1 in float64: the mean over the views of 1 / (1 + exp(-x_q))."""
    xs = unwarped(logits.astype(np.float64), n, mask)
    return sum(1.0 / (1.0 + np.exp(-x)) for x in xs) / len(xs)


def prob_bound(K):
    """|float32 mode-1 score - merge_prob64| <= prob_bound(K); derived in test_tta_cpu.py."""
    return (5.0 + (K + 1) / 2.0) * U * 1.01


# ---- cases: (shape, view mask) ----
DIRECT_SHAPES = [(2, 2, 3, 5), (1, 2, 130, 67)]          # H != W: views 0..3 only
SQUARE_SHAPES = [(1, 1, 1, 1), (2, 2, 70, 70), (1, 1, 64, 64)]  # all eight views
BIG = ((2, 1, 512, 512), 0xFF)                            # GPU only


def cases():
    out = []
    for s in DIRECT_SHAPES:
        out += [(s, 1 << k) for k in range(4)] + [(s, SETS["hflip"]), (s, SETS["flips"])]
    for s in SQUARE_SHAPES:
        out += [(s, 1 << k) for k in range(8)] + [(s, m) for m in SETS.values()]
    return out


def case_id(c):
    (n, ch, h, w), m = c
    return f"{n}x{ch}x{h}x{w}-0x{m:02x}"


def ramp(shape, planes_k=1):
    """arange-like float32 content of (planes_k * N, C, H, W): element i is (i - c) / 64 with
    c = floor(0.4 n) + 1/16.  No two elements are equal, no view is a symmetry of it, every
    value is exact in float32 and neither a value nor a sum of K <= 8 of them is zero (K / 16 is
    no integer), so masks and votes do not hang on the last bit of an exp."""
    n = planes_k * int(np.prod(shape))
    assert 16 * n < 2 ** 24
    c = np.floor(0.4 * n) + 1.0 / 16
    x = ((np.arange(n, dtype=np.float64) - c) / 64).astype(np.float32)
    return x.reshape((planes_k * shape[0],) + tuple(shape[1:]))


def short_random(shape, seed):
    """Random float32 with 16 significant bits (integers in [-2^15, 2^15) / 256): a sum of up to
    8 equal values and its division by 8 are exact, so a round trip is bit-exact."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-2 ** 15, 2 ** 15, size=shape).astype(np.float32) / np.float32(256))


# seeds of the N(0, 3^2) logits of the mode-1 tests, chosen so that no float64 mean probability
# lies within prob_bound(K) of 0.5 (prob_inputs asserts it): no pixel is ever excluded
PROB_SEEDS = {((2, 2, 70, 70), 0x0F): 1016, ((2, 2, 70, 70), 0xFF): 1256}  # others: 1000 + mask


@functools.lru_cache(maxsize=None)
def prob_inputs(shape, mask):
    """(logits float32 (K N, C, H, W), float64 reference score, reference mask uint8); shared,
    read-only."""
    K = len(numbers(mask))
    seed = PROB_SEEDS.get((shape, mask), 1000 + mask)
    rng = np.random.default_rng(seed)
    logits = (3.0 * rng.standard_normal((K * shape[0],) + tuple(shape[1:]))).astype(np.float32)
    ref = merge_prob64(logits, shape[0], mask)
    margin = np.abs(ref - 0.5).min()
    assert margin > prob_bound(K), (shape, mask, seed, margin, prob_bound(K))
    for a in (logits, ref):
        a.setflags(write=False)
    ref_mask = (ref > 0.5).astype(np.uint8)
    ref_mask.setflags(write=False)
    return logits, ref, ref_mask
