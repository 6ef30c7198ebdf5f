"""CPU: everything Trainer.test reports -- the log text, what it prints and the returned dict -- against a
recording, with every device entry replaced by its host twin.  Two configurations switch every metric
block on between them (``threshold`` and ``tta`` exclude each other):

* (A) tta="d4", surface_metrics, pp_largest + pp_min_area=8 + pp_fill_holes, lesion_metrics, lesion_shape
* (B) curve_metrics, curve_bins=64, threshold="val-dice", surface_metrics

Two batches of 3 and 2 samples from the scene generators of curve_ref and surface_ref: (B) at 32 x 48;
(A) at 48 x 48, because the quarter-turn views of "d4" are refused on a plane that is not square.  One
sample's target is empty: the surface blocks count it as undefined and the lesion block finds no
component in it.

The recordings (tests/golden/trainer_test_report_{a,b}.txt) were taken by running this test on the
Trainer.test that wrote every block out inline; every float in a message is printed at .4f or .6f and
the host twins are deterministic.  Should a value ever sit on a rounding boundary, change the seed, not
the comparison."""
import io
import logging
import os
import types

import numpy as np
import pytest
import torch

import curve_ref as R
import surface_ref as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class _StubRuntime:
    """unet_mask_counts restated in torch for the CPU (away from logits in (0, 2^-24])."""

    def mask_counts(self, logits, targets, counts, mask=None):
        pr = logits > 0
        tu = targets.to(torch.int64)
        if mask is not None:
            mask.copy_(pr)
        counts += torch.stack([(pr & (tu == 1)).sum(), (pr & (tu == 0)).sum(), (~pr & (tu == 1)).sum(),
                               (~pr & (tu == 0)).sum(), (pr & (targets != 0)).sum(),
                               (pr | (targets != 0)).sum()])


class _StubModel:
    """The "image" is the logit plane, plus a ramp along the columns: the stub is not equivariant under
    the flips and turns, so the views of the test-time augmentation disagree near the rim."""

    def eval(self):
        return self

    def __call__(self, images):
        w = images.shape[-1]
        return images + torch.linspace(-1.5, 1.5, w, dtype=torch.float32)


def _cpu_trainer(tmp_path, logger, test_batches, val_batches, **cfg):
    from utils.trainer import Trainer
    tr = object.__new__(Trainer)
    tr.config = types.SimpleNamespace(result_dir=str(tmp_path), **cfg)
    tr.logger = logger
    tr.rank0, tr.ddp, tr.device = True, None, torch.device("cpu")
    tr.model, tr.rt = _StubModel(), _StubRuntime()
    tr.test_loader, tr.val_loader = test_batches, val_batches
    tr._plot_contours = lambda keep: None
    return tr


def _loader(seed, h, w, bias=0.0):
    """Batches of 3 and 2 samples.  Sample 1 predicts a ring (a hole to fill) with an island beside it,
    sample 3 has an empty target."""
    r = np.random.default_rng(seed)
    out = []
    for n in (3, 2):
        x, t = R._scene(r, n, h, w)
        x = (x + np.float32(bias)).reshape(n, 1, h, w)
        t = t.reshape(n, 1, h, w)
        x[np.abs(x) < 1e-3] = 0.0
        out.append((x, t))
    ring = S.ellipse(h, w, h * 0.5, w * 0.45, h * 0.3, w * 0.3) & ~S.ellipse(h, w, h * 0.5, w * 0.45, h * 0.12, w * 0.12)
    ring[2:4, w - 5:w - 2] = True
    out[0][0][1, 0] = np.where(ring, 4.0, -6.0) + r.normal(0, 0.5, ring.shape)
    out[1][1][0] = 0.0
    return [(torch.from_numpy(x), torch.from_numpy(t)) for x, t in out]


@pytest.fixture
def host_ops(monkeypatch):
    """Every device entry Trainer.test reaches, replaced by the library's host twin.  tta_predict has
    none of its own: it runs as it is over the twins of its two device calls."""
    import unet_hip
    for name in ("surface_metrics", "postprocess_mask", "lesion_metrics", "lesion_morphometry", "curve_hist",
                 "curve_stats"):
        monkeypatch.setattr(unet_hip, name, getattr(unet_hip, name + "_host"))
    monkeypatch.setattr(unet_hip.functional, "tta_views", unet_hip.tta_views_host)
    monkeypatch.setattr(unet_hip.functional, "tta_merge", unet_hip.tta_merge_host)


CONFIGS = {
    "a": dict(size=(48, 48), cfg=dict(tta="d4", surface_metrics=True, pp_largest=True, pp_min_area=8,
                                      pp_fill_holes=True, lesion_metrics=True, lesion_shape=True)),
    "b": dict(size=(32, 48), cfg=dict(curve_metrics=True, curve_bins=64, threshold="val-dice",
                                      surface_metrics=True)),
}


def report(name, tmp_path, capsys):
    """Run Trainer.test in configuration `name`; the log, the printed text and the dict as one text."""
    h, w = CONFIGS[name]["size"]
    test, val = _loader(11, h, w, -2.0), _loader(12, h, w, -2.0)
    logger = logging.getLogger("trainer_report_cpu_" + name)
    logger.setLevel(logging.INFO)
    logger.propagate = False
    log = io.StringIO()
    handler = logging.StreamHandler(log)
    handler.setFormatter(logging.Formatter("%(levelname)s %(message)s"))
    logger.addHandler(handler)
    capsys.readouterr()
    try:
        m = _cpu_trainer(tmp_path, logger, test, val, **CONFIGS[name]["cfg"]).test()
    finally:
        logger.removeHandler(handler)
    out = capsys.readouterr().out
    items = "".join(f"{k!r}: {v!r}\n" for k, v in m.items())
    return f"==== log ====\n{log.getvalue()}==== stdout ====\n{out}==== dict ====\n{items}"


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_trainer_test_report_is_the_recording(name, tmp_path, host_ops, capsys):
    got = report(name, tmp_path, capsys)
    with open(os.path.join(GOLDEN, f"trainer_test_report_{name}.txt"), encoding="utf-8") as f:
        want = f.read()
    assert got == want
