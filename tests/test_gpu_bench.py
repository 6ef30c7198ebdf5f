"""bench.py end to end on one GPU at a tiny shape: the plain run's result line and
--dump-outputs files, and what --full adds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")
TINY = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2", "--size", "64"]

pytestmark = pytest.mark.gpu


def _bench(args):
    r = subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [s for s in r.stdout.splitlines() if s.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_and_dump_outputs(tmp_path):
    d = _bench(TINY + ["--dump-outputs", str(tmp_path)])
    assert d["steps"] == 3 and d["warmup"] == 1
    assert d["unit"] == "images/sec" and d["higher_is_better"] is True and d["dtype"] == "fp32"
    assert d["ms_per_step"] > 0
    # value and ms_per_step describe the same timed region: 2 images per step
    assert abs(d["value"] - 2 * 1000 / d["ms_per_step"]) <= 0.01 * d["value"]
    for k in ("roofline", "cpu_baseline", "dice_vs_ref"):
        assert k not in d  # those take runs of their own: --full
    want = ["bn_stats.npy", "grad_sample.npy", "logits.npy", "loss.npy", "param_sample.npy",
            "sample_index.npy"]
    assert d["outputs"] == want and sorted(os.listdir(tmp_path)) == want
    a = {n[:-4]: np.load(os.path.join(tmp_path, n)) for n in want}
    assert sum(v.nbytes for v in a.values()) <= 64 * 2 ** 20
    for v in a.values():
        assert v.dtype in (np.float32, np.float64) and np.isfinite(v).all()
    assert a["logits"].shape == (2, 1, 64, 64) and a["loss"].shape == (3,)
    assert abs(a["loss"][0] - (a["loss"][1] + a["loss"][2])) <= 1e-6 * abs(a["loss"][0])
    n = a["sample_index"].size
    assert a["param_sample"].shape == a["grad_sample"].shape == (n,)
    assert (np.diff(a["sample_index"]) >= 0).all() and 0 <= a["sample_index"][0]
    assert a["sample_index"][-1] < 31_042_369 and np.abs(a["grad_sample"]).max() > 0


def test_full_adds_roofline():
    d = _bench(TINY + ["--full", "--no-cpu-baseline"])
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    r = d["roofline"]
    assert r["kernel"] and r["launches"] > 0 and r["achieved"] > 0 and 0 < r["frac"] < 1
    assert d["cpu_baseline"] is None
