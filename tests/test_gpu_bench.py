"""GPU: a plain bench.py run (what every later change is measured with) and
its --dump-outputs: one JSON line with the headline fields, no CPU baseline
without --full, --steps timed steps, and the dumped ensemble of the last
timed step identical from run to run for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, STEPS = 64, 3


def _bench(out):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", "1", "--walkers", str(W), "--dump-outputs", str(out)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, check=True)
    lines = r.stdout.decode().strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_line_and_dump(tmp_path):
    line = _bench(tmp_path / "a")
    assert line["steps"] == STEPS and line["n_gpus"] == 1
    assert line["unit"] == "walker ln_prob evals/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0
    # value = walkers x steps / the timed region, ms_per_step = that region / steps
    assert line["value"] == pytest.approx(W / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert line["cpu_baseline"] is None and "cpu_baseline_oracle" not in line   # --full only
    ndim = line["config"]["ndim"]
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("pos", "lnprob", "naccept")}
    assert sorted(os.listdir(tmp_path / "a")) == ["lnprob.npy", "naccept.npy", "pos.npy"]
    assert a["pos"].shape == (W, ndim) and a["lnprob"].shape == (W,) and a["naccept"].shape == (W,)
    assert all(v.dtype == np.float64 for v in a.values())
    assert np.isfinite(a["pos"]).all() and np.isfinite(a["lnprob"]).all()
    # accepted moves since the starting ball: whole numbers, at most one per step (warmup included)
    assert np.array_equal(a["naccept"], np.round(a["naccept"]))
    assert a["naccept"].min() >= 0 and a["naccept"].max() <= STEPS + 1 and a["naccept"].sum() > 0
    assert line["acceptance_fraction"] == pytest.approx(a["naccept"].mean() / (STEPS + 1))
    # the same arguments: the same inputs, the same ensemble, bit for bit
    _bench(tmp_path / "b")
    for n, v in a.items():
        np.testing.assert_array_equal(np.load(tmp_path / "b" / (n + ".npy")), v)
