"""GPU (-m gpu): a plain `bench.py` run (no --full) times the headline workload and prints its line, nothing else; with
--dump-outputs it writes what the last timed step computed, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8", "--iters", "10",
           "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.rstrip().splitlines()
    assert len([ln for ln in lines if ln.startswith("{")]) == 1 and lines[-1].startswith("{")
    return json.loads(lines[-1])


def test_plain_run_times_the_headline_and_dumps_its_outputs(tmp_path):
    import bench
    d = _plain_run(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True and d["dtype"] == "f32"
    B, T, F, it = d["config"]["batch_per_gpu"], d["config"]["frames"], d["config"]["bins"], d["config"]["iters"]
    assert (B, T, F, it) == (8, 500, 513, 10)
    assert np.isclose(d["value"], B * T * F * it / (d["ms_per_step"] * 1e-3), rtol=1e-5)
    assert d["cpu_baseline"] is None and "extra_file" not in d          # nothing beyond the headline without --full
    got = np.load(tmp_path / "a" / "spectrograms.npy")
    idx = np.load(tmp_path / "a" / "spectrogram_index.npy")
    assert got.dtype == np.float32 and got.shape == (B, T, F, 2) and np.array_equal(idx, np.arange(B))
    assert np.isfinite(got).all()
    mags = bench.synth_magnitudes(B, T, F, 20260928)
    assert np.abs(np.hypot(got[..., 0], got[..., 1]) - mags).max() < 1e-5 * mags.max()   # the state keeps its magnitudes
    assert np.abs(got[..., 1]).max() > 0.1 * mags.max()                                   # ... and the sweeps gave it phases
    d2 = _plain_run(tmp_path / "b")
    assert d2["config"] == d["config"]
    assert np.array_equal(np.load(tmp_path / "b" / "spectrograms.npy"), got)              # same inputs, same outputs
