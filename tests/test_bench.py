"""bench.py's run modes on a small workload: a plain run carries the headline fields only, --full adds the side measurements,
and --dump-outputs writes the last timed step's arrays - the same ones from both runs (same arguments, same seeded inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--envs", "8", "--bank-mib", "64", "--spinup-steps", "0"]


def _bench(args, timeout):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + args, capture_output=True, text=True,
                         timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_and_full_runs_dump_the_same_step(tmp_path):
    plain = _bench(["--dump-outputs", str(tmp_path / "plain")], 300)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["steps"] == 3
    for k in ("cpu_baseline", "roofline", "pipelined", "dependent", "plugin_path", "preplanned_single_stream"):
        assert k not in plain
    assert plain["sustained"] is None and plain["host_us_per_call"] is None
    full = _bench(["--full", "--cpu-seconds", "1", "--sustain", "0.1", "--dump-outputs", str(tmp_path / "full")], 600)
    for k in ("cpu_baseline", "roofline", "pipelined", "dependent", "plugin_path", "preplanned_single_stream"):
        assert k in full
    assert plain["dumped_outputs"]["arrays"] == full["dumped_outputs"]["arrays"] == ["spectrogram"]
    a, b = np.load(tmp_path / "plain" / "spectrogram.npy"), np.load(tmp_path / "full" / "spectrogram.npy")
    assert a.dtype == np.float32 and a.shape == (8, 65, 26, 2) and np.isfinite(a).all() and a.any()
    assert np.array_equal(a, b)
