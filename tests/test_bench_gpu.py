"""bench.py's plain run: the headline only (side legs need --full), and --dump-outputs
writes what the last timed step computed, the same values from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE_LEGS = ("variational", "variational_cfg3", "backward", "posterior", "cfg2", "exact_large",
             "strong_share", "fp32_update", "e2e_step", "cpu_baseline", "elbo_rel_err_vs_fp64_oracle")


def _run(out_dir, steps):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--B", "64", "--N", "128", "--dump-outputs", str(out_dir)],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_plain_run_is_headline_only_and_dumps_its_outputs(tmp_path):
    line, a = _run(tmp_path / "a", 3)
    _, b = _run(tmp_path / "b", 2)
    assert not [k for k in SIDE_LEGS if k in line]
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "windows/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert set(a) == {"mll", "info", "L", "L_windows"} == set(b)
    assert all(v.dtype == np.float32 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["mll"].shape == (64,) and a["info"].shape == (64,) and a["L"].shape == (64, 128, 128)
    assert (a["info"] == 0).all() and np.isfinite(a["L"]).all()
    assert (np.triu(a["L"], 1) == 0).all() and (np.diagonal(a["L"], axis1=1, axis2=2) > 0).all()
    assert abs(a["mll"].astype(np.float64).mean() - line["mean_mll"]) <= 1e-6 * abs(line["mean_mll"])
    for k in a:   # seeded inputs, deterministic kernel: the step count does not change the outputs
        assert np.array_equal(a[k], b[k]), k
