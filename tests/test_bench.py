"""bench.py's plain run and --dump-outputs: the plain line carries the headline figure and nothing that takes runs of its own
(those are --full), and the dumped outputs of two runs with the same arguments can be compared element for element."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_samples_large_arrays_at_fixed_indices_and_caps_the_total(tmp_path):
    n = bench.DUMP_SAMPLE + 5
    arrays = {"big": np.arange(n, dtype=np.float64), "small": np.ones((2, 3), dtype=np.float16), "loss": np.float32(1.5)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    got = {k: np.load(str(tmp_path / "a" / (k + ".npy"))) for k in arrays}
    assert got["big"].dtype == np.float64 and got["big"].shape == (bench.DUMP_SAMPLE,)
    assert np.all(np.diff(got["big"]) > 0) and got["big"][0] >= 0 and got["big"][-1] < n      # distinct elements, in index order
    assert got["small"].dtype == np.float32 and got["small"].shape == (2, 3) and float(got["loss"]) == 1.5
    for k in arrays:
        assert np.array_equal(got[k], np.load(str(tmp_path / "b" / (k + ".npy"))))
    too_much = {k: np.zeros(bench.DUMP_SAMPLE, dtype=np.float32) for k in ("x", "y", "z")}
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path / "c"), too_much)
    assert not (tmp_path / "c").exists()                     # checked before anything is written


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs_repeat(tmp_path):
    """Two plain runs with the same arguments dump bit-identical outputs in the deterministic mode (PHX_DETERMINISTIC=1: fixed
    summation orders; the default mode's atomics agree up to rounding only): the same seeded inputs, initial weights and noise,
    and the dumped step starts from the seeded state again, whatever the timed steps did to it."""
    env = dict(os.environ, PYTHONPATH=ROOT, PHX_DETERMINISTIC="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    runs = []
    for name in ("a", "b"):
        d = tmp_path / name
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "4",
               "--dump-outputs", str(d)]
        r = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        out = json.loads(lines[0])
        assert out["steps"] == 3 and out["warmup"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0
        assert out["unit"] == "images/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
        assert not {"roofline", "cpu_baseline", "train_api_images_per_s"} & set(out) and "other_workloads" not in out["config"]
        files = sorted(os.listdir(str(d)))
        assert files == ["loss_tot.npy", "params.npy", "state.npy"], files
        arrs = {f: np.load(str(d / f)) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
        assert sum(a.nbytes for a in arrs.values()) <= bench.DUMP_MAX_BYTES
        assert np.isfinite(float(arrs["loss_tot.npy"])) and float(arrs["loss_tot.npy"]) > 0
        assert np.all(np.isfinite(arrs["params.npy"])) and np.all(np.isfinite(arrs["state.npy"]))
        runs.append(arrs)
    for f in runs[0]:
        assert np.array_equal(runs[0][f], runs[1][f]), f
