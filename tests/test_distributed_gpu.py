"""Data-parallel ENGINE step without an 8-GPU node: two ranks share the one GPU of the test box
(gloo carries the exchange) and each runs the engine on its shard; the result must equal the single-process step on the
whole batch.  Group norm: no cross-sample statistics, so the data-parallel step is exactly the big-batch step
(reference phiseg_model.py:221,236: the losses are means over the global batch)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _launch(nproc, out_dir, case, dtype, steps, port, extra_env=None):
    env = dict(os.environ, PHX_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT, **(extra_env or {}))
    env.pop("RANK", None); env.pop("WORLD_SIZE", None)
    if nproc == 1:
        cmd = [sys.executable, os.path.join(ROOT, "tests", "dp_worker.py"), out_dir, case, dtype, str(steps)]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr",
               "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "dp_worker.py"), out_dir, case, dtype, str(steps)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("mode", ["atomics", "deterministic"])
def test_two_rank_engine_step_equals_single_process_big_batch(tmp_path, mode):
    """mode "deterministic" (PHX_DETERMINISTIC=1: ordered reductions, no atomics) holds the tight 2e-3 gradient bound; the default
    mode's bound absorbs the run-to-run order of its atomic accumulations (advisor finding, round 3)."""
    import json
    case = "tiny_phiseg_gn4"
    xenv = {"PHX_DETERMINISTIC": "1"} if mode == "deterministic" else None
    d2, d1 = tmp_path / "dp2", tmp_path / "single"
    d2.mkdir(); d1.mkdir()
    _launch(2, str(d2), case, "f32", 2, 29541 if xenv is None else 29547, xenv)
    # the single-process reference: the same worker with a fixture whose batch is twice as large
    g = np.load(os.path.join(ROOT, "tests", "golden", case + ".npz"))
    cfg = json.loads(str(g["meta/cfg_json"]))
    big = tmp_path / "golden_big"
    big.mkdir()
    cfg2 = dict(cfg, B=2 * cfg["B"])
    np.savez(str(big / (case + "_x2.npz")), **{k: (np.array(json.dumps(cfg2)) if k == "meta/cfg_json" else g[k]) for k in g.files})
    env_golden = os.environ.get("PHX_TEST_GOLDEN_DIR")
    os.environ["PHX_TEST_GOLDEN_DIR"] = str(big)
    try:
        _launch(1, str(d1), case + "_x2", "f32", 2, 0, xenv)
    finally:
        if env_golden is None:
            os.environ.pop("PHX_TEST_GOLDEN_DIR", None)
        else:
            os.environ["PHX_TEST_GOLDEN_DIR"] = env_golden
    r0, r1, ref = np.load(str(d2 / "rank0.npz")), np.load(str(d2 / "rank1.npz")), np.load(str(d1 / "rank0.npz"))
    # every rank reports the GLOBAL-batch loss terms, equal to the big-batch step's
    np.testing.assert_allclose(r0["losses"], ref["losses"], rtol=2e-5)
    np.testing.assert_allclose(r1["losses"], ref["losses"], rtol=2e-5)
    assert int(r0["n_live"]) < int(r0["n_train"])            # never-consumed branches are not reduced
    n = 0
    for k in ref.files:
        if k.startswith("grad/") or k.startswith("param/"):
            # fp32 summation order differs between 2 + 2 and 4 samples (conditioning bound of the gradients: 3e-2, see
            # test_model_gpu.GRAD_RTOL); Adam moves a weight by ~lr = 1e-5 per step whatever the gradient's size
            # (atomic accumulation order varies run to run: 3.2e-3 of a tensor's largest entry seen once in eight runs of this test,
            # always in the first run on a cold device -- 1e-2 stays 3x under the conditioning bound)
            gtol = 2e-3 if mode == "deterministic" else 1e-2
            tol = gtol * max(np.abs(ref[k]).max(), 1e-6) if k.startswith("grad/") else 5e-5
            np.testing.assert_allclose(r0[k], ref[k], rtol=0, atol=tol, err_msg=k)
            np.testing.assert_allclose(r1[k], r0[k], rtol=0, atol=0, err_msg=k + " (replicas diverged)")
            n += 1
    assert n > 500


def _big_batch_fixture(tmp_path, case):
    import json
    g = np.load(os.path.join(ROOT, "tests", "golden", case + ".npz"))
    cfg = json.loads(str(g["meta/cfg_json"]))
    big = tmp_path / "golden_big"
    big.mkdir(exist_ok=True)
    np.savez(str(big / (case + "_x2.npz")), **{k: (np.array(json.dumps(dict(cfg, B=2 * cfg["B"]))) if k == "meta/cfg_json" else g[k])
                                              for k in g.files})
    return str(big)


def test_two_rank_weight_decay_share(tmp_path):
    """The weight-decay term (phiseg_model.py:126-128, 290-299) under data parallelism: every rank evaluates it on the full parameter
    set and the scalar fetches / the gradient arena are summed over the ranks, so each rank must carry a 1 / world share -- the
    reported term, the total loss and the parameters after one Adam step equal the single-process step on the doubled batch."""
    case = "tiny_phiseg_gn4"
    d2, d1 = tmp_path / "dp2", tmp_path / "single"
    d2.mkdir(); d1.mkdir()
    wd = {"PHX_TEST_WD": "0.37"}
    _launch(2, str(d2), case, "f32", 1, 29543, wd)
    _launch(1, str(d1), case + "_x2", "f32", 1, 0, dict(wd, PHX_TEST_GOLDEN_DIR=_big_batch_fixture(tmp_path, case)))
    r0, r1, ref = np.load(str(d2 / "rank0.npz")), np.load(str(d2 / "rank1.npz")), np.load(str(d1 / "rank0.npz"))
    keys = [str(k) for k in ref["keys"]]
    assert "weight_decay" in keys
    np.testing.assert_allclose(r0["losses"], ref["losses"], rtol=2e-5)
    np.testing.assert_allclose(r1["losses"], ref["losses"], rtol=2e-5)
    assert ref["losses"][0][keys.index("weight_decay")] > 1.0          # (a real contribution, not a rounding-level term)
    for k in ref.files:
        if k.startswith("grad/"):        # (conv biases in front of a group norm: +-2e3 values that cancel -> 3e-3 from the summation order)
            np.testing.assert_allclose(r0[k], ref[k], rtol=0, atol=1e-2 * max(np.abs(ref[k]).max(), 1e-6), err_msg=k)   # (run-to-run atomics order: see above)
            if k.endswith("/W"):         # the decay term's own contribution: a doubled (un-shared) term would be off by 0.37 * W
                w = ref["param/" + k[5:]]
                assert np.abs(r0[k] - ref[k]).max() <= 0.05 * 0.37 * np.abs(w).max() + 6e-3 * np.abs(ref[k]).max(), k
        elif k.startswith("param/"):
            np.testing.assert_allclose(r0[k], ref[k], rtol=0, atol=5e-5, err_msg=k)
            np.testing.assert_allclose(r1[k], r0[k], rtol=0, atol=0, err_msg=k + " (replicas diverged)")


def test_two_rank_train_through_validations(tmp_path):
    """model.train(data, log_dir) on two ranks, validating at every step (4 validations): the ranks score different images with
    different annotators and noise, so their best-of comparisons differ from the second validation on -- rank 0's decisions are
    broadcast and the replica statistics are averaged once per validation, so no rank waits in a collective the other one skips
    (it used to: save_weights averaged the batch-norm statistics inside the per-rank `if better:`).  Also: checkpoint pruning
    (Saver(max_to_keep=1) for model.ckpt, 2 per best-of saver, phiseg_model.py:144-148)."""
    d2 = tmp_path / "dp2"
    d2.mkdir()
    log_dir = tmp_path / "run"
    _launch(2, str(d2), "tiny_phiseg_bn", "f32", 0, 29545, {"PHX_TEST_TRAIN_DIR": str(log_dir)})
    r0, r1 = np.load(str(d2 / "rank0.npz")), np.load(str(d2 / "rank1.npz"))
    assert len(r0["losses"]) == 4 and np.all(np.isfinite(r0["losses"])) and np.all(np.isfinite(r1["losses"]))
    np.testing.assert_allclose(r0["losses"], r1["losses"], rtol=1e-6)   # (Session.run reports the global-batch loss on every rank)
    files = sorted(os.listdir(str(log_dir)))
    latest = [f for f in files if f.startswith("model.ckpt-")]
    assert latest == ["model.ckpt-3.npz"], files                         # max_to_keep = 1
    for crit in ("dice", "loss", "ged", "ncc"):
        n = [f for f in files if f.startswith("model_best_%s.ckpt-" % crit)]
        assert 1 <= len(n) <= 2, files                                   # max_to_keep = 2


def _n_devices():
    import torch
    return torch.cuda.device_count() if torch.cuda.is_available() else 0


@pytest.mark.skipif(_n_devices() < 2, reason="the native RCCL exchange needs two devices (RCCL refuses duplicate devices)")
def test_native_rccl_allreduce_two_devices(tmp_path):
    """phx_comm_allreduce_sum_f32 with world = 2 on two GPUs -- the path `bench.py --gpus N` and data-parallel training take
    (distributed.DistContext._native: rendezvous id over torch.distributed, ncclCommInitRank, bucketed in-place all-reduce on the
    plan's HIP stream) -- against the single-process sum.  The 1-GPU test box skips it; tests/dp_worker.py covers the engine's
    data-parallel step there through gloo."""
    n = 3_000_001                                         # several 64 K buckets and a ragged tail
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT)
    env.pop("RANK", None); env.pop("WORLD_SIZE", None); env.pop("PHX_DIST_BACKEND", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29547", os.path.join(ROOT, "tests", "rccl_worker.py"), str(tmp_path), str(n)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    a0 = np.random.default_rng(100).standard_normal(n).astype(np.float32)
    a1 = np.random.default_rng(101).standard_normal(n).astype(np.float32)
    ref = 2.0 * (a0 + a1)                                 # two all-reduces: x -> x0 + x1 -> 2 (x0 + x1)
    for rk in (0, 1):
        np.testing.assert_allclose(np.load(str(tmp_path / ("rank%d.npy" % rk))), ref, rtol=1e-6, atol=1e-6)


def _bench_two_ranks(tmp_path, *flags):
    """`python bench.py --gpus 2 --batch 4 <flags>` from a plain shell (gloo: both ranks on the test box's one GPU) -> the one line."""
    import json
    env = dict(os.environ, PHX_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "2", "--batch", "4"] + list(flags)
    r = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 8 and out["config"]["parallelism"] == "dp2"
    assert out["config"]["comm"]["path"] == "torch_gloo_host_staged" and out["config"]["comm"]["ranks_seen"] == 2
    assert out["value"] > 0 and out["ms_per_step"] > 0 and np.isfinite(out["config"]["final_loss"])
    return out


def test_bench_self_launches_its_ranks(tmp_path):
    """`python bench.py --gpus 2` from a plain shell (no WORLD_SIZE): bench.py runs itself under torch.distributed.run as a child with
    two ranks (here both on the test box's one GPU, gloo carrying the exchange), rank 0 prints the one JSON line, and the line says
    which transport the timed gradient exchange took and how many ranks took part (config.comm); with --full also the exchange's
    duration."""
    comm = _bench_two_ranks(tmp_path, "--full", "--no-cpu-baseline", "--no-roofline", "--no-other-workloads")["config"]["comm"]
    # the line diagnoses a multi-GPU run by itself: the exchange's duration (HIP events around it on the plan's stream) and every rank's own step time
    assert comm["allreduce_ms_median_rank0"] > 0 and comm["allreduce_ms_max_over_ranks"] >= comm["allreduce_ms_median_rank0"] * 0.999
    assert len(comm["ms_per_step_per_rank"]) == 2 and all(v > 0 for v in comm["ms_per_step_per_rank"]) and comm["allreduce_mbytes"] > 1


def test_bench_plain_two_rank_line_and_dump(tmp_path):
    """The plain data-parallel line (no --full: no exchange diagnostics) and --dump-outputs with two ranks: every rank replays the
    step from the seeded state (it includes the gradient exchange), rank 0 writes the loss and the updated model."""
    out = _bench_two_ranks(tmp_path, "--dump-outputs", str(tmp_path / "dump"))
    assert "allreduce_ms_median_rank0" not in out["config"]["comm"] and "roofline" not in out
    files = sorted(os.listdir(str(tmp_path / "dump")))
    assert files == ["loss_tot.npy", "params.npy", "state.npy"], files
    assert all(np.all(np.isfinite(np.load(str(tmp_path / "dump" / f)))) for f in files)
