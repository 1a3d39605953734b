"""`python bench.py --gpus N` must START by itself: with no launcher environment it re-executes under
torch.distributed.run, every rank rendezvouses on 127.0.0.1, the time is the max over the ranks and rank 0 prints ONE JSON line.
Checked here over gloo without a GPU (GENNBV_BENCH_DRY=1 skips the hot path, nothing else)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra_env, *argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(extra_env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, capture_output=True, text=True, timeout=300)


def test_gpus2_self_launches_and_prints_one_json_line():
    r = _run({"GENNBV_BENCH_DRY": "1"}, "--gpus", "2", "--steps", "3", "--warmup", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1
    assert out["max_rank_seconds"] >= 0.02  # rank 1 sleeps 20 ms: the max over the ranks, not rank 0's own time
    assert "torch.distributed.run" in r.stderr  # the launcher line goes to stderr, never in front of the JSON


def test_gpus1_needs_no_launcher():
    r = _run({"GENNBV_BENCH_DRY": "1"}, "--gpus", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["n_gpus"] == 1


def test_without_gpus_the_real_bench_fails_loudly():
    r = _run({}, "--gpus", "1", "--steps", "1", "--warmup", "0")
    assert r.returncode != 0 and "GPU" in (r.stderr + r.stdout)


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample_of_large_ones(tmp_path):
    import types

    import numpy as np
    import torch

    import bench
    n_big = bench.DUMP_SAMPLE + 12345
    buf = types.SimpleNamespace(observations=torch.randn(3, 4, 5), grid_i8=torch.randint(-1, 2, (n_big,), dtype=torch.int8),
                                actions=torch.randn(2, 4, 6), rewards=torch.randn(2, 4, 1),
                                episode_starts=torch.ones(2, 4, 1, dtype=torch.uint8), values=torch.randn(2, 4, 1),
                                log_probs=torch.randn(2, 4, 1), advantages=torch.randn(2, 4, 1), returns=torch.randn(2, 4, 1))
    policy = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.BatchNorm1d(2))
    algo = types.SimpleNamespace(rollout_buffer=buf, policy=policy, last_train_stats=np.arange(12.0).reshape(4, 3))
    info = [bench.dump_outputs(algo, str(tmp_path / d)) for d in ("a", "b")]
    names = sorted(f[:-4] for f in os.listdir(tmp_path / "a"))
    assert info[0]["files"] == len(names) == 9 + 7 + 1 and info[0]["bytes"] <= 64 << 20
    assert "rollout_grid_i8_sample" in names and "policy.1.num_batches_tracked" in names and "train_stats" in names
    for name in names:
        a, b = (np.load(tmp_path / d / (name + ".npy")) for d in ("a", "b"))
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), name
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "rollout_observations.npy"), buf.observations.numpy())
    assert np.load(tmp_path / "a" / "train_stats.npy").dtype == np.float64
    grid = np.load(tmp_path / "a" / "rollout_grid_i8_sample.npy")
    assert grid.shape == (bench.DUMP_SAMPLE,) and set(np.unique(grid)) <= {-1.0, 0.0, 1.0}


def test_full_is_opt_in(monkeypatch):
    """A plain run times the headline only; the checks and extra measurements after the timed steps need --full."""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--full"])
    assert bench.parse().full is True
