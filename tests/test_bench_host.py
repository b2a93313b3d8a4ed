"""Host-side pieces of bench.py (no GPU): the algorithmic-bytes model and the CPU-baseline leg."""
import pytest

import bench


def test_algorithmic_bytes_per_env_step_rollout():
    # f32, K = 5000: 65 B of outputs per env-step plus the per-launch state/scenario/route traffic
    n_env, k = 32768, 5000
    b = bench.algorithmic_bytes_per_launch(n_env, k, 4, 3.0, 5.0, "rollout")
    per = b / (n_env * k)
    assert 65.0 < per < 65.2
    # longer launches amortise the state read/write: bytes per env-step fall towards 65
    b200 = bench.algorithmic_bytes_per_launch(n_env, 200, 4, 3.0, 5.0, "rollout") / (n_env * 200)
    assert b200 > per


def test_cpu_baseline_workers_report():
    r = bench.cpu_baseline(0.5, 25450, 3)     # 2 vectorised workers + the scalar loop, concurrently
    assert r["kind"] == "port" and r["unit"] == "env-steps/s"
    assert r["cores"] == 2 and r["value"] > 0 and r["per_core_value"] > 0
    assert "2 single-threaded processes" in r["sample"]
    sc = r["scalar_1core"]
    assert sc["cores"] == 1 and sc["value"] > 0
    if bench.latest_calibration() is not None:
        assert sc["reference_estimate"] == pytest.approx(sc["value"] * sc["calibration"]["ratio_reference_over_restatement"])


def _run_bench(*argv, env_extra=None, timeout=300):
    import json
    import os
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                             "MASTER_PORT")}
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(bench.__file__), "bench.py"), *argv],
                       capture_output=True, text=True, timeout=timeout, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p.returncode, (json.loads(lines[-1]) if lines else None), p.stderr


def test_bench_gpus_flag_starts_ranks_itself():
    """`bench.py --gpus 2` without torchrun's environment re-launches itself as 2 rank processes
    (torch.distributed.run, 127.0.0.1); rank 0 prints one JSON line with n_gpus = world size = 2
    after the pipelined transition gather moved every rank's records to the learner (gloo here,
    RCCL on the GPU node)."""
    rc, line, err = _run_bench("--gpus", "2", "--dry-run")
    assert rc == 0, err[-2000:]
    assert line["n_gpus"] == 2 and line["world_size"] == 2 and line["dry_run"]
    assert line["records_per_launch_ok"] is True and line["dropped"] == 0
    assert line["gathered"] == sum(3 + i + r for i in range(line["launches"]) for r in range(2))


def test_bench_rejects_gpus_world_size_mismatch():
    rc, line, err = _run_bench("--gpus", "4", "--dry-run", env_extra={"WORLD_SIZE": "2", "RANK": "0",
                                                                       "LOCAL_RANK": "0"})
    assert rc != 0 and line is None
    assert "WORLD_SIZE=2" in err


def test_launch_plan_whole_launches():
    """The timed launches add up to exactly --steps (whole launches, then the remainder); the warm-up
    stays whole launches, at least min_warmup_launches."""
    import argparse
    a = argparse.Namespace(steps=20, warmup=5, min_launches=3, min_warmup_launches=8)
    assert bench.launch_plan(a, 5000) == ([20], 40000)
    a = argparse.Namespace(steps=20001, warmup=45000, min_launches=3, min_warmup_launches=8)
    assert bench.launch_plan(a, 5000) == ([5000] * 4 + [1], 45000)
    a = argparse.Namespace(steps=15000, warmup=45001, min_launches=3, min_warmup_launches=8)
    assert bench.launch_plan(a, 5000) == ([5000] * 3, 50000)
    a = argparse.Namespace(steps=7, warmup=0, min_launches=3, min_warmup_launches=8)
    assert bench.launch_plan(a, 1) == ([1] * 7, 8)          # step mode: one launch per step


def test_dump_outputs_formats(tmp_path):
    """--dump-outputs: reals keep their precision, flags / counts / status words become float64, an
    array above the per-array limit is a fixed sample of its rows, ranks get their own files."""
    import numpy as np
    import torch
    big = torch.arange(3 * (bench.DUMP_ARRAY_BYTES // 8), dtype=torch.float32).reshape(-1, 2)
    arrays = {"next_state": torch.arange(20, dtype=torch.float32).reshape(2, 10), "reward": torch.ones(2, dtype=torch.float64),
              "done": torch.tensor([0, 1], dtype=torch.uint8), "status": torch.tensor([-2 ** 31, 5], dtype=torch.int32),
              "big": big}
    bench.dump_outputs(str(tmp_path / "a"), arrays, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), arrays, 0, 1)
    got = {f: np.load(tmp_path / "a" / f"{f}.npy") for f in arrays}
    assert got["next_state"].dtype == np.float32 and got["reward"].dtype == np.float64
    assert got["done"].dtype == np.float64 and got["done"].tolist() == [0.0, 1.0]
    assert got["status"].dtype == np.float64 and got["status"].tolist() == [-2.0 ** 31, 5.0]
    assert got["big"].nbytes <= bench.DUMP_ARRAY_BYTES and got["big"].shape[1] == 2
    assert np.all(np.diff(got["big"][:, 0]) > 0)                          # rows of `big`, in order
    assert np.array_equal(got["big"], np.load(tmp_path / "b" / "big.npy"))   # the same sample every time
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == sorted(f"{f}.npy" for f in arrays)
    # non-finite entries: 0 in the array, 1 in the mask beside it; ranks get their own files
    act = torch.tensor([[1.0, float("nan")], [float("inf"), 2.0]], dtype=torch.float32)
    bench.dump_outputs(str(tmp_path / "c"), {"action": act}, 1, 2)
    assert np.load(tmp_path / "c" / "action_rank1.npy").tolist() == [[1.0, 0.0], [0.0, 2.0]]
    assert np.load(tmp_path / "c" / "action_nonfinite_rank1.npy").tolist() == [[0.0, 1.0], [1.0, 0.0]]


def test_canonical_transitions_order_free():
    """The dumped transition records do not depend on the order the kernel appended them in."""
    import torch
    g = torch.Generator().manual_seed(3)
    rec = torch.rand(500, 24, generator=g, dtype=torch.float64)
    rec[:, 23] = torch.randint(1000, 1000 + 2 * bench.DUMP_TRANSITION_ENVS, (500,), generator=g).double()
    rec[40:, 23] = rec[:460, 23]                                           # several records per env
    a = bench.canonical_transitions(rec, 480, 1000)
    perm = torch.randperm(480, generator=g)
    b = bench.canonical_transitions(torch.cat([rec[:480][perm], rec[480:]]), 480, 1000)
    assert torch.equal(a, b) and 0 < a.shape[0] < 480
    assert bool((a[:, 23] < 1000 + bench.DUMP_TRANSITION_ENVS).all()) and bool((a[1:, 23] >= a[:-1, 23]).all())
    assert bench.canonical_transitions(rec, 0, 1000).shape == (0, 24)
