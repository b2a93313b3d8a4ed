"""A plain ``bench.py`` run on cuda:0 at a small size: --steps sets the timed steps exactly (whole
launches and a shorter last one), the result line holds the headline alone, and --dump-outputs writes
what the last timed step returned — checked bit for bit against the same launch sequence driven
directly through ``VecMultiShipRLEnv.rollout`` in this process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sit = pytest.importorskip("sac_maritime_ast_amd")
from sac_maritime_ast_amd import VecMultiShipRLEnv, make_scenario  # noqa: E402

import bench  # noqa: E402

N_ENV, CHUNK, STEPS, WARM, SEED = 512, 50, 120, 100, 25450     # launches: 2 warm-up, then 50 + 50 + 20 timed


def test_plain_run_times_exactly_steps_and_dumps_last_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, bench.__file__, "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARM),
                        "--n-env", str(N_ENV), "--chunk", str(CHUNK), "--min-warmup-launches", "2",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == STEPS and d["warmup"] == WARM and d["dtype"] == "f32" and d["higher_is_better"] is True
    assert d["config"]["n_launch"] == 3 and d["config"]["last_launch_steps"] == 20
    assert d["value"] == pytest.approx(N_ENV * STEPS / (d["ms_per_step"] * 1e-3 * STEPS))
    assert not {"c5", "c3_f64", "c5_torch_actor", "cpu_baseline"} & set(d)       # --full only

    e = VecMultiShipRLEnv(scenario=make_scenario(N_ENV, cap=48, seed=SEED), precision=32, device="cuda:0")
    e.reset()
    e.init_step()
    cap = max(N_ENV, N_ENV * CHUNK // 192)
    for k in (CHUNK, CHUNK, CHUNK, CHUNK, 20):
        out = e.rollout(k, seed=SEED, transition_capacity=cap)
    torch.cuda.synchronize()
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert all(np.isfinite(a).all() and a.dtype in (np.float32, np.float64) for a in got.values())
    for f in ("next_state", "reward", "done", "status"):
        assert np.array_equal(got[f], out[f][-1].cpu().numpy().astype(got[f].dtype)), f
    act = out["action"][-1].cpu().numpy()
    assert np.array_equal(got["action"], np.where(np.isfinite(act), act, np.float32(0)))
    assert np.array_equal(got.get("action_nonfinite", np.zeros_like(act)) != 0, ~np.isfinite(act))
    assert np.array_equal(got["done_count"], out["done_count"].cpu().numpy().astype(np.float64))
    count = int(out["transition_count"].item())
    assert got["transition_count"].tolist() == [float(count)] and count <= cap
    want = bench.canonical_transitions(out["transitions"], count, 0).numpy()
    want = np.where(np.isfinite(want), want, np.float32(0))
    assert got["transitions"].shape == want.shape and np.array_equal(got["transitions"], want)
