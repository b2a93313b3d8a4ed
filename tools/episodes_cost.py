#!/usr/bin/env python3
"""Cost of the device-side episode reducer next to the rollout launch it follows (GPU).

    python3 tools/episodes_cost.py [--n-env 32768] [--steps 2000] [--launches 12] [--warmup 2] [out.json]

float32, synthetic sampler: each launch is one sit_rollout of `steps` rows (about 4.3 GB of rows at the
default shape) followed by one sit_episodes_update over them, on one stream.  HIP events time the two
separately; the medians over the launches after the warm-up go to profiles/r07_episodes_cost.json with
the bytes the update reads and the rate they imply, next to the floor those bytes set at the measured
HBM copy rate."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_TBS = 6.29     # measured float4 copy rate of the MI355X (8.0 TB/s spec)


def update_bytes(n_env: int, steps: int, real: int = 4) -> dict:
    """Bytes one update reads, from the shapes.  The count pass reads done (status only on done rows);
    the walk reads reward, done and status of every row and the event flag action_out[k][e][3], which
    drags in the whole 4-real action rows; next_state and the angle are read on done / event rows only
    (not counted).  `needed` counts the flag alone."""
    rows = n_env * steps
    count = rows * 1
    walk = rows * (real + 1 + 4)
    return {"count_pass": count, "walk_rows": walk, "walk_action_lines": rows * 4 * real,
            "fetched": count + walk + rows * 4 * real, "needed": count + walk + rows * real}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n-env", type=int, default=32768)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "r07_episodes_cost.json"))
    a = ap.parse_args()
    if a.launches < 10:
        ap.error("time at least 10 launches")
    import torch
    if not torch.cuda.is_available():
        sys.exit("episodes_cost: needs a GPU (a CPU run gives no time)")
    from sac_maritime_ast_amd import EpisodeLog, VecMultiShipRLEnv, make_scenario

    dev = "cuda:0"
    env = VecMultiShipRLEnv(scenario=make_scenario(a.n_env), precision=32, device=dev)
    env.reset()
    env.init_step()
    log = EpisodeLog(env, capacity=1 << 20)
    want = ("next_state", "reward", "done", "status", "action")
    out = {}
    t_roll, t_upd, episodes = [], [], 0
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for i in range(a.warmup + a.launches):
        ev[0].record()
        env.rollout(a.steps, seed=25450, want=want, out=out)
        ev[1].record()
        log.update(out)
        ev[2].record()
        torch.cuda.synchronize()
        got = log.drain()
        if i >= a.warmup:
            t_roll.append(ev[0].elapsed_time(ev[1]))
            t_upd.append(ev[1].elapsed_time(ev[2]))
            episodes += len(got["env"]) + got["dropped"]
    b = update_bytes(a.n_env, a.steps)
    roll_ms, upd_ms = statistics.median(t_roll), statistics.median(t_upd)
    row_bytes = a.n_env * a.steps * (4 * (10 + 1 + 4) + 1 + 4)
    res = {
        "what": "sit_episodes_update after sit_rollout, float32, synthetic sampler, HIP events, medians",
        "n_env": a.n_env, "steps": a.steps, "launches": a.launches, "warmup": a.warmup,
        "step_kernel": env.lib.sit_step_kernel(env.handle).decode(),
        "rollout_rows_bytes": row_bytes,
        "rollout_ms": roll_ms, "rollout_ms_min_max": [min(t_roll), max(t_roll)],
        "rollout_env_steps_per_s": a.n_env * a.steps / (roll_ms * 1e-3),
        "update_ms": upd_ms, "update_ms_min_max": [min(t_upd), max(t_upd)],
        "update_over_rollout": upd_ms / roll_ms,
        "update_bytes": b,
        "update_tb_per_s_fetched": b["fetched"] / (upd_ms * 1e-3) / 1e12,
        "update_tb_per_s_needed": b["needed"] / (upd_ms * 1e-3) / 1e12,
        "hbm_copy_tb_per_s": HBM_COPY_TBS,
        "byte_floor_ms_fetched": b["fetched"] / (HBM_COPY_TBS * 1e12) * 1e3,
        "byte_floor_ms_needed": b["needed"] / (HBM_COPY_TBS * 1e12) * 1e3,
        "episodes_per_launch": episodes / a.launches,
    }
    res["update_over_byte_floor_fetched"] = upd_ms / res["byte_floor_ms_fetched"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
