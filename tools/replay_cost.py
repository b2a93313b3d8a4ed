#!/usr/bin/env python3
"""Cost of the device-side replay memory next to the rollout launch it follows (GPU).

    python3 tools/replay_cost.py [--n-env 32768] [--steps 40000] [--launches 12] [--warmup 2] [out.json]

float32, synthetic sampler, the bench's C3 shape: each launch is one sit_rollout of `steps` rows whose
sampling-event transitions go to a buffer of the bench's capacity (max(n_env, n_env * steps / 192)
records), followed by one sit_replay_push of that buffer and one sample(64, 64), on one stream.  HIP
events time the three separately; the medians over the launches after the warm-up go to
profiles/r07_replay_cost.json with the bytes each moves.  The push's sort runs over the whole source
capacity whatever the count; its copy moves the valid records only."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_TBS = 6.29     # measured float4 copy rate of the MI355X (8.0 TB/s spec)
RECORD = 24 * 4         # bytes of a float32 transition record


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n-env", type=int, default=32768)
    ap.add_argument("--steps", type=int, default=40000)
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--capacity", type=int, default=1 << 23, help="ring records")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--n-batches", type=int, default=64)
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "r07_replay_cost.json"))
    a = ap.parse_args()
    if a.launches < 10:
        ap.error("time at least 10 launches")
    import torch
    if not torch.cuda.is_available():
        sys.exit("replay_cost: needs a GPU (a CPU run gives no time)")
    from sac_maritime_ast_amd import ReplayMemory, VecMultiShipRLEnv, make_scenario

    dev = "cuda:0"
    env = VecMultiShipRLEnv(scenario=make_scenario(a.n_env, cap=48), precision=32, device=dev)
    env.reset()
    env.init_step()
    tcap = max(a.n_env, a.n_env * a.steps // 192)          # bench.py's capacity per launch
    mem = ReplayMemory(env, a.capacity)
    mem.reserve(tcap)
    out, batches = {}, None
    t_roll, t_push, t_sample, counts = [], [], [], []
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for i in range(a.warmup + a.launches):
        ev[0].record()
        env.rollout(a.steps, seed=25450, out=out, transition_capacity=tcap)
        ev[1].record()
        mem.push(out)
        ev[2].record()
        batches = mem.sample(a.batch, a.n_batches, out=batches)
        ev[3].record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            t_roll.append(ev[0].elapsed_time(ev[1]))
            t_push.append(ev[1].elapsed_time(ev[2]))
            t_sample.append(ev[2].elapsed_time(ev[3]))
            counts.append(int(out["transition_count"].item()))
    # the same push with a zero count: the key pass and the sort over the whole capacity, no copy
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    t_sort = []
    for _ in range(a.launches):
        ev[0].record()
        mem.push(transitions=out["transitions"], count=zero)
        ev[1].record()
        torch.cuda.synchronize()
        t_sort.append(ev[0].elapsed_time(ev[1]))
    roll_ms, push_ms, sample_ms =(statistics.median(t) for t in (t_roll, t_push, t_sample))
    valid = statistics.median(min(c, tcap) for c in counts)
    copied = min(valid, a.capacity)
    # keys: one id per source row read, key and value written; the sort's passes are hipcub's own and
    # not counted; the scatter reads the order and moves the copied records once each way
    push_bytes = {"key_pass": tcap * (4 + 8), "scatter": int(copied) * (2 * RECORD + 4),
                  "sort_items": tcap, "sort_pair_bytes": tcap * 8}
    n_out = a.batch * a.n_batches
    sample_bytes = n_out * (RECORD + 23 * 4 + 2 * 4)
    pushed, dropped, draws, _ = (int(v) for v in mem.cursor.cpu())
    res = {
        "what": "sit_replay_push and sit_replay_sample after sit_rollout, float32, synthetic sampler, HIP events, medians",
        "n_env": a.n_env, "steps": a.steps, "launches": a.launches, "warmup": a.warmup,
        "step_kernel": env.lib.sit_step_kernel(env.handle).decode(),
        "transition_capacity": tcap, "ring_capacity": a.capacity, "batch": a.batch, "n_batches": a.n_batches,
        "records_per_launch_median": valid, "records_per_launch_min_max": [min(counts), max(counts)],
        "rollout_ms": roll_ms, "rollout_ms_min_max": [min(t_roll), max(t_roll)],
        "rollout_env_steps_per_s": a.n_env * a.steps / (roll_ms * 1e-3),
        "push_ms": push_ms, "push_ms_min_max": [min(t_push), max(t_push)],
        "push_over_rollout": push_ms / roll_ms,
        "push_empty_ms": statistics.median(t_sort), "push_empty_ms_min_max": [min(t_sort), max(t_sort)],
        "push_bytes": push_bytes,
        "push_copy_floor_ms": push_bytes["scatter"] / (HBM_COPY_TBS * 1e12) * 1e3,
        "sample_ms": sample_ms, "sample_ms_min_max": [min(t_sample), max(t_sample)],
        "sample_over_rollout": sample_ms / roll_ms,
        "sample_bytes": sample_bytes,
        "hbm_copy_tb_per_s": HBM_COPY_TBS,
        "cursor": {"pushed": pushed, "dropped": dropped, "draws": draws},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
