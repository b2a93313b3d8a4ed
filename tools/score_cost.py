#!/usr/bin/env python3
"""Cost of the device-side scores: the update, keep, and both inside the training iteration (GPU).

    python3 tools/score_cost.py [--n-env 32768] [--chunk 80] [--runs 25] [--warmup 3] [out.json]

Every figure is a median over `runs` timed runs (at least 20) after `warmup` untimed ones, HIP events:
 * the stand-alone sit_score_update at record capacity 65 536 with m = 0, 256 and 65 536 valid records and at
   capacity 256 with m = 256.  A call is a few microseconds, below what a pair of events resolves, so a run is
   one replay of a HIP graph of `--calls` consecutive updates and the figure is the replay time per call.  The
   grid is sized by the capacity and blocks past m exit after one load, so m = 256 at capacity 65 536 should
   cost the capacity-256 call plus the dispatch of 255 empty blocks (`early_exit_ratio`);
 * sit_score_keep of the actor block with score[7] = 1 (the copy) and = 0 (nothing written), the same way;
 * EpisodeLog.update and Scoreboard.update behind one policy launch of the iteration's shape, one call per run;
 * the iteration graph (launch, push, [score update, keep,] update_many(batch, n)) with and without the two
   score calls, replays of the two graphs alternating.
Writes profiles/r14_score_cost.json."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n-env", type=int, default=32768)
    ap.add_argument("--chunk", type=int, default=80)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--n-updates", type=int, default=4)
    ap.add_argument("--episode-capacity", type=int, default=8192)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=32, help="stand-alone calls per timed graph replay")
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "r14_score_cost.json"))
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("time at least 20 runs")
    import torch
    if not torch.cuda.is_available():
        sys.exit("score_cost: needs a GPU (a CPU run gives no time)")
    from sac_maritime_ast_amd import ReplayMemory, Scoreboard, VecMultiShipRLEnv, _lib, make_scenario, sac
    from sac_maritime_ast_amd.samplers import GaussianPolicy, PolicySampler

    dev = "cuda:0"
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn, per=1):
        """{median, min, max} of fn()'s time in microseconds per call over the timed runs."""
        ts = []
        for i in range(a.warmup + a.runs):
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ts.append(ev[0].elapsed_time(ev[1]) * 1e3 / per)
        return {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts)}

    def graph_of(fn, calls):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(calls):
                fn()
        return g

    env = VecMultiShipRLEnv(scenario=make_scenario(a.n_env, cap=48), precision=32, device=dev)
    env.reset()
    env.init_step()
    res = {"what": "sit_score_update / sit_score_keep alone and inside the iteration graph, HIP events, medians",
           "n_env": a.n_env, "chunk": a.chunk, "batch": a.batch, "n_updates": a.n_updates, "runs": a.runs,
           "warmup": a.warmup, "calls_per_standalone_run": a.calls}

    # ---- the stand-alone update ----
    board = Scoreboard(env)
    board.reserve(65536)
    gen = torch.Generator().manual_seed(1)
    update = {}
    for capacity, m in ((65536, 0), (65536, 256), (65536, 65536), (256, 256)):
        records = torch.randn((capacity, _lib.SIT_EPISODE_DIM), generator=gen, dtype=torch.float64).to(dev)
        records[:, 4] = torch.randint(0, 1 << 14, (capacity,), generator=gen).to(dev)
        count = torch.tensor([m], dtype=torch.int64, device=dev)
        g = graph_of(lambda: board.update(records=records, count=count), a.calls)
        update[f"capacity_{capacity}_m_{m}"] = timed(g.replay, a.calls)
        update[f"capacity_{capacity}_m_{m}"]["eager_one_call"] = timed(lambda: board.update(records=records, count=count))
    res["update"] = update
    res["early_exit_ratio"] = update["capacity_65536_m_256"]["median_us"] / update["capacity_256_m_256"]["median_us"]

    # ---- keep ----
    src, dst = torch.randn(_lib.SIT_ACTOR_WEIGHTS, device=dev), torch.zeros(_lib.SIT_ACTOR_WEIGHTS, device=dev)
    stamp = torch.zeros(1, dtype=torch.int64, device=dev)
    g = graph_of(lambda: board.keep([(src, dst)], stamp=stamp), a.calls)
    keep = {}
    for name, flag in (("copy", 1.0), ("no_copy", 0.0)):
        board.block[7] = flag
        keep[name] = timed(g.replay, a.calls)
    keep["actor_block_bytes"] = 4 * _lib.SIT_ACTOR_WEIGHTS
    res["keep"] = keep

    # ---- the iteration ----
    torch.manual_seed(4)
    pol = GaussianPolicy().to(dev)
    with torch.no_grad():
        pol.net[0].weight.mul_(1e-3)
    tcap = max(a.n_env, a.n_env * a.chunk // 192)
    sampler = PolicySampler(env, pol, chunk=a.chunk, transition_capacity=tcap, episode_capacity=a.episode_capacity)
    learner = sac.SacLearner(env, pol, gradient="hip")
    sampler.share_weights(learner.actor_weights)
    mem = ReplayMemory(env, 1 << 20)
    mem.reserve(tcap)
    board.reserve(a.episode_capacity)
    board.reset()
    best_actor = torch.zeros_like(learner.actor_weights)
    while len(mem) <= a.batch:
        mem.push(sampler.launch())
    out = sampler.launch()
    res["episodes_update_same_shape"] = {
        "rows": [a.chunk, a.n_env], "record_capacity": a.episode_capacity,
        "EpisodeLog.update": timed(lambda: sampler.episodes.update(out)),
        "Scoreboard.update": timed(lambda: board.update(sampler.episodes)),
        "records_in_log": min(int(sampler.episodes.count.item()), a.episode_capacity)}
    sampler.episodes.count.zero_()
    board.reset()

    def iteration(score):
        mem.push(sampler.launch())
        if score:
            board.update(sampler.episodes, consume=True)
            board.keep([(learner.actor_weights, best_actor)], stamp=learner.clock)
        learner.update_many(mem, a.batch, a.n_updates)
    graphs = {name: graph_of(lambda: iteration(score), 1) for name, score in (("with_score", True), ("without_score", False))}
    ts = {name: [] for name in graphs}
    for i in range(a.warmup + a.runs):
        for name, g in graphs.items():
            ev[0].record()
            g.replay()
            ev[1].record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ts[name].append(ev[0].elapsed_time(ev[1]) * 1e3)
    res["iteration_graph"] = {name: {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t)}
                              for name, t in ts.items()}
    res["iteration_graph"]["score_calls_us"] = (res["iteration_graph"]["with_score"]["median_us"]
                                                - res["iteration_graph"]["without_score"]["median_us"])
    res["iteration_graph"]["board"] = {k: v for k, v in board.read().items() if k != "best"}
    res["step_kernel"] = env.lib.sit_step_kernel(env.handle).decode()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
