#!/usr/bin/env python3
"""Cost of the observation normalisation: update, fold, the normalised sample, and the iteration graph (GPU).

    python3 tools/obsnorm_cost.py [--n-env 32768] [--chunk 80] [--runs 25] [--warmup 3] [out.json]

Every figure is a median over `runs` timed runs (at least 20) after `warmup` untimed ones, HIP events, by the method
of tools/score_cost.py: a call is a few microseconds, so a stand-alone run is one replay of a HIP graph of `--calls`
consecutive calls and the figure is the replay time per call.
 * ObsNormalizer.update at 1 024, 16 384 and 65 536 new records.  An update consumes its records, so every call
   of the timed graph is preceded by a one-element add that moves the replay cursor on by that many records; the
   same graph of the adds alone is timed too and subtracted (`update_us`);
 * ObsNormalizer.fold of the actor block;
 * ReplayMemory.sample plain against normalised at (B 64, U 8) and (B 16 384, U 1);
 * the iteration graph (launch, push, [norm.update,] score update, keep, update_many(batch, n)) with the normaliser
   (serving the folded block, normalised minibatches, the fold at the end) and without it, which is the iteration
   of the commit before; two envs of the same shape on the same device, replays of the two graphs alternating.
Writes profiles/r15_obsnorm_cost.json."""
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
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "r15_obsnorm_cost.json"))
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("time at least 20 runs")
    import torch
    if not torch.cuda.is_available():
        sys.exit("obsnorm_cost: needs a GPU (a CPU run gives no time)")
    from sac_maritime_ast_amd import ObsNormalizer, ReplayMemory, Scoreboard, VecMultiShipRLEnv, _lib, make_scenario, sac
    from sac_maritime_ast_amd.obsnorm import REFERENCE_OBS_HIGH, REFERENCE_OBS_LOW
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

    def started_env():
        e = VecMultiShipRLEnv(scenario=make_scenario(a.n_env, cap=48), precision=32, device=dev)
        e.reset()
        e.init_step()
        return e

    env = started_env()
    res = {"what": "ObsNormalizer.update / fold, plain against normalised sample, and the iteration graph with and "
                   "without the normaliser, HIP events, medians",
           "n_env": a.n_env, "chunk": a.chunk, "batch": a.batch, "n_updates": a.n_updates, "runs": a.runs,
           "warmup": a.warmup, "calls_per_standalone_run": a.calls}
    gen = torch.Generator().manual_seed(1)
    lo, hi = torch.from_numpy(REFERENCE_OBS_LOW), torch.from_numpy(REFERENCE_OBS_HIGH)

    def filled(capacity):
        mem = ReplayMemory(env, capacity)
        ring = torch.randn((capacity, _lib.SIT_TRANSITION_DIM), generator=gen)
        for c0 in (0, 12):
            ring[:, c0:c0 + 10] = lo + (hi - lo) * torch.rand((capacity, 10), generator=gen)
        mem.ring.copy_(ring)
        mem.cursor[0] = capacity
        return mem

    # ---- update ----
    update = {}
    for m in (1024, 16384, 65536):
        mem = filled(m)
        norm = ObsNormalizer(env)                    # (a fresh one: `seen` starts below this memory's cursor)
        norm.reserve(65536)

        def advance():
            mem.cursor[0:1].add_(m)

        def advance_and_update():
            advance()
            norm.update(mem, m)
        both = timed(graph_of(advance_and_update, a.calls).replay, a.calls)
        add = timed(graph_of(advance, a.calls).replay, a.calls)
        update[f"new_{m}"] = {"cursor_add_and_update": both, "cursor_add": add, "update_us": both["median_us"] - add["median_us"]}
        out = norm.read()
        update[f"new_{m}"]["accounted"] = {k: out[k] for k in ("n", "updates", "seen", "skipped")}
    res["update"] = update

    # ---- fold ----
    src, dst = torch.randn(_lib.SIT_ACTOR_WEIGHTS, device=dev), torch.zeros(_lib.SIT_ACTOR_WEIGHTS, device=dev)
    res["fold"] = timed(graph_of(lambda: norm.fold(src, dst), a.calls).replay, a.calls)
    res["fold"]["actor_block_bytes"] = 4 * _lib.SIT_ACTOR_WEIGHTS

    # ---- sample ----
    mem = filled(1 << 17)
    sample = {}
    for B, U in ((64, 8), (16384, 1)):
        row = {}
        for name, kw in (("plain", {}), ("normalised", {"normalizer": norm})):
            buf = mem.sample(B, U, **kw)
            row[name] = timed(graph_of(lambda: mem.sample(B, U, out=buf, **kw), a.calls).replay, a.calls)
        row["normalised_minus_plain_us"] = row["normalised"]["median_us"] - row["plain"]["median_us"]
        sample[f"B_{B}_U_{U}"] = row
    res["sample"] = sample

    # ---- the iteration, with and without the normaliser ----
    def iteration_of(e, with_norm):
        torch.manual_seed(4)
        pol = GaussianPolicy().to(dev)
        if not with_norm:
            with torch.no_grad():
                pol.net[0].weight.mul_(1e-3)         # raw observations: keep the actions inside (-1, 1)
        tcap = max(a.n_env, a.n_env * a.chunk // 192)
        sampler = PolicySampler(e, pol, chunk=a.chunk, transition_capacity=tcap, episode_capacity=a.episode_capacity)
        nrm = ObsNormalizer(e) if with_norm else None
        learner = sac.SacLearner(e, pol, gradient="hip", obs_norm=nrm)
        sampler.share_weights(learner.serving_weights if with_norm else learner.actor_weights)
        mem = ReplayMemory(e, 1 << 20)
        mem.reserve(tcap)
        board = Scoreboard(e)
        board.reserve(a.episode_capacity)
        best = [torch.zeros_like(learner.actor_weights) for _ in range(2)]
        best_affine = torch.zeros(_lib.SIT_OBSNORM_AFFINE, device=dev)
        if with_norm:
            nrm.reserve(tcap)
        while len(mem) <= a.batch:
            mem.push(sampler.launch())

        def iteration():
            mem.push(sampler.launch())
            pairs = [(learner.actor_weights, best[0])]
            if with_norm:
                nrm.update(mem, tcap)
                pairs += [(learner.serving_weights, best[1]), (nrm.affine, best_affine)]
            board.update(sampler.episodes, consume=True)
            board.keep(pairs, stamp=learner.clock)
            learner.update_many(mem, a.batch, a.n_updates)
        return iteration, nrm, board

    other = started_env()
    parts = {"with_normaliser": iteration_of(env, True), "without_normaliser": iteration_of(other, False)}
    graphs = {name: graph_of(p[0], 1) for name, p in parts.items()}
    ts = {name: [] for name in graphs}
    for i in range(a.warmup + a.runs):
        for name, g in graphs.items():
            ev[0].record()
            g.replay()
            ev[1].record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ts[name].append(ev[0].elapsed_time(ev[1]) * 1e3)
    it = {name: {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t)} for name, t in ts.items()}
    it["normaliser_us"] = it["with_normaliser"]["median_us"] - it["without_normaliser"]["median_us"]
    it["without_normaliser_is"] = "the iteration of the commit before (no normaliser: the same calls and bits)"
    out = parts["with_normaliser"][1].read()
    it["normaliser"] = {k: (out[k] if isinstance(out[k], int) else [float(v) for v in out[k]]) for k in
                        ("n", "updates", "seen", "skipped", "shift", "scale")}
    it["episodes"] = {name: p[2].read()["episodes"] for name, p in parts.items()}
    res["iteration_graph"] = it
    res["step_kernel"] = env.lib.sit_step_kernel(env.handle).decode()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
