#!/usr/bin/env python3
"""Cost of the SAC learner's no-gradient half: the fused HIP path next to PyTorch (GPU).

    python3 tools/sac_cost.py [--calls 30] [--warmup 5] [out.json]
    python3 tools/sac_cost.py --gradient [--calls 30] [--warmup 5] [out.json]
    python3 tools/sac_cost.py --weight-gradient [--calls 30] [--warmup 5] [out.json]
    python3 tools/sac_cost.py --rows [--calls 30] [--warmup 5] [out.json]
    python3 tools/sac_cost.py --clocked [--parent build_diag/libsit_parent.so] [--large] [--order a,b,c,a0] [out.json]
    rocprofv3 --kernel-trace --stats ... -- python3 tools/sac_cost.py --rows --trace valu|mfma

float32 handle of 64 envs, the reference's networks (actor 10-256-256-2, twin critic 11-256-256-1,
default initialisation), a ring of 4096 synthetic normalised records.  Every figure is the median of
`calls` HIP-event spans after `warmup` calls, the alternatives interleaved call by call on one stream:

  target   sit_sac_target against the same formulas as PyTorch ops without gradients (torch_target; its
           noise by torch.randn on the device), at B = 64, 256, 4096
  polyak   sit_sac_polyak on the packed two-critic block (alone, and with the in-place repack of the online
           critics that precedes it in SacLearner) against the per-parameter update t += tau (p - t)
  update   a whole SacLearner.update_parameters at batch 64 with target="hip" and target="torch" (each
           ends with the host reading the five results, so the span is also the wall time)

and the share of an update the no-gradient half takes (target + Polyak over the update).  There is no
pass threshold; the result goes to profiles/r08_sac_cost.json.

--gradient measures the gradient half instead (profiles/r09_sac_update_cost.json), the same way:

  update   a whole SacLearner.update_parameters at batch 64 with gradient="hip" and gradient="torch" (both
           target="hip"), interleaved call by call
  calls    sit_sac_critic_step and sit_sac_policy_step alone, on a learner's own blocks
  read     the host read of the five results alone (``_results.tolist()`` on an idle stream), and its share
           of a gradient="hip" update

--weight-gradient measures the tiled weight-gradient calls next to the plain ones
(profiles/r10_sac_wgrad_cost.json), at B = 64, 256, 1024, 4096 and 16384 from a ring of 32768 records:

  calls    sit_sac_critic_step against sit_sac_critic_step_tiled and sit_sac_policy_step against
           sit_sac_policy_step_tiled, on a learner's own blocks, interleaved call by call
  update   a whole SacLearner.update_parameters with weight_gradient="sum" and "mfma" (both gradient="hip")

with, per pair, whether the tiled call's min-max range lies wholly below the plain call's.

--rows measures the wide (32 rows per block, MFMA) row kernels next to the narrow ones
(profiles/r12_sac_rows_cost.json), at the same batch sizes from the same ring:

  calls    sit_sac_target against sit_sac_target_wide, sit_sac_critic_step_tiled against
           sit_sac_critic_step_wide and sit_sac_policy_step_tiled against sit_sac_policy_step_wide, interleaved
           call by call (each pair differs in its row kernel only)
  update   a whole SacLearner.update_parameters with row_pass="valu" and "mfma" (both weight_gradient="mfma")

with, per pair, whether the wide call's min-max range lies wholly below the narrow call's, and the smallest
batch from which that holds for all four.  --rows --trace MODE times nothing: it runs `warmup + calls` updates
at B = 16384 with row_pass=MODE and exits, for a kernel trace of one mode in a run of its own (the
row-kernel / tile-kernel split of an update: profiles/r12_sac_rows_kernel_stats.csv).

--clocked measures ``SacLearner.update_many`` next to ``update_parameters`` (profiles/r13_sac_clock_cost.json): the
time per update of a span of 8 updates at B = 64, 256 (sum/valu) and 4096 (mfma/valu), with --large also 16384
(mfma/mfma), from a ring of 32768 records, the variants of one batch size interleaved span by span:

  a    8 update_parameters calls (each reads its results on the host)
  b    update_many(memory, B, 8), eagerly
  c    a replay of a HIP graph of update_many(memory, B, 8)
  a0   the same 8 update_parameters calls on a handle of the parent revision's library (--parent: a library
       built by `tools/build_variant.py parent --rev <parent>`; without one the variant is left out)

with, per batch size, whether c's whole min-max range lies below a0's and whether a's range overlaps a0's.
--order sets the order of the variants within a round (a variant's span starts where its predecessor's ended)."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--gradient", action="store_true", help="measure the gradient half (r09_sac_update_cost.json)")
    ap.add_argument("--weight-gradient", action="store_true",
                    help="measure the tiled weight-gradient calls against the plain ones (r10_sac_wgrad_cost.json)")
    ap.add_argument("--rows", action="store_true",
                    help="measure the wide row-kernel calls against the narrow ones (r12_sac_rows_cost.json)")
    ap.add_argument("--trace", choices=("valu", "mfma"), default=None,
                    help="with --rows: only run updates at B = 16384 in this mode, for a profiler's kernel trace")
    ap.add_argument("--clocked", action="store_true",
                    help="measure update_many (eager and as a graph) against update_parameters (r13_sac_clock_cost.json)")
    ap.add_argument("--parent", default=None, help="with --clocked: the parent revision's library (variant a0)")
    ap.add_argument("--large", action="store_true", help="with --clocked: also B = 16384 with mfma/mfma")
    ap.add_argument("--order", default="a,b,c,a0", help="with --clocked: the order of the variants within a round")
    ap.add_argument("out", nargs="?", default=None)
    a = ap.parse_args()
    if a.trace and not a.rows:
        ap.error("--trace goes with --rows")
    if a.gradient + a.weight_gradient + a.rows + a.clocked > 1:
        ap.error("--gradient, --weight-gradient, --rows and --clocked are separate measurements")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "r13_sac_clock_cost.json" if a.clocked else
                             "r12_sac_rows_cost.json" if a.rows else
                             "r10_sac_wgrad_cost.json" if a.weight_gradient else
                             "r09_sac_update_cost.json" if a.gradient else "r08_sac_cost.json")
    if a.calls < 20:
        ap.error("time at least 20 calls")
    import torch
    if not torch.cuda.is_available():
        sys.exit("sac_cost: needs a GPU (a CPU run gives no time)")
    from sac_maritime_ast_amd import ReplayMemory, VecMultiShipRLEnv, _lib, make_scenario, sac
    from sac_maritime_ast_amd.samplers import GaussianPolicy

    dev = "cuda:0"
    env = VecMultiShipRLEnv(scenario=make_scenario(64), precision=32, device=dev)
    torch.manual_seed(0)
    pol0, q0 = GaussianPolicy(), sac.QNetwork()

    def learner(target, gradient="torch", weight_gradient="sum", row_pass="valu", env=env):
        return sac.SacLearner(env, copy.deepcopy(pol0).to(dev), critic=copy.deepcopy(q0), target=target, seed=1,
                              gradient=gradient, weight_gradient=weight_gradient, row_pass=row_pass)

    def memory(capacity=4096, env=env):
        mem = ReplayMemory(env, capacity, seed=1)
        g = torch.Generator(device=dev).manual_seed(2)
        mem.ring.copy_(torch.randn(mem.ring.shape, generator=g, device=dev))
        mem.ring[:, 10].tanh_()
        mem.ring[:, 22] = (mem.ring[:, 22] > -0.7).to(mem.ring.dtype)
        mem.cursor[0] = capacity
        return mem

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def span(fn):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3     # microseconds

    def interleaved(fns):
        """{name: median us} of the named calls, run in turn `warmup + calls` times."""
        t = {k: [] for k in fns}
        for i in range(a.warmup + a.calls):
            for k, fn in fns.items():
                us = span(fn)
                if i >= a.warmup:
                    t[k].append(us)
        return {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in t.items()}

    def finish(res):
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        env.close()

    if a.clocked:
        env0 = None
        if a.parent:                               # a second handle, on the parent revision's library
            ours, path = _lib._lib, _lib.LIB_PATH
            _lib._lib, _lib.LIB_PATH = None, os.path.abspath(a.parent)
            try:
                env0 = VecMultiShipRLEnv(scenario=make_scenario(64), precision=32, device=dev)
            finally:
                _lib._lib, _lib.LIB_PATH = ours, path
            assert env0.lib is not env.lib and not hasattr(env0.lib, "sit_sac_updates")
        res = clocked(a, torch, env, env0, learner, memory, interleaved)
        if env0 is not None:
            env0.close()
        return finish(res)
    if a.gradient:
        return finish(gradient_half(a, torch, env, _lib, learner, memory, interleaved))
    if a.weight_gradient:
        return finish(weight_gradient(a, torch, env, _lib, learner, memory, interleaved))
    if a.rows and a.trace:
        lrn, mem = learner("hip", "hip", "mfma", a.trace), memory(32768)
        for u in range(a.warmup + a.calls):
            assert lrn.update_parameters(mem, 16384, u) is not None
        torch.cuda.synchronize()
        return env.close()
    if a.rows:
        return finish(row_kernels(a, torch, env, _lib, learner, memory, interleaved))
    hip, tor = learner("hip"), learner("torch")
    res = {"what": __doc__.split("\n\n")[0], "calls": a.calls, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "target": {}, "polyak": {}, "update": {}}
    # ---- target ----
    for B in (64, 256, 4096):
        ns = torch.randn(B, _lib.SIT_OBS_DIM, device=dev)
        reward, mask = torch.randn(B, device=dev), torch.ones(B, device=dev)

        def by_torch():
            eps = torch.randn(B, device=dev)
            return sac.torch_target(tor.policy, tor.target_critic, ns, reward, mask, eps, tor.alpha, tor.gamma)["y"]
        r = interleaved({"hip": lambda: hip.td_target(ns, reward, mask, 7), "torch": by_torch})
        r["torch_over_hip"] = r["torch"]["median_us"] / r["hip"]["median_us"]
        res["target"][str(B)] = r
    # ---- polyak ----
    def hip_kernel():
        with torch.cuda.device(env.device):
            env._call("sit_sac_polyak", hip.target_weights.data_ptr(), hip.online_weights.data_ptr(),
                      hip.online_weights.numel(), hip.tau, env._stream())
    r = interleaved({"hip_kernel": hip_kernel, "hip_repack_and_kernel": hip._polyak, "torch": tor._polyak})
    r["torch_over_hip_repack_and_kernel"] = r["torch"]["median_us"] / r["hip_repack_and_kernel"]["median_us"]
    res["polyak"] = r
    # ---- a whole update ----
    mems = {"hip": memory(), "torch": memory()}
    count = {"hip": 0, "torch": 0}
    wall = {"hip": [], "torch": []}

    def update(mode, lrn):
        def fn():
            t0 = time.perf_counter()
            out = lrn.update_parameters(mems[mode], 64, count[mode])
            wall[mode].append((time.perf_counter() - t0) * 1e6)
            count[mode] += 1
            assert out is not None
        return fn
    r = interleaved({"hip": update("hip", hip), "torch": update("torch", tor)})
    for mode in ("hip", "torch"):
        r[mode]["wall_median_us"] = statistics.median(wall[mode][a.warmup:])
    r["torch_over_hip"] = r["torch"]["median_us"] / r["hip"]["median_us"]
    res["update"] = r
    t64 = res["target"]["64"]
    res["no_grad_share_of_update"] = {
        "hip": (t64["hip"]["median_us"] + res["polyak"]["hip_repack_and_kernel"]["median_us"]) / r["hip"]["median_us"],
        "torch": (t64["torch"]["median_us"] + res["polyak"]["torch"]["median_us"]) / r["torch"]["median_us"]}
    res["faster_update_at_batch_64"] = "hip" if r["hip"]["median_us"] <= r["torch"]["median_us"] else "torch"
    finish(res)


def step_calls(torch, env, _lib, h, B):
    """The two gradient calls alone at batch B on learner h's blocks (its parameters move as in training):
    critic_step(suffix) and policy_step(suffix) return the call of that entry point ("" or "_tiled")."""
    from ctypes import byref
    dev, dt = env.device, env.dtype
    state, action, y = (torch.randn(B, 10, device=dev, dtype=dt), torch.rand(B, device=dev, dtype=dt) * 2 - 1,
                        torch.randn(B, device=dev, dtype=dt))
    ws = torch.empty(2 * B * _lib.SIT_SAC_WORKSPACE_ROW, dtype=torch.float32, device=dev)
    c, p = _lib.SacCriticStepArgs(), _lib.SacPolicyStepArgs()
    c.batch, c.workspace_floats = B, ws.numel()
    c.critic_weights, c.critic_m, c.critic_v = h.online_weights.data_ptr(), h._m["critic"].data_ptr(), h._v["critic"].data_ptr()
    c.state, c.action, c.y, c.workspace, c.results = (state.data_ptr(), action.data_ptr(), y.data_ptr(), ws.data_ptr(),
                                                      h._results.data_ptr())
    p.batch, p.tune, p.workspace_floats, p.seed, p.target_entropy = B, 1, ws.numel(), 1, -1.0
    p.actor_weights, p.actor_m, p.actor_v = h.actor_weights.data_ptr(), h._m["policy"].data_ptr(), h._v["policy"].data_ptr()
    p.critic_weights, p.alpha = h.online_weights.data_ptr(), h.alpha.data_ptr()
    p.log_alpha, p.log_alpha_m, p.log_alpha_v = h.log_alpha.data_ptr(), h._m["alpha"].data_ptr(), h._v["alpha"].data_ptr()
    p.state, p.workspace, p.results = state.data_ptr(), ws.data_ptr(), h._results.data_ptr()
    n = {"u": 0}
    keep = (state, action, y, ws)                  # the arguments hold addresses only

    def critic_step(suffix=""):
        def fn(keep=keep):
            c.adam = h._adam("critic")
            with torch.cuda.device(dev):
                env._call("sit_sac_critic_step" + suffix, byref(c), env._stream())
        return fn

    def policy_step(suffix=""):
        def fn(keep=keep):
            n["u"] += 1
            p.update, p.adam, p.alpha_adam = n["u"], h._adam("policy"), h._adam("alpha")
            with torch.cuda.device(dev):
                env._call("sit_sac_policy_step" + suffix, byref(p), env._stream())
        return fn
    return critic_step, policy_step


def weight_gradient(a, torch, env, _lib, learner, memory, interleaved):
    """The --weight-gradient measurement (see the module docstring)."""
    batches = (64, 256, 1024, 4096, 16384)
    capacity = 32768
    res = {"what": "Cost of the tiled (MFMA) weight-gradient calls next to the plain ones, and of a whole update with "
                   "weight_gradient='mfma' next to 'sum' (GPU).", "calls": a.calls, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "ring_records": capacity, "batch": {}}
    lrn = {"sum": learner("hip", "hip", "sum"), "mfma": learner("hip", "hip", "mfma")}
    mems = {k: memory(capacity) for k in lrn}
    count = {k: 0 for k in lrn}
    h = learner("hip", "hip")

    def update(mode, B):
        def fn():
            out = lrn[mode].update_parameters(mems[mode], B, count[mode])
            count[mode] += 1
            assert out is not None
        return fn

    def below(r, tiled, plain):
        return r[tiled]["max_us"] < r[plain]["min_us"]
    for B in batches:
        assert len(mems["sum"]) > B
        critic_step, policy_step = step_calls(torch, env, _lib, h, B)
        r = interleaved({"sit_sac_critic_step": critic_step(), "sit_sac_critic_step_tiled": critic_step("_tiled"),
                         "sit_sac_policy_step": policy_step(), "sit_sac_policy_step_tiled": policy_step("_tiled"),
                         "update_sum": update("sum", B), "update_mfma": update("mfma", B)})
        assert all(v == v for v in h._results.tolist())
        r["tiled_range_below_plain"] = {"critic": below(r, "sit_sac_critic_step_tiled", "sit_sac_critic_step"),
                                        "policy": below(r, "sit_sac_policy_step_tiled", "sit_sac_policy_step"),
                                        "update": below(r, "update_mfma", "update_sum")}
        r["plain_over_tiled_median"] = {
            "critic": r["sit_sac_critic_step"]["median_us"] / r["sit_sac_critic_step_tiled"]["median_us"],
            "policy": r["sit_sac_policy_step"]["median_us"] / r["sit_sac_policy_step_tiled"]["median_us"],
            "update": r["update_sum"]["median_us"] / r["update_mfma"]["median_us"]}
        res["batch"][str(B)] = r
    res["tiled_calls_below_plain_at_every_batch_from_1024"] = all(
        res["batch"][str(B)]["tiled_range_below_plain"][k] for B in batches if B >= 1024 for k in ("critic", "policy"))
    return res


def row_kernels(a, torch, env, _lib, learner, memory, interleaved):
    """The --rows measurement (see the module docstring)."""
    batches = (64, 256, 1024, 4096, 16384)
    capacity = 32768
    res = {"what": "Cost of the wide (32 rows per block, MFMA) row-kernel calls next to the narrow ones, and of a whole "
                   "update with row_pass='mfma' next to 'valu', both weight_gradient='mfma' (GPU).", "calls": a.calls,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "ring_records": capacity, "batch": {}}
    lrn = {m: learner("hip", "hip", "mfma", m) for m in ("valu", "mfma")}
    mems = {k: memory(capacity) for k in lrn}
    count = {k: 0 for k in lrn}
    h = learner("hip", "hip", "mfma")
    dev = env.device
    pairs = {"target": ("sit_sac_target", "sit_sac_target_wide"),
             "critic": ("sit_sac_critic_step_tiled", "sit_sac_critic_step_wide"),
             "policy": ("sit_sac_policy_step_tiled", "sit_sac_policy_step_wide"), "update": ("update_valu", "update_mfma")}

    def update(mode, B):
        def fn():
            out = lrn[mode].update_parameters(mems[mode], B, count[mode])
            count[mode] += 1
            assert out is not None
        return fn

    def target(mode, ns, reward, mask):
        def fn():
            h.row_pass = mode
            h.td_target(ns, reward, mask, 7)
        return fn
    for B in batches:
        assert len(mems["valu"]) > B
        critic_step, policy_step = step_calls(torch, env, _lib, h, B)
        ns = torch.randn(B, _lib.SIT_OBS_DIM, device=dev)
        reward, mask = torch.randn(B, device=dev), torch.ones(B, device=dev)
        r = interleaved({"sit_sac_target": target("valu", ns, reward, mask),
                         "sit_sac_target_wide": target("mfma", ns, reward, mask),
                         "sit_sac_critic_step_tiled": critic_step("_tiled"), "sit_sac_critic_step_wide": critic_step("_wide"),
                         "sit_sac_policy_step_tiled": policy_step("_tiled"), "sit_sac_policy_step_wide": policy_step("_wide"),
                         "update_valu": update("valu", B), "update_mfma": update("mfma", B)})
        assert all(v == v for v in h._results.tolist())
        r["wide_range_below_narrow"] = {k: r[w]["max_us"] < r[n]["min_us"] for k, (n, w) in pairs.items()}
        r["narrow_over_wide_median"] = {k: r[n]["median_us"] / r[w]["median_us"] for k, (n, w) in pairs.items()}
        res["batch"][str(B)] = r
    holds = [B for B in batches if all(res["batch"][str(B)]["wide_range_below_narrow"].values())]
    from_b = [B for B in batches if all(b in holds for b in batches if b >= B)]
    res["smallest_batch_from_which_all_four_ranges_lie_below"] = from_b[0] if from_b else None
    return res


def clocked(a, torch, env, env0, learner, memory, interleaved):
    """The --clocked measurement (see the module docstring)."""
    n, capacity = 8, 32768
    plan = [(64, "sum", "valu"), (256, "sum", "valu"), (4096, "mfma", "valu")] + ([(16384, "mfma", "mfma")] if a.large else [])
    res = {"what": "Time per SAC update: 8 update_parameters calls (a; a0 on the parent revision's library) next to "
                   "update_many(memory, B, 8) eagerly (b) and as a HIP-graph replay (c) (GPU).", "calls": a.calls,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "ring_records": capacity, "updates_per_span": n,
           "parent_library": os.path.basename(a.parent) if a.parent else None, "batch": {}}
    for B, wg, rp in plan:
        names = ["a", "b", "c"] + (["a0"] if env0 is not None else [])
        lrn = {k: learner("hip", "hip", wg, rp, env=env0 if k == "a0" else env) for k in names}
        mems = {k: memory(capacity, env=env0 if k == "a0" else env) for k in names}
        count = {k: 0 for k in names}

        def by_calls(k):
            def fn():
                for _ in range(n):
                    assert lrn[k].update_parameters(mems[k], B, count[k]) is not None
                    count[k] += 1
            return fn
        lrn["c"].update_many(mems["c"], B, n, first_update=0)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            lrn["c"].update_many(mems["c"], B, n)
        fns = {"a": by_calls("a"), "b": lambda: lrn["b"].update_many(mems["b"], B, n), "c": graph.replay}
        if env0 is not None:
            fns["a0"] = by_calls("a0")
        r = interleaved({k: fns[k] for k in a.order.split(",") if k in fns})
        r["order"] = a.order
        for k in names:
            r[k] = {f"{stat}_per_update": v / n for stat, v in r[k].items()}
        assert all(v == v for row in lrn["c"].results(last=n) for v in row)
        r["mode"] = f"{wg}/{rp}"
        r["a_over_b_median"] = r["a"]["median_us_per_update"] / r["b"]["median_us_per_update"]
        r["a_over_c_median"] = r["a"]["median_us_per_update"] / r["c"]["median_us_per_update"]
        r["c_range_below_a"] = r["c"]["max_us_per_update"] < r["a"]["min_us_per_update"]
        if env0 is not None:
            r["a0_over_c_median"] = r["a0"]["median_us_per_update"] / r["c"]["median_us_per_update"]
            r["c_range_below_a0"] = r["c"]["max_us_per_update"] < r["a0"]["min_us_per_update"]
            r["a_range_overlaps_a0"] = (r["a"]["min_us_per_update"] <= r["a0"]["max_us_per_update"]
                                        and r["a0"]["min_us_per_update"] <= r["a"]["max_us_per_update"])
        res["batch"][str(B)] = r
        del graph
    return res


def gradient_half(a, torch, env, _lib, learner, memory, interleaved):
    """The --gradient measurement (see the module docstring)."""
    B = 64
    lrn = {"hip": learner("hip", "hip"), "torch": learner("hip", "torch")}
    mems = {k: memory() for k in lrn}
    count = {k: 0 for k in lrn}
    wall = {k: [] for k in lrn}

    def update(mode):
        def fn():
            t0 = time.perf_counter()
            out = lrn[mode].update_parameters(mems[mode], B, count[mode])
            wall[mode].append((time.perf_counter() - t0) * 1e6)
            count[mode] += 1
            assert out is not None
        return fn
    res = {"what": "Cost of a SAC update with the gradient half in HIP (gradient='hip') next to autograd "
                   "(gradient='torch'), batch 64 (GPU).", "calls": a.calls, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "parent_update_us": 3411.4, "parent_source": "profiles/r08_sac_cost.json"}
    r = interleaved({k: update(k) for k in lrn})
    for mode in lrn:
        r[mode]["wall_median_us"] = statistics.median(wall[mode][a.warmup:])
    r["torch_over_hip"] = r["torch"]["median_us"] / r["hip"]["median_us"]
    res["update"] = r
    # ---- the two calls alone, on a third learner's blocks (its parameters move as in training) ----
    h = learner("hip", "hip")
    critic_step, policy_step = step_calls(torch, env, _lib, h, B)
    res["calls_alone"] = interleaved({"sit_sac_critic_step": critic_step(), "sit_sac_policy_step": policy_step(),
                                      "results_host_read": lambda: h._results.tolist()})
    assert all(v == v for v in h._results.tolist())
    res["host_read_share_of_hip_update"] = res["calls_alone"]["results_host_read"]["median_us"] / r["hip"]["median_us"]
    res["hip_update_over_parent"] = r["hip"]["median_us"] / res["parent_update_us"]
    res["faster_update_at_batch_64"] = "hip" if r["hip"]["median_us"] <= r["torch"]["median_us"] else "torch"
    return res


if __name__ == "__main__":
    main()
