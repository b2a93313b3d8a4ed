"""The map predicates and the step kernels on maps that reach every path of the spatial index.

tests/test_gpu_map.py and every step-level parity test use one map, the scenario's four islands: the packed
index and the mixed-cell records both in use, at most one further candidate group per cell, integer vertices,
an image that fits every kernel's LDS budget.  The maps of tests/map_cases.py (its docstring: what each is for)
reach what that map cannot: full scans (use_index = 0, with and without mixed-cell records), band scans
(use_cells = 0), long candidate lists, 32 rings, nested / overlapping / clockwise rings, negative coordinates,
a zero-length edge, and images beyond the one-wave kernel's 80 KB budget and beyond a CU's 160 KB of LDS, which
change the kernel launch_steps picks and where that kernel reads the map.

Probe parity (sit_probe_map on a 64-env handle, both precisions, every map).  map_info() is asserted against
the builder's recorded flags first, so a builder change that stops a map from reaching its path fails here.
Points, seeded, about 40 000 per map: uniform over the extent grown by 3000 m (inside the class grid, between
its 100 m margin and the candidate grid's 0.1 max(extent) + 500 m, beyond both); per edge a band of offsets
log-uniform from 1e-9 m to 80 m on both sides, the vertex, the midpoint, rays along the vertex latitude and
hull corners landing on the vertex; points on and one ulp (float64 and float32) either side of every line of
the candidate grid, the class grid and the bands, the outermost lines included, recomputed here from the
extent with build_map_image's formulas; points in and around every ring.
  float64: containment and the hull test identical to the oracle everywhere, distance within 1e-12 relative
           (floor 1 m).
  float32: the oracle evaluates the float32-rounded points in float64, on the rings as a float32 handle holds
           them (sit_load_map rounds the vertices to float32: the same rings for the whole-metre maps,
           rings up to 2.4e-4 m off for gon256, whose vertices are no float32 numbers -- against the
           unrounded rings its distances differ by that much, 1.9 times the bound below, before any
           arithmetic); containment and the hull test identical everywhere; distance within 1e-5 max(d, 10 m) + 16 * 2^-24 (l + d), l the map's longest
           edge.  The second term models the segment branch's cross product qy ex - qx ey in float32: about
           five half-ulp roundings of magnitude |q| |e| <= (l + d) l, divided by |e| = l, with 16 as the
           allowance over that count.  The worst error-to-bound ratio per map is printed.

Step kernels on comb_v, comb_h, comb_h64 and squares32 (128 envs of make_scenario with the map's rings): a
float64 synthetic rollout of 300 steps in launches of 100 and then 20 one-step launches against the oracle
(next_state, reward, action within 1e-9; done, status, done_count identical; the final state), with the kernel
name of each kind of launch asserted against launch_steps' dispatch.  Both ships must end episodes on terrain
in 0.5 % to 50 % of the oracle's rows, so the terrain decisions are exercised.  float32 (comb_h, comb_v): one
teacher-forced step from float32-rounded states of a 512-env float64 rollout at depths 150 and 300; continuous
outputs within 1e-5, waypoint bookkeeping identical, done / status mismatches only in rows whose oracle
post-step position (either ship's centre or a hull corner) lies within 1e-3 m of a boundary, those rows being
at most 0.5 % of all rows.
"""
import functools

import numpy as np
import pytest
import torch

import map_cases as mc
from helpers import OBS_SCALE, SCALE, rel_err
from oracle import sit_oracle as so

pytestmark = pytest.mark.gpu

sit = pytest.importorskip("sac_maritime_ast_amd")
from sac_maritime_ast_amd import VecMultiShipRLEnv, make_scenario  # noqa: E402
from sac_maritime_ast_amd.scenario import Scenario  # noqa: E402

DEV = "cuda:0"
TOL64 = 1e-9
SEED = 25450


def scenario(name, n_env):
    sc = make_scenario(n_env, cap=32)
    return Scenario(sc.routes, sc.n_wpt, sc.init, list(mc.load(name)))


def assert_map_info(env, name):
    want = mc.expected(name, 4 if env.precision == 32 else 8)
    info = env.map_info()
    got = {"use_index": info["use_index"], "use_cells": info["use_cells"], "n_mixed": info["mixed_cells"],
           "n_live": info["live_edges"], "map_bytes": info["map_bytes"]}
    assert got == {k: want[k] for k in got}, f"{name}: the builder no longer makes the image this test needs"


@functools.lru_cache(maxsize=None)
def oracle_at(name, precision):
    """The oracle's (distance, contains, hull) at the map's probe points, points and rings as a handle of that
    precision holds them, and the longest edge of those rings."""
    pts, polys = mc.probe_points(name), mc.load(name)
    if precision == 32:
        pts = pts.astype(np.float32).astype(np.float64)
        polys = tuple(r.astype(np.float32).astype(np.float64) for r in polys)
    return (*mc.oracle_predicates(polys, pts), mc.longest_edge(polys))


# ------------------------------------------------------------------------------------------
# probe parity on every map
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", mc.MAPS)
def test_map_predicates_on_every_index_path(name, precision):
    env = VecMultiShipRLEnv(scenario=scenario(name, 64), precision=precision, device=DEV)
    assert_map_info(env, name)
    pts = mc.probe_points(name)
    if precision == 32:
        pts = pts.astype(np.float32)
    dist, inside, hull = (x.cpu().numpy() for x in env.probe_map(torch.from_numpy(pts)))
    d_ref, in_ref, hull_ref, longest = oracle_at(name, precision)
    p = pts.astype(np.float64)
    err = np.abs(dist.astype(np.float64) - d_ref)
    if precision == 64:
        bound = 1e-12 * np.maximum(d_ref, 1.0)
    else:
        bound = 1e-5 * np.maximum(d_ref, 10.0) + 16 * 2.0 ** -24 * (longest + d_ref)
    ratio = err / bound
    w = int(np.argmax(ratio))
    print(f"{name} float{precision}: {len(p)} points, inside {int(in_ref.sum())}, hull {int(hull_ref.sum())}, "
          f"worst distance error / bound {ratio[w]:.3f} at {p[w].tolist()} (d = {d_ref[w]:.6g})")
    assert ratio[w] <= 1.0, f"distance {dist[w]!r} vs {d_ref[w]!r} at {p[w].tolist()}: {ratio[w]:.3f} of the bound"
    bad = np.nonzero(inside != in_ref)[0]
    assert bad.size == 0, f"{bad.size} contains mismatches, e.g. {p[bad[:5]].tolist()}"
    bad = np.nonzero(hull != hull_ref)[0]
    assert bad.size == 0, f"{bad.size} hull mismatches, e.g. {p[bad[:5]].tolist()}"


# ------------------------------------------------------------------------------------------
# step kernels on the maps that change the dispatch
# ------------------------------------------------------------------------------------------
N_ENV, FUSED, CHUNK, SINGLE = 128, 300, 100, 20
# launch_steps' choice per map for a fused launch (100 steps) and a one-step launch (sit_host.h):
#   comb_v     no packed index: sync_launch_lds refuses, the one-wave kernel; 28 KB staged into LDS when the
#              launch has >= 8 steps
#   comb_h     49 KB: the two-wave kernel with the map in LDS
#   comb_h64   262 KB > a CU's 160 KB: a fused launch falls back to the one-wave kernel, whose 80 KB budget it
#              exceeds too (map=global); a one-step launch stages nothing, so the two-wave kernel takes it
#   squares32  84 KB: within the two-wave kernel's LDS, beyond the one-wave kernel's budget
KERNELS = {
    "comb_v": (("k_env_steps<", "map=LDS"), ("k_env_steps<", "map=global")),
    "comb_h": (("k_env_steps_sync<", "map=LDS"), ("k_env_steps_sync<", "map=global")),
    "comb_h64": (("k_env_steps<", "map=global"), ("k_env_steps_sync<", "map=global")),
    "squares32": (("k_env_steps_sync<", "map=LDS"), ("k_env_steps_sync<", "map=global")),
}


@functools.lru_cache(maxsize=None)
def oracle_rollout(name):
    """The oracle's 300 + 20 steps on a map: the outputs per launch and the states after the fused part and at
    the end.  Computed once per map; nothing changes it afterwards."""
    sc = scenario(name, N_ENV)
    o = so.OracleEnvs(dict(so.DEFAULT_PARAMS), sc.routes, sc.n_wpt, sc.init, sc.polys)
    o.reset()
    o.init_step()
    fused = [o.rollout(CHUNK, seed=SEED) for _ in range(FUSED // CHUNK)]
    mid = {k: np.copy(v) for k, v in o.get_state().items()}
    single = [o.rollout(1, seed=SEED) for _ in range(SINGLE)]
    end = {k: np.copy(v) for k, v in o.get_state().items()}
    return fused, mid, single, end


def np_state(env):
    return {k: v.cpu().numpy() for k, v in env.get_state().items()}


def check_state(got, want, tol, where):
    for k in so.SHIP_INT + ("ep_step", "event", "episodes"):
        assert np.array_equal(got[k].astype(np.int64), np.asarray(want[k]).astype(np.int64)), f"{where}: {k}"
    for k in so.SHIP_REAL:
        err = rel_err(got[k], want[k], SCALE[k]).max()
        assert err <= tol, f"{where}: {k} rel err {err:.3e}"


def check_launch(out, r, where):
    assert rel_err(out["next_state"].cpu().numpy(), r["next_state"], OBS_SCALE).max() <= TOL64, where
    assert rel_err(out["reward"].cpu().numpy(), r["reward"], 1.0).max() <= TOL64, where
    assert np.array_equal(out["done"].cpu().numpy().astype(bool), r["done"]), where
    assert np.array_equal(out["status"].cpu().numpy().astype(np.int64) & 0xFFFFFFFF, r["status"].astype(np.int64)), where
    act = out["action"].cpu().numpy()
    assert np.array_equal(np.isnan(act[..., 2]), np.isnan(r["action"][..., 2])), where
    assert rel_err(act[..., :2], r["action"][..., :2], 1e4).max() <= TOL64, where
    assert np.array_equal(out["done_count"].cpu().numpy(), r["done"].sum(axis=1)), where


def kernel_name(env):
    return env.lib.sit_step_kernel(env.handle).decode()


def assert_kernel(env, want, where):
    name = kernel_name(env)
    assert name.startswith(want[0]) and want[1] in name, f"{where}: launched {name}, expected {want}"


@pytest.mark.parametrize("name", mc.STEP_MAPS)
def test_oracle_rollout_ends_episodes_on_terrain(name):
    """No vacuous pass: on the oracle's output alone, each ship ends episodes on terrain in 0.5 % to 50 % of rows."""
    fused, _, single, _ = oracle_rollout(name)
    st = np.concatenate([r["status"] for r in fused + single]).astype(np.int64)
    for bit, ship in ((so.ST_TEST_TERRAIN, "test ship"), (so.ST_OBS_TERRAIN, "obstacle ship")):
        share = float(((st & bit) != 0).mean())
        print(f"{name}: {ship} terrain rows {int(((st & bit) != 0).sum())} of {st.size} ({100 * share:.2f} %)")
        assert 0.005 <= share <= 0.5, f"{name}: {ship} ends on terrain in {100 * share:.2f} % of rows"


def run_f64_rollout(name, kernels):
    fused, mid, single, end = oracle_rollout(name)
    env = VecMultiShipRLEnv(scenario=scenario(name, N_ENV), precision=64, device=DEV)
    assert_map_info(env, name)
    env.reset()
    env.init_step()
    for i, r in enumerate(fused):
        out = env.rollout(CHUNK, seed=SEED)
        assert_kernel(env, kernels[0], f"{name} fused launch")
        check_launch(out, r, f"{name} steps [{i * CHUNK},{(i + 1) * CHUNK})")
    check_state(np_state(env), mid, 1e-8, f"{name} state after {FUSED} steps")
    for i, r in enumerate(single):
        out = env.rollout(1, seed=SEED)
        assert_kernel(env, kernels[1], f"{name} one-step launch")
        check_launch(out, r, f"{name} single step {i}")
    check_state(np_state(env), end, 1e-8, f"{name} final state")


@pytest.mark.parametrize("name", mc.STEP_MAPS)
def test_f64_rollout_vs_oracle_on_dispatch_maps(name):
    run_f64_rollout(name, KERNELS[name])


def test_f64_rollout_vs_oracle_squares32_classic(monkeypatch):
    """The one-wave kernel on an image beyond its 80 KB budget: it reads the map from global memory."""
    monkeypatch.setenv("SIT_STEP_KERNEL", "classic")
    run_f64_rollout("squares32", (("k_env_steps<", "map=global"), ("k_env_steps<", "map=global")))


@pytest.mark.parametrize("name", ["comb_h", "comb_v"])
def test_f32_teacher_forced_vs_oracle_on_scan_maps(name):
    n_env = 512
    sc = scenario(name, n_env)
    polys = sc.polys
    env64 = VecMultiShipRLEnv(scenario=sc, precision=64, device=DEV)
    env64.reset()
    env64.init_step()
    env32 = VecMultiShipRLEnv(scenario=sc, precision=32, device=DEV)
    assert_map_info(env32, name)
    o = so.OracleEnvs(dict(so.DEFAULT_PARAMS), sc.routes, sc.n_wpt, sc.init, polys)
    worst, rows, near_rows, n_disc, stray = {}, 0, 0, 0, []
    for depth in (150, 300):
        env64.rollout(150, seed=SEED)
        st = np_state(env64)
        st32 = {k: (v.astype(np.float32).astype(np.float64) if v.dtype == np.float64 else v) for k, v in st.items()}
        o.set_state(st32)
        env32.set_state(st32)
        rng = np.random.default_rng(depth)
        sac = rng.random(n_env) < 0.1
        ang = rng.uniform(-np.pi / 6, np.pi / 6, n_env)
        act = np.stack([st32["north"][1] + o.ab_len * np.cos(o.ab_alpha + ang),
                        st32["east"][1] + o.ab_len * np.sin(o.ab_alpha + ang)], 1)
        act = act.astype(np.float32).astype(np.float64)
        init = np.zeros(n_env, bool)
        ns_r, rew_r, done_r, st_r = o.step(act, sac, init)
        # the oracle's own decision margin: either ship's centre or a hull corner within 1e-3 m of a boundary
        near = np.minimum(mc.corner_margin(polys, ns_r[:, 0], ns_r[:, 1]),
                          mc.corner_margin(polys, ns_r[:, 6], ns_r[:, 7])) < 1e-3
        ns, rew, done, stat = (x.cpu().numpy() for x in env32.step(act, sac, init))
        disc = (done != done_r) | (stat != st_r)
        stray += [(depth, int(i)) for i in np.nonzero(disc & ~near)[0]]
        rows, near_rows, n_disc = rows + n_env, near_rows + int(near.sum()), n_disc + int(disc.sum())
        same = ~disc               # a row that decided otherwise (allowed only near a boundary) also ends otherwise
        for key, e in (("next_state", rel_err(ns, ns_r, OBS_SCALE)), ("reward", rel_err(rew, rew_r, 1.0))):
            worst[key] = max(worst.get(key, 0), e[same].max())
        post, ref = np_state(env32), o.get_state()
        for k in so.SHIP_REAL:
            worst[k] = max(worst.get(k, 0), rel_err(post[k], ref[k], SCALE[k])[:, same].max())
        for k in ("next_wpt", "n_wpt", "stop"):
            assert np.array_equal(post[k], ref[k]), f"depth {depth}: {k}"
    print(f"{name} f32 teacher-forced worst:", {k: f"{v:.2e}" for k, v in worst.items()},
          f"rows within 1e-3 m of a boundary: {near_rows} of {rows}, discrete mismatches: {n_disc}")
    assert near_rows <= 0.005 * rows, f"{near_rows} of {rows} oracle rows within 1e-3 m of a boundary"
    assert not stray, f"done/status mismatches away from every boundary, (depth, env): {stray[:5]}"
    for k, v in worst.items():
        assert v <= 1e-5, f"{k}: {v:.3e}"
