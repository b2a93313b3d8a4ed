"""GPU checks of the device-side episode reducer (sit_episodes_*, episodes.EpisodeLog) against
episodes_reference, the executable specification; for the real rollout also against the CPU oracle."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import sit_oracle as so  # noqa: E402
from sac_maritime_ast_amd import VecMultiShipRLEnv, _lib, make_scenario  # noqa: E402
from sac_maritime_ast_amd.episodes import EpisodeLog, columns, episodes_reference  # noqa: E402
from sac_maritime_ast_amd.samplers import IntermediateWaypointSampler  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_ENV, K = 300, 97            # four full waves + 44 lanes: two blocks of 256 threads
SPLITS = {"whole": (97,), "1+96": (1, 96), "40+40+17": (40, 40, 17), "singles": (1,) * 97}
NP_REAL = {32: np.float32, 64: np.float64}


@functools.lru_cache(maxsize=None)
def synthetic_rows(precision):
    """Rows [K, N_ENV] with rewards +-10^U(-3, 3) (summation order is visible), ~5 % done rows, ~20 %
    SIT_ST_NO_STEP rows carrying reward NaN and a random done flag, and the forced cases:
    env 0 never done, env 1 done on every row, env 2 done on the last row of every split of SPLITS
    with more than one row, env 3 with 20 events inside one episode."""
    rng = np.random.default_rng(20240607)
    real = NP_REAL[precision]
    reward = (rng.choice([-1.0, 1.0], (K, N_ENV)) * 10.0 ** rng.uniform(-3, 3, (K, N_ENV)))
    done = rng.random((K, N_ENV)) < 0.05
    status = rng.integers(0, 1 << 14, (K, N_ENV)).astype(np.int64)
    status |= (rng.random((K, N_ENV)) < 0.1).astype(np.int64) << 31          # SIT_ST_ROUTE_OVERFLOW: uint32 range
    skip = rng.random((K, N_ENV)) < 0.2
    event = rng.random((K, N_ENV)) < 0.04
    skip[:, 1] = False
    done[:, 1] = True
    done[:, 0] = False
    for k in (0, 39, 79, 96):
        skip[k, 2], done[k, 2] = False, True
    skip[:70, 3], done[:70, 3], event[:70, 3] = False, False, False
    event[5:65:3, 3] = True                                                  # 20 events
    skip[70, 3], done[70, 3] = False, True
    done = np.where(skip, rng.random((K, N_ENV)) < 0.5, done)
    done[:, 0] &= skip[:, 0]                                                 # env 0: done only on skipped rows
    reward[skip] = np.nan
    status = np.where(skip, status | _lib.ST_NO_STEP, status)
    action = rng.uniform(-1e4, 1e4, (K, N_ENV, 4))
    action[..., 2] = np.where(event, rng.uniform(-0.55, 0.55, (K, N_ENV)), np.nan)
    action[..., 3] = event
    next_state = rng.uniform(-1e4, 1e4, (K, N_ENV, _lib.SIT_OBS_DIM))
    assert event[:, 3].sum() == 20 and not (done[:, 0] & ~skip[:, 0]).any()
    return dict(reward=reward.astype(real), done=done.astype(np.uint8), status=status.astype(np.uint32).view(np.int32),
                action=action.astype(real), next_state=next_state.astype(real))


@functools.lru_cache(maxsize=None)
def synthetic_reference(precision, with_action=True, with_next_state=True):
    r = synthetic_rows(precision)
    rec, hist, _ = episodes_reference(r["reward"], r["done"], r["status"], r["action"] if with_action else None,
                                      r["next_state"] if with_next_state else None)
    rec.setflags(write=False)
    hist.setflags(write=False)
    return rec, hist


@functools.lru_cache(maxsize=None)
def small_env(precision):
    return VecMultiShipRLEnv(scenario=make_scenario(N_ENV, cap=8), precision=precision, device=DEV)


@functools.lru_cache(maxsize=None)
def device_rows(precision):
    return {k: torch.as_tensor(v, device=DEV) for k, v in synthetic_rows(precision).items()}


def feed(log, rows, split, with_action=True, with_next_state=True, start=0):
    k0 = start
    for m in split:
        part = {k: v[k0:k0 + m] for k, v in rows.items()}
        log.update(reward=part["reward"], done=part["done"], status=part["status"],
                   action=part["action"] if with_action else None,
                   next_state=part["next_state"] if with_next_state else None)
        k0 += m
    return k0


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def by_env_episode(rec):
    return rec[np.lexsort((rec[:, 1], rec[:, 0]))]


# 1. synthetic rows, both precisions: every column, the order, hist and count equal the reference
@pytest.mark.parametrize("precision", [32, 64])
def test_synthetic_rows_match_reference(precision):
    ref, ref_hist = synthetic_reference(precision)
    assert len(ref) > 400 and (ref[:, 5] == 20).any() and (ref[ref[:, 0] == 1][:, 2] == 1).all()
    assert not (ref[:, 0] == 0).any()
    log = EpisodeLog(small_env(precision), capacity=2048)
    feed(log, device_rows(precision), SPLITS["whole"])
    torch.cuda.synchronize()
    assert int(log.count.item()) == len(ref)
    hist = log.hist.cpu().numpy()
    got = log.drain()
    assert got["dropped"] == 0 and int(log.count.item()) == 0
    assert same(got["records"], ref)
    assert np.array_equal(hist, ref_hist)
    assert np.array_equal(got["steps"], ref[:, 2].astype(np.int64)) and same(got["angles"], ref[:, 18:])
    counts = log.status_counts()
    assert sum(counts.values()) == ref_hist.sum()


# 2. partition invariance: one update, 1+96, 40+40+17 and 97 single-row updates give the same records
@pytest.mark.parametrize("precision", [32, 64])
def test_partition_invariance(precision):
    ref, ref_hist = synthetic_reference(precision)
    want = by_env_episode(ref)
    for name, split in SPLITS.items():
        log = EpisodeLog(small_env(precision), capacity=2048)
        feed(log, device_rows(precision), split)
        hist = log.hist.cpu().numpy()
        got = log.drain()
        assert got["dropped"] == 0, name
        assert same(by_env_episode(got["records"]), want), name         # column 6 (row index) included
        assert np.array_equal(hist, ref_hist), name


# 3. capacity: the written records are the first of the specified order; count and hist cover all
def test_capacity_drops_but_counts():
    ref, ref_hist = synthetic_reference(32)
    rows = device_rows(32)
    log = EpisodeLog(small_env(32), capacity=10)
    feed(log, rows, (40,))
    ref40, hist40, carry = episodes_reference(*(synthetic_rows(32)[k][:40] for k in ("reward", "done", "status", "action",
                                                                                   "next_state")))
    assert len(ref40) > 10
    torch.cuda.synchronize()
    assert same(log.records.cpu().numpy(), ref40[:10])
    assert int(log.count.item()) == len(ref40) and np.array_equal(log.hist.cpu().numpy(), hist40)
    feed(log, rows, (57,), start=40)                                         # appends nothing, keeps counting
    torch.cuda.synchronize()
    assert same(log.records.cpu().numpy(), ref40[:10])
    assert int(log.count.item()) == len(ref) and np.array_equal(log.hist.cpu().numpy(), ref_hist)
    got = log.drain()
    assert got["dropped"] == len(ref) - 10 and same(got["records"], ref40[:10])
    none = EpisodeLog(small_env(32), capacity=0)                             # records = NULL, capacity = 0
    feed(none, rows, SPLITS["whole"])
    torch.cuda.synchronize()
    assert int(none.count.item()) == len(ref) and np.array_equal(none.hist.cpu().numpy(), ref_hist)
    assert none.drain()["records"].shape == (0, _lib.SIT_EPISODE_DIM)


# 4. optional inputs: NaN columns, nothing else changes
def test_optional_inputs():
    full, full_hist = synthetic_reference(64)
    for with_action, with_ns in ((False, True), (True, False), (False, False)):
        ref, ref_hist = synthetic_reference(64, with_action, with_ns)
        log = EpisodeLog(small_env(64), capacity=2048)
        feed(log, device_rows(64), SPLITS["40+40+17"], with_action, with_ns)
        got = by_env_episode(log.drain()["records"])                         # (three updates: sorted as one)
        assert same(got, ref)
        if not with_action:
            assert np.isnan(got[:, 18:]).all() and (got[:, 5] == 0).all()
        if not with_ns:
            assert np.isnan(got[:, 8:18]).all()
        keep = [0, 1, 2, 3, 4, 6, 7] + ([5] + list(range(18, 32)) if with_action else []) + \
            (list(range(8, 18)) if with_ns else [])
        assert same(got[:, keep], full[:, keep])
        assert np.array_equal(log.hist.cpu().numpy(), full_hist)


# 5. checkpoint: state() after 40 rows, load_state into a fresh env's log, feed the rest
@pytest.mark.parametrize("precision", [32, 64])
def test_checkpoint_resume(precision):
    ref, _ = synthetic_reference(precision)
    rows = device_rows(precision)
    log = EpisodeLog(small_env(precision), capacity=2048)
    feed(log, rows, (40,))
    blob = log.state().clone()
    first = log.drain()["records"]
    fresh = VecMultiShipRLEnv(scenario=make_scenario(N_ENV, cap=8), precision=precision, device=DEV)
    log2 = EpisodeLog(fresh, capacity=2048)
    log2.load_state(blob)
    feed(log2, rows, (40, 17), start=40)
    rest = log2.drain()["records"]
    assert len(first) and len(rest)
    assert same(by_env_episode(np.concatenate([first, rest])), by_env_episode(ref))
    fresh.close()


# 6. real rollout: make_scenario(128), 4 launches x 100 steps, seed 25450
LAUNCHES, CHUNK, SEED, N_REAL = 4, 100, 25450, 128
ROW_KEYS = ("reward", "done", "status", "action", "next_state")


def started_env(precision):
    env = VecMultiShipRLEnv(scenario=make_scenario(N_REAL), precision=precision, device=DEV)
    env.reset()
    env.init_step()
    return env


@functools.lru_cache(maxsize=None)
def real_rollout(precision, chunk=CHUNK, launches=LAUNCHES):
    """(records the GPU reduced, hist, the GPU's own rows on the host) of an eager run."""
    env = started_env(precision)
    log = EpisodeLog(env, capacity=256)
    rows = {k: [] for k in ROW_KEYS}
    for _ in range(launches):
        out = env.rollout(chunk, seed=SEED)
        log.update(out)
        for k in ROW_KEYS:
            rows[k].append(out[k].cpu().numpy())
    hist = log.hist.cpu().numpy()
    rec = log.drain()["records"]
    env.close()
    rec.setflags(write=False)
    return rec, hist, {k: np.concatenate(v) for k, v in rows.items()}


@pytest.mark.parametrize("precision", [64, 32])
def test_real_rollout_vs_own_rows(precision):
    rec, hist, rows = real_rollout(precision)
    ref, ref_hist, _ = episodes_reference(rows["reward"], rows["done"], rows["status"], rows["action"], rows["next_state"])
    assert len(rec) >= 20
    assert same(by_env_episode(rec), ref)
    assert np.array_equal(hist, ref_hist)
    # within one update the records are in (env, episode) order
    for a in range(LAUNCHES):
        part = rec[(rec[:, 6] >= a * CHUNK) & (rec[:, 6] < (a + 1) * CHUNK)]
        assert same(part, by_env_episode(part))


def test_real_rollout_vs_oracle():
    rec, hist, _ = real_rollout(64)
    sc = make_scenario(N_REAL)
    o = so.OracleEnvs(dict(so.DEFAULT_PARAMS), sc.routes, sc.n_wpt, sc.init, sc.polys)
    o.reset()
    o.init_step()
    r = o.rollout(LAUNCHES * CHUNK, seed=SEED)
    ref, ref_hist, _ = episodes_reference(r["reward"], r["done"], r["status"], r["action"], r["next_state"])
    assert len(ref) >= 20
    c = columns(ref)
    assert c["env"][0] == 0 and c["row"][0] == 0 and c["steps"][0] == 1         # env 0 ends at row 0, then episode 1
    got = by_env_episode(rec)
    g = columns(got)
    for k in ("env", "episode", "steps", "status", "events", "row"):
        assert np.array_equal(g[k], c[k]), k
    assert np.array_equal(hist, ref_hist)
    rew = np.abs(r["reward"])
    for i in range(len(ref)):
        e, last, steps = int(c["env"][i]), int(c["row"][i]), int(c["steps"][i])
        bound = 1e-9 * np.maximum(rew[last - steps + 1:last + 1, e], 1.0).sum()
        assert abs(g["ret"][i] - c["ret"][i]) <= bound, (i, g["ret"][i], c["ret"][i], bound)


# 7. graph capture: rollout(50) + update in one HIP graph, replayed four times
def test_graph_capture_matches_eager():
    eager, eager_hist, _ = real_rollout(32, 50, 4)
    assert len(eager) >= 1
    env = started_env(32)
    log = EpisodeLog(env, capacity=256)
    out = env.rollout(50, seed=SEED, want=ROW_KEYS)                           # eager warm-up: every buffer exists
    log.update(out)
    env.restart()
    env.reset()
    env.init_step()
    log.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        env.rollout(50, seed=SEED, want=ROW_KEYS, out=out)
        log.update(out)
    env.restart()
    env.reset()
    env.init_step()
    log.reset()
    for _ in range(4):
        graph.replay()
    hist = log.hist.cpu().numpy()
    got = log.drain()["records"]
    assert same(got, eager) and np.array_equal(hist, eager_hist)
    env.close()


# 8. sampler wiring
def test_sampler_owns_episode_log():
    rec, hist, _ = real_rollout(32)
    env = started_env(32)
    sm = IntermediateWaypointSampler(env, chunk=CHUNK, seed=SEED, episode_capacity=256)
    for _ in range(LAUNCHES):
        out = sm.launch()
    assert same(sm.episodes.drain()["records"], rec)
    assert np.array_equal(sm.episodes.hist.cpu().numpy(), hist)
    plain = IntermediateWaypointSampler(env, chunk=CHUNK, seed=SEED)
    assert plain.episodes is None
    assert set(plain.launch()) == set(out) == {"next_state", "reward", "done", "status", "action", "done_count"}
    env.close()


# 8b. policy mode: rows of waiting envs (SIT_ST_NO_STEP) from a real producer; the update inside the graph
def policy_sampler_records(graph):
    from sac_maritime_ast_amd.samplers import GaussianPolicy, PolicySampler
    env = started_env(32)
    torch.manual_seed(5)
    pol = GaussianPolicy(hidden=(256, 256))
    with torch.no_grad():
        pol.net[0].weight.mul_(1e-3)
    sm = PolicySampler(env, pol.to(dtype=torch.float32, device=DEV), chunk=40, seed=SEED, episode_capacity=256)
    rows = {k: [] for k in ROW_KEYS}
    if graph:
        sm.capture(2, want=("reward",))                                       # two eager launches, two recorded
        for _ in range(5):
            sm.replay()
    else:
        for _ in range(12):
            out = sm.launch(want=("reward",))                                 # the log adds the rows it needs
            for k in rows:
                if k in out:
                    rows[k].append(out[k].cpu().numpy())
    hist = sm.episodes.hist.cpu().numpy()
    rec = sm.episodes.drain()["records"]
    env.close()
    return rec, hist, {k: np.concatenate(v) for k, v in rows.items() if v}


def test_policy_sampler_episode_log_eager_and_graph():
    rec, hist, rows = policy_sampler_records(graph=False)
    assert set(rows) == {"reward", "done", "status", "action"}
    assert (rows["status"] & _lib.ST_NO_STEP).any() and len(rec) >= 1
    ref, ref_hist, _ = episodes_reference(rows["reward"], rows["done"], rows["status"], rows["action"])
    assert same(by_env_episode(rec), ref) and np.array_equal(hist, ref_hist)
    assert np.isnan(rec[:, 8:18]).all()                                       # no next_state rows were asked for
    grec, ghist, _ = policy_sampler_records(graph=True)
    assert same(grec, rec) and np.array_equal(ghist, hist)


# 9. argument errors
def test_argument_errors():
    env = small_env(32)
    log = EpisodeLog(env, capacity=16)
    rows = device_rows(32)

    def args(**over):
        a = _lib.EpisodesArgs()
        a.n_steps, a.record_capacity = K, log.capacity
        a.reward, a.done, a.status = rows["reward"].data_ptr(), rows["done"].data_ptr(), rows["status"].data_ptr()
        a.records, a.record_count = log.records.data_ptr(), log.count.data_ptr()
        for k, v in over.items():
            setattr(a, k, v)
        return a

    for over, word in (({"done": None}, "done"), ({"n_steps": 0}, "n_steps"), ({"record_capacity": -1}, "record_capacity"),
                       ({"records": None}, "records"), ({"record_count": None}, "record_count")):
        with pytest.raises(_lib.SitError, match=rf"sit error {_lib.SIT_E_INVALID}: .*{word}"):
            env._call("sit_episodes_update", ctypes.byref(args(**over)), env._stream())
    with pytest.raises(ValueError, match="reward"):
        log.update(reward=rows["reward"].double(), done=rows["done"], status=rows["status"])
    with pytest.raises(ValueError, match="status"):
        log.update(reward=rows["reward"], done=rows["done"], status=rows["status"][:, :-1].contiguous())
    torch.cuda.synchronize()
    assert int(log.count.item()) == 0
