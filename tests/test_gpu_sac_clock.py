"""The SAC learner's device clock on the GPU: ``SacLearner.update_many`` / sit_sac_updates against the same number
of ``update_parameters`` calls, bit for bit (include/sit.h "many updates per call from a device clock").

Every comparison is ``torch.equal`` on the learner's whole state: the three packed blocks (padding included, which
is how skipping the padding in the fused Polyak update is checked), the six moment blocks, log_alpha with its
moments, alpha, the result rows against the returned tuples and the memory's cursor.  The ring is
sac_cases.device_memory (256 records), batches are at most 67; the twin learner has a twin memory.

1. sit_sac_adam_scalars against sac.adam_scalars_reference: the device's double divide and sqrt are the
   correctly rounded ones.  2. Equality in the three modes at B = 9 (a partial block of 8 and of 32) and 67
   (several blocks, a ragged last one).  3. Polyak gating.  4. Untuned temperature.  5. A captured graph (a
   baked-in step count or update number fails here).  6. The results ring.  7. Mixing the two paths and
   checkpoints.  8. Rejections.  9. Rollout, push and updates as one graph.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sit = pytest.importorskip("sac_maritime_ast_amd")
from sac_maritime_ast_amd import ReplayMemory, VecMultiShipRLEnv, _lib, make_scenario, sac  # noqa: E402
from sac_maritime_ast_amd.samplers import GaussianPolicy, PolicySampler  # noqa: E402
from sac_cases import (ADAM_EPS, AW, BETA1, BETA2, CANARY, CW, DEV, ROW, SEED, bits, blocks_are_the_modules, device_memory,  # noqa: E402
                       learner_err, learner_params, new_learner, reference_run)

MODES = {"sum/valu": dict(weight_gradient="sum", row_pass="valu"), "mfma/valu": dict(weight_gradient="mfma", row_pass="valu"),
         "mfma/mfma": dict(weight_gradient="mfma", row_pass="mfma")}
BIG_STEPS = [355, 1000, 37400, 10 ** 6, 2 ** 40]
MARGIN = 4.0                             # of tests/test_gpu_sac_grad.py::test_checkpoints_cross_the_gradient_modes


@pytest.fixture(scope="module", params=[32, 64])
def env(request):
    e = VecMultiShipRLEnv(scenario=make_scenario(64), precision=request.param, device=DEV)
    yield e
    e.close()


def hip_learner(env, fresh=False, **kw):
    return new_learner(env, fresh=fresh, gradient="hip", **kw)


def twin_run(env, batch, updates, **kw):
    """The reference of every comparison: one update_parameters call per update number on a twin learner."""
    learner, mem = hip_learner(env, **kw), device_memory(env)
    return learner, mem, [learner.update_parameters(mem, batch, u) for u in updates]


def state_of(learner):
    out = {k: getattr(learner, k) for k in ("actor_weights", "online_weights", "target_weights", "log_alpha", "alpha")}
    for k in ("policy", "critic", "alpha"):
        out["m_" + k], out["v_" + k] = learner._m[k], learner._v[k]
    return out


def assert_same_state(a, b, mem_a=None, mem_b=None):
    torch.cuda.synchronize()
    sa, sb = state_of(a), state_of(b)
    differ = [k for k in sa if not torch.equal(sa[k].detach(), sb[k].detach())]
    assert not differ, differ
    if mem_a is not None:
        assert torch.equal(mem_a.cursor, mem_b.cursor), (mem_a.cursor.tolist(), mem_b.cursor.tolist())


def clock_words(learner):
    return learner.clock[:5].tolist()


# ---------------------------------------------------------------------------------------------
# 1. the scalars
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lr,beta1,beta2", [(3e-4, BETA1, BETA2), (1e-3, 0.5, 0.99)])
def test_device_scalars_are_the_reference_bits(env, lr, beta1, beta2):
    o = _lib.SacAdam(lr, beta1, beta2, ADAM_EPS, 0.0, 0.0)
    runs = [(1, 4096)] + [(t, 1) for t in BIG_STEPS]
    for t0, n in runs:
        out = torch.full((n * 6 + 8,), CANARY, dtype=torch.float32, device=DEV)
        with torch.cuda.device(env.device):
            env._call("sit_sac_adam_scalars", ctypes.byref(o), t0, n, out.data_ptr(), env._stream())
        torch.cuda.synchronize()
        assert torch.all(out[-8:] == CANARY)
        got = out[:-8].cpu().numpy().reshape(n, 6)
        want = sac.adam_scalars_reference(lr, beta1, beta2, ADAM_EPS, np.arange(t0, t0 + n, dtype=np.int64))
        differ = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
        assert differ.size == 0, (t0, differ[:5], got[differ[:2]], want[differ[:2]])


# ---------------------------------------------------------------------------------------------
# 2.-4. equality with update_parameters
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [9, 67])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_update_many_equals_update_parameters(env, mode, batch):
    twin, tmem, tuples = twin_run(env, batch, range(5), **MODES[mode])
    learner, mem = hip_learner(env, **MODES[mode]), device_memory(env)
    assert learner.update_many(mem, batch, 5, first_update=0) is None
    assert_same_state(learner, twin, mem, tmem)
    assert learner.results() == tuples
    assert blocks_are_the_modules(learner)
    assert clock_words(learner) == [5, 5, 5, 5, 5]
    assert not torch.equal(learner.target_weights, hip_learner(env).target_weights)


def test_polyak_gating(env):
    kw = dict(target_update_interval=3)
    twin, tmem, tuples = twin_run(env, 9, range(1, 8), **kw)
    learner, mem = hip_learner(env, **kw), device_memory(env)
    learner.update_many(mem, 9, 7, first_update=1)
    assert_same_state(learner, twin, mem, tmem)
    assert learner.results() == tuples
    assert clock_words(learner) == [8, 7, 7, 7, 7]
    every, emem = hip_learner(env), device_memory(env)
    every.update_many(emem, 9, 7, first_update=1)
    torch.cuda.synchronize()
    assert not torch.equal(every.target_weights, learner.target_weights)


def test_untuned_temperature(env):
    kw = dict(automatic_entropy_tuning=False)
    twin, tmem, tuples = twin_run(env, 9, range(5), **kw)
    learner, mem = hip_learner(env, **kw), device_memory(env)
    alpha, log_alpha = learner.alpha.clone(), learner.log_alpha.detach().clone()
    learner.update_many(mem, 9, 5, first_update=0)
    assert_same_state(learner, twin, mem, tmem)
    assert torch.equal(learner.alpha, alpha) and torch.equal(learner.log_alpha.detach(), log_alpha)
    assert clock_words(learner) == [5, 5, 5, 0, 5]
    rows = learner.results()
    assert rows == tuples and all(r[3] == 0.0 and r[4] == float(alpha[0]) for r in rows)


# ---------------------------------------------------------------------------------------------
# 5. a captured graph
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sum/valu", "mfma/mfma"])
def test_graph_replays_continue_the_clock(env, mode):
    twin, tmem, tuples = twin_run(env, 64, range(12), **MODES[mode])
    learner, mem = hip_learner(env, **MODES[mode]), device_memory(env)
    learner.update_many(mem, 64, 3, first_update=0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        learner.update_many(mem, 64, 3)
    for _ in range(3):
        graph.replay()
    assert_same_state(learner, twin, mem, tmem)
    assert clock_words(learner) == [12, 12, 12, 12, 12]
    assert learner.results() == tuples
    sd = learner.state_dict()                       # (the host's counts follow the replays)
    assert {int(s["step"]) for k in ("critic", "policy", "alpha") for s in sd["optims"][k]["state"].values()} == {12}


# ---------------------------------------------------------------------------------------------
# 6. the results ring
# ---------------------------------------------------------------------------------------------
def test_results_ring_wraps(env):
    twin, tmem, tuples = twin_run(env, 9, range(6))
    learner, mem = hip_learner(env, results_capacity=4), device_memory(env)
    assert learner.results() == []
    learner.update_many(mem, 9, 6, first_update=0)
    assert learner.results() == tuples[2:]
    assert learner.results(last=2) == tuples[4:]
    assert learner.results(last=100) == tuples[2:] and learner.results(last=0) == []
    assert clock_words(learner)[4] == 6


# ---------------------------------------------------------------------------------------------
# 7. mixing the paths, checkpoints
# ---------------------------------------------------------------------------------------------
def test_mixed_paths_and_checkpoints(env):
    B, n_more = 64, 2
    twin, tmem, tuples = twin_run(env, B, range(8))
    a, mem = hip_learner(env), device_memory(env)
    got = [a.update_parameters(mem, B, u) for u in range(2)]
    a.update_many(mem, B, 3)                                    # continues at update 2
    got += a.results()
    sd, msd = a.state_dict(), mem.state_dict()
    for k in ("critic", "policy", "alpha"):
        assert {int(s["step"]) for s in sd["optims"][k]["state"].values()} == {5}, k
    assert a._steps == {"critic": 5, "policy": 5, "alpha": 5}
    b = hip_learner(env, fresh=True)
    b.load_state_dict(sd)
    assert clock_words(b)[1:4] == [5, 5, 5]
    got.append(b.update_parameters(mem, B, 5))
    b.update_many(mem, B, 2)                                    # continues at update 6
    got += b.results()
    assert_same_state(b, twin, mem, tmem)
    assert got == tuples
    assert clock_words(b) == [8, 8, 8, 8, 2]
    assert b.state_dict()["optims"]["critic"]["state"][0]["step"] == 8

    # the same checkpoint continues in gradient="torch" within the margin of test_checkpoints_cross_the_gradient_modes
    ref_t, _, ref_p = reference_run(env.precision, B, 5, n_more)
    straight, smem = new_learner(env, gradient="torch"), device_memory(env)
    stuples = [straight.update_parameters(smem, B, u) for u in range(5 + n_more)]
    base = learner_err(stuples[5:], learner_params(straight), ref_t[5:], ref_p)
    other = new_learner(env, fresh=True, gradient="torch")
    other.load_state_dict(sd)
    mem.load_state_dict(msd)
    otuples = [other.update_parameters(mem, B, u) for u in range(5, 5 + n_more)]
    err = learner_err(otuples, learner_params(other), ref_t[5:], ref_p)
    print(f"sac clocked checkpoint, f{env.precision}, hip (mixed paths) -> torch:", {k: f"{v:.2e}" for k, v in err.items()},
          "torch straight through:", {k: f"{v:.2e}" for k, v in base.items()})
    bad = {k: (v, base[k]) for k, v in err.items() if v > MARGIN * base[k]}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------
# 8. rejections
# ---------------------------------------------------------------------------------------------
def canaried_updates_args(env, B=9, U=2, cap=4):
    dt = env.dtype
    buf = lambda n, d=torch.float32: torch.full((n + 8,), CANARY, dtype=d, device=DEV)  # noqa: E731
    bufs = {"critic_weights": buf(2 * CW), "critic_m": buf(2 * CW), "critic_v": buf(2 * CW), "actor_weights": buf(AW),
            "actor_m": buf(AW), "actor_v": buf(AW), "target_weights": buf(2 * CW), "alpha": buf(1), "log_alpha": buf(1),
            "log_alpha_m": buf(1), "log_alpha_v": buf(1), "state": buf(U * B * 10, dt), "action": buf(U * B, dt),
            "reward": buf(U * B, dt), "next_state": buf(U * B * 10, dt), "mask": buf(U * B, dt), "y": buf(B, dt),
            "workspace": buf(2 * B * ROW), "results": buf(cap * 5),
            "clock": torch.full((_lib.SIT_SAC_CLOCK_WORDS + 8,), -12345, dtype=torch.int64, device=DEV)}
    a = _lib.SacUpdatesArgs()
    a.mode, a.batch, a.n_updates, a.tune, a.seed = _lib.SIT_SAC_UPDATES_PLAIN, B, U, 1, SEED
    a.gamma, a.reward_scale, a.target_entropy, a.tau = 0.99, 1.0, -1.0, 0.005
    a.target_update_interval, a.workspace_floats, a.results_capacity = 1, 2 * B * ROW, cap
    a.critic_adam = a.actor_adam = a.alpha_adam = _lib.SacAdam(3e-4, BETA1, BETA2, ADAM_EPS, 1.0, 1.0)
    for k, t in bufs.items():
        setattr(a, k, t.data_ptr())
    return a, bufs


def test_invalid_arguments_launch_nothing(env):
    a, bufs = canaried_updates_args(env)
    good = {k: getattr(a, k) for k, _ in a._fields_ if not k.endswith("_adam")}
    cases = [(k, None) for k in ("critic_weights", "actor_m", "target_weights", "state", "mask", "y", "workspace", "clock",
                                 "results", "log_alpha")]
    cases += [("critic_weights", good["critic_weights"] + 4), ("actor_v", good["actor_v"] + 8),
              ("target_weights", good["target_weights"] + 12), ("clock", good["clock"] + 4),
              ("n_updates", 0), ("n_updates", -1), ("batch", 0), ("results_capacity", 0), ("results_capacity", -3),
              ("target_update_interval", 0), ("workspace_floats", good["workspace_floats"] - 1), ("mode", 3)]
    for field, value in cases:
        setattr(a, field, value)
        with torch.cuda.device(env.device):
            rc = env.lib.sit_sac_updates(env.handle, ctypes.byref(a), env._stream())
        setattr(a, field, good[field])
        assert rc == _lib.SIT_E_INVALID, (field, value)
        assert env.lib.sit_last_error(env.handle).decode().startswith("sac: "), field
    o = _lib.SacAdam(3e-4, BETA1, BETA2, ADAM_EPS, 0.0, 0.0)
    out = bufs["results"]
    for t0, n, ptr in ((0, 1, out.data_ptr()), (1, 0, out.data_ptr()), (1, 1, None)):
        with torch.cuda.device(env.device):
            assert env.lib.sit_sac_adam_scalars(env.handle, ctypes.byref(o), t0, n, ptr, env._stream()) == _lib.SIT_E_INVALID
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert torch.all(t == (-12345 if k == "clock" else CANARY)), f"{k}: written by a rejected call"


def test_update_many_rejections_touch_nothing(env):
    torch_mode = new_learner(env, gradient="torch")
    with pytest.raises(ValueError, match="gradient='hip'"):
        torch_mode.update_many(device_memory(env), 9, 2)
    learner, mem = hip_learner(env), device_memory(env)
    before = {k: v.detach().clone() for k, v in state_of(learner).items()}
    clock, cursor = learner.clock.clone(), mem.cursor.clone()

    def untouched():
        torch.cuda.synchronize()
        return (all(torch.equal(v.detach(), before[k]) for k, v in state_of(learner).items())
                and torch.equal(learner.clock, clock) and torch.equal(mem.cursor, cursor))
    for batch in (256, 300):                                    # len(memory) <= batch_size
        with pytest.raises(ValueError, match="more than batch_size"):
            learner.update_many(mem, batch, 2, first_update=0)
    with pytest.raises(ValueError):
        learner.update_many(mem, 9, 0)
    assert untouched()
    # under capture: a missing buffer (no eager call with this (batch, n) yet), then a given first_update; both
    # raise before anything is enqueued, so the graph holds the one good call behind them and nothing else
    twin, tmem, tuples = twin_run(env, 9, range(4))
    learner.update_many(mem, 9, 2, first_update=0)
    torch.cuda.synchronize()
    raised = []
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for kw in (dict(n_updates=3), dict(n_updates=2, first_update=4)):
            try:
                learner.update_many(mem, 9, **kw)
            except ValueError as e:
                raised.append(str(e))
        learner.update_many(mem, 9, 2)
    assert len(raised) == 2 and "eagerly" in raised[0] and "first_update" in raised[1], raised
    graph.replay()
    assert_same_state(learner, twin, mem, tmem)
    assert learner.results() == tuples and clock_words(learner) == [4, 4, 4, 4, 4]


# ---------------------------------------------------------------------------------------------
# 9. rollout, push and updates as one graph
# ---------------------------------------------------------------------------------------------
def loop_parts():
    e = VecMultiShipRLEnv(scenario=make_scenario(64), precision=32, device=DEV)
    e.reset()
    e.init_step()
    torch.manual_seed(4)
    pol = GaussianPolicy().to(DEV)
    with torch.no_grad():
        pol.net[0].weight.mul_(1e-3)             # raw observations: keep the actions inside (-1, 1)
    sampler = PolicySampler(e, pol, chunk=750, seed=SEED, transition_capacity=4096)
    learner = sac.SacLearner(e, pol, seed=SEED, gradient="hip")
    mem = ReplayMemory(e, 8192, seed=SEED)
    for _ in range(4):
        mem.push(sampler.launch())
    return e, sampler, learner, mem


def test_the_loop_as_one_graph():
    """launch, push, two updates: once eagerly, then captured and replayed three times with share_weights, against
    the same four iterations run eagerly with update_parameters on twins."""
    e, sampler, learner, mem = loop_parts()
    te, tsampler, twin, tmem = loop_parts()
    try:
        assert len(mem) > 64
        for i in range(4):
            tmem.push(tsampler.launch())
            for u in (2 * i, 2 * i + 1):
                twin.update_parameters(tmem, 64, u)
        sampler.share_weights(learner.actor_weights)
        assert sampler._w is learner.actor_weights and sampler.io["actor_weights"] is learner.actor_weights
        sampler.refresh_weights()                               # a no-op now

        def iteration():
            mem.push(sampler.launch())
            learner.update_many(mem, 64, 2)
        iteration()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            iteration()
        for _ in range(3):
            graph.replay()
        assert_same_state(learner, twin, mem, tmem)
        assert torch.equal(mem.ring, tmem.ring)
        assert torch.equal(sampler.served, tsampler.served) and int(sampler.served.item()) > 0
        assert clock_words(learner) == [8, 8, 8, 8, 8]
    finally:
        e.close()
        te.close()
