"""GPU checks of the observation normalisation (include/sit.h: sit_obsnorm_*, sit_replay_sample_normalised;
sac_maritime_ast_amd/obsnorm.py), on both handles.

1. update: block and affine against ObsNormReference bit for bit (sizes across the chunk and group boundaries of
   the summation tree, the wrap / skip / max_new sequences, a checkpoint round trip).  2. normalize and the
   normalised gather, with canaries behind every output.  3. fold.  4. Serving: the actor kernel on the folded
   block and raw rows against the float64 policy on float64-normalised rows, bounded by
   (1 + max |shift| scale) * 4 * e_base with e_base the same kernel on the master block and reference-normalised
   rows (both printed).  5. The learner with a frozen affine against the learner on a pre-normalised ring (bits)
   and against the float64 reference (the tolerance of tests/test_gpu_sac.py).  6. The iteration as one graph.
7. Argument errors."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sit = pytest.importorskip("sac_maritime_ast_amd")
from sac_maritime_ast_amd import (ObsNormalizer, ObsNormReference, ReplayMemory, Scoreboard, VecMultiShipRLEnv, _lib,  # noqa: E402
                                  make_scenario, replay_reference, sac)
from sac_maritime_ast_amd.samplers import GaussianPolicy, LOG_SIG_CAP_MAX, LOG_SIG_CAP_MIN, PolicySampler  # noqa: E402
import obsnorm_cases as C  # noqa: E402
from helpers import OBS_SCALE  # noqa: E402
import sac_cases as S  # noqa: E402
from sac_cases import DEV, dev  # noqa: E402

AW, OBS = _lib.SIT_ACTOR_WEIGHTS, _lib.SIT_OBS_DIM
SEED = 25450
CANARY = -12345.5
# tests/test_gpu_sac.py: the learner's error against the float64 reference after 3 updates of batch 64, and its margin
LEARNER_TORCH_ERR = {"tuple": 1.14e-07, "params": 1.64e-07}
LEARNER_MARGIN = 4.0


@pytest.fixture(scope="module", params=[32, 64])
def env(request):
    e = VecMultiShipRLEnv(scenario=make_scenario(64), precision=request.param, device=DEV)
    yield e
    e.close()


def mirror(env, ref_mem, mem=None):
    """A ReplayMemory holding the reference memory's ring and cursor."""
    mem = ReplayMemory(env, ref_mem.capacity, seed=ref_mem.seed) if mem is None else mem
    mem.ring.copy_(dev(ref_mem.ring))
    mem.cursor.copy_(dev(ref_mem.cursor))
    return mem


def same_state(norm, ref):
    torch.cuda.synchronize()
    block, affine = norm.block.cpu().numpy(), norm.affine.cpu().numpy()
    return (np.array_equal(C.bits(block), C.bits(ref.block)) and np.array_equal(C.bits(affine), C.bits(ref.affine)),
            (block[:4], ref.block[:4], affine[:26], ref.affine[:26]))


def with_tail(shape, dtype, fill=None):
    """A contiguous device tensor of `shape` with 8 canary elements behind it in the same allocation: (view, flat)."""
    n = int(np.prod(shape))
    flat = torch.full((n + 8,), CANARY if dtype.is_floating_point else -12345, dtype=dtype, device=DEV)
    view = flat[:n].view(shape)
    if fill is not None:
        view.copy_(dev(fill, dtype))
    return view, flat


def tails_intact(flats):
    torch.cuda.synchronize()
    return all(torch.all(f[-8:] == (CANARY if f.dtype.is_floating_point else -12345)) for f in flats)


# ---------------------------------------------------------------------------------------------
# 1. update
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [0, 1, 255, 256, 257, 65536, 65537])
def test_update_bit_for_bit(env, m):
    rec = C.rows(max(m, 1), 100 + m)
    ref_mem = C.memory(rec, m + 3, m, env.precision)
    mem = mirror(env, ref_mem)
    ring_before = mem.ring.clone()
    ref, norm = ObsNormReference(), ObsNormalizer(env)
    ref.update(ref_mem)
    norm.update(mem)
    ok, shown = same_state(norm, ref)
    assert ok, shown
    out = norm.read()
    assert (out["n"], out["updates"], out["seen"], out["skipped"]) == (m, 1, m, 0)
    assert torch.equal(mem.ring.view(torch.uint8), ring_before.view(torch.uint8))
    assert mem.cursor.tolist() == [m, 0, 0, 0]


@pytest.mark.parametrize("name", sorted(C.SEQUENCES))
def test_sequences_bit_for_bit_and_checkpoint(env, name):
    capacity, max_new, pushes = C.SEQUENCES[name]
    rec = C.rows(max(pushes), 5)
    ref_mem = replay_reference(capacity, C.NP_REAL[env.precision])
    mem = ReplayMemory(env, capacity)
    ref, norm, loaded = ObsNormReference(), ObsNormalizer(env), None
    norm.reserve(capacity)
    for i, pushed in enumerate(pushes):
        mirror(env, C.fill(ref_mem, rec, pushed), mem)
        ref.update(ref_mem, max_new)
        norm.update(mem, max_new)
        ok, shown = same_state(norm, ref)
        assert ok, (i, shown)
        if loaded is not None:
            loaded.update(mem, max_new)
            ok, shown = same_state(loaded, ref)
            assert ok, ("loaded", i, shown)
        if i == 0:                                   # a fresh normaliser continues from the checkpoint
            loaded = ObsNormalizer(env, min_std=7.0)
            loaded.load_state_dict(norm.state_dict())
    out = norm.read()
    want = {"wrap_and_skip": (750, 1200, 450), "max_new": (250, 250, 0), "nothing_new": (120, 120, 0)}[name]
    assert (out["n"], out["seen"], out["skipped"]) == want and out["updates"] == len(pushes)


# ---------------------------------------------------------------------------------------------
# 2. normalize and the normalised gather
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted(env):
    """(ObsNormalizer, ObsNormReference) after one update over 500 synthetic records."""
    ref_mem = C.memory(C.rows(500, 2), 500, 500, env.precision)
    ref, norm = ObsNormReference(), ObsNormalizer(env)
    ref.update(ref_mem)
    norm.update(mirror(env, ref_mem))
    ok, shown = same_state(norm, ref)
    assert ok, shown
    return norm, ref


@pytest.mark.parametrize("n", [1, 7, 64])
def test_normalize_equals_the_reference(env, fitted, n):
    norm, ref = fitted
    dt = C.NP_REAL[env.precision]
    rows = C.rows(2 * n, 40 + n)
    host_x, host_y = rows[:n, :OBS].astype(dt), rows[n:, :OBS].astype(dt)
    host_x[0, 3] = np.nan
    x, fx = with_tail((n, OBS), env.dtype, host_x)
    y, fy = with_tail((n, OBS), env.dtype, host_y)
    one, f1 = with_tail((n, OBS), env.dtype, host_x)
    assert norm.normalize(x, y) == (x, y) and norm.normalize(one) is one
    assert tails_intact([fx, fy, f1])
    want_x, want_y = ref.apply(host_x.copy(), host_y.copy())
    assert np.array_equal(C.bits(x.cpu().numpy()), C.bits(want_x)) and np.array_equal(C.bits(y.cpu().numpy()), C.bits(want_y))
    assert np.array_equal(C.bits(one.cpu().numpy()), C.bits(want_x)) and np.isnan(want_x[0, 3])


@pytest.mark.parametrize("B,U", [(1, 1), (7, 3), (64, 8)])
def test_normalised_sample_equals_sample_then_normalize(env, fitted, B, U):
    norm, ref = fitted
    rec = C.rows(300, 6)
    ref_mem = C.memory(rec, 300, 300, env.precision)
    ref_mem.cursor[2] = 11
    a, b = mirror(env, ref_mem), mirror(env, ref_mem)
    shapes = {"state": (U, B, OBS), "action": (U, B, 1), "reward": (U, B), "next_state": (U, B, OBS), "mask": (U, B)}
    outs, flats = [], []
    for _ in range(2):
        views = {k: with_tail(s, env.dtype) for k, s in shapes.items()}
        views.update({k: with_tail((U, B), torch.int32) for k in ("env", "index")})
        outs.append({k: v[0] for k, v in views.items()})
        flats += [v[1] for v in views.values()]
    got = a.sample(B, U, out=outs[0], normalizer=norm)
    want = b.sample(B, U, out=outs[1])
    norm.normalize(want["state"], want["next_state"])
    assert tails_intact(flats)
    spec = ref_mem.sample(B, U, normalizer=ref)
    for k in shapes.keys() | {"env", "index"}:
        assert got[k] is outs[0][k] and got[k].data_ptr() == outs[0][k].data_ptr(), k
        g = got[k].cpu().numpy()
        assert np.array_equal(C.bits(g), C.bits(want[k].cpu().numpy())), k
        assert np.array_equal(C.bits(g), C.bits(spec[k])), k
    assert a.cursor.tolist() == b.cursor.tolist() == [300, 0, 11 + U, 0]
    assert torch.equal(a.ring.view(torch.uint8), b.ring.view(torch.uint8))          # the ring keeps raw observations
    assert float(got["state"].abs().max()) < 4 and float(got["index"].min()) >= 0


def test_normalised_sample_from_an_empty_ring(env, fitted):
    norm, ref = fitted
    got = ReplayMemory(env, 16).sample(3, 2, normalizer=norm)
    want = replay_reference(16, C.NP_REAL[env.precision]).sample(3, 2, normalizer=ref)
    torch.cuda.synchronize()
    for k, v in want.items():
        assert np.array_equal(C.bits(got[k].cpu().numpy()), C.bits(v)), k


# ---------------------------------------------------------------------------------------------
# 3. fold
# ---------------------------------------------------------------------------------------------
def test_fold_equals_the_reference(env, fitted):
    norm, ref = fitted
    block = C.default_actor()
    src = dev(block)
    dst, flat = with_tail((AW,), torch.float32)
    assert norm.fold(src, dst) is dst
    assert tails_intact([flat])
    assert np.array_equal(C.bits(dst.cpu().numpy()), C.bits(ref.fold(block)))
    assert np.array_equal(C.bits(src.cpu().numpy()), C.bits(block))
    ident = ObsNormalizer(env)
    dst.fill_(CANARY)
    ident.fold(src, dst)
    torch.cuda.synchronize()
    assert torch.equal(dst.view(torch.int32), src.view(torch.int32))
    with pytest.raises(ValueError, match="overlap"):
        norm.fold(src, src)
    with torch.cuda.device(env.device):
        rc = env.lib.sit_obsnorm_fold(env.handle, norm.affine.data_ptr(), src.data_ptr(), src.data_ptr(), env._stream())
    assert rc == _lib.SIT_E_INVALID and b"must not overlap" in env.lib.sit_last_error(env.handle)


# ---------------------------------------------------------------------------------------------
# 4. serving
# ---------------------------------------------------------------------------------------------
def actor_kernel(env, block, obs, noise, deterministic):
    """sit_policy_actor on rows obs [n, 10], n_env rows per call with request_env = 0..: the n actions as float64."""
    out = []
    for r0 in range(0, len(obs), env.n_env):
        o, z = obs[r0:r0 + env.n_env], noise[r0:r0 + env.n_env]
        n = len(o)
        t = {"obs": dev(o, env.dtype), "noise": dev(z, env.dtype), "rows": torch.arange(n, dtype=torch.int32, device=DEV),
             "count": torch.tensor([n], dtype=torch.int32, device=DEV), "action": torch.zeros(n, dtype=env.dtype, device=DEV),
             "ready": torch.zeros(n, dtype=torch.int32, device=DEV)}
        with torch.cuda.device(env.device):
            env._call("sit_policy_actor", n, block.data_ptr(), t["obs"].data_ptr(), t["noise"].data_ptr(), t["rows"].data_ptr(),
                      t["count"].data_ptr(), int(deterministic), t["action"].data_ptr(), t["ready"].data_ptr(), None, None,
                      env._stream())
        torch.cuda.synchronize()
        assert torch.all(t["ready"] == 1)
        out.append(t["action"].double().cpu().numpy())
    return np.concatenate(out)


@pytest.mark.parametrize("deterministic", [True, False])
def test_folded_block_serves_the_normalised_policy(env, fitted, deterministic):
    obs = S.records()[:, :OBS]
    assert len(obs) >= 256
    ref = C.own_statistics(obs)
    norm = ObsNormalizer(env)
    norm.load_state_dict({"block": dev(ref.block), "affine": dev(ref.affine)})
    block = C.default_actor()
    noise = np.random.default_rng(3).normal(size=len(obs)).astype(np.float32).astype(np.float64)
    head = C.head(block, ref.normalized(obs, np.float64), np.float64)
    x = head[:, 0] if deterministic else head[:, 0] + np.exp(np.clip(head[:, 1], LOG_SIG_CAP_MIN, LOG_SIG_CAP_MAX)) * noise
    want = np.tanh(x)
    master = dev(block)
    serving = norm.fold(master, torch.empty_like(master))
    e_base = np.abs(actor_kernel(env, master, ref.normalized(obs.astype(C.NP_REAL[env.precision])), noise, deterministic)
                    - want).max()
    e_fold = np.abs(actor_kernel(env, serving, obs, noise, deterministic) - want).max()
    factor = C.fold_factor(ref)
    print(f"serving, f{env.precision}, deterministic={deterministic}: e_base {e_base:.3e} e_fold {e_fold:.3e} "
          f"factor {factor:.2f} bound {factor * 4 * e_base:.3e}")
    assert e_base > 0 and np.abs(want).max() < 1
    assert e_fold <= factor * 4 * e_base


# ---------------------------------------------------------------------------------------------
# 5. the learner
# ---------------------------------------------------------------------------------------------
N_REC, BATCH, N_UPD = 256, 64, 3


def raw_ring(precision):
    """The 256 records of sac_cases, raw, in a reference memory."""
    rec = S.records()[:N_REC].astype(C.NP_REAL[precision])
    ring = replay_reference(N_REC, C.NP_REAL[precision], seed=SEED)
    ring.push(rec, N_REC)
    return ring


def learner_blocks(learner):
    b = {"actor": learner.actor_weights, "critic": learner.online_weights, "target": learner.target_weights,
         "log_alpha": learner.log_alpha.detach(), "alpha": learner.alpha}
    for k in ("policy", "critic", "alpha"):
        b["m_" + k], b["v_" + k] = learner._m[k], learner._v[k]
    return {k: v.clone() for k, v in b.items()}


def test_learner_with_a_frozen_affine_equals_the_learner_on_a_normalised_ring(env):
    norm, ref = ObsNormalizer.from_bounds(env), ObsNormReference.from_bounds()
    assert np.array_equal(C.bits(norm.affine.cpu().numpy()), C.bits(ref.affine))
    raw = raw_ring(env.precision)
    pre = raw_ring(env.precision)
    ref.apply(pre.ring[:, 0:OBS], pre.ring[:, OBS + 2:2 * OBS + 2])
    assert np.abs(pre.ring[:, 0:OBS]).max() < 2 < np.abs(raw.ring[:, 0:OBS]).max()
    with_norm, plain = S.new_learner(env, gradient="hip", obs_norm=norm), S.new_learner(env, gradient="hip")
    with pytest.raises(ValueError, match="obs_norm"):
        plain.serving_weights
    assert np.array_equal(C.bits(with_norm.serving_weights.cpu().numpy()), C.bits(ref.fold(with_norm.actor_weights.cpu().numpy())))
    mem_raw, mem_pre = mirror(env, raw), mirror(env, pre)
    got = [with_norm.update_parameters(mem_raw, BATCH, u) for u in range(N_UPD)]
    want = [plain.update_parameters(mem_pre, BATCH, u) for u in range(N_UPD)]
    assert got == want and all(np.isfinite(t).all() for t in got)
    a, b = learner_blocks(with_norm), learner_blocks(plain)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert not torch.equal(a["actor"], S.new_learner(env, gradient="hip").actor_weights)      # the updates moved it
    assert np.array_equal(C.bits(with_norm.serving_weights.cpu().numpy()), C.bits(ref.fold(a["actor"].cpu().numpy())))
    assert "obs_norm" not in with_norm.state_dict() and set(with_norm.state_dict()) == set(plain.state_dict())
    assert torch.equal(mem_raw.ring.view(torch.uint8), dev(raw.ring).view(torch.uint8))


def test_torch_gradient_learner_against_the_float64_reference(env):
    """The tolerance of tests/test_gpu_sac.py (4 x the float32 learner's own error, LEARNER_TORCH_ERR) was measured on
    the records divided by helpers.OBS_SCALE, so the frozen affine here is that regime's: shift 0, scale
    1 / OBS_SCALE, on the raw ring.  Measured on an MI355X: tuple 1.15e-07, params 1.73e-07 on either handle.
    (The figure belongs to the regime, not to the normaliser: with the box affine of the test above the learner is
    6.6e-07 (f32) and 9.6e-07 (f64) from the reference in the parameters, and just as far, 7.0e-07 and 9.6e-07,
    from a reference without a normaliser that is fed the very inputs the device sees, the ring pre-normalised in
    the handle's precision; the test above shows that those are the bits of the learner without a normaliser.)"""
    bounds = (-OBS_SCALE, OBS_SCALE)
    norm, ref = ObsNormalizer.from_bounds(env, *bounds), ObsNormReference.from_bounds(*bounds)
    assert not ref.shift.any() and np.array_equal(ref.scale, (1.0 / OBS_SCALE).astype(np.float32))
    pol, q = S.networks()
    spec = sac.sac_update_reference(pol, q, obs_norm=ref, **S.LEARNER_KW)
    ring = raw_ring(env.precision)
    ref_t = [spec.update_parameters(ring, BATCH, u) for u in range(N_UPD)]
    ref_p = [p.detach().numpy().copy() for m in (spec.policy, spec.critic, spec.target_critic) for p in m.parameters()]
    learner = S.new_learner(env, gradient="torch", obs_norm=norm)
    mem = mirror(env, raw_ring(env.precision))
    tuples = [learner.update_parameters(mem, BATCH, u) for u in range(N_UPD)]
    err = S.learner_err(tuples, S.learner_params(learner), ref_t, ref_p)
    print(f"sac learner with obs_norm, f{env.precision}, gradient=torch against float64:", {k: f"{v:.2e}" for k, v in err.items()})
    bad = {k: v for k, v in err.items() if v > LEARNER_MARGIN * LEARNER_TORCH_ERR[k]}
    assert not bad, bad
    assert np.array_equal(C.bits(learner.serving_weights.cpu().numpy()), C.bits(ref.fold(learner.actor_weights.cpu().numpy())))


# ---------------------------------------------------------------------------------------------
# 6. the iteration as one graph: launch, push, norm.update, board.update / keep, update_many
# ---------------------------------------------------------------------------------------------
REPLAYS = 3


def iteration_parts(precision):
    e = VecMultiShipRLEnv(scenario=make_scenario(256), precision=precision, device=DEV)
    e.reset()
    e.init_step()
    torch.manual_seed(4)
    pol = GaussianPolicy().to(DEV)
    norm = ObsNormalizer(e)
    learner = sac.SacLearner(e, pol, seed=SEED, gradient="hip", obs_norm=norm)
    sampler = PolicySampler(e, pol, chunk=40, seed=SEED, transition_capacity=4096, episode_capacity=512)
    sampler.share_weights(learner.serving_weights)
    mem = mirror(e, C.memory(C.rows(256, 77), 4096, 256, precision))     # the first update has its batch
    mem.reserve(4096)
    norm.reserve(4096)
    board = Scoreboard(e)
    board.reserve(512)
    kept = {k: torch.full((n,), CANARY, device=DEV) for k, n in (("actor", AW), ("serving", AW), ("affine", _lib.SIT_OBSNORM_AFFINE))}

    def iteration():
        mem.push(sampler.launch())
        norm.update(mem)
        board.update(sampler.episodes, consume=True)
        board.keep([(learner.actor_weights, kept["actor"]), (learner.serving_weights, kept["serving"]),
                    (norm.affine, kept["affine"])], stamp=learner.clock)
        learner.update_many(mem, 64, 2)

    def state():
        torch.cuda.synchronize()
        return {"block": norm.block, "affine": norm.affine, "actor": learner.actor_weights, "serving": learner.serving_weights,
                "critic": learner.online_weights, "target": learner.target_weights, "clock": learner.clock, "ring": mem.ring,
                "cursor": mem.cursor, "score": board.block, **{"kept_" + k: v for k, v in kept.items()}}
    return e, norm, learner, iteration, state


@pytest.mark.parametrize("precision", [32, 64])
def test_the_iteration_as_one_graph(precision):
    e, norm, learner, iteration, state = iteration_parts(precision)
    te, tnorm, tlearner, titeration, tstate = iteration_parts(precision)
    try:
        for _ in range(1 + REPLAYS):
            titeration()
        iteration()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            iteration()
        for _ in range(REPLAYS):
            graph.replay()
        got, want = state(), tstate()
        for k in want:
            assert torch.equal(got[k].view(torch.uint8), want[k].view(torch.uint8)), k
        out = norm.read()
        print(f"iteration graph, f{precision}:", {k: out[k] for k in ("n", "updates", "seen", "skipped")})
        assert out["updates"] == 1 + REPLAYS and out["n"] == out["seen"] > 256 and out["skipped"] == 0
        assert int(learner.clock[0]) == 2 * (1 + REPLAYS)
        ref = ObsNormReference()
        ref.load_state_dict({"block": norm.block.cpu().numpy(), "affine": norm.affine.cpu().numpy()})
        assert np.array_equal(C.bits(learner.serving_weights.cpu().numpy()), C.bits(ref.fold(learner.actor_weights.cpu().numpy())))
        assert not np.array_equal(out["scale"], np.ones(OBS, dtype=np.float32))
    finally:
        e.close()
        te.close()


# ---------------------------------------------------------------------------------------------
# 7. argument errors raise before anything is enqueued
# ---------------------------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing(env, fitted):
    norm, ref = fitted
    before = (norm.block.clone(), norm.affine.clone())
    other = torch.float64 if env.precision == 32 else torch.float32
    good = torch.zeros((4, OBS), dtype=env.dtype, device=DEV)
    with pytest.raises(ValueError, match="^x: dtype"):
        norm.normalize(torch.zeros((4, OBS), dtype=other, device=DEV))
    with pytest.raises(ValueError, match="^x: a tensor on"):
        norm.normalize(torch.zeros((4, OBS), dtype=env.dtype))
    with pytest.raises(ValueError, match="^x: a contiguous"):
        norm.normalize(torch.zeros((4, OBS + 1), dtype=env.dtype, device=DEV))
    with pytest.raises(ValueError, match="^y: 40 elements"):
        norm.normalize(good, torch.zeros((5, OBS), dtype=env.dtype, device=DEV))
    with pytest.raises(ValueError, match="^out: a contiguous float32"):
        norm.fold(torch.zeros(AW, device=DEV), torch.zeros(AW + 1, device=DEV))
    with pytest.raises(ValueError, match="^src_block: a tensor on"):
        norm.fold(torch.zeros(AW), torch.zeros(AW, device=DEV))
    with pytest.raises(ValueError, match="^memory:"):
        norm.update(replay_reference(16))
    mem = ReplayMemory(env, 16)
    with pytest.raises(ValueError, match="^max_new"):
        norm.update(mem, 0)
    with pytest.raises(ValueError, match="^max_new"):
        norm.reserve(0)
    with pytest.raises(ValueError, match="^normalizer"):
        mem.sample(4, normalizer=ref)
    frozen = ObsNormalizer.from_bounds(env)
    with pytest.raises(ValueError, match="fixed"):
        frozen.update(mem)
    with pytest.raises(ValueError, match="^obs_norm"):
        S.new_learner(env, obs_norm=ref)
    # the library refuses an update beyond the reserve, and says which argument
    a = _lib.ObsnormArgs()
    a.capacity, a.max_new = 16, 1 << 30
    a.ring, a.cursor, a.block, a.affine = mem.ring.data_ptr(), mem.cursor.data_ptr(), norm.block.data_ptr(), norm.affine.data_ptr()
    with torch.cuda.device(env.device):
        rc = env.lib.sit_obsnorm_update(env.handle, ctypes.byref(a), env._stream())
    assert rc == _lib.SIT_E_INVALID and b"max_new exceeds the reserve" in env.lib.sit_last_error(env.handle)
    torch.cuda.synchronize()
    assert torch.equal(norm.block, before[0]) and torch.equal(norm.affine, before[1]) and not good.any()
