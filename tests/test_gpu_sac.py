"""GPU checks of the SAC learner's HIP half (sit_sac_target / sit_sac_polyak, csrc/sit_sac.h) and of
SacLearner, against sac_target_reference (float64 NumPy) and sac_update_reference (float64 PyTorch on
the CPU), on float32 and float64 handles.

Error measure, for every output: |got - ref| / max(1, |ref|).

Inputs: the transition records of one float64 rollout of 64 envs (synthetic sampler), pushed through a
ReplayMemory (so their order is the canonical one), rounded to float32 so that both handles and the
reference see the same numbers.  Networks: default torch initialisation under a fixed seed.

Bounds
  normalised regime (observations / helpers.OBS_SCALE): 1e-5, the project's float32 contract.
  raw regime (observations up to 1e4): float32 sums lose digits, so the bound is 4 x the error a float32
    CPU PyTorch evaluation of the same formulas makes on these inputs against float64 (RAW_F32_CPU_ERR,
    measured once, below); the factor 4 is for the different summation order of the split-K layer.
  saturation sweep: next_logp 1e-5, next_action 1e-6 (a float32 `1 - a * a` log term misses by two orders).
  learner: 4 x the error of SacLearner(target="torch") in float32 against the float64 reference after 3
    updates (LEARNER_TORCH_ERR, measured once, below).
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from helpers import OBS_SCALE

pytestmark = pytest.mark.gpu

sit = pytest.importorskip("sac_maritime_ast_amd")
from sac_maritime_ast_amd import ReplayMemory, VecMultiShipRLEnv, _lib, make_scenario, sac  # noqa: E402
from sac_maritime_ast_amd.samplers import GaussianPolicy, PolicySampler, pack_actor_weights  # noqa: E402
from sac_cases import (AW, CANARY, CW, DEV, GAMMA, LEARNER_KW, SEED, bits, dev, device_memory, learner_err,  # noqa: E402
                       learner_params, networks, new_learner, records, reference_run, scaled_err)

OUTPUTS = ("y", "next_action", "next_logp", "q1", "q2")
BATCHES = (1, 7, 8, 9, 64, 67)         # one partial block, one full, one row into the second, many, 8 blocks + 3 rows
NMAX = 67
TOL = 1e-5
# Raw regime: max |float32 CPU PyTorch - float64| / max(1, |float64|) per output over the 67 fixture rows
# (alpha 0.2, given noise): cpu_f32_error("raw") below, as test_target_raw_regime prints it.
# (next_action: 0 -- on raw observations this actor saturates, a' = +-1 exactly in both precisions.)  The device,
# for comparison: y 6.9e-7, next_action 0, next_logp 2.8e-6, q1 1.3e-6, q2 9.2e-7 on either handle.
RAW_F32_CPU_ERR = {"y": 7.047e-07, "next_action": 0.0, "next_logp": 4.274e-06, "q1": 9.947e-07, "q2": 1.017e-06}
RAW_MARGIN = 4.0
# Learner: max error of SacLearner(target="torch") (float32, on the device) against sac_update_reference
# after 3 updates of batch 64 on the 256 normalised records: the 5-tuples, and all parameters.
# (target="hip" measured the same two figures.)
LEARNER_TORCH_ERR = {"tuple": 1.14e-07, "params": 1.64e-07}
LEARNER_MARGIN = 4.0


@pytest.fixture(scope="module", params=[32, 64])
def env(request):
    e = VecMultiShipRLEnv(scenario=make_scenario(64), precision=request.param, device=DEV)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def inputs(regime):
    """next_state [67, 10], reward (odd rows negative), mask (every third row 0), noise of the fixture rows."""
    rec = records()[:NMAX]
    ns = rec[:, 12:22] / OBS_SCALE if regime == "normalised" else rec[:, 12:22]
    ns = ns.astype(np.float32).astype(np.float64)
    reward = rec[:, 11].copy()
    reward[1::2] = -1.5 - np.arange(NMAX)[1::2] / 64.0
    mask = np.ones(NMAX)
    mask[::3] = 0.0
    noise = np.random.default_rng(3).standard_normal(NMAX).astype(np.float32).astype(np.float64)
    assert np.abs(ns).max() > (1e3 if regime == "raw" else 0.1)
    return ns, reward, mask, noise


@functools.lru_cache(maxsize=None)
def reference(regime, alpha, drawn):
    pol, q = networks()
    ns, reward, mask, noise = inputs(regime)
    return sac.sac_target_reference(pack_actor_weights(pol), sac.pack_critic_weights(q), ns, reward, mask,
                                    alpha=float(np.float32(alpha)), gamma=GAMMA, noise=None if drawn else noise,
                                    seed=SEED, update=(3 << 32) | 5)


class Target:
    """One sit_sac_target call through ctypes on buffers with 8 canary elements behind each output."""

    def __init__(self, env, aw, cw, ns, reward, mask, alpha, noise=None, diag=True, reward_scale=1.0, seed=SEED,
                 update=(3 << 32) | 5):
        self.env, self.B = env, int(ns.shape[0])
        dt = env.dtype
        self.keep = [dev(aw, torch.float32), dev(cw, torch.float32), torch.tensor([alpha], dtype=torch.float32, device=DEV),
                     dev(ns, dt), dev(reward, dt), dev(mask, dt), None if noise is None else dev(noise, dt)]
        self.out = {k: torch.full((self.B + 8,), CANARY, dtype=dt, device=DEV) for k in (OUTPUTS if diag else ("y",))}
        a = self.args = _lib.SacTargetArgs()
        a.batch, a.seed, a.update, a.gamma, a.reward_scale = self.B, seed, update, GAMMA, reward_scale
        a.actor_weights, a.critic_weights, a.alpha, a.next_state, a.reward, a.mask = (t.data_ptr() for t in self.keep[:6])
        a.noise = None if noise is None else self.keep[6].data_ptr()
        for k, t in self.out.items():
            setattr(a, k, t.data_ptr())

    def call(self):
        with torch.cuda.device(self.env.device):
            return self.env.lib.sit_sac_target(self.env.handle, ctypes.byref(self.args), self.env._stream())

    def run(self):
        assert self.call() == _lib.SIT_OK, self.env.lib.sit_last_error(self.env.handle)
        torch.cuda.synchronize()
        got = {k: t.cpu().numpy() for k, t in self.out.items()}
        for k, v in got.items():
            assert np.all(v[self.B:] == CANARY), f"{k}: written past row {self.B}"
        return {k: v[:self.B] for k, v in got.items()}


def fixture_target(env, regime, B, alpha, drawn, **kw):
    pol, q = networks()
    ns, reward, mask, noise = inputs(regime)
    return Target(env, pack_actor_weights(pol).numpy(), sac.pack_critic_weights(q).numpy(), ns[:B], reward[:B], mask[:B],
                  alpha, None if drawn else noise[:B], **kw)


# ---------------------------------------------------------------------------------------------
# sit_sac_target against the specification
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
def test_target_normalised_regime(env, B):
    worst = {}
    for alpha in (0.0, 0.2):
        for drawn in (False, True):
            got = fixture_target(env, "normalised", B, alpha, drawn).run()
            ref = reference("normalised", alpha, drawn)
            for k in OUTPUTS:
                worst[k] = max(worst.get(k, 0.0), scaled_err(got[k], ref[k][:B]))
    print(f"sac target, normalised, f{env.precision}, B={B}:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert all(v <= TOL for v in worst.values()), worst


def test_target_inputs_cover_masks_and_negative_rewards():
    ns, reward, mask, noise = inputs("normalised")
    assert set(mask[:7]) == {0.0, 1.0} and (reward[:7] < 0).any() and (reward < 0).sum() >= 33
    ref = reference("normalised", 0.2, False)
    assert np.array_equal(ref["y"][mask == 0], reward[mask == 0])             # terminal rows: y = reward
    assert np.abs(ref["y"] - reference("normalised", 0.0, False)["y"])[mask == 1].min() > 1e-3    # alpha matters


def test_target_device_noise_is_the_specifications_draw(env):
    """a' = tanh(mu + sigma eps) with the drawn eps: recover eps from the diagnostics of a constant head
    (W3 = 0, b3 = (0, 0): x = eps) and compare with sac_noise, as the policy's event noise is compared."""
    aw = np.zeros(AW, dtype=np.float32)
    cw = np.zeros(2 * CW, dtype=np.float32)
    B, update = 67, (9 << 32) | 2
    zeros = np.zeros(B)
    t = Target(env, aw, cw, np.zeros((B, 10)), zeros, zeros, 0.0, None, seed=SEED + 1, update=update)
    got = t.run()
    eps = sac.sac_noise(SEED + 1, np.arange(B), update)
    # logp = -0.5 eps^2 - 0.5 log(2 pi) - log(1 - tanh(eps)^2 + 1e-6), a' = tanh(eps)
    assert scaled_err(got["next_action"], np.tanh(eps)) <= 1e-6
    want = -0.5 * eps ** 2 - 0.5 * math.log(2 * math.pi) - sac.log_one_minus_tanh_sq(eps)
    assert scaled_err(got["next_logp"], want) <= TOL
    assert np.abs(eps).max() > 2.0 and (eps < 0).any() and (eps > 0).any()


def cpu_f32_error(regime):
    """The error of a float32 CPU PyTorch evaluation of the formulas on the fixture inputs against float64
    (how RAW_F32_CPU_ERR was measured)."""
    pol, q = networks()
    f32 = lambda a: torch.from_numpy(np.asarray(a)).to(torch.float32)  # noqa: E731
    ns, reward, mask, noise = inputs(regime)
    got = sac.torch_target(pol, q, f32(ns), f32(reward), f32(mask), f32(noise), 0.2, GAMMA)
    ref = reference(regime, 0.2, False)
    return {k: scaled_err(got[k].numpy(), ref[k]) for k in OUTPUTS}


def test_target_raw_regime(env):
    print("float32 CPU PyTorch against float64, raw:", {k: f"{v:.3e}" for k, v in cpu_f32_error("raw").items()},
          "normalised:", {k: f"{v:.3e}" for k, v in cpu_f32_error("normalised").items()})
    got = fixture_target(env, "raw", NMAX, 0.2, False).run()
    ref = reference("raw", 0.2, False)
    err = {k: scaled_err(got[k], ref[k]) for k in OUTPUTS}
    print(f"sac target, raw, f{env.precision}:", {k: f"{v:.2e}" for k, v in err.items()},
          "bounds", {k: f"{RAW_MARGIN * v:.2e}" for k, v in RAW_F32_CPU_ERR.items()})
    bad = {k: v for k, v in err.items() if v > RAW_MARGIN * RAW_F32_CPU_ERR[k]}
    assert not bad, bad


@pytest.mark.parametrize("ls_raw", [-25.0, -20.0, 0.0, 2.0, 3.0])
def test_target_saturation_sweep(env, ls_raw):
    """An actor with W3 = 0 and b3 = (0, ls): the head's inputs are exact, x = exp(clip(ls)) eps sweeps
    [-12, 12] in 257 rows.  logp within 1e-5 and a' within 1e-6 of float64."""
    pol, q = networks()
    aw = pack_actor_weights(pol).numpy().copy()
    aw[-2 * 256 - 2:] = 0.0                       # W3 and b3
    aw[-1] = ls_raw
    cw = sac.pack_critic_weights(q).numpy()
    B = 257
    ls = min(max(ls_raw, -20.0), 2.0)
    eps = (np.linspace(-12.0, 12.0, B) / math.exp(ls)).astype(np.float32).astype(np.float64)
    ns = inputs("normalised")[0][np.arange(B) % NMAX]
    reward, mask = np.zeros(B), np.ones(B)
    got = Target(env, aw, cw, ns, reward, mask, 0.2, eps).run()
    ref = sac.sac_target_reference(aw, cw, ns, reward, mask, alpha=float(np.float32(0.2)), gamma=GAMMA, noise=eps)
    assert abs(ref["x"][0] + 12.0) < 1e-5 and abs(ref["x"][-1] - 12.0) < 1e-5
    e_logp, e_act = scaled_err(got["next_logp"], ref["next_logp"]), scaled_err(got["next_action"], ref["next_action"])
    print(f"sac saturation, f{env.precision}, ls={ls_raw}: logp {e_logp:.2e} action {e_act:.2e}")
    assert e_logp <= 1e-5 and e_act <= 1e-6
    # the cancelled form in float32 would miss the bound a hundredfold (0.06 absolute around |x| = 8)
    naive = -0.5 * eps ** 2 - ls - 0.5 * math.log(2 * math.pi) - np.log(1.0 - np.tanh(ref["x"]).astype(np.float32).astype(np.float64) ** 2 + 1e-6)
    if ls_raw == 0.0:
        assert scaled_err(naive, ref["next_logp"]) > 1e-3
    for k in ("y", "q1", "q2"):
        assert scaled_err(got[k], ref[k]) <= TOL, k


# ---------------------------------------------------------------------------------------------
# kernel properties
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drawn", [False, True])
def test_target_is_deterministic_and_rows_do_not_depend_on_the_batch(env, drawn):
    t = fixture_target(env, "raw", 67, 0.2, drawn)
    first, second = t.run(), t.run()
    small = fixture_target(env, "raw", 9, 0.2, drawn).run()
    for k in OUTPUTS:
        assert np.array_equal(bits(first[k]), bits(second[k])), k
        assert np.array_equal(bits(first[k][:9]), bits(small[k])), k


def test_target_null_diagnostics_and_reward_scale(env):
    full = fixture_target(env, "normalised", 9, 0.2, False).run()
    only_y = fixture_target(env, "normalised", 9, 0.2, False, diag=False).run()
    assert set(only_y) == {"y"} and np.array_equal(bits(full["y"]), bits(only_y["y"]))
    scaled = fixture_target(env, "normalised", 9, 0.2, False, diag=False, reward_scale=3.0).run()
    ns, reward, mask, noise = inputs("normalised")
    assert scaled_err(scaled["y"] - full["y"], 2.0 * reward[:9]) <= TOL


def test_target_rejects_invalid_arguments_without_a_launch(env):
    t = fixture_target(env, "normalised", 9, 0.2, False)
    good = {k: getattr(t.args, k) for k, _ in t.args._fields_}
    cases = [(k, None) for k in ("actor_weights", "critic_weights", "alpha", "next_state", "reward", "mask", "y")]
    cases += [("batch", 0), ("batch", -1), ("actor_weights", good["actor_weights"] + 4),
              ("critic_weights", good["critic_weights"] + 8)]
    for field, value in cases:
        setattr(t.args, field, value)
        assert t.call() == _lib.SIT_E_INVALID, field
        assert b"sac" in env.lib.sit_last_error(env.handle), field
        setattr(t.args, field, good[field])
    with torch.cuda.device(env.device):
        assert env.lib.sit_sac_target(env.handle, None, env._stream()) == _lib.SIT_E_INVALID
    torch.cuda.synchronize()
    for k, v in t.out.items():
        assert torch.all(v == CANARY), f"{k}: an invalid call wrote"
    t.run()                                          # and the restored arguments are accepted


# ---------------------------------------------------------------------------------------------
# sit_sac_polyak
# ---------------------------------------------------------------------------------------------
def polyak(env, target, online, n, tau):
    with torch.cuda.device(env.device):
        return env.lib.sit_sac_polyak(env.handle, ctypes.c_void_p(target.data_ptr() if target is not None else None),
                                      ctypes.c_void_p(online.data_ptr() if online is not None else None), n, tau,
                                      env._stream())


@pytest.mark.parametrize("tau", [0.0, 0.005, 1.0])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 2 * CW])
def test_polyak(env, n, tau):
    """t' = fma(tau, p - t, t) in float32 against t + tau (p - t) in float64 (tau as the float32 the call
    receives), within one float32 ulp at the largest value the formula forms, max(|t|, |p|, |p - t|): the
    difference p - t is rounded once (half an ulp of |p - t|, times tau <= 1) and the fma once (half an
    ulp of the result, which lies between t and p)."""
    rng = np.random.default_rng(n)
    t0 = rng.standard_normal(n + 8).astype(np.float32)
    p = rng.standard_normal(n + 8).astype(np.float32)
    t0[n:] = CANARY
    target, online = dev(t0), dev(p)
    assert polyak(env, target, online, n, tau) == _lib.SIT_OK
    torch.cuda.synchronize()
    got = target.cpu().numpy()
    assert np.all(got[n:] == CANARY) and np.array_equal(online.cpu().numpy(), p)
    t64, p64 = t0[:n].astype(np.float64), p[:n].astype(np.float64)
    want = t64 + float(np.float32(tau)) * (p64 - t64)
    ulp = np.spacing(np.maximum(np.maximum(np.abs(t0[:n]), np.abs(p[:n])), np.abs(p64 - t64).astype(np.float32)))
    assert np.all(np.abs(got[:n].astype(np.float64) - want) <= ulp.astype(np.float64))
    if tau == 0.0:
        assert np.array_equal(bits(got[:n]), bits(t0[:n]))
    if tau == 1.0:
        assert np.all(np.abs(got[:n].astype(np.float64) - p64) <= ulp.astype(np.float64))


def test_polyak_rejects_invalid_arguments(env):
    t, p = torch.full((16,), CANARY, device=DEV), torch.zeros(16, device=DEV)
    assert polyak(env, None, p, 4, 0.5) == _lib.SIT_E_INVALID
    assert polyak(env, t, None, 4, 0.5) == _lib.SIT_E_INVALID
    assert polyak(env, t, p, 0, 0.5) == _lib.SIT_E_INVALID and polyak(env, t, p, -4, 0.5) == _lib.SIT_E_INVALID
    assert polyak(env, t[1:], p, 4, 0.5) == _lib.SIT_E_INVALID and polyak(env, t, p[2:], 4, 0.5) == _lib.SIT_E_INVALID
    torch.cuda.synchronize()
    assert torch.all(t == CANARY)


# ---------------------------------------------------------------------------------------------
# SacLearner against sac_update_reference
# ---------------------------------------------------------------------------------------------
N_REC, BATCH, N_UPD = 256, 64, 3


def learner_run(env, target):
    learner, mem = new_learner(env, target=target), device_memory(env, N_REC)
    tuples = [learner.update_parameters(mem, BATCH, u) for u in range(N_UPD)]
    return learner, mem, tuples


def test_learner_matches_the_float64_reference(env):
    ref_t, ref_p, _ = reference_run(env.precision, BATCH, N_UPD)
    runs = {}
    for target in ("torch", "hip"):
        learner, mem, tuples = learner_run(env, target)
        runs[target] = (tuples, learner_params(learner))
        err = learner_err(tuples, runs[target][1], ref_t, ref_p)
        print(f"sac learner, f{env.precision}, target={target} against float64:", {k: f"{v:.2e}" for k, v in err.items()})
        if target == "hip":
            bad = {k: v for k, v in err.items() if v > LEARNER_MARGIN * LEARNER_TORCH_ERR[k]}
            assert not bad, bad
            assert torch.equal(learner.actor_weights, pack_actor_weights(learner.policy))
    err = learner_err(*runs["hip"], *runs["torch"])
    print(f"sac learner, f{env.precision}, hip against torch:", {k: f"{v:.2e}" for k, v in err.items()})
    bad = {k: v for k, v in err.items() if v > LEARNER_MARGIN * LEARNER_TORCH_ERR[k]}
    assert not bad, bad
    # the losses are losses of this problem, and alpha moved
    assert all(math.isfinite(v) for t in ref_t for v in t) and ref_t[-1][4] != ref_t[0][4]


@pytest.mark.parametrize("target", ["hip", "torch"])
def test_learner_state_dict_round_trip(env, target):
    learner, mem, _ = learner_run(env, target)
    sd, msd = learner.state_dict(), mem.state_dict()
    want = learner.update_parameters(mem, BATCH, N_UPD)
    torch.manual_seed(99)
    other = sac.SacLearner(env, GaussianPolicy().to(DEV), target=target, **LEARNER_KW)     # other initial values
    other.load_state_dict(sd)
    mem.load_state_dict(msd)
    got = other.update_parameters(mem, BATCH, N_UPD)
    assert got == want
    assert torch.equal(other.actor_weights, pack_actor_weights(other.policy))


def test_learner_waits_for_more_than_a_batch_and_rejects_other_architectures(env):
    learner, mem = new_learner(env), device_memory(env, N_REC)
    assert learner.update_parameters(mem, N_REC, 0) is None and int(mem.cursor[2]) == 0
    with pytest.raises(ValueError):
        sac.SacLearner(env, GaussianPolicy(hidden=(64, 64)).to(DEV), **LEARNER_KW)
    small = sac.SacLearner(env, GaussianPolicy(hidden=(64, 64)).to(DEV), critic=sac.QNetwork(hidden=64), target="torch",
                           **LEARNER_KW)
    out = small.update_parameters(mem, BATCH, 0)
    assert len(out) == 5 and all(math.isfinite(v) for v in out)


# ---------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------
def test_rollout_push_update_serve():
    """A float32 policy rollout of 64 envs and 4 launches into the replay memory, one update from it, and the
    refreshed actor block served by the next launch."""
    e = VecMultiShipRLEnv(scenario=make_scenario(64), precision=32, device=DEV)
    try:
        e.reset()
        e.init_step()
        torch.manual_seed(4)
        pol = GaussianPolicy().to(DEV)
        with torch.no_grad():
            pol.net[0].weight.mul_(1e-3)             # raw observations: keep the actions inside (-1, 1)
        sampler = PolicySampler(e, pol, chunk=750, seed=SEED, transition_capacity=4096)
        learner = sac.SacLearner(e, pol, seed=SEED)
        mem = ReplayMemory(e, 8192, seed=SEED)
        for _ in range(4):
            mem.push(sampler.launch())
        assert len(mem) > BATCH, len(mem)
        before = sampler._w.clone()
        out = learner.update_parameters(mem, BATCH, 0)
        assert len(out) == 5 and all(math.isfinite(v) for v in out), out
        assert torch.equal(before, sampler._w) and torch.equal(learner.actor_weights, pack_actor_weights(pol))
        sampler.refresh_weights()
        assert not torch.equal(before, sampler._w) and torch.equal(sampler._w, learner.actor_weights)
        served = int(sampler.served.item())
        res = sampler.launch()
        torch.cuda.synchronize()
        assert int(sampler.served.item()) > served and torch.isfinite(res["reward"]).all()
    finally:
        e.close()
