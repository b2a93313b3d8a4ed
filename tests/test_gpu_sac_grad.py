"""GPU checks of the gradient half of a SAC update in HIP (sit_sac_critic_step / sit_sac_policy_step,
csrc/sit_sac_grad.h) and of SacLearner(gradient="hip"), on float32 and float64 handles.

1. Gradients, one step from zero moments.  After the first Adam step from m = 0, m = (1 - beta1) g, so the
   moment blocks expose every gradient.  Reference: float64 CPU autograd of the same losses followed by
   torch.optim.Adam (tests/sac_grad_reference.py).  Inputs: states and actions uniform in [-1, 1], y and eps
   standard normal, all rounded to float32; default-initialised networks under a fixed seed.
   Error measure, per tensor: max |got - ref| / max |ref|.
   Yardstick Y: the largest such error that float32 CPU autograd makes on the same inputs against float64,
   over every gradient tensor and the five results; computed by the test at run time.
   Bound: LEARNER_MARGIN (4) x Y for every gradient tensor, the five results and log_alpha (the factor is
   the project's margin for a different summation order).
   Updated parameters: the first Adam step moves an element by lr g / (|g| + 1e-8), which is
   ill-conditioned where |g| is near 1e-8 (a float32 CPU run misses float64 by 1e-6 .. 1e-4 of max |p|
   through one or two such elements, whatever its gradient error, and by another amount on another
   machine), so they are checked twice: against float64 Adam applied to the device's own gradient, within
   one float32 ulp of max |p| (half an ulp for the final rounding; the update itself is at most lr and
   known to about 1e-6 of that), and end to end against the reference, per element, within what a
   gradient error of 4 Y can move the step (adam_first_step_bound).
   Conditions on the reference (asserted; the seeds below were chosen on the CPU as the first seed >= 1
   whose float64 reference meets them): every hidden pre-activation of the five network passes has
   |z| >= 1e-6, |q1 - q2| >= 1e-4 in the policy pass, ls_raw at least 1e-4 from both clip bounds, Y <= 2e-6.
   Seeds: B = 1: 1, 7: 1, 8: 2, 9: 2, 64: 2, 67: 2.  Y on two CPUs: 3.9e-7, 3.9e-7, 3.8e-7 / 4.1e-7,
   4.5e-7 / 4.9e-7, 4.8e-7 / 5.6e-7, 1.1e-6; the float32 CPU error of the updated parameters, end to end:
   5.5e-8, 4.8e-6 / 5.4e-6, 1.4e-6 / 2.2e-6, 4.0e-6 / 1.6e-6, 1.7e-5 / 2.9e-5, 7.0e-6 / 4.5e-6.
   Measured on the MI355X, either handle, in the same order of B: worst gradient tensor 5.6e-7, 2.8e-7,
   4.1e-7, 1.0e-6, 3.4e-7, 8.8e-7; results 1.4e-7, 4.8e-7, 7.0e-8, 1.4e-7, 4.5e-8, 4.9e-8; log_alpha 3.1e-8;
   updated parameters against float64 Adam of the device's gradient at most 6.0e-8, end to end 5.5e-8,
   4.5e-6, 3.0e-7, 2.3e-6, 2.3e-5, 7.3e-6.
2. Clip and saturation at B = 8: an actor with W3 = 0 and b3 = (0, ls_raw); ls_raw at -25, -20, 2, 3, and
   x sweeping [-12, 12] at ls_raw = 0.  Measured: dls at -20 and 2 1.0e-7 and 1.2e-7 (float32 CPU 1.1e-7,
   2.2e-4); saturation 1.1e-7 (float32 CPU 3.0e-2).
3. Determinism, canaries behind every buffer and in the blocks' padding, tune = 0.
4. SacLearner(gradient="hip") against gradient="torch" and sac_update_reference over 8 updates: the hip
   error against float64 is at most 4 x the torch mode's, measured in the same run.  Measured: torch 1.14e-7
   (5-tuples) and 3.85e-7 (parameters), hip 1.00e-7 and 7.5e-7.
5. Checkpoints.  6. Serving.  7. Rejections.
"""
import copy
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sit = pytest.importorskip("sac_maritime_ast_amd")
from sac_maritime_ast_amd import ReplayMemory, VecMultiShipRLEnv, _lib, make_scenario, sac  # noqa: E402
from sac_maritime_ast_amd.samplers import GaussianPolicy, PolicySampler  # noqa: E402
import sac_grad_reference as R  # noqa: E402
from sac_cases import (ADAM_EPS, BETA1, BETA2, CANARY, DEV, ROW, SEED, SEEDS, UPDATE, Steps, bits, blocks_are_the_modules,  # noqa: E402
                       case_of, device_memory, learner_err, learner_params, new_learner, reference_run)

MARGIN = 4.0                             # LEARNER_MARGIN / RAW_MARGIN of tests/test_gpu_sac.py


@pytest.fixture(scope="module", params=[32, 64])
def env(request):
    e = VecMultiShipRLEnv(scenario=make_scenario(64), precision=request.param, device=DEV)
    yield e
    e.close()


def adam_first_step(p0, g, lr=R.LR):
    """torch.optim.Adam's first step from zero moments in float64."""
    m, v = (1.0 - BETA1) * g, (1.0 - BETA2) * g * g
    return p0 - (lr / (1.0 - BETA1)) * m / (np.sqrt(v) / math.sqrt(1.0 - BETA2) + ADAM_EPS)


def adam_first_step_bound(g_ref, rel, p_max, lr=R.LR):
    """Per element, how far the first Adam step of a gradient within rel * max |g_ref| of g_ref may land from
    the step of g_ref itself: the step is -lr u(g), u = g / (|g| + eps), |u| < 1, u' = eps / (|g| + eps)^2, so
    |du| <= min(2, dg eps / (max(|g_ref| - dg, 0) + eps)^2); plus one float32 ulp of max |p| for the
    arithmetic."""
    dg = rel * np.abs(g_ref).max()
    du = np.minimum(2.0, dg * ADAM_EPS / (np.maximum(np.abs(g_ref) - dg, 0.0) + ADAM_EPS) ** 2)
    return lr * du + 2.0 ** -23 * p_max


def initial_params(case):
    return {"critic_params": [p.detach().double().numpy() for p in case["critic"].parameters()],
            "policy_params": [p.detach().double().numpy() for p in case["policy"].parameters()]}


# ---------------------------------------------------------------------------------------------
# 1. gradients, one step from zero moments
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture_case(B):
    case = case_of(B)
    ref = R.autograd_steps(case, torch.float64)
    f32 = R.autograd_steps(case, torch.float32)
    return case, ref, R.errors(f32, ref)


@pytest.mark.parametrize("B", sorted(SEEDS))
def test_gradients_one_step(env, B):
    case, ref, cpu = fixture_case(B)
    yard = max(cpu["critic_grads"], cpu["policy_grads"], cpu["results"])
    print(f"sac grad, B={B}, seed {SEEDS[B]}: reference conditions", {k: f"{v:.2e}" for k, v in ref["conditions"].items()},
          "float32 CPU against float64:", {k: f"{v:.2e}" for k, v in cpu.items()}, f"yardstick {yard:.2e}")
    cond = ref["conditions"]
    assert cond["z_min"] >= 1e-6 and cond["q_gap"] >= 1e-4 and cond["ls_margin"] >= 1e-4 and yard <= 2e-6
    got = Steps(env, case).run()
    err = R.errors(got, ref)
    err["log_alpha"] = abs(got["log_alpha"] - ref["log_alpha"]) / abs(ref["log_alpha"])
    err["alpha_grad"] = abs(got["alpha_grad"] - ref["alpha_grad"]) / abs(ref["alpha_grad"])
    own = {}
    p0 = initial_params(case)
    for g, k in (("critic_grads", "critic_params"), ("policy_grads", "policy_params")):
        own[k] = max(R.tensor_err(p, adam_first_step(a, b)) for p, a, b in zip(got[k], p0[k], got[g]))
    print(f"sac grad, f{env.precision}, B={B}: device against float64:", {k: f"{v:.2e}" for k, v in err.items()},
          "updated parameters against float64 Adam of the device's gradient:", {k: f"{v:.2e}" for k, v in own.items()})
    for k in ("critic_grads", "policy_grads", "results", "log_alpha", "alpha_grad"):
        assert err[k] <= MARGIN * yard, (k, err[k], yard)
    for g, k in (("critic_grads", "critic_params"), ("policy_grads", "policy_params")):
        assert own[k] <= 2.0 ** -23, (k, own[k])
        for p, pr, gr in zip(got[k], ref[k], ref[g]):
            assert np.all(np.abs(p - pr) <= adam_first_step_bound(gr, MARGIN * yard, np.abs(pr).max())), k
    # second moments: v = (1 - beta2) g^2, and alpha = exp(log_alpha)
    for g, k in (("critic_grads", "critic_v"), ("policy_grads", "policy_v")):
        assert max(R.tensor_err(v, (1.0 - BETA2) * a * a) for v, a in zip(got[k], got[g])) <= 1e-6
    assert abs(got["alpha"] - math.exp(got["log_alpha"])) <= 1e-6 * got["alpha"]
    assert abs(got["results"][4] - got["alpha"]) == 0.0


def test_reference_losses_are_the_learners():
    """The reference of this file is sac._gradient_half's: one update of SacUpdateReference from the same
    networks gives the gradients' Adam step (checked on the critic parameters, where y is an input)."""
    case, ref, _ = fixture_case(8)
    pol, q = copy.deepcopy(case["policy"]).double(), copy.deepcopy(case["critic"]).double()
    optims = {"critic": torch.optim.Adam(q.parameters(), lr=R.LR), "policy": torch.optim.Adam(pol.parameters(), lr=R.LR)}
    log_alpha = torch.full((1,), math.log(R.ALPHA0), dtype=torch.float32).double().requires_grad_(True)
    optims["alpha"] = torch.optim.Adam([log_alpha], lr=R.LR)
    t = lambda k: torch.from_numpy(case[k])  # noqa: E731
    out = sac._gradient_half(pol, q, optims, log_alpha, log_alpha.detach().exp(), True,
                             {"state": t("state"), "action": t("action")[:, None]}, t("y"), t("eps"))
    assert np.allclose([float(v) for v in out[:4]] + [float(out[4][0])], ref["results"], rtol=1e-12, atol=0)
    for a, b in zip(list(q.parameters()) + list(pol.parameters()), ref["critic_params"] + ref["policy_params"]):
        assert np.allclose(a.detach().numpy(), b, rtol=1e-12, atol=1e-15)


# ---------------------------------------------------------------------------------------------
# 2. clip and saturation
# ---------------------------------------------------------------------------------------------
def head_case(ls_raw, eps=None):
    """The B = 8 case with the actor's head replaced by W3 = 0 and b3 = (0, ls_raw): mu = 0 and this ls_raw
    exactly in every row, x = exp(clip(ls_raw)) eps.  The hidden layers then receive no gradient;
    dW3 = sum_b g[b] h2[b] and db3 = sum_b g[b] carry (dmu, dls)."""
    case = dict(case_of(8))
    case["policy"] = copy.deepcopy(case["policy"])
    with torch.no_grad():
        case["policy"].net[4].weight.zero_()
        case["policy"].net[4].bias.copy_(torch.tensor([0.0, ls_raw]))
    if eps is not None:
        case["eps"] = R.F32(eps)
    return case


W3, B3 = 4, 5                                   # parameters() order: the head's weight [2, 256] and bias [2]


@pytest.mark.parametrize("ls_raw", [-25.0, -20.0, 2.0, 3.0])
def test_clip_passes_the_gradient_at_the_bounds_only(env, ls_raw):
    """Rows with ls_raw at -25, -20, 2 and 3 (the fixture's standard normal eps): dls is zero in every row
    outside [-20, 2] and passes at the bounds, as torch.clamp's does; there it matches float64 within 4 x
    the float32 CPU error on the same tensors (row 1 of dW3, db3[1])."""
    case = head_case(ls_raw)
    ref, cpu = R.autograd_steps(case, torch.float64), R.autograd_steps(case, torch.float32)
    got = Steps(env, case).run()
    dls = lambda r: [r["policy_grads"][W3][1], r["policy_grads"][B3][1:]]  # noqa: E731
    for i in range(4):                          # the hidden layers: no gradient reaches them
        assert not got["policy_grads"][i].any() and not ref["policy_grads"][i].any()
    assert all(np.isfinite(t).all() for t in got["policy_grads"]) and np.isfinite(got["results"]).all()
    if ls_raw < -20.0 or ls_raw > 2.0:
        assert not any(t.any() for t in dls(got)) and not any(t.any() for t in dls(ref))
    else:
        assert all(t.any() for t in dls(got)) and all(t.any() for t in dls(ref))
        yard = max(R.tensor_err(a, b) for a, b in zip(dls(cpu), dls(ref)))
        err = max(R.tensor_err(a, b) for a, b in zip(dls(got), dls(ref)))
        print(f"sac grad clip, f{env.precision}, ls_raw={ls_raw}: dls float32 CPU {yard:.2e}, device {err:.2e}")
        assert err <= MARGIN * yard, (err, yard)


def test_saturation(env):
    """x sweeping [-12, 12] over the 8 rows (ls_raw = 0, eps = x; rows 0 and 7 at -12 and 12): dx is finite and
    (dmu, dls), read from dW3 and db3, match float64 within 4 x the float32 CPU error on the same inputs
    -- and within 1e-5, the project's float32 contract (the bound of test_gpu_sac.py's saturation sweep):
    float32 autograd forms 1 - a * a, which cancels, and misses dls by percents here."""
    case = head_case(0.0, np.linspace(-12.0, 12.0, 8))
    ref, cpu = R.autograd_steps(case, torch.float64), R.autograd_steps(case, torch.float32)
    got = Steps(env, case).run()
    assert all(np.isfinite(t).all() for t in got["policy_grads"]) and np.isfinite(got["results"]).all()
    rel = lambda r: max([R.tensor_err(r["policy_grads"][i], ref["policy_grads"][i]) for i in (W3, B3)]  # noqa: E731
                        + [abs(a - b) / abs(b) for a, b in zip(r["results"], ref["results"])])
    yard, err = rel(cpu), rel(got)
    print(f"sac grad saturation, f{env.precision}: float32 CPU {yard:.2e}, device {err:.2e}")
    assert ref["policy_grads"][B3][0] != 0.0 and yard > 1e-3
    assert err <= MARGIN * yard and err <= 1e-5, (err, yard)


# ---------------------------------------------------------------------------------------------
# 3. determinism and bounds
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [9, 67])
def test_two_runs_are_bit_identical(env, B):
    case = fixture_case(B)[0]
    a, b = Steps(env, case).run()["raw"], Steps(env, case).run()["raw"]
    for k in a:
        if k != "ws":
            assert torch.equal(bits(a[k]), bits(b[k])), k
    assert torch.equal(bits(a["ws"][:B * ROW]), bits(b["ws"][:B * ROW]))       # the policy step's records
    assert torch.all(a["ws"][:B * ROW] != CANARY) and torch.isfinite(a["ws"]).all()


def test_drawn_noise_is_policy_noise(env):
    B = 67
    case = dict(fixture_case(B)[0])
    case["eps"] = R.F32(sac.policy_noise(SEED + 1, UPDATE, B))
    given = Steps(env, case).run()
    drawn = Steps(env, case, drawn=True, seed=SEED + 1).run()
    assert np.allclose(drawn["results"], given["results"], rtol=1e-5, atol=0)
    for a, b in zip(drawn["policy_grads"], given["policy_grads"]):
        assert R.tensor_err(a, b) <= 1e-5
    other = Steps(env, case, drawn=True, seed=SEED + 2).run()
    assert not np.allclose(other["results"][2:4], given["results"][2:4], rtol=1e-5, atol=0)


def test_untuned_temperature_is_untouched(env):
    case, ref, _ = fixture_case(9)
    s = Steps(env, case, tune=False)
    before = s.scalars.clone()
    got = s.run()
    assert torch.equal(bits(s.scalars), bits(before))
    assert got["results"][3] == 0.0 and got["results"][4] == got["alpha"]
    tuned = Steps(env, case).run()
    assert np.array_equal(got["results"][:3], tuned["results"][:3])
    for a, b in zip(got["policy_params"], tuned["policy_params"]):
        assert np.array_equal(a, b)
    # and without the three pointers
    s = Steps(env, case, tune=False)
    s.policy_args.log_alpha = s.policy_args.log_alpha_m = s.policy_args.log_alpha_v = None
    assert np.array_equal(s.run()["results"], got["results"])


# ---------------------------------------------------------------------------------------------
# 7. rejections
# ---------------------------------------------------------------------------------------------
def test_invalid_arguments_launch_nothing(env):
    case = fixture_case(9)[0]
    s = Steps(env, case)
    before = {k: t.clone() for k, t in s.buffers().items()}
    for which in ("critic", "policy"):
        for args, field, value, good in s.invalid_arguments(which):
            setattr(args, field, value)
            assert s.call(which) == _lib.SIT_E_INVALID, (which, field)
            assert b"sac" in env.lib.sit_last_error(env.handle), (which, field)
            setattr(args, field, good)
    with torch.cuda.device(env.device):
        assert env.lib.sit_sac_critic_step(env.handle, None, env._stream()) == _lib.SIT_E_INVALID
        assert env.lib.sit_sac_policy_step(env.handle, None, env._stream()) == _lib.SIT_E_INVALID
    torch.cuda.synchronize()
    for k, t in s.buffers().items():
        assert torch.equal(bits(t), bits(before[k])), f"{k}: an invalid call wrote"
    s.run()                                          # and the restored arguments are accepted


def test_learner_rejects_other_modes_and_architectures(env):
    pol = GaussianPolicy().to(DEV)
    with pytest.raises(ValueError):
        sac.SacLearner(env, pol, gradient="hip", target="torch")
    with pytest.raises(ValueError):
        sac.SacLearner(env, GaussianPolicy(hidden=(64, 64)).to(DEV), critic=sac.QNetwork(hidden=64), gradient="hip")
    with pytest.raises(ValueError):
        sac.SacLearner(env, pol, critic=sac.QNetwork(hidden=64), gradient="hip")


# ---------------------------------------------------------------------------------------------
# 4. SacLearner against sac_update_reference (the fixture of tests/sac_cases.py)
# ---------------------------------------------------------------------------------------------
N_REC, BATCH, N_UPD, N_MORE = 256, 64, 8, 2


def learner_run(env, gradient, n=N_UPD):
    learner, mem, tuples = new_learner(env, gradient=gradient), device_memory(env, N_REC), []
    for u in range(n):
        tuples.append(learner.update_parameters(mem, BATCH, u))
        if gradient == "hip":
            assert blocks_are_the_modules(learner), u
    return learner, mem, tuples


def test_learner_matches_the_float64_reference(env):
    ref_t, ref_p, _ = reference_run(env.precision, BATCH, N_UPD, N_MORE)
    err = {}
    for gradient in ("torch", "hip"):
        learner, mem, tuples = learner_run(env, gradient)
        assert all(len(t) == 5 and all(isinstance(v, float) and math.isfinite(v) for v in t) for t in tuples)
        err[gradient] = learner_err(tuples, learner_params(learner), ref_t[:N_UPD], ref_p)
        print(f"sac learner, f{env.precision}, gradient={gradient}, {N_UPD} updates against float64:",
              {k: f"{v:.2e}" for k, v in err[gradient].items()})
    bad = {k: (v, err["torch"][k]) for k, v in err["hip"].items() if v > MARGIN * err["torch"][k]}
    assert not bad, bad
    assert ref_t[N_UPD - 1][4] != ref_t[0][4] and ref_t[N_UPD - 1][0] != ref_t[0][0]


# ---------------------------------------------------------------------------------------------
# 5. checkpoints
# ---------------------------------------------------------------------------------------------
def test_hip_state_dict_round_trip_is_exact(env):
    learner, mem, _ = learner_run(env, "hip", 3)
    sd, msd = learner.state_dict(), mem.state_dict()
    want = learner.update_parameters(mem, BATCH, 3)
    other = new_learner(env, fresh=True, gradient="hip")
    other.load_state_dict(sd)
    assert blocks_are_the_modules(other)
    mem.load_state_dict(msd)
    got = other.update_parameters(mem, BATCH, 3)
    assert got == want
    for k in ("actor_weights", "online_weights", "target_weights"):
        assert torch.equal(getattr(other, k), getattr(learner, k)), k
    for k in ("policy", "critic", "alpha"):
        assert torch.equal(other._m[k], learner._m[k]) and torch.equal(other._v[k], learner._v[k]), k
    assert other._steps == learner._steps == {"critic": 4, "policy": 4, "alpha": 4}


@pytest.mark.parametrize("first,second", [("torch", "hip"), ("hip", "torch")])
def test_checkpoints_cross_the_gradient_modes(env, first, second):
    """N_UPD updates in one mode, a checkpoint, N_MORE updates in the other: the error against the float64
    reference stays within 4 x the error of the torch mode run straight through, measured here."""
    ref_t, _, ref_p = reference_run(env.precision, BATCH, N_UPD, N_MORE)
    straight, smem, stuples = learner_run(env, "torch", N_UPD + N_MORE)
    base = learner_err(stuples[N_UPD:], learner_params(straight), ref_t[N_UPD:], ref_p)
    learner, mem, _ = learner_run(env, first)
    other = new_learner(env, fresh=True, gradient=second)
    other.load_state_dict(learner.state_dict())
    tuples = [other.update_parameters(mem, BATCH, u) for u in range(N_UPD, N_UPD + N_MORE)]
    err = learner_err(tuples, learner_params(other), ref_t[N_UPD:], ref_p)
    print(f"sac checkpoint, f{env.precision}, {first} -> {second}:", {k: f"{v:.2e}" for k, v in err.items()},
          "torch straight through:", {k: f"{v:.2e}" for k, v in base.items()})
    bad = {k: (v, base[k]) for k, v in err.items() if v > MARGIN * base[k]}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------
# 6. serving
# ---------------------------------------------------------------------------------------------
def test_rollout_push_update_serve_hip():
    """The rollout-push-update-serve loop of tests/test_gpu_sac.py with gradient="hip": the sampler's next
    launch notices the changed actor by itself and serves the learner's block."""
    e = VecMultiShipRLEnv(scenario=make_scenario(64), precision=32, device=DEV)
    try:
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
        assert len(mem) > BATCH, len(mem)
        before = sampler._w.clone()
        assert torch.equal(before, learner.actor_weights)
        out = learner.update_parameters(mem, BATCH, 0)
        assert len(out) == 5 and all(math.isfinite(v) for v in out), out
        assert torch.equal(before, sampler._w) and blocks_are_the_modules(learner)
        assert not torch.equal(before, learner.actor_weights)
        served = int(sampler.served.item())
        res = sampler.launch()                       # no refresh_weights(): the launch sees the new versions
        torch.cuda.synchronize()
        assert torch.equal(sampler._w, learner.actor_weights)
        assert int(sampler.served.item()) > served and torch.isfinite(res["reward"]).all()
    finally:
        e.close()
