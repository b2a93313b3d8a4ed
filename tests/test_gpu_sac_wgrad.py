"""GPU checks of the tiled weight-gradient calls (sit_sac_critic_step_tiled / sit_sac_policy_step_tiled,
csrc/sit_sac_wgrad.h) and of SacLearner(weight_gradient="mfma"), on float32 and float64 handles.

The tiled calls form each weight gradient as 32 x 32 MFMA tiles whose k index is the batch row; the
float32-input MFMA is a k-ordered fmaf chain, which is the sum the plain calls form per element, so every
check here is equality of bits against the plain calls from the same state, not a tolerance.

1. One critic step and one policy step: the six blocks (padding included), results[0:5] and the four
   temperature scalars, at B = 1, 2, 3 (the odd tail and one MFMA), 7, 8, 9 (a row-block edge), 31, 32, 33 (the
   edge of the 32-row prefetch group), 64, 67, 1025 and 4096 (long chains), with the temperature tuned and
   not, the noise given and drawn.
2. Two consecutive steps (non-zero moments, bias corrections of t = 1 and t = 2) at B = 9 and 64.
3. Canaries behind every buffer and in the critic blocks' padding after the tiled calls at B = 1, 9, 67
   (the lanes of the odd row past the batch must not load); two tiled runs give the same bits.
4. The tiled calls reject what the plain calls reject and launch nothing.
5. SacLearner(weight_gradient="mfma") against "sum": 3 updates of batch 64 from a 256-record memory, and a
   checkpoint written in either mode and continued in the other.

The buffers are those of tests/sac_cases.py (its Steps: 8 canaries behind every buffer, the critic blocks'
padding set to the canary), the cases tests/sac_grad_reference.make_case(B, seed).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

sit = pytest.importorskip("sac_maritime_ast_amd")
from sac_maritime_ast_amd import VecMultiShipRLEnv, _lib, make_scenario  # noqa: E402
from sac_cases import (CANARY, CRITIC_SIZE, CW, DEV, ROW, Steps, bits, blocks_are_the_modules, case_of,  # noqa: E402
                       device_memory, new_learner)

BATCH = 64
BATCHES = [1, 2, 3, 7, 8, 9, 31, 32, 33, 64, 67, 1025, 4096]
BLOCKS = ("critic", "critic_m", "critic_v", "actor", "actor_m", "actor_v")


@pytest.fixture(scope="module", params=[32, 64])
def env(request):
    e = VecMultiShipRLEnv(scenario=make_scenario(64), precision=request.param, device=DEV)
    yield e
    e.close()


def assert_same_state(a, b, what):
    """The six blocks with their padding, the five results and the four temperature scalars, bit for bit."""
    for k in BLOCKS + ("results", "scalars"):
        if not torch.equal(bits(a[k]), bits(b[k])):
            differ = (bits(a[k]) != bits(b[k])).nonzero().flatten()
            i = int(differ[0])
            raise AssertionError(f"{what}: {k} differs in {differ.numel()} of {a[k].numel()} elements, first at {i}: "
                                 f"{float(a[k][i])!r} against {float(b[k][i])!r}")
    assert a["results"].numel() == 5 and a["scalars"].numel() == 4


# ---------------------------------------------------------------------------------------------
# 1. one critic step and one policy step
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
def test_tiled_steps_are_the_plain_steps(env, B):
    case = case_of(B)
    for tune in (True, False):
        for drawn in (False, True):
            plain = Steps(env, case, tune=tune, drawn=drawn, tiled=False).run()["raw"]
            tiled = Steps(env, case, tune=tune, drawn=drawn, tiled=True).run()["raw"]
            assert_same_state(tiled, plain, f"B={B}, tune={tune}, drawn={drawn}")
            assert torch.isfinite(tiled["results"]).all() and tiled["actor_m"].any() and tiled["critic_m"].any()
            if not tune:
                assert tiled["results"][3] == 0.0 and tiled["scalars"][2] == 0.0


# ---------------------------------------------------------------------------------------------
# 2. non-zero moments
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [9, 64])
def test_two_consecutive_steps(env, B):
    case = case_of(B)
    out = {}
    for tiled in (False, True):
        s = Steps(env, case, tiled=tiled)
        first = s.run()["raw"]
        s.set_step(2)
        out[tiled] = (first, s.run()["raw"])
    assert_same_state(out[True][0], out[False][0], f"B={B}, t=1")
    assert_same_state(out[True][1], out[False][1], f"B={B}, t=2")
    assert not torch.equal(out[True][1]["actor"], out[True][0]["actor"])          # the second step moved on


# ---------------------------------------------------------------------------------------------
# 3. bounds and determinism
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 9, 67])
def test_tiled_calls_keep_canaries_and_repeat(env, B):
    case = case_of(B)
    runs = []
    for _ in range(2):
        s = Steps(env, case, tiled=True)
        got = s.run()["raw"]                             # run() checks every canary and the padding
        assert torch.all(s.ws[s.n_ws:] == CANARY)        # the float behind row B - 1's record, where row B would be
        for k in ("critic", "critic_m", "critic_v"):
            assert torch.all(got[k].view(2, CW)[:, CRITIC_SIZE:] == CANARY), k
        assert torch.isfinite(got["ws"]).all() and torch.all(got["ws"][:B * ROW] != CANARY)
        runs.append(got)
    for k in runs[0]:
        assert torch.equal(bits(runs[0][k]), bits(runs[1][k])), k


# ---------------------------------------------------------------------------------------------
# 4. rejections
# ---------------------------------------------------------------------------------------------
def test_tiled_calls_reject_what_the_plain_calls_reject(env):
    s = Steps(env, case_of(9), tiled=True)
    before = {k: t.clone() for k, t in s.buffers().items()}
    for which in ("critic", "policy"):
        for args, field, value, good in s.invalid_arguments(which):
            setattr(args, field, value)
            tiled_rc = s.call(which)
            tiled_why = env.lib.sit_last_error(env.handle)
            s.tiled = False
            assert s.call(which) == tiled_rc == _lib.SIT_E_INVALID, (which, field)
            assert env.lib.sit_last_error(env.handle) == tiled_why and b"sac" in tiled_why, (which, field)
            s.tiled = True
            setattr(args, field, good)
    with torch.cuda.device(env.device):
        assert env.lib.sit_sac_critic_step_tiled(env.handle, None, env._stream()) == _lib.SIT_E_INVALID
        assert env.lib.sit_sac_policy_step_tiled(env.handle, None, env._stream()) == _lib.SIT_E_INVALID
    torch.cuda.synchronize()
    for k, t in s.buffers().items():
        assert torch.equal(bits(t), bits(before[k])), f"{k}: an invalid call wrote"
    s.run()                                              # and the restored arguments are accepted


# ---------------------------------------------------------------------------------------------
# 5. the learner
# ---------------------------------------------------------------------------------------------
def assert_same_learner(a, b):
    for k in ("actor_weights", "online_weights", "target_weights", "log_alpha", "alpha"):
        assert torch.equal(bits(getattr(a, k).detach()), bits(getattr(b, k).detach())), k
    for k in ("policy", "critic", "alpha"):
        assert torch.equal(bits(a._m[k]), bits(b._m[k])) and torch.equal(bits(a._v[k]), bits(b._v[k])), k
    for p, q in zip(list(a.policy.parameters()) + list(a.critic.parameters()),
                    list(b.policy.parameters()) + list(b.critic.parameters())):
        assert torch.equal(bits(p.detach()), bits(q.detach()))
    assert a._steps == b._steps


def test_learner_modes_agree_and_share_checkpoints(env):
    lrn = {m: new_learner(env, gradient="hip", weight_gradient=m) for m in ("sum", "mfma")}
    mem = {m: device_memory(env) for m in lrn}
    assert lrn["mfma"].weight_gradient == "mfma" and lrn["sum"].weight_gradient == "sum"
    for u in range(3):
        out = {m: lrn[m].update_parameters(mem[m], BATCH, u) for m in lrn}
        assert out["mfma"] is not None and len(out["mfma"]) == 5
        assert out["mfma"] == out["sum"], u
        assert blocks_are_the_modules(lrn["mfma"])
    assert_same_learner(lrn["mfma"], lrn["sum"])
    # a checkpoint written in one mode, continued in the other
    want = None
    for first, second in (("mfma", "sum"), ("sum", "mfma")):
        sd, msd = lrn[first].state_dict(), mem[first].state_dict()
        other = new_learner(env, fresh=True, gradient="hip", weight_gradient=second)
        other.load_state_dict(sd)
        omem = device_memory(env)
        omem.load_state_dict(msd)
        got = other.update_parameters(omem, BATCH, 3)
        want = got if want is None else want
        assert got == want
        lrn[first + ">" + second] = other
    for m in ("sum", "mfma"):
        assert lrn[m].update_parameters(mem[m], BATCH, 3) == want
    assert_same_learner(lrn["mfma>sum"], lrn["sum>mfma"])
    assert_same_learner(lrn["mfma>sum"], lrn["mfma"])
    assert_same_learner(lrn["sum"], lrn["mfma"])
