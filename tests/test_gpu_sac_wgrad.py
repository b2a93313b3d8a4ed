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

The buffers are those of tests/test_gpu_sac_grad.py (its Steps: 8 canaries behind every buffer, the critic
blocks' padding set to the canary), the cases tests/sac_grad_reference.make_case(B, seed).
"""
import copy
import ctypes
import functools

import pytest
import torch

import sac_grad_reference as R
from test_gpu_sac_grad import (BATCH, CANARY, CRITIC_SIZE, CW, DEV, LEARNER_KW, ROW, SEEDS, Steps, adam_scalars, bits,
                               blocks_are_the_modules, device_memory, networks)

pytestmark = pytest.mark.gpu

sit = pytest.importorskip("sac_maritime_ast_amd")
from sac_maritime_ast_amd import VecMultiShipRLEnv, _lib, make_scenario, sac  # noqa: E402

BATCHES = [1, 2, 3, 7, 8, 9, 31, 32, 33, 64, 67, 1025, 4096]
BLOCKS = ("critic", "critic_m", "critic_v", "actor", "actor_m", "actor_v")


@pytest.fixture(scope="module", params=[32, 64])
def env(request):
    e = VecMultiShipRLEnv(scenario=make_scenario(64), precision=request.param, device=DEV)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def case_of(B):
    return R.make_case(B, SEEDS.get(B, 2))


class PathSteps(Steps):
    """Steps through the plain calls (tiled=False) or the _tiled ones."""

    def __init__(self, env, case, tiled, **kw):
        super().__init__(env, case, **kw)
        self.tiled = tiled

    def call(self, which):
        fn = getattr(self.env.lib, f"sit_sac_{which}_step" + ("_tiled" if self.tiled else ""))
        args = self.critic_args if which == "critic" else self.policy_args
        with torch.cuda.device(self.env.device):
            return fn(self.env.handle, ctypes.byref(args), self.env._stream())

    def set_step(self, t):
        self.critic_args.adam = adam_scalars(t)
        self.policy_args.adam = self.policy_args.alpha_adam = adam_scalars(t)


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
            plain = PathSteps(env, case, False, tune=tune, drawn=drawn).run()["raw"]
            tiled = PathSteps(env, case, True, tune=tune, drawn=drawn).run()["raw"]
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
        s = PathSteps(env, case, tiled)
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
        s = PathSteps(env, case, True)
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
    s = PathSteps(env, case_of(9), True)
    before = {k: t.clone() for k, t in s.buffers().items()}
    for which, args in (("critic", s.critic_args), ("policy", s.policy_args)):
        good = {k: getattr(args, k) for k, _ in args._fields_ if k not in ("adam", "alpha_adam")}
        block = "critic_weights" if which == "critic" else "actor_weights"
        moment = "critic_m" if which == "critic" else "actor_v"
        cases = [(k, None) for k in (block, moment, "state", "workspace", "results")]
        cases += [("batch", 0), ("batch", -1), (block, good[block] + 4), (moment, good[moment] + 8),
                  ("workspace_floats", s.n_ws - 1)]
        if which == "policy":
            cases += [("critic_weights", None), ("critic_weights", good["critic_weights"] + 4), ("alpha", None),
                      ("log_alpha", None)]
        else:
            cases += [("action", None), ("y", None)]
        for field, value in cases:
            setattr(args, field, value)
            tiled_rc = s.call(which)
            tiled_why = env.lib.sit_last_error(env.handle)
            s.tiled = False
            assert s.call(which) == tiled_rc == _lib.SIT_E_INVALID, (which, field)
            assert env.lib.sit_last_error(env.handle) == tiled_why and b"sac" in tiled_why, (which, field)
            s.tiled = True
            setattr(args, field, good[field])
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
def new_learner(env, weight_gradient, fresh=False):
    pol, q = networks()
    if fresh:
        torch.manual_seed(99)
        pol, q = type(pol)(), sac.QNetwork()             # other initial values
    return sac.SacLearner(env, copy.deepcopy(pol).to(DEV), critic=copy.deepcopy(q), gradient="hip",
                          weight_gradient=weight_gradient, **LEARNER_KW)


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
    lrn = {m: new_learner(env, m) for m in ("sum", "mfma")}
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
        other = new_learner(env, second, fresh=True)
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
