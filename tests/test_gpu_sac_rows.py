"""GPU checks of the wide row-kernel calls (sit_sac_target_wide / sit_sac_critic_step_wide /
sit_sac_policy_step_wide, csrc/sit_sac_rows.h) and of SacLearner(row_pass="mfma"), on float32 and float64
handles.

The wide row kernels take 32 rows per block and run forward and backward layer 2 as float32-input MFMA
chains in the order in which the narrow kernels add with fmaf (four K-quarter chains joined as
((q0 + q1) + (q2 + q3)) + b2; one chain over n = 0..255), and everything else is the narrow kernels'
arithmetic.  So every check here is equality of bits against sit_sac_target and the _tiled step calls from
the same state, not a tolerance.

Batch sizes: 1 (one row), 2, 7, 8, 9 (the narrow kernels' 8-row edge), 31, 32, 33 (the 32-row block edge), 63, 64,
65, 67 (two blocks, with and without a tail) and 1025 (33 blocks, a one-row tail).

1. The target: y, next_action, next_logp, q1, q2 on canaried buffers, the noise given and drawn.
2. One critic step and one policy step: the six blocks with their padding, results[0:5], the four temperature
   scalars, and the workspace records of rows < B after each call (what the row kernel itself writes), with
   the temperature tuned and not, the noise given and drawn.
3. Two consecutive steps (non-zero moments, t = 1 then 2) at B = 33 and 64.
4. Canaries behind every buffer and in the critic blocks' padding, the float behind row B - 1's record, and
   two runs giving the same bits, at B = 1, 33, 67.
5. The wide calls reject what the plain calls reject, with the same error string, and launch nothing.
6. SacLearner(row_pass="mfma") against "valu": 3 updates of batch 64, a checkpoint written in either mode and
   continued in the other, then 3 updates of batch 100, from a 256-record memory.

The cases are tests/sac_cases.case_of(B); the target's inputs are made of the same case (its state as
next_state, its y as the reward, its eps as the noise, every third row masked).
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sit = pytest.importorskip("sac_maritime_ast_amd")
from sac_maritime_ast_amd import VecMultiShipRLEnv, _lib, make_scenario, sac  # noqa: E402
from sac_maritime_ast_amd.samplers import pack_actor_weights  # noqa: E402
from sac_cases import (CANARY, CRITIC_SIZE, CW, DEV, GAMMA, ROW, SEED, UPDATE, Steps, bits, blocks_are_the_modules,  # noqa: E402
                       case_of, device_memory, new_learner, with_tail)

BATCHES = [1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 67, 1025]
BLOCKS = ("critic", "critic_m", "critic_v", "actor", "actor_m", "actor_v")
OUTPUTS = ("y", "next_action", "next_logp", "q1", "q2")


@pytest.fixture(scope="module", params=[32, 64])
def env(request):
    e = VecMultiShipRLEnv(scenario=make_scenario(64), precision=request.param, device=DEV)
    yield e
    e.close()


def assert_same_bits(a, b, keys, what):
    for k in keys:
        if not torch.equal(bits(a[k]), bits(b[k])):
            differ = (bits(a[k]) != bits(b[k])).nonzero().flatten()
            i = int(differ[0])
            raise AssertionError(f"{what}: {k} differs in {differ.numel()} of {a[k].numel()} elements, first at {i}: "
                                 f"{float(a[k][i])!r} against {float(b[k][i])!r}")


class WideSteps(Steps):
    """Steps whose calls are sit_sac_critic_step_wide / sit_sac_policy_step_wide."""

    def call(self, which):
        fn = getattr(self.env.lib, f"sit_sac_{which}_step_wide")
        args = self.critic_args if which == "critic" else self.policy_args
        with torch.cuda.device(self.env.device):
            return fn(self.env.handle, ctypes.byref(args), self.env._stream())


def steps_of(wide, env, case, **kw):
    return WideSteps(env, case, tiled=True, **kw) if wide else Steps(env, case, tiled=True, **kw)


def run_both_calls(s):
    """The critic step, then the policy step; `ws_critic` is the workspace between the two (both critic passes'
    records: the policy step overwrites the first)."""
    after_critic = s.run(("critic",))["raw"]
    out = s.run(("policy",))["raw"]
    out["ws_critic"] = after_critic["ws"]
    return out


STATE = BLOCKS + ("results", "scalars", "ws_critic", "ws")


# ---------------------------------------------------------------------------------------------
# 1. the target
# ---------------------------------------------------------------------------------------------
class Target:
    """sit_sac_target or sit_sac_target_wide on the case's networks and rows, 8 canaries behind every buffer."""

    def __init__(self, env, case, drawn):
        self.env, self.B = env, case["B"]
        B, dt = self.B, env.dtype
        mask = (np.arange(B) % 3 != 0).astype(np.float32)
        self.inputs = {"actor": with_tail(pack_actor_weights(case["policy"]).numpy(), torch.float32),
                       "critic": with_tail(sac.pack_critic_weights(case["critic"]).numpy(), torch.float32),
                       "alpha": with_tail(np.array([0.2], dtype=np.float32), torch.float32),
                       "next_state": with_tail(case["state"], dt), "reward": with_tail(case["y"], dt),
                       "mask": with_tail(mask, dt), "noise": with_tail(case["eps"], dt)}
        self.out = {k: torch.full((B + 8,), CANARY, dtype=dt, device=DEV) for k in OUTPUTS}
        a = self.args = _lib.SacTargetArgs()
        a.batch, a.seed, a.update, a.gamma, a.reward_scale = B, SEED, UPDATE, GAMMA, 1.5
        a.actor_weights, a.critic_weights, a.alpha = (self.inputs[k].data_ptr() for k in ("actor", "critic", "alpha"))
        a.next_state, a.reward, a.mask = (self.inputs[k].data_ptr() for k in ("next_state", "reward", "mask"))
        a.noise = None if drawn else self.inputs["noise"].data_ptr()
        for k, t in self.out.items():
            setattr(a, k, t.data_ptr())

    def run(self, name):
        before = {k: t.clone() for k, t in self.inputs.items()}
        with torch.cuda.device(self.env.device):
            rc = getattr(self.env.lib, name)(self.env.handle, ctypes.byref(self.args), self.env._stream())
        assert rc == _lib.SIT_OK, self.env.lib.sit_last_error(self.env.handle)
        torch.cuda.synchronize()
        for k, t in self.out.items():
            assert torch.all(t[self.B:] == CANARY), f"{k}: written past row {self.B}"
            assert torch.isfinite(t[:self.B]).all() and torch.all(t[:self.B] != CANARY), k
        for k, t in self.inputs.items():
            assert torch.equal(bits(t), bits(before[k])), f"{k}: an input was written"
        return {k: t[:self.B].clone() for k, t in self.out.items()}


@pytest.mark.parametrize("B", BATCHES)
def test_wide_target_is_the_target(env, B):
    case = case_of(B)
    for drawn in (False, True):
        narrow = Target(env, case, drawn).run("sit_sac_target")
        wide = Target(env, case, drawn).run("sit_sac_target_wide")
        assert_same_bits(wide, narrow, OUTPUTS, f"B={B}, drawn={drawn}")
        if B >= 4:
            assert not torch.all(wide["y"] == torch.from_numpy(case["y"]).to(DEV) * 1.5)   # unmasked rows took a soft value


# ---------------------------------------------------------------------------------------------
# 2. one critic step and one policy step
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
def test_wide_steps_are_the_tiled_steps(env, B):
    case = case_of(B)
    for tune in (True, False):
        for drawn in (False, True):
            tiled = run_both_calls(steps_of(False, env, case, tune=tune, drawn=drawn))
            wide = run_both_calls(steps_of(True, env, case, tune=tune, drawn=drawn))
            assert wide["ws"].numel() == wide["ws_critic"].numel() == 2 * B * ROW        # the records of rows < B
            assert_same_bits(wide, tiled, STATE, f"B={B}, tune={tune}, drawn={drawn}")
            assert wide["results"].numel() == 5 and wide["scalars"].numel() == 4
            assert torch.isfinite(wide["results"]).all() and wide["actor_m"].any() and wide["critic_m"].any()
            assert torch.all(wide["ws_critic"] != CANARY) and torch.all(wide["ws"] != CANARY)
            if not tune:
                assert wide["results"][3] == 0.0 and wide["scalars"][2] == 0.0


# ---------------------------------------------------------------------------------------------
# 3. non-zero moments
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [33, 64])
def test_two_consecutive_steps(env, B):
    case = case_of(B)
    out = {}
    for wide in (False, True):
        s = steps_of(wide, env, case)
        first = run_both_calls(s)
        s.set_step(2)
        out[wide] = (first, run_both_calls(s))
    assert_same_bits(out[True][0], out[False][0], STATE, f"B={B}, t=1")
    assert_same_bits(out[True][1], out[False][1], STATE, f"B={B}, t=2")
    assert not torch.equal(out[True][1]["actor"], out[True][0]["actor"])          # the second step moved on


# ---------------------------------------------------------------------------------------------
# 4. bounds and determinism
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 33, 67])
def test_wide_calls_keep_canaries_and_repeat(env, B):
    case = case_of(B)
    runs = []
    for _ in range(2):
        s = steps_of(True, env, case)
        got = run_both_calls(s)                          # run() checks every canary and the padding
        assert torch.all(s.ws[s.n_ws:] == CANARY)        # the float behind row B - 1's record, where row B would be
        for k in ("critic", "critic_m", "critic_v"):
            assert torch.all(got[k].view(2, CW)[:, CRITIC_SIZE:] == CANARY), k
        assert torch.isfinite(got["ws"]).all() and torch.all(got["ws"] != CANARY)
        runs.append(got)
    for k in runs[0]:
        assert torch.equal(bits(runs[0][k]), bits(runs[1][k])), k


# ---------------------------------------------------------------------------------------------
# 5. rejections
# ---------------------------------------------------------------------------------------------
def test_wide_calls_reject_what_the_plain_calls_reject(env):
    s = steps_of(True, env, case_of(9))
    s.tiled = False                                      # Steps.call(s, ...) is then the plain call
    before = {k: t.clone() for k, t in s.buffers().items()}
    for which in ("critic", "policy"):
        for args, field, value, good in s.invalid_arguments(which):
            setattr(args, field, value)
            wide_rc = s.call(which)
            wide_why = env.lib.sit_last_error(env.handle)
            assert Steps.call(s, which) == wide_rc == _lib.SIT_E_INVALID, (which, field)
            assert env.lib.sit_last_error(env.handle) == wide_why and b"sac" in wide_why, (which, field)
            setattr(args, field, good)
    t = Target(env, case_of(9), drawn=False)
    t_before = {k: v.clone() for k, v in t.out.items()}
    good = {k: getattr(t.args, k) for k in ("batch", "actor_weights", "critic_weights", "alpha", "next_state", "reward",
                                            "mask", "y")}
    cases = [(k, None) for k in good if k != "batch"] + [("batch", 0), ("batch", -1),
                                                          ("actor_weights", good["actor_weights"] + 4),
                                                          ("critic_weights", good["critic_weights"] + 8)]
    with torch.cuda.device(env.device):
        for field, value in cases:
            setattr(t.args, field, value)
            wide_rc = env.lib.sit_sac_target_wide(env.handle, ctypes.byref(t.args), env._stream())
            wide_why = env.lib.sit_last_error(env.handle)
            assert env.lib.sit_sac_target(env.handle, ctypes.byref(t.args), env._stream()) == wide_rc == _lib.SIT_E_INVALID, field
            assert env.lib.sit_last_error(env.handle) == wide_why and b"sac" in wide_why, field
            setattr(t.args, field, good[field])
        for name in ("sit_sac_target_wide", "sit_sac_critic_step_wide", "sit_sac_policy_step_wide"):
            assert getattr(env.lib, name)(env.handle, None, env._stream()) == _lib.SIT_E_INVALID, name
    torch.cuda.synchronize()
    for k, v in s.buffers().items():
        assert torch.equal(bits(v), bits(before[k])), f"{k}: an invalid call wrote"
    for k, v in t.out.items():
        assert torch.equal(bits(v), bits(t_before[k])), f"{k}: an invalid call wrote"
    run_both_calls(s)                                    # and the restored arguments are accepted
    t.run("sit_sac_target_wide")


# ---------------------------------------------------------------------------------------------
# 6. the learner
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
    kw = dict(gradient="hip", weight_gradient="mfma")
    lrn = {m: new_learner(env, row_pass=m, **kw) for m in ("valu", "mfma")}
    mem = {m: device_memory(env) for m in lrn}
    assert lrn["mfma"].row_pass == "mfma" and lrn["valu"].row_pass == "valu"
    assert new_learner(env, **kw).row_pass == "valu"                              # the default
    assert "row_pass" not in lrn["mfma"].state_dict()

    def both(batch, u):
        out = {m: lrn[m].update_parameters(mem[m], batch, u) for m in ("valu", "mfma")}
        assert out["mfma"] is not None and len(out["mfma"]) == 5
        assert out["mfma"] == out["valu"], (batch, u)
        assert blocks_are_the_modules(lrn["mfma"])
        return out["mfma"]

    for u in range(3):
        both(64, u)
    assert_same_learner(lrn["mfma"], lrn["valu"])
    # a checkpoint written in one mode, continued in the other: the same fourth update
    crossed = {}
    for first, second in (("mfma", "valu"), ("valu", "mfma")):
        sd, msd = lrn[first].state_dict(), mem[first].state_dict()
        other = new_learner(env, fresh=True, row_pass=second, **kw)
        other.load_state_dict(sd)
        omem = device_memory(env)
        omem.load_state_dict(msd)
        crossed[second] = (other, other.update_parameters(omem, 64, 3))
    want = both(64, 3)
    assert crossed["valu"][1] == crossed["mfma"][1] == want
    assert_same_learner(crossed["valu"][0], crossed["mfma"][0])
    assert_same_learner(crossed["mfma"][0], lrn["mfma"])
    assert_same_learner(lrn["valu"], lrn["mfma"])
    for u in range(4, 7):                                # a batch that is no multiple of 32: 3 blocks and 4 rows
        both(100, u)
    assert_same_learner(lrn["valu"], lrn["mfma"])
