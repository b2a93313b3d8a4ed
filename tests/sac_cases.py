"""The cases the SAC GPU tests share (tests/test_gpu_sac.py, test_gpu_sac_grad.py, test_gpu_sac_wgrad.py;
tools/sac_bits.py builds its cases here too).  A plain module: everything is built on first use and kept for
the session.

  records / networks / normalised_ring / device_memory   the learner's fixture: the transition records of one
      float64 rollout of 64 envs (synthetic sampler) pushed through a ReplayMemory (so their order is the
      canonical one) and rounded to float32, so that both handles and the float64 reference see the same
      numbers; default-initialised networks under a fixed seed
  new_learner / reference_run / learner_params / learner_err   a SacLearner from those networks, the float64
      reference's run on the same ring, and the error between two runs
  Steps   sit_sac_critic_step and sit_sac_policy_step (or the _tiled calls) through ctypes on buffers with 8
      canary elements behind each; the cases are tests/sac_grad_reference.make_case(B, seed)
"""
import copy
import ctypes
import functools
import math

import numpy as np
import torch

import sac_grad_reference as R
from helpers import OBS_SCALE
from sac_maritime_ast_amd import ReplayMemory, VecMultiShipRLEnv, _lib, make_scenario, replay_reference, sac
from sac_maritime_ast_amd.samplers import GaussianPolicy, pack_actor_weights

DEV = "cuda:0"
CW, AW, ROW = _lib.SIT_CRITIC_WEIGHTS, _lib.SIT_ACTOR_WEIGHTS, _lib.SIT_SAC_WORKSPACE_ROW
CRITIC_SIZE = CW - 3                     # the packed network; 3 padding floats follow
CANARY = -12345.5
NP_REAL = {32: np.float32, 64: np.float64}
GAMMA, SEED, UPDATE = 0.99, 25450, (3 << 32) | 5
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8
# make_case's seed at the batch sizes of test_gpu_sac_grad.py (its docstring: how they were chosen); 2 elsewhere
SEEDS = {1: 1, 7: 1, 8: 2, 9: 2, 64: 2, 67: 2}
LEARNER_KW = dict(gamma=GAMMA, tau=0.005, lr=3e-4, alpha=0.2, automatic_entropy_tuning=True, target_update_interval=1,
                  seed=SEED)


def scaled_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


def bits(a):
    """The bit patterns of a float tensor or array as integers of the same width."""
    if isinstance(a, torch.Tensor):
        return a.contiguous().view(torch.int32 if a.element_size() == 4 else torch.int64)
    return np.asarray(a).view({4: np.uint32, 8: np.uint64}[np.asarray(a).dtype.itemsize])


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


# ---------------------------------------------------------------------------------------------
# the learner's fixture
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def records():
    """>= 256 transition records [n, 24] of a 64-env float64 rollout in canonical order, rounded to float32."""
    e = VecMultiShipRLEnv(scenario=make_scenario(64), precision=64, device=DEV)
    try:
        e.reset()
        e.init_step()
        out = e.rollout(3000, seed=SEED, transition_capacity=4096)
        mem = ReplayMemory(e, 4096)
        mem.push(out)
        n = len(mem)
        rec = mem.ring[:n].cpu().numpy()
    finally:
        e.close()
    print("sac fixture: transition records of the 64-env rollout:", n)
    assert 256 <= n < 4096, n
    return rec.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def networks():
    torch.manual_seed(11)
    return GaussianPolicy(), sac.QNetwork()


def normalised_ring(precision, n_rec=256):
    rec = records()[:n_rec].copy()
    rec[:, 0:10] /= OBS_SCALE
    rec[:, 12:22] /= OBS_SCALE
    rec = rec.astype(np.float32)
    ring = replay_reference(n_rec, NP_REAL[precision], seed=SEED)
    ring.push(rec.astype(NP_REAL[precision]), n_rec)
    return ring


def device_memory(env, n_rec=256):
    ring = normalised_ring(env.precision, n_rec)
    mem = ReplayMemory(env, n_rec, seed=SEED)
    mem.ring.copy_(dev(ring.ring))
    mem.cursor.copy_(dev(ring.cursor))
    return mem


def new_learner(env, fresh=False, **kw):
    """A SacLearner on copies of networks(), or with fresh=True on other initial values."""
    pol, q = networks()
    if fresh:
        torch.manual_seed(99)
        pol, q = GaussianPolicy(), sac.QNetwork()
    return sac.SacLearner(env, copy.deepcopy(pol).to(DEV), critic=copy.deepcopy(q), **{**LEARNER_KW, **kw})


def learner_params(learner):
    """Policy, online and target critic parameters as float64 arrays, in parameters() order."""
    if learner.target == "hip":
        tq = sac.unpack_critic_weights(learner.target_weights.cpu(), sac.QNetwork())
    else:
        tq = learner.target_critic
    return [p.detach().cpu().double().numpy() for m in (learner.policy, learner.critic, tq) for p in m.parameters()]


@functools.lru_cache(maxsize=None)
def reference_run(precision, batch, n_upd, n_more=0):
    """The float64 reference's tuples of n_upd + n_more updates, and its parameters after n_upd and at the end."""
    pol, q = networks()
    ref = sac.sac_update_reference(pol, q, **LEARNER_KW)
    ring = normalised_ring(precision)
    snap = lambda: [p.detach().numpy().copy() for m in (ref.policy, ref.critic, ref.target_critic) for p in m.parameters()]  # noqa: E731
    tuples = [ref.update_parameters(ring, batch, u) for u in range(n_upd)]
    first = snap()
    tuples += [ref.update_parameters(ring, batch, u) for u in range(n_upd, n_upd + n_more)]
    return tuples, first, snap()


def learner_err(tuples, params, ref_tuples, ref_params):
    return {"tuple": scaled_err(tuples, ref_tuples), "params": max(scaled_err(a, b) for a, b in zip(params, ref_params))}


def blocks_are_the_modules(learner):
    return (torch.equal(learner.actor_weights, pack_actor_weights(learner.policy))
            and torch.equal(learner.online_weights, sac.pack_critic_weights(learner.critic)))


# ---------------------------------------------------------------------------------------------
# the two gradient calls on canaried buffers
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_of(B):
    return R.make_case(B, SEEDS.get(B, 2))


def adam_scalars(t=1, lr=R.LR):
    return _lib.SacAdam(lr, BETA1, BETA2, ADAM_EPS, 1.0 - BETA1 ** t, 1.0 - BETA2 ** t)


def with_tail(a, dtype):
    """A device tensor of `a` with 8 canary elements behind it."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype).reshape(-1)
    return torch.cat([t, torch.full((8,), CANARY, dtype=dtype)]).to(DEV)


class Steps:
    """sit_sac_critic_step and sit_sac_policy_step (tiled: the _tiled calls) through ctypes on buffers with 8
    canary elements behind each, the critic blocks' padding set to the canary as well, and zero moments."""

    def __init__(self, env, case, alpha=R.ALPHA0, tune=True, drawn=False, seed=SEED, update=UPDATE, tiled=False):
        self.env, self.B, self.tiled = env, case["B"], tiled
        B, dt = self.B, env.dtype
        cw = sac.pack_critic_weights(case["critic"]).numpy().copy()
        cw.reshape(2, CW)[:, CRITIC_SIZE:] = CANARY
        zero_c = np.zeros(2 * CW, dtype=np.float32)
        zero_c.reshape(2, CW)[:, CRITIC_SIZE:] = CANARY
        self.blocks = {"critic": with_tail(cw, torch.float32), "critic_m": with_tail(zero_c, torch.float32),
                       "critic_v": with_tail(zero_c, torch.float32),
                       "actor": with_tail(pack_actor_weights(case["policy"]).numpy(), torch.float32),
                       "actor_m": with_tail(np.zeros(AW, dtype=np.float32), torch.float32),
                       "actor_v": with_tail(np.zeros(AW, dtype=np.float32), torch.float32)}
        self.n_ws = 2 * B * ROW
        self.ws = torch.full((self.n_ws + 8,), CANARY, dtype=torch.float32, device=DEV)
        self.results = torch.full((5 + 8,), CANARY, dtype=torch.float32, device=DEV)
        log_alpha = np.float32(math.log(alpha))
        self.scalars = with_tail(np.array([np.exp(np.float64(log_alpha)), log_alpha, 0.0, 0.0]), torch.float32)
        self.inputs = {k: with_tail(case[k], dt) for k in ("state", "action", "y", "eps")}
        c = self.critic_args = _lib.SacCriticStepArgs()
        c.batch, c.workspace_floats, c.adam = B, self.n_ws, adam_scalars()
        c.critic_weights, c.critic_m, c.critic_v = (self.blocks[k].data_ptr() for k in ("critic", "critic_m", "critic_v"))
        c.state, c.action, c.y = (self.inputs[k].data_ptr() for k in ("state", "action", "y"))
        c.workspace, c.results = self.ws.data_ptr(), self.results.data_ptr()
        p = self.policy_args = _lib.SacPolicyStepArgs()
        p.batch, p.tune, p.workspace_floats, p.seed, p.update = B, int(tune), self.n_ws, seed, update
        p.target_entropy, p.adam, p.alpha_adam = R.TARGET_ENTROPY, adam_scalars(), adam_scalars()
        p.actor_weights, p.actor_m, p.actor_v = (self.blocks[k].data_ptr() for k in ("actor", "actor_m", "actor_v"))
        p.critic_weights = self.blocks["critic"].data_ptr()
        s = self.scalars.data_ptr()
        p.alpha, p.log_alpha, p.log_alpha_m, p.log_alpha_v = s, s + 4, s + 8, s + 12
        p.state, p.noise = self.inputs["state"].data_ptr(), None if drawn else self.inputs["eps"].data_ptr()
        p.workspace, p.results = self.ws.data_ptr(), self.results.data_ptr()

    def set_step(self, t):
        self.critic_args.adam = adam_scalars(t)
        self.policy_args.adam = self.policy_args.alpha_adam = adam_scalars(t)

    def call(self, which):
        fn = getattr(self.env.lib, f"sit_sac_{which}_step" + ("_tiled" if self.tiled else ""))
        args = self.critic_args if which == "critic" else self.policy_args
        with torch.cuda.device(self.env.device):
            return fn(self.env.handle, ctypes.byref(args), self.env._stream())

    def buffers(self):
        return {**self.blocks, "ws": self.ws, "results": self.results, "scalars": self.scalars, **self.inputs}

    def check_canaries(self):
        torch.cuda.synchronize()
        for k, t in self.buffers().items():
            assert torch.all(t[-8:] == CANARY), f"{k}: written past its end"
        for k in ("critic", "critic_m", "critic_v"):
            assert torch.all(self.blocks[k][:2 * CW].view(2, CW)[:, CRITIC_SIZE:] == CANARY), f"{k}: padding written"

    def run(self, steps=("critic", "policy")):
        for which in steps:
            assert self.call(which) == _lib.SIT_OK, self.env.lib.sit_last_error(self.env.handle)
        self.check_canaries()
        return self.read()

    def read(self):
        torch.cuda.synchronize()
        host = {k: t[:-8].cpu() for k, t in self.buffers().items()}
        pol, q = GaussianPolicy(), sac.QNetwork()
        views = lambda k, layers: [v.double().numpy().copy() for v in sac.block_views(host[k], layers)]  # noqa: E731
        cl, al = sac._critic_layers(q), [sac._actor_layers(pol)]
        g = float(np.float32(1.0 - BETA1))       # m = (1 - beta1) g in float32
        sc = host["scalars"].double().numpy()
        return {"critic_grads": [m / g for m in views("critic_m", cl)], "critic_params": views("critic", cl),
                "policy_grads": [m / g for m in views("actor_m", al)], "policy_params": views("actor", al),
                "critic_v": views("critic_v", cl), "policy_v": views("actor_v", al),
                "results": host["results"].double().numpy(), "alpha": sc[0], "log_alpha": sc[1], "alpha_grad": sc[2] / g,
                "raw": host}

    def invalid_arguments(self, which):
        """(args, field, invalid value, valid value) of the `which` call: what both its entry points reject."""
        args = self.critic_args if which == "critic" else self.policy_args
        good = {k: getattr(args, k) for k, _ in args._fields_ if k not in ("adam", "alpha_adam")}
        block = "critic_weights" if which == "critic" else "actor_weights"
        moment = "critic_m" if which == "critic" else "actor_v"
        cases = [(k, None) for k in (block, moment, "state", "workspace", "results")]
        cases += [("batch", 0), ("batch", -1), (block, good[block] + 4), (moment, good[moment] + 8),
                  ("workspace_floats", self.n_ws - 1)]
        if which == "policy":
            cases += [("critic_weights", None), ("critic_weights", good["critic_weights"] + 4), ("alpha", None),
                      ("log_alpha", None)]
        else:
            cases += [("action", None), ("y", None)]
        return [(args, field, value, good[field]) for field, value in cases]
