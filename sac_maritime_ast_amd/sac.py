"""The SAC learner: ``agent.update_parameters(memory, batch_size, updates)`` of
``test_beds/main_ast.py:350-362``.

The reference's ``ast_core/algorithms/sac.py`` is an empty file; ``main_ast.py:41-90`` fixes the
algorithm: twin Q networks of hidden size 256, gamma 0.99, tau 0.005, lr 3e-4, alpha 0.2,
automatic entropy tuning, target_update_interval 1, batch_size 64 -- standard SAC (Haarnoja et al.
2018) with the actor of ``samplers.GaussianPolicy``.

One update has two halves.  The gradient half (two critic losses, the policy loss, the temperature
loss and their Adam steps) is PyTorch autograd by default, or with ``SacLearner(gradient="hip")`` the
HIP calls ``sit_sac_critic_step`` / ``sit_sac_policy_step`` (csrc/sit_sac_grad.h: forward and backward
passes per row, weight gradients fused with Adam), which update the packed blocks in place; the
networks' parameters are then views into those blocks.  ``weight_gradient="mfma"`` swaps both for their
``_tiled`` forms (csrc/sit_sac_wgrad.h), which form the weight gradients as 32 x 32 MFMA tiles over the
batch instead of one serial sum per element: the same bits, and the choice for batches in the thousands.
``row_pass="mfma"`` on top of that swaps the three row kernels for their ``_wide`` forms (csrc/sit_sac_rows.h:
32 rows per block, both 256 x 256 products of a network pass as MFMA chains): the same bits again, and
faster from batches of about 16 384.
The no-gradient half is inference only and is HIP
(csrc/sit_sac.h, include/sit.h "SAC learner"): ``sit_sac_target`` evaluates the actor at next_state
with its log-probability, both target critics at (next_state, a') and the TD target in one kernel, and
``sit_sac_polyak`` moves the packed target block towards the online critics in another.
``SacLearner(target="torch")`` computes the same formulas with PyTorch ops (the A/B, and the path for
architectures ``pack_actor_weights`` / ``pack_critic_weights`` decline).

``sac_target_reference`` is the executable specification of ``sit_sac_target`` in float64 NumPy,
noise draw included; ``sac_update_reference`` is a whole update in float64 PyTorch on the CPU.

``update_many`` (gradient="hip") runs n updates in one call, ``sit_sac_updates``: the update number, the Adam
step counts and the results row come from a clock in device memory that the kernels advance themselves
(csrc/sit_sac_clock.h), so nothing is read back, a HIP graph of the call replays as the next n updates, and
with ``PolicySampler.share_weights`` a whole "rollout, push, n updates" iteration is one graph.  The bits are
those of the same number of ``update_parameters`` calls; ``adam_scalars_reference`` is the specification of the
clock's Adam scalars.

``SacLearner(..., obs_norm=norm)`` (an ``obsnorm.ObsNormalizer``): every minibatch is drawn normalised
(``ReplayMemory.sample(normalizer=norm)``), and every update call ends by folding ``actor_weights`` into
``serving_weights`` on the stream (``sit_obsnorm_fold``), the block the samplers serve from; no learner kernel
changes.  ``SacUpdateReference(obs_norm=ObsNormReference)`` normalises its float64 batches with the same float32
affine values.

Not included: HIP gradients for other architectures, prioritised replay, n-step returns,
multi-rank learners, hyper-parameter schedules inside a graph, a device-side gate
on len(memory).
"""
from __future__ import annotations

import copy
import math
from ctypes import byref, c_void_p

import numpy as np
import torch
from torch import nn

from . import _lib
from .replay import philox4x32_10
from .samplers import EPS, LOG_SIG_CAP_MAX, LOG_SIG_CAP_MIN, block_segments, pack_actor_weights

OBS, H = _lib.SIT_OBS_DIM, _lib.SIT_ACTOR_HIDDEN
CRITIC_IN = _lib.SIT_CRITIC_INPUT
CRITIC_WEIGHTS = _lib.SIT_CRITIC_WEIGHTS
TARGET_NOISE_TAG = 0x5441      # counter word 1 of sit_sac_target's draw
POLICY_NOISE_TAG = 0x5049      # counter word 1 of the policy loss's draw
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
_M32 = 0xFFFFFFFF


class QNetwork(nn.Module):
    """Twin critic: two MLPs (obs + action) 11 -> 256 -> ReLU -> 256 -> ReLU -> 1 (main_ast.py:67,
    ``hidden_size`` 256)."""

    def __init__(self, obs_dim: int = OBS, act_dim: int = 1, hidden: int = H):
        super().__init__()

        def mlp():
            return nn.Sequential(nn.Linear(obs_dim + act_dim, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU(),
                                 nn.Linear(hidden, 1))
        self.q1, self.q2 = mlp(), mlp()

    def forward(self, state: torch.Tensor, action: torch.Tensor):
        x = torch.cat([state, action.reshape(state.shape[0], -1)], dim=-1)
        return self.q1(x)[:, 0], self.q2(x)[:, 0]


def _critic_layers(q: nn.Module):
    """[(l1, l2, l3) of q1, of q2] when q is the twin 11 -> 256 -> 256 -> 1 ReLU critic, else None."""
    out = []
    for net in (getattr(q, "q1", None), getattr(q, "q2", None)):
        if not isinstance(net, nn.Sequential) or len(net) != 5:
            return None
        l1, r1, l2, r2, l3 = net
        ok = (all(isinstance(m, nn.Linear) and m.bias is not None for m in (l1, l2, l3))
              and isinstance(r1, nn.ReLU) and isinstance(r2, nn.ReLU)
              and tuple(l1.weight.shape) == (H, CRITIC_IN) and tuple(l2.weight.shape) == (H, H)
              and tuple(l3.weight.shape) == (1, H))
        if not ok:
            return None
        out.append((l1, l2, l3))
    return out


def _block_and_parameters(block: torch.Tensor, layers):
    """(view into the packed block, parameter) pairs in ``parameters()`` order; `layers` as for ``block_views``."""
    flat = block.view(-1)
    for c, net in enumerate(layers):
        n_in, n_out = net[0].weight.shape[1], net[2].weight.shape[0]
        for layer, name, seg in block_segments(flat, n_in, n_out, c * CRITIC_WEIGHTS):
            yield seg, getattr(net[layer], name)


def pack_critic_weights(q: nn.Module, out: torch.Tensor | None = None) -> torch.Tensor | None:
    """The float32 block of sit_sac_target's critics (include/sit.h: two SIT_CRITIC_WEIGHTS blocks, Q1's
    then Q2's, each W1 [256][11], b1, W2^T, b2, W3, b3 and zero padding to a multiple of 4 floats) from a
    ``QNetwork``, or None for any other architecture.  With `out` the parameters are copied in place,
    one copy per parameter; the padding is left as it is."""
    layers = _critic_layers(q)
    if layers is None:
        return None
    with torch.no_grad():
        if out is None:
            p = next(q.parameters())
            out = torch.zeros(2 * CRITIC_WEIGHTS, dtype=torch.float32, device=p.device)
        elif out.numel() != 2 * CRITIC_WEIGHTS or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"pack_critic_weights: out must be a contiguous float32 tensor of {2 * CRITIC_WEIGHTS} "
                             f"elements (got {tuple(out.shape)} {out.dtype}, contiguous={out.is_contiguous()})")
        for seg, p in _block_and_parameters(out, layers):
            seg.copy_(p.detach())
    return out


def unpack_critic_weights(block: torch.Tensor, q: nn.Module) -> nn.Module:
    """The inverse of ``pack_critic_weights``: the block's values into q's parameters."""
    layers = _critic_layers(q)
    if layers is None or block.numel() != 2 * CRITIC_WEIGHTS:
        raise ValueError("unpack_critic_weights: a twin 11 -> 256 -> 256 -> 1 critic and its packed block are required")
    with torch.no_grad():
        for seg, p in _block_and_parameters(block.reshape(-1), layers):
            p.copy_(seg)
    return q


def _actor_layers(policy: nn.Module):
    """(l1, l2, l3) when policy is the reference's actor (``pack_actor_weights`` accepts it), else None."""
    net = getattr(policy, "net", None)
    if net is None or pack_actor_weights(policy) is None:
        return None
    return net[0], net[2], net[4]


def block_views(block: torch.Tensor, layers) -> list:
    """Views into a packed block (or a moment block of the same layout), one per parameter in
    ``parameters()`` order and of the parameter's shape: `layers` is ``[(l1, l2, l3)]`` of the actor or
    ``_critic_layers(q)`` of the twin critic.  l2.weight's view is the transpose of its W2^T segment.
    layers None: the block is one parameter by itself (log_alpha's moments)."""
    return [block] if layers is None else [seg for seg, _ in _block_and_parameters(block, layers)]


def bind_parameters(block: torch.Tensor, layers) -> list:
    """Make the layers' parameters views into `block` (which must hold their values already:
    ``pack_actor_weights`` / ``pack_critic_weights``).  The Parameter objects stay the same; an in-place
    write to the block is a write to the module.  Returns the parameters, in ``parameters()`` order."""
    params = [p for ls in layers for l in ls for p in (l.weight, l.bias)]
    for p, v in zip(params, block_views(block, layers)):
        p.data = v
    return params


def touch_parameters(params) -> None:
    """Bump the version counters of parameters whose storage a kernel has written, so that change
    detection by ``_version`` (``PolicySampler.launch``) sees the write."""
    torch.autograd.graph.increment_version(list(params))


def moments_to_adam_state(m: torch.Tensor, v: torch.Tensor, layers, step: int) -> dict:
    """``torch.optim.Adam.state_dict()["state"]`` of packed moment blocks: per parameter index step,
    exp_avg, exp_avg_sq (contiguous, the parameter's shape).  Empty before the first step, as torch's."""
    if step <= 0:
        return {}
    return {i: {"step": torch.tensor(float(step)), "exp_avg": a.clone(memory_format=torch.contiguous_format),
                "exp_avg_sq": b.clone(memory_format=torch.contiguous_format)}
            for i, (a, b) in enumerate(zip(block_views(m, layers), block_views(v, layers)))}


def adam_state_to_moments(state: dict, m: torch.Tensor, v: torch.Tensor, layers) -> int:
    """The inverse: fill the packed moment blocks from an Adam state (zeros when it is empty) and return
    the step count."""
    with torch.no_grad():
        m.zero_()
        v.zero_()
        if not state:
            return 0
        steps = set()
        for i, (a, b) in enumerate(zip(block_views(m, layers), block_views(v, layers))):
            st = state[i]
            a.copy_(st["exp_avg"])
            b.copy_(st["exp_avg_sq"])
            steps.add(int(st["step"]))
        if len(steps) != 1:
            raise ValueError(f"adam_state_to_moments: parameters at different steps {sorted(steps)}")
        return steps.pop()


# ---------------------------------------------------------------------------------------------
# noise: Philox4x32-10 and the Box-Muller step of the policy's event noise (csrc/sit_device.h)
# ---------------------------------------------------------------------------------------------
def sac_noise(seed: int, rows, update: int, tag: int = TARGET_NOISE_TAG) -> np.ndarray:
    """Standard normals (float64) of Philox4x32-10(key = seed, ctr = (row, tag, update lo, update hi)):
    u1 in (0, 1] and u2 in [0, 1) from 53 bits each, sqrt(-2 log u1) cos(2 pi u2).  tag 0x5441 is
    sit_sac_target's device draw."""
    rows = np.asarray(rows, dtype=np.uint64)
    seed, update = int(seed) & 0xFFFFFFFFFFFFFFFF, int(update) & 0xFFFFFFFFFFFFFFFF
    full = lambda v: np.full(rows.shape, v, dtype=np.uint64)  # noqa: E731
    c = philox4x32_10((rows, full(tag), full(update & _M32), full(update >> 32)), (seed & _M32, seed >> 32))
    f = [x.astype(np.float64) for x in ((c[0] >> np.uint32(5)), (c[1] >> np.uint32(6)), (c[2] >> np.uint32(5)),
                                        (c[3] >> np.uint32(6)))]
    u1 = (f[0] * 67108864.0 + f[1] + 1.0) * (1.0 / 9007199254740992.0)
    u2 = (f[2] * 67108864.0 + f[3]) * (1.0 / 9007199254740992.0)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def policy_noise(seed: int, update: int, batch: int) -> np.ndarray:
    """The policy loss's reparameterisation noise of one update: float64 [batch], a function of
    (seed, update) that a device learner and a reference learner share."""
    return sac_noise(seed, np.arange(batch), update, POLICY_NOISE_TAG)


def adam_scalars_reference(lr: float, beta1: float, beta2: float, eps: float, t) -> np.ndarray:
    """The six float32 scalars of Adam step(s) `t` >= 1 as sit_sac_updates' clock forms them (include/sit.h):
    [..., 6] = one_minus_beta1, beta2, one_minus_beta2, step_size, sqrt_bias2, eps.  beta^t is a product by
    repeated squaring in IEEE double, then step_size = float32(lr / (1 - beta1^t)) and sqrt_bias2 =
    float32(sqrt(1 - beta2^t)); `t` may be an integer or an integer array."""
    t = np.asarray(t, dtype=np.int64)
    if (t < 1).any():
        raise ValueError("adam_scalars_reference: t must be at least 1")

    def pow_sq(beta):
        r, b, n = np.ones(t.shape, dtype=np.float64), np.full(t.shape, beta, dtype=np.float64), t.copy()
        with np.errstate(under="ignore"):
            while n.any():
                r = np.where(n & 1, r * b, r)
                b = b * b
                n >>= 1
        return r
    bias1, bias2 = 1.0 - pow_sq(float(beta1)), 1.0 - pow_sq(float(beta2))
    out = np.empty(t.shape + (6,), dtype=np.float32)
    out[..., 0] = np.float32(1.0 - float(beta1))
    out[..., 1] = np.float32(float(beta2))
    out[..., 2] = np.float32(1.0 - float(beta2))
    out[..., 3] = (float(lr) / bias1).astype(np.float32)
    out[..., 4] = np.sqrt(bias2).astype(np.float32)
    out[..., 5] = np.float32(float(eps))
    return out


# ---------------------------------------------------------------------------------------------
# the specification of sit_sac_target
# ---------------------------------------------------------------------------------------------
def _mlp64(w: np.ndarray, n_in: int, n_out: int, x: np.ndarray) -> np.ndarray:
    """A packed (n_in -> 256 -> 256 -> n_out) block applied to x [B, n_in] in float64."""
    w1, b1, w2, b2, w3, b3 = (seg for _, _, seg in block_segments(np.asarray(w, dtype=np.float64), n_in, n_out))
    h = np.maximum(x @ w1.T + b1, 0.0)
    h = np.maximum(h @ w2.T + b2, 0.0)
    return h @ w3.T + b3


def log_one_minus_tanh_sq(x):
    """log(1 - tanh(x)^2 + 1e-6) from x without cancellation: 1 - tanh(x)^2 = 4 (em + 1) / (em + 2)^2 with
    em = expm1(2 |x|).  (1 - a * a with a = tanh(x) loses every digit once a rounds to 1.)  NumPy arrays
    or torch tensors, in their own precision."""
    if isinstance(x, torch.Tensor):
        em = torch.expm1(2.0 * x.abs().clamp(max=40.0))
        rc = 1.0 / (em + 2.0)
        return torch.log(4.0 * ((em + 1.0) * rc) * rc + EPS)
    em = np.expm1(2.0 * np.minimum(np.abs(x), 300.0))
    rc = 1.0 / (em + 2.0)
    return np.log(4.0 * ((em + 1.0) * rc) * rc + EPS)


def sac_target_reference(actor_weights, critic_weights, next_state, reward, mask, *, alpha: float, gamma: float,
                         reward_scale: float = 1.0, noise=None, seed: int = 0, update: int = 0) -> dict:
    """sit_sac_target (include/sit.h "SAC learner") in float64 NumPy, from the packed float32 blocks.
    noise None: the device draw, ``sac_noise(seed, row, update)``.  Returns y, next_action, next_logp, q1,
    q2 (and noise, x: the draw and the pre-squash sample), each float64 [B]."""
    as64 = lambda a: np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)  # noqa: E731
    aw, cw = as64(actor_weights).reshape(-1), as64(critic_weights).reshape(-1)
    if aw.size != _lib.SIT_ACTOR_WEIGHTS or cw.size != 2 * CRITIC_WEIGHTS:
        raise ValueError("sac_target_reference: packed actor and two-critic blocks are required")
    ns = as64(next_state).reshape(-1, OBS)
    B = ns.shape[0]
    reward, mask = as64(reward).reshape(B), as64(mask).reshape(B)
    eps = sac_noise(seed, np.arange(B), update) if noise is None else as64(noise).reshape(B)
    head = _mlp64(aw, OBS, 2, ns)
    mu, ls = head[:, 0], np.clip(head[:, 1], LOG_SIG_CAP_MIN, LOG_SIG_CAP_MAX)
    x = np.exp(ls) * eps + mu
    a = np.tanh(x)
    logp = -0.5 * eps * eps - ls - HALF_LOG_2PI - log_one_minus_tanh_sq(x)
    xin = np.concatenate([ns, a[:, None]], axis=1)
    q1 = _mlp64(cw[:CRITIC_WEIGHTS], CRITIC_IN, 1, xin)[:, 0]
    q2 = _mlp64(cw[CRITIC_WEIGHTS:], CRITIC_IN, 1, xin)[:, 0]
    y = reward_scale * reward + mask * gamma * (np.minimum(q1, q2) - float(alpha) * logp)
    return {"y": y, "next_action": a, "next_logp": logp, "q1": q1, "q2": q2, "noise": eps, "x": x}


def torch_target(policy, target_critic, next_state, reward, mask, eps, alpha, gamma, reward_scale=1.0) -> dict:
    """The formulas of sit_sac_target with PyTorch ops, in the dtype and on the device of the networks
    and inputs (no gradients): y, next_action, next_logp, q1, q2."""
    with torch.no_grad():
        head = policy.net(next_state)
        mu, ls = head[:, 0], head[:, 1].clamp(LOG_SIG_CAP_MIN, LOG_SIG_CAP_MAX)
        x = torch.addcmul(mu, ls.exp(), eps)
        a = torch.tanh(x)
        logp = -0.5 * eps * eps - ls - HALF_LOG_2PI - log_one_minus_tanh_sq(x)
        q1, q2 = target_critic(next_state, a[:, None])
        y = reward_scale * reward + mask * gamma * (torch.min(q1, q2) - alpha * logp)
        return {"y": y, "next_action": a, "next_logp": logp, "q1": q1, "q2": q2}


def _sample(memory, batch_size, normalizer=None):
    """One minibatch of a ReplayMemory (device tensors) or a ReplayReference (NumPy) as [B, ...] items."""
    b = memory.sample(batch_size) if normalizer is None else memory.sample(batch_size, normalizer=normalizer)
    return {k: b[k][0] for k in ("state", "action", "reward", "next_state", "mask")}


def _gradient_half(pol, critic, optims, log_alpha, alpha, auto, batch, y, eps_pi, target_entropy=-1.0):
    """The gradient half of one update, shared by the learner and the float64 reference: the two critic
    MSE losses and their Adam step, the policy loss mean(alpha logp - min(Q1, Q2)(s, pi(s))) and its
    step, the temperature loss -mean(log_alpha (logp + target_entropy).detach()) and its step.
    Returns the four losses (tensors) and the new alpha (a tensor when tuned)."""
    state, action = batch["state"], batch["action"]
    q1, q2 = critic(state, action)
    l1, l2 = nn.functional.mse_loss(q1, y), nn.functional.mse_loss(q2, y)
    optims["critic"].zero_grad(set_to_none=True)
    (l1 + l2).backward()
    optims["critic"].step()
    pi, logp, _, _ = pol(state, eps_pi[:, None])
    q1p, q2p = critic(state, pi)
    lp = (alpha * logp - torch.min(q1p, q2p)).mean()
    optims["policy"].zero_grad(set_to_none=True)
    lp.backward()
    optims["policy"].step()
    if auto:
        la = -(log_alpha * (logp + target_entropy).detach()).mean()
        optims["alpha"].zero_grad(set_to_none=True)
        la.backward()
        optims["alpha"].step()
        alpha = log_alpha.detach().exp()
    else:
        la = torch.zeros((), dtype=l1.dtype, device=l1.device)
    return l1.detach(), l2.detach(), lp.detach(), la.detach(), alpha


class _SacState:
    """What ``SacLearner`` and ``SacUpdateReference`` set up alike: the hyper-parameters, log_alpha and alpha
    (tensors of one element in the networks' dtype and on their device) and the Adam optimisers."""

    def _setup(self, dtype, device, *, gamma, tau, lr, alpha, automatic_entropy_tuning, target_update_interval,
               reward_scale, seed):
        self.gamma, self.tau, self.reward_scale = float(gamma), float(tau), float(reward_scale)
        self.target_update_interval, self.seed = int(target_update_interval), int(seed)
        self.auto = bool(automatic_entropy_tuning)
        self.log_alpha = torch.full((1,), math.log(alpha), dtype=dtype, device=device, requires_grad=self.auto)
        self.alpha = self.log_alpha.detach().exp()
        self.optims = {"critic": torch.optim.Adam(self.critic.parameters(), lr=lr),
                       "policy": torch.optim.Adam(self.policy.parameters(), lr=lr)}
        if self.auto:
            self.optims["alpha"] = torch.optim.Adam([self.log_alpha], lr=lr)

    def _polyak_torch(self):
        with torch.no_grad():
            for t, p in zip(self.target_critic.parameters(), self.critic.parameters()):
                t.add_(p - t, alpha=self.tau)


class SacLearner(_SacState):
    """SAC updates on the device of one ``VecMultiShipRLEnv`` from its ``ReplayMemory``.

    `policy` is the ``GaussianPolicy`` the samplers serve (float32, on the env's device); the learner
    owns the twin critic (``critic``: a ``QNetwork`` to start from, default a fresh one), the target
    critics (copies of the online critics at construction), the three Adam optimisers and log_alpha.
    target="hip": the no-gradient half is ``sit_sac_target`` / ``sit_sac_polyak`` and the targets live
    only as the packed block ``target_weights``; it needs the reference's architectures
    (``pack_actor_weights`` / ``pack_critic_weights``) and raises for others -- pick target="torch" for
    those, which computes the same formulas with PyTorch ops on a target ``QNetwork``.
    gradient="torch" (the default): the gradient half is autograd and three ``torch.optim.Adam``.
    gradient="hip": it is ``sit_sac_critic_step`` / ``sit_sac_policy_step``; it needs target="hip" and the
    reference's architectures.  The packed blocks ``actor_weights`` and ``online_weights`` are then the
    master copy of the parameters, the Adam moments are packed blocks of the same layout, and the
    parameters of `policy` and ``critic`` are views into the blocks (``bind_parameters``), so both modules
    hold the current values after every update without a copy.  The policy noise is drawn on the device
    from (seed, update) (``policy_noise`` is its specification).  A checkpoint of either mode loads into
    the other.
    weight_gradient="sum" (the default): the plain calls, whose Adam kernel sums each element's gradient
    over the rows in one thread.  weight_gradient="mfma": ``sit_sac_critic_step_tiled`` /
    ``sit_sac_policy_step_tiled``, the same sums as MFMA tiles with the batch as the k index; it needs
    gradient="hip", gives the same bits and keeps the same state, so checkpoints do not see it.
    row_pass="valu" (the default): the row kernels of ``sit_sac_target`` and the step calls, 8 rows per block
    on the VALU.  row_pass="mfma": ``sit_sac_target_wide`` / ``sit_sac_critic_step_wide`` /
    ``sit_sac_policy_step_wide`` (csrc/sit_sac_rows.h), 32 rows per block with the two 256 x 256 products of
    a network pass on the matrix cores; it needs weight_gradient="mfma", gives the same bits and keeps the
    same state, so checkpoints do not see it either.  It is the mode for large batches.

    ``actor_weights`` is the packed actor block sit_sac_target reads, repacked in place at the end of
    every update.  A ``PolicySampler`` built on the same `policy` keeps a block of its own: call its
    ``refresh_weights()`` after an update (its ``launch()`` does so by itself when the parameters
    changed, except inside a HIP-graph replay); with gradient="hip" its ``share_weights(learner.actor_weights)``
    makes it serve from this block instead.

    ``update_many(memory, batch_size, n_updates)`` (gradient="hip"): n updates in one ``sit_sac_updates`` call
    driven by ``clock``, the int64 device clock (words 0..4: update, critic_steps, policy_steps, alpha_steps,
    results_written); the five results of each go to a ring of `results_capacity` rows that ``results()``
    reads.  ``update_parameters``, ``update_many``, graph replays, ``state_dict`` and ``load_state_dict`` may be
    mixed freely: the clock's step words are the master copy once ``update_many`` has run, and the host's
    counts are reconciled with them (one read) where they are needed.

    obs_norm (an ``ObsNormalizer`` of the same env): ``update_parameters`` (all modes) and ``update_many`` draw
    normalised minibatches, and each ends by folding ``actor_weights`` into ``serving_weights`` on the stream, so
    the fold is part of a captured ``update_many``; serve with ``sampler.share_weights(learner.serving_weights)``.
    Update the normaliser after the push and before the learner's call: the minibatches and the fold then use
    one affine.  ``state_dict`` is unchanged; the normaliser checkpoints itself."""

    def __init__(self, env, policy: nn.Module, *, gamma: float = 0.99, tau: float = 0.005, lr: float = 3e-4,
                 alpha: float = 0.2, automatic_entropy_tuning: bool = True, target_update_interval: int = 1,
                 reward_scale: float = 1.0, seed: int = 25450, target: str = "hip", critic: nn.Module | None = None,
                 gradient: str = "torch", weight_gradient: str = "sum", row_pass: str = "valu",
                 results_capacity: int = 1024, obs_norm=None):
        if target not in ("hip", "torch"):
            raise ValueError("target must be 'hip' or 'torch'")
        if gradient not in ("hip", "torch"):
            raise ValueError("gradient must be 'hip' or 'torch'")
        if gradient == "hip" and target != "hip":
            raise ValueError("gradient='hip' needs target='hip'")
        if weight_gradient not in ("sum", "mfma"):
            raise ValueError("weight_gradient must be 'sum' or 'mfma'")
        if weight_gradient == "mfma" and gradient != "hip":
            raise ValueError("weight_gradient='mfma' needs gradient='hip'")
        if row_pass not in ("valu", "mfma"):
            raise ValueError("row_pass must be 'valu' or 'mfma'")
        if row_pass == "mfma" and weight_gradient != "mfma":
            raise ValueError("row_pass='mfma' needs weight_gradient='mfma'")
        self.weight_gradient, self.row_pass = weight_gradient, row_pass
        self.env, self.policy, self.target, self.gradient = env, policy, target, gradient
        self.lr, self.target_entropy = float(lr), -1.0
        dev = env.device
        self.critic = (critic if critic is not None else QNetwork()).to(device=dev, dtype=torch.float32)
        # (alpha: float32[1] on the device, where sit_sac_target reads it)
        self._setup(torch.float32, dev, gamma=gamma, tau=tau, lr=lr, alpha=alpha,
                    automatic_entropy_tuning=automatic_entropy_tuning, target_update_interval=target_update_interval,
                    reward_scale=reward_scale, seed=seed)
        self._ready = False
        self._out = {}
        self.obs_norm, self._serving = obs_norm, None
        if obs_norm is not None:
            affine = getattr(obs_norm, "affine", None)
            if getattr(obs_norm, "env", None) is not env or not isinstance(affine, torch.Tensor):
                raise ValueError("obs_norm: an ObsNormalizer of the learner's env is required")
        if target == "hip":
            self.actor_weights = pack_actor_weights(policy)
            self.online_weights = pack_critic_weights(self.critic)
            if self.actor_weights is None or self.online_weights is None:
                raise ValueError("target='hip' needs the reference's actor (10 -> 256 -> 256 -> 2) and twin critic "
                                 "(11 -> 256 -> 256 -> 1); use target='torch' for other architectures")
            if self.actor_weights.device != dev or self.actor_weights.dtype != torch.float32:
                raise ValueError(f"target='hip' needs a float32 policy on {dev}")
            self.target_weights = self.online_weights.clone()
            self.target_critic = None
        else:
            self.actor_weights = pack_actor_weights(policy)      # None for other architectures
            self.online_weights = self.target_weights = None
            self.target_critic = copy.deepcopy(self.critic).requires_grad_(False)
        if gradient == "hip":
            self._layers = {"policy": [_actor_layers(self.policy)], "critic": _critic_layers(self.critic), "alpha": None}
            self._blocks = {"policy": self.actor_weights, "critic": self.online_weights}
            self._params = (bind_parameters(self.actor_weights, self._layers["policy"])
                            + bind_parameters(self.online_weights, self._layers["critic"]))
            self._m = {k: torch.zeros_like(b) for k, b in self._blocks.items()}
            self._v = {k: torch.zeros_like(b) for k, b in self._blocks.items()}
            self._m["alpha"], self._v["alpha"] = torch.zeros_like(self.alpha), torch.zeros_like(self.alpha)
            self._steps = {k: 0 for k in self.optims}
            self._results = torch.zeros(5, dtype=torch.float32, device=dev)
            self._ws = None
            # update_many: the device clock, the results ring and the minibatch buffers per (batch, n_updates)
            if int(results_capacity) <= 0:
                raise ValueError("results_capacity must be positive")
            self.clock = torch.zeros(_lib.SIT_SAC_CLOCK_WORDS, dtype=torch.int64, device=dev)
            self._ring = torch.zeros((int(results_capacity), 5), dtype=torch.float32, device=dev)
            self._many = {}
            self._next_update = 0         # what the clock's update word starts from when update_many first runs
            self._clocked = False         # update_many has run: the clock's step words are the master copy
            self._clock_dirty = False     # clocked work since the host's counts were last reconciled
            self._captured = False        # an update_many was captured: replays advance the clock unseen
        if obs_norm is not None:
            if self.actor_weights is None:
                raise ValueError("obs_norm needs the reference's actor (10 -> 256 -> 256 -> 2): its block is folded")
            self._serving = torch.empty_like(self.actor_weights)
            self._fold()

    @property
    def serving_weights(self) -> torch.Tensor:
        """The packed block the samplers serve with a normaliser: ``actor_weights`` with the affine folded into
        its first layer, rewritten at the end of every update call."""
        if self._serving is None:
            raise ValueError("serving_weights needs obs_norm; without a normaliser serve actor_weights")
        return self._serving

    def _fold(self):
        if self._serving is not None:
            self.obs_norm.fold(self.actor_weights, self._serving)

    # ---------------- the no-gradient half ----------------
    def td_target(self, next_state, reward, mask, update: int, noise=None, diagnostics: dict | None = None):
        """y [B] (the env's real type) of one minibatch through sit_sac_target; noise None draws on the
        device.  diagnostics: a dict that receives next_action, next_logp, q1, q2."""
        B = int(next_state.shape[0])
        dt, dev = self.env.dtype, self.env.device
        y = self._out.get(B)
        if y is None:
            y = self._out[B] = torch.empty(B, dtype=dt, device=dev)
        a = _lib.SacTargetArgs()
        a.batch, a.seed, a.update = B, self.seed & 0xFFFFFFFFFFFFFFFF, int(update) & 0xFFFFFFFFFFFFFFFF
        a.gamma, a.reward_scale = self.gamma, self.reward_scale
        a.actor_weights, a.critic_weights = self.actor_weights.data_ptr(), self.target_weights.data_ptr()
        a.alpha = self.alpha.data_ptr()
        for name, t in (("next_state", next_state), ("reward", reward), ("mask", mask)):
            setattr(a, name, self._pointer(name, t))
        a.y = y.data_ptr()
        a.noise = None if noise is None else noise.data_ptr()
        if diagnostics is not None:
            for k in ("next_action", "next_logp", "q1", "q2"):
                diagnostics[k] = torch.empty(B, dtype=dt, device=dev)
                setattr(a, k, diagnostics[k].data_ptr())
        with torch.cuda.device(dev):
            self.env._call("sit_sac_target_wide" if self.row_pass == "mfma" else "sit_sac_target", byref(a),
                           self.env._stream())
        return y

    def _pointer(self, name: str, t: torch.Tensor) -> int:
        """The address of a kernel's input: a contiguous tensor of the env's real type on the env's device."""
        if t.dtype != self.env.dtype or t.device != self.env.device or not t.is_contiguous():
            raise ValueError(f"{name}: a contiguous {self.env.dtype} tensor on {self.env.device} is required")
        return t.data_ptr()

    def _host_noise(self, values: np.ndarray):
        return torch.from_numpy(values.astype(np.float32)).to(self.env.device, non_blocking=True)

    def _polyak(self):
        if self.target == "hip":
            pack_critic_weights(self.critic, out=self.online_weights)
            with torch.cuda.device(self.env.device):
                self.env._call("sit_sac_polyak", c_void_p(self.target_weights.data_ptr()),
                               c_void_p(self.online_weights.data_ptr()), self.online_weights.numel(), self.tau,
                               self.env._stream())
        else:
            self._polyak_torch()

    # ---------------- one update ----------------
    def update_parameters(self, memory, batch_size: int, updates: int):
        """One SAC update from one minibatch of `memory`; `updates` is the caller's update counter
        (main_ast.py:350-362).  Returns (critic_1_loss, critic_2_loss, policy_loss, ent_loss, alpha) as
        floats, or None while len(memory) <= batch_size (nothing is done then)."""
        B = int(batch_size)
        if not self._ready:
            if len(memory) <= B:
                return None
            self._ready = True        # a ring never shrinks
        raw = _sample(memory, B, self.obs_norm)
        if self.gradient == "hip":
            return self._hip_update(raw, B, updates)
        if self.target == "hip":
            y = self.td_target(raw["next_state"], raw["reward"], raw["mask"], updates).to(torch.float32)
            batch = {k: v.to(torch.float32) for k, v in raw.items()}
        else:
            batch = {k: v.to(torch.float32) for k, v in raw.items()}
            eps = self._host_noise(sac_noise(self.seed, np.arange(B), updates))
            y = torch_target(self.policy, self.target_critic, batch["next_state"], batch["reward"], batch["mask"], eps,
                             self.alpha, self.gamma, self.reward_scale)["y"]
        eps_pi = self._host_noise(policy_noise(self.seed, updates, B))
        l1, l2, lp, la, alpha = _gradient_half(self.policy, self.critic, self.optims, self.log_alpha, self.alpha,
                                               self.auto, batch, y, eps_pi)
        if self.auto:
            self.alpha.copy_(alpha)
        if updates % self.target_update_interval == 0:
            self._polyak()
        if self.actor_weights is not None:
            pack_actor_weights(self.policy, out=self.actor_weights)
        self._fold()
        return tuple(torch.stack([l1, l2, lp, la.reshape(()), self.alpha[0]]).tolist())

    # ---------------- one update, gradient="hip" ----------------
    def _adam(self, key: str) -> _lib.SacAdam:
        """The scalars of one Adam step of optimiser `key`; its step count advances here, on the host."""
        self._steps[key] += 1
        t = self._steps[key]
        g = self.optims[key].param_groups[0]
        b1, b2 = g["betas"]
        return _lib.SacAdam(float(g["lr"]), float(b1), float(b2), float(g["eps"]), 1.0 - b1 ** t, 1.0 - b2 ** t)

    def _hip_update(self, raw, B: int, updates: int):
        dev = self.env.device
        self._reconcile()
        y = self.td_target(raw["next_state"], raw["reward"], raw["mask"], updates)
        state, action = self._pointer("state", raw["state"]), self._pointer("action", raw["action"])
        n_ws = 2 * B * _lib.SIT_SAC_WORKSPACE_ROW
        if self._ws is None or self._ws.numel() < n_ws:
            self._ws = torch.empty(n_ws, dtype=torch.float32, device=dev)
        c = _lib.SacCriticStepArgs()
        c.batch, c.workspace_floats, c.adam = B, self._ws.numel(), self._adam("critic")
        c.critic_weights, c.critic_m, c.critic_v = (self.online_weights.data_ptr(), self._m["critic"].data_ptr(),
                                                    self._v["critic"].data_ptr())
        c.state, c.action, c.y = state, action, y.data_ptr()
        c.workspace, c.results = self._ws.data_ptr(), self._results.data_ptr()
        p = _lib.SacPolicyStepArgs()
        p.batch, p.tune, p.workspace_floats = B, int(self.auto), self._ws.numel()
        p.seed, p.update = self.seed & 0xFFFFFFFFFFFFFFFF, int(updates) & 0xFFFFFFFFFFFFFFFF
        p.target_entropy, p.adam = self.target_entropy, self._adam("policy")
        p.actor_weights, p.actor_m, p.actor_v = (self.actor_weights.data_ptr(), self._m["policy"].data_ptr(),
                                                 self._v["policy"].data_ptr())
        p.critic_weights, p.alpha = self.online_weights.data_ptr(), self.alpha.data_ptr()
        if self.auto:
            p.alpha_adam = self._adam("alpha")
            p.log_alpha, p.log_alpha_m, p.log_alpha_v = (self.log_alpha.data_ptr(), self._m["alpha"].data_ptr(),
                                                         self._v["alpha"].data_ptr())
        p.state, p.noise = state, None
        p.workspace, p.results = self._ws.data_ptr(), self._results.data_ptr()
        with torch.cuda.device(dev):
            stream = self.env._stream()
            tiled = "_wide" if self.row_pass == "mfma" else "_tiled" if self.weight_gradient == "mfma" else ""
            self.env._call("sit_sac_critic_step" + tiled, byref(c), stream)
            self.env._call("sit_sac_policy_step" + tiled, byref(p), stream)
            if updates % self.target_update_interval == 0:
                self.env._call("sit_sac_polyak", c_void_p(self.target_weights.data_ptr()),
                               c_void_p(self.online_weights.data_ptr()), self.online_weights.numel(), self.tau, stream)
        self._fold()
        touch_parameters(self._params + ([self.log_alpha] if self.auto else []))
        self._next_update = int(updates) + 1
        if self._clocked:
            self._write_clock()
        return tuple(self._results.tolist())

    # ---------------- many updates per call, gradient="hip" ----------------
    def _write_clock(self):
        """The host's step counts and next update number into the clock's state words, on the stream (fills)."""
        for word, value in ((0, self._next_update), (1, self._steps["critic"]), (2, self._steps["policy"]),
                            (3, self._steps.get("alpha", 0))):
            self.clock[word:word + 1].fill_(int(value))

    def _reconcile(self):
        """The host's step counts from the clock: one read when clocked work happened since the last one."""
        if self.gradient != "hip" or not self._clock_dirty:
            return
        c = self.clock[:8].tolist()
        self._next_update = c[0]
        self._steps["critic"], self._steps["policy"] = c[1], c[2]
        if "alpha" in self._steps:
            self._steps["alpha"] = c[3]
        self._clock_dirty = self._captured       # a captured graph may advance the clock again at any time

    def _clocked_adam(self, key: str) -> _lib.SacAdam:
        g = self.optims[key].param_groups[0]
        b1, b2 = g["betas"]
        return _lib.SacAdam(float(g["lr"]), float(b1), float(b2), float(g["eps"]), 1.0, 1.0)

    def update_many(self, memory, batch_size: int, n_updates: int, first_update: int | None = None) -> None:
        """`n_updates` SAC updates from `n_updates` fresh minibatches of `memory` in one ``sit_sac_updates`` call;
        nothing is read back (``results()`` reads the losses).  first_update: the update number of the first
        one (the `updates` of ``update_parameters``); None continues from the clock.  Raises ValueError while
        len(memory) <= batch_size, and touches nothing then.  After one eager call with the same (batch_size,
        n_updates) the call can be captured in a HIP graph (one stream; first_update must be None there): a
        replay runs the next `n_updates` updates."""
        if self.gradient != "hip":
            raise ValueError("update_many needs gradient='hip'")
        B, U = int(batch_size), int(n_updates)
        if B <= 0 or U <= 0:
            raise ValueError("batch_size and n_updates must be positive")
        dev, key = self.env.device, (B, U)
        n_ws = 2 * B * _lib.SIT_SAC_WORKSPACE_ROW
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing:
            if first_update is not None:
                raise ValueError("update_many: first_update cannot be given under graph capture")
            if (not self._ready or not self._clocked or key not in self._many or B not in self._out
                    or self._ws is None or self._ws.numel() < n_ws):
                raise ValueError("update_many: call it once eagerly with the same (batch_size, n_updates) before "
                                 "capturing it")
        if not self._ready:
            if len(memory) <= B:
                raise ValueError(f"update_many: the memory must hold more than batch_size = {B} records")
            self._ready = True        # a ring never shrinks
        if self._ws is None or self._ws.numel() < n_ws:
            self._ws = torch.empty(n_ws, dtype=torch.float32, device=dev)
        y = self._out.get(B)
        if y is None:
            y = self._out[B] = torch.empty(B, dtype=self.env.dtype, device=dev)
        with torch.cuda.device(dev):
            if not self._clocked:
                self._write_clock()
                self._clocked = True
            if first_update is not None:
                self.clock[0:1].fill_(int(first_update))
            if self.obs_norm is None:
                mb = self._many[key] = memory.sample(B, n_batches=U, out=self._many.get(key))
            else:
                mb = self._many[key] = memory.sample(B, n_batches=U, out=self._many.get(key), normalizer=self.obs_norm)
            a = _lib.SacUpdatesArgs()
            a.mode = (_lib.SIT_SAC_UPDATES_WIDE if self.row_pass == "mfma" else
                      _lib.SIT_SAC_UPDATES_TILED if self.weight_gradient == "mfma" else _lib.SIT_SAC_UPDATES_PLAIN)
            a.batch, a.n_updates, a.tune, a.seed = B, U, int(self.auto), self.seed & 0xFFFFFFFFFFFFFFFF
            a.gamma, a.reward_scale, a.target_entropy, a.tau = self.gamma, self.reward_scale, self.target_entropy, self.tau
            a.target_update_interval, a.workspace_floats = self.target_update_interval, self._ws.numel()
            a.results_capacity = self._ring.shape[0]
            a.critic_adam, a.actor_adam = self._clocked_adam("critic"), self._clocked_adam("policy")
            a.critic_weights, a.critic_m, a.critic_v = (self.online_weights.data_ptr(), self._m["critic"].data_ptr(),
                                                        self._v["critic"].data_ptr())
            a.actor_weights, a.actor_m, a.actor_v = (self.actor_weights.data_ptr(), self._m["policy"].data_ptr(),
                                                     self._v["policy"].data_ptr())
            a.target_weights, a.alpha = self.target_weights.data_ptr(), self.alpha.data_ptr()
            if self.auto:
                a.alpha_adam = self._clocked_adam("alpha")
                a.log_alpha, a.log_alpha_m, a.log_alpha_v = (self.log_alpha.data_ptr(), self._m["alpha"].data_ptr(),
                                                             self._v["alpha"].data_ptr())
            for name in ("state", "action", "reward", "next_state", "mask"):
                setattr(a, name, self._pointer(name, mb[name]))
            a.y, a.workspace = y.data_ptr(), self._ws.data_ptr()
            a.clock, a.results = self.clock.data_ptr(), self._ring.data_ptr()
            self.env._call("sit_sac_updates", byref(a), self.env._stream())
            self._fold()
        self._clock_dirty = True
        self._captured = self._captured or capturing
        touch_parameters(self._params + ([self.log_alpha] if self.auto else []))

    def results(self, last: int | None = None) -> list:
        """The newest min(last, written, capacity) result rows of ``update_many``'s updates, oldest first, as
        (critic_1_loss, critic_2_loss, policy_loss, ent_loss, alpha) tuples.  The one call that synchronises."""
        if self.gradient != "hip":
            raise ValueError("results needs gradient='hip'")
        written = int(self.clock[4].item())
        ring = self._ring.tolist()
        cap = len(ring)
        n = min(written, cap) if last is None else max(0, min(int(last), written, cap))
        return [tuple(ring[(written - n + i) % cap]) for i in range(n)]

    def _optim_state_dicts(self) -> dict:
        """The three optimisers' state in ``torch.optim.Adam.state_dict()`` form (both gradient modes write
        this one format; in hip mode the moments come from the packed blocks and the host's step counts)."""
        if self.gradient != "hip":
            return {k: copy.deepcopy(o.state_dict()) for k, o in self.optims.items()}
        out = {}
        for k, o in self.optims.items():
            out[k] = copy.deepcopy(o.state_dict())
            out[k]["state"] = moments_to_adam_state(self._m[k], self._v[k], self._layers[k], self._steps[k])
        return out

    def _load_optim_state_dicts(self, optims: dict):
        if self.gradient != "hip":
            for k, o in self.optims.items():
                o.load_state_dict(optims[k])
            return
        for k, o in self.optims.items():
            o.load_state_dict({"state": {}, "param_groups": optims[k]["param_groups"]})    # lr, betas, eps
            self._steps[k] = adam_state_to_moments(optims[k]["state"], self._m[k], self._v[k], self._layers[k])

    # ---------------- checkpoint ----------------
    def state_dict(self) -> dict:
        """Networks, optimisers (in ``torch.optim.Adam``'s form in both gradient modes: in hip mode the packed
        moment blocks and the step counts, converted), targets (as the packed block, in both modes) and
        log_alpha."""
        tw = self.target_weights if self.target == "hip" else pack_critic_weights(self.target_critic)
        self._reconcile()
        return {"policy": copy.deepcopy(self.policy.state_dict()), "critic": copy.deepcopy(self.critic.state_dict()),
                "critic_target": None if tw is None else tw.clone(),
                "critic_target_state": None if tw is not None else copy.deepcopy(self.target_critic.state_dict()),
                "log_alpha": self.log_alpha.detach().clone(),
                "optims": self._optim_state_dicts()}

    def load_state_dict(self, sd: dict):
        self.policy.load_state_dict(sd["policy"])
        self.critic.load_state_dict(sd["critic"])
        if self.target == "hip":
            if sd.get("critic_target") is None:
                raise ValueError("this checkpoint holds no packed target block")
            self.target_weights.copy_(sd["critic_target"])
            if self.gradient != "hip":                   # there the parameters are the block
                pack_critic_weights(self.critic, out=self.online_weights)
        elif sd.get("critic_target") is not None:
            unpack_critic_weights(sd["critic_target"].to(self.env.device), self.target_critic)
        else:
            self.target_critic.load_state_dict(sd["critic_target_state"])
        with torch.no_grad():
            self.log_alpha.copy_(sd["log_alpha"])
            self.alpha.copy_(self.log_alpha.detach().exp())
        self._load_optim_state_dicts(sd["optims"])
        if self.gradient == "hip":
            touch_parameters(self._params)
            with torch.cuda.device(self.env.device):
                self._write_clock()        # (the update number is no part of a checkpoint: it stays)
            self._clock_dirty = self._captured
        elif self.actor_weights is not None:
            pack_actor_weights(self.policy, out=self.actor_weights)


class SacUpdateReference(_SacState):
    """``SacLearner``'s update in float64 PyTorch on the CPU: deep copies of the networks, a target
    ``QNetwork``, the TD target by the formulas of ``sac_target_reference`` and the same noise draws."""

    def __init__(self, policy: nn.Module, critic: nn.Module, *, gamma: float = 0.99, tau: float = 0.005, lr: float = 3e-4,
                 alpha: float = 0.2, automatic_entropy_tuning: bool = True, target_update_interval: int = 1,
                 reward_scale: float = 1.0, seed: int = 25450, obs_norm=None):
        self.obs_norm = obs_norm          # an ObsNormReference: its float32 affine's values, applied in float64
        self.policy = copy.deepcopy(policy).to(device="cpu", dtype=torch.float64)
        self.critic = copy.deepcopy(critic).to(device="cpu", dtype=torch.float64)
        self.target_critic = copy.deepcopy(self.critic).requires_grad_(False)
        self._setup(torch.float64, "cpu", gamma=gamma, tau=tau, lr=lr, alpha=alpha,
                    automatic_entropy_tuning=automatic_entropy_tuning, target_update_interval=target_update_interval,
                    reward_scale=reward_scale, seed=seed)

    def update_parameters(self, memory, batch_size: int, updates: int):
        B = int(batch_size)
        if len(memory) <= B:
            return None
        as64 = lambda v: (v.detach().cpu() if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))).to(torch.float64)  # noqa: E731
        batch = {k: as64(v) for k, v in _sample(memory, B).items()}
        if self.obs_norm is not None:
            for k in ("state", "next_state"):
                batch[k] = torch.from_numpy(self.obs_norm.normalized(batch[k].numpy(), np.float64))
        eps = torch.from_numpy(sac_noise(self.seed, np.arange(B), updates))
        y = torch_target(self.policy, self.target_critic, batch["next_state"], batch["reward"], batch["mask"], eps,
                         self.alpha, self.gamma, self.reward_scale)["y"]
        eps_pi = torch.from_numpy(policy_noise(self.seed, updates, B))
        l1, l2, lp, la, alpha = _gradient_half(self.policy, self.critic, self.optims, self.log_alpha, self.alpha,
                                               self.auto, batch, y, eps_pi)
        if self.auto:
            self.alpha = alpha
        if updates % self.target_update_interval == 0:
            self._polyak_torch()
        return float(l1), float(l2), float(lp), float(la), float(self.alpha[0])


def sac_update_reference(policy: nn.Module, critic: nn.Module, **kw) -> SacUpdateReference:
    """A float64 CPU learner with ``SacLearner``'s update (``SacUpdateReference``), started from copies of
    `policy` and `critic`."""
    return SacUpdateReference(policy, critic, **kw)


__all__ = ["QNetwork", "SacLearner", "SacUpdateReference", "pack_critic_weights",
           "unpack_critic_weights", "block_views", "bind_parameters", "touch_parameters", "moments_to_adam_state",
           "adam_state_to_moments", "sac_noise", "policy_noise", "adam_scalars_reference", "log_one_minus_tanh_sq", "sac_target_reference", "torch_target",
           "sac_update_reference"]
