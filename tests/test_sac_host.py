"""CPU checks of the SAC learner's host side (sac_maritime_ast_amd/sac.py): the packed critic block, the
Philox / Box-Muller noise, sac_target_reference against a hand-computed example, and the float64
reference update on a synthetic ring.  Nothing here launches a kernel."""
import math

import numpy as np
import pytest
import torch
from torch import nn

from oracle import sit_oracle as so

sit = pytest.importorskip("sac_maritime_ast_amd")
from sac_maritime_ast_amd import _lib, replay_reference, sac  # noqa: E402
from sac_maritime_ast_amd.samplers import GaussianPolicy, pack_actor_weights  # noqa: E402

H, CW, AW = _lib.SIT_ACTOR_HIDDEN, _lib.SIT_CRITIC_WEIGHTS, _lib.SIT_ACTOR_WEIGHTS
# offsets inside one critic block (include/sit.h "SAC learner")
W1, B1 = 0, H * 11
W2T = B1 + H
B2 = W2T + H * H
W3 = B2 + H
B3 = W3 + H


def test_exports_and_constants():
    for name in ("QNetwork", "SacLearner", "pack_critic_weights", "sac_target_reference", "sac_update_reference"):
        assert getattr(sit, name) is getattr(sac, name) and name in sit.__all__
    assert CW == 69124 and CW % 4 == 0 and B3 + 1 == 69121 and W2T % 4 == 0


# ---------------------------------------------------------------------------------------------
# pack_critic_weights
# ---------------------------------------------------------------------------------------------
def test_pack_critic_weights_layout_padding_and_out():
    torch.manual_seed(3)
    q = sac.QNetwork()
    w = sac.pack_critic_weights(q)
    assert w.dtype == torch.float32 and tuple(w.shape) == (2 * CW,) and w.is_contiguous()
    for c, net in enumerate((q.q1, q.q2)):
        b = w[c * CW:(c + 1) * CW]
        l1, l2, l3 = net[0], net[2], net[4]
        assert torch.equal(b[W1:B1].view(H, 11), l1.weight.detach())
        assert torch.equal(b[B1:W2T], l1.bias.detach())
        assert torch.equal(b[W2T:B2].view(H, H), l2.weight.detach().t())      # [in][out]
        assert torch.equal(b[B2:W3], l2.bias.detach())
        assert torch.equal(b[W3:B3], l3.weight.detach()[0])
        assert torch.equal(b[B3:B3 + 1], l3.bias.detach())
        assert torch.equal(b[B3 + 1:], torch.zeros(3))                         # padding to 4 floats
    # in place: the same tensor comes back, refreshed after a parameter change, the padding left alone
    out = torch.full((2 * CW,), 7.0)
    assert sac.pack_critic_weights(q, out=out) is out
    assert torch.equal(out[:B3 + 1], w[:B3 + 1]) and torch.equal(out[B3 + 1:CW], torch.full((3,), 7.0))
    with torch.no_grad():
        q.q2[2].weight[5, 9] = 123.0
    sac.pack_critic_weights(q, out=out)
    assert out[CW + W2T + 9 * H + 5] == 123.0
    # the round trip
    q2 = sac.unpack_critic_weights(out, sac.QNetwork())
    assert all(torch.equal(a, b) for a, b in zip(q.state_dict().values(), q2.state_dict().values()))
    with pytest.raises(ValueError):
        sac.pack_critic_weights(q, out=torch.zeros(2 * CW - 1))
    with pytest.raises(ValueError):
        sac.pack_critic_weights(q, out=torch.zeros(2 * CW, dtype=torch.float64))


def test_pack_critic_weights_declines_other_architectures():
    assert sac.pack_critic_weights(sac.QNetwork(hidden=128)) is None
    assert sac.pack_critic_weights(sac.QNetwork(obs_dim=12)) is None
    assert sac.pack_critic_weights(nn.Linear(11, 1)) is None
    q = sac.QNetwork()
    q.q1[1] = nn.Tanh()
    assert sac.pack_critic_weights(q) is None


# ---------------------------------------------------------------------------------------------
# noise
# ---------------------------------------------------------------------------------------------
def test_noise_is_philox_box_muller_of_row_and_update():
    seed, update = 0x1234_5678_9ABC_DEF0, (7 << 32) | 11
    rows = np.arange(5)
    z = sac.sac_noise(seed, rows, update)
    # the construction, from the oracle's Philox: ctr = (row, 0x5441, update lo, update hi), key = seed
    key = (np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))
    c = so.philox4x32_10((rows.astype(np.uint64), np.uint64(0x5441), np.uint64(11), np.uint64(7)), key)
    u1 = ((c[0] >> np.uint32(5)).astype(np.float64) * 2.0 ** 26 + (c[1] >> np.uint32(6)).astype(np.float64) + 1.0) / 2.0 ** 53
    u2 = ((c[2] >> np.uint32(5)).astype(np.float64) * 2.0 ** 26 + (c[3] >> np.uint32(6)).astype(np.float64)) / 2.0 ** 53
    assert np.array_equal(z, np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2))
    # row, update (either word), seed and tag each change the draw
    assert not np.any(z == sac.sac_noise(seed, rows + 5, update))
    assert not np.any(z == sac.sac_noise(seed, rows, update + 1))
    assert not np.any(z == sac.sac_noise(seed, rows, update + (1 << 32)))
    assert not np.any(z == sac.sac_noise(seed + 1, rows, update))
    assert not np.any(z == sac.policy_noise(seed, update, 5))
    assert np.array_equal(sac.policy_noise(seed, update, 5), sac.sac_noise(seed, rows, update, sac.POLICY_NOISE_TAG))


def test_noise_moments():
    """200 000 draws: the mean within 4 standard errors (4 / sqrt(n) = 0.009) and the standard
    deviation within 4 of its own (4 / sqrt(2 n) = 0.0063); rows of one update and updates of one row."""
    n = 200_000
    for z in (sac.sac_noise(25450, np.arange(n), 3), np.concatenate([sac.sac_noise(25450, [0], u) for u in range(2000)])):
        k = len(z)
        assert abs(z.mean()) < 4 / math.sqrt(k) and abs(z.std() - 1.0) < 4 / math.sqrt(2 * k)
    z = sac.sac_noise(25450, np.arange(n), 3)
    assert abs(np.mean(z ** 3)) < 0.05 and abs(np.mean(z ** 4) - 3.0) < 0.1 and np.abs(z).max() < 6.5


# ---------------------------------------------------------------------------------------------
# sac_target_reference
# ---------------------------------------------------------------------------------------------
def hand_blocks(mu, ls):
    """An actor whose head is the constant (mu, ls), Q1 = 2 relu(a') + 0.5, Q2 = -relu(next_state[0]) + 0.25."""
    aw = np.zeros(AW, dtype=np.float32)
    aw[-2:] = (mu, ls)
    cw = np.zeros(2 * CW, dtype=np.float32)
    cw[W1 + 0 * 11 + 10] = 1.0           # Q1: unit 0 of layer 1 = relu(a')
    cw[W2T + 0 * H + 0] = 1.0            #     unit 0 of layer 2 = that
    cw[W3 + 0], cw[B3] = 2.0, 0.5
    o = CW
    cw[o + W1 + 1 * 11 + 0] = 1.0        # Q2: unit 1 of layer 1 = relu(next_state[0])
    cw[o + W2T + 1 * H + 3] = 1.0        #     unit 3 of layer 2 = that (W2^T is [in][out])
    cw[o + W3 + 3], cw[o + B3] = -1.0, 0.25
    return aw, cw


def test_target_reference_hand_computed_two_rows():
    mu, ls, alpha, gamma, rs = 0.25, -1.0, 0.2, 0.99, 2.0
    aw, cw = hand_blocks(mu, ls)
    ns = np.zeros((2, 10))
    ns[:, 0] = (0.75, -3.0)
    ns[:, 4] = (5.0, -6.0)               # ignored by every network
    eps, reward, mask = (0.5, -1.5), (-1.0, 0.5), (1.0, 0.0)
    got = sac.sac_target_reference(aw, cw, ns, reward, mask, alpha=alpha, gamma=gamma, reward_scale=rs, noise=eps)
    for b in range(2):
        x = mu + math.exp(ls) * eps[b]
        a = math.tanh(x)
        logp = -0.5 * eps[b] ** 2 - ls - 0.5 * math.log(2 * math.pi) - math.log(1.0 - a * a + 1e-6)
        q1, q2 = 2.0 * max(a, 0.0) + 0.5, -max(ns[b, 0], 0.0) + 0.25
        y = rs * reward[b] + mask[b] * gamma * (min(q1, q2) - alpha * logp)
        want = {"x": x, "next_action": a, "next_logp": logp, "q1": q1, "q2": q2, "y": y, "noise": eps[b]}
        for k, v in want.items():
            assert got[k][b] == pytest.approx(v, rel=1e-13, abs=1e-13), (b, k)
    # row 0: a' > 0 so Q1 = 0.5 + 2 a' > Q2 = -0.5; row 1 is terminal: y = reward_scale * reward
    assert got["q1"][0] > got["q2"][0] and got["y"][1] == rs * reward[1]


def test_target_reference_saturation_and_clips():
    """|x| up to 12: the log term follows 4 (em + 1) / (em + 2)^2, not the cancelled 1 - a * a; log sigma
    is clipped to [-20, 2]."""
    for ls_raw, ls in ((-25.0, -20.0), (3.0, 2.0), (0.0, 0.0)):
        aw, cw = hand_blocks(0.0, ls_raw)
        x = np.linspace(-12.0, 12.0, 49)
        eps = x / math.exp(ls)
        got = sac.sac_target_reference(aw, cw, np.zeros((49, 10)), np.zeros(49), np.ones(49), alpha=0.0, gamma=1.0, noise=eps)
        assert np.allclose(got["x"], x, rtol=1e-12, atol=1e-12)
        sech2 = 1.0 / np.cosh(x) ** 2
        want = -0.5 * eps ** 2 - ls - 0.5 * math.log(2 * math.pi) - np.log(sech2 + 1e-6)
        assert np.allclose(got["next_logp"], want, rtol=1e-12, atol=1e-12)


def test_target_reference_equals_the_modules():
    """The packed blocks give what GaussianPolicy and QNetwork give in float64; the drawn noise is sac_noise."""
    torch.manual_seed(5)
    pol, q = GaussianPolicy().double(), sac.QNetwork().double()
    rng = np.random.default_rng(5)
    ns, reward, mask = rng.standard_normal((9, 10)), rng.standard_normal(9), (rng.random(9) < 0.7).astype(np.float64)
    # (the blocks are float32: round the parameters first so both sides hold the same numbers)
    with torch.no_grad():
        for p in list(pol.parameters()) + list(q.parameters()):
            p.copy_(p.float().double())
    got = sac.sac_target_reference(pack_actor_weights(pol), sac.pack_critic_weights(q), ns, reward, mask, alpha=0.2,
                                   gamma=0.99, seed=77, update=4)
    assert np.array_equal(got["noise"], sac.sac_noise(77, np.arange(9), 4))
    with torch.no_grad():
        t = torch.from_numpy(ns)
        a, logp, _, _ = pol(t, torch.from_numpy(got["noise"])[:, None])
        q1, q2 = q(t, a)
    assert np.allclose(got["next_action"], a[:, 0].numpy(), rtol=0, atol=1e-13)
    assert np.allclose(got["next_logp"], logp.numpy(), rtol=0, atol=1e-9)      # (the module's 1 - a * a, in float64)
    assert np.allclose(got["q1"], q1.numpy(), rtol=0, atol=1e-13) and np.allclose(got["q2"], q2.numpy(), rtol=0, atol=1e-13)
    y = reward + mask * 0.99 * (np.minimum(got["q1"], got["q2"]) - 0.2 * got["next_logp"])
    assert np.allclose(got["y"], y, rtol=0, atol=1e-14)


# ---------------------------------------------------------------------------------------------
# sac_update_reference
# ---------------------------------------------------------------------------------------------
def synthetic_ring(n=128, seed=8):
    """n records whose reward is a function of (state, action): something a critic can learn."""
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, _lib.SIT_TRANSITION_DIM), dtype=np.float32)
    rec[:, 0:10] = rng.standard_normal((n, 10))
    rec[:, 10] = np.tanh(rng.standard_normal(n))
    rec[:, 11] = rec[:, 0] - 0.5 * rec[:, 10]
    rec[:, 12:22] = rec[:, 0:10] + 0.1 * rng.standard_normal((n, 10))
    rec[:, 22] = rng.random(n) < 0.75
    rec[:, 23] = np.arange(n)
    ring = replay_reference(n, np.float32, seed=seed)
    ring.push(rec, n)
    return ring


def test_update_reference_lowers_the_critic_loss():
    torch.manual_seed(8)
    pol, q = GaussianPolicy(), sac.QNetwork()
    ring = synthetic_ring()
    ref = sac.sac_update_reference(pol, q, seed=8)
    assert all(p.dtype == torch.float64 for p in ref.critic.parameters())
    before = [p.detach().clone() for p in pol.parameters()]
    out = [ref.update_parameters(ring, 64, u) for u in range(50)]
    assert all(len(o) == 5 and all(math.isfinite(v) for v in o) for o in out)
    c1, c2 = np.array([o[0] for o in out]), np.array([o[1] for o in out])
    # minibatch losses are noisy: the first and the last ten updates
    assert c1[-10:].mean() < 0.5 * c1[:10].mean() and c2[-10:].mean() < 0.5 * c2[:10].mean(), (c1, c2)
    # entropy above the target of -1 lowers alpha, by at most lr per Adam step
    alphas = [o[4] for o in out]
    assert all(b < a for a, b in zip(alphas, alphas[1:])) and alphas[-1] > 0.2 * math.exp(-50 * 3e-4 * 1.001)
    # the caller's modules are untouched; the targets moved a little towards the critics
    assert all(torch.equal(a, b) for a, b in zip(before, pol.parameters()))
    gap = max(float((t - p.detach()).abs().max()) for t, p in zip(ref.target_critic.parameters(), ref.critic.parameters()))
    moved = max(float((t - p.detach().double()).abs().max()) for t, p in zip(ref.target_critic.parameters(), q.parameters()))
    assert 0 < moved < gap


def test_update_reference_waits_for_more_than_a_batch():
    """main_ast.py:350: no update while len(memory) <= batch_size; nothing is drawn either."""
    ring = synthetic_ring(64)
    ref = sac.sac_update_reference(GaussianPolicy(), sac.QNetwork())
    assert ref.update_parameters(ring, 64, 0) is None and int(ring.cursor[2]) == 0
    assert ref.update_parameters(ring, 63, 0) is not None and int(ring.cursor[2]) == 1


def test_update_reference_is_a_function_of_seed_and_update():
    torch.manual_seed(9)
    pol, q = GaussianPolicy(), sac.QNetwork()
    runs = []
    for seed in (1, 1, 2):
        ref, ring = sac.sac_update_reference(pol, q, seed=seed), synthetic_ring()
        runs.append([ref.update_parameters(ring, 32, u) for u in range(2)])
    assert runs[0] == runs[1] and runs[0] != runs[2]
