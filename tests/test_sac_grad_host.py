"""Host-side pieces of SacLearner(gradient="hip") on CPU tensors: the views that make the networks'
parameters segments of the packed blocks, the torch-Adam <-> packed-moment conversion, and the ctypes
declarations of sit_sac_critic_step / sit_sac_policy_step.  No GPU."""
import ctypes
import os

import pytest
import torch

from sac_maritime_ast_amd import _lib, sac
from sac_maritime_ast_amd.samplers import GaussianPolicy, pack_actor_weights


def networks(seed=3):
    torch.manual_seed(seed)
    return GaussianPolicy(), sac.QNetwork()


def layers_and_block(kind):
    pol, q = networks()
    if kind == "actor":
        return pol, [sac._actor_layers(pol)], pack_actor_weights(pol), pack_actor_weights
    return q, sac._critic_layers(q), sac.pack_critic_weights(q), sac.pack_critic_weights


@pytest.mark.parametrize("kind", ["actor", "critic"])
def test_bound_parameters_are_the_block(kind):
    module, layers, block, pack = layers_and_block(kind)
    before = [p.detach().clone() for p in module.parameters()]
    ids = [id(p) for p in module.parameters()]
    params = sac.bind_parameters(block, layers)
    assert [id(p) for p in module.parameters()] == ids == [id(p) for p in params]     # the same Parameter objects
    assert all(torch.equal(a, b) for a, b in zip(before, module.parameters()))
    lo, hi = block.data_ptr(), block.data_ptr() + 4 * block.numel()
    assert all(lo <= p.data_ptr() < hi for p in params)
    assert not layers[0][1].weight.is_contiguous()             # l2.weight: the transposed view of W2^T
    # an in-place write to the block is a write to the module, padding excepted
    x = torch.randn(5, layers[0][0].weight.shape[1])
    y0 = layers[0][0](x)
    with torch.no_grad():
        block.mul_(1.5).add_(0.25)
    assert torch.equal(pack(module), block) if kind == "actor" else torch.equal(
        pack(module).view(2, -1)[:, :-3], block.view(2, -1)[:, :-3])
    assert not torch.equal(layers[0][0](x), y0)
    # and the module still trains through the views
    head = layers[0][2](torch.relu(layers[0][1](torch.relu(layers[0][0](x)))))
    head.sum().backward()
    assert all(p.grad is not None and p.grad.shape == p.shape for ls in layers[:1] for l in ls for p in (l.weight, l.bias))


def test_touch_parameters_bumps_the_versions():
    module, layers, block, _ = layers_and_block("actor")
    params = sac.bind_parameters(block, layers)
    v0 = [p._version for p in params]
    ptr0 = [p.data_ptr() for p in params]
    sac.touch_parameters(params)
    assert [p._version for p in params] == [v + 1 for v in v0]
    assert [p.data_ptr() for p in params] == ptr0


def test_critic_padding_is_no_parameter():
    q, layers, block, _ = layers_and_block("critic")
    covered = torch.zeros_like(block)
    for v in sac.block_views(covered, layers):
        v.fill_(1.0)
    assert covered.view(2, -1)[:, :-3].min() == 1.0 and covered.view(2, -1)[:, -3:].max() == 0.0
    assert [tuple(v.shape) for v in sac.block_views(block, layers)] == [tuple(p.shape) for p in q.parameters()]


@pytest.mark.parametrize("kind", ["actor", "critic"])
def test_adam_state_round_trips_through_packed_moments(kind):
    module, layers, block, pack = layers_and_block(kind)
    opt = torch.optim.Adam(module.parameters(), lr=3e-4)
    for _ in range(3):
        opt.zero_grad()
        x = torch.randn(6, layers[0][0].weight.shape[1])
        loss = sum((ls[2](torch.relu(ls[1](torch.relu(ls[0](x))))) ** 2).sum() for ls in layers)
        loss.backward()
        opt.step()
    state = opt.state_dict()["state"]
    m, v = torch.full_like(block, 7.0), torch.full_like(block, 7.0)
    assert sac.adam_state_to_moments(state, m, v, layers) == 3
    # the moments are laid out as the weights are: packing a module that holds them gives the block
    holder = type(module)()
    with torch.no_grad():
        for p, i in zip(holder.parameters(), range(len(state))):
            p.copy_(state[i]["exp_avg"])
    packed = pack(holder)
    assert torch.equal(packed, m)
    back = sac.moments_to_adam_state(m, v, layers, 3)
    assert set(back) == set(state)
    for i, st in state.items():
        assert float(back[i]["step"]) == float(st["step"]) == 3.0
        assert torch.equal(back[i]["exp_avg"], st["exp_avg"]) and torch.equal(back[i]["exp_avg_sq"], st["exp_avg_sq"])
        assert back[i]["exp_avg"].is_contiguous() and back[i]["exp_avg"].shape == st["exp_avg"].shape
    # a torch optimiser accepts the converted state and continues exactly as the original does
    other_module = type(module)()
    other_module.load_state_dict(module.state_dict())
    other = torch.optim.Adam(other_module.parameters(), lr=3e-4)
    other.load_state_dict({"state": back, "param_groups": opt.state_dict()["param_groups"]})
    for mod, o in ((module, opt), (other_module, other)):
        o.zero_grad()
        sum((p ** 2).sum() for p in mod.parameters()).backward()
        o.step()
    assert all(torch.equal(a, b) for a, b in zip(module.parameters(), other_module.parameters()))
    # before the first step both forms are empty / zero
    assert sac.moments_to_adam_state(m, v, layers, 0) == {}
    assert sac.adam_state_to_moments({}, m, v, layers) == 0 and not m.any() and not v.any()


def test_lib_declares_the_new_calls():
    for name in ("sit_sac_workspace_floats", "sit_sac_critic_step_args_size", "sit_sac_policy_step_args_size",
                 "sit_sac_critic_step", "sit_sac_policy_step"):
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["sit_sac_critic_step"][1][1]._type_ is _lib.SacCriticStepArgs
    assert _lib.SIGNATURES["sit_sac_policy_step"][1][1]._type_ is _lib.SacPolicyStepArgs
    assert ctypes.sizeof(_lib.SacAdam) == 48
    assert ctypes.sizeof(_lib.SacCriticStepArgs) == 16 + 48 + 8 * 8
    assert ctypes.sizeof(_lib.SacPolicyStepArgs) == 16 + 16 + 8 + 2 * 48 + 12 * 8
    assert _lib.SIT_SAC_WORKSPACE_ROW == 12 + 4 * _lib.SIT_ACTOR_HIDDEN + 4


def test_args_sizes_match_the_built_library():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsit.so is not built")
    lib = _lib.load()
    assert lib.sit_sac_critic_step_args_size() == ctypes.sizeof(_lib.SacCriticStepArgs)
    assert lib.sit_sac_policy_step_args_size() == ctypes.sizeof(_lib.SacPolicyStepArgs)
    assert lib.sit_sac_workspace_floats(64) == 2 * 64 * _lib.SIT_SAC_WORKSPACE_ROW
    assert lib.sit_sac_workspace_floats(0) == 0 and lib.sit_sac_workspace_floats(-5) == 0
    assert lib.sit_sac_workspace_floats(2 ** 31 - 1) == 2 * (2 ** 31 - 1) * _lib.SIT_SAC_WORKSPACE_ROW


def test_gradient_argument_is_validated():
    with pytest.raises(ValueError, match="gradient"):
        sac.SacLearner(None, GaussianPolicy(), gradient="cuda")
    with pytest.raises(ValueError, match="target='hip'"):
        sac.SacLearner(None, GaussianPolicy(), gradient="hip", target="torch")
