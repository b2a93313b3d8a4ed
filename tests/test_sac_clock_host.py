"""The host side of the SAC update clock (include/sit.h: sit_sac_updates, sit_sac_adam_scalars).

``sac.adam_scalars_reference`` is the NumPy statement of the clock's Adam scalars (powers by repeated squaring
in double).  It must give the bits the existing path gives, where the host forms 1 - beta ** t and
sac_adam_scalars (csrc/sit_sac_grad.h) rounds lr / bias1 and sqrt(bias2) to float32, so that ``update_many``
reproduces ``update_parameters`` at the default hyper-parameters.

tests/csrc/sac_updates_args_main.cpp includes only sit_sac_args.h and sit_sac_clock.h (and include/sit.h).  It
is compiled here with the host compiler (-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all) and run
as a child process; nothing is preloaded and nothing is loaded into Python.  The library calls the same checks
before any launch, and compiles the same scalar function for the device."""
import math

import numpy as np
import pytest

import sac_cases as C
from helpers import sanitized_program_cases
from sac_maritime_ast_amd import sac

STEPS = [1, 2, 3, 355, 1000, 37400, 10 ** 6, 2 ** 40]
HYPER = {"default": (3e-4, 0.9, 0.999), "other": (1e-3, 0.5, 0.99)}


def existing_scalars(t, lr):
    """sac_adam_scalars (csrc/sit_sac_grad.h) of sac_cases.adam_scalars(t, lr): what update_parameters' kernels take."""
    o = C.adam_scalars(t, lr)
    return np.array([1.0 - o.beta1, o.beta2, 1.0 - o.beta2, o.lr / o.bias1, math.sqrt(o.bias2), o.eps]).astype(np.float32)


@pytest.mark.parametrize("lr", [3e-4, 1e-3, 1e-4])
def test_reference_equals_the_existing_host_formula(lr):
    t = np.arange(1, 300001, dtype=np.int64)
    got = sac.adam_scalars_reference(lr, C.BETA1, C.BETA2, C.ADAM_EPS, t)
    bias1 = 1.0 - np.array([C.BETA1 ** int(k) for k in t])
    bias2 = 1.0 - np.array([C.BETA2 ** int(k) for k in t])
    want = np.empty_like(got)
    want[:, 0], want[:, 1], want[:, 2] = np.float32(1.0 - C.BETA1), np.float32(C.BETA2), np.float32(1.0 - C.BETA2)
    want[:, 3], want[:, 4], want[:, 5] = (lr / bias1).astype(np.float32), np.sqrt(bias2).astype(np.float32), np.float32(C.ADAM_EPS)
    differ = np.flatnonzero((C.bits(got) != C.bits(want)).any(axis=1))
    assert differ.size == 0, f"first differing steps: {t[differ[:5]]}"
    for k in (1, 2, 999, 300000):          # the vectorised `want` is the per-step formula
        assert np.array_equal(C.bits(want[k - 1]), C.bits(existing_scalars(k, lr))), k


def test_reference_shapes_and_domain():
    one = sac.adam_scalars_reference(3e-4, 0.9, 0.999, 1e-8, 7)
    assert one.shape == (6,) and one.dtype == np.float32
    many = sac.adam_scalars_reference(3e-4, 0.9, 0.999, 1e-8, [[7, 8]])
    assert many.shape == (1, 2, 6) and np.array_equal(C.bits(many[0, 0]), C.bits(one))
    assert one[3] == np.float32(3e-4 / (1.0 - 0.9 ** 7))
    with pytest.raises(ValueError):
        sac.adam_scalars_reference(3e-4, 0.9, 0.999, 1e-8, 0)
    big = sac.adam_scalars_reference(3e-4, 0.9, 0.999, 1e-8, 2 ** 40)       # beta^t underflows to 0: bias = 1
    assert big[3] == np.float32(3e-4) and big[4] == np.float32(1.0)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    return sanitized_program_cases("sac_updates_args_main", tmp_path_factory)


def test_acceptable_arguments(cases):
    for name in ("good", "mode_tiled", "mode_wide", "smallest", "largest", "untuned", "long_workspace", "interval_1000",
                 "scalars_good"):
        assert cases[name] == ["ok"], name


def test_rejections_name_the_argument(cases):
    assert cases["null_args"] == ["sac: null args"]
    assert cases["mode_bad"] == ["sac: mode must be one of SIT_SAC_UPDATES_*"] * 2
    assert cases["batch_not_positive"] == ["sac: batch must be positive"] * 3
    assert cases["n_updates_not_positive"] == ["sac: n_updates must be positive"] * 3
    assert cases["results_capacity_not_positive"] == ["sac: results_capacity must be positive"] * 3
    assert cases["interval_not_positive"] == ["sac: target_update_interval must be positive"] * 3
    for field in ("critic_weights", "critic_m", "critic_v", "actor_weights", "actor_m", "actor_v", "target_weights", "alpha",
                  "log_alpha", "log_alpha_m", "log_alpha_v", "state", "action", "reward", "next_state", "mask", "y",
                  "workspace", "clock", "results"):
        assert cases["null_" + field] == [f"sac: {field} is required"], field
    for field in ("critic_weights", "critic_m", "critic_v", "actor_weights", "actor_m", "actor_v", "target_weights"):
        assert cases["misaligned_" + field] == [f"sac: {field} must be 16-byte aligned"] * 3, field     # 4, 8, 12 bytes
    assert cases["misaligned_alpha"] == ["sac: alpha must be 4-byte aligned"]
    assert cases["misaligned_log_alpha"] == ["sac: log_alpha and its moments must be 4-byte aligned"]
    assert cases["misaligned_clock"] == ["sac: clock must be 8-byte aligned"]
    assert cases["misaligned_results"] == ["sac: results must be 4-byte aligned"]
    assert cases["misaligned_workspace"] == ["sac: workspace must be 4-byte aligned"]
    assert cases["short_workspace"] == ["sac: workspace is too small"] * 2
    assert cases["critic_beta_1"] == ["sac: betas must lie in [0, 1)"]
    assert cases["actor_lr_negative"] == ["sac: lr must be >= 0"]
    assert cases["alpha_eps_negative"] == ["sac: eps must be >= 0"]
    assert cases["scalars_null_adam"] == ["sac: null args"]
    assert cases["scalars_t0_0"] == ["sac: t0 must be at least 1"]
    assert cases["scalars_n_0"] == ["sac: n must be positive"]
    assert cases["scalars_null_out"] == ["sac: out is required"]


@pytest.mark.parametrize("tag", sorted(HYPER))
def test_host_scalars_are_the_reference_bits(cases, tag):
    lr, b1, b2 = HYPER[tag]
    for t in STEPS:
        want = sac.adam_scalars_reference(lr, b1, b2, 1e-8, t)
        assert cases[f"scalars_{tag}_{t}"] == [" ".join(f"{int(u):08x}" for u in C.bits(want))], (tag, t)
