"""The argument checks of sit_sac_critic_step / sit_sac_policy_step (csrc/sit_sac_args.h) under ASan + UBSan.

tests/csrc/sac_update_args_main.cpp includes only sit_sac_args.h (and include/sit.h).  It is compiled here
with the host compiler (-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all) and run as a
child process; nothing is preloaded and nothing is loaded into Python.  The library calls the same
functions before any launch (sit_kernels.hip), so these are the messages sit_last_error gives."""
import pytest

from helpers import sanitized_program_cases

ROW = 1040          # SIT_SAC_WORKSPACE_ROW


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    return sanitized_program_cases("sac_update_args_main", tmp_path_factory)


def test_workspace_size(cases):
    assert cases["workspace_floats"] == [f"0 0 {2 * ROW} {2 * 64 * ROW} {2 * (2 ** 31 - 1) * ROW}"]


@pytest.mark.parametrize("call", ["critic", "policy"])
def test_acceptable_arguments(cases, call):
    names = ["good", "batch_1", "batch_2147483647"]
    names += ["long_workspace", "step_1000"] if call == "critic" else ["with_noise", "untuned"]
    for name in names:
        assert cases[f"{call}_{name}"] == ["ok"], name


def test_critic_rejections_name_the_argument(cases):
    assert cases["critic_null_args"] == ["sac: null args"]
    for name in ("batch_0", "batch_-1", "batch_-2147483648"):
        assert cases["critic_" + name] == ["sac: batch must be positive"], name
    for field in ("critic_weights", "critic_m", "critic_v", "state", "action", "y", "workspace", "results"):
        assert cases["critic_null_" + field] == [f"sac: {field} is required"], field
    assert cases["critic_misaligned_weights"] == ["sac: critic_weights must be 16-byte aligned"] * 3   # 4, 8, 12 bytes
    assert cases["critic_misaligned_m"] == ["sac: critic_m must be 16-byte aligned"] * 3
    assert cases["critic_misaligned_v"] == ["sac: critic_v must be 16-byte aligned"] * 3
    assert cases["critic_short_workspace"] == ["sac: workspace is too small"] * 3
    assert cases["critic_bias_0"] == cases["critic_bias_big"] == ["sac: the bias corrections must lie in (0, 1]"]
    assert cases["critic_beta_1"] == ["sac: betas must lie in [0, 1)"]
    assert cases["critic_lr_negative"] == ["sac: lr must be >= 0"]


def test_policy_rejections_name_the_argument(cases):
    assert cases["policy_null_args"] == ["sac: null args"]
    for name in ("batch_0", "batch_-1", "batch_-2147483648"):
        assert cases["policy_" + name] == ["sac: batch must be positive"], name
    for field in ("actor_weights", "actor_m", "actor_v", "critic_weights", "alpha", "log_alpha", "log_alpha_m",
                  "log_alpha_v", "state", "workspace", "results"):
        assert cases["policy_null_" + field] == [f"sac: {field} is required"], field
    assert cases["policy_misaligned_weights"] == ["sac: actor_weights must be 16-byte aligned"] * 3
    assert cases["policy_misaligned_m"] == ["sac: actor_m must be 16-byte aligned"] * 3
    assert cases["policy_misaligned_v"] == ["sac: actor_v must be 16-byte aligned"] * 3
    assert cases["policy_misaligned_critic"] == ["sac: critic_weights must be 16-byte aligned"] * 3
    assert cases["policy_misaligned_alpha"] == ["sac: alpha must be 4-byte aligned"]
    assert cases["policy_misaligned_log_alpha"] == ["sac: log_alpha and its moments must be 4-byte aligned"]
    assert cases["policy_short_workspace"] == ["sac: workspace is too small"]
    assert cases["policy_alpha_bias_0"] == ["sac: the bias corrections must lie in (0, 1]"]
    assert cases["policy_eps_negative"] == ["sac: eps must be >= 0"]
