"""The argument checks of sit_sac_target / sit_sac_polyak (csrc/sit_sac_args.h) under ASan + UBSan.

tests/csrc/sac_args_main.cpp includes only sit_sac_args.h (and include/sit.h).  It is compiled here
with the host compiler (-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all) and run as a
child process; nothing is preloaded and nothing is loaded into Python.  The library calls the same
two functions before any launch (sit_kernels.hip), so these are the messages sit_last_error gives."""
import pytest

from helpers import sanitized_program_cases


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    return sanitized_program_cases("sac_args_main", tmp_path_factory)


def test_acceptable_arguments(cases):
    for name in ("good", "with_optionals", "batch_1", "batch_2147483647", "polyak_good", "polyak_big"):
        assert cases[name] == ["ok"], name


def test_target_rejections_name_the_argument(cases):
    assert cases["null_args"] == ["sac: null args"]
    for name in ("batch_0", "batch_-1", "batch_-2147483648"):
        assert cases[name] == ["sac: batch must be positive"], name
    for field in ("actor_weights", "critic_weights", "alpha", "next_state", "reward", "mask", "y"):
        assert cases["null_" + field] == [f"sac: {field} is required"], field
    assert cases["misaligned_actor"] == ["sac: actor_weights must be 16-byte aligned"] * 3     # offsets of 4, 8, 12 bytes
    assert cases["misaligned_critic"] == ["sac: critic_weights must be 16-byte aligned"] * 3
    assert cases["misaligned_alpha"] == ["sac: alpha must be 4-byte aligned"]


def test_polyak_rejections_name_the_argument(cases):
    assert cases["polyak_null_target"] == ["sac: target is required"]
    assert cases["polyak_null_online"] == ["sac: online is required"]
    for name in ("polyak_n_0", "polyak_n_negative"):
        assert cases[name] == ["sac: n must be positive"], name
    for name in ("polyak_n_too_big", "polyak_n_max"):
        assert cases[name] == ["sac: n must not exceed 2^34"], name
    assert cases["polyak_misaligned_target"] == ["sac: target must be 16-byte aligned"]
    assert cases["polyak_misaligned_online"] == ["sac: online must be 16-byte aligned"]
