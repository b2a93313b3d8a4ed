"""Host-side pieces of the wide row-kernel calls (sit_sac_target_wide / sit_sac_critic_step_wide /
sit_sac_policy_step_wide, csrc/sit_sac_rows.h): their declarations in the header, in the ctypes table and in the
built library, and SacLearner's row_pass argument.  No GPU."""
import ctypes
import os
import re

import pytest

from sac_maritime_ast_amd import _lib, sac
from sac_maritime_ast_amd.samplers import GaussianPolicy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = {"sit_sac_target_wide": ("sit_sac_target", "sit_sac_target_args", _lib.SacTargetArgs),
        "sit_sac_critic_step_wide": ("sit_sac_critic_step", "sit_sac_critic_step_args", _lib.SacCriticStepArgs),
        "sit_sac_policy_step_wide": ("sit_sac_policy_step", "sit_sac_policy_step_args", _lib.SacPolicyStepArgs)}


def test_header_declares_the_wide_calls():
    text = open(os.path.join(ROOT, "include", "sit.h")).read()
    for name, (_, args, _) in WIDE.items():
        assert re.search(rf"\bint {name}\(sit_handle\* h, const {args}\* a, void\* stream\);", text), name
    assert re.search(r"#define SIT_ABI_VERSION\s+1\b", text)


def test_lib_declares_the_wide_calls_as_the_plain_ones():
    for name, (plain, _, struct) in WIDE.items():
        assert name in _lib.SIGNATURES, name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[plain], name
        assert _lib.SIGNATURES[name][1][1]._type_ is struct, name


def test_built_library_exports_the_wide_calls():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsit.so is not built")
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in WIDE:
        assert hasattr(raw, name), name
    lib = _lib.load()
    for name in WIDE:
        assert getattr(lib, name).restype is ctypes.c_int32, name


def test_row_pass_argument_is_validated():
    hip = dict(gradient="hip", weight_gradient="mfma")
    for bad in ("wmma", "", "MFMA", None):
        with pytest.raises(ValueError, match=r"^row_pass must be 'valu' or 'mfma'$"):
            sac.SacLearner(None, GaussianPolicy(), row_pass=bad, **hip)
    with pytest.raises(ValueError, match=r"^row_pass='mfma' needs weight_gradient='mfma'$"):
        sac.SacLearner(None, GaussianPolicy(), gradient="hip", weight_gradient="sum", row_pass="mfma")
    with pytest.raises(ValueError, match=r"^row_pass='mfma' needs weight_gradient='mfma'$"):
        sac.SacLearner(None, GaussianPolicy(), row_pass="mfma")                  # the defaults: torch, sum
    # the earlier checks still run first
    with pytest.raises(ValueError, match="target must be"):
        sac.SacLearner(None, GaussianPolicy(), target="cuda", row_pass="wmma")
    with pytest.raises(ValueError, match="gradient must be"):
        sac.SacLearner(None, GaussianPolicy(), gradient="cuda", row_pass="mfma")
    with pytest.raises(ValueError, match="needs target='hip'"):
        sac.SacLearner(None, GaussianPolicy(), gradient="hip", target="torch", weight_gradient="mfma", row_pass="mfma")
    with pytest.raises(ValueError, match="weight_gradient must be"):
        sac.SacLearner(None, GaussianPolicy(), gradient="hip", weight_gradient="wmma", row_pass="mfma")
    with pytest.raises(ValueError, match="needs gradient='hip'"):
        sac.SacLearner(None, GaussianPolicy(), gradient="torch", weight_gradient="mfma", row_pass="mfma")
