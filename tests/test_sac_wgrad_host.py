"""Host-side pieces of the tiled weight-gradient calls (sit_sac_critic_step_tiled / sit_sac_policy_step_tiled,
csrc/sit_sac_wgrad.h): their declarations in the header, in the ctypes table and in the built library, and
SacLearner's weight_gradient argument.  No GPU."""
import ctypes
import os
import re

import pytest

from sac_maritime_ast_amd import _lib, sac
from sac_maritime_ast_amd.samplers import GaussianPolicy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILED = {"sit_sac_critic_step_tiled": ("sit_sac_critic_step", "sit_sac_critic_step_args"),
         "sit_sac_policy_step_tiled": ("sit_sac_policy_step", "sit_sac_policy_step_args")}


def test_header_declares_the_tiled_calls():
    text = open(os.path.join(ROOT, "include", "sit.h")).read()
    for name, (_, args) in TILED.items():
        assert re.search(rf"\bint {name}\(sit_handle\* h, const {args}\* a, void\* stream\);", text), name
    assert "#define SIT_ABI_VERSION 1\n" in text or re.search(r"#define SIT_ABI_VERSION\s+1\b", text)


def test_lib_declares_the_tiled_calls_as_the_plain_ones():
    for name, (plain, _) in TILED.items():
        assert name in _lib.SIGNATURES, name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[plain], name
    assert _lib.SIGNATURES["sit_sac_critic_step_tiled"][1][1]._type_ is _lib.SacCriticStepArgs
    assert _lib.SIGNATURES["sit_sac_policy_step_tiled"][1][1]._type_ is _lib.SacPolicyStepArgs


def test_built_library_exports_the_tiled_calls():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsit.so is not built")
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in TILED:
        assert hasattr(raw, name), name
    lib = _lib.load()
    for name in TILED:
        assert getattr(lib, name).restype is ctypes.c_int32, name


def test_weight_gradient_argument_is_validated():
    with pytest.raises(ValueError, match="weight_gradient"):
        sac.SacLearner(None, GaussianPolicy(), gradient="hip", weight_gradient="wmma")
    with pytest.raises(ValueError, match="weight_gradient"):
        sac.SacLearner(None, GaussianPolicy(), weight_gradient="")
    with pytest.raises(ValueError, match="needs gradient='hip'"):
        sac.SacLearner(None, GaussianPolicy(), gradient="torch", weight_gradient="mfma")
    with pytest.raises(ValueError, match="needs gradient='hip'"):
        sac.SacLearner(None, GaussianPolicy(), weight_gradient="mfma")            # the default gradient is torch
    # the other arguments are still checked first, and "sum" passes this check in both gradient modes
    with pytest.raises(ValueError, match="target='hip'"):
        sac.SacLearner(None, GaussianPolicy(), gradient="hip", target="torch", weight_gradient="mfma")
    with pytest.raises(ValueError, match="gradient must be"):
        sac.SacLearner(None, GaussianPolicy(), gradient="cuda", weight_gradient="sum")
