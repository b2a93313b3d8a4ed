"""CPU checks of the episode records: the ABI additions and episodes_reference (the executable
specification of include/sit.h "episode records") on golden fixtures of the reference's own runs."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import ROOT, golden

from sac_maritime_ast_amd import _lib, episodes, status_string
from sac_maritime_ast_amd.episodes import episodes_reference

# reference status string pieces -> bits (a terminal-state bit is set when its "not in terminal
# state" piece is absent)
PIECES = {"|Test ship reaches endpoint|": _lib.ST_TEST_ENDPOINT, "|Test ship hits map horizon|": _lib.ST_TEST_HORIZON,
          "|Test ship collides with the terrain|": _lib.ST_TEST_TERRAIN,
          "|Test ship mechanical failure|": _lib.ST_TEST_MECHANICAL,
          "|Test ship navigation failure|": _lib.ST_TEST_NAVIGATION,
          "|Test ship blackout failure|": _lib.ST_TEST_BLACKOUT,
          "|Obstacle ship reaches endpoint|": _lib.ST_OBS_ENDPOINT,
          "|Obstacle ship hits map horizon|": _lib.ST_OBS_HORIZON,
          "|Obstacle ship collides with the terrain|": _lib.ST_OBS_TERRAIN,
          "|Obstacle ship IW sampled in terminal state|": _lib.ST_OBS_IW_TERMINAL,
          "|Obstacle ship navigation failure|": _lib.ST_OBS_NAVIGATION, "|Ship collision|": _lib.ST_COLLISION}


def status_bits(text: str) -> int:
    bits = sum(bit for piece, bit in PIECES.items() if piece in text)
    if "|Test ship not in terminal state|" not in text:
        bits |= _lib.ST_TEST_DONE
    if "|Obstacle ship not in terminal state|" not in text:
        bits |= _lib.ST_OBS_DONE
    assert status_string(bits) == text
    return bits


def fixture_rows(name):
    """A golden env fixture as the reducer's rows for one env: reward, done, status [K], action [K, 4]
    (IW north, IW east, NaN angle, SAC_update), next_state [K, 10]."""
    d = golden(name)
    K = len(d["reward"])
    status = np.array([status_bits(str(s)) for s in d["status"]], dtype=np.int64)
    action = np.stack([d["action_n"], d["action_e"], np.arange(K) * 0.25 - 1.0, d["sac_update"]], axis=1)
    return dict(reward=d["reward"].copy(), done=d["done"].copy(), status=status, action=action,
                next_state=d["next_state"].copy()), d


def left_to_right_sum(x):
    s = 0.0
    for v in x:
        s = s + float(v)
    return s


def test_header_constants_match_binding():
    src = open(os.path.join(ROOT, "include", "sit.h")).read()
    for name in ("SIT_EPISODE_ACTIONS", "SIT_EPISODE_DIM"):
        m = re.search(rf"#define {name} (\d+)", src)
        assert m and int(m.group(1)) == getattr(_lib, name), name
    assert _lib.SIT_EPISODE_DIM == 8 + _lib.SIT_OBS_DIM + _lib.SIT_EPISODE_ACTIONS
    assert "call reset once before capturing" in re.sub(r"\s+", " ", src)


def test_episodes_args_layout():
    lib = _lib.load()
    assert lib.sit_episodes_args_size() == ctypes.sizeof(_lib.EpisodesArgs)


def test_update_rejects_null_handle():
    lib = _lib.load()
    a = _lib.EpisodesArgs()
    assert lib.sit_episodes_update(None, ctypes.byref(a), None) == _lib.SIT_E_INVALID
    assert lib.sit_episodes_reset(None, None) == _lib.SIT_E_INVALID


@pytest.mark.parametrize("name,rows", [("env_collision", 12), ("env_test_terrain", 13), ("env_test_arrival", 40),
                                       ("env_nominal", 1694)])
def test_reference_on_golden_episode(name, rows):
    r, d = fixture_rows(name)
    assert len(r["reward"]) == rows
    rec, hist, carry = episodes_reference(**r, env_id_offset=7)
    assert rec.shape == (1, _lib.SIT_EPISODE_DIM)
    c = episodes.columns(rec)
    assert c["env"][0] == 7 and c["episode"][0] == 0 and c["steps"][0] == rows and c["row"][0] == rows - 1
    assert status_string(int(c["status"][0])) == str(d["status"][-1])
    assert c["ret"][0] == left_to_right_sum(d["reward"])
    assert c["terminal_reward"][0] == d["reward"][-1]
    assert np.array_equal(c["terminal_state"][0], d["next_state"][-1])
    n_ev = int(np.count_nonzero(d["sac_update"]))
    assert c["events"][0] == n_ev
    ang = r["action"][d["sac_update"] != 0, 2][:_lib.SIT_EPISODE_ACTIONS]
    assert np.array_equal(c["angles"][0, :len(ang)], ang) and np.isnan(c["angles"][0, len(ang):]).all()
    bits = int(c["status"][0])
    assert np.array_equal(hist, [(bits >> b) & 1 for b in range(32)])
    assert carry["steps"][0] == 0 and carry["ret"][0] == 0.0 and carry["episode"][0] == 1
    assert carry["rows_seen"] == rows and np.isnan(carry["angle"]).all()


def test_reference_without_done_keeps_carry():
    r, d = fixture_rows("env_many_inserts")
    rec, hist, carry = episodes_reference(**r)
    assert rec.shape == (0, _lib.SIT_EPISODE_DIM) and not hist.any()
    assert carry["steps"][0] == 300 and carry["rows_seen"] == 300 and carry["episode"][0] == 0
    assert carry["ret"][0] == left_to_right_sum(d["reward"])
    assert carry["events"][0] == np.count_nonzero(d["sac_update"])


@pytest.mark.parametrize("name", ["env_collision", "env_test_terrain", "env_test_arrival", "env_nominal",
                                  "env_many_inserts"])
def test_reference_split_with_carry_is_bit_identical(name):
    r, _ = fixture_rows(name)
    K = len(r["reward"])
    whole, hist, carry = episodes_reference(**r)
    rng = np.random.default_rng(K)
    for cut in sorted({1, K - 1, *rng.integers(1, K, 3).tolist()}):
        a, ha, ca = episodes_reference(**{k: v[:cut] for k, v in r.items()})
        b, hb, cb = episodes_reference(**{k: v[cut:] for k, v in r.items()}, carry=ca)
        both = np.concatenate([a, b])
        assert both.tobytes() == whole.tobytes(), f"{name} cut {cut}"
        assert np.array_equal(ha + hb, hist)
        assert cb["rows_seen"] == K and cb["steps"][0] == carry["steps"][0]
        assert np.array_equal(cb["ret"], carry["ret"]) and np.array_equal(cb["angle"], carry["angle"], equal_nan=True)


def test_reference_skips_no_step_rows_and_optional_inputs():
    reward = np.array([[1.0], [np.nan], [2.0], [np.nan], [4.0]], dtype=np.float32)
    status = np.array([[0], [_lib.ST_NO_STEP], [_lib.ST_COLLISION], [_lib.ST_NO_STEP], [0]])
    done = np.array([[0], [1], [1], [1], [0]])
    rec, hist, carry = episodes_reference(reward, done, status)
    c = episodes.columns(rec)
    assert rec.shape[0] == 1 and c["steps"][0] == 2 and c["ret"][0] == 3.0 and c["row"][0] == 2 and c["events"][0] == 0
    assert np.isnan(rec[0, 8:]).all()
    assert hist[11] == 1 and hist.sum() == 1
    assert carry["steps"][0] == 1 and carry["ret"][0] == 4.0
