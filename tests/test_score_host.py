"""CPU checks of the scores (sac_maritime_ast_amd/score.py, csrc/sit_score_args.h): the NumPy specification
against a plain loop, the summation tree, the reference's seven classes against the status texts, the
inverse of pack_actor_weights, and the argument checks as a stand-alone sanitized program."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from helpers import ROOT, sanitized_program_cases
import score_cases as C

sit = pytest.importorskip("sac_maritime_ast_amd")
from sac_maritime_ast_amd import _lib, score, status_string  # noqa: E402
from sac_maritime_ast_amd.score import REFERENCE_CLASSES, score_reference  # noqa: E402


def test_package_exports():
    for name in ("Scoreboard", "Scorer", "score_reference", "REFERENCE_CLASSES"):
        assert getattr(sit, name) is getattr(score, name) and name in sit.__all__


def test_header_constants_match_binding():
    src = open(os.path.join(ROOT, "include", "sit.h")).read()
    for name in ("SIT_SCORE_DIM", "SIT_SCORE_CLASSES", "SIT_SCORE_KEEP_BLOCKS"):
        assert int(re.search(rf"#define {name} (\d+)", src).group(1)) == getattr(_lib, name), name
    for name in ("SIT_SCORE_CONSUME", "SIT_SCORE_FRESH"):
        assert int(re.search(rf"#define {name} (\d+)u", src).group(1)) == getattr(_lib, name), name
    assert re.search(r"#define SIT_ABI_VERSION 1\b", src)
    assert "scoring the same buffer twice counts its records twice" in re.sub(r"[\s*]+", " ", src)
    assert src.index("sit_episodes_set(") < src.index("sit_score_reset(") < src.index("sit_replay_reserve(")


def test_args_layouts_and_null_handle():
    lib = _lib.load()
    assert lib.sit_score_args_size() == ctypes.sizeof(_lib.ScoreArgs)
    assert lib.sit_score_keep_args_size() == ctypes.sizeof(_lib.ScoreKeepArgs)
    assert lib.sit_score_update(None, ctypes.byref(_lib.ScoreArgs()), None) == _lib.SIT_E_INVALID
    assert lib.sit_score_keep(None, ctypes.byref(_lib.ScoreKeepArgs()), None) == _lib.SIT_E_INVALID
    assert lib.sit_score_reset(None, None, None) == _lib.SIT_E_INVALID
    assert lib.sit_score_reserve(None, 1) == _lib.SIT_E_INVALID


def test_build_tracks_the_new_headers():
    """build() recompiles the strict translation unit, and only it, when one of the score headers changes."""
    import __graft_entry__ as g
    for name in ("sit_score.h", "sit_score_args.h"):
        path = os.path.join(g.PKG, "csrc", name)
        assert os.path.exists(path) and path in g.HEADERS, name
        assert path in g.TU_DEPS[g.SOURCES[0]] and path not in g.TU_DEPS[g.SOURCES[1]], name
    src = open(g.SOURCES[0]).read()
    assert '#include "sit_score.h"' in src and "sit_score" not in open(g.SOURCES[1]).read()


def slow_tree(x):
    """The tree of include/sit.h with Python lists and floats."""
    def halve(v):
        v = list(v) + [0.0] * (256 - len(v))
        s = 128
        while s:
            for i in range(s):
                v[i] = v[i] + v[i + s]
            s //= 2
        return v[0]
    chunks = [halve(x[i:i + 256]) for i in range(0, len(x), 256)]
    total = 0.0
    for i in range(0, len(chunks), 256):
        total = total + halve(chunks[i:i + 256])
    return total


@pytest.mark.parametrize("m", C.SIZES)
def test_tree_sum_is_the_documented_tree(m):
    x = C.synthetic(m, 100 + m)[:, 3]
    assert C.bits(score.tree_sum(x)) == C.bits(slow_tree([float(v) for v in x]))


def test_summation_order_shows_in_these_inputs():
    x = C.synthetic(65537, 7)[:, 3]
    forward = 0.0
    for v in x:
        forward = forward + float(v)
    assert len({C.bits(score.tree_sum(x)).item(), C.bits(forward).item(), C.bits(float(np.sum(x))).item()}) > 1


@pytest.mark.parametrize("m", C.SIZES)
def test_reference_against_a_plain_loop(m):
    rec = C.synthetic(m, m)
    before = rec.copy()
    block = score_reference(rec)
    assert block.shape == (64,) and block.dtype == np.float64
    assert np.array_equal(C.bits(rec), C.bits(before))
    C.assert_block_matches_loop(block, C.plain_loop(rec))


FORCED = C.forced_cases()


@pytest.mark.parametrize("name", sorted(FORCED))
def test_forced_cases(name):
    rec, kw = FORCED[name]
    block = score_reference(rec, **kw)
    classes = kw.get("classes", REFERENCE_CLASSES)
    C.assert_block_matches_loop(block, C.plain_loop(rec, classes, kw.get("episode_limit", 0)), classes)
    if name == "equal_best":
        assert block[32 + 3] == 7.25 and block[32 + 0] == 130 % 37 and block[32 + 1] == 130 // 37
    if name == "nan_return":
        assert block[0] == 300 and np.isnan(block[1]) and block[4] < 0 and not np.isnan(block[35])
    if name == "nan_only":
        assert block[0] == 5 and block[3] == math.inf and block[4] == -math.inf and block[7] == 0
    if name == "minus_zero":
        for k in (1, 3, 4):
            assert block[k] == 0.0 and not np.signbit(block[k]), k
        assert block[35] == 0.0 and block[32 + 1] == 0 and block[32 + 0] == 0    # slot 0
    if name == "empty":
        want = score.new_block()
        want[6] = 1
        assert np.array_equal(C.bits(block), C.bits(want))
    if name == "limit_1":
        assert block[0] == 200 and block[32 + 1] == 0
    if name == "limit_2":
        assert block[0] == 400 and block[32 + 1] in (0, 1)
    if name == "unused_class":
        assert block[8 + 2] == 0 and block[8 + 1] > 0
    if name == "eight_classes":
        assert block[15] > 0


@pytest.mark.parametrize("cuts", [(0,), (1, 256), (255, 255, 700), (300, 301, 302, 1000)])
def test_partition_with_carry(cuts):
    """Feeding the records in pieces gives the same integers, min, max and best as one piece (the sum is
    another order of the same terms: within the bound)."""
    rec = C.synthetic(1100, 21)
    rec[[100, 400, 900], 3] = 5e3                      # the same greatest return in three pieces: the first stays
    whole = score_reference(rec)
    block, loop = None, None
    edges = [0, *cuts, len(rec)]
    for a, b in zip(edges[:-1], edges[1:]):
        block = score_reference(rec[a:b], block)
        loop = C.plain_loop(rec[a:b], carry=loop)
    C.assert_block_matches_loop(block, loop)
    same = [0, 2, 3, 4, 5, *range(8, 64)]
    assert np.array_equal(C.bits(block[same]), C.bits(whole[same]))
    assert block[6] == len(edges) - 1 and block[32 + 0] == 100 % 37 and block[32 + 1] == 100 // 37


def test_carry_is_not_modified_and_limits_are_checked():
    rec = C.synthetic(40, 3)
    first = score_reference(rec[:20])
    kept = first.copy()
    score_reference(rec[20:], first)
    assert np.array_equal(C.bits(first), C.bits(kept))
    with pytest.raises(ValueError, match="episode_limit"):
        score_reference(rec, episode_limit=-1)
    with pytest.raises(ValueError, match="classes"):
        score_reference(rec, classes=[("c", 1, 0)] * 9)


CLASS_TEXTS = {"blackout": ("|Test ship blackout failure|",),
               "mechanical": ("|Test ship mechanical failure|",),
               "navigation": ("|Test ship navigation failure|",),
               "collision": ("|Ship collision|", "|Test ship collides with the terrain|"),
               "arrival": ("|Test ship reaches endpoint|",),
               "route_or_horizon": ("|Obstacle ship IW sampled in terminal state|", "|Test ship hits map horizon|",
                                    "|Obstacle ship hits map horizon|"),
               "not_terminal": ("Test ship not in terminal state",)}


def test_reference_classes_follow_the_status_texts():
    """For all 2^14 status masks, one record each: a default class counts the record exactly when one of
    its texts is in status_string(bits)."""
    assert [c[0] for c in REFERENCE_CLASSES] == list(CLASS_TEXTS)
    masks = np.arange(1 << 14)
    rec = np.zeros((len(masks), C.DIM))
    rec[:, 4] = masks
    texts = [status_string(int(b)) for b in masks]
    want = [sum(any(t in s for t in CLASS_TEXTS[name]) for s in texts) for name, _, _ in REFERENCE_CLASSES]
    assert list(score_reference(rec)[8:15]) == want
    for b in (0, 1, 1 << 5, 1 << 11, (1 << 12) | (1 << 2), (1 << 9) | (1 << 13), (1 << 14) - 1):
        got = score_reference(rec[b:b + 1])[8:15]
        assert list(got) == [float(any(t in texts[b] for t in CLASS_TEXTS[name])) for name, _, _ in REFERENCE_CLASSES], b
    # record by record: every mask with a text of the class counts for it, and no other mask does
    for k, (name, _, _) in enumerate(REFERENCE_CLASSES):
        hit = np.array([any(t in s for t in CLASS_TEXTS[name]) for s in texts])
        assert score_reference(rec[hit])[8 + k] == hit.sum() > 0 and score_reference(rec[~hit])[8 + k] == 0, name


def test_read_block_names_the_fields():
    rec = C.synthetic(300, 5)
    out = score.read_block(score_reference(rec))
    loop = C.plain_loop(rec)
    assert out["episodes"] == 300 and out["updates"] == 1 and out["dropped"] == 0 and out["best_stamp"] is None
    assert out["mean_steps"] == loop["steps"] / 300 and out["min"] == loop["min"] and out["max"] == loop["max"]
    assert out["status_record"] == dict(zip([c[0] for c in REFERENCE_CLASSES], loop["classes"]))
    assert out["best"]["ret"] == loop["best"][3] and out["best"]["env"] == int(loop["best"][0])
    assert out["best"]["terminal_state"].shape == (10,) and out["best"]["angles"].shape == (14,)
    empty = score.read_block(score.new_block())
    assert empty["episodes"] == 0 and empty["best"] is None and math.isnan(empty["mean_return"])


def test_unpack_actor_weights_round_trips():
    torch = pytest.importorskip("torch")
    from sac_maritime_ast_amd.samplers import GaussianPolicy, pack_actor_weights, unpack_actor_weights
    torch.manual_seed(3)
    p, q = GaussianPolicy(), GaussianPolicy()
    block = pack_actor_weights(p)
    assert not torch.equal(pack_actor_weights(q), block)
    assert unpack_actor_weights(block, q) is q
    for a, b in zip(p.parameters(), q.parameters()):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(pack_actor_weights(q).view(torch.int32), block.view(torch.int32))
    with pytest.raises(ValueError, match="architecture"):
        unpack_actor_weights(block, GaussianPolicy(hidden=(64, 64)))
    with pytest.raises(ValueError, match="block"):
        unpack_actor_weights(block[:-1], q)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    return sanitized_program_cases("score_args_main", tmp_path_factory)


def test_acceptable_arguments(cases):
    for name in ("good", "flag_consume", "flag_fresh", "flag_both", "smallest", "largest", "limit_2", "all_class_bits",
                 "reset_good", "keep_good", "keep_no_stamp", "keep_no_blocks", "keep_one_block", "keep_largest"):
        assert cases[name] == ["ok"], name
    assert cases["reserve_good"] == ["ok"] * 2


def test_rejections_name_the_argument(cases):
    assert cases["null_args"] == ["score: null args"] and cases["keep_null_args"] == ["score: null args"]
    assert cases["flags_unknown"] == ["score: flags has unknown bits"] * 2
    assert cases["limit_negative"] == ["score: episode_limit must be >= 0"] * 2
    assert cases["capacity_not_positive"] == ["score: record_capacity must be positive"] * 3
    assert cases["max_records_not_positive"] == ["score: max_records must be positive"] * 3
    for field in ("records", "record_count", "score"):
        assert cases["null_" + field] == [f"score: {field} is required"], field
        assert cases["misaligned_" + field] == [f"score: {field} must be 8-byte aligned"] * 7, field
    assert cases["reset_null_score"] == ["score: score is required"]
    assert cases["reset_misaligned_score"] == ["score: score must be 8-byte aligned"] * 7
    assert cases["keep_n_blocks_outside"] == ["score: n_blocks must lie in 0..4"] * 3
    assert cases["keep_floats_too_many"] == ["score: floats must not exceed 2^34"]
    assert cases["keep_floats_not_positive"] == ["score: floats must be positive"] * 8
    assert cases["keep_null_src"] == ["score: src is required"] * 4
    assert cases["keep_null_dst"] == ["score: dst is required"] * 4
    assert cases["keep_misaligned_src"] == ["score: src must be 16-byte aligned"] * 12
    assert cases["keep_misaligned_dst"] == ["score: dst must be 16-byte aligned"] * 12
    assert cases["keep_null_score"] == ["score: score is required"]
    assert cases["keep_misaligned_score"] == ["score: score must be 8-byte aligned"]
    assert cases["keep_misaligned_stamp"] == ["score: stamp must be 8-byte aligned"]
    assert len(cases) == 39, sorted(cases)
