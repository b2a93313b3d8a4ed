"""CPU checks of the observation normalisation (sac_maritime_ast_amd/obsnorm.py, csrc/sit_obsnorm_args.h): the
NumPy specification against a plain loop of the documented tree, its statistics against np.mean / np.var, the
book-keeping of seen / skipped / max_new, apply and fold, the sampled minibatch, the folded actor's error, and the
argument checks as a stand-alone sanitized program."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import ROOT, sanitized_program_cases

sit = pytest.importorskip("sac_maritime_ast_amd")
from sac_maritime_ast_amd import _lib, obsnorm, replay_reference  # noqa: E402
from sac_maritime_ast_amd.obsnorm import ObsNormReference  # noqa: E402
import obsnorm_cases as C  # noqa: E402


def test_package_exports():
    for name in ("ObsNormalizer", "ObsNormReference", "REFERENCE_OBS_LOW", "REFERENCE_OBS_HIGH"):
        assert getattr(sit, name) is getattr(obsnorm, name) and name in sit.__all__, name
    assert obsnorm.REFERENCE_OBS_LOW.shape == obsnorm.REFERENCE_OBS_HIGH.shape == (10,)
    assert np.all(obsnorm.REFERENCE_OBS_HIGH > obsnorm.REFERENCE_OBS_LOW)
    want = 1e-3 * (obsnorm.REFERENCE_OBS_HIGH.astype(np.float64) - obsnorm.REFERENCE_OBS_LOW) / 2
    assert np.array_equal(obsnorm.default_min_std(), want.astype(np.float32))


def test_header_constants_match_binding():
    src = open(os.path.join(ROOT, "include", "sit.h")).read()
    for name in ("SIT_OBSNORM_DIM", "SIT_OBSNORM_AFFINE"):
        assert int(re.search(rf"#define {name} (\d+)", src).group(1)) == getattr(_lib, name), name
    assert (obsnorm.DIM, obsnorm.AFFINE) == (64, 48)
    assert re.search(r"#define SIT_ABI_VERSION 1\b", src)
    # the new section stands behind the learner's, the normalised sample behind the plain one
    assert src.index("sit_sac_adam_scalars(") < src.index("sit_obsnorm_args_size(") < src.index("sit_obsnorm_reset(")
    assert src.index("int sit_replay_sample(") < src.index("int sit_replay_sample_normalised(") < src.index("sit_sac_target_args")
    assert src.index("sit_episodes_set(") < src.index("sit_score_reset(") < src.index("sit_replay_reserve(")


def test_args_layout_and_null_handle():
    lib = _lib.load()
    assert lib.sit_obsnorm_args_size() == ctypes.sizeof(_lib.ObsnormArgs)
    assert lib.sit_obsnorm_reset(None, None, None, None, None) == _lib.SIT_E_INVALID
    assert lib.sit_obsnorm_reserve(None, 1) == _lib.SIT_E_INVALID
    assert lib.sit_obsnorm_update(None, ctypes.byref(_lib.ObsnormArgs()), None) == _lib.SIT_E_INVALID
    assert lib.sit_obsnorm_apply(None, None, None, None, 1, None) == _lib.SIT_E_INVALID
    assert lib.sit_obsnorm_fold(None, None, None, None, None) == _lib.SIT_E_INVALID
    assert lib.sit_replay_sample_normalised(None, ctypes.byref(_lib.ReplaySampleArgs()), None, None) == _lib.SIT_E_INVALID


def test_build_tracks_the_new_headers():
    """build() recompiles the strict translation unit, and only it, when one of the new headers changes."""
    import __graft_entry__ as g
    for name in ("sit_obsnorm.h", "sit_obsnorm_args.h"):
        path = os.path.join(g.PKG, "csrc", name)
        assert os.path.exists(path) and path in g.HEADERS, name
        assert path in g.TU_DEPS[g.SOURCES[0]] and path not in g.TU_DEPS[g.SOURCES[1]], name
    src = open(g.SOURCES[0]).read()
    assert '#include "sit_obsnorm.h"' in src and "obsnorm" not in open(g.SOURCES[1]).read()
    # nor does anything the float32 step TU includes
    for name in ("sit_host.h", "sit_impl.h", "sit_device.h", "sit_serve.h", "sit_sync.h", "sit_actor.h"):
        assert '#include "sit_obsnorm' not in open(os.path.join(g.PKG, "csrc", name)).read(), name


# ---------------------------------------------------------------------------------------------
# update
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", C.SIZES)
def test_update_is_the_documented_loop(m):
    rec = C.rows(m, 100 + m)
    mem = C.memory(rec, m + 3, m)
    before = mem.ring.copy()
    ref = ObsNormReference()
    ref.update(mem)
    block, affine = C.plain_update(np.zeros(64), obsnorm.new_affine(), mem.ring, m, m + 3, m + 3)
    assert np.array_equal(C.bits(ref.block), C.bits(np.array(block)))
    assert np.array_equal(C.bits(ref.affine), C.bits(np.array(affine, dtype=np.float32)))
    assert np.array_equal(C.bits(mem.ring), C.bits(before)) and int(mem.cursor[2]) == 0     # the memory is only read
    out = ref.read()
    assert (out["n"], out["updates"], out["seen"], out["skipped"]) == (m, 1, m, 0)
    assert not ref.block[18:24].any() and not ref.block[34:].any() and not ref.block[4:8].any()
    assert not ref.affine[10:16].any() and not ref.affine[26:32].any() and not ref.affine[42:].any()


def test_second_update_merges_as_the_documented_loop():
    rec = C.rows(700, 8)
    ref = ObsNormReference()
    block, affine = np.zeros(64), obsnorm.new_affine()
    for pushed in (257, 700):
        mem = C.memory(rec, 1024, pushed, 32)
        ref.update(mem)
        block, affine = C.plain_update(block, affine, mem.ring, pushed, 1024, 1024)
    assert np.array_equal(C.bits(ref.block), C.bits(np.array(block)))
    assert np.array_equal(C.bits(ref.affine), C.bits(np.array(affine, dtype=np.float32)))


def test_statistics_against_numpy_after_three_uneven_updates():
    rec = C.rows(5000, 3)
    ref = ObsNormReference()
    for pushed in (1, 1300, 5000):
        ref.update(C.memory(rec, 8192, pushed))
    out = ref.read()
    x = rec[:, :10]
    assert out["n"] == 5000 and out["updates"] == 3
    assert np.max(np.abs(out["mean"] - x.mean(0)) / np.abs(x.mean(0))) <= 1e-12
    assert np.max(np.abs(out["std"] ** 2 - x.var(0)) / x.var(0)) <= 1e-12
    assert np.array_equal(out["shift"], out["mean"].astype(np.float32))
    assert np.array_equal(out["scale"], (1.0 / out["std"]).astype(np.float32))     # no column is at its floor here


def test_min_std_bounds_the_scale():
    rec = C.rows(300, 4)
    rec[:, 2] = 0.25                                         # a constant column: std 0
    ref = ObsNormReference()
    ref.update(C.memory(rec, 300, 300))
    floor = obsnorm.default_min_std()
    assert ref.scale[2] == np.float32(1.0 / np.float64(floor[2])) and ref.shift[2] == np.float32(0.25)
    wide = ObsNormReference(min_std=1e9)
    wide.update(C.memory(rec, 300, 300))
    assert np.all(wide.scale == np.float32(1e-9))
    with pytest.raises(ValueError, match="min_std"):
        ObsNormReference(min_std=-1.0)


def test_wrap_and_skip_bookkeeping():
    ref, reads, rec = C.run_sequence("wrap_and_skip")
    assert [(r["n"], r["seen"], r["skipped"], r["updates"]) for r in reads] == [(200, 200, 0, 1), (450, 450, 0, 2),
                                                                                 (750, 1200, 450, 3)]
    x = np.concatenate([rec[:450, :10], rec[900:1200, :10]])
    assert np.max(np.abs(reads[-1]["mean"] - x.mean(0)) / np.abs(x.mean(0))) <= 1e-12
    assert np.max(np.abs(reads[-1]["std"] ** 2 - x.var(0)) / x.var(0)) <= 1e-12


def test_max_new_leaves_the_remainder_to_the_next_update():
    ref, reads, rec = C.run_sequence("max_new")
    assert [(r["n"], r["seen"], r["skipped"]) for r in reads] == [(100, 100, 0), (200, 200, 0), (250, 250, 0)]
    x = rec[:250, :10]
    assert np.max(np.abs(reads[-1]["mean"] - x.mean(0)) / np.abs(x.mean(0))) <= 1e-12
    with pytest.raises(ValueError, match="max_new"):
        ref.update(C.memory(rec, 400, 250), 0)


def test_an_update_with_nothing_new_writes_only_its_count():
    ref, reads, _ = C.run_sequence("nothing_new")
    first = ObsNormReference()
    first.update(C.memory(C.rows(120, 5), 300, 120))
    want = first.block.copy()
    want[1] = 2
    assert np.array_equal(C.bits(ref.block), C.bits(want)) and np.array_equal(C.bits(ref.affine), C.bits(first.affine))
    empty = ObsNormReference()
    empty.update(replay_reference(16))
    want = np.zeros(64)
    want[1] = 1
    assert np.array_equal(C.bits(empty.block), C.bits(want))
    assert np.array_equal(C.bits(empty.affine), C.bits(obsnorm.new_affine()))


def test_from_bounds_is_frozen():
    ref = ObsNormReference.from_bounds()
    lo, hi = obsnorm.REFERENCE_OBS_LOW.astype(np.float64), obsnorm.REFERENCE_OBS_HIGH.astype(np.float64)
    assert np.array_equal(ref.shift, ((lo + hi) / 2).astype(np.float32))
    assert np.array_equal(ref.scale, (2 / (hi - lo)).astype(np.float32))
    edge = ref.normalized(np.stack([lo, hi]))
    assert np.max(np.abs(np.abs(edge) - 1)) <= 1e-6
    with pytest.raises(ValueError, match="fixed"):
        ref.update(replay_reference(16))
    with pytest.raises(ValueError, match="high > low"):
        ObsNormReference.from_bounds(hi, lo)


# ---------------------------------------------------------------------------------------------
# apply, the sampled minibatch, fold
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
def test_apply_is_two_roundings_and_passes_nan(precision):
    dt = C.NP_REAL[precision]
    ref = C.own_statistics(C.rows(500, 2)[:, :10])
    x = C.rows(64, 9)[:, :10].astype(dt)
    x[3, 4] = np.nan
    got = ref.apply(x.copy())
    shift, scale = ref.shift.astype(dt), ref.scale.astype(dt)
    for r in (0, 3, 63):
        for c in range(10):
            want = dt(dt(x[r, c] - shift[c]) * scale[c])
            assert C.bits(got[r, c]) == C.bits(want) or (np.isnan(want) and np.isnan(got[r, c])), (r, c)
    assert got.dtype == dt and np.isnan(got[3, 4]) and np.isnan(got).sum() == 1
    assert np.abs(got[~np.isnan(got)]).max() < 4
    with pytest.raises(ValueError, match="apply"):
        ref.apply(np.zeros((4, 9), dtype=dt))


@pytest.mark.parametrize("precision", [32, 64])
def test_reference_sample_with_a_normaliser_is_sample_then_apply(precision):
    rec = C.rows(300, 6)
    norm = C.own_statistics(rec[:, :10])
    a, b = (C.memory(rec, 300, 300, precision) for _ in range(2))
    got = a.sample(7, 3, normalizer=norm)
    want = b.sample(7, 3)
    raw_state = want["state"].copy()
    norm.apply(want["state"], want["next_state"])
    assert not np.array_equal(raw_state, want["state"])
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(C.bits(got[k]), C.bits(want[k])), k
    assert np.array_equal(a.cursor, b.cursor) and int(a.cursor[2]) == 3
    assert np.array_equal(C.bits(a.ring), C.bits(b.ring))                 # the ring keeps raw observations


def test_identity_fold_returns_the_blocks_bits():
    block = C.default_actor()
    block[5] = -0.0
    assert np.array_equal(C.bits(ObsNormReference().fold(block)), C.bits(block))
    with pytest.raises(ValueError, match="fold"):
        ObsNormReference().fold(block[:-1])


def test_fold_touches_the_first_layer_only_and_follows_the_formula():
    block = C.default_actor()
    ref = C.own_statistics(C.rows(400, 12)[:, :10])
    out = ref.fold(block)
    assert out.dtype == np.float32 and np.array_equal(C.bits(out[C.H * 11:]), C.bits(block[C.H * 11:]))
    for j in (0, 17, 255):
        acc = 0.0
        for i in range(10):
            w = np.float32(block[j * 10 + i] * ref.scale[i])
            assert C.bits(out[j * 10 + i]) == C.bits(w)
            acc = acc + float(w) * float(ref.shift[i])
        assert C.bits(out[C.H * 10 + j]) == C.bits(np.float32(float(block[C.H * 10 + j]) - acc))


@pytest.mark.parametrize("spread,seed", [(1.0, 21), (0.2, 22)])
def test_folded_actor_on_raw_rows_serves_the_normalised_policy(spread, seed):
    """float32 forward of the folded block on raw rows against the float64 forward on float64-normalised rows:
    at most (1 + max |shift| scale) * 4 * e_base, e_base the float32 forward of the unfolded block on
    float32-normalised rows against the same float64 forward.  Rows uniform in the box (factor 2.8), and rows
    clustered in a fifth of it around its middle (a larger factor: the shift is many standard deviations)."""
    block = C.default_actor()
    obs = C.rows(2048, seed, spread)[:, :10]
    if spread < 1:
        obs = (obs + 0.6 * (obsnorm.REFERENCE_OBS_HIGH - obsnorm.REFERENCE_OBS_LOW) / 2).astype(np.float32).astype(np.float64)
    ref = C.own_statistics(obs)
    want = C.head(block, ref.normalized(obs, np.float64), np.float64)
    e_base = np.abs(C.head(block, ref.normalized(obs.astype(np.float32)), np.float32) - want).max()
    e_fold = np.abs(C.head(ref.fold(block), obs.astype(np.float32), np.float32) - want).max()
    factor = C.fold_factor(ref)
    print(f"fold error, spread {spread}: e_base {e_base:.3e} e_fold {e_fold:.3e} ratio {e_fold / e_base:.2f} factor {factor:.1f}")
    assert e_base > 0 and e_fold <= factor * 4 * e_base


# ---------------------------------------------------------------------------------------------
# the argument checks, sanitized
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    return sanitized_program_cases("obsnorm_args_main", tmp_path_factory)


def test_acceptable_arguments(cases):
    for name in ("reset_good", "reset_no_min_std", "reset_zero_min_std", "update_good_f32", "update_good_f64",
                 "update_at_the_reserve", "update_largest", "apply_good_f32", "apply_good_f64", "apply_one_array",
                 "apply_largest", "fold_good", "fold_adjacent", "affine_good"):
        assert cases[name] == ["ok"], name
    assert cases["reserve_good"] == ["ok"] * 2


def test_rejections_name_the_argument(cases):
    assert cases["update_null_args"] == ["obsnorm: null args"]
    assert cases["reset_null_block"] == ["obsnorm: block is required"]
    assert cases["reset_null_affine"] == ["obsnorm: affine is required"]
    assert cases["reset_misaligned_block"] == ["obsnorm: block must be 8-byte aligned"] * 7
    assert cases["reset_misaligned_affine"] == ["obsnorm: affine must be 16-byte aligned"] * 3
    assert cases["reset_bad_min_std"] == ["obsnorm: min_std must be finite and >= 0"] * 3
    assert cases["max_new_not_positive"] == ["obsnorm: max_new must be positive"] * 6
    assert cases["capacity_not_positive"] == ["obsnorm: capacity must be positive"] * 3
    assert cases["update_beyond_the_reserve"] == ["obsnorm: max_new exceeds the reserve (sit_obsnorm_reserve)"] * 2
    for field in ("ring", "cursor", "block", "affine"):
        assert cases["update_null_" + field] == [f"obsnorm: {field} is required"], field
    assert cases["update_misaligned_ring"] == ["obsnorm: ring must be aligned to 4 reals"] * 2
    assert cases["update_misaligned_cursor"] == ["obsnorm: cursor must be 8-byte aligned"]
    assert cases["update_misaligned_block"] == ["obsnorm: block must be 8-byte aligned"]
    assert cases["update_misaligned_affine"] == ["obsnorm: affine must be 16-byte aligned"]
    assert cases["apply_null_affine"] == ["obsnorm: affine is required"]
    assert cases["apply_null_rows_a"] == ["obsnorm: rows_a is required"]
    assert cases["apply_rows_not_positive"] == ["obsnorm: n_rows must be positive"] * 3
    assert cases["apply_rows_too_many"] == ["obsnorm: n_rows must not exceed 2^30"]
    assert cases["apply_misaligned_rows_a"] == ["obsnorm: rows_a must be aligned to 2 reals"] * 2
    assert cases["apply_misaligned_rows_b"] == ["obsnorm: rows_b must be aligned to 2 reals"] * 2
    assert cases["fold_null_affine"] == ["obsnorm: affine is required"]
    assert cases["fold_null_src"] == ["obsnorm: src is required"]
    assert cases["fold_null_dst"] == ["obsnorm: dst is required"]
    assert cases["fold_misaligned_src"] == ["obsnorm: src must be 16-byte aligned"] * 3
    assert cases["fold_misaligned_dst"] == ["obsnorm: dst must be 16-byte aligned"] * 3
    assert cases["fold_overlap"] == ["obsnorm: src and dst must not overlap"] * 4
    assert cases["affine_null"] == ["obsnorm: affine is required"]
    assert cases["affine_misaligned"] == ["obsnorm: affine must be 16-byte aligned"] * 3
    assert len(cases) == 46, sorted(cases)
