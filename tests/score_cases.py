"""Shared inputs of the score tests (tests/test_score_host.py, tests/test_gpu_score.py): synthetic episode
records whose returns make the summation order visible, the forced cases, and the reduction as a plain loop."""
from __future__ import annotations

import math

import numpy as np

from sac_maritime_ast_amd import _lib
from sac_maritime_ast_amd.score import REFERENCE_CLASSES

DIM = _lib.SIT_EPISODE_DIM
SIZES = (0, 1, 255, 256, 257, 65537)          # 65 537 records: 257 chunks, so two groups at the second level


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


def synthetic(m: int, seed: int = 0, n_env: int = 37) -> np.ndarray:
    """[m, 32] records as an EpisodeLog holds them: env j % n_env, episode j // n_env, returns +-10^U(-3, 3)
    (as the episode tests use: sums in another order round differently), status bits over all 14 reasons."""
    rng = np.random.default_rng(seed)
    rec = rng.standard_normal((m, DIM))
    j = np.arange(m)
    rec[:, 0], rec[:, 1] = j % n_env, j // n_env
    rec[:, 2] = rng.integers(1, 5000, m)
    rec[:, 3] = rng.choice([-1.0, 1.0], m) * 10.0 ** rng.uniform(-3, 3, m)
    rec[:, 4] = rng.integers(0, 1 << 14, m)
    rec[:, 5] = rng.integers(0, 40, m)
    rec[:, 6] = rng.integers(0, 1 << 40, m)
    rec[:, 18:][rng.random((m, DIM - 18)) < 0.5] = np.nan     # NaN-padded angles
    return rec


def forced_cases() -> dict:
    """name -> (records, kwargs of score_reference)."""
    out = {}
    rec = synthetic(700, 11)                    # equal greatest returns in different chunks: slot 130 wins
    rec[:, 3] = -np.abs(rec[:, 3])
    rec[[600, 130, 300], 3] = 7.25
    out["equal_best"] = (rec, {})
    rec = synthetic(300, 12)                    # a NaN return: counted, never min, max or best
    rec[:, 3] = -np.abs(rec[:, 3])
    rec[17, 3] = np.nan
    out["nan_return"] = (rec, {})
    rec = synthetic(5, 13)                      # only NaN returns: no best at all
    rec[:, 3] = np.nan
    out["nan_only"] = (rec, {})
    rec = synthetic(260, 14)                    # returns -0.0 only: min, max and the sum read +0.0
    rec[:, 3] = -0.0
    out["minus_zero"] = (rec, {})
    out["empty"] = (synthetic(0, 15), {})
    out["limit_1"] = (synthetic(600, 16, n_env=200), {"episode_limit": 1})
    out["limit_2"] = (synthetic(600, 17, n_env=200), {"episode_limit": 2})
    unused = list(REFERENCE_CLASSES)
    unused[2] = ("unused", 0, 0)
    out["unused_class"] = (synthetic(300, 18), {"classes": tuple(unused)})
    out["eight_classes"] = (synthetic(300, 19), {"classes": tuple(REFERENCE_CLASSES) + (("any_failure", 0x3C, 0x1),)})
    return out


def plain_loop(records, classes=REFERENCE_CLASSES, episode_limit: int = 0, carry=None) -> dict:
    """The reduction record by record with Python scalars; the return sum as math.fsum (exact, rounded once)."""
    c = carry or {"episodes": 0, "steps": 0, "classes": [0] * len(classes), "min": math.inf, "max": -math.inf,
                  "best": None, "updates": 0, "returns": []}
    c = dict(c, classes=list(c["classes"]), returns=list(c["returns"]))
    best, replaced = None, False
    for slot, rec in enumerate(np.asarray(records).reshape(-1, DIM)):
        if episode_limit and not rec[1] < episode_limit:
            continue
        ret, status = float(rec[3]), int(rec[4])
        c["episodes"] += 1
        c["steps"] += int(rec[2])
        c["returns"].append(ret)
        for k, (_, any_, none) in enumerate(classes):
            if (any_ or none) and (not any_ or status & any_) and not status & none:
                c["classes"][k] += 1
        if math.isnan(ret):
            continue
        c["min"], c["max"] = min(c["min"], ret), max(c["max"], ret)
        if best is None or ret > best[3]:
            best = rec.copy()
    if best is not None and (c["best"] is None or best[3] > c["best"][3]):
        c["best"], replaced = best, True
    c["updates"] += 1
    c["replaced"] = replaced
    return c


def assert_block_matches_loop(block, loop, classes=REFERENCE_CLASSES):
    """Integer fields, min, max and best exactly; the tree sum within (n - 1) 2^-53 sum|ret| of fsum."""
    assert block[0] == loop["episodes"] and block[2] == loop["steps"] and block[6] == loop["updates"]
    assert block[7] == (1.0 if loop["replaced"] else 0.0)
    assert list(block[8:8 + len(classes)]) == loop["classes"] and not block[8 + len(classes):16].any()
    assert block[5] == 0 and not block[17:32].any()
    assert block[3] == loop["min"] and block[4] == loop["max"]
    assert not np.signbit(block[3]) or block[3] != 0.0
    assert not np.signbit(block[4]) or block[4] != 0.0
    if loop["best"] is None:
        assert np.isnan(block[32:]).all()
    else:
        assert np.array_equal(bits(block[32:]), bits(loop["best"]))
    rets = loop["returns"]
    if any(math.isnan(r) for r in rets):
        assert np.isnan(block[1])
    else:
        n = len(rets)
        bound = max(n - 1, 0) * 2.0 ** -53 * math.fsum(abs(r) for r in rets)
        assert abs(block[1] - math.fsum(rets)) <= bound, (block[1], math.fsum(rets), bound)
