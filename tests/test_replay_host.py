"""CPU checks of the replay memory: the ABI additions and replay_reference (the executable
specification of include/sit.h "replay memory"): canonical push order, the ring and the keyed
permutation behind the minibatches."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import ROOT
from oracle import sit_oracle as so

from sac_maritime_ast_amd import _lib, replay, replay_reference

DIM = _lib.SIT_TRANSITION_DIM


def records(envs, first=0.0, dtype=np.float32, room=None):
    """A source buffer whose row i has env id envs[i] and first + i in every other column."""
    src = np.zeros((len(envs) if room is None else room, DIM), dtype=dtype)
    src[:len(envs), :DIM - 1] = (first + np.arange(len(envs)))[:, None]
    src[:len(envs), DIM - 1] = envs
    return src


def test_philox_equals_oracle():
    m = 0xFFFFFFFF
    kat = [((0, 0, 0, 0), (0, 0), [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
           ((m, m, m, m), (m, m), [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1])]
    for ctr, key, want in kat:
        assert [int(x) for x in replay.philox4x32_10(ctr, key)] == want
        assert [int(x) for x in so.philox4x32_10(ctr, key)] == want
    rng = np.random.default_rng(7)
    ctr = [rng.integers(0, 1 << 32, 1000, dtype=np.uint64) for _ in range(4)]
    key = [rng.integers(0, 1 << 32, 1000, dtype=np.uint64) for _ in range(2)]
    got, want = replay.philox4x32_10(ctr, key), so.philox4x32_10(ctr, key)
    for g, w in zip(got, want):
        assert g.dtype == np.uint32 and np.array_equal(g, w)


def test_push_canonical_order_wrap_overflow_dropped():
    """Seven records of three envs into five slots, then a push that wraps, then one whose source
    buffer had overflowed; every expected ring is written out by hand."""
    mem = replay_reference(5)
    # rows 0..6; env-major with source order inside an env: env 1 rows 1, 4; env 2 rows 3, 6; env 3 rows 0, 2, 5
    mem.push(records([3, 1, 3, 2, 1, 3, 2], room=8), 7)
    # n = 7 > 5: canonical records j = 2..6 (rows 3, 6, 0, 2, 5) go to slots 2, 3, 4, 0, 1
    assert mem.ring[:, 0].tolist() == [2, 5, 3, 6, 0]
    assert mem.ring[:, DIM - 1].tolist() == [3, 3, 2, 2, 3]
    assert mem.cursor.tolist() == [7, 0, 0, 0] and len(mem) == 5
    # canonical rows 13, 11, 12, 10 to slots 7 % 5 = 2, 3, 4, 0
    mem.push(records([9, 4, 4, 0], first=10.0), np.array([4], np.int32))
    assert mem.ring[:, 0].tolist() == [10, 5, 13, 11, 12]
    assert mem.cursor.tolist() == [11, 0, 0, 0]
    # the producer counted 5 records into room for 3: two are dropped; equal ids keep their order
    mem.push(records([5, 5, 5], first=20.0), 5)
    assert mem.ring[:, 0].tolist() == [10, 20, 21, 22, 12]
    assert mem.cursor.tolist() == [14, 2, 0, 0] and mem.dropped == 2
    mem.push(records([1, 2]), 0)
    assert mem.cursor.tolist() == [14, 2, 0, 0]


def test_push_moves_bits():
    src = records([2, 1, 1])
    bits = src.view(np.uint32)
    bits[0, 3], bits[1, 4], bits[2, 5] = 0x7FC12345, 0x80000000, 0xFFC00001     # NaN payloads and -0.0
    want = bits.copy()
    mem = replay_reference(4)
    mem.push(src, 3)
    assert np.array_equal(mem.ring.view(np.uint32)[:3], want[[1, 2, 0]])
    out = mem.sample(3)
    assert np.array_equal(out["state"].view(np.uint32)[0], mem.ring.view(np.uint32)[out["index"][0], :10])


def filled(size, capacity=None, seed=25450):
    mem = replay_reference(capacity or max(size, 1), seed=seed)
    if size:
        mem.push(records(np.arange(size) % 50), size)
    return mem


@pytest.mark.parametrize("size,batch", [(257, 64), (65, 64), (64, 64), (5, 4), (1, 1)])
def test_sample_indices(size, batch):
    mem = filled(size)
    out = mem.sample(batch, 8)
    idx = out["index"]
    assert idx.shape == (8, batch) and idx.dtype == np.int32
    assert idx.min() >= 0 and idx.max() < size
    for row in idx:
        assert len(set(row.tolist())) == batch
    assert np.array_equal(out["state"], mem.ring[idx, :10]) and np.array_equal(out["reward"], mem.ring[idx, 11])
    assert np.array_equal(out["env"], mem.ring[idx, DIM - 1].astype(np.int32))
    assert mem.cursor[2] == 8
    # the same (seed, draw) again; minibatch u of one call is draw number draws + u
    again = filled(size)
    assert np.array_equal(again.sample(batch, 8)["index"], idx)
    one = filled(size)
    one.cursor[2] = 3
    assert np.array_equal(one.sample(batch, 1)["index"][0], idx[3])
    if size > 1:
        assert not np.array_equal(idx[0], idx[1])                                     # the next draw
        assert not np.array_equal(filled(size, seed=1).sample(batch, 8)["index"], idx)   # another seed


def test_sample_wraps_past_size_and_empty_ring():
    mem = filled(40, capacity=64)
    idx = mem.sample(64)["index"][0]
    assert sorted(idx[:40].tolist()) == list(range(40)) and np.array_equal(idx[40:], idx[:24])
    empty = replay_reference(16)
    out = empty.sample(4, 2)
    assert (out["index"] == -1).all() and not out["state"].any() and not out["env"].any()
    assert out["action"].shape == (2, 4, 1) and empty.cursor.tolist() == [0, 0, 2, 0]


def test_permutation_is_a_bijection():
    for size in (1, 2, 3, 4, 5, 16, 17, 64, 65, 257, 1000):
        x = np.arange(size)
        for draw in (0, 1, (1 << 40) + 5):
            assert sorted(replay.permute(x, size, 25450, draw).tolist()) == list(range(size)), (size, draw)


def test_sample_uniformity_fixed_seed():
    """Chi-square of where positions 0 and B-1 of 4 096 consecutive minibatches land among 257 ring rows:
    each at most df + 5 sqrt(2 df), df = 256 (mean df, standard deviation sqrt(2 df) under the uniform law)."""
    size, batch, draws, df = 257, 64, 4096, 256
    idx = filled(size).sample(batch, draws)["index"]
    bound = df + 5.0 * np.sqrt(2.0 * df)
    for pos in (0, batch - 1):
        counts = np.bincount(idx[:, pos], minlength=size)
        chi2 = float(((counts - draws / size) ** 2).sum() / (draws / size))
        print(f"position {pos}: chi-square {chi2:.1f} (bound {bound:.1f})")
        assert chi2 <= bound, (pos, chi2)


def test_header_and_ctypes_agree_on_replay_args():
    text = open(os.path.join(ROOT, "include", "sit.h")).read()
    for struct, cls in (("sit_replay_push_args", _lib.ReplayPushArgs), ("sit_replay_sample_args", _lib.ReplaySampleArgs)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
        assert names == [n for n, _ in cls._fields_]
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.sit_replay_push_args_size() == ctypes.sizeof(_lib.ReplayPushArgs)
        assert lib.sit_replay_sample_args_size() == ctypes.sizeof(_lib.ReplaySampleArgs)
