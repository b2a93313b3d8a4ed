"""The cases the observation-normalisation tests share (tests/test_obsnorm_host.py, tests/test_gpu_obsnorm.py).
NumPy only: synthetic transition rows whose observation columns span the reference's box, reference memories
filled directly (ring and cursor, as the GPU tests fill theirs), the documented update as a plain-Python loop,
and the book-keeping sequences."""
import math

import numpy as np

from sac_maritime_ast_amd import _lib, replay_reference
from sac_maritime_ast_amd.obsnorm import REFERENCE_OBS_HIGH, REFERENCE_OBS_LOW, ObsNormReference, default_min_std

DIM, OBS = _lib.SIT_TRANSITION_DIM, _lib.SIT_OBS_DIM
AW, H = _lib.SIT_ACTOR_WEIGHTS, _lib.SIT_ACTOR_HIDDEN
SIZES = (1, 255, 256, 257, 65537)            # 65 537: the first size with a second group of chunk sums
NP_REAL = {32: np.float32, 64: np.float64}
# (capacity, max_new or None, the cursor's `pushed` before each update)
SEQUENCES = {"wrap_and_skip": (300, None, (200, 450, 1200)),
             "max_new": (400, 100, (250, 250, 250)),
             "nothing_new": (300, None, (120, 120))}


def bits(a):
    a = np.asarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def rows(m, seed, spread=1.0):
    """[m, 24] float64 holding float32 values: state and next_state uniform in the middle `spread` of the box
    (heading columns included), the other columns plain numbers, column 23 an env id."""
    rng = np.random.default_rng(seed)
    lo, hi = REFERENCE_OBS_LOW.astype(np.float64), REFERENCE_OBS_HIGH.astype(np.float64)
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * spread
    rec = rng.normal(size=(m, DIM))
    rec[:, 0:OBS] = mid + half * rng.uniform(-1, 1, size=(m, OBS))
    rec[:, OBS + 2:2 * OBS + 2] = mid + half * rng.uniform(-1, 1, size=(m, OBS))
    rec[:, DIM - 2] = rng.integers(0, 2, m)
    rec[:, DIM - 1] = rng.integers(0, 64, m)
    return rec.astype(np.float32).astype(np.float64)


def fill(mem, rec, pushed):
    """Make the reference memory `mem` hold logical records [pushed - capacity, pushed) of `rec`, row g mod capacity."""
    cap = mem.capacity
    for g in range(max(0, pushed - cap), pushed):
        mem.ring[g % cap] = rec[g]
    mem.cursor[0] = pushed
    return mem


def memory(rec, capacity, pushed, precision=64):
    return fill(replay_reference(capacity, NP_REAL[precision]), rec, pushed)


def run_sequence(name, precision=64, seed=5, on_step=None):
    """The reference through one of SEQUENCES; on_step(mem, max_new, i) runs before each update (the GPU test
    mirrors the memory there).  Returns (ObsNormReference, read() after each update)."""
    capacity, max_new, pushes = SEQUENCES[name]
    rec = rows(max(pushes), seed)
    mem = replay_reference(capacity, NP_REAL[precision])
    ref, reads = ObsNormReference(), []
    for i, pushed in enumerate(pushes):
        fill(mem, rec, pushed)
        if on_step is not None:
            on_step(mem, max_new, i)
        ref.update(mem, max_new)
        reads.append(ref.read())
    return ref, reads, rec


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


def plain_update(block, affine, ring, pushed, capacity, max_new):
    """One sit_obsnorm_update as include/sit.h states it, on Python lists and floats (float32 roundings through
    np.float32): returns the new (block, affine) lists."""
    block, affine = [float(v) for v in block], [float(v) for v in affine]
    seen = int(block[2])
    start = max(seen, pushed - capacity)
    m = min(pushed - start, max_new)
    if m <= 0:
        block[1] += 1.0
        return block, affine
    n = block[0]
    n2 = n + float(m)
    for c in range(OBS):
        x = [float(ring[(start + j) % capacity][c]) for j in range(m)]
        mean_b = slow_tree(x) / float(m)
        q = slow_tree([(v - mean_b) * (v - mean_b) for v in x])
        mean = block[8 + c]
        d = mean_b - mean
        block[8 + c] = mean + d * (float(m) / n2)
        block[24 + c] = (block[24 + c] + q) + (d * d) * ((n * float(m)) / n2)
        std = max(math.sqrt(block[24 + c] / n2), affine[32 + c])
        affine[16 + c] = float(np.float32(1.0 / std))
        affine[c] = float(np.float32(block[8 + c]))
    block[3] += float(start - seen)
    block[2] = float(start + m)
    block[0] = n2
    block[1] += 1.0
    return block, affine


def default_actor(seed=11):
    """The packed block of a default-initialised GaussianPolicy (float32 NumPy)."""
    import torch
    from sac_maritime_ast_amd.samplers import GaussianPolicy, pack_actor_weights
    torch.manual_seed(seed)
    return pack_actor_weights(GaussianPolicy()).numpy().copy()


def head(block, x, dtype):
    """(mu, log_sigma) [n, 2] of the packed actor block on rows x [n, 10], everything in `dtype`."""
    from sac_maritime_ast_amd.samplers import block_segments
    w1, b1, w2, b2, w3, b3 = (np.asarray(seg, dtype=dtype) for _, _, seg in block_segments(np.asarray(block), OBS, 2))
    h = np.maximum(np.asarray(x, dtype=dtype) @ w1.T + b1, 0)
    h = np.maximum(h @ w2.T + b2, 0)
    out = h @ w3.T + b3
    assert out.dtype == dtype
    return out


def own_statistics(obs):
    """The reference normaliser after one update over the observation rows `obs` [n, 10]."""
    rec = np.zeros((len(obs), DIM))
    rec[:, :OBS] = obs
    ref = ObsNormReference()
    ref.update(memory(rec, len(obs), len(obs)))
    return ref


def fold_factor(ref):
    """1 + max_i |shift_i| scale_i: how far the folded first layer's terms exceed the normalised ones."""
    return 1.0 + float(np.max(np.abs(ref.shift.astype(np.float64)) * ref.scale.astype(np.float64)))


__all__ = ["SIZES", "SEQUENCES", "bits", "rows", "fill", "memory", "run_sequence", "slow_tree", "plain_update",
           "default_actor", "head", "own_statistics", "fold_factor", "default_min_std"]
