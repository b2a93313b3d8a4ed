"""Replay memory on the device: an ordered ring push and seeded minibatches.

``test_beds/main_ast.py`` keeps ``memory = ReplayMemory(replay_size)``, pushes one
``(state, action, reward, next_state, mask)`` per sampling event (385-396) and draws minibatches for
``agent.update_parameters(memory, batch_size, updates)`` (350-362).  The step kernels write those
events as 24-real transition records (include/sit.h "replay transition record"), in the order their
waves reach the counter.  ``ReplayMemory`` holds them in a ring on the device and hands out
minibatches (``sit_replay_push`` / ``sit_replay_sample``, include/sit.h "replay memory"); ring
contents and minibatches depend on the records, the seed and the draw counter only.
``replay_reference`` is the same thing in plain NumPy: the executable specification, which the
device path equals bit for bit.

Push: the n = min(count, src_capacity) valid records are taken in canonical order (ascending env id,
column 23; within one env the order in which they stand in the source), record j of that order goes
to slot (pushed + j) mod capacity, and only the last `capacity` of them are written.
Sample: element b of the minibatch with draw number d is ring row P(b mod size), P a keyed bijection
of [0, size): a 4-round balanced Feistel network on 2h bits, h = ceil(max(bit_length(size - 1), 2) / 2),
round function the low h bits of word 0 of Philox4x32-10(key = seed, ctr = (R, 0x525000 | round,
d_lo, d_hi)), cycle-walked into [0, size).
"""
from __future__ import annotations

from ctypes import byref

import numpy as np

from . import _lib

DIM, OBS = _lib.SIT_TRANSITION_DIM, _lib.SIT_OBS_DIM
CURSOR = {"pushed": 0, "dropped": 1, "draws": 2}
FEISTEL_TAG = 0x5250
FEISTEL_ROUNDS = 4
SAMPLE_KEYS = ("state", "action", "reward", "next_state", "mask", "env", "index")
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al. SC'11) on arrays: ctr four words, key two words; four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & _M32 for x in ctr]
    k0, k1 = (np.asarray(k, dtype=np.uint64) & _M32 for k in key)
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _M32]
    return [x.astype(np.uint32) for x in c]


def half_bits(size: int) -> int:
    """h: the Feistel network permutes [0, 4**h), the smallest such range of at least 4 that holds size."""
    return (max(int(size - 1).bit_length(), 2) + 1) // 2


def permute(x, size: int, seed: int, draw):
    """P_{seed,draw}(x) for x in [0, size) (arrays; draw broadcasts against x)."""
    x = np.array(x, dtype=np.uint64)
    draw = np.broadcast_to(np.asarray(draw, dtype=np.uint64), x.shape)
    h = np.uint64(half_bits(size))
    low = (np.uint64(1) << h) - np.uint64(1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = (seed & 0xFFFFFFFF, seed >> 32)
    todo = np.ones(x.shape, dtype=bool)
    while todo.any():
        v, d = x[todo], draw[todo]
        left, right = v >> h, v & low
        for r in range(FEISTEL_ROUNDS):
            f = philox4x32_10((right, np.uint64((FEISTEL_TAG << 8) | r), d & _M32, d >> np.uint64(32)), key)[0]
            left, right = right, left ^ (f.astype(np.uint64) & low)
        x[todo] = (left << h) | right
        todo = x >= np.uint64(size)
    return x.astype(np.int64)


def env_keys(ids) -> np.ndarray:
    """Sort key of column 23: the id as uint32; anything that is no id in [0, 2**32 - 2) sorts last."""
    ids = np.asarray(ids, dtype=np.float64)
    ok = (ids >= 0) & (ids < 4294967294.0)
    return np.where(ok, np.where(ok, ids, 0).astype(np.uint64), 0xFFFFFFFE).astype(np.uint32)


def env_ids(ids) -> np.ndarray:
    """Column 23 as int32 (-1 for what is no id below 2**31)."""
    ids = np.asarray(ids, dtype=np.float64)
    ok = (ids >= 0) & (ids < 2147483648.0)
    return np.where(ok, np.where(ok, ids, 0).astype(np.int64), -1).astype(np.int32)


class ReplayReference:
    """The ring, cursor, push and sample of include/sit.h ("replay memory") as plain NumPy."""

    def __init__(self, capacity: int, dtype=np.float32, seed: int = 25450):
        if capacity <= 0:
            raise ValueError("capacity must be positive")
        self.capacity, self.seed = int(capacity), int(seed)
        self.ring = np.zeros((self.capacity, DIM), dtype=dtype)
        self.cursor = np.zeros(4, dtype=np.int64)

    def __len__(self):
        return int(min(self.cursor[0], self.capacity))

    @property
    def dropped(self):
        return int(self.cursor[1])

    def push(self, src, count):
        src = np.asarray(src)
        if src.ndim != 2 or src.shape[1] != DIM or src.dtype != self.ring.dtype:
            raise ValueError(f"src: [*, {DIM}] of {self.ring.dtype} required")
        count = max(int(np.asarray(count).reshape(-1)[0]), 0)
        n = min(count, src.shape[0])
        order = np.argsort(env_keys(src[:n, DIM - 1]), kind="stable")
        pushed = int(self.cursor[0])
        for j in range(max(0, n - self.capacity), n):
            self.ring[(pushed + j) % self.capacity] = src[order[j]]
        self.cursor[0] += n
        self.cursor[1] += count - n

    def sample(self, batch: int, n_batches: int = 1, normalizer=None) -> dict:
        """normalizer: an ``ObsNormReference`` applied to state and next_state (sample, then apply)."""
        B, U = int(batch), int(n_batches)
        if B <= 0 or U <= 0:
            raise ValueError("batch and n_batches must be positive")
        size, draws = len(self), int(self.cursor[2])
        dt = self.ring.dtype
        if size == 0:
            out = {"state": np.zeros((U, B, OBS), dt), "action": np.zeros((U, B, 1), dt), "reward": np.zeros((U, B), dt),
                   "next_state": np.zeros((U, B, OBS), dt), "mask": np.zeros((U, B), dt),
                   "env": np.zeros((U, B), np.int32), "index": np.full((U, B), -1, np.int32)}
        else:
            x = np.broadcast_to(np.arange(B, dtype=np.uint64) % np.uint64(size), (U, B))
            d = (draws + np.arange(U, dtype=np.uint64))[:, None]
            idx = permute(x, size, self.seed, d)
            rec = self.ring[idx]
            out = {"state": rec[..., :OBS].copy(), "action": rec[..., OBS:OBS + 1].copy(), "reward": rec[..., OBS + 1].copy(),
                   "next_state": rec[..., OBS + 2:2 * OBS + 2].copy(), "mask": rec[..., DIM - 2].copy(),
                   "env": env_ids(rec[..., DIM - 1]), "index": idx.astype(np.int32)}
        self.cursor[2] += U
        if normalizer is not None:
            normalizer.apply(out["state"], out["next_state"])
        return out


def replay_reference(capacity: int, dtype=np.float32, seed: int = 25450) -> ReplayReference:
    """A NumPy replay memory with the device path's semantics (``ReplayReference``)."""
    return ReplayReference(capacity, dtype, seed)


class ReplayMemory:
    """Replay ring of one ``VecMultiShipRLEnv``'s handle, resident on its device.

    ``ring`` [capacity, 24] (the handle's real type) and ``cursor`` int64[4] = {pushed, dropped, draws, 0}
    are plain device tensors: a checkpoint is those two.  ``push`` and ``sample`` launch on the current
    stream without synchronising; after a sufficient ``reserve`` they allocate nothing in the library, so
    both can be captured in a HIP graph (give ``sample`` its ``out``)."""

    def __init__(self, env, capacity: int, seed: int = 25450):
        import torch
        if capacity <= 0:
            raise ValueError("capacity must be positive")
        self.env, self.capacity, self.seed = env, int(capacity), int(seed)
        self.ring = torch.zeros((self.capacity, DIM), dtype=env.dtype, device=env.device)
        self.cursor = torch.zeros(4, dtype=torch.int64, device=env.device)

    def _device(self):
        import torch
        return torch.cuda.device(self.env.device)

    def reserve(self, max_src_capacity: int):
        """Allocate the push's sort scratch for source buffers of up to `max_src_capacity` records."""
        with self._device():
            self.env._call("sit_replay_reserve", int(max_src_capacity), self.env._stream())

    def push(self, out: dict | None = None, *, transitions=None, count=None):
        """Push the valid records of one source buffer: a rollout's or sampler's `out` dict
        ("transitions", "transition_count") or explicit tensors ([src_capacity, 24], int32[1])."""
        import torch
        if out is not None:
            transitions = out.get("transitions") if transitions is None else transitions
            count = out.get("transition_count") if count is None else count
        if transitions is None or count is None:
            raise ValueError("ReplayMemory.push needs transitions and their count")
        dev = self.ring.device
        if not isinstance(transitions, torch.Tensor) or transitions.device != dev:
            raise ValueError(f"transitions: a tensor on {dev} is required")
        if transitions.dtype != self.env.dtype:
            raise ValueError(f"transitions: dtype {self.env.dtype} required for this handle (got {transitions.dtype})")
        if transitions.dim() != 2 or transitions.shape[1] != DIM:
            raise ValueError(f"transitions: shape [src_capacity, {DIM}] required (got {tuple(transitions.shape)})")
        if not transitions.is_contiguous():
            raise ValueError("transitions: must be contiguous")
        if not isinstance(count, torch.Tensor) or count.device != dev or count.dtype != torch.int32 or count.numel() != 1:
            raise ValueError(f"count: an int32[1] tensor on {dev} is required")
        if transitions.shape[0] == 0:       # a buffer without room holds no record
            return
        a = _lib.ReplayPushArgs()
        a.capacity, a.src_capacity = self.capacity, int(transitions.shape[0])
        a.ring, a.cursor = self.ring.data_ptr(), self.cursor.data_ptr()
        a.src, a.src_count = transitions.data_ptr(), count.data_ptr()
        with self._device():
            self.env._call("sit_replay_push", byref(a), self.env._stream())

    def sample(self, batch: int, n_batches: int = 1, out: dict | None = None, normalizer=None) -> dict:
        """`n_batches` minibatches of `batch` records: state [U, B, 10], action [U, B, 1], reward [U, B],
        next_state [U, B, 10], mask [U, B], env int32 [U, B], index int32 [U, B] (the ring row; -1 and
        zeros from an empty ring).  Tensors of `out` with the right shape and type are reused.
        normalizer: an ``ObsNormalizer`` of the same device; state and next_state then leave the gather
        normalised by its current affine (``sit_replay_sample_normalised``; the bits of sample + normalize)."""
        import torch
        B, U = int(batch), int(n_batches)
        dt, dev = self.env.dtype, self.ring.device
        affine = None
        if normalizer is not None:
            affine = getattr(normalizer, "affine", None)
            if (not isinstance(affine, torch.Tensor) or affine.device != dev or affine.dtype != torch.float32
                    or affine.numel() != _lib.SIT_OBSNORM_AFFINE or not affine.is_contiguous()):
                raise ValueError(f"normalizer: an ObsNormalizer on {dev} is required")
        shapes = {"state": ((U, B, OBS), dt), "action": ((U, B, 1), dt), "reward": ((U, B), dt),
                  "next_state": ((U, B, OBS), dt), "mask": ((U, B), dt), "env": ((U, B), torch.int32),
                  "index": ((U, B), torch.int32)}
        out = {} if out is None else out
        if B > 0 and U > 0:
            for k, (shp, d) in shapes.items():
                t = out.get(k)
                if t is None or tuple(t.shape) != shp or t.dtype != d or t.device != dev or not t.is_contiguous():
                    out[k] = torch.empty(shp, dtype=d, device=dev)
        a = _lib.ReplaySampleArgs()
        a.capacity, a.batch, a.n_batches, a.seed = self.capacity, B, U, self.seed & 0xFFFFFFFFFFFFFFFF
        a.ring, a.cursor = self.ring.data_ptr(), self.cursor.data_ptr()
        for k in SAMPLE_KEYS:
            t = out.get(k)
            setattr(a, k, None if t is None else t.data_ptr())
        with self._device():
            if affine is None:
                self.env._call("sit_replay_sample", byref(a), self.env._stream())
            else:
                self.env._call("sit_replay_sample_normalised", byref(a), affine.data_ptr(), self.env._stream())
        return out

    def _cursor(self):
        import torch
        torch.cuda.synchronize(self.env.device)
        return [int(v) for v in self.cursor.cpu()]

    def __len__(self):
        return min(self._cursor()[0], self.capacity)

    @property
    def dropped(self) -> int:
        """Records that found their source buffer full (counted by the kernels, never written)."""
        return self._cursor()[1]

    def state_dict(self) -> dict:
        return {"ring": self.ring.clone(), "cursor": self.cursor.clone(), "seed": self.seed}

    def load_state_dict(self, sd: dict):
        ring, cursor = sd["ring"], sd["cursor"]
        if tuple(ring.shape) != tuple(self.ring.shape) or ring.dtype != self.ring.dtype:
            raise ValueError("replay ring shape/dtype mismatch")
        if tuple(cursor.shape) != (4,) or cursor.dtype != self.cursor.dtype:
            raise ValueError("replay cursor shape/dtype mismatch")
        self.ring.copy_(ring)
        self.cursor.copy_(cursor)
        self.seed = int(sd["seed"])
