"""Observation normalisation on the device: running statistics, the affine, the folded actor block.

The networks of ``test_beds/main_ast.py`` see the env's observation, positions up to 1e4 m beside headings
of +-pi (the box of ``RLEnv/MSRL_Env.py:69-78``: ``REFERENCE_OBS_LOW`` / ``REFERENCE_OBS_HIGH``).  Here
x^_i = (x_i - shift_i) * scale_i per column, with the affine either fixed from bounds
(``ObsNormalizer.from_bounds``) or derived on the device from the running mean and variance of the
observations entering a ``ReplayMemory`` (``update``).  It is applied at two places, so that no step kernel
and no learner kernel knows of it:

* where minibatches are drawn: ``ReplayMemory.sample(..., normalizer=norm)`` hands out normalised ``state``
  and ``next_state`` (``sit_replay_sample_normalised``); the ring keeps raw observations, normalised at sample
  time with the affine current then;
* where the actor is served: ``fold`` writes a serving block from the master actor block, W1' = W1 diag(scale),
  b1' = b1 - W1' shift, so that ``PolicySampler.share_weights(serving_block)`` serves pi(normalise(obs)).

x^ is never clipped (a clip cannot be folded into W1, and the served actor must be the trained one): outliers
are bounded by a per-column floor on the standard deviation, ``min_std``.

State (include/sit.h "observation normalisation"), two plain device tensors; a checkpoint is those two:
``block`` float64[64]: 0 n, 1 updates, 2 seen, 3 skipped, 8:18 mean, 24:34 M2; ``affine`` float32[48]: 0:10
shift, 16:26 scale, 32:42 min_std.

``ObsNormReference`` is the same thing in NumPy, summation tree included (``score.tree_sum``): the executable
specification, which the device path equals bit for bit.

Not included: the PyTorch-actor queue path (``PolicySampler(fused_actor=False)``), where users normalise in
their own module, and merging statistics across ranks.
"""
from __future__ import annotations

from ctypes import byref, c_void_p

import numpy as np

from . import _lib
from .score import tree_sum

DIM, AFFINE, OBS = _lib.SIT_OBSNORM_DIM, _lib.SIT_OBSNORM_AFFINE, _lib.SIT_OBS_DIM
ACTOR_WEIGHTS, HIDDEN = _lib.SIT_ACTOR_WEIGHTS, _lib.SIT_ACTOR_HIDDEN
FIELDS = {"n": 0, "updates": 1, "seen": 2, "skipped": 3, "mean": slice(8, 8 + OBS), "m2": slice(24, 24 + OBS)}
SHIFT, SCALE, MIN_STD = slice(0, OBS), slice(16, 16 + OBS), slice(32, 32 + OBS)
# the observation box of the reference's env (RLEnv/MSRL_Env.py:69-78)
REFERENCE_OBS_LOW = np.array([0, 0, -np.pi, -3000, 0, 0, 0, 0, -np.pi, 0], dtype=np.float32)
REFERENCE_OBS_HIGH = np.array([10000, 20000, np.pi, 3000, 1000, 2000, 10000, 20000, np.pi, 1000], dtype=np.float32)


def default_min_std() -> np.ndarray:
    """1e-3 of the half-width of the reference's observation box, float32[10]."""
    return (1e-3 * (REFERENCE_OBS_HIGH.astype(np.float64) - REFERENCE_OBS_LOW.astype(np.float64)) / 2.0).astype(np.float32)


def _min_std(min_std) -> np.ndarray:
    if min_std is None:
        return default_min_std()
    ms = np.broadcast_to(np.asarray(min_std, dtype=np.float32), (OBS,)).copy()
    if not (np.isfinite(ms).all() and (ms >= 0).all()):
        raise ValueError("min_std: ten finite values >= 0 are required")
    return ms


def _bounds_affine(low, high):
    low, high = (np.broadcast_to(np.asarray(v, dtype=np.float64), (OBS,)) for v in (low, high))
    if not (np.isfinite(low).all() and np.isfinite(high).all() and (high > low).all()):
        raise ValueError("low, high: ten finite bounds with high > low are required")
    return ((low + high) / 2.0).astype(np.float32), (2.0 / (high - low)).astype(np.float32)


def new_affine(min_std=None) -> np.ndarray:
    """A reset affine (sit_obsnorm_reset): shift 0, scale 1, the given min_std."""
    a = np.zeros(AFFINE, dtype=np.float32)
    a[SCALE] = 1.0
    a[MIN_STD] = _min_std(min_std)
    return a


def read_state(block, affine) -> dict:
    """(block, affine) as named values: n, updates, seen, skipped, mean, std (the unfloored sqrt(M2 / n); NaN
    before the first record), shift, scale."""
    b = np.asarray(block, dtype=np.float64).reshape(DIM)
    a = np.asarray(affine, dtype=np.float32).reshape(AFFINE)
    n = b[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        std = np.sqrt(b[FIELDS["m2"]] / n) if n else np.full(OBS, np.nan)
    return {"n": int(n), "updates": int(b[1]), "seen": int(b[2]), "skipped": int(b[3]), "mean": b[FIELDS["mean"]].copy(),
            "std": std, "shift": a[SHIFT].copy(), "scale": a[SCALE].copy()}


class ObsNormReference:
    """``ObsNormalizer`` in NumPy: ``block`` float64[64], ``affine`` float32[48], and update / apply / fold as
    include/sit.h states them."""

    def __init__(self, min_std=None):
        self.block = np.zeros(DIM)
        self.affine = new_affine(min_std)
        self.frozen = False

    @classmethod
    def from_bounds(cls, low=REFERENCE_OBS_LOW, high=REFERENCE_OBS_HIGH) -> "ObsNormReference":
        """The frozen affine that maps [low, high] to [-1, 1]: shift = (low + high) / 2, scale = 2 / (high - low)."""
        self = cls()
        self.affine[SHIFT], self.affine[SCALE] = _bounds_affine(low, high)
        self.frozen = True
        return self

    @property
    def shift(self):
        return self.affine[SHIFT]

    @property
    def scale(self):
        return self.affine[SCALE]

    def update(self, memory, max_new: int | None = None):
        """Account the records of `memory` (a ``ReplayReference``) that are new since the last update."""
        if self.frozen:
            raise ValueError("update: this normaliser's affine is fixed (from_bounds)")
        cap = int(memory.capacity)
        max_new = cap if max_new is None else int(max_new)
        if max_new <= 0:
            raise ValueError("max_new: must be positive")
        b = self.block
        pushed, seen = int(memory.cursor[0]), int(b[2])
        start = max(seen, pushed - cap, 0)
        m = max(min(pushed - start, max_new), 0)
        if m == 0:
            b[1] += 1.0
            return
        rows = (start + np.arange(m, dtype=np.int64)) % cap
        x = np.asarray(memory.ring)[rows, :OBS].astype(np.float64)
        md = np.float64(m)
        n = np.float64(b[0])
        n2 = n + md
        with np.errstate(all="ignore"):
            r, w = md / n2, (n * md) / n2
            for c in range(OBS):
                mean_b = np.float64(tree_sum(x[:, c])) / md
                d = x[:, c] - mean_b
                q = np.float64(tree_sum(d * d))
                mean = np.float64(b[8 + c])
                d = mean_b - mean
                mean2 = mean + d * r
                m2 = (np.float64(b[24 + c]) + q) + (d * d) * w
                b[8 + c], b[24 + c] = mean2, m2
                s, least = np.sqrt(m2 / n2), np.float64(self.affine[32 + c])
                sd = s if s > least else least
                self.affine[16 + c] = np.float32(np.float64(1.0) / sd)
                self.affine[c] = np.float32(mean2)
        b[3] += float(start - seen)
        b[2] = float(start + m)
        b[0] = n2
        b[1] += 1.0

    def apply(self, x, y=None):
        """x^ = (x - shift) * scale in x's own float type, in place over [..., 10] arrays (two roundings)."""
        for v in (x,) if y is None else (x, y):
            if not isinstance(v, np.ndarray) or v.dtype not in (np.float32, np.float64) or v.shape[-1] != OBS:
                raise ValueError("apply: float32 or float64 arrays [..., 10] are required")
            with np.errstate(all="ignore"):
                np.subtract(v, self.affine[SHIFT].astype(v.dtype), out=v)
                np.multiply(v, self.affine[SCALE].astype(v.dtype), out=v)
        return x if y is None else (x, y)

    def normalized(self, x, dtype=None) -> np.ndarray:
        """A normalised copy of x [..., 10] in `dtype` (default x's own): float64 uses the float32 affine's values."""
        v = np.array(x, dtype=np.asarray(x).dtype if dtype is None else dtype, copy=True)
        return self.apply(v)

    def fold(self, src) -> np.ndarray:
        """The serving block of the packed actor block `src` (sit_obsnorm_fold)."""
        src = np.asarray(src, dtype=np.float32).reshape(-1)
        if src.size != ACTOR_WEIGHTS:
            raise ValueError(f"fold: a packed actor block of {ACTOR_WEIGHTS} floats is required")
        out = src.copy()
        shift, scale = self.affine[SHIFT], self.affine[SCALE]
        with np.errstate(all="ignore"):
            w1 = src[:HIDDEN * OBS].reshape(HIDDEN, OBS) * scale[None, :]          # float32 products
            acc = np.zeros(HIDDEN)
            for i in range(OBS):
                acc = acc + w1[:, i].astype(np.float64) * np.float64(shift[i])
            out[:HIDDEN * OBS] = w1.reshape(-1)
            out[HIDDEN * OBS:HIDDEN * OBS + HIDDEN] = (src[HIDDEN * OBS:HIDDEN * OBS + HIDDEN].astype(np.float64) - acc
                                                       ).astype(np.float32)
        return out

    def read(self) -> dict:
        return read_state(self.block, self.affine)

    def state_dict(self) -> dict:
        return {"block": self.block.copy(), "affine": self.affine.copy(), "frozen": self.frozen}

    def load_state_dict(self, sd: dict):
        self.block[:] = np.asarray(sd["block"], dtype=np.float64).reshape(DIM)
        self.affine[:] = np.asarray(sd["affine"], dtype=np.float32).reshape(AFFINE)
        self.frozen = bool(sd.get("frozen", False))


class ObsNormalizer:
    """The normaliser of one ``VecMultiShipRLEnv``'s handle, resident on its device.

    ``block`` (float64[64]) and ``affine`` (float32[48]) are plain device tensors.  Every call launches on the
    current stream without synchronising; after a sufficient ``reserve`` nothing is allocated, so all of them
    can be captured in a HIP graph.  ``read()`` is the one call that synchronises.  Order rule: update the
    normaliser after the push and before ``SacLearner.update_many``, so that the call's minibatches and the
    fold at its end use one affine."""

    def __init__(self, env, min_std=None):
        import torch
        self.env, self.frozen = env, False
        self._min_std = _min_std(min_std)
        self.block = torch.zeros(DIM, dtype=torch.float64, device=env.device)
        self.affine = torch.zeros(AFFINE, dtype=torch.float32, device=env.device)
        self._reserved = 0
        self.reset()

    @classmethod
    def from_bounds(cls, env, low=REFERENCE_OBS_LOW, high=REFERENCE_OBS_HIGH) -> "ObsNormalizer":
        """The frozen affine that maps [low, high] to [-1, 1]; ``update`` raises ValueError."""
        import torch
        shift, scale = _bounds_affine(low, high)
        self = cls(env)
        a = new_affine(self._min_std)
        a[SHIFT], a[SCALE] = shift, scale
        self.affine.copy_(torch.from_numpy(a))
        self.frozen = True
        return self

    def _device(self):
        import torch
        return torch.cuda.device(self.env.device)

    def reset(self):
        """No records accounted; shift 0, scale 1."""
        if self.frozen:
            raise ValueError("reset: this normaliser's affine is fixed (from_bounds)")
        with self._device():
            self.env._call("sit_obsnorm_reset", self.block.data_ptr(), self.affine.data_ptr(),
                           self._min_std.ctypes.data_as(c_void_p), self.env._stream())

    def reserve(self, max_new: int):
        """Allocate the update's scratch for up to `max_new` new records per update."""
        if int(max_new) <= 0:
            raise ValueError("max_new: must be positive")
        with self._device():
            self.env._call("sit_obsnorm_reserve", int(max_new))
        self._reserved = max(self._reserved, int(max_new))

    def update(self, memory, max_new: int | None = None):
        """Account the records of `memory` (a ``ReplayMemory`` of the same env) pushed since the last update,
        at most `max_new` of them (default the memory's capacity; the rest is picked up next time), and derive
        the affine.  Grows the scratch by itself outside a graph capture."""
        import torch
        if self.frozen:
            raise ValueError("update: this normaliser's affine is fixed (from_bounds)")
        ring, cursor = getattr(memory, "ring", None), getattr(memory, "cursor", None)
        dev = self.block.device
        if not isinstance(ring, torch.Tensor) or ring.device != dev or ring.dtype != self.env.dtype:
            raise ValueError(f"memory: a ReplayMemory of {self.env.dtype} on {dev} is required")
        if ring.dim() != 2 or ring.shape[1] != _lib.SIT_TRANSITION_DIM or not ring.is_contiguous() or ring.shape[0] == 0:
            raise ValueError(f"memory: ring shape [capacity > 0, {_lib.SIT_TRANSITION_DIM}] required (got {tuple(ring.shape)})")
        if not isinstance(cursor, torch.Tensor) or cursor.device != dev or cursor.dtype != torch.int64 or cursor.numel() != 4:
            raise ValueError(f"memory: cursor must be an int64[4] tensor on {dev}")
        max_new = int(ring.shape[0]) if max_new is None else int(max_new)
        if max_new <= 0:
            raise ValueError("max_new: must be positive")
        if max_new > self._reserved:
            if torch.cuda.is_current_stream_capturing():
                raise ValueError(f"max_new: reserve({max_new}) before capturing an update")
            self.reserve(max_new)
        a = _lib.ObsnormArgs()
        a.capacity, a.max_new = int(ring.shape[0]), max_new
        a.ring, a.cursor = ring.data_ptr(), cursor.data_ptr()
        a.block, a.affine = self.block.data_ptr(), self.affine.data_ptr()
        with self._device():
            self.env._call("sit_obsnorm_update", byref(a), self.env._stream())

    def _rows(self, name, t):
        import torch
        if not isinstance(t, torch.Tensor) or t.device != self.block.device:
            raise ValueError(f"{name}: a tensor on {self.block.device} is required")
        if t.dtype != self.env.dtype:
            raise ValueError(f"{name}: dtype {self.env.dtype} required for this handle (got {t.dtype})")
        if t.dim() < 1 or t.shape[-1] != OBS or t.numel() == 0 or not t.is_contiguous():
            raise ValueError(f"{name}: a contiguous tensor [..., {OBS}] with at least one row is required (got {tuple(t.shape)})")
        if t.data_ptr() % (2 * t.element_size()):
            raise ValueError(f"{name}: must be aligned to 2 elements")
        return t.data_ptr()

    def normalize(self, x, y=None):
        """x^ = (x - shift) * scale in place over `x` [..., 10] and, when given, `y` of the same size."""
        px = self._rows("x", x)
        py = None
        if y is not None:
            py = self._rows("y", y)
            if y.numel() != x.numel():
                raise ValueError(f"y: {x.numel()} elements required (got {y.numel()})")
        with self._device():
            self.env._call("sit_obsnorm_apply", self.affine.data_ptr(), px, py, x.numel() // OBS, self.env._stream())
        return x if y is None else (x, y)

    def fold(self, src_block, out):
        """The serving block `out` of the packed actor block `src_block` (float32[SIT_ACTOR_WEIGHTS] each)."""
        import torch
        for name, t in (("src_block", src_block), ("out", out)):
            if not isinstance(t, torch.Tensor) or t.device != self.block.device:
                raise ValueError(f"{name}: a tensor on {self.block.device} is required")
            if t.dtype != torch.float32 or t.numel() != ACTOR_WEIGHTS or not t.is_contiguous():
                raise ValueError(f"{name}: a contiguous float32 tensor of {ACTOR_WEIGHTS} elements is required "
                                 f"(got {tuple(t.shape)} {t.dtype})")
            if t.data_ptr() % 16:
                raise ValueError(f"{name}: must be 16-byte aligned")
        s, d, nbytes = src_block.data_ptr(), out.data_ptr(), 4 * ACTOR_WEIGHTS
        if s < d + nbytes and d < s + nbytes:
            raise ValueError("out: must not overlap src_block")
        with self._device():
            self.env._call("sit_obsnorm_fold", self.affine.data_ptr(), s, d, self.env._stream())
        return out

    def read(self) -> dict:
        """Synchronise and return n, updates, seen, skipped, mean, std, shift, scale (``read_state``)."""
        import torch
        torch.cuda.synchronize(self.env.device)
        return read_state(self.block.cpu().numpy(), self.affine.cpu().numpy())

    def state_dict(self) -> dict:
        return {"block": self.block.clone(), "affine": self.affine.clone(), "frozen": self.frozen}

    def load_state_dict(self, sd: dict):
        block, affine = sd["block"], sd["affine"]
        if tuple(block.shape) != (DIM,) or block.dtype != self.block.dtype:
            raise ValueError("obsnorm block shape/dtype mismatch")
        if tuple(affine.shape) != (AFFINE,) or affine.dtype != self.affine.dtype:
            raise ValueError("obsnorm affine shape/dtype mismatch")
        self.block.copy_(block)
        self.affine.copy_(affine)
        self.frozen = bool(sd.get("frozen", False))


__all__ = ["ObsNormalizer", "ObsNormReference", "REFERENCE_OBS_LOW", "REFERENCE_OBS_HIGH", "default_min_std", "new_affine",
           "read_state"]
