"""Scores over episodes, reduced on the device: mean return, status record, the best episode and the
weights that produced it.

``test_beds/main_ast.py:432-444`` keeps ``best_reward`` and saves a checkpoint when an episode beats it;
lines 453-523 run ``num_scoring_episodes`` deterministic episodes every ``scoring_episode_every`` episodes
and report ``avg_reward`` and the seven-entry ``status_record``.  Here the episodes of N envs finish inside
fused launches (``EpisodeLog``), so both are reductions over the log's records:

* ``Scoreboard`` runs ``sit_score_update`` (include/sit.h) over an ``EpisodeLog`` on the current stream: no
  synchronisation, capturable in a HIP graph.  The result is one float64[64] block on the device;
  ``keep`` then copies weight blocks iff the update found a new best episode (``sit_score_keep``), decided
  on the device.  ``read()`` is the one call that synchronises.
* ``Scorer`` is the scoring round on an env of its own, serving a packed actor block deterministically.
* ``score_reference`` is the same reduction in NumPy, summation tree included: the executable
  specification, and the CPU path for dumped records.

Scoring the same records twice counts them twice: score a log with ``consume=True`` (which empties it),
or drain it between updates.

Block layout (``FIELDS``): 0 episodes, 1 return_sum, 2 step_sum, 3 min, 4 max, 5 dropped, 6 updates,
7 replaced, 8:16 class counts, 16 best_stamp, 17:32 zero, 32:64 the best episode's record.
"""
from __future__ import annotations

from ctypes import byref

import numpy as np

from . import _lib
from .episodes import DIM as RECORD_DIM, columns

DIM, CLASSES, KEEP_BLOCKS = _lib.SIT_SCORE_DIM, _lib.SIT_SCORE_CLASSES, _lib.SIT_SCORE_KEEP_BLOCKS
CHUNK = 256                       # slots per chunk and chunk sums per group of the summation tree
BEST = DIM - RECORD_DIM           # first word of the best episode's record
FIELDS = {"episodes": 0, "return_sum": 1, "step_sum": 2, "min": 3, "max": 4, "dropped": 5, "updates": 6,
          "replaced": 7, "classes": slice(8, 8 + CLASSES), "best_stamp": 16, "best": slice(BEST, DIM)}
assert BEST == 32 and 8 + CLASSES == 16

# The reference's seven status_record classes (main_ast.py:453-523 looks for substrings of the one-ship
# env's status text) over this env's status bits, as (name, any, none): a record counts for a class when
# its terminal status has one of the `any` bits (any = 0: no condition) and none of the `none` bits.
REFERENCE_CLASSES = (
    ("blackout", _lib.ST_TEST_BLACKOUT, 0),
    ("mechanical", _lib.ST_TEST_MECHANICAL, 0),
    ("navigation", _lib.ST_TEST_NAVIGATION, 0),
    ("collision", _lib.ST_COLLISION | _lib.ST_TEST_TERRAIN, 0),
    ("arrival", _lib.ST_TEST_ENDPOINT, 0),
    ("route_or_horizon", _lib.ST_OBS_IW_TERMINAL | _lib.ST_TEST_HORIZON | _lib.ST_OBS_HORIZON, 0),
    ("not_terminal", 0, _lib.ST_TEST_DONE),
)


def _check_classes(classes):
    classes = tuple((str(n), int(a) & 0xFFFFFFFF, int(x) & 0xFFFFFFFF) for n, a, x in classes)
    if len(classes) > CLASSES:
        raise ValueError(f"classes: at most {CLASSES} classes (got {len(classes)})")
    return classes


def new_block() -> np.ndarray:
    """A reset score block (sit_score_reset)."""
    b = np.zeros(DIM)
    b[FIELDS["min"]], b[FIELDS["max"]], b[FIELDS["best_stamp"]] = np.inf, -np.inf, np.nan
    b[FIELDS["best"]] = np.nan
    return b


def _halve(x: np.ndarray) -> np.ndarray:
    """x [g, 256] -> [g]: x[i] += x[i + s] for s = 128, 64, ..., 1."""
    x = x.copy()
    s = CHUNK // 2
    while s:
        x[:, :s] = x[:, :s] + x[:, s:2 * s]
        s //= 2
    return x[:, 0]


def _padded(x: np.ndarray) -> np.ndarray:
    g = -(-x.size // CHUNK)
    out = np.zeros(g * CHUNK)
    out[:x.size] = x
    return out.reshape(g, CHUNK)


def tree_sum(x) -> float:
    """The round's return sum of include/sit.h: chunks of 256 (zero-padded) through the halving tree, the
    chunk sums in groups of 256 through the same tree, the group sums added in ascending order from +0.0."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    total = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for group in _halve(_padded(_halve(_padded(x)))) if x.size else ():
            total = total + float(group)
    return total


def score_reference(records, carry=None, *, classes=REFERENCE_CLASSES, episode_limit: int = 0) -> np.ndarray:
    """One sit_score_update (without flags) over records [m, 32] in NumPy: the new float64[64] block.

    carry: the block of the preceding updates (None: a reset block); it is not modified."""
    classes = _check_classes(classes)
    if episode_limit < 0:
        raise ValueError("episode_limit: must be >= 0")
    rec = np.asarray(records, dtype=np.float64).reshape(-1, RECORD_DIM)
    b = new_block() if carry is None else np.array(carry, dtype=np.float64, copy=True).reshape(DIM)
    inc = np.ones(len(rec), dtype=bool) if episode_limit == 0 else rec[:, 1] < episode_limit
    ret = rec[:, 3]
    status = rec[inc, 4].astype(np.int64) & 0xFFFFFFFF
    b[0] += int(inc.sum())
    b[2] += int(rec[inc, 2].astype(np.int64).sum())
    b[6] += 1
    for c, (_, any_, none) in enumerate(classes):
        if any_ == 0 and none == 0:
            continue
        hit = ((status & any_) != 0 if any_ else np.ones(len(status), dtype=bool)) & ((status & none) == 0)
        b[8 + c] += int(hit.sum())
    with np.errstate(invalid="ignore", over="ignore"):
        b[1] = b[1] + tree_sum(np.where(inc, ret, 0.0))
    ok = inc & ~np.isnan(ret)
    b[7] = 0.0
    if ok.any():
        b[3] = min(b[3], float(ret[ok].min())) + 0.0
        b[4] = max(b[4], float(ret[ok].max())) + 0.0
        slot = int(np.flatnonzero(ok)[np.argmax(ret[ok])])      # the first of equal greatest returns
        if np.isnan(b[BEST + 3]) or ret[slot] > b[BEST + 3]:
            b[BEST:] = rec[slot]
            b[7] = 1.0
    else:
        b[3], b[4] = b[3] + 0.0, b[4] + 0.0
    return b


def read_block(block, classes=REFERENCE_CLASSES) -> dict:
    """A score block as named values: episodes, mean_return, min, max, mean_steps, status_record {class
    name: count}, dropped, updates, best (the best episode's record as named columns, None without one)
    and best_stamp (None when no ``keep`` stamped it)."""
    classes = _check_classes(classes)
    b = np.asarray(block, dtype=np.float64).reshape(DIM)
    n = int(b[0])
    best = None
    if not np.isnan(b[BEST + 3]):
        best = {k: (v[0].item() if v[0].ndim == 0 else v[0].copy()) for k, v in columns(b[BEST:]).items()}
    return {"episodes": n, "mean_return": b[1] / n if n else float("nan"),
            "min": float(b[3]), "max": float(b[4]), "mean_steps": b[2] / n if n else float("nan"),
            "status_record": {name: int(b[8 + c]) for c, (name, _, _) in enumerate(classes)},
            "dropped": int(b[5]), "updates": int(b[6]), "best": best,
            "best_stamp": None if np.isnan(b[16]) else int(b[16])}


class Scoreboard:
    """The score block of one ``VecMultiShipRLEnv``'s handle, resident on its device.

    ``block`` (float64[64]) is a plain device tensor: a checkpoint is that tensor.  ``update`` and ``keep``
    launch on the current stream without synchronising; after a sufficient ``reserve`` (``update`` grows
    the scratch by itself outside a capture) both can be captured in a HIP graph."""

    def __init__(self, env, classes=REFERENCE_CLASSES):
        import torch
        self.env, self.classes = env, _check_classes(classes)
        self.block = torch.zeros(DIM, dtype=torch.float64, device=env.device)
        self.reset()

    def _device(self):
        import torch
        return torch.cuda.device(self.env.device)

    def reset(self):
        """An empty block: no episodes, min +inf, max -inf, no best episode."""
        with self._device():
            self.env._call("sit_score_reset", self.block.data_ptr(), self.env._stream())

    def reserve(self, n: int):
        """Allocate the update's scratch for record buffers of up to `n` records."""
        with self._device():
            self.env._call("sit_score_reserve", int(n))

    def update(self, log=None, *, records=None, count=None, episode_limit: int = 0, consume: bool = False,
               fresh: bool = False):
        """Score the records of an ``EpisodeLog`` (or explicit ``records`` [capacity, 32] float64 and
        ``count`` int64[1] device tensors).  episode_limit E > 0: only episodes 0..E-1 of every env;
        consume: count the records the log had no room for and empty the log; fresh: reset the block
        first."""
        import torch
        if log is not None:
            records = log.records if records is None else records
            count = log.count if count is None else count
        if records is None or count is None:
            raise ValueError("Scoreboard.update needs an EpisodeLog, or records and count")
        dev = self.block.device
        if not isinstance(records, torch.Tensor) or records.device != dev:
            raise ValueError(f"records: a tensor on {dev} is required")
        if records.dtype != torch.float64:
            raise ValueError(f"records: dtype torch.float64 required (got {records.dtype})")
        if records.dim() != 2 or records.shape[1] != RECORD_DIM or records.shape[0] == 0:
            raise ValueError(f"records: shape [capacity > 0, {RECORD_DIM}] required (got {tuple(records.shape)})")
        if not records.is_contiguous():
            raise ValueError("records: must be contiguous")
        if not isinstance(count, torch.Tensor) or count.device != dev or count.dtype != torch.int64 or count.numel() != 1:
            raise ValueError(f"count: an int64[1] tensor on {dev} is required")
        if int(episode_limit) < 0:
            raise ValueError("episode_limit: must be >= 0")
        a = _lib.ScoreArgs()
        a.record_capacity, a.episode_limit = int(records.shape[0]), int(episode_limit)
        a.flags = (_lib.SIT_SCORE_CONSUME if consume else 0) | (_lib.SIT_SCORE_FRESH if fresh else 0)
        a.records, a.record_count, a.score = records.data_ptr(), count.data_ptr(), self.block.data_ptr()
        for c, (_, any_, none) in enumerate(self.classes):
            a.class_any[c], a.class_none[c] = any_, none
        with self._device():
            self.env._call("sit_score_update", byref(a), self.env._stream())

    def keep(self, blocks, stamp=None):
        """Copy src to dst for every (src, dst) of `blocks` (float32 device tensors of equal size, at most
        four pairs) iff the last ``update`` found a new best episode, decided on the device; `stamp` (an
        int64 device tensor, e.g. ``learner.clock``, whose word 0 is the update number) is then recorded
        as ``best_stamp``."""
        import torch
        dev = self.block.device
        blocks = list(blocks)
        if len(blocks) > KEEP_BLOCKS:
            raise ValueError(f"blocks: at most {KEEP_BLOCKS} (src, dst) pairs (got {len(blocks)})")
        a = _lib.ScoreKeepArgs()
        a.n_blocks = len(blocks)
        for i, (src, dst) in enumerate(blocks):
            for name, t in (("src", src), ("dst", dst)):
                if not isinstance(t, torch.Tensor) or t.device != dev:
                    raise ValueError(f"blocks[{i}] {name}: a tensor on {dev} is required")
                if t.dtype != torch.float32:
                    raise ValueError(f"blocks[{i}] {name}: dtype torch.float32 required (got {t.dtype})")
                if not t.is_contiguous() or t.numel() == 0:
                    raise ValueError(f"blocks[{i}] {name}: a contiguous tensor with at least one element is required")
                if t.data_ptr() % 16:
                    raise ValueError(f"blocks[{i}] {name}: must be 16-byte aligned")
            if src.numel() != dst.numel():
                raise ValueError(f"blocks[{i}] dst: {src.numel()} elements required (got {dst.numel()})")
            a.src[i], a.dst[i], a.floats[i] = src.data_ptr(), dst.data_ptr(), src.numel()
        if stamp is not None:
            if (not isinstance(stamp, torch.Tensor) or stamp.device != dev or stamp.dtype != torch.int64
                    or stamp.numel() < 1 or not stamp.is_contiguous()):
                raise ValueError(f"stamp: a contiguous int64 tensor on {dev} is required")
            a.stamp = stamp.data_ptr()
        a.score = self.block.data_ptr()
        with self._device():
            self.env._call("sit_score_keep", byref(a), self.env._stream())

    def read(self) -> dict:
        """Synchronise and return the block as named values (``read_block``)."""
        import torch
        torch.cuda.synchronize(self.env.device)
        return read_block(self.block.cpu().numpy(), self.classes)

    def state_dict(self) -> dict:
        return {"block": self.block.clone(), "classes": [list(c) for c in self.classes]}

    def load_state_dict(self, sd: dict):
        block = sd["block"]
        if tuple(block.shape) != (DIM,) or block.dtype != self.block.dtype:
            raise ValueError("score block shape/dtype mismatch")
        if "classes" in sd and _check_classes(sd["classes"]) != self.classes:
            raise ValueError("score classes mismatch")
        self.block.copy_(block)


class Scorer:
    """The scoring round of main_ast.py:453-523 on an env of its own: `episodes_per_env` deterministic
    episodes (mode 2) of every env, scored on the device.

    ``run(weights, max_launches)`` restarts the env, serves `weights` (a packed actor block, e.g. a block
    kept by ``Scoreboard.keep``, or a policy module) deterministically in launches of `chunk` steps and
    scores each launch's finished episodes with ``episode_limit=episodes_per_env``; it reads the block
    every `check_every` launches and stops once every env has finished its episodes, or after
    `max_launches`.  Returns ``Scoreboard.read()`` plus ``complete`` and ``launches``."""

    def __init__(self, env, *, episodes_per_env: int = 1, chunk: int = 40, capacity: int | None = None,
                 seed: int = 25450, classes=REFERENCE_CLASSES):
        if episodes_per_env <= 0:
            raise ValueError("episodes_per_env: must be positive")
        if chunk <= 0:
            raise ValueError("chunk: must be positive")
        self.env, self.episodes_per_env, self.chunk, self.seed = env, int(episodes_per_env), int(chunk), int(seed)
        self.capacity = 4 * env.n_env if capacity is None else int(capacity)
        if self.capacity <= 0:
            raise ValueError("capacity: must be positive")
        self.board = Scoreboard(env, classes)
        self.board.reserve(self.capacity)
        self._policy = None

    def _sampler(self, weights):
        import torch
        from .samplers import GaussianPolicy, PolicySampler
        kw = dict(chunk=self.chunk, seed=self.seed, deterministic=True, episode_capacity=self.capacity)
        if isinstance(weights, torch.Tensor):
            if self._policy is None:      # the architecture the block belongs to; its own values are not served
                self._policy = GaussianPolicy().to(self.env.device)
            sampler = PolicySampler(self.env, self._policy, **kw)
            sampler.share_weights(weights)
            return sampler
        return PolicySampler(self.env, weights, **kw)

    def run(self, weights, max_launches: int, check_every: int = 8) -> dict:
        if max_launches <= 0:
            raise ValueError("max_launches: must be positive")
        if check_every <= 0:
            raise ValueError("check_every: must be positive")
        env = self.env
        env.restart()
        env.reset()
        env.init_step()
        sampler = self._sampler(weights)          # (a new EpisodeLog: the handle's accumulator is reset)
        self.board.reset()
        want = self.episodes_per_env * env.n_env
        out, launches = None, 0
        while launches < max_launches:
            sampler.launch()
            self.board.update(sampler.episodes, episode_limit=self.episodes_per_env, consume=True)
            launches += 1
            if launches % check_every == 0 or launches == max_launches:
                out = self.board.read()
                if out["episodes"] == want:
                    break
        out["complete"] = out["episodes"] == want
        out["launches"] = launches
        return out
