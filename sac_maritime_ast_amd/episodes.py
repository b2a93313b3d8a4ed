"""Episode records: what the reference's driver loop keeps per episode, reduced on the device.

``test_beds/main_ast.py:310-440`` accumulates ``episode_reward``, ``episode_steps``, the terminal
``status`` and ``action_record[i_episode]`` while it steps one env.  The HIP rollout steps N envs
for K rows per launch and hands back [K, n_env] rows, far too many to fetch at speed;
``EpisodeLog`` runs the library's episode reducer (``sit_episodes_update``, include/sit.h) over the
rows of each launch, on the same stream, and keeps one 32-column float64 record per finished
episode plus a histogram of the terminal status bits.  ``episodes_reference`` is the same
reduction as a plain NumPy loop: the executable specification, and the CPU path for small dumps.

Record columns (``COLUMNS``; include/sit.h "episode records"):
  0 env  1 episode  2 steps  3 ret  4 status  5 events  6 row  7 terminal_reward
  8:18 terminal_state (the done row's next_state)  18:32 angles (route angles of the first 14
  sampling events, NaN-padded)
"""
from __future__ import annotations

from ctypes import byref, c_size_t

import numpy as np

from . import _lib
from .status import status_string

DIM, ACTIONS, OBS = _lib.SIT_EPISODE_DIM, _lib.SIT_EPISODE_ACTIONS, _lib.SIT_OBS_DIM
COLUMNS = {"env": 0, "episode": 1, "steps": 2, "ret": 3, "status": 4, "events": 5, "row": 6,
           "terminal_reward": 7, "terminal_state": slice(8, 8 + OBS), "angles": slice(8 + OBS, DIM)}
_INT_COLUMNS = ("env", "episode", "steps", "status", "events", "row")
assert 8 + OBS + ACTIONS == DIM


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def columns(records) -> dict:
    """Named columns of a [m, 32] record array (integer columns as int64)."""
    rec = np.asarray(records, dtype=np.float64).reshape(-1, DIM)
    out = {k: rec[:, c].copy() for k, c in COLUMNS.items()}
    for k in _INT_COLUMNS:
        out[k] = out[k].astype(np.int64)
    return out


def new_carry(n_env: int) -> dict:
    """The running values of a fresh accumulator (sit_episodes_reset)."""
    return {"ret": np.zeros(n_env), "steps": np.zeros(n_env, np.int64), "events": np.zeros(n_env, np.int64),
            "episode": np.zeros(n_env, np.int64), "angle": np.full((n_env, ACTIONS), np.nan), "rows_seen": 0}


def episodes_reference(reward, done, status, action=None, next_state=None, carry=None, env_id_offset=0):
    """The episode reduction of include/sit.h over rows [K, n_env] (a single env's [K] rows are
    taken as n_env = 1), as a plain loop.

    reward [K, n] (float32 or float64), done [K, n], status [K, n] (bitmask, any integer type),
    action [K, n, 4] or None, next_state [K, n, 10] or None; carry: the running values returned by
    an earlier call over the preceding rows (None: a fresh accumulator).
    Returns (records [m, 32] float64 in ascending (env, episode) order, hist int64[32], carry)."""
    reward = _np(reward)
    if reward.ndim == 1:
        reward = reward[:, None]
    K, n = reward.shape
    done = _np(done).reshape(K, n) != 0
    status = _np(status).reshape(K, n).astype(np.int64) & 0xFFFFFFFF
    action = None if action is None else _np(action).reshape(K, n, 4)
    next_state = None if next_state is None else _np(next_state).reshape(K, n, OBS)
    c = new_carry(n) if carry is None else {k: (np.array(v, copy=True) if k != "rows_seen" else int(v))
                                            for k, v in carry.items()}
    row0 = int(c["rows_seen"])
    records = []
    hist = np.zeros(32, dtype=np.int64)
    stepped = (status & _lib.ST_NO_STEP) == 0
    for e in range(n):
        ret, steps, events = float(c["ret"][e]), int(c["steps"][e]), int(c["events"][e])
        episode, angle = int(c["episode"][e]), c["angle"][e]
        r64 = reward[:, e].astype(np.float64)
        for k in np.nonzero(stepped[:, e])[0]:
            ret = ret + float(r64[k])           # one IEEE add per row, in row order
            steps += 1
            if action is not None and action[k, e, 3] != 0:
                if events < ACTIONS:
                    angle[events] = float(action[k, e, 2])
                events += 1
            if done[k, e]:
                rec = np.full(DIM, np.nan)
                rec[:8] = (env_id_offset + e, episode, steps, ret, status[k, e], events, row0 + int(k), r64[k])
                if next_state is not None:
                    rec[8:8 + OBS] = next_state[k, e]
                rec[8 + OBS:] = angle
                records.append(rec)
                bits = int(status[k, e])
                for b in range(32):
                    hist[b] += (bits >> b) & 1
                episode += 1
                ret, steps, events = 0.0, 0, 0
                angle[:] = np.nan
        c["ret"][e], c["steps"][e], c["events"][e], c["episode"][e] = ret, steps, events, episode
    c["rows_seen"] = row0 + K
    rec = np.stack(records) if records else np.zeros((0, DIM))
    return rec, hist, c


class EpisodeLog:
    """Device-side episode records of one ``VecMultiShipRLEnv`` (one log per env: the running
    values live in the env's handle).

    ``update`` reduces the rows of one launch (one ``sit_episodes_update`` on the current stream, no
    synchronisation, capturable in a HIP graph); ``drain`` fetches the finished episodes.  Records
    past `capacity` between two drains are counted (``dropped``) and still enter the histogram."""

    def __init__(self, env, capacity: int, env_id_offset: int = 0):
        import torch
        if capacity < 0:
            raise ValueError("capacity must be >= 0")
        self.env, self.capacity, self.env_id_offset = env, int(capacity), int(env_id_offset)
        dev = env.device
        self.records = torch.zeros((self.capacity, DIM), dtype=torch.float64, device=dev)
        self.count = torch.zeros(1, dtype=torch.int64, device=dev)
        self.hist = torch.zeros(32, dtype=torch.int64, device=dev)
        nb = c_size_t()
        env._call("sit_episodes_bytes", byref(nb))
        self._bytes = nb.value
        self.reset()

    def reset(self):
        """Zero the running values of every env, the row counter, the record count and the histogram."""
        with self._device():
            self.env._call("sit_episodes_reset", self.env._stream())
        self.count.zero_()
        self.hist.zero_()

    def _device(self):
        import torch
        return torch.cuda.device(self.env.device)

    def _rows(self, name, t, dtype, tail=()):
        import torch
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or t.device != self.records.device:
            raise ValueError(f"{name}: a tensor on {self.records.device} is required")
        if t.dtype == torch.bool and dtype == torch.uint8:
            t = t.view(torch.uint8)
        if t.dtype != dtype:
            raise ValueError(f"{name}: dtype {dtype} required for this handle (got {t.dtype})")
        if t.dim() != 2 + len(tail) or t.shape[1] != self.env.n_env or tuple(t.shape[2:]) != tuple(tail):
            raise ValueError(f"{name}: shape [K, {self.env.n_env}{''.join(f', {d}' for d in tail)}] required "
                             f"(got {tuple(t.shape)})")
        if not t.is_contiguous():
            raise ValueError(f"{name}: must be contiguous")
        return t

    def update(self, out: dict | None = None, *, reward=None, done=None, status=None, action=None,
               next_state=None):
        """Reduce the rows of one launch: a rollout's `out` dict (its "action" / "next_state" are used
        when present) or explicit [K, n_env, ...] tensors."""
        import torch
        if out is not None:
            reward = out.get("reward") if reward is None else reward
            done = out.get("done") if done is None else done
            status = out.get("status") if status is None else status
            action = out.get("action") if action is None else action
            next_state = out.get("next_state") if next_state is None else next_state
        if reward is None or done is None or status is None:
            raise ValueError("EpisodeLog.update needs reward, done and status rows")
        dt = self.env.dtype
        reward = self._rows("reward", reward, dt)
        K = int(reward.shape[0])
        done = self._rows("done", done, torch.uint8)
        status = self._rows("status", status, torch.int32)
        action = self._rows("action", action, dt, (4,))
        next_state = self._rows("next_state", next_state, dt, (OBS,))
        for name, t in (("done", done), ("status", status), ("action", action), ("next_state", next_state)):
            if t is not None and t.shape[0] != K:
                raise ValueError(f"{name}: {K} rows required (got {t.shape[0]})")
        if K == 0:
            raise ValueError("EpisodeLog.update needs at least one row")
        a = _lib.EpisodesArgs()
        a.n_steps, a.record_capacity, a.env_id_offset = K, self.capacity, self.env_id_offset
        a.reward, a.done, a.status = reward.data_ptr(), done.data_ptr(), status.data_ptr()
        a.action_out = None if action is None else action.data_ptr()
        a.next_state = None if next_state is None else next_state.data_ptr()
        a.records = self.records.data_ptr() if self.capacity > 0 else None
        a.record_count, a.status_hist = self.count.data_ptr(), self.hist.data_ptr()
        with self._device():
            self.env._call("sit_episodes_update", byref(a), self.env._stream())

    def drain(self) -> dict:
        """Synchronise and return the finished episodes since the last drain as named NumPy columns
        (env, episode, steps, ret, status, events, row, terminal_reward, terminal_state [m, 10],
        angles [m, 14]; "records" is the raw [m, 32] array) and `dropped`, the episodes that found
        the buffer full; then empty the buffer."""
        import torch
        torch.cuda.synchronize(self.env.device)
        total = int(self.count.item())
        m = min(total, self.capacity)
        rec = self.records[:m].cpu().numpy()
        self.count.zero_()
        out = columns(rec)
        out["records"] = rec
        out["dropped"] = total - m
        return out

    def status_counts(self) -> dict:
        """{reference status string: finished episodes whose terminal status has it}, over every
        episode since the last reset (dropped ones included)."""
        hist = self.hist.cpu().numpy()
        out: dict = {}
        for b in range(32):
            if hist[b]:
                key = status_string(1 << b)
                out[key] = out.get(key, 0) + int(hist[b])
        return out

    def state(self):
        """The accumulator (running values of every env and the row counter) as a uint8 device tensor."""
        import torch
        blob = torch.empty(self._bytes, dtype=torch.uint8, device=self.env.device)
        with self._device():
            self.env._call("sit_episodes_get", blob.data_ptr(), self.env._stream())
        return blob

    def load_state(self, blob):
        import torch
        if blob.numel() != self._bytes or blob.dtype != torch.uint8:
            raise ValueError("episode accumulator blob size/dtype mismatch")
        blob = blob.to(self.env.device).contiguous()
        with self._device():
            self.env._call("sit_episodes_set", blob.data_ptr(), self.env._stream())
