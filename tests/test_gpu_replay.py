"""GPU checks of the replay memory (sit_replay_push / sit_replay_sample behind ReplayMemory) against
replay_reference, the NumPy specification: rings, cursors and minibatches are compared as integer
views (push and sample only move bits), for float32 and float64 handles."""
import numpy as np
import pytest
import torch

from helpers import OBS_SCALE, rel_err
from oracle import sit_oracle as so

pytestmark = pytest.mark.gpu

sit = pytest.importorskip("sac_maritime_ast_amd")
from sac_maritime_ast_amd import ReplayMemory, VecMultiShipRLEnv, _lib, make_scenario, replay_reference  # noqa: E402

DEV = "cuda:0"
DIM = _lib.SIT_TRANSITION_DIM
TOL64 = 1e-9
SRC_CAP, RING_CAP, ID0, N_IDS = 700, 257, 1000, 300
ROLL_ENVS, ROLL_STEPS, ROLL_LAUNCHES, ROLL_TCAP, ROLL_RING = 1024, 100, 4, 8192, 4096
NP_REAL = {32: np.float32, 64: np.float64}
NP_BITS = {32: np.uint32, 64: np.uint64}


@pytest.fixture(scope="module", params=[32, 64])
def env(request):
    e = VecMultiShipRLEnv(scenario=make_scenario(64), precision=request.param, device=DEV)
    yield e
    e.close()


def bits(a):
    """An array or tensor as unsigned integers of its element width."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_memory(mem, ref):
    torch.cuda.synchronize()
    assert np.array_equal(mem.cursor.cpu().numpy(), ref.cursor), (mem.cursor.cpu().numpy(), ref.cursor)
    assert np.array_equal(bits(mem.ring), bits(ref.ring))


def same_batches(got, want):
    torch.cuda.synchronize()
    assert set(got) == set(want)
    for k in want:
        g = got[k].cpu().numpy()
        assert g.shape == want[k].shape and g.dtype == want[k].dtype, k
        assert np.array_equal(bits(g), bits(want[k])), k


def source(rng, precision, count, room=SRC_CAP, id0=ID0, n_ids=None):
    """A source buffer of `room` rows: min(count, room) valid records of few enough envs that several have
    2-5 records, random payload with NaN payloads and -0.0 planted; the rows behind them hold other
    records, which a push must not read."""
    n = min(count, room)
    n_ids = min(N_IDS, max(1, n // 2)) if n_ids is None else n_ids
    src = rng.standard_normal((room, DIM)).astype(NP_REAL[precision])
    src[:, DIM - 1] = id0 + rng.integers(0, n_ids, room)
    b = src.view(NP_BITS[precision])
    nan = {32: 0x7FC00000, 64: 0x7FF8000000000000}[precision]
    neg0 = {32: 0x80000000, 64: 0x8000000000000000}[precision]
    for i in range(0, room, 7):
        b[i, i % 22] = nan | (i + 1)          # quiet NaNs with distinct payloads
        b[i, (i + 5) % 22] = neg0
    return src


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def count_of(c):
    return torch.tensor([c], dtype=torch.int32, device=DEV)


def push_both(mem, ref, src, count):
    mem.push(transitions=dev(src), count=count_of(count))
    ref.push(src, count)


# ---------------------------------------------------------------------------------------------
# synthetic push
# ---------------------------------------------------------------------------------------------
def test_push_sequence_equals_reference(env):
    """Counts 0, 1, 63, 64, 65, 700 and 900 (200 dropped) of a 700-row source into 257 slots: the ring wraps
    across pushes, and the 700- and 900-record pushes each keep their last 257 records."""
    rng = np.random.default_rng(11)
    mem, ref = ReplayMemory(env, RING_CAP), replay_reference(RING_CAP, NP_REAL[env.precision])
    for count in (0, 1, 63, 64, 65, 700, 900):
        src = source(rng, env.precision, count)
        ids, per_env = np.unique(src[:min(count, SRC_CAP), DIM - 1], return_counts=True)
        if count >= 63:
            assert (per_env >= 2).sum() >= 3 and per_env.max() <= 12
        push_both(mem, ref, src, count)
        same_memory(mem, ref)
    assert ref.cursor.tolist() == [0 + 1 + 63 + 64 + 65 + 700 + 700, 200, 0, 0]
    assert len(mem) == RING_CAP and mem.dropped == 200


def test_push_ignores_arrival_order(env):
    """Permuting the valid source rows while every env keeps its records' relative order leaves ring and
    cursor unchanged."""
    rng = np.random.default_rng(12)
    n = 650
    src = source(rng, env.precision, n)
    ids = src[:n, DIM - 1]
    moved = src.copy()
    new_ids = ids[rng.permutation(n)]
    for e in np.unique(ids):
        moved[:n][new_ids == e] = src[:n][ids == e]      # env e's records, in their order, at its new rows
    assert not np.array_equal(bits(moved), bits(src))
    for cap in (RING_CAP, 1024):
        a, b = ReplayMemory(env, cap), ReplayMemory(env, cap)
        ref = replay_reference(cap, NP_REAL[env.precision])
        push_both(a, ref, src, n)
        b.push(transitions=dev(moved), count=count_of(n))
        same_memory(a, ref)
        same_memory(b, ref)


def test_push_in_rank_order_equals_one_push(env):
    """Two buffers with disjoint ascending id ranges pushed one after the other equal their concatenation."""
    rng = np.random.default_rng(13)
    lo = source(rng, env.precision, 300, room=400, id0=ID0, n_ids=150)
    hi = source(rng, env.precision, 350, room=400, id0=ID0 + 150, n_ids=150)
    both = np.concatenate([lo[:300], hi[:350]])
    for cap in (RING_CAP, 1024):
        two, one = ReplayMemory(env, cap), ReplayMemory(env, cap)
        ref = replay_reference(cap, NP_REAL[env.precision])
        for part, n in ((lo, 300), (hi, 350)):
            two.push(transitions=dev(part), count=count_of(n))
        one.push(transitions=dev(both), count=count_of(650))
        ref.push(both, 650)
        same_memory(one, ref)
        same_memory(two, ref)       # at 257 slots too: record j of the second push is record 300 + j of the one push


# ---------------------------------------------------------------------------------------------
# real rollout
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_launches():
    """The oracle's transitions of four launches of 1 024 envs (computed once for both precisions)."""
    sc = make_scenario(ROLL_ENVS, cap=32)
    o = so.OracleEnvs(dict(so.DEFAULT_PARAMS), sc.routes, sc.n_wpt, sc.init, sc.polys)
    o.reset()
    o.init_step()
    launches = [o.rollout(ROLL_STEPS, seed=99, mask_horizon=600)["transitions"].copy() for _ in range(ROLL_LAUNCHES)]
    # within-env order is only tested if some env has two records in one launch
    most = max(np.unique(t[:, DIM - 1], return_counts=True)[1].max() for t in launches if len(t))
    assert most >= 2
    assert sum(len(t) > 0 for t in launches) >= 2
    return sc, launches


def run_rollouts(sc, precision, check=None):
    env = VecMultiShipRLEnv(scenario=sc, precision=precision, device=DEV)
    env.reset()
    env.init_step()
    mem = ReplayMemory(env, ROLL_RING)
    mem.reserve(ROLL_TCAP)
    out = {}
    for launch in range(ROLL_LAUNCHES):
        env.rollout(ROLL_STEPS, seed=99, transition_capacity=ROLL_TCAP, mask_horizon=600, out=out)
        mem.push(out)
        if check is not None:
            check(launch, mem, out)
    torch.cuda.synchronize()
    ring, cursor = mem.ring.clone(), mem.cursor.clone()
    env.close()
    return ring, cursor


def test_rollout_ring_vs_reference_and_oracle(env, oracle_launches):
    """1 024 envs, synthetic sampler, four launches of 100 steps pushed into 4 096 slots: after each push the
    ring equals replay_reference fed the same device buffers, and matches the oracle's transitions pushed the
    same way (columns 22 and 23 exactly, the rest within the parity tolerances); a second run from the same
    initial state gives the same ring bit for bit."""
    sc, launches = oracle_launches
    precision = env.precision
    ref = replay_reference(ROLL_RING, NP_REAL[precision])          # fed the device's own buffers
    want = replay_reference(ROLL_RING, np.float64)                 # fed the oracle's records
    worst = {}

    def check(launch, mem, out):
        torch.cuda.synchronize()
        count = int(out["transition_count"].item())
        assert count == len(launches[launch]), f"launch {launch}: {count} records vs {len(launches[launch])}"
        ref.push(out["transitions"].cpu().numpy(), count)
        same_memory(mem, ref)
        want.push(launches[launch], count)
        n = len(want)
        got, exp = mem.ring[:n].cpu().numpy().astype(np.float64), want.ring[:n]
        assert np.array_equal(got[:, 23], exp[:, 23]), f"launch {launch}: env ids"
        assert np.array_equal(got[:, 22], exp[:, 22]), f"launch {launch}: masks"
        cols = np.r_[0:10, 12:22]
        if n:
            worst["obs"] = max(worst.get("obs", 0.0), rel_err(got[:, cols], exp[:, cols], np.r_[OBS_SCALE, OBS_SCALE]).max())
            worst["reward"] = max(worst.get("reward", 0.0), rel_err(got[:, 11], exp[:, 11], 1.0).max())
            worst["action_rel"] = max(worst.get("action_rel", 0.0), rel_err(got[:, 10], exp[:, 10], 1.0).max())
            worst["action_abs"] = max(worst.get("action_abs", 0.0), np.abs(got[:, 10] - exp[:, 10]).max())

    ring, cursor = run_rollouts(sc, precision, check)
    print(f"float{precision} ring vs oracle, worst:", {k: f"{v:.2e}" for k, v in worst.items()}, "cursor", cursor.tolist())
    assert int(cursor[0]) == sum(len(t) for t in launches) and int(cursor[1]) == 0
    if precision == 64:
        assert worst["obs"] <= TOL64 and worst["reward"] <= TOL64 and worst["action_rel"] <= TOL64, worst
    else:
        assert worst["obs"] <= 1e-5 and worst["reward"] <= 1e-5 and worst["action_abs"] <= 1e-6, worst
    # the same initial state again: the same ring, bit for bit
    ring2, cursor2 = run_rollouts(sc, precision)
    assert torch.equal(cursor, cursor2) and np.array_equal(bits(ring), bits(ring2))


# ---------------------------------------------------------------------------------------------
# sample
# ---------------------------------------------------------------------------------------------
def test_sample_equals_reference(env):
    """U = 33 minibatches of B = 64 (no multiple of the block) from an empty ring, sizes 1, 40 (the batch
    wraps), 64 and 257, and a wrapped ring."""
    rng = np.random.default_rng(14)
    U, B = 33, 64
    mem, ref = ReplayMemory(env, RING_CAP, seed=77), replay_reference(RING_CAP, NP_REAL[env.precision], seed=77)
    draws = 0
    for add, size in ((0, 0), (1, 1), (39, 40), (24, 64), (193, 257), (100, 257)):
        if add:
            push_both(mem, ref, source(rng, env.precision, add), add)
        got, want = mem.sample(B, U), ref.sample(B, U)
        same_batches(got, want)
        draws += U
        assert len(mem) == size and int(mem.cursor[2].item()) == draws
        if size == 0:
            assert (got["index"] == -1).all() and not got["state"].any()
        else:
            idx = got["index"].cpu().numpy()
            assert all(len(set(row[:size].tolist())) == min(size, B) for row in idx)
        again = mem.sample(B, U)
        same_batches(again, ref.sample(B, U))
        draws += U
        if size > 1:
            assert not torch.equal(again["index"], got["index"])
    same_memory(mem, ref)
    assert int(ref.cursor[0]) > RING_CAP          # the last state was a wrapped ring
    # a checkpoint replays the same minibatches
    sd = mem.state_dict()
    first = {k: v.clone() for k, v in mem.sample(B, U).items()}
    push_both(mem, ref, source(rng, env.precision, 50), 50)
    other = ReplayMemory(env, RING_CAP, seed=1)
    other.load_state_dict(sd)
    replay = other.sample(B, U)
    torch.cuda.synchronize()
    for k in first:
        assert np.array_equal(bits(replay[k]), bits(first[k])), k


def test_sample_reuses_out(env):
    mem = ReplayMemory(env, 64)
    mem.push(transitions=dev(source(np.random.default_rng(1), env.precision, 64, room=64)), count=count_of(64))
    out = mem.sample(8, 2)
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    out2 = mem.sample(8, 2, out=out)
    assert out2 is out and {k: v.data_ptr() for k, v in out.items()} == ptrs
    assert mem.sample(8, 3, out=out)["state"].shape == (3, 8, 10)


# ---------------------------------------------------------------------------------------------
# graph
# ---------------------------------------------------------------------------------------------
def test_push_and_sample_in_a_graph(env):
    """After reserve, push + sample captured as one linear chain; three replays with new source contents."""
    rng = np.random.default_rng(15)
    U, B = 3, 64
    mem, ref = ReplayMemory(env, RING_CAP), replay_reference(RING_CAP, NP_REAL[env.precision])
    mem.reserve(SRC_CAP)
    src = torch.zeros((SRC_CAP, DIM), dtype=env.dtype, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)

    def load(c):
        a = source(rng, env.precision, c)
        src.copy_(dev(a))
        count.fill_(c)
        return a
    # one eager pass on a side stream first (it also fixes the output tensors the graph writes)
    a = load(100)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        mem.push(transitions=src, count=count)
        out = mem.sample(B, U)
    torch.cuda.current_stream(DEV).wait_stream(side)
    ref.push(a, 100)
    same_batches(out, ref.sample(B, U))
    graph = torch.cuda.CUDAGraph()
    a = load(90)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        mem.push(transitions=src, count=count)
        mem.sample(B, U, out=out)
    same_memory(mem, ref)                      # capturing ran nothing
    for c in (90, 700, 33):
        a = load(c)
        graph.replay()
        ref.push(a, c)
        same_batches(out, ref.sample(B, U))
        same_memory(mem, ref)


# ---------------------------------------------------------------------------------------------
# validation
# ---------------------------------------------------------------------------------------------
def test_invalid_arguments_rejected(env):
    mem = ReplayMemory(env, RING_CAP)
    good = torch.zeros((SRC_CAP, DIM), dtype=env.dtype, device=DEV)
    one = count_of(1)
    flat = torch.zeros(SRC_CAP * DIM + 4, dtype=env.dtype, device=DEV)
    with pytest.raises(_lib.SitError, match="src must be aligned to 4 reals"):
        mem.push(transitions=flat[1:1 + SRC_CAP * DIM].view(SRC_CAP, DIM), count=one)
    other = torch.float64 if env.precision == 32 else torch.float32
    with pytest.raises(ValueError, match="dtype"):
        mem.push(transitions=good.to(other), count=one)
    with pytest.raises(ValueError, match="contiguous"):
        mem.push(transitions=torch.zeros((SRC_CAP, DIM + 1), dtype=env.dtype, device=DEV)[:, :DIM], count=one)
    with pytest.raises(ValueError, match="shape"):
        mem.push(transitions=good.view(-1, DIM // 2), count=one)
    with pytest.raises(ValueError, match="int32"):
        mem.push(transitions=good, count=one.to(torch.int64))
    with pytest.raises(_lib.SitError, match="batch must be positive"):
        mem.sample(0)
    with pytest.raises(_lib.SitError, match="n_batches must be positive"):
        mem.sample(4, 0)
    with pytest.raises(_lib.SitError, match="max_src_capacity must be positive"):
        mem.reserve(0)
    ring = torch.zeros(RING_CAP * DIM + 4, dtype=env.dtype, device=DEV)
    mem.ring = ring[1:1 + RING_CAP * DIM].view(RING_CAP, DIM)
    with pytest.raises(_lib.SitError, match="ring must be aligned to 4 reals"):
        mem.push(transitions=good, count=one)
    with pytest.raises(_lib.SitError, match="ring must be aligned to 4 reals"):
        mem.sample(4)
    torch.cuda.synchronize()
    assert mem.cursor.cpu().tolist() == [0, 0, 0, 0]      # nothing was launched
