"""GPU checks of the scores (include/sit.h: sit_score_*; sac_maritime_ast_amd/score.py).

1. Synthetic record buffers against score_reference, the whole block bit for bit (sizes across the chunk and
   group boundaries of the summation tree, a count above the capacity, the forced cases).  2. Consecutive
   updates, consume, fresh.  3. keep.  4. update + keep as a HIP graph over changing buffers.  5. The training
   iteration (launch, push, update, keep, update_many) captured against the same iteration run eagerly.
6. A real producer.  7. Scorer.run.  8. Argument errors."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sit = pytest.importorskip("sac_maritime_ast_amd")
from sac_maritime_ast_amd import (EpisodeLog, ReplayMemory, Scoreboard, Scorer, VecMultiShipRLEnv, _lib,  # noqa: E402
                                  make_scenario, sac, score_reference)
from sac_maritime_ast_amd.samplers import GaussianPolicy, PolicySampler, pack_actor_weights, unpack_actor_weights  # noqa: E402
from sac_maritime_ast_amd.score import REFERENCE_CLASSES, new_block  # noqa: E402
import score_cases as C  # noqa: E402
from sac_cases import DEV, device_memory  # noqa: E402

AW = _lib.SIT_ACTOR_WEIGHTS
SEED = 25450
JUNK = 9e9                                   # fills the slots past the count: reading one shows in every field


@pytest.fixture(scope="module")
def env():
    e = VecMultiShipRLEnv(scenario=make_scenario(64), precision=32, device=DEV)
    yield e
    e.close()


def buffer(rec, capacity=None, count=None):
    """Device (records [capacity, 32], count int64[1]) holding `rec` in its first rows, junk behind them."""
    capacity = len(rec) + 3 if capacity is None else capacity
    host = np.full((capacity, C.DIM), JUNK)
    host[:, 1] = 0                           # junk passes every episode_limit
    n = min(len(rec), capacity)
    host[:n] = rec[:n]
    return (torch.from_numpy(host).to(DEV),
            torch.tensor([len(rec) if count is None else count], dtype=torch.int64, device=DEV))


def block_of(board):
    torch.cuda.synchronize()
    return board.block.cpu().numpy()


def same_bits(got, want):
    return np.array_equal(C.bits(got), C.bits(want))


# ---------------------------------------------------------------------------------------------
# 1. synthetic buffers, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", C.SIZES)
def test_synthetic_records_bit_for_bit(env, m):
    rec = C.synthetic(m, m)
    records, count = buffer(rec)
    board = Scoreboard(env)
    board.update(records=records, count=count)
    got = block_of(board)
    assert same_bits(got, score_reference(rec)), (got[:17], score_reference(rec)[:17])
    assert got[0] == m and int(count.item()) == m


def test_count_above_capacity_and_below_zero(env):
    rec = C.synthetic(1000, 5)
    records, count = buffer(rec, capacity=300)
    board = Scoreboard(env)
    board.update(records=records, count=count)
    assert same_bits(block_of(board), score_reference(rec[:300]))
    board.update(records=records, count=count, consume=True)
    want = score_reference(rec[:300], score_reference(rec[:300]))
    want[5] = 700
    assert same_bits(block_of(board), want) and int(count.item()) == 0
    count.fill_(-5)
    board.update(records=records, count=count, consume=True, fresh=True)
    want = new_block()
    want[6] = 1
    assert same_bits(block_of(board), want) and int(count.item()) == 0


FORCED = C.forced_cases()


@pytest.mark.parametrize("name", sorted(FORCED))
def test_forced_cases(env, name):
    rec, kw = FORCED[name]
    records, count = buffer(rec)
    board = Scoreboard(env, kw.get("classes", REFERENCE_CLASSES))
    board.update(records=records, count=count, episode_limit=kw.get("episode_limit", 0))
    assert same_bits(block_of(board), score_reference(rec, **kw))


# ---------------------------------------------------------------------------------------------
# 2. consecutive updates, consume, fresh
# ---------------------------------------------------------------------------------------------
def test_three_updates_equal_the_reference_fed_the_pieces(env):
    rec = C.synthetic(900, 31)
    rec[[50, 400, 800], 3] = 4e3                                   # the first piece's best stays
    pieces = [rec[:257], rec[257:300], rec[300:]]
    board, want = Scoreboard(env), None
    for i, piece in enumerate(pieces):
        records, count = buffer(piece, capacity=700)
        board.update(records=records, count=count)
        want = score_reference(piece, want)
        assert same_bits(block_of(board), want), i
    assert want[6] == 3 and want[7] == 0 and want[32 + 0] == 50 % 37


def test_consume_empties_the_log_and_plain_updates_write_nothing(env):
    rec = C.synthetic(500, 32)
    records, count = buffer(rec, capacity=400)
    before = records.clone()
    board = Scoreboard(env)
    board.update(records=records, count=count)
    board.update(records=records, count=count, episode_limit=3)
    torch.cuda.synchronize()
    assert torch.equal(records.view(torch.int64), before.view(torch.int64)) and int(count.item()) == 500
    assert block_of(board)[5] == 0
    want = score_reference(rec[:400], score_reference(rec[:400]), episode_limit=3)
    for i in range(2):
        count.fill_(500)
        board.update(records=records, count=count, consume=True)
        want = score_reference(rec[:400], want)
        want[5] = 100 * (i + 1)
        assert same_bits(block_of(board), want) and int(count.item()) == 0
    assert torch.equal(records.view(torch.int64), before.view(torch.int64))
    board.update(records=records, count=count, consume=True)      # the log is empty now: nothing new, nothing dropped
    want[6], want[7] = want[6] + 1, 0
    assert same_bits(block_of(board), want)


def test_fresh_resets_first(env):
    a, b = C.synthetic(300, 33), C.synthetic(200, 34)
    a[7, 3] = 1e6                                                  # a best the second buffer cannot beat
    board = Scoreboard(env)
    board.update(records=buffer(a)[0], count=buffer(a)[1])
    records, count = buffer(b)
    board.update(records=records, count=count, fresh=True)
    assert same_bits(block_of(board), score_reference(b))
    board.reset()
    assert same_bits(block_of(board), new_block())


def test_state_dict_round_trip(env):
    rec = C.synthetic(300, 35)
    board, other = Scoreboard(env), Scoreboard(env)
    board.update(records=buffer(rec)[0], count=buffer(rec)[1])
    other.load_state_dict(board.state_dict())
    assert same_bits(block_of(other), score_reference(rec))
    out = other.read()
    assert out["episodes"] == 300 and out["best"]["ret"] == rec[:, 3].max() and out["best_stamp"] is None
    with pytest.raises(ValueError):
        other.load_state_dict({"block": board.block[:-1]})


# ---------------------------------------------------------------------------------------------
# 3. keep
# ---------------------------------------------------------------------------------------------
SENTINEL = -777.25


def keep_blocks():
    g = torch.Generator().manual_seed(9)
    src = [torch.randn(n, generator=g).to(DEV) for n in (1, 3, AW)]
    dst = [torch.full_like(s, SENTINEL) for s in src]
    return src, dst


def test_keep_copies_after_an_improving_update_only(env):
    low, high = C.synthetic(100, 41), C.synthetic(100, 42)
    low[:, 3], high[:, 3] = -np.abs(low[:, 3]), -np.abs(high[:, 3])
    high[60, 3] = 12.5
    board = Scoreboard(env)
    src, dst = keep_blocks()
    stamp = torch.tensor([41, -1, -1], dtype=torch.int64, device=DEV)
    board.update(records=buffer(high)[0], count=buffer(high)[1])
    board.keep(list(zip(src, dst)), stamp=stamp)
    torch.cuda.synchronize()
    for s, d in zip(src, dst):
        assert torch.equal(s.view(torch.int32), d.view(torch.int32))
    want = score_reference(high)
    want[16] = 41
    assert same_bits(block_of(board), want) and board.read()["best_stamp"] == 41
    # a non-improving update: sentinel-filled destinations and [16] stay as they are
    dst2 = [torch.full_like(s, SENTINEL) for s in src]
    stamp.fill_(99)
    board.update(records=buffer(low)[0], count=buffer(low)[1])
    board.keep(list(zip(src, dst2)), stamp=stamp)
    torch.cuda.synchronize()
    for d in dst2:
        assert torch.all(d == SENTINEL)
    want = score_reference(low, want)
    assert want[7] == 0 and want[16] == 41 and same_bits(block_of(board), want)
    # an equal return does not replace either; a greater one does, and without a stamp [16] stays
    board.update(records=buffer(high)[0], count=buffer(high)[1])
    board.keep(list(zip(src, dst2)), stamp=stamp)
    want = score_reference(high, want)
    assert want[7] == 0 and same_bits(block_of(board), want) and all(torch.all(d == SENTINEL) for d in dst2)
    high[60, 3] = 13.0
    board.update(records=buffer(high)[0], count=buffer(high)[1])
    board.keep([(src[1], dst2[1])])
    board.keep([], stamp=None)
    torch.cuda.synchronize()
    assert torch.equal(dst2[1], src[1]) and torch.all(dst2[0] == SENTINEL) and torch.all(dst2[2] == SENTINEL)
    want = score_reference(high, want)
    assert want[7] == 1 and same_bits(block_of(board), want)
    board.keep([], stamp=stamp)                                    # no blocks: the stamp alone
    assert block_of(board)[16] == 99


# ---------------------------------------------------------------------------------------------
# 4. update + keep as a graph over changing buffers
# ---------------------------------------------------------------------------------------------
def test_graph_of_update_and_keep_equals_the_eager_sequence(env):
    rounds = [C.synthetic(n, 50 + i) for i, n in enumerate((300, 0, 513, 40, 700))]
    for i, r in enumerate(rounds):
        r[:, 3] = -np.abs(r[:, 3])
    rounds[0][5, 3], rounds[2][400, 3], rounds[3][7, 3], rounds[4][699, 3] = 1.0, 3.0, 2.0, 3.0   # improve: 0, 2 only
    weights = [torch.full((AW,), float(i), device=DEV) for i in range(len(rounds))]

    def run(graph):
        board = Scoreboard(env)
        board.reserve(768)
        records, count = buffer(np.zeros((0, C.DIM)), capacity=768)
        src, kept = torch.zeros(AW, device=DEV), torch.full((AW,), SENTINEL, device=DEV)
        stamp = torch.zeros(1, dtype=torch.int64, device=DEV)

        def step():
            board.update(records=records, count=count, consume=True)
            board.keep([(src, kept)], stamp=stamp)
        if graph:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step()
            board.reset()
        blocks = []
        for i, r in enumerate(rounds):
            records[:len(r)].copy_(torch.from_numpy(r))
            count.fill_(len(r))
            src.copy_(weights[i])
            stamp.fill_(100 + i)
            g.replay() if graph else step()
            blocks.append(block_of(board))
        return blocks, kept.cpu()
    eager, kept_eager = run(False)
    replayed, kept_graph = run(True)
    want = None
    for i, r in enumerate(rounds):
        want = score_reference(r, want)
        if want[7]:
            want[16] = 100 + i
        assert same_bits(eager[i], want) and same_bits(replayed[i], want), i
    assert want[16] == 102 and torch.all(kept_eager == 2.0) and torch.all(kept_graph == 2.0)


# ---------------------------------------------------------------------------------------------
# 5. the training iteration: launch, push, update, keep, update_many
# ---------------------------------------------------------------------------------------------
ITERATIONS = 10


def iteration_parts():
    e = VecMultiShipRLEnv(scenario=make_scenario(32), precision=32, device=DEV)
    e.reset()
    e.init_step()
    torch.manual_seed(4)
    pol = GaussianPolicy().to(DEV)
    with torch.no_grad():
        pol.net[0].weight.mul_(1e-3)             # raw observations: keep the actions inside (-1, 1)
    sampler = PolicySampler(e, pol, chunk=40, seed=SEED, transition_capacity=1024, episode_capacity=128)
    learner = sac.SacLearner(e, pol, seed=SEED, gradient="hip")
    sampler.share_weights(learner.actor_weights)
    mem = device_memory(e)                       # 256 records to start from, so the first update has its batch
    mem.reserve(1024)
    board = Scoreboard(e)
    board.reserve(128)
    best_actor = torch.full((AW,), SENTINEL, device=DEV)

    def iteration():
        mem.push(sampler.launch())
        board.update(sampler.episodes, consume=True)
        board.keep([(learner.actor_weights, best_actor)], stamp=learner.clock)
        learner.update_many(mem, 64, 2)
    return e, board, best_actor, learner, iteration


def test_the_iteration_as_one_graph():
    e, board, best_actor, learner, iteration = iteration_parts()
    te, tboard, tbest, tlearner, titeration = iteration_parts()
    try:
        for _ in range(ITERATIONS):
            titeration()
        iteration()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            iteration()
        for _ in range(ITERATIONS - 1):
            graph.replay()
        got, want = block_of(board), block_of(tboard)
        print("iteration graph:", tboard.read())
        assert same_bits(got, want)
        assert torch.equal(best_actor.view(torch.int32), tbest.view(torch.int32))
        assert torch.equal(learner.actor_weights.view(torch.int32), tlearner.actor_weights.view(torch.int32))
        out = board.read()
        assert out["updates"] == ITERATIONS and out["episodes"] >= 1 and out["dropped"] == 0
        # the kept block is the actor as it stood before update number best_stamp, not the current one
        assert out["best_stamp"] is not None and out["best_stamp"] % 2 == 0 and out["best_stamp"] < 2 * ITERATIONS
        assert not torch.any(best_actor == SENTINEL) and not torch.equal(best_actor, learner.actor_weights)
        pol = unpack_actor_weights(best_actor, GaussianPolicy().to(DEV))
        assert torch.equal(pack_actor_weights(pol), best_actor)
    finally:
        e.close()
        te.close()


# ---------------------------------------------------------------------------------------------
# 6. a real producer: make_scenario(128), 4 launches x 100 steps (tests/test_gpu_episodes.py)
# ---------------------------------------------------------------------------------------------
LAUNCHES, CHUNK, N_REAL = 4, 100, 128


def started_env(n, precision=32):
    e = VecMultiShipRLEnv(scenario=make_scenario(n), precision=precision, device=DEV)
    e.reset()
    e.init_step()
    return e


def test_real_producer_scored_per_launch():
    ref_env = started_env(N_REAL)
    log = EpisodeLog(ref_env, capacity=256)
    for _ in range(LAUNCHES):
        log.update(ref_env.rollout(CHUNK, seed=SEED))
    rec = log.drain()["records"]
    ref_env.close()
    assert len(rec) >= 20
    e = started_env(N_REAL)
    log, board = EpisodeLog(e, capacity=256), Scoreboard(e)
    want = None
    for a in range(LAUNCHES):
        log.update(e.rollout(CHUNK, seed=SEED))
        board.update(log, consume=True)
        part = rec[(rec[:, 6] >= a * CHUNK) & (rec[:, 6] < (a + 1) * CHUNK)]
        want = score_reference(part, want)
        assert same_bits(block_of(board), want), a
    out = board.read()
    assert out["episodes"] == len(rec) and out["dropped"] == 0 and int(log.count.item()) == 0
    assert out["mean_return"] == want[1] / len(rec) and sum(out["status_record"].values()) >= len(rec)
    e.close()


# ---------------------------------------------------------------------------------------------
# 7. Scorer.run
# ---------------------------------------------------------------------------------------------
SCORE_LAUNCHES, SCORE_CHUNK, N_SCORE = 12, 40, 64


@functools.lru_cache(maxsize=None)
def scoring_policy():
    torch.manual_seed(6)
    pol = GaussianPolicy().to(DEV)
    with torch.no_grad():
        pol.net[0].weight.mul_(1e-3)
    return pol


def test_scorer_runs_a_deterministic_round():
    pol = scoring_policy()
    block = pack_actor_weights(pol).to(DEV)
    e = VecMultiShipRLEnv(scenario=make_scenario(N_SCORE), precision=32, device=DEV)
    scorer = Scorer(e, episodes_per_env=1, chunk=SCORE_CHUNK, seed=SEED)
    assert scorer.capacity == 4 * N_SCORE
    first = scorer.run(block, SCORE_LAUNCHES, check_every=5)
    first_bits = block_of(scorer.board)
    second = scorer.run(block, SCORE_LAUNCHES, check_every=5)
    assert same_bits(block_of(scorer.board), first_bits)
    module = scorer.run(pol, SCORE_LAUNCHES, check_every=5)
    assert same_bits(block_of(scorer.board), first_bits)
    e.close()
    # an independent EpisodeLog of the same run
    e = started_env(N_SCORE)
    sm = PolicySampler(e, pol, chunk=SCORE_CHUNK, seed=SEED, deterministic=True, episode_capacity=4 * N_SCORE)
    for _ in range(first["launches"]):
        sm.launch()
    rec = sm.episodes.drain()["records"]
    e.close()
    finished = rec[rec[:, 1] == 0]
    print("scorer:", {k: v for k, v in first.items() if k != "best"}, "records", len(rec))
    assert len(np.unique(finished[:, 0])) == len(finished) >= 1
    assert first["episodes"] == len(finished) and first["dropped"] == 0
    assert first["complete"] == (len(finished) == N_SCORE)
    assert first["launches"] == SCORE_LAUNCHES or (first["complete"] and first["launches"] % 5 == 0)
    assert first["best"]["episode"] < 1 and first["best"]["ret"] == finished[:, 3].max() == first["max"]
    assert first["mean_return"] == second["mean_return"] == module["mean_return"]
    assert first["status_record"] == second["status_record"] and sum(first["status_record"].values()) >= len(finished)


# ---------------------------------------------------------------------------------------------
# 8. argument errors
# ---------------------------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing(env):
    rec = C.synthetic(50, 61)
    records, count = buffer(rec)
    board = Scoreboard(env)
    board.update(records=records, count=count)
    before = block_of(board).copy()
    src, dst = keep_blocks()
    cpu = torch.zeros(4)
    bad_updates = [("records", dict(records=records.cpu(), count=count)), ("records", dict(records=records.float(), count=count)),
                   ("records", dict(records=records[:, :31], count=count)), ("records", dict(records=records[:0], count=count)),
                   ("records", dict(records=records.t(), count=count)), ("records", dict(records=records[:, ::2], count=count)),
                   ("count", dict(records=records, count=count.int())), ("count", dict(records=records, count=count.cpu())),
                   ("count", dict(records=records, count=torch.zeros(2, dtype=torch.int64, device=DEV))),
                   ("episode_limit", dict(records=records, count=count, episode_limit=-1)),
                   ("records", dict())]
    for word, kw in bad_updates:
        with pytest.raises(ValueError, match=word):
            board.update(**kw)
    with pytest.raises(ValueError, match="records"):
        board.update(EpisodeLog(env, capacity=0))
    with pytest.raises(ValueError, match="classes"):
        Scoreboard(env, [("c", 1, 0)] * 9)
    bad_keeps = [("blocks", dict(blocks=[(src[0], dst[0])] * 5)), ("src", dict(blocks=[(cpu, dst[0])])),
                 ("dst", dict(blocks=[(src[1], dst[1].double())])), ("dst", dict(blocks=[(src[1], dst[0])])),
                 ("src", dict(blocks=[(src[2][1:4], dst[1])])), ("dst", dict(blocks=[(src[1], dst[2][2:5])])),
                 ("src", dict(blocks=[(src[2][:0], dst[2][:0])])), ("src", dict(blocks=[(src[2][::2], dst[2][::2])])),
                 ("stamp", dict(blocks=[(src[0], dst[0])], stamp=torch.zeros(1, dtype=torch.int32, device=DEV))),
                 ("stamp", dict(blocks=[(src[0], dst[0])], stamp=torch.zeros(1, dtype=torch.int64)))]
    for word, kw in bad_keeps:
        with pytest.raises(ValueError, match=word):
            board.keep(**kw)

    def args(**over):
        a = _lib.ScoreArgs()
        a.record_capacity, a.records, a.record_count = records.shape[0], records.data_ptr(), count.data_ptr()
        a.score = board.block.data_ptr()
        for k, v in over.items():
            setattr(a, k, v)
        return a
    for over, word in (({"records": None}, "records"), ({"record_count": None}, "record_count"), ({"score": None}, "score"),
                       ({"record_capacity": 0}, "record_capacity"), ({"flags": 4}, "flags"), ({"episode_limit": -2}, "episode_limit"),
                       ({"score": board.block.data_ptr() + 4}, "score")):
        with pytest.raises(_lib.SitError, match=rf"sit error {_lib.SIT_E_INVALID}: score: {word}"):
            env._call("sit_score_update", ctypes.byref(args(**over)), env._stream())
    k = _lib.ScoreKeepArgs()
    k.n_blocks, k.score = 1, board.block.data_ptr()
    k.src[0], k.dst[0], k.floats[0] = src[1].data_ptr(), dst[1].data_ptr(), 3
    for field, value, word in (("n_blocks", 5, "n_blocks"), ("score", None, "score")):
        good = getattr(k, field)
        setattr(k, field, value)
        with pytest.raises(_lib.SitError, match=rf"sit error {_lib.SIT_E_INVALID}: score: {word}"):
            env._call("sit_score_keep", ctypes.byref(k), env._stream())
        setattr(k, field, good)
    for field, value, word in (("floats", 0, "floats"), ("src", src[1].data_ptr() + 4, "src"), ("dst", None, "dst")):
        good = getattr(k, field)[0]
        getattr(k, field)[0] = value
        with pytest.raises(_lib.SitError, match=rf"sit error {_lib.SIT_E_INVALID}: score: {word}"):
            env._call("sit_score_keep", ctypes.byref(k), env._stream())
        getattr(k, field)[0] = good
    with pytest.raises(_lib.SitError, match="max_records"):
        board.reserve(0)
    with pytest.raises(_lib.SitError, match="score: score"):
        env._call("sit_score_reset", None, env._stream())
    assert same_bits(block_of(board), before) and int(count.item()) == 50
    for d in dst:
        assert torch.all(d == SENTINEL)
