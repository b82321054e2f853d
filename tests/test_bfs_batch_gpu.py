"""
The pooled BFS (rc_bfs_batch_* behind `BFS.search_batch(..., slots=S)` and `BFSBatch`) against the restated FIFO loop
(oracle/agents.py:BFS), game by game and without tolerance, for every number of slots and every chunk; against the reference's own
runs (tests/golden/bfs_golden.npz, bfs_cut_golden.npz); step by step against the oracle's discovery order; and against the serial
form of the same agent.  The oracle runs once per max_states (<= 0.2 s each) and is shared by the tests.
"""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import agents as oa  # noqa: E402  (checker only)
from oracle import cube as oc  # noqa: E402

CAPS = (1, 13, 300, 2000)


@functools.lru_cache(maxsize=None)
def games() -> np.ndarray:
    """24 games: game g is the solved cube after g % 6 random moves, all drawn from one stream."""
    rng = np.random.RandomState(7)
    out = []
    for g in range(24):
        s = oc.get_solved()
        for a in rng.randint(0, 12, size=g % 6):
            s = oc.rotate(s, *oc.ACTION_SPACE[a])
        out.append(s)
    return np.array(out)


@functools.lru_cache(maxsize=None)
def expected(cap: int) -> tuple:
    """Per game (solved, len(agent), action queue) of the oracle under max_states = cap."""
    out = []
    for s in games():
        ref = oa.BFS()
        ok = ref.search(s, cap)
        out.append((ok, len(ref), list(ref.action_queue)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def discovery(g: int) -> dict:
    """Game g's states in the oracle's discovery order (its dict in insertion order) with parent index and action: from a run whose
    cap no search of these tests reaches, so every committed node store is a prefix of it."""
    ref = oa.BFS()
    ref.search(games()[g], 2100)
    keys = list(ref.states.keys())
    index = {k: i for i, k in enumerate(keys)}
    return {"states": np.array([np.frombuffer(k, dtype=np.int8) for k in keys]).reshape(len(keys), 20),
            "parent": np.array([0 if ref.states[k][0] is None else index[ref.states[k][0]] for k in keys], dtype=np.int64),
            "action": np.array([0 if ref.states[k][1] is None else ref.states[k][1] for k in keys], dtype=np.int64)}


def _same(res, want, what):
    for g, (ok, seen, queue) in enumerate(want):
        assert bool(res.solved[g]) == ok, (what, g)
        assert res.nodes[g] == seen, (what, g, int(res.nodes[g]), seen)
        assert res.lengths[g] == (len(queue) if ok else -1), (what, g)
        assert list(res.queues[g]) == queue, (what, g)


def test_the_inputs_hold_every_outcome():
    """What the cases below rest on: solved roots, solutions of 1, 2 and 3 moves, games cut at exactly 2000, overshoots at 13 / 300."""
    at = expected(2000)
    assert [seen for ok, seen, q in at if ok and len(q) == 1] == [6, 8, 2, 4, 1, 7]
    assert {len(q) for ok, _, q in at if ok} == {0, 1, 2, 3} and sum(1 for ok, seen, _ in at if not ok and seen == 2000) >= 3
    assert {seen for ok, seen, _ in expected(13) if not ok} == {13} and {seen for ok, seen, _ in expected(300) if not ok} == {306}
    assert all(seen == (0 if ok else 1) for ok, seen, _ in expected(1))


@pytest.mark.parametrize("chunk", [1, 5, 37, 1024])
@pytest.mark.parametrize("slots", [1, 3, 24])
def test_mixed_pool_equals_the_oracle_for_every_slot_count_and_chunk(slots, chunk):
    from librubiks.solving.agents import BFS
    agent = BFS(chunk=chunk)
    for cap in CAPS:
        res = agent.search_batch(games(), None, cap, slots=slots)
        _same(res, expected(cap), (slots, chunk, cap))
        ok = np.array([e[0] for e in expected(cap)])
        seen = np.array([e[1] for e in expected(cap)])
        assert np.array_equal(res.status, np.where(ok, np.where(seen == 0, 4, 1), 2))
        assert len(agent) == expected(cap)[0][1] and list(agent.action_queue) == expected(cap)[0][2]
        assert res.game_seconds.shape == (24,) and (res.game_seconds >= 0).all()
    assert set(res.status.tolist()) == {1, 2, 4}           # solved, cut and solved root all occur at 2000
    assert (res.iterations[res.status == 4] == 0).all() and (res.iterations[res.status != 4] >= 1).all()


def test_identical_scrambles_keep_their_own_tables():
    """The same scramble in neighbouring slots: were a table or a child segment shared, each would see the other's states as known."""
    from librubiks.solving.agents import BFS
    which = [23, 23, 17, 23, 17, 9, 9]
    res = BFS(chunk=5).search_batch(games()[which], None, 2000, slots=4)
    _same(res, [expected(2000)[g] for g in which], "twins")


def _plant(batch, slots, roots, first, caps):
    batch.plant(np.asarray(slots), roots, first, np.asarray(caps))


def _words(batch):
    import torch
    host, ev = batch.snapshot()
    ev.synchronize()
    torch.cuda.synchronize()
    return host.numpy().copy()


def test_after_every_step_the_node_store_is_a_prefix_of_the_discovery_order():
    from librubiks.cube.device import DeviceCubes
    from librubiks.solving import bfs_batch_device as bb
    S, C, cap = 3, 5, 2000
    roots = DeviceCubes.from_numpy(games())
    batch = bb.BFSBatch(S, cap, C)
    owner, waiting = np.full(S, -1), list(range(24))
    committed, frozen, results = np.zeros(S, dtype=np.int64), {}, {}
    words = _words(batch)
    assert (words[bb.W_STATUS] == bb.EMPTY).all()
    steps = 0
    while waiting or (owner >= 0).any():
        for s in range(S):
            if owner[s] < 0 and waiting:
                owner[s] = waiting.pop(0)
                _plant(batch, [s], roots, owner[s], [cap])
                frozen.pop(s, None)
                committed[s] = 1
        batch.step(1)
        steps += 1
        words = _words(batch)
        bb.check_words(words, batch.capacity)
        for s in np.flatnonzero(owner >= 0):
            w, g = words[:, s], owner[s]
            assert 0 <= w[bb.W_LO] <= w[bb.W_LEVEL_END] <= w[bb.W_NODES] and w[bb.W_MAX_STATES] == cap, (g, w)
            if w[bb.W_STATUS] == bb.RUNNING:
                assert w[bb.W_LO] < w[bb.W_LEVEL_END] and w[bb.W_NODES] < cap, (g, w)
                committed[s] = w[bb.W_NODES]
            elif s in frozen:
                assert np.array_equal(frozen[s], w), (g, frozen[s], w)      # a finished slot's words no longer change
            else:
                frozen[s] = w.copy()
            if w[bb.W_STATUS] == bb.ROOT_SOLVED:                           # nothing stored (agents.py:100)
                assert w[bb.W_NODES] == 0
                continue
            n, d = int(committed[s]), discovery(g)
            arr = batch.node_arrays(s, n)
            assert n <= len(d["states"]), (g, n)
            assert np.array_equal(arr["states"], d["states"][:n]), (g, steps)
            assert np.array_equal(arr["parent"], d["parent"][:n]) and np.array_equal(arr["action"], d["action"][:n]), (g, steps)
        for s in np.flatnonzero(owner >= 0):
            if s in frozen and (steps % 3 == 0 or not waiting):             # (a finished game stays a while: see `frozen`)
                w = frozen[s]
                q = batch.take_queues(np.array([s]), max(1, w[bb.W_QUEUE_LEN]))
                q[1].synchronize()
                solved = w[bb.W_STATUS] in (bb.SOLVED, bb.ROOT_SOLVED)
                results[owner[s]] = (bool(solved), int(w[bb.W_NODES]), q[0].numpy()[0, :w[bb.W_QUEUE_LEN]].tolist() if solved else [])
                owner[s] = -1
        assert steps < 10_000
    assert [results[g] for g in range(24)] == list(expected(cap))


def test_reference_runs_of_config1_on_four_slots(bfs_golden):
    from librubiks.solving.agents import BFS
    res = BFS().search_batch(bfs_golden["states"], None, 10_000_000, slots=4)
    assert res.solved.all() and np.array_equal(res.lengths, bfs_golden["lengths"]) and np.array_equal(res.nodes, bfs_golden["seen"])
    for g, (length, queue) in enumerate(zip(bfs_golden["lengths"], bfs_golden["queues"])):
        assert list(res.queues[g]) == list(queue[:length])


def _run_pool(batch, roots, caps):
    """Every game of `roots` through the slots of `batch` with its own cap: -> per game (solved, nodes, queue)."""
    from librubiks.solving import bfs_batch_device as bb
    S, G = batch.S, roots.n
    owner, nxt, out = np.full(S, -1), 0, {}
    while len(out) < G:
        free = np.flatnonzero(owner < 0)[:G - nxt]
        if len(free):
            _plant(batch, free, roots, nxt, caps[nxt:nxt + len(free)])
            owner[free] = np.arange(nxt, nxt + len(free))
            nxt += len(free)
        batch.step(4)
        words = _words(batch)
        bb.check_words(words, batch.capacity)
        done = np.flatnonzero((owner >= 0) & (words[bb.W_STATUS] != bb.RUNNING))
        if len(done):
            host, ev, _ = batch.take_queues(done, max(1, words[bb.W_QUEUE_LEN, done].max()))
            ev.synchronize()
            for i, s in enumerate(done):
                solved = words[bb.W_STATUS, s] in (bb.SOLVED, bb.ROOT_SOLVED)
                out[owner[s]] = (bool(solved), int(words[bb.W_NODES, s]), host.numpy()[i, :words[bb.W_QUEUE_LEN, s]].tolist() if solved else [])
            owner[done] = -1
    return [out[g] for g in range(G)]


def test_reference_runs_with_a_cut_as_one_pool_with_per_game_caps():
    from conftest import GOLDEN
    from librubiks.cube.device import DeviceCubes
    from librubiks.solving import bfs_batch_device as bb
    g = np.load(os.path.join(GOLDEN, "bfs_cut_golden.npz"))
    batch = bb.BFSBatch(8, int(g["caps"].max()), 100)
    got = _run_pool(batch, DeviceCubes.from_numpy(g["states"]), g["caps"])
    for i, (solved, seen, queue) in enumerate(zip(g["solved"], g["seen"], g["queues"])):
        assert got[i] == (bool(solved), int(seen), [a for a in queue if a >= 0]), (i, int(g["caps"][i]))


def test_slot_reuse_first_col_and_skipped_list_entries():
    """A shallow game after a game cut at 2000 in the same slot; roots read from column 16 on of a table whose other columns hold
    the code 23; list entries -1 and S name no slot."""
    import torch
    from librubiks.cube.device import DeviceCubes
    from librubiks.solving import bfs_batch_device as bb
    S, cap = 4, 2000
    batch = bb.BFSBatch(S, cap, 37)
    deep, shallow, other = 4, 1, 8            # cut at 2000; solved in 1 move, 6 states in; solved in 2 moves, 27 states in
    assert expected(cap)[deep][:2] == (False, 2000)
    _plant(batch, [1], DeviceCubes.from_numpy(games()[[deep]]), 0, [cap])
    for _ in range(100):
        batch.step(4)
        if _words(batch)[bb.W_STATUS, 1] != bb.RUNNING:
            break
    w = _words(batch)
    assert w[bb.W_STATUS, 1] == bb.CUT and w[bb.W_NODES, 1] == 2000 and (w[bb.W_STATUS, [0, 2, 3]] == bb.EMPTY).all()
    table = DeviceCubes(torch.full((20, 48), 23, dtype=torch.int8, device="cuda"), 48)
    table.soa[:, 16:20] = torch.from_numpy(np.ascontiguousarray(games()[[shallow, deep, other, deep]].T)).cuda()
    before = w[:, [0, 3]].copy()
    _plant(batch, [1, -1, 2, S], table, 16, [cap, 7, cap, 7])          # columns 17 and 19 go nowhere
    w = _words(batch)
    assert np.array_equal(w[:, [0, 3]], before) and (w[bb.W_STATUS, [1, 2]] == bb.RUNNING).all() and (w[bb.W_NODES, [1, 2]] == 1).all()
    assert (w[bb.W_MAX_STATES, [1, 2]] == cap).all()
    for g, s in ((shallow, 1), (other, 2)):
        assert np.array_equal(batch.node_arrays(s, 1)["states"][0], games()[g])
    batch.step(4)
    w = _words(batch)
    bb.check_words(w, batch.capacity)
    host, ev, _ = batch.take_queues(np.array([1, 2]), 8)
    ev.synchronize()
    for i, (g, s) in enumerate(((shallow, 1), (other, 2))):
        ok, seen, queue = expected(cap)[g]
        assert ok and w[bb.W_STATUS, s] == bb.SOLVED and w[bb.W_NODES, s] == seen
        assert host.numpy()[i, :w[bb.W_QUEUE_LEN, s]].tolist() == queue
    assert (w[bb.W_STATUS, [0, 3]] == bb.EMPTY).all()


def test_pooled_search_batch_equals_the_serial_form_field_for_field():
    from librubiks.solving.agents import BFS
    serial = BFS().search_batch(games(), None, 2000)
    pooled = BFS().search_batch(games(), None, 2000, slots=5)
    for name in ("solved", "lengths", "nodes", "iterations", "status"):
        a, b = getattr(serial, name), getattr(pooled, name)
        assert a.shape == b.shape and np.array_equal(a, b), (name, a, b)
    assert np.array_equal(serial.queues.lengths(), pooled.queues.lengths())
    assert [list(q) for q in serial.queues] == [list(q) for q in pooled.queues]
    assert pooled.game_seconds.shape == serial.game_seconds.shape and pooled.seconds > 0


def test_evaluator_routes_bfs_to_the_pool_and_gets_the_same_games():
    from librubiks.solving.agents import BFS
    from librubiks.solving.evaluation import Evaluator
    out = []
    for slots in (None, 4):
        np.random.seed(42)
        agent = BFS()
        res, states, times = Evaluator(n_games=6, scrambling_depths=[1, 2, 3], max_states=500, slots=slots).eval(agent)
        assert (agent._pool is not None) == (slots is not None)             # the pooled form ran iff slots were given
        out.append((res, states))
        assert times.shape == (3, 6)
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert (out[0][0] != -1).any()


def test_a_time_limit_that_has_passed_ends_every_game_unsolved():
    from librubiks.solving.agents import BFS
    which = [g for g in range(24) if g % 6]                                  # (a solved root is solved before the clock is read)
    res = BFS().search_batch(games()[which], 1e-9, 2000, slots=4)
    assert not res.solved.any() and (res.lengths == -1).all() and (res.status == 2).all()
    assert (res.nodes[:4] == 1).all() and (res.nodes[4:] == 0).all()        # four were planted, nothing was expanded
    assert (res.game_seconds[4:] == 0).all() and (res.iterations[4:] == 0).all()
    assert all(len(q) == 0 for q in res.queues)
