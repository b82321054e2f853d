"""
tests/shorten_model.py -- the NumPy model the rc_shorten_* kernels are compared with -- pinned to the oracle: for every case an
oracle.agents.MCTS is filled by hand with the distinct states of the path (`indices`, `states`, zeroed `neighbors`, every node a
leaf), its own `_complete_graph` and `_shorten_action_queue(target)` run, and the model's queue must be the oracle's.  Every
result is replayed to its end state.  The oracle's nodes are numbered densely here and by first position in the model: the queue
must not depend on that.
"""
from collections import deque

import numpy as np
import pytest

import conftest  # noqa: F401
import shorten_model as sm
from oracle import agents as oa
from oracle import cube as oc


def oracle_shorten(root: np.ndarray, queue) -> list:
    states = [np.asarray(root, dtype=np.int8)]
    for a in queue:
        states.append(oc.rotate(states[-1], *oc.ACTION_SPACE[int(a)]))
    m = oa.MCTS(None, 0.6, True)
    m.action_queue = deque()
    m.indices = {}
    for s in states:
        m.indices.setdefault(s.tobytes(), len(m.indices) + 1)
    n = len(m.indices)
    m.states = np.empty((n + 1, 20), dtype=np.int8)
    for key, i in m.indices.items():
        m.states[i] = np.frombuffer(key, dtype=np.int8)
    m.neighbors = np.zeros((n + 1, 12), dtype=int)
    m.leaves = np.ones(n + 1, dtype=bool)
    m._complete_graph()
    m._shorten_action_queue(m.indices[states[-1].tobytes()])
    return [int(a) for a in m.action_queue]


def check(root, queue):
    b = sm.shorten([root], [queue])
    assert b.status[0] == sm.OK
    got = b.result(0)
    assert got == oracle_shorten(root, queue)
    assert len(got) <= len(queue)
    assert np.array_equal(sm.replay(root, got), sm.replay(root, queue))
    return got, b.counts[0]


def test_small_cases():
    want = {"empty": 0, "one move": 1, "there and back": 0, "one move four times": 0, "commuting shortcut": 1, "two routes, FIFO decides": 2}
    for name, root, queue in sm.small_cases():
        got, counts = check(root, queue)
        assert len(got) == want[name], name
        if name in ("empty", "there and back", "one move four times"):
            assert counts.get("target_is_root") == 1
    _, root, queue = sm.small_cases()[4]
    assert check(root, queue)[0] == [sm.B]                     # an edge the queue itself never took
    _, root, queue = sm.small_cases()[5]
    assert check(root, queue)[0] == [sm.F, sm.B]               # F B and B F both lead there: the scan order 0 .. 11 picks F first


def test_euler_tours_of_the_balls():
    for (name, root, queue), depth, moves, states in zip(sm.ball_cases(), (2, 3), (290, 3195), (127, 1195)):
        assert len(queue) == moves
        got, counts = check(root, queue)
        assert counts["nodes"] == states and len(got) == depth, name
    assert counts["passes"] >= 1 + 1 + 6                        # level 2 of the depth-3 ball: 114 nodes, 1 368 scan items, 6 passes of 256
    assert counts["claims_lost"] > 0 and counts["visited_skipped"] > 0


def test_random_walks_with_back_tracks():
    for name, root, queue in sm.walk_cases():
        got, counts = check(root, queue)
        assert counts["revisits"] > 0 and len(got) < len(queue), name


def test_oracle_egvm_games_of_the_main_set(standin_net):
    from test_egvm_batch_gpu import MAIN, inputs, oracle_games
    seed, n, depth_of, solved_at, eps, W, D, cap, _ = MAIN
    states, seeds = inputs(seed, n, depth_of, solved_at)
    games = oracle_games(oa.TorchNet(standin_net, device="cpu"), states, seeds, eps, W, D, cap)
    solved = [g for g in range(n) if games[g][0]]
    assert len(solved) == 29
    shrunk = []
    for g in solved:
        got, _ = check(states[g], games[g][2])
        assert np.array_equal(sm.replay(states[g], got), oc.get_solved())
        if len(got) < len(games[g][2]):
            shrunk.append((len(games[g][2]), len(got)))
    assert sorted(shrunk) == sorted([(5, 3), (5, 1), (11, 1), (15, 1), (4, 2), (6, 2)])


def test_statuses_and_batches():
    root = sm.scrambled(3)
    b = sm.Batch([root] * 4, [[0, 2], [0, 12, 2], [0, 1], [4, 6, 8]], select=[1, 1, 0, 1], out_width=2)
    sm.index(b), sm.neighbours(b), sm.bfs(b)
    assert list(b.status) == [sm.OK, sm.BAD_ACTION, sm.SKIPPED, sm.NO_ROOM]
    assert list(b.out_lens) == [2, -1, -1, 3] and b.result(0) == [0, 2]
    assert sm.workspace_bytes(1000, 4096) == 16128 + 4096 + 48128 + 8192 + 2 * 4096 + 16384
    assert [sm.table_cells(L) for L in (0, 1, 2, 3, 4, 1023, 1024)] == [2, 4, 8, 8, 16, 2048, 4096]
