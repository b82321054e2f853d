"""
The search beyond the near-solved table on the device (csrc/rubiks_near_reach.hip through NearTable.reach) against
tests/near_reach_model.py: distances, levels, lengths and every queue byte of whole searches, the best words and live bytes after
every single launch, and -- without the model -- two tables of different depth against each other on states whose distance the
deeper one knows, and two splits of K + J = 10 against each other on real scrambles.  Every comparison is of integers.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import near_model as nm  # noqa: E402
import near_reach_model as rm  # noqa: E402
from keys_model import pack_keys  # noqa: E402
from oracle import cube as oc  # noqa: E402


@pytest.fixture(scope="module")
def m5():
    return nm.NearModel(5)


@pytest.fixture(scope="module")
def level6(m5):
    return m5.next_level()


@pytest.fixture(scope="module")
def reach5(m5):
    return rm.ReachModel(m5)


@pytest.fixture(scope="module")
def inputs(m5, level6):
    """The solved state, all 126 states of depths 1-2, 256 sampled nodes of depths 3-5 and 64 states of depth 6."""
    rng, lo = np.random.RandomState(1), np.cumsum([0] + list(m5.counts))
    pick = np.concatenate([np.sort(rng.choice(np.arange(lo[d], lo[d + 1]), k, replace=False)) for d, k in ((3, 32), (4, 96), (5, 128))])
    states = np.concatenate([m5.states[:127], m5.states[pick], level6[:64]]).astype(np.int8)
    assert len(states) == 447 and set(m5.node_depth[pick]) == {3, 4, 5}
    return states


@pytest.fixture(scope="module")
def input_depths(m5, inputs):
    return np.concatenate([m5.depths(inputs[:-64]), np.full(64, 6)]).astype(int)


@pytest.fixture(scope="module")
def tables():
    from librubiks.solving.near import NearTable
    return {K: NearTable(K) for K in (1, 2, 3, 4, 5)}


@pytest.fixture(scope="module")
def table6():
    from librubiks.solving.near import NearTable
    return NearTable.get(6)


def _same(got, want, what=""):
    dist, levels, lengths, queues = want
    assert got.distances.dtype == np.int8 and got.levels.dtype == np.int8 and got.lengths.dtype == np.int32
    assert np.array_equal(got.distances, dist) and np.array_equal(got.levels, levels) and np.array_equal(got.lengths, lengths), what
    assert [list(q) for q in got.queues] == queues, what


@pytest.mark.parametrize("K", [1, 2, 3])
def test_reach_equals_the_model(reach5, inputs, input_depths, tables, K):
    for J in (0, 1, 2, 3):
        want = reach5.reach(inputs, J, depth=K)
        got = tables[K].reach(inputs, extra=J)
        _same(got, want, f"K {K}, J {J}")
        assert got.seconds > 0 and (got.items > 0) == (J > 0)
    assert np.array_equal(want[0], np.where(input_depths <= K + 3, input_depths, -1))
    assert set(want[1]) >= {0, 1, 2, 3}                                                       # the states end at different levels
    for n in (1, 63, 64, 65):
        _same(tables[K].reach(inputs[-n:], extra=3), tuple(w[-n:] for w in want), f"K {K}, the last {n}")
        _same(tables[K].reach(inputs[100:100 + n], extra=3), tuple(w[100:100 + n] for w in want), f"K {K}, {n} from 100")
    twice = np.array([5, 5, 200, 440, 200, 5, 0, 440, 0])
    _same(tables[K].reach(inputs[twice], extra=3), tuple([w[i] for i in twice] if isinstance(w, list) else w[twice] for w in want), "duplicates")


def test_no_extra_moves_is_depths_and_solve(inputs, tables):
    for K in (2, 5):
        got = tables[K].reach(inputs, extra=0)
        queues, lengths = tables[K].solve(inputs)
        assert np.array_equal(got.distances, tables[K].depths(inputs)) and np.array_equal(got.lengths, lengths) and got.items == 0
        assert [list(q) for q in got.queues] == [list(q) for q in queues] and np.array_equal(got.levels, np.where(lengths >= 0, 0, -1))


@pytest.mark.parametrize("P,per", [(2, 1), (2, 7), (2, 145), (1, 13), (0, 3)])
def test_every_launch_equals_the_model(m5, level6, reach5, tables, P, per):
    """begin / level / finish by hand through the struct: best words, live bytes and the count the host reads, after every call."""
    from librubiks.solving.near import ReachBatch
    K, J = 2, 3
    states = np.concatenate([m5.states[[0, 7, 300, 2000, 40000]], level6[:1]]).astype(np.int8)
    assert list(m5.node_depth[[0, 7, 300, 2000, 40000]]) == [0, 1, 3, 4, 5]
    model = rm.Launches(reach5, states, P, depth=K)
    batch = ReachBatch(tables[K], states, J, prefix=P)

    def same(what):
        assert np.array_equal(batch.words(), model.best), what
        assert np.array_equal(batch.live.cpu().numpy(), model.live) and batch.unresolved() == model.unresolved(), what
    model.begin()
    batch.begin()
    same("begin")
    for level in range(1, J + 1):
        assert batch.items(level) == model.items(level)
        for first in range(0, model.items(level), per):
            count = min(per, model.items(level) - first)
            model.level(level, first, count)
            batch.level(level, first, count)
            same(f"level {level}, items {first} .. {first + count - 1}")
    batch.finish()
    assert batch.status.tolist() == [0, 1]                                                    # the depth-6 state is beyond 2 + 3
    want = reach5.reach(states, J, depth=K)
    assert np.array_equal(batch.dist_out.cpu().numpy(), want[0]) and np.array_equal(batch.level_out.cpu().numpy(), want[1])
    assert batch.dist_out.tolist() == [0, 1, 3, 4, 5, -1]
    rows = batch.out_queues.cpu().numpy()
    assert [list(rows[i, :max(want[0][i], 0)]) for i in range(len(states))] == want[3]


def test_two_tables_agree(table6, tables):
    """No model: what the depth-6 table knows of its own nodes, the depth-4 table finds with two more moves."""
    keys, depth, _ = table6.nodes()
    rng = np.random.RandomState(5)
    lo5, lo6 = int(table6.counts[:5].sum()), int(table6.counts[:6].sum())
    pick = np.concatenate([rng.choice(np.arange(lo5, lo6), 512, replace=False), rng.choice(np.arange(lo6, table6.n_nodes), 512, replace=False),
                           rng.choice(table6.n_nodes, 3072, replace=False)])
    states = rm.unpack_keys(keys[pick])
    assert np.array_equal(pack_keys(states), keys[pick]) and (depth[pick] == 5).sum() >= 512 and (depth[pick] == 6).sum() >= 512
    own = table6.depths(states)
    assert np.array_equal(own, depth[pick])
    got = tables[4].reach(states, extra=2)
    assert np.array_equal(got.distances, own) and np.array_equal(got.levels, np.maximum(own.astype(int) - 4, 0))
    assert all(oc.is_solved(nm.replay(s, q)) and len(q) == d for s, q, d in zip(states[:600], got.queues[:600], own[:600]))
    # children of depth-6 nodes that the depth-6 table does not hold are 7 moves away
    deep = states[own == 6][:64]
    kids = oc.expand12(deep)
    kids = kids[table6.depths(kids) == -1][:256]
    assert len(kids) == 256
    assert (tables[4].reach(kids, extra=2).distances == -1).all()
    far = tables[4].reach(kids, extra=3)
    assert (far.distances == 7).all() and (far.levels == 3).all() and (far.lengths == 7).all()
    assert all(oc.is_solved(nm.replay(s, q)) and len(q) == 7 for s, q in zip(kids, far.queues))


def test_two_splits_agree_on_scrambles(table6, tables):
    np.random.seed(10)
    states = np.array([oc.scramble(10, True)[0] for _ in range(64)])
    a, b = table6.reach(states, extra=4), tables[5].reach(states, extra=5)
    D = a.distances.astype(int)
    assert np.array_equal(a.distances, b.distances) and (D >= 0).all() and (D <= 10).all() and (D % 2 == 0).all() and (D > 6).sum() > 10
    assert np.array_equal(a.levels, np.maximum(D - 6, 0)) and np.array_equal(b.levels, np.maximum(D - 5, 0))
    assert (b.levels[D >= 6] == a.levels[D >= 6] + 1).all()
    for r in (a, b):
        assert np.array_equal(r.lengths, D)
        assert all(len(q) == d and oc.is_solved(nm.replay(s, q)) for s, q, d in zip(states, r.queues, D))


def test_result_depends_on_neither_ranges_nor_prefix(inputs, tables):
    from librubiks.cube.device import DeviceCubes
    from librubiks.solving.near import ReachResult
    table = tables[2]
    whole = table.reach(inputs, extra=3)
    assert isinstance(whole, ReachResult) and whole.items == 447 * (12 + 144 + 1728)          # n = 447: P = 3 by default
    want = (whole.distances, whole.levels, whole.lengths, [list(q) for q in whole.queues])
    for launch_items, P in [(1000, None), (77777, None), (12 ** 3 + 1, 1), (5000, 4), (None, 0)]:
        timings = {}
        got = table.reach(inputs, extra=3, launch_items=launch_items, prefix=P, timings=timings)
        _same(got, want, f"launch_items {launch_items}, prefix {P}")
        assert sorted(timings) == [1, 2, 3] and sum(len(v) for v in timings.values()) >= 3
        if launch_items:
            assert len(timings[3]) == -(-447 * 12 ** min(3, 3 if P is None else P) // launch_items)
    # n = 0, and a batch that is a part of wider planes
    none = table.reach(np.zeros((0, 20), dtype=np.int8), extra=3)
    assert len(none.distances) == len(none.queues) == len(none.lengths) == len(none.levels) == 0 and none.items == 0
    wide = DeviceCubes.from_numpy(inputs)
    assert wide.stride == 512
    part = DeviceCubes(wide.soa, 65)
    _same(table.reach(part, extra=3), tuple(w[:65] for w in want), "65 of 447 columns")
    _same(table.reach(wide, extra=3), want, "DeviceCubes")


def test_arguments_are_checked(inputs, tables):
    from librubiks import _hip
    from librubiks.solving.near import MAX_EXTRA, ReachBatch
    table = tables[2]
    for kwargs in ({"extra": -1}, {"extra": MAX_EXTRA + 1}, {"extra": 2, "launch_items": 0}, {"extra": 2, "launch_items": -5},
                   {"extra": 2, "prefix": MAX_EXTRA + 1}, {"extra": 2, "prefix": -1}):
        with pytest.raises(ValueError):
            table.reach(inputs[:4], **kwargs)
    narrow = ReachBatch(table, inputs[:4], 2, out_width=3)                                    # K + J = 4
    narrow.begin()
    narrow.level(1, 0, narrow.items(1))
    with pytest.raises(_hip.RubiksHipError):
        narrow.finish()
    with pytest.raises(_hip.RubiksHipError):
        narrow.level(3, 0, 1)                                                                # beyond extra
    with pytest.raises(_hip.RubiksHipError):
        narrow.level(2, narrow.items(2) - 1, 2)                                              # beyond the level's items
    with pytest.raises(_hip.RubiksHipError):
        narrow.level(2, 0, 0)


def test_batch_result_excess(standin_net, tables):
    from librubiks.solving.agents import MCTS
    from librubiks.solving.results import BatchResult, QueueTable
    agent = MCTS(standin_net.cuda(), c=0.6, search_graph=False, net_dtype=torch.float32)
    np.random.seed(31)                                                                        # test_near_gpu.py's shallow games
    states = np.array([oc.scramble(1 + i % 5, True)[0] for i in range(40)])
    states[3] = oc.get_solved()
    raw = agent.search_batch(states, None, 300)
    won = np.asarray(raw.solved, dtype=bool)
    assert 5 <= won.sum() < 40
    excess = raw.excess(tables[3], states, extra=2)
    exact = tables[5].depths(states).astype(np.int32)
    assert excess.dtype == np.int32 and (exact >= 0).all()
    assert np.array_equal(excess, np.where(won, raw.lengths - exact, -1)) and (excess[won] >= 0).all()
    assert (raw.excess(tables[3], states, extra=0)[won & (exact > 3)] == -1).all()            # beyond K + J
    best = raw.shortened(states).tightened(tables[5]).excess(tables[3], states, extra=2)
    assert (best[won] <= excess[won]).all() and (best[won] >= 0).all() and (best[~won] == -1).all()
    mask = np.arange(40) % 3 != 0
    assert np.array_equal(raw.select(mask).excess(tables[3], states[mask], extra=2), excess[mask])
    # the table's own solutions are optimal
    queues, lengths = tables[5].solve(states)
    n = len(states)
    own = BatchResult(lengths >= 0, lengths.astype(np.int64), np.zeros(n, dtype=np.int64), queues, 0.0, np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64))
    assert isinstance(queues, QueueTable) and (own.excess(tables[2], states, extra=3) == 0).all()
    # ... and a detour of 2 (g % 3) moves in front of them is that much excess (the search above solves its games optimally)
    detours = QueueTable.from_queues([[nm.R_, nm.r_] * (g % 3) + list(queues[g]) for g in range(n)])
    longer = BatchResult(lengths >= 0, detours.lengths().copy(), own.nodes, detours, 0.0, own.iterations, own.status)
    assert np.array_equal(longer.excess(tables[2], states, extra=3), 2 * (np.arange(n) % 3))
