"""
The near-solved table on the device (csrc/rubiks_near.hip through librubiks/solving/near.py) against tests/near_model.py: the build
node for node and whatever the chunking, `depths` and `solve` state for state (and `solve` against the device BFS, which shares
nothing with the table but the move kernels), `tighten` queue for queue and status for status, and `BatchResult.tightened` on a
small real search.  Every comparison is of integers.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import near_model as nm  # noqa: E402
from conftest import GOLDEN  # noqa: E402
from keys_model import pack_keys  # noqa: E402
from oracle import cube as oc  # noqa: E402


@pytest.fixture(scope="module")
def m5():
    return nm.NearModel(5)


@pytest.fixture(scope="module")
def level6(m5):
    return m5.next_level()


@pytest.fixture(scope="module")
def tables():
    from librubiks.solving.near import NearTable
    return {K: NearTable(K) for K in (1, 3, 5)}


@pytest.fixture(scope="module")
def queue_sets():
    mcts, egvm = nm.fixture_queues(GOLDEN)
    return mcts + egvm, nm.detour_queues(256)


def _same_nodes(table, model, n):
    keys, depth, action = table.nodes()
    assert table.n_nodes == n and np.array_equal(keys, pack_keys(model.states[:n].astype(np.int8)))
    assert np.array_equal(depth, model.node_depth[:n]) and np.array_equal(action, model.node_action[:n])


@pytest.mark.parametrize("K", [1, 2, 3, 5])
def test_build_equals_the_model_node_for_node(m5, K):
    from librubiks.solving.near import NearTable
    table = NearTable(K)
    n = sum(m5.counts[:K + 1])
    assert list(table.counts) == m5.counts[:K + 1] and table.bytes == 17 * n + 4 * len(table.hash)
    _same_nodes(table, m5, n)
    cells = table.hash.cpu().numpy()
    filled = np.flatnonzero(cells)
    assert len(cells) >= 2 * n and np.array_equal(np.sort(cells[filled]), np.arange(1, n + 1))   # every node in one cell


def test_build_does_not_depend_on_the_chunking(m5, tables):
    from librubiks.solving.near import NearTable
    whole = tables[5].nodes()
    _same_nodes(tables[5], m5, m5.n_nodes)
    for rows in (64, 12 * 1000 + 7):
        got = NearTable(5, chunk_rows=rows).nodes()
        assert all(np.array_equal(a, b) for a, b in zip(got, whole)), f"chunk_rows {rows}"


def test_depth_six_counts(m5, level6):
    from librubiks.solving.near import NearTable
    table = NearTable.get(6)
    assert list(table.counts) == m5.counts + [len(level6)] and table.n_nodes == 983926 == int(table.counts.sum())
    assert NearTable.get(6) is table and NearTable.DEFAULT_DEPTH == 6


def test_depths_equal_the_model(m5, level6, tables):
    from librubiks import cube
    from librubiks.cube.device import DeviceCubes
    t5, t3 = tables[5], tables[3]
    d, nodes = t5.depths(m5.states.astype(np.int8), with_nodes=True)
    assert d.dtype == np.int8 and np.array_equal(d, m5.node_depth) and np.array_equal(nodes, np.arange(m5.n_nodes))
    assert np.array_equal(t3.depths(m5.states[:20000].astype(np.int8)), m5.depths(m5.states[:20000], depth=3))
    far = level6[np.random.RandomState(0).choice(len(level6), 5000, replace=False)].astype(np.int8)
    d, nodes = t5.depths(far, with_nodes=True)
    assert (d == -1).all() and (nodes == -1).all()
    np.random.seed(6)
    deep = cube.scramble_batch(4096, 20, True)[0]
    want = m5.depths(deep.numpy())
    assert np.array_equal(t5.depths(deep), want)
    mixed = np.concatenate([m5.states[::26].astype(np.int8), far])[:4097]
    want = m5.depths(mixed)
    assert (want >= 0).sum() > 4000 and (want < 0).sum() > 50
    for n in (1, 63, 64, 65, 4097):
        assert np.array_equal(t5.depths(mixed[-n:]), want[-n:]), n
        assert np.array_equal(t5.depths(DeviceCubes.from_numpy(mixed[:n])), want[:n]), n


def test_solve_is_optimal_and_agrees_with_the_device_bfs(m5, tables):
    from librubiks import cube
    from librubiks.solving.agents import BFS
    np.random.seed(12)
    states = np.concatenate([cube.scramble_batch(100, depth, True)[0].numpy() for depth in (1, 2, 3, 4, 5)])
    queues, lens = tables[5].solve(states)
    want_q, want_l = m5.solve(states)
    assert np.array_equal(lens, want_l) and (lens >= 1).all() and (lens <= 5).all() and (lens == 5).sum() > 20
    assert [list(q) for q in queues] == want_q
    ends = np.array([nm.replay(s, q) for s, q in zip(states, queues)])
    assert cube.multi_is_solved(ends).all()
    bfs = BFS().search_batch(states, None, 200_000, slots=64)
    assert bfs.solved.all() and np.array_equal(bfs.lengths, lens)
    # a shallower table says -1 exactly where the state lies beyond it, and its solutions are the deeper table's
    q3, l3 = tables[3].solve(states)
    assert np.array_equal(l3, np.where(lens <= 3, lens, -1))
    assert all(list(q3[g]) == (want_q[g] if lens[g] <= 3 else []) for g in range(len(states)))


@pytest.mark.parametrize("K", [1, 3, 5])
def test_tighten_equals_the_model(m5, tables, queue_sets, K):
    fixture, made = queue_sets
    shorter = 0
    for queues in (fixture, made):
        for W in (1, 2, 7, None):
            want, want_status = m5.tighten(queues, window=W, depth=K)
            got, status = tables[K].tighten(queues, window=W)
            assert np.array_equal(status, want_status) and (status == nm.OK).all()
            assert [list(q) for q in got] == want, f"K {K}, window {W}"
            shorter += sum(len(w) < len(q) for w, q in zip(want, queues))
    assert shorter > 100                                                           # the case cannot pass by doing nothing
    assert {0, 1, 2, 63, 64, 65, 300} <= {len(q) for q in made}


def test_tighten_selection_bad_bytes_and_chunks(m5, tables, queue_sets):
    from librubiks.solving.near import BAD_ACTION, OK, SKIPPED, plan_tighten_chunks
    _, made = queue_sets
    queues = [list(q) for q in made[:40]]
    lens = np.array([len(q) for q in queues])
    padded = np.full((40, 320), 0, dtype=np.uint8)
    for g, q in enumerate(queues):
        padded[g, :len(q)] = q
    g_bad, g_beyond = int(np.flatnonzero(lens > 20)[0]), int(np.flatnonzero(lens > 20)[1])
    padded[g_bad, 9] = 12                                                          # inside the length
    padded[g_beyond, lens[g_beyond]] = 200                                         # beyond it: not the game's
    select = np.ones(40, dtype=bool)
    select[[5, 8, 17, 39]] = False
    want, _ = m5.tighten(queues)
    got, status = tables[5].tighten(padded, lengths=lens, select=select)
    for g in range(40):
        if not select[g]:
            assert status[g] == SKIPPED and list(got[g]) == queues[g]
        elif g == g_bad:
            assert status[g] == BAD_ACTION and list(got[g]) == [int(a) for a in padded[g, :lens[g]]]
        else:
            assert status[g] == OK and list(got[g]) == want[g], g
    # one game a chunk (queues of 90 .. 120 moves: no two of them fit the workspace of the longest): the same rows
    from librubiks.solving.near import band_bytes, workspace_bytes
    alike = [q for q in made if 90 <= len(q) <= 120]
    lens = np.array([len(q) for q in alike])
    budget = workspace_bytes(int(band_bytes(lens).max()), int(lens.max()) + 1)
    assert len(alike) >= 20 and plan_tighten_chunks(lens, None, budget) == [(g, g + 1) for g in range(len(alike))]
    info = {}
    whole, _ = tables[5].tighten(alike, info=info)
    assert info["chunks"] == 1
    cut, cut_status = tables[5].tighten(alike, budget_bytes=budget, info=info)
    assert info["chunks"] == len(alike) and (cut_status == OK).all()
    assert [list(q) for q in cut] == [list(q) for q in whole] == m5.tighten(alike)[0]


def test_a_narrow_output_row_reports_no_room(m5, tables):
    from librubiks.solving.near import NO_ROOM, OK, TightenBatch
    R, r, T, F = nm.R_, nm.r_, nm.T_, nm.F_
    queues = [[R, r, T, F, T, F, R], [R, r], [T, F, R, R, R]]                      # results of 5, 0 and 3 moves
    padded = np.zeros((3, 8), dtype=np.uint8)
    for g, q in enumerate(queues):
        padded[g, :len(q)] = q
    batch = TightenBatch(tables[5], padded, [7, 2, 5], [1, 1, 1], out_width=4)
    batch.out_queues.fill_(99)
    batch.run()
    assert batch.status.tolist() == [NO_ROOM, OK, OK] and batch.out_lens.tolist() == [5, 0, 3] == [len(m5.tighten_one(q)) for q in queues]
    rows = batch.out_queues.cpu().numpy()
    assert (rows[0] == 99).all() and (rows[1] == 99).all() and list(rows[2]) == m5.tighten_one(queues[2]) + [99]


def _check_tightened(states, raw, tight, table_model):
    won = np.flatnonzero(raw.solved)
    assert tight.tighten_seconds > 0 and np.array_equal(tight.raw_lengths, raw.lengths) and raw.raw_lengths is None and raw.tighten_seconds is None
    want, _ = table_model.tighten([list(raw.queues[g]) for g in won])
    for i, g in enumerate(won):
        assert list(tight.queues[g]) == want[i] and tight.lengths[g] == len(want[i]) <= raw.lengths[g]
        assert oc.is_solved(nm.replay(states[g], tight.queues[g]))
    for g in np.flatnonzero(~raw.solved):
        assert list(tight.queues[g]) == list(raw.queues[g]) and tight.lengths[g] == raw.lengths[g]
    assert np.array_equal(tight.solved, raw.solved) and np.array_equal(tight.nodes, raw.nodes) and tight.seconds == raw.seconds
    return int((tight.lengths[won] < raw.lengths[won]).sum())


def test_batch_result_tightened_on_a_real_search(standin_net, tables, m5):
    from librubiks.solving.agents import MCTS
    net = standin_net.cuda()
    agent = MCTS(net, c=0.6, search_graph=False, net_dtype=torch.float32)
    # 32 depth-8 games: the stand-in net solves few of them (one, in the oracle's run of these inputs), the rest must stay as they are
    np.random.seed(41)
    deep = np.array([oc.scramble(8, True)[0] for _ in range(32)])
    raw = agent.search_batch(deep, None, 2000)
    assert 1 <= raw.solved.sum() < 32
    tight = raw.tightened(tables[5])
    assert tight.shorten_seconds is None
    _check_tightened(deep, raw, tight, m5)
    # ... and the shallow games the shorten tests use, of which it solves enough to have queues that get shorter
    np.random.seed(31)
    states = np.array([oc.scramble(1 + i % 5, True)[0] for i in range(40)])
    states[3] = oc.get_solved()
    raw = agent.search_batch(states, None, 300)
    won = np.flatnonzero(raw.solved)
    assert len(won) >= 5
    shrunk = _check_tightened(states, raw, raw.tightened(tables[5]), m5)
    print(f"{len(won)} solved, {shrunk} got shorter")
    short = raw.shortened(states)
    both = short.tightened(tables[5], window=16)
    assert np.array_equal(both.raw_lengths, raw.lengths) and both.shorten_seconds == short.shorten_seconds > 0 and both.tighten_seconds > 0
    assert (both.lengths[won] <= short.lengths[won]).all() and (short.lengths[won] <= raw.lengths[won]).all()
    assert all(oc.is_solved(nm.replay(states[g], both.queues[g])) for g in won)
    assert all(list(both.queues[g]) == list(raw.queues[g]) for g in np.flatnonzero(~raw.solved))
