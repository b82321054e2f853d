"""
Queue shortening from the public interface: `shorten_queues` equals tests/shorten_model.py on random games, gives the same bytes
however the batch is cut into chunks, and every result replays to its queue's end state; `shorten=True` on EGVM (batched, on 16
slots, and game by game through `search`), on the sampled policy and on RandomSearch returns, for every solved game, the model's
shortening of the queue the search returns without the flag and leaves everything else of the result as it is; and
`BatchResult.shortened` does the same to a result of MCTS(search_graph=False).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import shorten_model as sm  # noqa: E402
from oracle import agents as oa  # noqa: E402
from oracle import cube as oc  # noqa: E402
from test_egvm_batch_gpu import MAIN, inputs, oracle_games  # noqa: E402


@pytest.fixture(scope="module")
def net_gpu(standin_net):
    return standin_net.cuda()


@pytest.fixture(scope="module")
def random_games():
    """200 games: walks of 0 .. 150 moves with back-tracks from scrambled roots, and what the model makes of them."""
    rng = np.random.RandomState(2)
    roots = np.array([sm.scrambled(1000 + g, int(rng.randint(0, 25))) for g in range(200)])
    queues = [sm.random_walk(g, int(rng.randint(0, 151)), back_prob=float(rng.choice([0.0, 0.2, 0.5]))) for g in range(200)]
    model = sm.shorten(roots, queues)
    assert (model.status == sm.OK).all()
    return roots, queues, model


def _rows(table):
    return [list(q) for q in table]


def test_shorten_queues_equals_the_model_whatever_the_chunks(random_games):
    from librubiks.cube.device import DeviceCubes
    from librubiks.solving.shorten import OK, plan_chunks, shorten_queues
    roots, queues, model = random_games
    want = [model.result(g) for g in range(200)]
    info = {}
    got, status = shorten_queues(roots, queues, info=info)
    assert (status == OK).all() and _rows(got) == want and info["chunks"] == 1
    assert sum(len(w) < len(q) for w, q in zip(want, queues)) > 50                     # the case cannot pass by doing nothing
    lens = np.array([len(q) for q in queues])
    assert (got.lengths() == [len(w) for w in want]).all() and (got.lengths() <= lens).all()

    budget = info["workspace_bytes"] // 5
    assert len(plan_chunks(lens, budget)) >= 4
    acts, _ = got.padded(fill=0)
    chunked, status = shorten_queues(DeviceCubes.from_numpy(roots), queues, budget_bytes=budget, info=info)
    assert (status == OK).all() and info["chunks"] >= 4
    assert np.array_equal(chunked.padded(fill=0)[0], acts) and (chunked.lengths() == got.lengths()).all()
    single = [list(shorten_queues(roots[g:g + 1], [queues[g]])[0][0]) for g in range(200)]
    assert single == want

    # every result ends where its queue ends: both replayed on the device, move by move (12 = the identity padding)
    def end_states(rows):
        cubes = DeviceCubes.from_numpy(roots)
        padded = np.full((256, max(1, max(len(r) for r in rows))), 12, dtype=np.uint8)
        for g, r in enumerate(rows):
            padded[g, :len(r)] = r
        steps = torch.from_numpy(padded).cuda()
        for i in range(padded.shape[1]):
            cubes = cubes.multi_rotate(steps[:, i].contiguous())
        return cubes.numpy()
    assert np.array_equal(end_states(want), end_states(queues))
    assert np.array_equal(end_states(_rows(got))[7], sm.replay(roots[7], queues[7]))


def test_selection_lengths_and_bad_actions(random_games):
    from librubiks.solving.shorten import BAD_ACTION, OK, SKIPPED, shorten_queues
    roots, queues, model = random_games
    n = 12
    padded = np.zeros((n, 160), dtype=np.uint8)
    lens = np.array([len(q) for q in queues[:n]])
    for g in range(n):
        padded[g, :lens[g]] = queues[g]
    g_bad = int(np.flatnonzero(lens > 3)[0])
    padded[g_bad, 2] = 12
    select = np.ones(n, dtype=bool)
    select[[1, 5]] = False
    got, status = shorten_queues(roots[:n], padded, lengths=lens, select=select)
    for g in range(n):
        if g in (1, 5):
            assert status[g] == SKIPPED and list(got[g]) == queues[g]
        elif g == g_bad:
            assert status[g] == BAD_ACTION and list(got[g]) == [int(a) for a in padded[g, :lens[g]]]
        else:
            assert status[g] == OK and list(got[g]) == model.result(g)


def _check_flag(states, raw, short, label):
    """`short` (shorten=True) against `raw` (the same search without the flag)."""
    assert np.array_equal(short.solved, raw.solved) and np.array_equal(short.nodes, raw.nodes) and np.array_equal(short.status, raw.status)
    assert np.array_equal(short.raw_lengths, raw.lengths) and raw.raw_lengths is None and short.shorten_seconds > 0
    won = [g for g in range(len(states)) if raw.solved[g]]
    assert won, f"{label}: the inputs solve nothing"
    model = sm.shorten(states[won], [list(raw.queues[g]) for g in won])
    shrunk = 0
    for i, g in enumerate(won):
        assert list(short.queues[g]) == model.result(i) and short.lengths[g] == len(model.result(i)), f"{label}: game {g}"
        assert np.array_equal(sm.replay(states[g], short.queues[g]), oc.get_solved())
        shrunk += short.lengths[g] < raw.lengths[g]
    for g in range(len(states)):
        if not raw.solved[g] or raw.lengths[g] == 0:                                   # unsolved and root-solved games: untouched
            assert list(short.queues[g]) == list(raw.queues[g]) and short.lengths[g] == raw.lengths[g]
    return shrunk


def test_egvm_under_the_flag_on_the_main_set(net_gpu):
    from librubiks.solving.agents import EGVM
    seed, n, depth_of, solved_at, eps, W, D, cap, _ = MAIN
    states, seeds = inputs(seed, n, depth_of, solved_at)
    want = oracle_games(oa.TorchNet(net_gpu, device="cuda"), states, seeds, eps, W, D, cap)
    won = [g for g in range(n) if want[g][0]]
    model = sm.shorten(states[won], [want[g][2] for g in won])
    expect = {g: model.result(i) for i, g in enumerate(won)}
    assert len(won) == 29 and sum(len(expect[g]) < len(want[g][2]) for g in won) == 6
    agent = lambda flag: EGVM(net_gpu, eps, W, D, net_dtype=torch.float32, shorten=flag)   # noqa: E731
    raw = agent(False).search_batch(states, None, cap, seeds=seeds)
    for kw in ({}, {"slots": 16}):
        short = agent(True).search_batch(states, None, cap, seeds=seeds, **kw)
        assert _check_flag(states, raw, short, f"EGVM {kw}") == 6
        for g in won:
            assert list(short.queues[g]) == expect[g]
    one = agent(True)
    for g in range(n):
        np.random.seed(int(seeds[g]))
        assert one.search(states[g], None, cap) == want[g][0] and len(one) == want[g][1]
        assert list(one.action_queue) == (expect[g] if want[g][0] else want[g][2]), f"search, game {g}"
    # the serial batch (global stream): one shortening of the assembled result
    np.random.seed(5)
    serial_raw = agent(False).search_batch(states[:12], None, cap)
    np.random.seed(5)
    serial = agent(True).search_batch(states[:12], None, cap)
    _check_flag(states[:12], serial_raw, serial, "EGVM serial")


def test_rollout_agents_under_the_flag(net_gpu):
    from librubiks.solving.agents import PolicySearch, RandomSearch
    np.random.seed(21)
    states = np.array([oc.scramble(1 + i % 4, True)[0] for i in range(64)])
    makers = {"sampled policy": lambda flag: PolicySearch(net_gpu, sample_policy=True, net_dtype=torch.float32, shorten=flag),
              "random": lambda flag: RandomSearch(shorten=flag)}
    for label, make in makers.items():
        raw = make(False).search_batch(states, None, 200, seeds=9)
        for kw in ({}, {"slots": 16}):
            short = make(True).search_batch(states, None, 200, seeds=9, **kw)
            # (with the stand-in net's arbitrary policy, and with random moves, few of these games are solved at all -- 1 and 2 --
            # and those in one move: the flag must then change nothing; queues that do get shorter are EGVM's and MCTS's above and below)
            shrunk = _check_flag(states, raw, short, f"{label} {kw}")
            print(f"{label} {kw}: {int(raw.solved.sum())} solved, {int(shrunk)} got shorter")
        np.random.seed(3)                                                              # the host-driven route and `search`
        a = make(False)
        ok_raw = a.search(states[0], None, 200)
        q_raw = list(a.action_queue)
        np.random.seed(3)
        b = make(True)
        assert b.search(states[0], None, 200) == ok_raw
        assert list(b.action_queue) == (sm.shorten(states[:1], [q_raw]).result(0) if ok_raw else q_raw)


def test_batch_result_shortened_on_a_tree_search_without_graph(net_gpu):
    from librubiks.solving.agents import MCTS
    np.random.seed(31)
    states = np.array([oc.scramble(1 + i % 5, True)[0] for i in range(40)])
    states[3] = oc.get_solved()
    raw = MCTS(net_gpu, c=0.6, search_graph=False, net_dtype=torch.float32).search_batch(states, None, 300)
    short = raw.shortened(states)
    assert raw.solved.sum() >= 5
    _check_flag(states, raw, short, "MCTS(search_graph=False)")
    assert short.seconds == raw.seconds and short.queues is not raw.queues and (short.lengths <= raw.lengths).all()
