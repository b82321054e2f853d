"""
A grid of (lambda, expansions) settings searched as one A* pool (`AStar.search_batch(..., lambda_=, expansions=)` with per-game
arrays, rc_astar_pop_expand_each / rc_astar_push_relax_each): game g ends exactly as game g of an agent built with its own
(lambda_[g], expansions[g]) -- against the oracle's single-problem runs on the plain fp32 engine, and against separate
`search_batch` calls with trained weights on the deterministic engine -- in whichever order the pool plants the games; and
`GridSearch` produces the same histories through the pool (`Evaluator.eval_sweep`) as through the reference's loop.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import ROOT  # noqa: E402
from oracle import agents as oa  # noqa: E402  (checker only)
from oracle import cube as oc  # noqa: E402

WEIGHTS = os.path.join(ROOT, "weights", "fc_small_r1")
GRID = [(lam, n_exp) for lam in (0.0, 0.2) for n_exp in (1, 5, 16)]
# max_states: at 200 and 400 every point of the grid has solved, exhausted and root-solved games (checked with the oracle on the CPU);
# at 100 a game with N 16 is exhausted at its first pop (1 + 12 * 16 > 100) while the others search on
CAPS = (100, 200, 400)


@pytest.fixture(scope="module")
def net_gpu(standin_net):
    return standin_net.cuda()


@pytest.fixture(scope="module")
def trained():
    from librubiks.model import Model
    return Model.load(WEIGHTS).cuda().eval()


def _easy_states(n=24, seed=21):
    """Depths 1-7, a solved root and duplicate scrambles (as tests/test_astar_pool_gpu.py)."""
    np.random.seed(seed)
    states = np.array([oc.scramble(1 + i % 7, True)[0] for i in range(n)])
    states[9] = oc.get_solved()
    states[20:24] = states[3:7]
    return states


@pytest.fixture(scope="module")
def oracle_runs(net_gpu):
    """cap -> per game of the pool (point-major): (solved, len(agent), queue) of the oracle's own search.  Computed once."""
    states, onet = _easy_states(), oa.TorchNet(net_gpu, device="cuda")
    runs = {}
    for cap in CAPS:
        runs[cap] = []
        for lam, n_exp in GRID:
            for s in states:
                r = oa.AStar(onet, lambda_=lam, expansions=n_exp)
                runs[cap].append((r.search(s, cap), len(r), list(r.action_queue)))
    return runs


@pytest.mark.parametrize("slots", [1, 7, None], ids=["slots_1", "slots_7", "slots_all"])
def test_pooled_grid_equals_the_oracle(net_gpu, oracle_runs, slots):
    from librubiks.solving import astar_device as ad
    from librubiks.solving.agents import AStar
    states = _easy_states()
    pool = np.tile(states, (len(GRID), 1))
    lam = np.repeat([g[0] for g in GRID], len(states))
    n_exp = np.repeat([g[1] for g in GRID], len(states))
    agent = AStar(net_gpu, lambda_=0.7, expansions=3, net_dtype=torch.float32)   # (its own values are used by no game)
    for cap in CAPS:
        res = agent.search_batch(pool, None, cap, slots=slots, lambda_=lam, expansions=n_exp)
        assert agent.batch.N == 16 and agent.batch.C >= 12 * 16 + 1
        for g, (ok, n, q) in enumerate(oracle_runs[cap]):
            assert (bool(res.solved[g]), int(res.nodes[g]), list(res.queues[g])) == (ok, n, q), f"cap {cap}, game {g} {GRID[g // len(states)]}"
            assert res.lengths[g] == (len(q) if ok else -1)
        status = res.status.reshape(len(GRID), len(states))
        if cap >= 200:
            for p in range(len(GRID)):
                assert {ad.SOLVED, ad.EXHAUSTED, ad.ROOT_SOLVED} <= set(status[p].tolist()), (cap, GRID[p])
        else:
            wide = np.flatnonzero(n_exp == 16)
            assert set(res.status[wide].tolist()) == {ad.EXHAUSTED, ad.ROOT_SOLVED} and (res.iterations[wide] == 0).all()
            assert (res.iterations[n_exp == 5] > 0).any() and ad.SOLVED in res.status[n_exp == 5]
    # game 0 stays inspectable, with game 0's lambda in `cost`
    alone = AStar(net_gpu, lambda_=GRID[0][0], expansions=GRID[0][1], net_dtype=torch.float32)
    alone.search(states[0], None, CAPS[-1])
    assert len(agent) == len(alone) and list(agent.action_queue) == list(alone.action_queue)
    for k in ("states", "G", "parents", "parent_actions"):
        assert np.array_equal(getattr(agent, k), getattr(alone, k)), k
    assert agent.open_queue == alone.open_queue
    idx = np.arange(1, len(alone) + 1)
    assert np.array_equal(agent.cost(alone.states[idx], idx), alone.cost(alone.states[idx], idx))


def _same(a, b, what):
    for k in ("solved", "status", "nodes", "iterations", "lengths"):
        assert np.array_equal(np.asarray(getattr(a, k)), np.asarray(getattr(b, k))), (what, k)
    assert all(list(a.queues[g]) == list(b.queues[g]) for g in range(len(a.solved))), what


def test_trained_pool_equals_separate_searches_in_either_planting_order(trained):
    from librubiks.solving.agents import AStar
    from librubiks.solving.results import BatchResult
    np.random.seed(29)
    states = np.array([oc.scramble(4 + i % 10, True)[0] for i in range(16)])   # depths 4-13: some games solve, some exhaust
    grid = [(lam, n_exp) for lam in (0.0, 0.1, 0.3) for n_exp in (1, 20, 50)]
    cap, G = 2500, len(states)
    parts = []
    for p, (lam, n_exp) in enumerate(grid):
        one = AStar(trained, lambda_=lam, expansions=n_exp, deterministic=True).search_batch(states, None, cap)
        parts.append((np.arange(p * G, (p + 1) * G), one))
    separate = BatchResult.merge(len(grid) * G, parts, 0.0)
    assert separate.solved.any()
    print("solved share", separate.solved.mean(), "statuses", np.bincount(separate.status))
    pool = np.tile(states, (len(grid), 1))
    lam = np.repeat([g[0] for g in grid], G)
    n_exp = np.repeat([g[1] for g in grid], G)
    assert (np.diff(n_exp) > 0).any() and (np.diff(n_exp) < 0).any()   # neither ascending nor descending: a reordering pool must map back
    for order in ("descending", "given"):
        agent = AStar(trained, lambda_=0.5, expansions=7, deterministic=True)
        agent.plant_order = order
        for slots in (40, None):
            got = agent.search_batch(pool, None, cap, slots=slots, lambda_=lam, expansions=n_exp)
            _same(got, separate, (order, slots))
            assert got.game_seconds.shape == (len(pool),) and (got.game_seconds > 0).all()
    # scalars broadcast: one lambda for every game, the agent's own expansions
    agent = AStar(trained, lambda_=0.5, expansions=20, deterministic=True)
    got = agent.search_batch(states, None, cap, slots=5, lambda_=0.1)
    _same(got, parts[4][1], "scalar lambda")


def test_grid_search_routes_produce_identical_histories(trained):
    from librubiks.solving.agents import AStar
    from librubiks.solving.evaluation import Evaluator
    from librubiks.solving.hyper_optim import GridSearch

    def prep(params):
        params["expansions"] = int(params["expansions"])
        return params
    out = {}
    for pooled in (True, False):
        np.random.seed(17)
        ev = Evaluator(12, [5, 11], None, 2000, slots=32)
        gs = GridSearch(None, {"lambda_": (0, 0.4), "expansions": (1, 40)}, pooled=pooled)
        gs.objective_from_evaluator(ev, AStar, {"net": trained, "deterministic": True}, param_prepper=prep, optim_lengths=True)
        assert gs.pooled_route_applies()
        best = gs.optimize(9)
        state = np.random.get_state()
        out[pooled] = (gs.score_history, gs.parameter_history, gs.optimal, gs.highscore, best, state[1].tolist(), state[2])
        assert len(ev.batch_seconds) == 1   # (the loop: the last point's pool; the sweep: the one pool)
    assert len(out[True][0]) == 9
    assert out[True] == out[False]
    assert [int(p["expansions"]) for p in out[True][1][:3]] == [1, 20, 40]


def test_eval_sweep_shapes_and_errors(trained):
    from librubiks.solving.agents import AStar, MCTS
    from librubiks.solving.evaluation import Evaluator
    agent = AStar(trained, lambda_=0.2, expansions=10, deterministic=True)
    np.random.seed(3)
    ev = Evaluator(5, [2, 4, 5], None, 1500, slots=8)
    res, states, times = ev.eval_sweep(agent, {"expansions": np.array([10, 3])})
    assert res.shape == states.shape == times.shape == (2, 3, 5) and (times > 0).all()
    np.random.seed(3)
    for p, n_exp in enumerate((10, 3)):
        r, s, _ = Evaluator(5, [2, 4, 5], None, 1500, slots=8).eval(AStar(trained, lambda_=0.2, expansions=n_exp, deterministic=True))
        assert np.array_equal(r, res[p]) and np.array_equal(s, states[p]), p
    with pytest.raises(ValueError, match="c"):
        ev.eval_sweep(agent, {"c": np.array([1.0])})
    with pytest.raises(ValueError):
        ev.eval_sweep(agent, {"lambda_": np.array([0.1, 0.2]), "expansions": np.array([1])})
    with pytest.raises(ValueError):
        ev.eval_sweep(MCTS(trained, c=0.6, search_graph=True), {"c": np.array([0.5])})
