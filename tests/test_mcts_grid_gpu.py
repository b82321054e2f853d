"""
A grid over the exploration constant c searched as one MCTS pool (`MCTS.search_batch(..., c=)` with a per-game array, the
rc_mcts_*_each entry points reading `MCTSForest.c_slot` by tree index): game g ends exactly as game g of an agent built with
c[g] -- against the oracle's single-tree runs on the plain fp32 engine, node for node where trees are compared, in every form and
launch shape of the tree kernel, and against separate `search_batch` calls with trained weights on the deterministic engine --
and `GridSearch` produces the same histories through the pool (`Evaluator.eval_sweep`) as through the reference's loop.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import ROOT  # noqa: E402
from mcts_lockstep import compare_tree, oracle_arrays  # noqa: E402
from oracle import agents as oa  # noqa: E402  (checker only)
from oracle import cube as oc  # noqa: E402

WEIGHTS = os.path.join(ROOT, "weights", "fc_small_r1")
C_GRID = (0.1, 0.6, 4.0, 100.0)
# With the oracle on the CPU: under every c and cap there are solved, exhausted and root-solved games; every pair of c values differs
# in (solved, nodes, queue) on at least 2 of the 24 games (0.1 against 0.6 at cap 100: games 13 and 18; every other pair: 6 and more);
# the longest descent is 42 levels (c 0.1, cap 400).
CAPS = (100, 200, 400)
OWN_C = 7.7            # the agents' own c: used by no game
TREE_GAMES = (2, 13, 18)
ITERS = 30
C_EIGHT = (0.1, 4.0, 1.0, 20.0, 0.6, 2.0, 100.0, 10.0)


@pytest.fixture(scope="module")
def net_gpu(standin_net):
    return standin_net.cuda()


@pytest.fixture(scope="module")
def trained():
    from librubiks.model import Model
    return Model.load(WEIGHTS).cuda().eval()


def _easy_states(n=24, seed=21):
    """The states of tests/test_astar_grid_gpu.py: depths 1-7, a solved root and duplicate scrambles."""
    np.random.seed(seed)
    states = np.array([oc.scramble(1 + i % 7, True)[0] for i in range(n)])
    states[9] = oc.get_solved()
    states[20:24] = states[3:7]
    return states


def _pool():
    """The 4 x 24 games, c-major, and every game's c."""
    states = _easy_states()
    return np.tile(states, (len(C_GRID), 1)), np.repeat(C_GRID, len(states))


def _outcome(ref, ok):
    return bool(ok), len(ref), int(getattr(ref, "iterations", 0)), list(ref.action_queue)   # (a solved root: the loop never ran)


@pytest.fixture(scope="module")
def oracle_runs(net_gpu):
    """(search_graph, cap) -> per game of the pool: (solved, len(agent), iterations, queue) of the oracle's own search; and
    (c index, game) -> the oracle agent of the naive search at the largest cap, for TREE_GAMES; and the levels of the longest descent
    of those searches.  Computed once."""
    states, onet = _easy_states(), oa.TorchNet(net_gpu, device="cuda")
    runs, agents, deepest = {}, {}, 0
    for graph in (False, True):
        for cap in CAPS:
            runs[graph, cap] = []
            for i, c in enumerate(C_GRID):
                for g, s in enumerate(states):
                    r = oa.MCTS(onet, c=c, search_graph=graph)
                    runs[graph, cap].append(_outcome(r, r.search(s, cap)))
                    if not graph and cap == CAPS[-1]:
                        deepest = max(deepest, r.deepest_path)
                        if g in TREE_GAMES:
                            agents[i, g] = r
    return runs, agents, deepest


def _check(res, expected, what):
    for g, (ok, n, its, q) in enumerate(expected):
        got = (bool(res.solved[g]), int(res.nodes[g]), int(res.iterations[g]), list(res.queues[g]))
        assert got == (ok, n, its, q), f"{what}, game {g}"
        assert res.lengths[g] == (len(q) if ok else -1)


@pytest.mark.parametrize("graph", [False, True], ids=["naive", "graph"])
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("slots", [1, 7, None], ids=["slots_1", "slots_7", "slots_all"])
def test_pooled_grid_equals_the_oracle(net_gpu, oracle_runs, slots, cap, graph):
    from librubiks.solving import mcts_device as md
    from librubiks.solving.agents import MCTS
    pool, c = _pool()
    order = np.arange(len(pool))
    if slots == 7:      # neighbouring slots hold different c, and a slot is planted again under another one
        order = np.random.RandomState(5).permutation(len(pool))
    assert len(set(c[order][:7])) > 1 or slots != 7
    agent = MCTS(net_gpu, c=OWN_C, search_graph=graph, net_dtype=torch.float32, sync_every=4)
    res = agent.search_batch(pool[order], None, cap, slots=slots, c=c[order])
    assert agent.forest.B == (slots or len(pool))
    _check(res, [oracle_runs[0][graph, cap][g] for g in order], (slots, cap, graph))
    for value in C_GRID:
        assert {md.SOLVED, md.EXHAUSTED, md.ROOT_SOLVED} <= set(res.status[c[order] == value].tolist()), value
    if slots is not None:
        assert agent.refill_stats["refills"] >= 2
    # game 0 stays inspectable through the reference's attributes, under game 0's c
    alone = MCTS(net_gpu, c=float(c[order][0]), search_graph=graph, net_dtype=torch.float32)
    alone.search(pool[order][0], None, cap)
    assert len(agent) == len(alone) and list(agent.action_queue) == list(alone.action_queue)
    for k in ("states", "neighbors", "leaves", "N", "W", "P", "V", "L"):
        assert np.array_equal(getattr(agent, k)[1:len(alone) + 1], getattr(alone, k)[1:len(alone) + 1]), k


def test_trees_are_the_oracles_node_for_node(net_gpu, oracle_runs):
    from librubiks.solving.agents import MCTS
    pool, c = _pool()
    agent = MCTS(net_gpu, c=OWN_C, search_graph=False, net_dtype=torch.float32, sync_every=4)
    agent.snapshot_trees = {}
    agent.search_batch(pool, None, CAPS[-1], slots=7, c=c)
    assert sorted(agent.snapshot_trees) == list(range(len(pool)))
    for (i, g), ref in oracle_runs[1].items():
        compare_tree(agent.snapshot_trees[i * 24 + g], oracle_arrays(ref), len(ref))


@pytest.fixture(scope="module")
def eight(net_gpu):
    """8 depth-20 scrambles, 8 values of c, and the oracle's naive trees after ITERS iterations."""
    np.random.seed(3)
    states = np.array([oc.scramble(20, True)[0] for _ in range(8)])
    onet = oa.TorchNet(net_gpu, device="cuda")
    refs = []
    for s, c in zip(states, C_EIGHT):
        ref = oa.MCTS(onet, c=c, search_graph=False)
        ref.search(s, 12 * ITERS + 64, max_iterations=ITERS)
        refs.append(ref)
    return states, refs


def test_three_phase_form_with_c_per_tree(net_gpu, eight):
    """`max_iterations` runs [rc_mcts_expand -> network -> rc_mcts_backup_select_each]."""
    from librubiks.solving.agents import MCTS
    states, refs = eight
    agent = MCTS(net_gpu, c=OWN_C, search_graph=False, net_dtype=torch.float32, sync_every=4)
    res = agent.search_batch(states, None, 12 * ITERS + 64, max_iterations=ITERS, compact=False, c=np.array(C_EIGHT))
    assert not agent.forest._one_launch
    for t, ref in enumerate(refs):
        assert res.iterations[t] == ref.iterations == ITERS and res.nodes[t] == len(ref)
        compare_tree(agent.forest.tree_arrays(t), oracle_arrays(ref), len(ref))


def _drive_select_each(net, states, c_each, iterations):
    """[rc_mcts_expand -> network -> rc_mcts_backup -> rc_mcts_select_each] (k_mcts_select<0> with c per tree), one iteration at
    a time, as mcts_lockstep.drive(form="select0") drives the scalar export."""
    from librubiks import _hip
    from librubiks.cube import DeviceCubes
    from librubiks.model import GenericNet
    from librubiks.solving import mcts_device as md
    cap = 12 * iterations + 64
    f = md.MCTSForest(len(states), cap, vmm=False)
    f.set_net(GenericNet(net), torch.float32)
    f.set_active(None)
    f.plant(None, DeviceCubes.from_numpy(np.asarray(states)), 0, None, c=torch.tensor(c_each, dtype=torch.float64, device=f.device))
    assert f.c_slot.cpu().tolist() == list(c_each)
    m, st = ctypes.byref(f.struct), _hip.stream_ptr()
    for _ in range(iterations + 1):      # a tree's first iteration takes two steps
        _hip.check(f.lib.rc_mcts_expand(m, cap, st))
        f._evaluate_children()
        _hip.check(f.lib.rc_mcts_backup(m, f.probs.data_ptr(), f.values.data_ptr(), st))
        _hip.check(f.lib.rc_mcts_select_each(m, f.c_slot.data_ptr(), 0, st))
    torch.cuda.synchronize()
    return f


def test_select_alone_with_c_per_tree(net_gpu, eight):
    states, refs = eight
    f = _drive_select_each(net_gpu, states, C_EIGHT, ITERS)
    assert f.iterations.cpu().tolist() == [ITERS] * 8
    for t, ref in enumerate(refs):
        compare_tree(f.tree_arrays(t), oracle_arrays(ref), len(ref))


@pytest.fixture(scope="module")
def many(net_gpu):
    """520 shallow scrambles, c cycling through the grid, and the oracle's graph search of each at cap 60 (5 iterations at most)."""
    np.random.seed(33)
    states = np.array([oc.scramble(1 + i % 7, True)[0] for i in range(520)])
    c = np.array([C_GRID[i % 4] for i in range(520)])
    onet = oa.TorchNet(net_gpu, device="cuda")
    runs = []
    for s, value in zip(states, c):
        r = oa.MCTS(onet, c=value, search_graph=True)
        runs.append(_outcome(r, r.search(s, 60)))
    return states, c, runs


@pytest.mark.parametrize("n_trees", [520, 300], ids=["256_threads", "512_threads"])
def test_launch_shapes_of_a_large_forest(net_gpu, many, n_trees):
    """More than 512 trees: 256 threads a tree; 257 .. 512 trees: 512 threads and four line waves (step_threads, line_waves)."""
    from librubiks.solving.agents import MCTS
    states, c, runs = many
    agent = MCTS(net_gpu, c=OWN_C, search_graph=True, net_dtype=torch.float32, sync_every=2)
    res = agent.search_batch(states[:n_trees], None, 60, c=c[:n_trees])
    assert agent.forest.B == n_trees and agent.forest._one_launch
    _check(res, runs[:n_trees], n_trees)


def test_launch_shape_of_a_small_forest(net_gpu, oracle_runs):
    """24 trees: 1 024 threads a tree, four line waves."""
    from librubiks.solving.agents import MCTS
    states = _easy_states()
    which = np.arange(24) % 4
    agent = MCTS(net_gpu, c=OWN_C, search_graph=True, net_dtype=torch.float32, sync_every=4)
    res = agent.search_batch(states, None, CAPS[-1], c=np.array(C_GRID)[which])
    assert agent.forest.B == 24
    _check(res, [oracle_runs[0][True, CAPS[-1]][i * 24 + g] for g, i in enumerate(which)], "24 trees")


def test_descents_below_the_lds_window(net_gpu, oracle_runs, monkeypatch):
    """8 path levels in LDS, 64-level blocks and ring lines: the descents of the c 0.1 games reach 42 levels, so most levels are
    decided where they lie in HBM (the DEEP body of the kernel), every tree under its own c."""
    from librubiks.solving import mcts_device as md
    from librubiks.solving.agents import MCTS
    for name, value in (("LDS_LEVELS", 8), ("PATH_BLOCK", 64), ("RING_LEVELS", 64)):
        monkeypatch.setattr(md, name, value)
    pool, c = _pool()
    agent = MCTS(net_gpu, c=OWN_C, search_graph=False, net_dtype=torch.float32, sync_every=4)
    agent.snapshot_trees = {}
    res = agent.search_batch(pool, None, CAPS[-1], slots=40, c=c)
    assert (agent.forest.lds_levels, agent.forest.path_block) == (8, 64)
    _check(res, oracle_runs[0][False, CAPS[-1]], "lds_levels 8")
    assert oracle_runs[2] == 42
    for (i, g), ref in oracle_runs[1].items():
        compare_tree(agent.snapshot_trees[i * 24 + g], oracle_arrays(ref), len(ref))


def _same(a, b, what):
    for k in ("solved", "status", "nodes", "iterations", "lengths"):
        assert np.array_equal(np.asarray(getattr(a, k)), np.asarray(getattr(b, k))), (what, k)
    assert all(list(a.queues[g]) == list(b.queues[g]) for g in range(len(a.solved))), what


def test_one_value_for_every_game_is_the_scalar_search(net_gpu):
    from librubiks.solving import mcts_device as md
    from librubiks.solving.agents import MCTS
    states = _easy_states()
    plain = MCTS(net_gpu, c=0.6, search_graph=True, net_dtype=torch.float32, sync_every=4)
    want = plain.search_batch(states, None, 400)
    assert plain.forest._graphs and not any(md.C_PER_TREE in key for key in plain.forest._graphs)     # c=None: graphs keyed by the value
    agent = MCTS(net_gpu, c=OWN_C, search_graph=True, net_dtype=torch.float32, sync_every=4)
    _same(agent.search_batch(states, None, 400, c=np.full(len(states), 0.6)), want, "array of one value")
    assert all(md.C_PER_TREE in key for key in agent.forest._graphs)
    _same(agent.search_batch(states, None, 400, c=0.6), want, "a scalar that is not the agent's own")
    _same(plain.search_batch(states, None, 400, c=0.6), want, "the agent's own c as a scalar")
    assert not any(md.C_PER_TREE in key for key in plain.forest._graphs)


def test_one_captured_graph_serves_every_value_of_c(net_gpu):
    from librubiks.solving import mcts_device as md
    from librubiks.solving.agents import MCTS
    pool, c = _pool()
    keys = []
    for values in (c, np.full(len(pool), 0.6)):         # four distinct values, one value
        agent = MCTS(net_gpu, c=OWN_C, search_graph=True, net_dtype=torch.float32, sync_every=4, use_graph=True)
        agent.search_batch(pool, None, 200, slots=32, c=values)
        keys.append(sorted(agent.forest._graphs, key=repr))
        assert keys[-1] and all(key[1] is md.C_PER_TREE for key in keys[-1])
    assert keys[0] == keys[1]


def test_prepare_captures_the_graphs_a_per_game_search_replays(net_gpu, oracle_runs):
    from librubiks.solving import mcts_device as md
    from librubiks.solving.agents import MCTS
    pool, c = _pool()
    agent = MCTS(net_gpu, c=OWN_C, search_graph=True, net_dtype=torch.float32, sync_every=4)
    agent.prepare(32, 200, per_game_c=True)
    keys = set(agent.forest._graphs)
    assert keys and all(key[1] is md.C_PER_TREE for key in keys)
    res = agent.search_batch(pool, None, 200, slots=32, c=c)
    assert set(agent.forest._graphs) == keys             # nothing was left to capture
    _check(res, oracle_runs[0][True, 200], "prepared")


def test_trained_pool_equals_separate_searches(trained):
    """The fused split engine (rc_mcts_step_head_each; with max_iterations rc_mcts_backup_select_head_each), deterministic: the
    pooled search against one `search_batch` per value of c."""
    from librubiks.solving.agents import MCTS
    from librubiks.solving.results import BatchResult
    np.random.seed(29)
    states = np.array([oc.scramble(3 + i % 10, True)[0] for i in range(16)])
    G, cap = len(states), 1500
    pool, c = np.tile(states, (len(C_GRID), 1)), np.repeat(C_GRID, G)
    for kwargs in ({}, {"max_iterations": 12}):
        parts = [(np.arange(p * G, (p + 1) * G), MCTS(trained, c=value, search_graph=True, deterministic=True).search_batch(states, None, cap, **kwargs))
                 for p, value in enumerate(C_GRID)]
        separate = BatchResult.merge(len(pool), parts, 0.0)
        if not kwargs:
            assert separate.solved.any() and not separate.solved.all()
        agent = MCTS(trained, c=OWN_C, search_graph=True, deterministic=True)
        for slots in ((24, None) if not kwargs else (None,)):
            _same(agent.search_batch(pool, None, cap, slots=slots, c=c, **kwargs), separate, (kwargs, slots))


@pytest.mark.parametrize("weights", ["standin", "trained"])
def test_grid_search_routes_produce_identical_histories(net_gpu, trained, weights):
    from librubiks.solving.agents import MCTS
    from librubiks.solving.evaluation import Evaluator
    from librubiks.solving.hyper_optim import GridSearch
    fixed = {"net": net_gpu, "search_graph": True, "net_dtype": torch.float32} if weights == "standin" else \
        {"net": trained, "search_graph": True, "deterministic": True}
    out = {}
    for pooled in (True, False):
        np.random.seed(17)
        ev = Evaluator(6, [4], None, 200, slots=8)
        gs = GridSearch(None, {"c": (0.1, 100)}, pooled=pooled)
        gs.objective_from_evaluator(ev, MCTS, fixed)
        assert gs.pooled_route_applies()
        best = gs.optimize(4)
        state = np.random.get_state()
        out[pooled] = (gs.score_history, gs.parameter_history, gs.optimal, gs.highscore, best, state[1].tolist(), state[2])
    assert len(out[True][0]) == 4 and [p["c"] for p in out[True][1]] == np.linspace(0.1, 100, 4).tolist()
    assert out[True] == out[False]
