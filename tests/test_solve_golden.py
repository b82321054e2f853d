"""
The trained network as the reference loads it, and the oracle's searches on it, against tests/golden/solve_golden.npz: outcomes of
the reference's own MCTS (c 0.6, graph search, cap 5 000) and A* (lambda 0.2, N 100, cap 20 000) on weights/fc_small_r1, 128 depth-20
scrambles of the seed-0 stream (tests/golden/make_golden_solve.py).  The GPU engines are held to the same fixture in
tests/test_solve_parity_gpu.py; these CPU tests pin the two things that comparison leans on -- the weights the build loads and the
oracle it replays trees on -- to the reference itself.
"""
import hashlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from oracle import agents as oa
from oracle import cube as oc

WEIGHTS = os.path.join(ROOT, "weights", "fc_small_r1")


@pytest.fixture(scope="module")
def solve_golden():
    return np.load(os.path.join(GOLDEN, "solve_golden.npz"))


@pytest.fixture(scope="module")
def trained_cpu():
    from librubiks.model import Model
    return Model.load(WEIGHTS).cpu().eval()


@pytest.fixture
def one_thread():
    """The reference played its games on one torch thread: the same summation order on the CPU here."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def test_fixture_is_self_consistent(solve_golden):
    g = solve_golden
    assert g["states"].shape == (128, 20) and g["mcts_params"].tolist() == [0.6, 1.0, 5000, 20]
    assert g["astar_params"].tolist() == [0.2, 100, 20000, 20]
    np.random.seed(0)
    assert np.array_equal(g["states"], [oc.scramble(20, True)[0] for _ in range(128)])        # the seed-0 stream, in game order
    for agent in ("mcts", "astar"):
        solved, nodes, qlen, queues = (g[f"{agent}_{k}"] for k in ("solved", "nodes", "qlen", "queues"))
        assert 0.10 < solved.mean() < 0.95                      # the caps leave both outcomes: the rate can tell engines apart
        assert ((queues >= 0).sum(1) == qlen).all() and (nodes <= g[f"{agent}_params"][2]).all()
        for s, ok, q, n in zip(g["states"], solved, queues, qlen):
            x = s
            for a in q[:n]:
                x = oc.rotate(x, *oc.ACTION_SPACE[a])
            assert oc.is_solved(x) == ok                        # a solved game's queue solves; an unsolved one's best guess does not
    assert len(g["probe_states"]) == len({s.tobytes() for s in g["probe_states"]})
    assert np.array_equal(g["probe_states"][:128], g["states"])


def test_loader_reads_the_checkpoint_as_the_reference_does(solve_golden, trained_cpu):
    """librubiks.model.Model.load(weights/fc_small_r1) gives the reference's state_dict tensor for tensor (the checkpoint stores
    float16; both loaders must widen it identically), and the module computes the reference module's function."""
    import copy
    g = solve_golden
    sd = trained_cpu.state_dict()
    assert list(sd.keys()) == g["sd_keys"].tolist()
    assert [str(t.dtype) for t in sd.values()] == g["sd_dtypes"].tolist()
    got = [hashlib.sha256(t.detach().contiguous().numpy().tobytes()).hexdigest() for t in sd.values()]
    bad = [k for k, h, w in zip(g["sd_keys"], got, g["sd_sha256"]) if h != w]
    assert not bad, bad
    net64 = copy.deepcopy(trained_cpu).double()
    with torch.no_grad():
        p64, v64 = net64(torch.from_numpy(oc.as_oh(g["probe_states"])).double())
    assert np.abs(p64.softmax(dim=1).numpy() - g["probe_p64"]).max() < 1e-12
    assert np.abs(v64.numpy().reshape(-1) - g["probe_v64"]).max() < 1e-10


def _agree(ref, ok, solved, nodes, qlen, queue):
    return ok == bool(solved) and len(ref) == nodes and len(ref.action_queue) == qlen and list(ref.action_queue) == list(queue[:qlen])


def test_oracle_mcts_ends_the_reference_games_as_the_reference(solve_golden, trained_cpu, one_thread):
    g = solve_golden
    net, cap = oa.TorchNet(trained_cpu), int(g["mcts_params"][2])
    for t in range(8):
        ref = oa.MCTS(net, c=float(g["mcts_params"][0]), search_graph=True)
        ok = ref.search(g["states"][t], cap)
        assert _agree(ref, ok, g["mcts_solved"][t], g["mcts_nodes"][t], g["mcts_qlen"][t], g["mcts_queues"][t]), f"game {t}"
    assert 0 < g["mcts_solved"][:8].sum() < 8                  # both outcomes among the replayed games


def test_oracle_astar_ends_the_reference_games_as_the_reference(solve_golden, trained_cpu, one_thread):
    g = solve_golden
    lam, n_exp, cap = float(g["astar_params"][0]), int(g["astar_params"][1]), int(g["astar_params"][2])
    net = oa.TorchNet(trained_cpu)
    for t in range(4):
        ref = oa.AStar(net, lam, n_exp)
        ok = ref.search(g["states"][t], cap)
        assert _agree(ref, ok, g["astar_solved"][t], g["astar_nodes"][t], g["astar_qlen"][t], g["astar_queues"][t]), f"game {t}"
    assert 0 < g["astar_solved"][:4].sum() < 4
