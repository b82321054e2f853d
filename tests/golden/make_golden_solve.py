"""
Trained-weight search outcomes recorded from the IMPORTED REFERENCE (librubiks/solving/agents.py MCTS, AStar) on
weights/fc_small_r1, loaded with the reference's own Model.load.  See make_golden.py for how to run (`solve`).

Every game runs in a worker process with one torch thread, so the recorded outputs do not depend on the machine's core
count; the games themselves are independent, so they are spread over a process pool.
"""
import hashlib
import multiprocessing as mp
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
WEIGHTS = os.path.join(os.path.dirname(os.path.dirname(OUT)), "weights", "fc_small_r1")

N_GAMES, DEPTH = 128, 20
MCTS_C, MCTS_CAP = 0.6, 5000                 # cap check: 54 / 128 solved, inside (10 %, 95 %): kept
ASTAR_LAMBDA, ASTAR_N = 0.2, 100
ASTAR_CAP, ASTAR_GAMES = 20000, 128          # cap check: 58 / 128 solved: kept (all 128 games fit the CPU time)
N_PROBE_TREES, PROBE_PER_TREE = 8, 512       # 8 x 512 distinct tree states (+ the 128 roots) for the network probe
WORKERS = 8

_net = None


def _load():
    from librubiks.model import Model
    torch.set_num_threads(1)
    net = Model.load(WEIGHTS)
    net.eval()
    return net


def _mcts_game(args):
    from librubiks.solving.agents import MCTS
    g, state, keep_states = args
    agent = MCTS(_net, c=MCTS_C, search_graph=True)
    ok = agent.search(state, None, MCTS_CAP)
    n = len(agent)
    return g, bool(ok), n, list(agent.action_queue), (agent.states[1:n + 1].copy() if keep_states else None)


def _astar_game(args):
    from librubiks.solving.agents import AStar
    g, state = args
    agent = AStar(_net, lambda_=ASTAR_LAMBDA, expansions=ASTAR_N)
    ok = agent.search(state, None, ASTAR_CAP)
    return g, bool(ok), len(agent), list(agent.action_queue), None


def _pad(queues):
    width = max(1, max(len(q) for q in queues))
    return np.array([q + [-1] * (width - len(q)) for q in queues], dtype=np.int16)


def _play(pool, fn, jobs):
    rows = sorted(pool.map(fn, jobs, chunksize=1), key=lambda r: r[0])
    solved = np.array([r[1] for r in rows])
    nodes = np.array([r[2] for r in rows], dtype=np.int32)
    qlen = np.array([len(r[3]) for r in rows], dtype=np.int32)
    return solved, nodes, qlen, _pad([r[3] for r in rows]), [r[4] for r in rows]


def make_solve():
    global _net
    from librubiks import cube
    from librubiks.model import Model
    _net = _load()
    fx = {}

    # weights as the reference's Model.load returns them: one sha256 per state_dict tensor, in state_dict order
    sd = _net.state_dict()
    fx["sd_keys"] = np.array(list(sd.keys()))
    fx["sd_sha256"] = np.array([hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for t in sd.values()])
    fx["sd_dtypes"] = np.array([str(t.dtype) for t in sd.values()])

    np.random.seed(0)
    states = np.array([cube.scramble(DEPTH, True)[0] for _ in range(N_GAMES)])
    fx["states"] = states
    fx["mcts_params"] = np.array([MCTS_C, 1.0, MCTS_CAP, DEPTH])                   # c, search_graph, max_states, depth
    fx["astar_params"] = np.array([ASTAR_LAMBDA, ASTAR_N, ASTAR_CAP, DEPTH])      # lambda, expansions, max_states, depth

    with mp.get_context("fork").Pool(WORKERS) as pool:
        solved, nodes, qlen, queues, trees = _play(pool, _mcts_game, [(g, states[g], g < N_PROBE_TREES) for g in range(N_GAMES)])
        fx["mcts_solved"], fx["mcts_nodes"], fx["mcts_qlen"], fx["mcts_queues"] = solved, nodes, qlen, queues
        print(f"MCTS c={MCTS_C} cap={MCTS_CAP}: solved {solved.sum()} / {N_GAMES}, nodes {nodes.min()}..{nodes.max()}")
        solved, nodes, qlen, queues, _ = _play(pool, _astar_game, [(g, states[g]) for g in range(ASTAR_GAMES)])
        fx["astar_solved"], fx["astar_nodes"], fx["astar_qlen"], fx["astar_queues"] = solved, nodes, qlen, queues
        print(f"A* lambda={ASTAR_LAMBDA} N={ASTAR_N} cap={ASTAR_CAP}: solved {solved.sum()} / {ASTAR_GAMES}, "
              f"nodes {nodes.min()}..{nodes.max()}")

    # network probe: the roots, then distinct states of the first MCTS trees (evenly strided over each tree's insertion order,
    # so that the deep end of the descents is in), through the reference module in fp32 and the same module cast to float64
    seen, probe = set(), []
    for s in states:
        if s.tobytes() not in seen:
            seen.add(s.tobytes()), probe.append(s)
    for tree in trees[:N_PROBE_TREES]:
        fresh = [s for s in tree if s.tobytes() not in seen]
        step = max(1, len(fresh) // PROBE_PER_TREE)
        for s in fresh[::step][:PROBE_PER_TREE]:
            seen.add(s.tobytes()), probe.append(s)
    probe = np.array(probe)
    with torch.no_grad():
        oh = cube.as_oh(probe).cpu()
        p, v = _net(oh)
        net64 = Model.create(_net.config).double()
        net64.load_state_dict({k: (t.double() if t.is_floating_point() else t) for k, t in _net.state_dict().items()})
        net64.eval()
        p64, v64 = net64(oh.double())
    fx["probe_states"] = probe
    fx["probe_p32"], fx["probe_v32"] = p.softmax(dim=1).numpy(), v.numpy().reshape(-1)
    fx["probe_p64"], fx["probe_v64"] = p64.softmax(dim=1).numpy(), v64.numpy().reshape(-1)
    assert fx["probe_p32"].dtype == np.float32 and fx["probe_p64"].dtype == np.float64
    print("probe:", len(probe), "states; fp32 error vs float64: P", np.abs(fx["probe_p32"] - fx["probe_p64"]).max(),
          "V", np.abs(fx["probe_v32"] - fx["probe_v64"]).max())
    fx["torch_version"] = np.array(torch.__version__)

    path = os.path.join(OUT, "solve_golden.npz")
    np.savez_compressed(path, **fx)
    size = os.path.getsize(path)
    print("solve_golden.npz:", len(fx), "arrays,", size, "bytes")
    assert size <= 1 << 20
    for name in ("mcts", "astar"):
        rate = fx[f"{name}_solved"].mean()
        assert 0.10 < rate < 0.95, (name, rate)                   # the cap check: a rate near 0 or 1 tells few engines apart


if __name__ == "__main__":
    sys.exit(make_solve())
