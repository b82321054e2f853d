"""
Continuous batching of A* (`AStar.search_batch(..., slots=S)`, rc_astar_plant, rc_astar_solutions): a game searched in a pool of
S problem slots is the game of a plain batch, and so of the oracle's single-problem run; replanted slots carry nothing of their
earlier tenants; the solutions walked on the device are those of a host walk; the pooled Evaluator and a pool bounded by time
report what the plain forms report.
"""
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import GOLDEN, ROOT  # noqa: E402
from oracle import agents as oa  # noqa: E402  (checker only)
from oracle import cube as oc  # noqa: E402

INT_MAX = 2 ** 31 - 1
WEIGHTS = os.path.join(ROOT, "weights", "fc_small_r1")


@pytest.fixture(scope="module")
def net_gpu(standin_net):
    return standin_net.cuda()


@pytest.fixture(scope="module")
def trained():
    from librubiks.model import Model
    return Model.load(WEIGHTS).cuda().eval()


def _easy_states(n=72, seed=21):
    """Depths 1-7, a solved root and duplicate scrambles."""
    np.random.seed(seed)
    states = np.array([oc.scramble(1 + i % 7, True)[0] for i in range(n)])
    states[9] = oc.get_solved()
    states[40:44] = states[3:7]
    return states


def _host_walk(arrays, goal):
    q, i = [], int(goal)
    while i != 1:
        q.append(int(arrays["parent_actions"][i]))
        i = int(arrays["parents"][i])
    return q[::-1]


def test_pooled_games_equal_the_oracle(net_gpu):
    from librubiks.solving import astar_device as ad
    from librubiks.solving.agents import AStar
    states = _easy_states()
    onet = oa.TorchNet(net_gpu, device="cuda")
    seen = set()
    for lam, nexp, cap in ((0.2, 16, 1500), (0.0, 5, 400)):
        ref = []
        for s in states:
            r = oa.AStar(onet, lambda_=lam, expansions=nexp)
            ref.append((r.search(s, cap), len(r), list(r.action_queue)))
        for slots in (1, 7, 32, len(states)):
            res = AStar(net_gpu, lambda_=lam, expansions=nexp, net_dtype=torch.float32).search_batch(states, None, cap, slots=slots)
            for g, (ok, n, q) in enumerate(ref):
                assert (bool(res.solved[g]), int(res.nodes[g]), list(res.queues[g])) == (ok, n, q), f"slots {slots}, game {g}"
                assert res.lengths[g] == (len(q) if ok else -1)
            seen |= set(res.status.tolist())
    assert {ad.SOLVED, ad.EXHAUSTED, ad.ROOT_SOLVED} <= seen


def _check_slot_hygiene(batch, b):
    n = int(batch.n_nodes[b].item())
    row = batch.hash[b].cpu().numpy()
    assert sorted(row[row != 0].tolist()) == list(range(1, n + 1)), f"slot {b}"
    lo = b * (batch.C + 1)
    assert bool((batch.claim[lo:lo + batch.C + 1] == INT_MAX).all()), f"slot {b}"


def test_replanted_slots_hold_only_their_last_problem(net_gpu):
    from librubiks.cube.device import DeviceCubes
    from librubiks.solving import astar_device as ad
    np.random.seed(5)
    deep = [oc.scramble(20, True)[0] for _ in range(2)]
    d1 = [oc.scramble(1, True)[0] for _ in range(2)]
    mid = oc.scramble(8, True)[0]
    pool = DeviceCubes.from_numpy(np.array(deep + [oc.get_solved()] * 2 + d1 + [mid]))
    lam, cap = 0.2, 3000
    batch = ad.AStarBatch(2, cap, 16)
    batch.set_net(net_gpu, torch.float32)
    batch.reset(pool)
    for _ in range(400):
        batch.iteration(lam, cap)
        if not batch.any_running():
            break
    assert (batch.status.cpu().numpy() == ad.EXHAUSTED).all()
    both = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    batch.plant(both, pool, 2)                           # large exhausted problems -> solved roots
    assert batch.status.tolist() == [ad.ROOT_SOLVED] * 2 and batch.n_nodes.tolist() == [0, 0]
    batch.iteration(lam, cap)
    batch.plant(both, pool, 4)                           # -> depth 1
    for _ in range(10):
        batch.iteration(lam, cap)
    assert batch.status.tolist() == [ad.SOLVED] * 2
    for b in range(2):
        _check_slot_hygiene(batch, b)
    before = {k: getattr(batch, k).clone() for k in ("status", "n_nodes", "hash", "heap_size")}
    batch.plant(torch.tensor([-1, 2], dtype=torch.int32, device="cuda"), pool, 0)   # no such slots: nothing is written
    for k, t in before.items():
        assert torch.equal(getattr(batch, k), t), k
    # a replanted problem after k iterations is the same problem in a fresh batch
    batch.plant(both[1:], pool, 6)
    fresh = ad.AStarBatch(1, cap, 16)
    fresh.set_net(net_gpu, torch.float32)
    fresh.reset(DeviceCubes.from_numpy(np.array([mid])))
    for _ in range(3):
        batch.iteration(lam, cap)
        fresh.iteration(lam, cap)
    got, want = batch.problem_arrays(1), fresh.problem_arrays(0)
    assert got["n"] == want["n"] > 1
    for k in ("states", "G", "parents", "parent_actions"):
        assert np.array_equal(got[k][1:], want[k][1:]), k
    assert got["open_queue"] == want["open_queue"]
    assert batch.iterations.tolist()[1] == fresh.iterations.tolist()[0] == 3
    for b in range(2):
        _check_slot_hygiene(batch, b)


def test_trained_pool_equals_the_plain_batch(trained):
    from librubiks import cube
    from librubiks.solving.agents import AStar
    golden = np.load(os.path.join(GOLDEN, "solve_golden.npz"))
    lam, n_exp, cap, _ = golden["astar_params"]
    states = golden["states"][:len(golden["astar_solved"])]
    assert len(states) == 128
    mk = lambda: AStar(trained, lambda_=float(lam), expansions=int(n_exp), deterministic=True)   # noqa: E731
    plain = mk().search_batch(states, None, int(cap))
    pooled = mk().search_batch(states, None, int(cap), slots=24)
    for k in ("solved", "nodes", "lengths", "iterations", "status"):
        assert np.array_equal(np.asarray(getattr(pooled, k)), np.asarray(getattr(plain, k))), k
    assert all(list(pooled.queues[g]) == list(plain.queues[g]) for g in range(len(states)))
    solved = golden["astar_solved"]
    agree = (pooled.solved == solved) & (pooled.nodes == golden["astar_nodes"]) & \
        (pooled.lengths == np.where(solved, golden["astar_qlen"], -1))
    assert agree.mean() >= 0.9, agree.mean()
    won = np.flatnonzero(pooled.solved)
    acts, lens = pooled.queues.padded(won)
    x = states[won].copy()
    for j in range(acts.shape[1]):
        move = lens > j
        x[move] = cube.multi_rotate(x[move], *cube.indices_to_actions(acts[move, j].astype(np.int64)))
    assert cube.multi_is_solved(x).all()


def test_pooled_evaluator_matches_per_depth_batches(trained):
    from librubiks.solving.agents import AStar
    from librubiks.solving.evaluation import Evaluator
    games, depths, cap, slots = 40, [2, 4, 6], 3000, 16
    mk = lambda: AStar(trained, lambda_=0.2, expansions=20, deterministic=True)   # noqa: E731
    np.random.seed(11)
    res0, states0, _ = Evaluator(games, depths, None, cap).eval(mk())
    np.random.seed(11)
    ev = Evaluator(games, depths, None, cap, slots=slots)
    res1, states1, times1 = ev.eval(mk())
    assert np.array_equal(res0, res1) and np.array_equal(states0, states1)
    assert len(ev.batch_seconds) == 1
    pool_s = ev.batch_seconds[0]
    assert (times1 > 0).all() and (times1 <= pool_s).all()
    later = times1.ravel()[slots:]
    assert later.mean() < pool_s


def test_time_limit_bounds_the_pool(net_gpu):
    from librubiks.solving import astar_device as ad
    from librubiks.solving.agents import AStar, astar_time_only_capacity
    np.random.seed(3)
    states = np.array([oc.scramble(20, True)[0] for _ in range(200)])
    agent = AStar(net_gpu, lambda_=0.2, expansions=10, net_dtype=torch.float32)
    agent.search_batch(states[:4], None, 2000)                        # engine and batch set up outside the timed search
    limit, cap = 0.5, 20_000
    t0 = time.perf_counter()
    res = agent.search_batch(states, limit, cap, slots=4)
    wall = time.perf_counter() - t0
    assert agent.batch.C == cap < astar_time_only_capacity(4)        # the node cap sized the batch, not the time limit
    never = (res.nodes == 0) & (res.status == ad.EXHAUSTED)
    assert never.sum() > 100 and not res.solved[never].any() and (res.lengths[never] == -1).all()
    assert (res.game_seconds[never] == 0).all() and (res.game_seconds[~never] > 0).all()
    assert res.seconds < limit + 0.25 and wall < limit + 0.5, (res.seconds, wall)


def test_device_solutions_match_a_host_walk(net_gpu):
    from librubiks import _hip
    from librubiks.solving import astar_device as ad
    from librubiks.solving.agents import AStar
    states = _easy_states()
    agent = AStar(net_gpu, lambda_=0.2, expansions=16, net_dtype=torch.float32)
    res = agent.search_batch(states, None, 1500)
    batch = agent.batch
    status, sol = batch.status.cpu().numpy(), batch.solved_idx.cpu().numpy()
    lens, queues = batch.solutions(np.arange(batch.B), width=3)       # most queues are longer than 3: the second pass
    assert (lens > 3).sum() >= 5
    for b in range(batch.B):
        if status[b] == ad.SOLVED:
            q = _host_walk(batch.problem_arrays(b), sol[b])
            assert lens[b] == len(q) and list(queues[b]) == q, f"problem {b}"
        else:
            assert lens[b] == (0 if status[b] == ad.ROOT_SOLVED else -1) and list(queues[b]) == []
        assert list(res.queues[b]) == list(queues[b])
    # rows that are not the problem's: a parent outside 1 .. n, and a cycle, are reported and never followed
    won = np.flatnonzero(status == ad.SOLVED)
    b, lo = int(won[0]), int(won[0]) * (batch.C + 1)
    n, goal = int(batch.n_nodes[b].item()), int(sol[won[0]])
    keep = int(batch.parents[lo + goal].item())
    for bad in (n + 7, goal):
        batch.parents[lo + goal] = bad
        with pytest.raises(_hip.RubiksHipError, match=f"problem {b} "):
            batch.solutions([b])
    batch.parents[lo + goal] = keep
    # game 0's attributes after a pooled search are those of a plain search of game 0
    pooled = AStar(net_gpu, lambda_=0.2, expansions=16, net_dtype=torch.float32)
    pooled.search_batch(states, None, 1500, slots=7)
    alone = AStar(net_gpu, lambda_=0.2, expansions=16, net_dtype=torch.float32)
    alone.search(states[0], None, 1500)
    assert len(pooled) == len(alone) and list(pooled.action_queue) == list(alone.action_queue)
    for k in ("states", "G", "parents", "parent_actions"):
        assert np.array_equal(getattr(pooled, k), getattr(alone, k)), k
    assert pooled.open_queue == alone.open_queue and pooled.indices == alone.indices
