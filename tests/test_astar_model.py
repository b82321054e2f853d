"""
The NumPy model of the A* kernels (tests/astar_model.py) on the CPU.  Driven as AStarBatch.iteration drives the kernels -- pop,
prefix sum, gather, the stand-in network on the gathered states, push -- its problems end exactly as oracle.agents.AStar's, problem
by problem: every state, G, parent and parent action, the sorted open list, the node count, the solved flag, the action queue and
the status.  That is what makes it a reference for tests/test_astar_kernels_gpu.py rather than a copy of the kernels.  Also here,
because it needs no GPU: the scenarios of that module reach every branch they are meant to reach (seeds and scripts are chosen
here).  The packing and the hash function it uses are pinned in tests/test_keys_model.py.
"""
import numpy as np
import pytest

import conftest  # noqa: F401  (puts the package on sys.path)
import astar_model as am
from oracle import agents as oa
from oracle import cube as oc


@pytest.fixture(scope="module")
def onet(standin_net):
    return oa.TorchNet(standin_net, device="cpu")


def play(onet, states: np.ndarray, lam: float, N: int, max_states: int) -> am.AStarModel:
    """AStar.search_batch on the model: every problem in a slot of its own, capacity = max_states."""
    B, C = len(states), max(max_states, 12 * N + 1)
    m = am.AStarModel(B, N, C, am.min_hash_size(C), out_bytes=20 * am.out_stride(12 * N * B, 0))
    m.init(states)
    while (m.status == am.RUNNING).any():
        m.pop_expand(max_states)
        off = am.offsets(m)
        stride = am.out_stride(int(off[-1]), 0)
        m.gather_new(off, stride)
        gathered = m.out_soa[:20 * stride].reshape(20, stride)
        # the oracle asks its network problem by problem: the same rows in the same call give the same bits
        per_problem = [onet.value(np.ascontiguousarray(gathered[:, off[b]:off[b + 1]].T)) for b in range(B)]
        values = np.concatenate(per_problem + [np.zeros(0, dtype=np.float32)])
        m.push_relax(off, values, lam)
    return m


@pytest.mark.parametrize("lam,N,max_states", [(0.2, 16, 1500), (0.0, 5, 400), (1.0, 1, 300)])
def test_the_model_plays_the_oracles_games(onet, lam, N, max_states):
    np.random.seed(21)
    states = np.array([oc.scramble(1 + i % 7, True)[0] for i in range(70)])   # the games of test_astar_gpu.test_batch_vs_oracle
    states[9] = oc.get_solved()
    m = play(onet, states, lam, N, max_states)
    seen = set()
    for b, s in enumerate(states):
        ref = oa.AStar(onet, lambda_=lam, expansions=N)
        ok = ref.search(s, max_states)
        got, n = m.problem(b), len(ref)
        assert got["n"] == n and got["solved"] == ok and got["queue"] == list(ref.action_queue), f"problem {b}"
        assert np.array_equal(got["states"][1:], ref.states[1:n + 1]), f"problem {b}"
        assert np.array_equal(got["G"][1:], ref.G[1:n + 1]), f"problem {b}"
        assert np.array_equal(got["parents"][2:], ref.parents[2:n + 1]), f"problem {b}"
        assert np.array_equal(got["parent_actions"][2:], ref.parent_actions[2:n + 1]), f"problem {b}"
        assert got["open"] == sorted((float(c), int(i)) for c, i in ref.open_queue), f"problem {b}"
        want = am.ROOT_SOLVED if b == 9 else am.SOLVED if ok else am.OPEN_EMPTY if ref.open_empty else am.EXHAUSTED
        assert got["status"] == want, f"problem {b}"
        assert m.iterations[b] == (0 if b == 9 else ref.iterations), f"problem {b}"
        seen.add(want)
    assert seen == {am.ROOT_SOLVED, am.SOLVED, am.EXHAUSTED}
    assert (m.claim == am.INT_MAX).all()


def test_the_cost_is_rounded_twice():
    """0.2 * 3 is inexact in float64: the product is rounded, then the sum -- a fused multiply-add gives another open list."""
    import math
    lam, G, v = 0.2, 3, np.float32(0.1)
    m = am.AStarModel(1, 1, 13, 32)
    m.init(am.after(oc.get_solved(), am._START)[None])
    m.pop_expand(13)
    m.G[0, 2:14] = G
    m.push_relax(am.offsets(m), np.full(12, v, dtype=np.float32), lam)
    want = float(np.float64(lam) * np.float64(G)) + float(-v)
    assert {c for c, _ in m.heap[0]} == {want}
    if hasattr(math, "fma"):
        assert math.fma(lam, G, float(-v)) != want


# ---- the scenarios of the GPU module: their coverage is a condition ------------------------------------------------------------
@pytest.mark.parametrize("li", range(len(am.LAMBDAS)), ids=["lambda_%g" % x for x in am.LAMBDAS])
@pytest.mark.parametrize("case", list(am.SEEDED_CASES), ids=lambda c: "B%d_N%d_C%d" % c)
def test_the_seeded_scenarios_reach_their_branches(case, li):
    lam = am.LAMBDAS[li]
    m = am.make_model(*case, am.SLACK[lam])
    assert m.H == am.min_hash_size(case[2])
    ops = []
    for launch in am.seeded_scenario(m, am.SEEDS[case][li], lam, am.SLACK[lam]):
        am.apply(m, launch)
        ops.append(launch["op"])
    missing = [k for k in am.SEEDED_WANTED[case] if m.count[k] < 1]
    assert not missing, (missing, dict(m.count))
    assert {"init", "plant", "pop", "gather", "push", "solutions"} <= set(ops)
    assert not (m.status == am.RUNNING).any() and (m.claim == am.INT_MAX).all()


@pytest.mark.parametrize("lam", am.LAMBDAS)
@pytest.mark.parametrize("N", list(am.SCRIPTED_CASES))
def test_the_scripted_searches_reach_their_branches(N, lam):
    m = am.scripted_model(N, am.SLACK[lam])
    for launch in am.scripted_scenario(m, lam, am.SLACK[lam]):
        am.apply(m, launch)
    missing = [k for k in am.scripted_wanted(N) if m.count[k] < 1]
    assert not missing, (missing, dict(m.count))
    names = am.scripts_for(N)
    for b, name in enumerate(names):   # every script by itself, too: the counters are the whole batch's
        if name == "open_empty":
            assert m.status[b] == am.OPEN_EMPTY
        if name.startswith("win"):   # the last launch read the queues with rows of three bytes
            assert m.status[b] == am.SOLVED and m.lengths[b] == 2
            assert m.queues[3 * b:3 * b + 3].tolist() == m.problem(b)["queue"] + [am.FILL] == [am.ACT["R'"], am.ACT["F"], am.FILL]
        if name.startswith("order"):   # U R' L is lowered to 3 in the last push; U R' L L keeps the 6 it was created with
            root = am.after(oc.get_solved(), am._START)
            lowered, kept = (m.index[b][am.after(root, moves).tobytes()] for moves in ("U R' L", "U R' L L"))
            assert m.G[b, lowered] == 3 and m.G[b, kept] == 6 and m.iterations[b] == 7
            writer, reader = (lowered, kept) if name == "order2" else (m.index[b][am.after(root, "U R'").tobytes()], lowered)
            assert m.popped[b].tolist().index(writer) == 6 and m.popped[b].tolist().index(reader) == 21
    if N == 1:
        b = names.index("case2")   # R' L: first G 4 below R R L, then G 2 below L (the larger of the two rows), by R'
        i = m.index[b][am.after(am.after(oc.get_solved(), am._START), "R' L").tobytes()]
        assert m.G[b, i] == 2 and m.parent_actions[b, i] == am.ACT["R'"]
        assert m.states[b, m.parents[b, i]].tobytes() == am.after(am.after(oc.get_solved(), am._START), "L").tobytes()
        b = names.index("win")     # R' L still has the G it was created with: the reference returns before it relaxes
        i = m.index[b][am.after(am.after(oc.get_solved(), "F' R"), "R' L").tobytes()]
        assert m.G[b, i] == 4
