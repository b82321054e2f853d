"""
Trained-weight searches on every engine the agents offer, against the reference's own games: tests/golden/solve_golden.npz holds the
outcomes of the reference's MCTS (c 0.6, graph search, cap 5 000) and A* (lambda 0.2, N 100, cap 20 000) on weights/fc_small_r1 for
128 depth-20 scrambles, and the reference module's fp32 / float64 outputs on the states those searches evaluate
(tests/golden/make_golden_solve.py; the loader and the oracle are held to the same fixture in tests/test_solve_golden.py).

(a) every engine's solve rate lies inside the reference's 95 % Bernoulli interval (its bernoulli_error, z = 1.96);
(b) the fp32-accurate engines end at least 90 % of the games as the reference does (solved, nodes, solution length); bf16's share is
    printed only.  Every solved game's queue solves its scramble;
(c) a game that ends otherwise does so because of the network's rounding, not because of the search: the oracle, fed the
    (state -> P, V) pairs the engine itself computed, rebuilds the engine's game exactly -- MCTS on every engine, A* on the
    deterministic split engine (whose values do not depend on the batch, so they can be recomputed for the replay);
(d) the engines' outputs on those states, as one launch and in windows of 352 and 5 632 rows (the row counts the layer plans
    switch at), against the reference module's outputs.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import GOLDEN, ROOT  # noqa: E402
from oracle import agents as oa  # noqa: E402  (checker only)
from oracle import cube as oc  # noqa: E402

WEIGHTS = os.path.join(ROOT, "weights", "fc_small_r1")
Z95 = 1.959963984540054     # the reference's z for alpha = 0.05 (librubiks/utils bernoulli_error)
ENGINES = ("f32s", "f32s-det", "fp32", "bf16")
MIN_AGREEMENT = {"f32s": 0.9, "f32s-det": 0.9, "fp32": 0.9, "bf16": None}     # bf16: reported, not asserted


def _dtype(engine):
    from librubiks.model import F32_SPLIT, F32_SPLIT_DET
    return {"f32s": F32_SPLIT, "f32s-det": F32_SPLIT_DET, "fp32": torch.float32, "bf16": torch.bfloat16}[engine]


class _TableNet:
    """The oracle's network as a lookup of recorded outputs: state -> (P, V) for MCTS, state -> V for A*."""

    def __init__(self, table):
        self.table = table

    def __call__(self, states):
        if len(states) == 0:
            return np.zeros((0, 12), dtype=np.float32), np.zeros(0, dtype=np.float32)
        rows = [self.table[s.tobytes()] for s in states]
        return np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], dtype=np.float32)

    def value(self, states):
        return np.array([self.table[s.tobytes()] for s in states], dtype=np.float32)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "solve_golden.npz"))


@pytest.fixture(scope="module")
def trained():
    from librubiks.model import Model
    return Model.load(WEIGHTS).cuda().eval()


@pytest.fixture(scope="module")
def played(golden, trained):
    """Every engine x agent on the fixture's games, one search_batch each: {(engine, agent): (BatchResult, what (c) replays)}.
    What a replay needs is read out right after each search and the searcher dropped, so that one forest's node store at a
    time exists (the next forest of the shape takes it over), as in every other test of the process."""
    import gc
    from librubiks.cube.device import DeviceCubes
    from librubiks.solving.agents import MCTS, AStar
    c, _, mcap, _ = golden["mcts_params"]
    lam, n_exp, acap, _ = golden["astar_params"]
    states = golden["states"]
    out = {}
    for e in ENGINES:
        m = MCTS(trained, c=float(c), search_graph=True, net_dtype=_dtype(e))
        res = m.search_batch(states, None, int(mcap), compact=False)                   # the trees stay in m.forest
        out[e, "mcts"] = (res, {int(t): m.forest.tree_arrays(int(t)) for t in np.flatnonzero(~_agreement(golden, "mcts", res))})
        a = AStar(trained, lambda_=float(lam), expansions=int(n_exp), net_dtype=_dtype(e))
        res = a.search_batch(states[:len(golden["astar_solved"])], None, int(acap))
        replay = {}
        if e == "f32s-det":     # the games that end otherwise, and the first four, so that the replay itself always runs
            for t in sorted(set(np.flatnonzero(~_agreement(golden, "astar", res)).tolist()) | {0, 1, 2, 3}):
                arr = a.batch.problem_arrays(t)
                visited = arr["states"][1:arr["n"] + 1]
                replay[t] = (visited, a.batch.engine.value_cubes(DeviceCubes.from_numpy(visited)).cpu().numpy())
        out[e, "astar"] = (res, replay)
        del m, a
        gc.collect()
    return out


def _agreement(golden, agent, res):
    solved = golden[f"{agent}_solved"]
    return (res.solved == solved) & (res.nodes == golden[f"{agent}_nodes"]) & (res.lengths == np.where(solved, golden[f"{agent}_qlen"], -1))


def test_engines_end_the_reference_games(golden, played):
    """(a) + (b), one table row per engine x agent."""
    rows, failed = [], []
    for e in ENGINES:
        for agent in ("mcts", "astar"):
            res, _ = played[e, agent]
            ref = golden[f"{agent}_solved"]
            p, n = float(ref.mean()), len(ref)
            err = Z95 * np.sqrt(p * (1 - p) / n)
            rate, same = float(res.solved.mean()), _agreement(golden, agent, res)
            rows.append(f"{e:9s} {agent:6s} {rate:6.3f}   [{p - err:.3f}, {p + err:.3f}]   {int(same.sum()):3d} / {n}")
            if not p - err <= rate <= p + err:
                failed.append(f"{e} {agent}: solve rate {rate:.3f} outside the reference's {p:.3f} +- {err:.3f}")
            if MIN_AGREEMENT[e] is not None and same.mean() < MIN_AGREEMENT[e]:
                failed.append(f"{e} {agent}: {int(same.sum())} of {n} games end as the reference's")
            for t in np.flatnonzero(res.solved):
                x = golden["states"][t]
                for a in res.queues[t]:
                    x = oc.rotate(x, *oc.ACTION_SPACE[a])
                assert oc.is_solved(x), (e, agent, t)
                assert len(res.queues[t]) == res.lengths[t]
    print("\nengine    agent    rate   reference 95 % interval   same games\n" + "\n".join(rows))
    assert not failed, failed


@pytest.mark.parametrize("engine", ENGINES)
def test_mcts_games_that_end_otherwise_are_the_networks_doing(golden, played, engine):
    """(c) for MCTS: every game the engine ends otherwise than the reference is the game the oracle plays on the engine's own
    outputs -- node count, queue and iterations."""
    res, trees = played[engine, "mcts"]
    c, _, cap, _ = golden["mcts_params"]
    print(f"\n{engine}: {len(trees)} MCTS games end otherwise than the reference's: {sorted(trees)}")
    for t, tree in trees.items():
        n = tree["n"]
        table = {tree["states"][i].tobytes(): (tree["P"][i].astype(np.float32), np.float32(tree["V"][i])) for i in range(1, n + 1)}
        ref = oa.MCTS(_TableNet(table), c=float(c), search_graph=True)
        ok = ref.search(golden["states"][t], int(cap))
        assert bool(res.solved[t]) == ok and res.nodes[t] == len(ref) == n, f"game {t}"
        assert list(res.queues[t]) == list(ref.action_queue) and res.iterations[t] == ref.iterations, f"game {t}"


def test_astar_games_that_end_otherwise_are_the_networks_doing(golden, played):
    """(c) for A* on the deterministic split engine: a state's value is the same in any launch, so the visited states' values are
    recomputed and the oracle replayed on them."""
    res, replay = played["f32s-det", "astar"]
    lam, n_exp, cap, _ = golden["astar_params"]
    print(f"\nf32s-det: {int((~_agreement(golden, 'astar', res)).sum())} A* games end otherwise than the reference's")
    for t, (visited, values) in replay.items():
        ref = oa.AStar(_TableNet(dict(zip((s.tobytes() for s in visited), values))), float(lam), int(n_exp))
        ok = ref.search(golden["states"][t], int(cap))
        assert bool(res.solved[t]) == ok and res.nodes[t] == len(ref), f"game {t}"
        assert list(res.queues[t]) == list(ref.action_queue), f"game {t}"


def _outputs(eng, states):
    """Softmaxed policy (float64, from the engine's logits), the value as the MCTS head gives it and the value as A*'s value head
    gives it, for one launch over `states`."""
    from librubiks.cube.device import DeviceCubes
    cubes = DeviceCubes.from_numpy(states)
    if eng.supports_cubes:
        out = eng.head_cubes(cubes).float()
        logits, v, v_only = out[:, :12], out[:, 12], eng.value_cubes(cubes)
    else:
        oh = cubes.as_oh(eng.input_dtype)
        logits, v = eng(oh)
        v_only = eng.value(oh)
    return (logits.double().softmax(dim=1).cpu().numpy(), v.double().cpu().numpy(), v_only.double().cpu().numpy())


def _module_error(trained, states, p64, v64, dtype):
    """Max |error| against float64 of the reference's module itself, cast to `dtype`, on this GPU (where a GPU exists the reference
    runs its forward there: librubiks/__init__.py `gpu`)."""
    import copy
    from librubiks.cube.device import DeviceCubes
    net = copy.deepcopy(trained).to(dtype)
    with torch.no_grad():
        logits, v = net(DeviceCubes.from_numpy(states).as_oh(torch.float32).to(dtype))
    P, V = logits.double().softmax(dim=1).cpu().numpy(), v.double().reshape(-1).cpu().numpy()
    return {"P": np.abs(P - p64).max(), "V": np.abs(V - v64).max()}


@pytest.mark.parametrize("engine", ENGINES)
def test_engine_outputs_on_the_states_deep_searches_evaluate(golden, trained, engine):
    """
    (d) The probe states twice over (7 724 rows) as one launch, in windows of 352 and in windows of 5 632 rows.
    Split engines: at most 1.25 x the largest fp32 error of the same network + 1e-7 -- the reference's module on its CPU run
    (fixture: P 9.9e-6, V 2.7e-6), the module on this GPU (P 4.1e-6, V 1.5e-5) and the plain fp32 GEMM chain of the
    BatchNorm-folded network the engines run (P 1.6e-5, V 2.6e-5; folding alone takes the CPU module's P error to 1.3e-5).  The
    split engines sit at P 1.3-1.4e-5, V 1.0-1.3e-5: inside the folded chain's error, above 1.25 x the unfolded module's in P.
    bf16: at most 1.25 x the error of the reference's module run in bfloat16 on this GPU (P 1.0e-1, V 5.7e-2: values reach -12.9).
    """
    from librubiks.model import make_inference_net
    eng = make_inference_net(trained, _dtype(engine))
    probe = golden["probe_states"]
    states, idx = np.concatenate([probe, probe]), np.tile(np.arange(len(probe)), 2)
    p32, v32, p64, v64 = (golden[k][idx] for k in ("probe_p32", "probe_v32", "probe_p64", "probe_v64"))
    cpu32 = {"P": np.abs(p32 - p64).max(), "V": np.abs(v32 - v64).max()}     # the reference's own fp32 error, on its CPU run
    gpu32 = _module_error(trained, states, p64, v64, torch.float32)
    P, V, _ = _outputs(make_inference_net(trained, torch.float32), states)
    chain32 = {"P": np.abs(P - p64).max(), "V": np.abs(V - v64).max()}      # the folded network on the fp32 GEMM chain
    e32 = {k: max(cpu32[k], gpu32[k], chain32[k]) for k in cpu32}
    e16 = _module_error(trained, states, p64, v64, torch.bfloat16) if engine == "bf16" else None
    print(f"\nreference module's max |error| vs float64: fp32 on its CPU run P {cpu32['P']:.3e}, V {cpu32['V']:.3e}; fp32 on this GPU "
          f"P {gpu32['P']:.3e}, V {gpu32['V']:.3e}; folded fp32 chain P {chain32['P']:.3e}, V {chain32['V']:.3e}" + ("" if e16 is None else f"; bf16 on this GPU P {e16['P']:.3e}, V {e16['V']:.3e}"))
    first = None
    for window in (len(states), 352, 5632):
        parts = [_outputs(eng, states[lo:lo + window]) for lo in range(0, len(states), window)]
        P, V, V_only = (np.concatenate(x) for x in zip(*parts))
        got = {"P": np.abs(P - p64).max(), "V": max(np.abs(V - v64).max(), np.abs(V_only - v64).max())}
        print(f"{engine}, windows of {window}: max |error| vs float64: P {got['P']:.3e}, V {got['V']:.3e}")
        if engine in ("f32s", "f32s-det"):
            for k in ("P", "V"):
                assert got[k] <= 1.25 * e32[k] + 1e-7, (window, k, got[k], e32[k])
        elif engine == "fp32":
            np.testing.assert_allclose(P, p32, rtol=1e-4, atol=1e-4)
            np.testing.assert_allclose(V, v32, rtol=1e-4, atol=1e-4)
            np.testing.assert_allclose(V_only, v32, rtol=1e-4, atol=1e-4)
        else:
            for k in ("P", "V"):
                assert got[k] <= 1.25 * e16[k], (window, k, got[k], e16[k])
        if engine == "f32s-det":    # one summation order whatever the launch: the same bits in every window
            if first is None:
                first = (P, V, V_only)
            assert all(np.array_equal(a, b) for a, b in zip(first, (P, V, V_only))), window
