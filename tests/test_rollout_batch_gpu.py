"""
The lock-step one-step agents (`RandomSearch / PolicySearch / ValueSearch.search_batch(..., seeds=, slots=)`, rc_rollout_plant /
rc_rollout_step_policy / rc_rollout_step_value): game g of a batch ends exactly as the reference's `search(states[g])` right after
np.random.seed(seeds[g]), stopped at `max_states` moves -- whoever shares the batch, however many slots there are, however many
moves a round has, replayed from a captured graph or launched one by one.  The stand-in net runs in fp32 (its outputs are exact
integers over 16, the same for every batch shape) unless a test says otherwise.
"""
import ctypes
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import GOLDEN, ROOT  # noqa: E402
from oracle import agents as oa  # noqa: E402  (checker only)
from oracle import cube as oc  # noqa: E402

WEIGHTS = os.path.join(ROOT, "weights", "fc_small_r1")
KINDS = ("random", "greedy", "sampled", "value")
PER_WORKGROUP = 4 * 256     # games one workgroup of the step kernels covers: four per lane


@pytest.fixture(scope="module")
def net_gpu(standin_net):
    return standin_net.cuda()


@pytest.fixture(scope="module")
def trained():
    from librubiks.model import Model
    return Model.load(WEIGHTS).cuda().eval()


def make(kind, net=None, **kw):
    from librubiks.solving.agents import PolicySearch, RandomSearch, ValueSearch
    if kind == "random":
        agent = RandomSearch()
        for k, v in kw.items():
            assert k in ("use_graph", "steps_per_round")
            setattr(agent, k, v)
        return agent
    kw.setdefault("net_dtype", torch.float32)
    return ValueSearch(net, **kw) if kind == "value" else PolicySearch(net, sample_policy=kind == "sampled", **kw)


def games_of(res):
    return [(bool(res.solved[g]), int(res.nodes[g]), list(res.queues[g])) for g in range(len(res.solved))]


def consistent(res):
    """The fields of a lock-step result that repeat each other."""
    lens = np.array([len(q) for q in res.queues])
    assert np.array_equal(res.nodes, lens) and np.array_equal(res.iterations, lens)
    assert np.array_equal(res.lengths, np.where(res.solved, lens, -1))
    assert res.game_seconds.shape == lens.shape and (res.game_seconds >= 0).all() and (res.game_seconds <= res.seconds).all()


def replay(state, queue):
    for a in queue:
        state = oc.rotate(state, *oc.ACTION_SPACE[int(a)])
    return state


def scrambles(seed, n, solved_at=()):
    np.random.seed(seed)
    states = np.array([oc.scramble(1 + i % 6, True)[0] for i in range(n)])
    for i in solved_at:
        states[i] = oc.get_solved()
    return states, np.random.randint(0, 2 ** 31 - 1, n)


# ---- 1. the reference's own games -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    return np.load(f"{GOLDEN}/rollout_golden.npz")


def recorded(solved, queues):
    return [(bool(ok), int((q >= 0).sum()), q[q >= 0].tolist()) for ok, q in zip(solved, queues)]


@pytest.mark.parametrize("kind", KINDS)
def test_reference_fixture(net_gpu, fx, kind):
    """Every recorded game in one lock-step batch at 64 moves.  Sampled policy: a game whose closest draw came within 1e-5 of
    a cdf edge is reported, not compared -- an fp32 softmax differs between implementations by a few ulp per term, at most
    about 3e-6 on an edge over 12 terms -- and at most 2 % of the games may be left out for that."""
    states, want = fx["states"], recorded(fx[f"{kind}_solved"], fx[f"{kind}_queues"])
    if kind == "value":   # ... and the solved games recorded earlier (tests/golden/simple_agents_golden.npz)
        old = np.load(f"{GOLDEN}/simple_agents_golden.npz")
        assert len(old["value_states"]) == 107
        states = np.concatenate([states, old["value_states"]])
        want = want + recorded(np.ones(107, dtype=bool), old["value_queues"])
    seeds = np.concatenate([fx["seeds"], np.zeros(len(states) - 300, dtype=np.int64)])
    res = make(kind, net_gpu).search_batch(states, None, 64, seeds=seeds)
    got = games_of(res)
    consistent(res)
    compared = np.ones(len(states), dtype=bool)
    if kind == "sampled":
        compared[:300] = fx["sampled_margin"] >= 1e-5
        left = np.flatnonzero(~compared)
        print(f"sampled: {len(left)} of 300 games not compared (margins {fx['sampled_margin'][left].tolist()}); "
              f"of those equal anyway: {sum(got[g] == want[g] for g in left)}")
        assert len(left) <= 0.02 * 300
    for g in np.flatnonzero(compared):
        assert got[g] == want[g], f"{kind} game {g}"
    print(f"{kind}: {int(compared.sum())} games equal, {int(res.solved.sum())} solved")


# ---- 2. the oracle, and the path without keywords ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,ref_cls", [("greedy", oa.PolicySearch), ("value", oa.ValueSearch)])
def test_oracle_parity(net_gpu, kind, ref_cls):
    from librubiks.solving import rollout_device as rd
    onet = oa.TorchNet(net_gpu, device="cuda")
    np.random.seed(4)
    states = np.array([oc.scramble(1 + i % 6, True)[0] for i in range(48)])   # the games of test_step_agents_vs_oracle
    states[5] = oc.get_solved()
    res = make(kind, net_gpu).search_batch(states, None, 30, slots=48)
    plain = make(kind, net_gpu).search_batch(states, None, 30)
    consistent(res)
    assert games_of(res) == games_of(plain) and np.array_equal(res.lengths, plain.lengths) and np.array_equal(res.status, plain.status)
    for g, s in enumerate(states):
        ref = ref_cls(onet)
        ok = ref.search(s, 30)
        assert games_of(res)[g] == (bool(ok), len(ref), [int(a) for a in ref.action_queue]), f"game {g}"
        assert oc.is_solved(replay(s, res.queues[g])) == ok
    assert res.status[5] == rd.ROOT_SOLVED and res.solved[5] and res.lengths[5] == 0
    assert set(res.status.tolist()) <= {rd.SOLVED, rd.EXHAUSTED, rd.ROOT_SOLVED} and (res.status == rd.EXHAUSTED).any()


def test_the_time_limit_ends_the_pool_after_its_first_round(net_gpu):
    """A time limit that has passed when the clock is first looked at, behind round 1: the two games in the slots made one round's
    moves and end EXHAUSTED (the time limit ended them), the four still waiting end as games that never got a slot."""
    from librubiks.solving import rollout_device as rd
    np.random.seed(19)
    states = np.array([oc.scramble(9, True)[0] for _ in range(6)])
    agent = make("greedy", net_gpu, steps_per_round=2)
    res = agent.search_batch(states, 1e-9, 1_000, slots=2)                    # (500 rounds fit: no cap ends a game)
    print("status", res.status.tolist(), "nodes", res.nodes.tolist(), "game_seconds", res.game_seconds.tolist(), "seconds", res.seconds)
    consistent(res)
    assert agent.batch_stats["rounds"] == 1
    assert not res.solved[2:].any() and (res.nodes[2:] == 0).all() and (res.game_seconds[2:] == 0).all()
    assert (res.status[2:] == rd.EXHAUSTED).all()
    played = ~res.solved[:2]
    assert played.any() and (res.status[:2][played] == rd.EXHAUSTED).all() and (res.status[:2][~played] == rd.SOLVED).all()
    assert (res.nodes[:2][played] == 2).all() and (res.game_seconds[:2] > 0).all()
    assert res.seconds >= res.game_seconds.max()


# ---- 3. shapes where the kernels can go wrong -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_every_shape_plays_the_same_games(net_gpu, kind):
    G = PER_WORKGROUP + 1
    states, seeds = scrambles(31, G, solved_at=(2, 16, G - 1))
    whole = make(kind, net_gpu).search_batch(states, None, 30, seeds=seeds)
    consistent(whole)
    want = games_of(whole)
    assert sum(w[0] for w in want) >= 3 and sum(not w[0] for w in want) >= 3

    def same(res, n, what):
        consistent(res)
        assert games_of(res) == want[:n] and np.array_equal(res.status, whole.status[:n]), f"{kind}: {what}"
    for n in (1, 3, 5, 16, 17):
        same(make(kind, net_gpu).search_batch(states[:n], None, 30, seeds=seeds[:n]), n, f"{n} games")
    for slots in (1, 5, 17):
        same(make(kind, net_gpu).search_batch(states[:17], None, 30, seeds=seeds[:17], slots=slots), 17, f"{slots} slots")
    for K in (1, 3, 8):                                 # 30 moves end in mid-round for K 8
        for graph in (True, False):
            agent = make(kind, net_gpu, steps_per_round=K, use_graph=graph)
            same(agent.search_batch(states[:17], None, 30, seeds=seeds[:17], slots=5), 17, f"K {K}, graph {graph}")
            assert bool(agent.batch._graphs) == graph and agent.batch.K == K
            one = agent.search_batch(states[:17], None, 1, seeds=seeds[:17], slots=5)      # one move per game
            consistent(one)
            assert games_of(one) == [(ok and n <= 1, min(n, 1), q[:1]) for ok, n, q in want[:17]], f"{kind}: cap 1, K {K}, graph {graph}"


# ---- 4. the random agent's streams ------------------------------------------------------------------------------------------
def test_random_search_streams():
    G, cap = 300, 30
    states, seeds = scrambles(41, G, solved_at=(9,))
    res = make("random").search_batch(states, None, cap, seeds=seeds)
    consistent(res)
    for g in range(G):
        draws = np.random.RandomState(int(seeds[g])).randint(12, size=cap).tolist()
        x, q = states[g], []
        while not oc.is_solved(x) and len(q) < cap:
            q.append(draws[len(q)])
            x = oc.rotate(x, *oc.ACTION_SPACE[q[-1]])
        assert games_of(res)[g] == (bool(oc.is_solved(x)), len(q), q), f"game {g}"
    assert 2 <= res.solved.sum() < G
    a = make("random").search_batch(states, None, cap, seeds=7)
    b = make("random").search_batch(states, None, cap, seeds=np.random.RandomState(7).randint(0, 2 ** 31 - 1, G))
    assert games_of(a) == games_of(b) != games_of(res)
    np.random.seed(77)                                   # seeds=None with slots: one draw of G seeds from the global stream at entry
    c = make("random").search_batch(states, None, cap, slots=64)
    after = np.random.get_state()
    np.random.seed(77)
    drawn = np.random.randint(0, 2 ** 31 - 1, size=G)
    assert np.array_equal(np.random.get_state()[1], after[1]) and np.random.get_state()[2] == after[2]
    assert games_of(c) == games_of(make("random").search_batch(states, None, cap, seeds=drawn))


# ---- 5. queue rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "value"])
def test_queue_rows_grow_in_a_search_bounded_by_time(net_gpu, kind):
    from librubiks.solving.agents import DEFAULT_STEP_CAP
    np.random.seed(9)
    deep = np.array([oc.scramble(30, True)[0] for _ in range(12)])
    narrow, wide = make(kind, net_gpu), make(kind, net_gpu)
    narrow.QUEUE_STEPS, wide.QUEUE_STEPS = 2, DEFAULT_STEP_CAP
    a = narrow.search_batch(deep, 120.0, None, seeds=3)   # (the step cap ends these games long before the time limit)
    b = wide.search_batch(deep, 120.0, None, seeds=3)
    consistent(a)
    assert wide.batch.Q == DEFAULT_STEP_CAP and narrow.batch.Q >= DEFAULT_STEP_CAP > 2
    assert games_of(a) == games_of(b) and np.array_equal(a.status, b.status)
    assert (a.nodes[~a.solved] == DEFAULT_STEP_CAP).all() and (~a.solved).any()
    held = narrow.batch.states.numpy()
    for g in range(len(deep)):                             # every queue replays to the state the slot holds
        assert np.array_equal(replay(deep[g], a.queues[g]), held[g]), f"game {g}"


def test_a_full_queue_row_ends_the_game_and_nothing_is_written_beyond_it():
    from librubiks import _hip
    from librubiks.cube import DeviceCubes
    from librubiks.solving import rollout_device as rd
    S, Q = 5, 2
    np.random.seed(10)
    deep = np.array([oc.scramble(20, True)[0] for _ in range(S)])
    batch = rd.RolloutBatch(S, "random", 1, Q, use_graph=False)
    guard = torch.full((S * Q + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    batch.struct.queues = guard.data_ptr()                 # the S rows of Q bytes, then 64 bytes nobody may touch
    batch.reset(DeviceCubes.from_numpy(deep))
    acts = np.random.randint(12, size=(3, 16)).astype(np.uint8)
    dec = torch.from_numpy(acts).cuda()
    lib, st = _hip.lib(), ctypes.byref(batch.struct)
    for t in range(3):
        _hip.check(lib.rc_rollout_step_policy(st, None, 0, 0, dec[t].data_ptr(), None, 10, _hip.stream_ptr()), "rc_rollout_step_policy")
    torch.cuda.synchronize()
    assert batch.status.tolist() == [rd.QUEUE_FULL] * S and batch.steps.tolist() == [Q] * S
    g = guard.cpu().numpy()
    assert np.array_equal(g[:S * Q].reshape(S, Q), acts[:2, :S].T) and (g[S * Q:] == 0xEE).all()
    held = batch.states.numpy()
    for i in range(S):                                     # the move that did not fit was not made
        assert np.array_equal(held[i], replay(deep[i], acts[:2, i]))


@pytest.mark.parametrize("bf16", [False, True])
def test_the_policy_step_on_a_head_of_its_own(bf16):
    """rc_rollout_step_policy through the C ABI on hand-made logits: np.argmax's order with ties and a NaN, np.random.choice for
    given uniforms (edges included), and a NaN probability."""
    from librubiks import _hip
    from librubiks.cube import DeviceCubes
    from librubiks.solving import rollout_device as rd
    S, ld = 21, 16
    rs = np.random.RandomState(2)
    logits = (rs.randint(-40, 40, (S, 12)) / 8).astype(np.float32)          # (exact in bf16 too)
    logits[3, [4, 9]] = logits[3].max() + 1                                  # a tie: the first maximum
    logits[5, 7], logits[6, [2, 10]] = np.nan, np.nan                        # a NaN is the maximum, the first one
    logits[8], logits[11] = 0.0, 1.5                                         # equal logits: p = 1 / 12 in every softmax, so the edges are exact
    head = torch.zeros((S, ld), dtype=torch.float32)
    head[:, :12] = torch.from_numpy(logits)
    head[:, 12:] = 99.0                                                      # the value column and the padding are not logits
    head = head.cuda().to(torch.bfloat16 if bf16 else torch.float32)
    np.random.seed(10)
    deep = np.array([oc.scramble(20, True)[0] for _ in range(S)])
    p = torch.softmax(torch.from_numpy(logits), dim=1).numpy()
    cdf = p.astype(np.float64).cumsum(1)
    cdf /= cdf[:, -1:]
    u = rs.random_sample(S)
    u[8], u[9], u[10], u[11] = cdf[8, 3], 0.0, np.nextafter(1.0, 0.0), np.nextafter(cdf[11, 5], 0.0)   # on an edge, the ends, just under an edge
    for sampled in (False, True):
        batch = rd.RolloutBatch(S, "sampled" if sampled else "greedy", 1, 4, use_graph=False)
        batch.reset(DeviceCubes.from_numpy(deep))
        uni = torch.from_numpy(np.concatenate([u, np.zeros(32 - S)])).cuda()
        _hip.check(_hip.lib().rc_rollout_step_policy(ctypes.byref(batch.struct), head.data_ptr(), ld, int(bf16), None,
                                                     uni.data_ptr() if sampled else None, 10, _hip.stream_ptr()), "rc_rollout_step_policy")
        torch.cuda.synchronize()
        status, steps, acts = batch.status.tolist(), batch.steps.tolist(), batch.queues[:, 0].tolist()
        for g in range(S):
            if sampled and g in (5, 6):                                      # np.random.choice: "probabilities contain NaN"
                assert (status[g], steps[g]) == (rd.BAD_POLICY, 0) and np.array_equal(batch.states.numpy()[g], deep[g])
                continue
            want = int(cdf[g].searchsorted(u[g], side="right")) if sampled else int(np.argmax(logits[g]))
            assert (status[g], steps[g], acts[g]) == (rd.RUNNING, 1, want), (sampled, g)
        if not sampled:
            assert acts[3] == 4 and acts[5] == 7 and acts[6] == 2 and acts[8] == 0
        else:
            assert acts[8] == 4 and acts[9] == 0 and acts[10] == 11 and acts[11] == 5


# ---- 6. the Evaluator -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_evaluator_pools_these_agents(net_gpu, kind):
    from librubiks.solving.evaluation import Evaluator
    games, depths, cap = 12, [1, 2, 4], 30
    agent = make(kind, net_gpu)
    calls, inner = [], agent.search_batch
    agent.search_batch = lambda states, *a, **kw: (calls.append((states.n, kw)), inner(states, *a, **kw))[1]
    agent.search_batch.__signature__ = inspect.signature(inner)
    np.random.seed(21)
    ev = Evaluator(games, depths, None, cap, slots=8)
    res1, states1, times1 = ev.eval(agent)
    assert calls == [(len(depths) * games, {"slots": 8})]                     # all depths in one pool
    assert res1.shape == states1.shape == times1.shape == (len(depths), games)
    assert len(ev.batch_seconds) == 1 and (times1 > 0).all() and (times1 <= ev.batch_seconds[0]).all()
    assert (states1[res1 == -1] == cap).all() and (states1[res1 >= 0] == res1[res1 >= 0]).all()
    if kind in ("greedy", "value"):                                           # nothing is drawn: the unpooled evaluator's games
        np.random.seed(21)
        res0, states0, _ = Evaluator(games, depths, None, cap).eval(make(kind, net_gpu))
        assert np.array_equal(res1, res0) and np.array_equal(states1, states0)
    if kind == "value":
        assert (res1[0] == 1).all()                                           # a scramble of one move is solved by one move


# ---- 7. trained weights ---------------------------------------------------------------------------------------------------------
def _depth8(n=64):
    np.random.seed(8)
    states = np.array([oc.scramble(8, True)[0] for _ in range(n)])
    return states, np.random.randint(0, 2 ** 31 - 1, n)


@pytest.mark.parametrize("kind", ["greedy", "sampled", "value"])
def test_trained_deterministic_is_batch_independent(trained, kind):
    from librubiks.model import F32_SPLIT
    states, seeds = _depth8()
    mk = lambda: make(kind, trained, net_dtype=F32_SPLIT, deterministic=True)   # noqa: E731
    plain = mk().search_batch(states, None, 50, seeds=seeds)
    pooled = mk().search_batch(states, None, 50, seeds=seeds, slots=16)
    consistent(plain)
    assert games_of(pooled) == games_of(plain) and np.array_equal(pooled.status, plain.status)
    alone, want = mk(), games_of(plain)
    for g in range(len(states)):
        one = alone.search_batch(states[g:g + 1], None, 50, seeds=seeds[g:g + 1])
        assert games_of(one) == [want[g]], f"game {g}"
    print(f"{kind}: {int(plain.solved.sum())} of {len(states)} solved, moves {int(plain.nodes.sum())}")
    for g in np.flatnonzero(plain.solved):
        assert oc.is_solved(replay(states[g], plain.queues[g]))


@pytest.mark.parametrize("engine", ["bf16", "686", "686_folded"])
def test_other_engines_run(trained, engine):
    from librubiks.model import F32_SPLIT, Folded, Model, ModelConfig
    np.random.seed(18)
    states = np.array([oc.scramble(1 + i % 3, True)[0] for i in range(40)])
    if engine == "bf16":
        net, dt = trained, torch.bfloat16
    else:
        torch.manual_seed(686)
        net = Model.create(ModelConfig(architecture="fc_small", is2024=False)).cuda().eval()
        net, dt = (Folded(net) if engine == "686_folded" else net), F32_SPLIT
    for kind in ("greedy", "sampled", "value"):
        res = make(kind, net, net_dtype=dt).search_batch(states, None, 20, seeds=5, slots=16)
        consistent(res)
        assert ((res.nodes == 20) | res.solved).all()
        for g in np.flatnonzero(res.solved):
            assert oc.is_solved(replay(states[g], res.queues[g])), (engine, kind, g)
        if kind == "value":
            assert res.solved[::3].all() and (res.lengths[::3] == 1).all()   # one move from solved: the first solved child is taken


# ---- 8. wall time -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_lock_step_is_no_slower_than_the_stepwise_batch(trained, kind):
    """The probe's smallest leg (tools/rollout_batch_probe.py): 512 depth-20 scrambles, 200 moves, the default engine; the two
    forms alternate in one process after a warm-up of both, three repetitions.  Lock step may be slower than the path without
    keywords by no more than that path's own min-max spread in this run."""
    spec = importlib.util.spec_from_file_location("rollout_batch_probe", os.path.join(ROOT, "tools", "rollout_batch_probe.py"))
    probe = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    from librubiks.model import F32_SPLIT
    out = probe.compare(probe.make_agent(kind, trained, F32_SPLIT), ["stepwise", "lockstep"], probe.scrambles(512, [20]), 200, reps=3)
    a, b = out["stepwise"]["seconds"], out["lockstep"]["seconds"]
    print(f"{kind}: stepwise {a}, lock step {b}, ratio of medians {a['median'] / b['median']:.2f}")
    assert b["median"] <= a["median"] + (a["max"] - a["min"]), (a, b)
