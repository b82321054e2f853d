"""
The NumPy model of the lock-step kernels (tests/lockstep_model.py) on the CPU: driven as the device batches drive the kernels --
decisions from the library's host generators (GameStreams.draw, rollout_device.draw), heads from the stand-in network -- its
games end exactly as the oracle's, game by game: solved flag, node count, action queue.  That is what makes it a reference for
tests/test_lockstep_kernels_gpu.py rather than a copy of the kernels.  Also here, because it needs no GPU: the seeded scenarios
of that module reach every branch they are meant to reach, and the model's sampled policy is np.random.choice.
"""
import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the package on sys.path)
import lockstep_model as lm
from oracle import agents as oa
from oracle import cube as oc
from test_egvm_batch_gpu import MAIN, MORE, inputs, oracle_games


@pytest.fixture(scope="module")
def onet(standin_net):
    return oa.TorchNet(standin_net, device="cpu")


def head_of(onet, states: np.ndarray) -> np.ndarray:
    """[n, 13] float32: 12 logits then the value, as the engines lay a head out."""
    return np.concatenate([onet.logits(states), onet.value(states)[:, None]], axis=1).astype(np.float32)


def play_egvm(onet, states, seeds, eps, W, D, cap) -> list:
    """EGVM._search_lockstep with every game in a slot of its own, on the model."""
    from librubiks.solving import egvm_device as ed
    n, rounds_cap = len(states), ed.queue_rounds(cap, W, D)
    m = lm.EgvmModel(n, W, D, D * max(1, rounds_cap))
    streams = ed.GameStreams(seeds)
    streams.start(np.arange(n))
    m.plant(np.arange(n), states)
    table = np.full((D, (m.R + 15) // 16 * 16), ed.POLICY, dtype=np.uint8)
    played = 0
    while rounds_cap >= 1 and (m.status == lm.EG_RUNNING).any():
        run = np.flatnonzero(m.status == lm.EG_RUNNING)
        streams.draw(run, run, ed.choice_cdf(eps), W, D, table, m.R)
        for d in range(D):
            m.step(d, table[d, :m.R], head_of(onet, m.rows))
        m.round_end(head_of(onet, m.rows)[:, lm.N_ACT], cap)
        played += 1
        assert played <= rounds_cap and not (m.status == lm.EG_QUEUE_FULL).any()
    return m.games(), m


@pytest.mark.parametrize("spec", [MAIN] + MORE, ids=["main", "eps0", "eps1_D1_W21", "W50_D3"])
def test_egvm_model_plays_the_oracles_games(onet, spec):
    seed, n, depth_of, solved_at, eps, W, D, cap, _ = spec
    states, seeds = inputs(seed, n, depth_of, solved_at)
    want = oracle_games(onet, states, seeds, eps, W, D, cap)
    got, m = play_egvm(onet, states, seeds, eps, W, D, cap)
    for g in range(n):
        assert got[g] == want[g], f"game {g} (eps {eps}, W {W}, D {D})"
    assert (m.status[list(solved_at)] == lm.EG_ROOT_SOLVED).all()
    assert set(m.status.tolist()) <= {lm.EG_SOLVED, lm.EG_EXHAUSTED, lm.EG_ROOT_SOLVED}
    assert (m.rounds == -(-m.nodes // (W * D))).all()   # a hit ends its round early


def test_egvm_model_when_no_round_fits(onet):
    states, seeds = inputs(5, 6, lambda i: 2 + i, (5,))
    got, _ = play_egvm(onet, states, seeds, 0.375, 8, 5, 39)
    assert got == oracle_games(onet, states, seeds, 0.375, 8, 5, 39) == [(g == 5, 0, []) for g in range(6)]


@pytest.mark.parametrize("kind,ref_cls", [("greedy", oa.PolicySearch), ("value", oa.ValueSearch)])
def test_rollout_model_plays_the_oracles_games(onet, kind, ref_cls):
    np.random.seed(4)
    states = np.array([oc.scramble(1 + i % 6, True)[0] for i in range(48)])   # the games of test_rollout_batch_gpu.test_oracle_parity
    states[5] = oc.get_solved()
    cap = 30
    m = lm.RolloutModel(48, cap)
    m.plant(np.arange(48), states, kind == "value")
    moves = 0
    while (m.status == lm.RO_RUNNING).any():
        if kind == "value":
            m.step_value(onet.value(m.kids), cap)
        else:
            m.step_policy(onet.logits(m.states), None, None, cap)
        moves += 1
        assert moves <= cap
    got = m.games()
    for g, s in enumerate(states):
        ref = ref_cls(onet)
        ok = ref.search(s, cap)
        assert got[g] == (bool(ok), len(ref), [int(a) for a in ref.action_queue]), f"game {g}"
    assert m.status[5] == lm.RO_ROOT_SOLVED and (m.status == lm.RO_EXHAUSTED).any()
    assert kind == "greedy" or (m.status == lm.RO_SOLVED).any()   # (the stand-in's policy is arbitrary: it solves nothing)
    assert set(m.status.tolist()) <= {lm.RO_SOLVED, lm.RO_EXHAUSTED, lm.RO_ROOT_SOLVED}


def test_random_moves_follow_the_library_draws():
    """Decision bytes: game g's move t is draw t of RandomState(seed).randint(12) (rollout_device.draw), until it is solved."""
    from librubiks.solving import egvm_device as ed
    from librubiks.solving import rollout_device as rd
    np.random.seed(41)
    states = np.array([oc.scramble(1 + i % 3, True)[0] for i in range(40)])
    seeds = np.random.randint(0, 2 ** 31 - 1, 40)
    cap = 12
    streams = ed.GameStreams(seeds)
    rd.start(streams, np.arange(40))
    table = np.zeros((cap, 48), dtype=np.uint8)
    rd.draw(streams, np.arange(40), np.arange(40), table)
    m = lm.RolloutModel(40, cap)
    m.plant(np.arange(40), states, False)
    for t in range(cap):
        m.step_policy(None, table[t, :40], None, cap)
    for g, (ok, n, queue) in enumerate(m.games()):
        x, q = states[g], []
        draws = np.random.RandomState(int(seeds[g])).randint(12, size=cap).tolist()
        while not oc.is_solved(x) and len(q) < cap:
            q.append(draws[len(q)])
            x = oc.rotate(x, *oc.ACTION_SPACE[q[-1]])
        assert (ok, n, queue) == (bool(oc.is_solved(x)), len(q), q), f"game {g}"
    assert 0 < sum(ok for ok, _, _ in m.games()) < 40


def test_sampled_policy_is_numpys_choice():
    """sample12 for the uniform np.random.choice would draw = np.random.choice(12, p=softmax(logits)) as the reference calls it."""
    rs = np.random.RandomState(3)
    for i in range(300):
        logits = (rs.randint(-40, 40, 12) / 8).astype(np.float32)
        if i % 5 == 0:
            logits[rs.randint(0, 12, 3)] = -np.inf
        p = torch.softmax(torch.from_numpy(logits), dim=0).numpy()
        a, margin = lm.sample12(logits, np.random.RandomState(i).random_sample())
        if margin >= lm.MARGIN:   # (torch's softmax and NumPy's may differ in the last bits of a cdf edge)
            assert a == np.random.RandomState(i).choice(12, p=p), i
    for bad in (np.nan, np.inf):
        logits = np.zeros(12, dtype=np.float32)
        logits[7] = bad
        assert lm.sample12(logits, 0.5)[0] == 12
    assert lm.sample12(np.full(12, -np.inf, dtype=np.float32), 0.5)[0] == 12
    flat = np.zeros(12, dtype=np.float32)
    cdf = np.cumsum(np.full(12, np.float32(1) / np.float32(12), dtype=np.float32).astype(np.float64))
    cdf /= cdf[-1]
    assert [lm.sample12(flat, u)[0] for u in (0.0, cdf[3], np.nextafter(cdf[5], 0.0), np.nextafter(1.0, 0.0))] == [0, 4, 5, 11]


# ---- the scenarios of the GPU module: their coverage is a condition --------------------------------------------------------------
def run_egvm_case(case, head_kind):
    S, W, D = case
    narrow, wanted = lm.EGVM_CASES[case]
    ld, bf16 = lm.EGVM_HEADS[head_kind]
    m = lm.EgvmModel(S, W, D, D + 1 if narrow else 3 * D + 2)
    for launch in lm.egvm_scenario(m, lm.EGVM_SEEDS[case + (head_kind,)], ld):
        lm.apply_egvm(m, launch, bf16)
    return m, wanted


@pytest.mark.parametrize("head_kind", list(lm.EGVM_HEADS))
@pytest.mark.parametrize("case", list(lm.EGVM_CASES), ids=lambda c: "S%d_W%d_D%d" % c)
def test_the_egvm_scenarios_reach_their_branches(case, head_kind):
    m, wanted = run_egvm_case(case, head_kind)
    missing = [k for k in wanted if m.count[k] < 1]
    assert not missing, (missing, dict(m.count))


@pytest.mark.parametrize("kind", ["value", "policy"])
@pytest.mark.parametrize("S,Q", lm.ROLLOUT_CASES)
def test_the_rollout_scenarios_reach_their_branches(kind, S, Q):
    m = lm.RolloutModel(S, Q)
    scenario = lm.value_scenario if kind == "value" else lm.policy_scenario
    for launch in scenario(m, lm.ROLLOUT_SEEDS[kind, S, Q]):
        lm.apply_rollout(m, launch)
    missing = [k for k in lm.rollout_wanted(kind, S, Q) if m.count[k] < 1]
    assert not missing, (missing, dict(m.count))
    assert m.min_margin >= lm.MARGIN
