"""
tests/golden/rollout_golden.npz on the CPU: the games recorded from the reference's RandomSearch, PolicySearch (greedy and
sampled) and ValueSearch are the oracle's games bounded at 64 moves, and a restatement of the random and the sampled step on a
game's own RandomState -- what the lock-step kernels are given -- reproduces the reference's draws from the global stream.
"""
import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import agents as oa
from oracle import cube as oc

CAP = 64


@pytest.fixture(scope="module")
def fx():
    return np.load(f"{GOLDEN}/rollout_golden.npz")


def _play(state, step):
    """(solved within CAP moves, the moves) of a game whose move at state x is step(x)."""
    q = []
    if oc.is_solved(state):
        return True, q
    while len(q) < CAP:
        a = int(step(state))
        q.append(a)
        state = oc.rotate(state, *oc.ACTION_SPACE[a])
        if oc.is_solved(state):
            return True, q
    return False, q


def _same(fx, name, g, ok, q):
    ref = fx[f"{name}_queues"][g]
    assert ok == bool(fx[f"{name}_solved"][g]) and q == ref[ref >= 0].tolist(), (name, g)


def test_the_fixture_is_what_the_issue_describes(fx):
    assert fx["states"].shape == (300, 20) and fx["seeds"].tolist() == [7000 + 1000 * d + s for d in (1, 2, 3) for s in range(100)]
    np.random.seed(2017)
    assert np.array_equal(fx["states"][117], oc.scramble(2, True)[0])
    for name in ("random", "greedy", "sampled", "value"):
        lens = (fx[f"{name}_queues"] >= 0).sum(1)
        assert (lens[~fx[f"{name}_solved"]] == CAP).all() and (lens[fx[f"{name}_solved"]] >= 1).all()
    m = fx["sampled_margin"]
    assert (m < 1e-5).sum() == 3 and (m < 1e-5).mean() <= 0.02 and 2e-6 < m.min() < 3e-6 and fx["sampled_solved"].sum() == 7


@pytest.mark.parametrize("name,cls", [("greedy", oa.PolicySearch), ("value", oa.ValueSearch)])
def test_the_oracle_plays_the_greedy_games(fx, standin_net, name, cls):
    onet = oa.TorchNet(standin_net)
    for g, s in enumerate(fx["states"]):
        agent = cls(onet)
        ok = agent.search(s, CAP)
        _same(fx, name, g, bool(ok), [int(a) for a in agent.action_queue])


def test_random_games_from_the_games_own_streams(fx):
    for g, (s, seed) in enumerate(zip(fx["states"], fx["seeds"])):
        rs = np.random.RandomState(int(seed))
        _same(fx, "random", g, *_play(s, lambda x: rs.randint(12)))


def test_sampled_games_from_the_games_own_streams(fx, standin_net):
    def step(x, rs):
        with torch.no_grad():
            p = torch.softmax(standin_net(torch.from_numpy(oc.as_oh(x[None])), value=False), dim=1).numpy()[0]
        cdf = p.astype(np.float64).cumsum()
        cdf /= cdf[-1]
        return min(11, int(cdf.searchsorted(rs.random_sample(), side="right")))
    for g, (s, seed) in enumerate(zip(fx["states"], fx["seeds"])):
        rs = np.random.RandomState(int(seed))
        _same(fx, "sampled", g, *_play(s, lambda x: step(x, rs)))
