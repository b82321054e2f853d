"""
The host's side of the batched EGVM search, on the CPU: the whole-round decision table of a game (rc_egvm_draw, the library's
host generator on the game's MT19937 state) is what the oracle's `_expand` draws step by step after np.random.seed(seed) -- same
decisions, same stream state afterwards; it is bit-equal to `RandomState.choice(2, W, p=...)` followed by
`RandomState.randint(0, 12, k)` across eps, W and seeds; and `seeds` takes the forms the search documents.
"""
import inspect

import numpy as np
import pytest

import conftest  # noqa: F401  (puts the package on sys.path)
from oracle import agents as oa
from oracle import cube as oc

EPS = (0, 0.1, 0.2, 0.375, 0.5, 1)


class _ConstantNet:
    """Policy that always prefers action 0: the oracle's draws do not depend on the network."""

    def logits(self, states):
        return np.tile(np.arange(12, 0, -1, dtype=np.float32), (len(states), 1))

    def value(self, states):
        return np.zeros(len(states), dtype=np.float32)


def _same_stream(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


def _numpy_round(rs, eps, W, D):
    """The reference's calls (agents.py:694-698) on a RandomState: 255 where the policy decides."""
    table = np.full((D, W), 255, dtype=np.uint8)
    for d in range(D):
        rnd = rs.choice(2, W, p=[1 - eps, eps]).astype(bool)
        table[d, rnd] = rs.randint(0, 12, rnd.sum())
    return table


def _library_round(streams, g, eps, W, D):
    from librubiks.solving.egvm_device import choice_cdf
    table = np.full((D, W + 7), 77, dtype=np.uint8)      # (a stride wider than the rows: the padding is not written)
    streams.draw([g], [0], choice_cdf(eps), W, D, table, W)
    assert (table[:, W:] == 77).all()
    return table[:, :W]


def test_library_draws_equal_numpys():
    """Every eps, every W from 1 to 500 under 40 of 200 seeds on one running stream each: the same tables as choice + randint
    and the same generator state afterwards."""
    from librubiks.solving.egvm_device import POLICY, GameStreams
    assert POLICY == 255
    seeds = np.arange(200) * 7919 + 3
    for eps in EPS:
        streams = GameStreams(seeds)
        streams.start(np.arange(200))
        for g, seed in enumerate(seeds):
            rs = np.random.RandomState(int(seed))
            for W in range(1 + g % 5, 501, 5):
                assert np.array_equal(_library_round(streams, g, eps, W, 2), _numpy_round(rs, eps, W, 2)), (eps, g, W)
            probe = np.random.RandomState(0)
            probe.set_state(streams.state(g))
            assert _same_stream(probe, rs), (eps, g)


@pytest.mark.parametrize("eps,W,D", [(0, 3, 4), (0.1, 7, 9), (0.2, 64, 3), (0.375, 10, 50), (0.5, 33, 5), (1, 5, 6), (0.375, 500, 250)])
def test_round_table_equals_the_oracles_draws(eps, W, D):
    from librubiks.solving.egvm_device import POLICY, GameStreams
    np.random.seed(4)
    state = oc.scramble(30, True)[0]           # deep: no worker meets the solved cube, so `_expand` runs all D steps
    seeds = np.array([0, 1, 12345, 2 ** 31 - 2])
    streams = GameStreams(seeds)
    streams.start(np.arange(len(seeds)))
    for g, seed in enumerate(seeds):
        np.random.seed(int(seed))
        for _ in range(2):                     # two rounds on the running stream, as the reference's next `_expand` goes on
            paths, _, hit = oa.EGVM(_ConstantNet(), eps, W, D)._expand(state)
            assert hit is None
            table = _library_round(streams, g, eps, W, D)
            # the oracle's path holds the random action where one was drawn and the policy's choice (action 0 here) elsewhere
            assert np.array_equal(np.where(table == POLICY, 0, table), paths.T)
            assert ((table == POLICY) | (table < 12)).all()
            assert eps != 0 or (table == POLICY).all()
            assert eps != 1 or (table < 12).all()
        after = np.random.get_state()
        got = streams.state(g)
        assert np.array_equal(got[1], after[1]) and got[2] == after[2]


def test_library_draw_rejects_bad_arguments():
    from librubiks import _hip
    from librubiks.solving.egvm_device import GameStreams
    streams = GameStreams(np.array([1, 2]))
    streams.start([0, 1])
    table = np.zeros((3, 16), dtype=np.uint8)
    before = (streams.keys.copy(), streams.pos.copy())
    for games, slots, W, n_rows in (([2], [0], 4, 16), ([-1], [0], 4, 16), ([0], [4], 4, 16), ([0], [-1], 4, 16), ([0], [0], 0, 16),
                                    ([0], [0], 4, 17), ([0, 1], [0, 3], 5, 16)):
        with pytest.raises(_hip.RubiksHipError):
            streams.draw(games, slots, 0.5, W, 3, table, n_rows)
    assert np.array_equal(streams.keys, before[0]) and np.array_equal(streams.pos, before[1]) and not table.any()
    streams.draw([0, 1], [0, 3], 0.5, 4, 3, table, 16)   # slots 0 and 3 of four: rows 0-3 and 12-15
    assert not table[:, 4:12].any() and table[:, :4].any() and table[:, 12:].any()


def test_seed_forms():
    from librubiks.solving.egvm_device import game_seeds
    given = np.array([5, 7, 2 ** 31 - 2])
    assert np.array_equal(game_seeds(given, 3), given)
    assert np.array_equal(game_seeds(9, 6), np.random.RandomState(9).randint(0, 2 ** 31 - 1, size=6))
    np.random.seed(3)
    want = np.random.randint(0, 2 ** 31 - 1, size=4)
    after = np.random.get_state()
    np.random.seed(3)
    assert np.array_equal(game_seeds(None, 4), want)
    assert np.array_equal(np.random.get_state()[1], after[1]) and np.random.get_state()[2] == after[2]
    with pytest.raises(ValueError):
        game_seeds(np.array([1, 2]), 3)
    with pytest.raises(ValueError):
        game_seeds(np.array([0.5, 1.5, 2.5]), 3)


def test_search_batch_signature():
    from librubiks.solving.agents import EGVM
    params = inspect.signature(EGVM.search_batch).parameters
    assert list(params)[1:] == ["states", "time_limit", "max_states", "seeds", "slots"]
    assert params["seeds"].default is None and params["slots"].default is None
    assert inspect.signature(EGVM.__init__).parameters["deterministic"].default is False
