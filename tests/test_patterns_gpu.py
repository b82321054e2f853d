"""
librubiks/analysis/pattern_mining.py on the device: find_generalized_patterns returns what the reference's function returned for
every recorded batch (tests/golden/patterns_golden.npz), order included, whichever of its three forms the batch comes in; a batch
over the budget or with a byte that is no action raises; generate_actions plays the reference's games as one search_batch and
returns what the reference's loop over `search` would; `mine` does both.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import conftest  # noqa: E402
import patterns_model as pm  # noqa: E402


@pytest.fixture(scope="module")
def records():
    fx = np.load(os.path.join(conftest.GOLDEN, "patterns_golden.npz"))
    out = {}
    for k in sorted(k[:-len("_support")] for k in fx.files if k.endswith("_support")):
        text = bytes(fx[f"{k}_patterns"]).decode()
        out[k] = (fx[f"{k}_acts"], fx[f"{k}_lens"], float(fx[f"{k}_support"]), list(zip(text.split("\n") if text else [], fx[f"{k}_values"].tolist())))
    assert len(out) == 46
    return out


def test_every_recorded_result_of_the_reference(records):
    from librubiks.analysis.pattern_mining import find_generalized_patterns
    for k, (acts, lens, support, want) in records.items():
        sequences = [pm.names_of(acts[s, :lens[s]]) for s in range(len(lens))]
        assert list(find_generalized_patterns(sequences, support).items()) == want, k
    assert find_generalized_patterns([], 0.5) == {}


def test_the_three_input_forms(records):
    from librubiks.analysis.pattern_mining import find_generalized_patterns
    from librubiks.solving.results import QueueTable
    for k in ("renaming", "ties", "random05", "ragged_03"):
        acts, lens, support, want = records[k]
        wide = np.full((len(lens), acts.shape[1] + 3), 77, dtype=np.uint8)   # bytes beyond a length are not looked at
        wide[:, :acts.shape[1]] = np.where(np.arange(acts.shape[1])[None] < lens[:, None], acts, 77)
        table = QueueTable.from_queues([acts[s, :lens[s]].tolist() for s in range(len(lens))])
        for form in ((acts, lens), (wide, lens.astype(np.int32)), table, QueueTable(acts, lens)):
            assert list(find_generalized_patterns(form, support).items()) == want, k


def test_what_raises(records):
    from librubiks import _hip
    from librubiks.analysis import pattern_mining as mining
    acts, lens, support, want = records["ragged_03"]
    need = mining.workspace_bytes(int(lens.sum()))
    with pytest.raises(ValueError, match=f"need {need} bytes"):
        mining.find_generalized_patterns((acts, lens), support, budget_bytes=need - 1)
    assert list(mining.find_generalized_patterns((acts, lens), support, budget_bytes=need).items()) == want
    bad = acts.copy()
    bad[4, 60] = 12
    with pytest.raises(_hip.RubiksHipError, match=r"sequences \[4\]: \['bad action'\]"):
        mining.find_generalized_patterns((bad, lens), support)
    bad[4, 60], bad[4, 64] = acts[4, 60], 12                                  # behind the sequence's 64 moves: not part of it
    assert lens[4] == 64 and list(mining.find_generalized_patterns((bad, lens), support).items()) == want


@pytest.fixture(scope="module")
def agent(standin_net):
    from librubiks.solving.agents import AStar
    return AStar(standin_net.cuda(), 0.2, 16)


def _one_by_one(agent, games, max_time, max_states, depth):
    """The reference's loop (pattern_mining.py:48-61): a scramble, then its search, game after game."""
    from librubiks import cube
    from librubiks.analysis.pattern_mining import names_of
    sequences, solved = [], 0
    for _ in range(games):
        state, _, _ = cube.scramble(depth(), True)
        if agent.search(state, max_time, max_states):
            sequences.append(names_of(agent.action_queue))
            solved += 1
    return sequences, solved


def test_generate_actions_plays_the_references_games(agent):
    from librubiks.analysis.pattern_mining import generate_actions
    np.random.seed(42)
    want, _ = _one_by_one(agent, 8, None, 2000, lambda: np.random.randint(100, 1000))
    np.random.seed(42)
    assert generate_actions(agent, 8, None, 2000) == want
    np.random.seed(42)
    assert generate_actions(agent, 8, None, 2000, slots=3) == want


def test_mine_end_to_end(agent, monkeypatch):
    from librubiks import cube
    from librubiks.analysis import pattern_mining as mining
    np.random.seed(42)
    patterns, sequences = mining.mine(agent, 8, None, 0.3, 2000)
    np.random.seed(42)
    assert sequences == mining.generate_actions(agent, 8, None, 2000)
    assert patterns == pm.mine_plain([pm.actions_of(q) for q in sequences], 0.3)
    # The same with scrambles the stand-in network solves (the reference's are 100 .. 999 moves deep): 8 games of 2 .. 5 moves
    # (deterministic: a game's network values are then the same alone and in the batch, so its queue is, move for move)
    from librubiks.solving.agents import AStar
    agent = AStar(agent.net, 0.2, 16, deterministic=True)
    deep = cube.scramble_batch
    monkeypatch.setattr(cube, "scramble_batch", lambda games, depth, force: deep(games, lambda: np.random.randint(2, 6), force))
    np.random.seed(7)
    want, solved = _one_by_one(agent, 8, None, 2000, lambda: np.random.randint(2, 6))
    np.random.seed(7)
    patterns, sequences = mining.mine(agent, 8, None, 0.3, 2000)
    assert sequences == want and solved >= 6 and max(map(len, sequences)) >= 3
    assert list(patterns.items()) == list(pm.mine_plain([pm.actions_of(q) for q in sequences], 0.3).items()) and "AB" in patterns
