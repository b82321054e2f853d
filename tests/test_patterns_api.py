"""
The host side of librubiks/analysis/pattern_mining.py without a device: the three forms a batch of sequences may come in are one
batch (shown through tests/patterns_model.mine_plain), names that are no moves and batches over the budget raise ValueError before
anything is launched, the result is built from the kernels' rows in the reference's order, and `generate_actions` writes an even
action in lower case, as the reference's does with this package's `action_space`.
"""
import numpy as np
import pytest

import conftest  # noqa: F401
import patterns_model as pm


@pytest.fixture(scope="module")
def mining():
    from librubiks.analysis import pattern_mining
    return pattern_mining


def test_the_three_input_forms_are_one_batch(mining):
    from librubiks.solving.results import QueueTable
    names = [list("RTr"), [], list("FLfF"), ["d"], list("bBbBtT")]
    indices = [pm.actions_of(q) for q in names]
    assert indices[0] == [11, 5, 10] and indices[3] == [6]
    acts, lens = pm.padded(indices)
    wide = np.full((5, 9), 200, dtype=np.uint8)            # bytes beyond a length are not part of the batch
    wide[:, :acts.shape[1]] = np.where(np.arange(acts.shape[1])[None] < lens[:, None], acts, 200)
    want = pm.mine_plain(indices, 0.3)
    assert list(want)[:2] == ["AB", "ABa"] and want["ABa"] == 2 / 5
    for form in (names, QueueTable.from_queues(indices), (acts, lens), (wide, lens.astype(np.int32))):
        a, ls = mining.as_actions(form)
        assert a.dtype == np.uint8 and a.ndim == 2 and a.shape[1] >= 1 and ls.dtype == np.int64 and ls.tolist() == lens.tolist()
        assert pm.mine_plain([a[s, :ls[s]].tolist() for s in range(5)], 0.3) == want
    a, ls = mining.as_actions([[], []])
    assert a.shape == (2, 1) and ls.tolist() == [0, 0]
    a, ls = mining.as_actions([])
    assert a.shape == (0, 1) and len(ls) == 0


def test_what_raises_before_a_launch(mining):
    for bad in ([list("RTr"), list("FxF")], [["F", "R2"]], [["F", 3]], [["F", ""]]):
        with pytest.raises(ValueError, match="no moves"):
            mining.find_generalized_patterns(bad, 0.3)
    with pytest.raises(ValueError, match="do not fit"):
        mining.as_actions((np.zeros((2, 3), dtype=np.uint8), np.array([2, 4])))
    with pytest.raises(ValueError, match="do not fit"):
        mining.as_actions((np.zeros((2, 3), dtype=np.uint8), np.array([2])))
    seqs = [list("FRfr") * 8] * 4
    need = mining.workspace_bytes(4 * 32)
    with pytest.raises(ValueError, match=f"need {need} bytes of workspace, the budget is {need - 1}"):
        mining.find_generalized_patterns(seqs, 0.3, budget_bytes=need - 1)
    assert mining.DEFAULT_BUDGET_BYTES == 2 << 30 and mining.workspace_bytes(100_000 * 25) < mining.DEFAULT_BUDGET_BYTES // 4
    assert mining.find_generalized_patterns([], 0.5) == {} and mining.find_generalized_patterns([[], ["F"][:0]], 0.0) == {}   # nothing to launch


def test_the_result_is_built_from_rows_in_the_references_order(mining):
    indices = [pm.actions_of(q) for q in ("FR", "RFRF", "ffLL", "LLff", "TdTd")]
    acts, lens = pm.padded(indices)
    want = pm.mine_plain(indices, 0)
    b = pm.Batch(acts, lens, 0)
    b.begin()
    rows = []
    while b.live:
        b.next_level()
        b.extend()
        b.close()
        rows += b.rows.tolist()
    shuffled = np.array(rows, dtype=np.uint32)[np.random.RandomState(3).permutation(len(rows))]   # the kernels write them in any order
    assert list(mining.result_of(shuffled, acts, 5).items()) == list(want.items())
    assert mining.generalize([1, 0, 0]) == "AaA" == pm.generalized([1, 0, 0]) and mining.generalize(pm.actions_of("RTrtLR")) == "ABabCA"


def test_generate_actions_names_an_even_action_in_lower_case(mining, monkeypatch):
    from librubiks import cube
    from librubiks.solving.results import BatchResult, QueueTable
    assert mining.SYMBOLS == pm.SYMBOLS and [cube.action_space[a][1] for a in range(12)] == [1, 0] * 6
    assert mining.names_of([0, 1, 10, 11, 4]) == ["f", "F", "r", "R", "t"]
    seen = {}

    def scramble_batch(games, depth, force_not_solved=False):
        np.random.seed(5)
        seen["scramble"] = (games, [depth() for _ in range(50)], force_not_solved)
        return "states", None, None

    class Agent:
        def search_batch(self, states, time_limit, max_states, **kwargs):
            seen["search"] = (states, time_limit, max_states, kwargs)
            queues = QueueTable.from_queues([[0, 3], [5], [], [11, 10, 11]])
            return BatchResult(np.array([True, False, True, True]), queues.lengths(), None, queues, 0.0, None, None)

    monkeypatch.setattr(cube, "scramble_batch", scramble_batch)
    logged = []
    monkeypatch.setattr(mining, "log", logged.append)
    assert mining.generate_actions(Agent(), 4, 1.5, 2000, slots=2) == [["f", "B"], [], ["R", "r", "R"]]
    assert logged == ["Game 2 was not won"]
    games, depths, force = seen["scramble"]
    assert games == 4 and force is True and min(depths) >= 100 and max(depths) < 1000 and len(set(depths)) > 40
    assert seen["search"] == ("states", 1.5, 2000, {"slots": 2})
