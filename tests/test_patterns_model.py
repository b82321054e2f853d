"""
The two restatements of pattern mining in tests/patterns_model.py -- the plain rules (`mine_plain`) and the level-wise model of
the kernels' launches (`mine_model`) -- against what the reference's find_generalized_patterns returned
(tests/golden/patterns_golden.npz, written by tests/golden/make_golden_patterns.py): the patterns, their values and their order.
And the threshold: a count reaches `min_count` exactly when count / n >= support as Python divides.
"""
import os

import numpy as np
import pytest

import conftest
import patterns_model as pm


@pytest.fixture(scope="module")
def records():
    fx = np.load(os.path.join(conftest.GOLDEN, "patterns_golden.npz"))
    names = sorted(k[:-len("_support")] for k in fx.files if k.endswith("_support"))
    assert len(names) == 46
    out = {}
    for k in names:
        text = bytes(fx[f"{k}_patterns"]).decode()
        want = list(zip(text.split("\n") if text else [], fx[f"{k}_values"].tolist()))
        out[k] = (fx[f"{k}_acts"], fx[f"{k}_lens"], float(fx[f"{k}_support"]), want, fx[f"{k}_counts"])
    return out


def test_the_fixture_holds_the_hand_made_cases(records):
    r = {k: dict(v[3]) for k, v in records.items()}
    assert r["renaming"]["ABa"] == 2 / 5 and r["renaming"]["AaA"] == 2 / 5 and "AAAa" in r["renaming"] and r["short_only"] == {}
    assert len(r["all_twelve"]) == 165 and max(len(p) for p in r["all_twelve"]) == 24   # (276 sub-sequences, many of one pattern)
    assert len(r["ragged_03"]) == 28 and len(r["ragged_05"]) == 10
    for acts, lens, support, want, counts in records.values():   # by falling count, and the values are count / n
        assert list(counts) == sorted(counts, reverse=True) and [c / len(lens) for c in counts] == [v for _, v in want]


def test_the_plain_restatement_reproduces_every_recorded_result(records):
    for k, (acts, lens, support, want, _) in records.items():
        if k.startswith("ragged"):
            continue   # (cubic in a sequence's length: the 300 moves are the model's and the kernels' to mine)
        got = pm.mine_plain([acts[s, :lens[s]].tolist() for s in range(len(lens))], support)
        assert list(got.items()) == want, k
    assert pm.mine_plain([], 0.5) == {}


def test_the_model_of_the_launches_reproduces_every_recorded_result(records):
    for k, (acts, lens, support, want, _) in records.items():
        assert list(pm.mine_model(acts, lens, support).items()) == want, k
    assert pm.mine_model(np.zeros((0, 1), dtype=np.uint8), np.zeros(0, dtype=np.int64), 0.5) == {}


def test_pruning_stops_the_levels_early(records):
    acts, lens = records["ragged_03"][:2]
    b = pm.Batch(acts, lens, pm.min_count(len(lens), 0.3))
    b.begin()
    assert b.live == int(np.maximum(lens - 1, 0).sum())
    levels = 0
    while b.live > 0:
        b.next_level()
        b.extend()
        b.close()
        levels += 1
    assert 1 + levels < 20 < lens.max()   # the 200 equal moves and the 300 of three symbols end long before their own lengths


def _supports(n):
    out = [0, 1, 1.5, 1 / 3, 0.3, 2 / n, -0.1]
    for c in range(n + 2):
        out += [c / n, np.nextafter(c / n, 2), np.nextafter(c / n, -1)]
    return out


def test_min_count_is_the_threshold_of_count_over_n():
    from librubiks.analysis import pattern_mining as mining
    for n in range(1, 65):
        for support in _supports(n):
            m = mining.min_count(n, support)
            assert m == pm.min_count(n, support) and 0 <= m <= n + 1
            assert all((c >= m) == (c / n >= support) for c in range(n + 1)), (n, support)
    assert mining.min_count(12, 0.3) == 4 and mining.min_count(12, 1 / 12) == 1 and mining.min_count(12, 1.5) == 13 and mining.min_count(3, 1 / 3) == 1
