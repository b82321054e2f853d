"""`plan_chunks` of librubiks/solving/shorten.py: a pure function of the queue lengths and the budget."""
import numpy as np
import pytest

import conftest  # noqa: F401
import shorten_model as sm


def _check(lengths, budget):
    from librubiks.solving.shorten import plan_chunks, table_cells, workspace_bytes
    chunks = plan_chunks(lengths, budget)
    L = np.asarray(lengths, dtype=np.int64)
    assert [lo for lo, _ in chunks] == [0] + [hi for _, hi in chunks[:-1]] and chunks[-1][1] == len(L)   # every game once, in order
    for lo, hi in chunks:
        assert hi > lo
        P, H = int(np.where(L[lo:hi] < 0, 0, L[lo:hi] + 1).sum()), int(table_cells(L[lo:hi]).sum())
        assert workspace_bytes(P, H) <= budget
        if hi < len(L):   # greedy: the next game would not have fitted
            P2, H2 = P + max(0, int(L[hi]) + 1), H + int(table_cells(L[hi:hi + 1])[0])
            assert workspace_bytes(P2, H2) > budget
    return chunks


def test_table_cells_is_the_models():
    from librubiks.solving.shorten import table_cells
    Ls = [0, 1, 2, 3, 4, 5, 7, 8, 1022, 1023, 1024, 174_999, 175_000, (1 << 20) - 1, 1 << 20, (1 << 27) - 2]
    assert list(table_cells(Ls)) == [sm.table_cells(L) for L in Ls]
    assert list(table_cells([-1, 3, -5])) == [0, 8, 0]


def test_chunks_cover_every_game_once_in_order_within_budget():
    rng = np.random.RandomState(0)
    lengths = rng.randint(0, 3000, 500)
    lengths[rng.rand(500) < 0.2] = -1                 # games that are left alone cost nothing
    assert _check(lengths, 1 << 40) == [(0, 500)]
    for budget in (1 << 24, 1 << 22, 400_000):
        assert len(_check(lengths, budget)) > 1
    # 2 500 games of 175 000 moves do not fit at once: ~100 B per position
    big = np.full(2500, 175_000)
    chunks = _check(big, 2 << 30)
    assert len(chunks) > 10 and all(hi - lo == chunks[0][1] - chunks[0][0] for lo, hi in chunks[:-1])


def test_a_game_larger_than_the_budget_raises_and_names_it():
    from librubiks.solving.shorten import plan_chunks
    with pytest.raises(ValueError, match="game 2"):
        plan_chunks([10, 20, 100_000, 5], 1 << 20)


def test_empty_input():
    from librubiks.solving.shorten import plan_chunks
    assert plan_chunks([], 1 << 20) == []
    assert plan_chunks(np.zeros(0, dtype=np.int64)) == []
    assert plan_chunks([-1, -1], 1 << 10) == [(0, 2)]
