"""
The seven kernels behind rc_bfs_batch_plant and rc_bfs_batch_step (csrc/rubiks_bfs_batch.hip) against the NumPy model of the two
entry points (tests/bfs_batch_model.py, pinned to oracle.agents.BFS by tests/test_bfs_batch_model.py), call by call through the C
ABI.  Every array of rc_bfs_batch_t, scan_tmp included, lives in one guarded arena of sentinel bytes; the words are the sentinel
too except that every status is RC_BFSB_EMPTY, which is all the header asks of the caller.  After every plant and every step the
whole arena is copied back, must be the model's by the rules of bfs_batch_model's docstring -- bit for bit except the hash layout,
which is checked structurally, and scan_tmp, which is not compared -- and every guard byte must still be the sentinel.

Shapes are the smallest at which these kernels can still go wrong: four slots, hash rows of twice the node rows (the smallest the
entry points admit, so probe chains are long and wrap), chunks of 1, 5 and 22 parents (264 rows a slot: a slot's segment spans two
workgroups, and a chunk of one parent sits beside one of 22).  The seeded scenario plays near and far roots with a cap per slot
(0, 1, above what the node rows hold, on a chosen parent of a level, exactly on a chunk boundary), twins in neighbouring slots,
replants over larger tenants from column 16 of a table whose other columns hold the code 23, list entries -1 and S, and a slot
that is never planted while its neighbours work.  The queue-row scenario has rows of one and two bytes with solutions that fill
them and solutions one move longer.  The range-check scenario overwrites words (or one parent / action entry) of one slot between
two steps and requires RC_BFSB_FAILED for that slot and nothing else for anybody; every hand-made value keeps the access it would
cause, were it not checked, within eight rows of the slot's arrays, inside the arena (tests/test_bfs_batch_model.py asserts it).
Which case occurred is counted by the model and asserted per scenario; seeds were chosen on the CPU, where the same assertions run.

Not here: RC_BFSB_GRAPH_DONE needs a whole level without a new state, which no consistent table of a real cube reaches.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import conftest  # noqa: E402,F401
import bfs_batch_model as bm  # noqa: E402


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def roots_table(roots: np.ndarray, first_col: int) -> torch.Tensor:
    """[20, stride] int8 with roots[i] in column first_col + i; the other columns hold a state nobody may plant."""
    n = len(roots)
    soa = np.full((20, (first_col + n + 15) // 16 * 16 + 16), 23, dtype=np.int8)
    soa[:, first_col:first_col + n] = roots.T
    return dev(soa)


def call_on_device(lib, b, arena, m: bm.BfsBatchModel, call: dict, stream):
    from librubiks import _hip
    op = call["op"]
    if op == "plant":
        slots, table, caps = dev(call["slots"]), roots_table(call["roots"], call["first_col"]), dev(call["max_states"].view(np.int32))
        _hip.check(lib.rc_bfs_batch_plant(b, slots.data_ptr(), len(call["slots"]), table.data_ptr(), table.shape[1], call["first_col"],
                                          caps.data_ptr(), stream), "rc_bfs_batch_plant")
    elif op == "step":
        _hip.check(lib.rc_bfs_batch_step(b, stream), "rc_bfs_batch_step")
    else:   # a hand-made entry: words[word][slot], parent[slot][node], action[slot][node]
        i, j = call["index"]
        arena.write(call["name"], i * (m.S if call["name"] == "words" else m.cap) + j, call["value"])
    torch.cuda.synchronize()


def run(m: bm.BfsBatchModel, scenario, wanted):
    from librubiks import _hip
    from librubiks.solving import bfs_batch_device  # noqa: F401  (registers the rc_bfs_batch_* signatures)
    lib, stream = _hip.lib(), _hip.stream_ptr()
    scan_bytes = int(lib.rc_bfs_batch_scan_bytes(m.S, m.C))
    assert scan_bytes > 0
    arena, struct = bm.bfs_batch_arena(m, scan_bytes)
    assert not m.differences(arena.read()), "the arena does not start as the model does"
    b = ctypes.byref(struct)
    for i, call in enumerate(scenario):
        bm.apply(m, call)
        call_on_device(lib, b, arena, m, call, stream)
        wrong = m.differences(arena.read())
        what = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in call.items() if k != "roots"}
        assert not wrong, f"call {i} {what}: {wrong} differ from the model"
    missing = [k for k in wanted if m.count[k] < 1]
    assert not missing, (missing, dict(m.count))
    print(f"S {m.S} C {m.C} capacity {m.cap} Q {m.Q}: {i + 1} calls, arena {arena.nbytes} bytes,", dict(m.count))


@pytest.mark.parametrize("C", list(bm.SHAPES))
def test_bfs_batch_kernels_equal_the_model_after_every_call(C):
    m = bm.make_model(C)
    run(m, bm.seeded_scenario(m, bm.SEEDS[C]), bm.SEEDED_WANTED[C])


@pytest.mark.parametrize("Q", [1, 2])
def test_a_solution_fills_its_queue_row_and_one_move_more_fails_the_slot(Q):
    m = bm.make_model(bm.QUEUE_C, Q)
    run(m, bm.queue_scenario(m), bm.QUEUE_WANTED)


def test_words_and_indices_out_of_range_fail_their_slot_and_nothing_else():
    m = bm.make_model(bm.RANGE_C)
    run(m, bm.range_scenario(m, 77), ("failed_on_words", "failed_on_path", "solution_written", "replanted_over_larger_tenant"))
    assert m.count["failed_on_words"] == len(bm.RUNNING_CORRUPTIONS) and m.count["failed_on_path"] == len(bm.PATH_CORRUPTIONS) - 1
