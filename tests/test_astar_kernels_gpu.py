"""
The six rc_astar_* kernels (csrc/rubiks_astar.hip) against the NumPy model of their entry points (tests/astar_model.py, pinned to
oracle.agents.AStar by tests/test_astar_model.py), launch by launch through the C ABI: every array of rc_astar_t, the gathered
network input and the solutions table live in one guarded arena of sentinel bytes (claim INT32_MAX, the hash rows zero, as
AStarBatch hands them over); after every launch the whole arena is copied back, must be the model's by the rules of
astar_model's docstring -- bit for bit except the hash layout and the open list's order in memory, which are checked structurally
-- and every guard byte must still be the sentinel.  Nothing is tolerated, no row is left out.

The launches are the scenarios of the model module.  Seeded: roots one to three moves from solved (and some far from it), values
from a palette that makes costs collide exactly, max_states on and one beyond the bound, capacity reached, hash rows of the
smallest legal size, queues read with a table one byte wide and a list that holds -1 and B, slots planted again from column 16 of
a table whose other columns hold the code 23, former tenants' rows above the new n_nodes, a pop after every problem has ended.
Queues are read twice, with rows of one byte and with rows that hold the longest queue.  Scripted: searches led state by state into
both relaxation passes, their elections, a win with relaxations pending, two parents with one new child, an open list emptied by
hand, and (N 22, 264 child rows) pushes in which a row of the lanes' second pass must decide on the G it gathered although a row
of another wave lowers that G in the same relaxation pass -- once in case 1, once in case 2.  Every index handed to a kernel is in
range; the list entries -1 and B are those the header defines as skipped.  Which branch decided what is counted by the model and asserted per case (seeds and scripts were
chosen on the CPU, where the same assertions run).
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import conftest  # noqa: E402,F401
import astar_model as am  # noqa: E402


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def roots_table(roots: np.ndarray, first_col: int) -> torch.Tensor:
    """[20, stride] int8 with roots[i] in column first_col + i; the other columns hold a state nobody may plant."""
    n = len(roots)
    soa = np.full((20, (first_col + n + 15) // 16 * 16 + 16), 23, dtype=np.int8)
    soa[:, first_col:first_col + n] = roots.T
    return dev(soa)


def launch_on_device(lib, a, arena, launch: dict, stream):
    from librubiks import _hip
    op = launch["op"]
    if op == "init":
        table = roots_table(launch["roots"], 0)
        _hip.check(lib.rc_astar_init(a, table.data_ptr(), table.shape[1], stream), "rc_astar_init")
    elif op == "plant":
        slots, table = dev(launch["slots"]), roots_table(launch["roots"], launch["first_col"])
        _hip.check(lib.rc_astar_plant(a, slots.data_ptr(), len(launch["slots"]), table.data_ptr(), table.shape[1], launch["first_col"],
                                      stream), "rc_astar_plant")
    elif op == "pop":
        _hip.check(lib.rc_astar_pop_expand(a, launch["max_states"], stream), "rc_astar_pop_expand")
    elif op == "gather":
        arena.write("out_soa", slice(None), am.FILL_I8)
        assert 20 * launch["stride"] <= arena.layout["out_soa"][1] and launch["new_offset"][-1] <= launch["stride"]
        offset = dev(launch["new_offset"])
        _hip.check(lib.rc_astar_gather_new(a, offset.data_ptr(), arena.ptr("out_soa"), launch["stride"], stream), "rc_astar_gather_new")
    elif op == "push":
        offset, values = dev(launch["new_offset"]), dev(np.concatenate([launch["values"], np.zeros(1, dtype=np.float32)]))
        _hip.check(lib.rc_astar_push_relax(a, offset.data_ptr(), values.data_ptr(), launch["lambda"], stream), "rc_astar_push_relax")
    elif op == "solutions":
        arena.write("queues", slice(None), am.FILL)
        arena.write("lengths", slice(None), int(am.filled((1,), np.int32)[0]))
        problems = dev(launch["problems"])
        assert len(launch["problems"]) * launch["width"] <= arena.layout["queues"][1]
        _hip.check(lib.rc_astar_solutions(a, problems.data_ptr(), len(launch["problems"]), arena.ptr("queues"), launch["width"],
                                          arena.ptr("lengths"), stream), "rc_astar_solutions")
    else:
        arena.write(launch["name"], launch["index"], launch["value"])
    torch.cuda.synchronize()


def run(m: am.AStarModel, scenario, wanted):
    from librubiks import _hip
    lib, stream = _hip.lib(), _hip.stream_ptr()
    arena, struct = am.astar_arena(m)
    a = ctypes.byref(struct)
    for i, launch in enumerate(scenario):
        am.apply(m, launch)
        launch_on_device(lib, a, arena, launch, stream)
        wrong = m.differences(arena.read())
        what = {k: v for k, v in launch.items() if k in ("op", "max_states", "stride", "lambda", "width", "first_col", "name", "index")}
        assert not wrong, f"launch {i} {what}: {wrong} differ from the model"
    missing = [k for k in wanted if m.count[k] < 1]
    assert not missing, (missing, dict(m.count))
    print(f"B {m.B} N {m.N} C {m.C}: {i + 1} launches, arena {arena.nbytes} bytes,", dict(m.count))


@pytest.mark.parametrize("li", range(len(am.LAMBDAS)), ids=["lambda_%g" % x for x in am.LAMBDAS])
@pytest.mark.parametrize("case", list(am.SEEDED_CASES), ids=lambda c: "B%d_N%d_C%d" % c)
def test_astar_kernels_equal_the_model_after_every_launch(case, li):
    lam = am.LAMBDAS[li]
    m = am.make_model(*case, am.SLACK[lam])
    run(m, am.seeded_scenario(m, am.SEEDS[case][li], lam, am.SLACK[lam]), am.SEEDED_WANTED[case])


@pytest.mark.parametrize("lam", am.LAMBDAS)
@pytest.mark.parametrize("N", list(am.SCRIPTED_CASES))
def test_astar_kernels_equal_the_model_on_the_scripted_searches(N, lam):
    m = am.scripted_model(N, am.SLACK[lam])
    run(m, am.scripted_scenario(m, lam, am.SLACK[lam]), am.scripted_wanted(N))
