"""
rc_astar_pop_expand_each / rc_astar_push_relax_each (csrc/rubiks_astar.hip) launch by launch through the C ABI, in the guarded
arena of tests/astar_model.py: problem b of a batch with the staging stride Nmax must evolve exactly as the single problem of its
own AStarModel(1, N_b, C, ...) fed the same root, the same values and lambda[b] (tests/astar_each_model.py).  After every launch the
whole arena is copied back; every model's `differences` runs on its problem's slices (all C + 1 node rows, the scalars,
popped[:N_b], the staging rows [:12 N_b], the hash row, the open list), popped[N_b:] and the staging rows [12 N_b:] must be what
they were, and every guard byte must be the sentinel.  Nothing is tolerated.

B 4 with N (1, 22, 2, 22) -- 264 child rows, a second pass of the 256-thread stride, and a 1 beside a 22, so that a kernel which
takes the count for the stride or the stride for the count reads its neighbour -- lambda (0.0, 0.2, 1.0, 0.5), values from the
palette that makes costs tie, hash rows of the smallest legal size, one launch in which a problem runs at n + 12 N_b == max_states
while another is exhausted at max_states + 1, capacity reached, a slot planted again with another (lambda, N).  The clamp case
hands the kernel Nmax + 1 for problem 1, then 0 for problem 2, then -1 for problem 0.  Which case occurred is counted by the models and asserted
(the seeds were chosen on the CPU: tests/test_astar_each_model.py).
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import conftest  # noqa: E402,F401
import astar_each_model as em  # noqa: E402
import astar_model as am  # noqa: E402


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def roots_table(roots: np.ndarray, first_col: int) -> torch.Tensor:
    """[20, stride] int8 with roots[i] in column first_col + i; the other columns hold a state nobody may plant."""
    n = len(roots)
    soa = np.full((20, (first_col + n + 15) // 16 * 16 + 16), 23, dtype=np.int8)
    soa[:, first_col:first_col + n] = roots.T
    return dev(soa)


def launch_on_device(lib, a, launch: dict, stream):
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
        each = dev(launch["expansions"].astype(np.int32))
        _hip.check(lib.rc_astar_pop_expand_each(a, launch["max_states"], each.data_ptr(), stream), "rc_astar_pop_expand_each")
    else:
        offset, values = dev(launch["new_offset"]), dev(np.concatenate([launch["values"], np.zeros(1, dtype=np.float32)]))
        lambdas = dev(launch["lambda"].astype(np.float64))
        _hip.check(lib.rc_astar_push_relax_each(a, offset.data_ptr(), values.data_ptr(), lambdas.data_ptr(), stream),
                   "rc_astar_push_relax_each")
    torch.cuda.synchronize()


def run(scenario, seed: int, wanted) -> em.EachPool:
    from librubiks import _hip
    lib, stream = _hip.lib(), _hip.stream_ptr()
    pool = em.EachPool()
    arena, struct = am.astar_arena(pool.shell)
    assert (struct.n_problems, struct.expansions, struct.hash_size) == (4, 22, am.min_hash_size(pool.C))
    a = ctypes.byref(struct)
    for i, launch in enumerate(scenario(pool, seed)):
        pool.apply(launch)
        launch_on_device(lib, a, launch, stream)
        wrong = pool.differences(arena.read())   # (raises if a guard byte changed)
        what = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in launch.items() if k in ("op", "max_states", "expansions", "lambda", "slots", "N", "lam")}
        assert not wrong, f"launch {i} {what}: {wrong} differ from the models"
    count = pool.counters()
    missing = [k for k in wanted if count[k] < 1]
    assert not missing, (missing, dict(count))
    print(f"{i + 1} launches, arena {arena.nbytes} bytes,", dict(count))
    return pool


def test_each_problem_evolves_as_its_own_single_problem_model():
    pool = run(em.seeded_scenario, em.SEED, em.WANTED)
    assert pool.N[em.REPLANT["slot"]] == em.REPLANT["N"]


def test_expansions_are_read_clamped_to_the_staging_stride():
    pool = run(em.clamp_scenario, em.CLAMP_SEED, em.CLAMP_WANTED)
    assert pool.models[2].status[0] == pool.models[0].status[0] == am.OPEN_EMPTY and pool.models[1].status[0] != am.OPEN_EMPTY
