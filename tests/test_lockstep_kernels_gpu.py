"""
The kernels of the lock-step agents (csrc/rubiks_egvm.hip, csrc/rubiks_rollout.hip) against the NumPy model of their six entry
points (tests/lockstep_model.py, pinned to the oracle's agents by tests/test_lockstep_model.py), launch by launch through the C
ABI: after every launch all arrays of the struct are copied back and must be the model's bit for bit -- floats as uint32, so NaNs
and the sign of zero compare; columns beyond the rows of a plane are padding -- and every guard byte around them must still be the
sentinel.  Nothing is tolerated and no row is left out.

The launches are the seeded scenarios of the model module: heads from a palette that is exact in bf16 (-inf, -2, -0.0, 0.0, 0.5,
3, +inf, and in about half the rounds NaN on about 2 % of the rows), decision bytes that mix the policy with actions, roots one or two moves from solved
whose chosen workers are led to the solved cube at chosen depths, narrow queue rows, max_states on the boundary, slots planted
again from column 16 of a table of roots with -1 and S in the list, and rounds that go on after games have ended.  Which branch
decided what is counted by the model and asserted per case (the seeds were chosen on the CPU, where the same assertions run).
The children and solved flags the rollout kernels write are the model's, which takes them from oracle.cube.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import conftest  # noqa: E402,F401
import lockstep_model as lm  # noqa: E402


def dev(a: np.ndarray) -> torch.Tensor:
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:   # (bf16 bit patterns)
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def roots_table(roots: np.ndarray, first_col: int) -> torch.Tensor:
    """[20, stride] int8 with roots[i] in column first_col + i; the other columns hold a state nobody may plant."""
    n = len(roots)
    soa = np.full((20, (first_col + n + 15) // 16 * 16 + 16), 23, dtype=np.int8)
    soa[:, first_col:first_col + n] = roots.T
    return dev(soa)


def check_after(i: int, launch: dict, model, arena):
    torch.cuda.synchronize()
    wrong = model.differences(arena.read())
    what = {k: v for k, v in launch.items() if k in ("op", "d", "first_col", "max_states", "max_steps", "bf16")}
    assert not wrong, f"launch {i} {what}: {wrong} differ from the model"


@pytest.mark.parametrize("head_kind", list(lm.EGVM_HEADS))
@pytest.mark.parametrize("case", list(lm.EGVM_CASES), ids=lambda c: "S%d_W%d_D%d" % c)
def test_egvm_kernels_equal_the_model_after_every_launch(case, head_kind):
    from librubiks import _hip
    lib, stream = _hip.lib(), _hip.stream_ptr()
    S, W, D = case
    narrow, wanted = lm.EGVM_CASES[case]
    ld, bf16 = lm.EGVM_HEADS[head_kind]
    Q = D + 1 if narrow else 3 * D + 2
    stride = (S * W + 15) // 16 * 16 + (16 if narrow else 0)   # the smallest the header allows, and one with room to spare
    arena, struct = lm.egvm_arena(S, W, D, Q, stride)
    e = ctypes.byref(struct)
    m = lm.EgvmModel(S, W, D, Q)
    for i, launch in enumerate(lm.egvm_scenario(m, lm.EGVM_SEEDS[case + (head_kind,)], ld)):
        lm.apply_egvm(m, launch, bf16)
        if launch["op"] == "plant":
            slots, table = dev(launch["slots"]), roots_table(launch["roots"], launch["first_col"])
            _hip.check(lib.rc_egvm_plant(e, slots.data_ptr(), len(launch["slots"]), table.data_ptr(), table.shape[1], launch["first_col"],
                                         stream), "rc_egvm_plant")
        elif launch["op"] == "step":
            decisions, head = dev(launch["decisions"]), dev(lm.head_bits(launch["head"], bf16)[0])
            _hip.check(lib.rc_egvm_step(e, launch["d"], decisions.data_ptr(), head.data_ptr(), ld, int(bf16), stream), "rc_egvm_step")
        else:
            values = dev(launch["values"])
            _hip.check(lib.rc_egvm_round_end(e, values.data_ptr(), launch["max_states"], stream), "rc_egvm_round_end")
        check_after(i, launch, m, arena)
    missing = [k for k in wanted if m.count[k] < 1]
    assert not missing, (missing, dict(m.count))
    print(f"{case} {head_kind}: {i + 1} launches,", dict(m.count))


@pytest.mark.parametrize("kind", ["value", "policy"])
@pytest.mark.parametrize("S,Q", lm.ROLLOUT_CASES)
def test_rollout_kernels_equal_the_model_after_every_launch(kind, S, Q):
    """Value runs plant with children, policy runs without: there kids_soa and kid_solved must stay the sentinel throughout."""
    from librubiks import _hip
    lib, stream = _hip.lib(), _hip.stream_ptr()
    arena, struct = lm.rollout_arena(S, Q, (S + 15) // 16 * 16 + (16 if Q == 2 else 0))
    r = ctypes.byref(struct)
    m = lm.RolloutModel(S, Q)
    scenario = lm.value_scenario if kind == "value" else lm.policy_scenario
    for i, launch in enumerate(scenario(m, lm.ROLLOUT_SEEDS[kind, S, Q])):
        lm.apply_rollout(m, launch)
        op = launch["op"]
        if op == "plant":
            slots, table = dev(launch["slots"]), roots_table(launch["roots"], launch["first_col"])
            _hip.check(lib.rc_rollout_plant(r, slots.data_ptr(), len(launch["slots"]), table.data_ptr(), table.shape[1], launch["first_col"],
                                            int(launch["with_children"]), stream), "rc_rollout_plant")
        elif op == "flags":
            for index in launch["index"]:
                arena.poke("kid_solved", index, 1)
        elif op == "value":
            values = dev(launch["values"])
            _hip.check(lib.rc_rollout_step_value(r, values.data_ptr(), launch["max_steps"], stream), "rc_rollout_step_value")
        else:
            bf16 = launch["bf16"]
            head = None if launch["head"] is None else dev(lm.head_bits(launch["head"], bf16)[0])
            decisions = None if launch["decisions"] is None else dev(launch["decisions"])
            uniforms = None if launch["uniforms"] is None else dev(launch["uniforms"])
            ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
            _hip.check(lib.rc_rollout_step_policy(r, ptr(head), 0 if head is None else launch["head"].shape[1], int(bf16), ptr(decisions),
                                                  ptr(uniforms), launch["max_steps"], stream), "rc_rollout_step_policy")
        check_after(i, launch, m, arena)
    missing = [k for k in lm.rollout_wanted(kind, S, Q) if m.count[k] < 1]
    assert not missing, (missing, dict(m.count))
    assert m.min_margin >= lm.MARGIN   # no sampled move hung on the last bits of an exponential
    print(f"{kind} S {S} Q {Q}: {i + 1} launches,", dict(m.count))
