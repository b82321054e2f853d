"""
CPU checks of the device entry points behind the pooled BFS (rc_bfs_batch_plant, rc_bfs_batch_step): argument errors are reported
before anything is launched, so they need no GPU; the ABI version stays where callers built against it expect it (symbols were only
added); and the host's plan of a batch (`bfs_batch_plan`) respects its byte budget and the 2^31 bound of the row space.
"""
import ctypes

import pytest

import conftest  # noqa: F401  (puts the package on sys.path)

RC_ERR_NULL, RC_ERR_ALIGN, RC_ERR_STRIDE, RC_ERR_RANGE = -1, -2, -3, -4
N_HEAD = 6   # the uint32 fields in front of the pointers


@pytest.fixture(scope="module")
def lib():
    from librubiks import _hip
    from librubiks.solving import bfs_batch_device  # noqa: F401  (registers the rc_bfs_batch_* signatures)
    return _hip.load()


def _struct(S=4, C=8, cap=200, hash_size=512, Q=64, **over):
    """A well-formed rc_bfs_batch_t whose pointers name no memory: every call below must fail its checks before it would use them."""
    from librubiks.solving.bfs_batch_device import _BfsBatchStruct
    s = _BfsBatchStruct()
    s.n_slots, s.chunk, s.capacity, s.hash_size, s.queue_width, s.reserved = S, C, cap, hash_size, Q, 0
    for i, (name, _) in enumerate(_BfsBatchStruct._fields_[N_HEAD:-1]):
        setattr(s, name, 0x1000 * (i + 1))
    s.scan_tmp_bytes = 1024
    for k, v in over.items():
        setattr(s, k, v)
    return s


def _pointer_fields():
    from librubiks.solving.bfs_batch_device import _BfsBatchStruct
    return [name for name, _ in _BfsBatchStruct._fields_[N_HEAD:-1]]


def test_abi_version_stays_10_and_the_entry_points_exist(lib):
    assert lib.rc_abi_version() == 10
    for name in ("rc_bfs_batch_plant", "rc_bfs_batch_step", "rc_bfs_batch_scan_bytes", "rc_bfs_batch_struct_bytes"):
        assert hasattr(lib, name)
    for name in ("rc_bfs_init", "rc_bfs_expand", "rc_bfs_commit", "rc_bfs_path"):   # the serial form keeps its own
        assert hasattr(lib, name)


def test_struct_mirror_has_the_compiled_size(lib):
    from librubiks.solving.bfs_batch_device import _BfsBatchStruct
    assert lib.rc_bfs_batch_struct_bytes() == ctypes.sizeof(_BfsBatchStruct)


def _bad_structs():
    """(struct, code) for every way the batch description itself can be wrong."""
    out = [(_struct(**{name: None}), RC_ERR_NULL) for name in _pointer_fields()]
    out += [(_struct(keys=0x1008), RC_ERR_ALIGN), (_struct(child_keys=0x5004), RC_ERR_ALIGN), (_struct(hash=0x4008), RC_ERR_ALIGN),
            (_struct(words=0x9004), RC_ERR_ALIGN),
            (_struct(S=0), RC_ERR_RANGE), (_struct(C=0), RC_ERR_RANGE), (_struct(Q=0), RC_ERR_RANGE),
            (_struct(hash_size=500), RC_ERR_RANGE),                                # not a power of two
            (_struct(hash_size=256), RC_ERR_RANGE),                                # < 2 * capacity
            (_struct(cap=12 * 8 + 1), RC_ERR_RANGE),                               # no room for one state beside a chunk's children
            (_struct(cap=2 ** 30, hash_size=2 ** 31), RC_ERR_RANGE),               # 32-bit hash cells
            (_struct(S=2 ** 16, C=2731, cap=2 ** 16, hash_size=2 ** 17), RC_ERR_RANGE),   # S 12 C = 2^31 + 2^17
            (_struct(S=2 ** 31 // 12 + 1, C=1), RC_ERR_RANGE)]
    return out


def test_the_largest_row_space_is_accepted_by_the_checks(lib):
    """S 12 C = 2^31 - 8 passes the struct checks (the call then fails on its own arguments, still before any launch)."""
    s = _struct(S=(2 ** 31 - 8) // 12, C=1)
    assert lib.rc_bfs_batch_plant(ctypes.byref(s), None, 1, None, 16, 0, None, None) == RC_ERR_NULL


def test_step_rejects_bad_arguments_without_a_launch(lib):
    assert lib.rc_bfs_batch_step(None, None) == RC_ERR_NULL
    for bad, code in _bad_structs():
        assert lib.rc_bfs_batch_step(ctypes.byref(bad), None) == code


def test_plant_rejects_bad_arguments_without_a_launch(lib):
    s, p = _struct(), ctypes.c_void_p(0x10000)
    plant = lambda st=s, slots=p, n=1, roots=p, stride=16, first=0, caps=p: lib.rc_bfs_batch_plant(   # noqa: E731
        None if st is None else ctypes.byref(st), slots, n, roots, stride, first, caps, None)
    assert plant(st=None) == RC_ERR_NULL
    assert plant(slots=None) == RC_ERR_NULL and plant(roots=None) == RC_ERR_NULL and plant(caps=None) == RC_ERR_NULL
    assert plant(slots=None, n=0) == RC_ERR_NULL
    assert plant(roots=ctypes.c_void_p(0x10004)) == RC_ERR_ALIGN
    assert plant(stride=24) == RC_ERR_ALIGN
    assert plant(caps=ctypes.c_void_p(0x10002)) == RC_ERR_ALIGN and plant(slots=ctypes.c_void_p(0x10001)) == RC_ERR_ALIGN
    assert plant(n=5) == RC_ERR_RANGE                       # more list entries than slots
    assert plant(n=2, first=15) == RC_ERR_RANGE             # columns beyond the stride
    assert plant(n=1, first=17) == RC_ERR_RANGE
    assert plant(n=1, first=2 ** 64 - 1) == RC_ERR_RANGE    # (no wrap-around in first + n)
    for bad, code in _bad_structs():
        assert plant(st=bad) == code


def test_scan_bytes_refuses_a_row_space_of_2_31(lib):
    assert lib.rc_bfs_batch_scan_bytes(0, 8) == 0 and lib.rc_bfs_batch_scan_bytes(8, 0) == 0
    assert lib.rc_bfs_batch_scan_bytes(2 ** 16, 2731) == 0


# ---- the host's plan ---------------------------------------------------------------------------------------------------------
def test_plan_shapes_a_slot_as_the_kernels_need_it():
    from librubiks.solving.bfs_batch_device import bfs_batch_plan
    S, C, cap, hs, total = bfs_batch_plan(24, 2000, 3, 37)
    assert (S, C, cap) == (3, 37, 2000 + 12 * 37 + 1)
    assert hs & (hs - 1) == 0 and hs >= 2 * cap and hs < 4 * cap
    assert total == 3 * (cap * 21 + hs * 4 + 12 * 37 * 28 + 14 * 8 + 64)
    assert bfs_batch_plan(24, 5, None, 1024)[1] == 5                      # a level has fewer parents than max_states
    assert bfs_batch_plan(24, 1, 1, 1)[2] == 14 and bfs_batch_plan(24, 1, 1, 1)[3] == 32


def test_plan_clamps_the_slots_to_the_games_and_to_the_budget():
    from librubiks.solving import agents
    from librubiks.solving.bfs_batch_device import bfs_batch_plan, slot_shape
    assert agents.BFS_BATCH_BYTES == 32 << 30 == agents.ASTAR_TIME_ONLY_BYTES
    assert bfs_batch_plan(24, 2000, 100, 16)[0] == 24 and bfs_batch_plan(24, 2000, None, 16)[0] == 24
    per_slot = slot_shape(175_000, 64)[2]
    for slots in (None, 10 ** 6):
        S, C, cap, hs, total = bfs_batch_plan(10 ** 6, 175_000, slots, 64)
        assert S == agents.BFS_BATCH_BYTES // per_slot and total == S * per_slot <= agents.BFS_BATCH_BYTES < (S + 1) * per_slot
    assert bfs_batch_plan(100, 2000, None, 16, budget=5 * slot_shape(2000, 16)[2] + 1)[0] == 5
    with pytest.raises(ValueError, match="one slot"):
        bfs_batch_plan(100, 2000, None, 16, budget=slot_shape(2000, 16)[2] - 1)
    with pytest.raises(ValueError):
        bfs_batch_plan(0, 2000, None, 16)
    with pytest.raises(ValueError):
        bfs_batch_plan(10, 2000, 0, 16)


def test_plan_caps_max_states_and_keeps_the_row_space_below_2_31():
    from librubiks.solving import agents
    from librubiks.solving.bfs_batch_device import bfs_batch_plan
    S, C, cap, hs, total = bfs_batch_plan(3, int(1e10), None, 1024)     # what `Agent.reset` hands on for "no limit"
    assert cap == agents.bd_MAX_STATES + 12 * 1024 + 1 and 1 <= S <= 3 and total <= agents.BFS_BATCH_BYTES
    for n, ms, c in ((10 ** 9, 1, 1), (10 ** 8, 40, 40), (10 ** 7, 1000, 1000)):
        S, C, _, _, _ = bfs_batch_plan(n, ms, None, c, budget=1 << 62)
        assert S * 12 * C < 2 ** 31 <= (S + 1) * 12 * C
    S, C, cap, _, _ = bfs_batch_plan(3, int(1e10), None, 2 ** 27, budget=1 << 62)   # the largest slot there is: 13 x 2^26 + 1 rows
    assert C == agents.bd_MAX_STATES and cap < 2 ** 30 and S * 12 * C < 2 ** 31
