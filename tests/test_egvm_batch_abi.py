"""
CPU checks of the device entry points behind the batched EGVM search (rc_egvm_step, rc_egvm_round_end, rc_egvm_plant): argument
errors are reported before anything is launched, so they need no GPU, and the ABI version stays where callers built against it
expect it (symbols were only added).
"""
import ctypes

import pytest

import conftest  # noqa: F401  (puts the package on sys.path)

RC_ERR_NULL, RC_ERR_ALIGN, RC_ERR_STRIDE, RC_ERR_RANGE = -1, -2, -3, -4


@pytest.fixture(scope="module")
def lib():
    from librubiks import _hip
    from librubiks.solving import egvm_device  # noqa: F401  (registers the rc_egvm_* signatures)
    return _hip.load()


def _struct(S=4, W=10, D=5, Q=40, **over):
    """A well-formed rc_egvm_t whose pointers name no memory: every call below must fail its checks before it would use them."""
    from librubiks.solving.egvm_device import _EgStruct
    s = _EgStruct()
    s.n_slots, s.workers, s.depth, s.queue_width, s.stride = S, W, D, Q, 256
    for i, (name, _) in enumerate(_EgStruct._fields_[5:]):
        setattr(s, name, 0x1000 * (i + 1))
    for k, v in over.items():
        setattr(s, k, v)
    return s


def _pointer_fields():
    from librubiks.solving.egvm_device import _EgStruct
    return [name for name, _ in _EgStruct._fields_[5:]]


def test_abi_version_stays_10_and_the_entry_points_exist(lib):
    assert lib.rc_abi_version() == 10
    for name in ("rc_egvm_step", "rc_egvm_round_end", "rc_egvm_plant", "rc_egvm_draw"):
        assert hasattr(lib, name)


def _bad_structs():
    """(struct, code) for every way the batch description itself can be wrong."""
    out = [(_struct(**{name: None}), RC_ERR_NULL) for name in _pointer_fields()]
    out += [(_struct(S=0), RC_ERR_RANGE), (_struct(W=0), RC_ERR_RANGE), (_struct(D=0), RC_ERR_RANGE), (_struct(Q=0), RC_ERR_RANGE),
            (_struct(W=0x10000), RC_ERR_RANGE), (_struct(D=0x8001), RC_ERR_RANGE),
            (_struct(rows_soa=0x1004), RC_ERR_ALIGN), (_struct(best_soa=0x2008), RC_ERR_ALIGN), (_struct(stride=264), RC_ERR_ALIGN),
            (_struct(S=30, stride=256), RC_ERR_STRIDE)]                                    # 300 rows need 304 bytes per plane
    return out


def test_step_rejects_bad_arguments_without_a_launch(lib):
    s, p = _struct(), ctypes.c_void_p(0x10000)
    ok = lambda st=s, d=0, dec=p, head=p, ld=13, bf=0: lib.rc_egvm_step(None if st is None else ctypes.byref(st), d, dec, head, ld, bf, None)  # noqa: E731
    assert ok(st=None) == RC_ERR_NULL
    assert ok(dec=None) == RC_ERR_NULL and ok(head=None) == RC_ERR_NULL
    assert ok(head=ctypes.c_void_p(0x10002)) == RC_ERR_ALIGN                                # float rows
    assert ok(head=ctypes.c_void_p(0x10001), bf=1) == RC_ERR_ALIGN
    assert ok(d=5) == RC_ERR_RANGE and ok(d=2 ** 32 - 1) == RC_ERR_RANGE                    # d >= D
    assert ok(ld=12) == RC_ERR_RANGE                                                        # no value column
    for bad, code in _bad_structs():
        assert ok(st=bad) == code


def test_round_end_rejects_bad_arguments_without_a_launch(lib):
    s, p = _struct(), ctypes.c_void_p(0x10000)
    assert lib.rc_egvm_round_end(None, p, 1000, None) == RC_ERR_NULL
    assert lib.rc_egvm_round_end(ctypes.byref(s), None, 1000, None) == RC_ERR_NULL
    assert lib.rc_egvm_round_end(ctypes.byref(s), ctypes.c_void_p(0x10002), 1000, None) == RC_ERR_ALIGN
    for bad, code in _bad_structs():
        assert lib.rc_egvm_round_end(ctypes.byref(bad), p, 1000, None) == code


def test_plant_rejects_bad_arguments_without_a_launch(lib):
    s, p = _struct(), ctypes.c_void_p(0x10000)
    assert lib.rc_egvm_plant(None, p, 1, p, 16, 0, None) == RC_ERR_NULL
    assert lib.rc_egvm_plant(ctypes.byref(s), None, 1, p, 16, 0, None) == RC_ERR_NULL
    assert lib.rc_egvm_plant(ctypes.byref(s), None, 0, p, 16, 0, None) == RC_ERR_NULL
    assert lib.rc_egvm_plant(ctypes.byref(s), p, 1, None, 16, 0, None) == RC_ERR_NULL
    assert lib.rc_egvm_plant(ctypes.byref(s), p, 1, ctypes.c_void_p(0x10004), 16, 0, None) == RC_ERR_ALIGN
    assert lib.rc_egvm_plant(ctypes.byref(s), p, 1, p, 24, 0, None) == RC_ERR_ALIGN
    assert lib.rc_egvm_plant(ctypes.byref(s), p, 5, p, 16, 0, None) == RC_ERR_RANGE        # more slots than S
    assert lib.rc_egvm_plant(ctypes.byref(s), p, 2, p, 16, 15, None) == RC_ERR_RANGE       # columns beyond the stride
    for bad, code in _bad_structs():
        assert lib.rc_egvm_plant(ctypes.byref(bad), p, 1, p, 16, 0, None) == code
