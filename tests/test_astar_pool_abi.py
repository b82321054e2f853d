"""
CPU checks of the two A* entry points behind continuous batching (rc_astar_plant, rc_astar_solutions): argument errors are
reported before anything is launched, so they need no GPU, and the ABI version stays where callers built against it expect it.
"""
import ctypes

import pytest

import conftest  # noqa: F401  (puts the package on sys.path)

RC_ERR_NULL, RC_ERR_ALIGN, RC_ERR_RANGE = -1, -2, -4


@pytest.fixture(scope="module")
def lib():
    from librubiks import _hip
    from librubiks.solving import astar_device  # noqa: F401  (registers the rc_astar_* signatures)
    return _hip.load()


def _struct(B=4, C=1201, N=100):
    """A well-formed rc_astar_t whose pointers name no memory: every call below must fail its checks before it would use them."""
    from librubiks.solving.astar_device import _AsStruct
    s = _AsStruct()
    s.n_problems, s.capacity, s.expansions = B, C, N
    s.hash_size = 1 << (2 * (C + 1) - 1).bit_length()
    for i, (name, _) in enumerate(_AsStruct._fields_[4:]):
        setattr(s, name, 0x1000 * (i + 1))
    return s


def test_abi_version_stays_10(lib):
    assert lib.rc_abi_version() == 10


def test_plant_rejects_bad_arguments_without_a_launch(lib):
    s, p = _struct(), ctypes.c_void_p(0x10000)
    assert lib.rc_astar_plant(None, p, 1, p, 16, 0, None) == RC_ERR_NULL
    assert lib.rc_astar_plant(ctypes.byref(s), None, 1, p, 16, 0, None) == RC_ERR_NULL
    assert lib.rc_astar_plant(ctypes.byref(s), None, 0, p, 16, 0, None) == RC_ERR_NULL
    assert lib.rc_astar_plant(ctypes.byref(s), p, 1, None, 16, 0, None) == RC_ERR_NULL
    assert lib.rc_astar_plant(ctypes.byref(s), p, 1, ctypes.c_void_p(0x10004), 16, 0, None) == RC_ERR_ALIGN
    assert lib.rc_astar_plant(ctypes.byref(s), p, 1, p, 24, 0, None) == RC_ERR_ALIGN
    assert lib.rc_astar_plant(ctypes.byref(s), p, 5, p, 16, 0, None) == RC_ERR_RANGE        # more slots than problems
    assert lib.rc_astar_plant(ctypes.byref(s), p, 2, p, 16, 15, None) == RC_ERR_RANGE       # columns beyond the stride
    s.keys = None
    assert lib.rc_astar_plant(ctypes.byref(s), p, 1, p, 16, 0, None) == RC_ERR_NULL


def test_solutions_rejects_bad_arguments_without_a_launch(lib):
    s, p = _struct(), ctypes.c_void_p(0x10000)
    assert lib.rc_astar_solutions(None, p, 1, p, 64, p, None) == RC_ERR_NULL
    assert lib.rc_astar_solutions(ctypes.byref(s), None, 1, p, 64, p, None) == RC_ERR_NULL
    assert lib.rc_astar_solutions(ctypes.byref(s), None, 0, p, 64, p, None) == RC_ERR_NULL
    assert lib.rc_astar_solutions(ctypes.byref(s), p, 1, None, 64, p, None) == RC_ERR_NULL
    assert lib.rc_astar_solutions(ctypes.byref(s), p, 1, p, 64, None, None) == RC_ERR_NULL
    assert lib.rc_astar_solutions(ctypes.byref(s), p, 1, p, 0, p, None) == RC_ERR_RANGE     # width 0
    s.capacity = 5                                                                              # < 12 N + 1
    assert lib.rc_astar_solutions(ctypes.byref(s), p, 1, p, 64, p, None) == RC_ERR_RANGE

