"""
CPU checks of what lets a grid of (lambda, expansions) settings be searched as one A* pool: the library exports
rc_astar_pop_expand_each / rc_astar_push_relax_each and their ctypes signatures are registered, argument errors are reported before
anything is launched, and `AStar.search_batch` refuses malformed per-game arrays before anything touches the device.
"""
import ctypes

import numpy as np
import pytest

import conftest  # noqa: F401  (puts the package on sys.path)

RC_ERR_NULL, RC_ERR_ALIGN, RC_ERR_RANGE = -1, -2, -4
NEW = ("rc_astar_pop_expand_each", "rc_astar_push_relax_each")


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


def test_the_library_exports_both_entry_points_and_the_abi_version_stays(lib):
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.rc_abi_version() == 10


def test_the_ctypes_signatures_are_registered(lib):
    from ctypes import POINTER, c_uint32, c_void_p
    from librubiks import _hip
    from librubiks.solving.astar_device import _AsStruct
    assert _hip.SIGNATURES["rc_astar_pop_expand_each"] == [POINTER(_AsStruct), c_uint32, c_void_p, c_void_p]
    assert _hip.SIGNATURES["rc_astar_push_relax_each"] == [POINTER(_AsStruct), c_void_p, c_void_p, c_void_p, c_void_p]
    for name in NEW:
        assert list(getattr(lib, name).argtypes) == _hip.SIGNATURES[name] and getattr(lib, name).restype is ctypes.c_int
    # the scalar forms keep theirs
    assert _hip.SIGNATURES["rc_astar_pop_expand"] == [POINTER(_AsStruct), c_uint32, c_void_p]
    assert _hip.SIGNATURES["rc_astar_push_relax"] == [POINTER(_AsStruct), c_void_p, c_void_p, ctypes.c_double, c_void_p]


def test_the_entry_points_reject_bad_arguments_without_a_launch(lib):
    s, p = _struct(), ctypes.c_void_p(0x10000)
    assert lib.rc_astar_pop_expand_each(None, 100, p, None) == RC_ERR_NULL
    assert lib.rc_astar_pop_expand_each(ctypes.byref(s), 100, None, None) == RC_ERR_NULL
    assert lib.rc_astar_pop_expand_each(ctypes.byref(s), 100, ctypes.c_void_p(0x10002), None) == RC_ERR_ALIGN
    assert lib.rc_astar_push_relax_each(None, p, p, p, None) == RC_ERR_NULL
    assert lib.rc_astar_push_relax_each(ctypes.byref(s), None, p, p, None) == RC_ERR_NULL
    assert lib.rc_astar_push_relax_each(ctypes.byref(s), p, None, p, None) == RC_ERR_NULL
    assert lib.rc_astar_push_relax_each(ctypes.byref(s), p, p, None, None) == RC_ERR_NULL
    assert lib.rc_astar_push_relax_each(ctypes.byref(s), p, p, ctypes.c_void_p(0x10004), None) == RC_ERR_ALIGN
    s.capacity = 5                                                                              # < 12 N + 1
    assert lib.rc_astar_pop_expand_each(ctypes.byref(s), 100, p, None) == RC_ERR_RANGE
    assert lib.rc_astar_push_relax_each(ctypes.byref(s), p, p, p, None) == RC_ERR_RANGE


G = 6
MALFORMED = {
    "lambda_wrong_shape": ({"lambda_": np.zeros(G + 1)}, "lambda_"),
    "lambda_two_dimensional": ({"lambda_": np.zeros((G, 1))}, "lambda_"),
    "lambda_nan": ({"lambda_": np.array([0.1, 0.2, np.nan, 0.1, 0.1, 0.1])}, "game 2"),
    "lambda_inf": ({"lambda_": np.array([0.1, 0.2, 0.1, 0.1, np.inf, 0.1])}, "game 4"),
    "lambda_minus_inf_scalar": ({"lambda_": -np.inf}, "game 0"),
    "expansions_wrong_shape": ({"expansions": np.ones(G - 1, dtype=int)}, "expansions"),
    "expansions_zero": ({"expansions": np.array([1, 2, 3, 0, 5, 6])}, "game 3"),
    "expansions_negative": ({"expansions": np.array([1, -2, 3, 4, 5, 6])}, "game 1"),
    "expansions_non_integer": ({"expansions": np.array([1, 2, 3, 4, 5, 6.5])}, "game 5"),
    "expansions_nan": ({"expansions": np.array([np.nan, 2, 3, 4, 5, 6])}, "game 0"),
    "expansions_zero_scalar": ({"expansions": 0}, "game 0"),
    "expansions_too_large": ({"expansions": np.array([1, 2, 2 ** 31, 4, 5, 6])}, "game 2"),
    "both_and_lambda_bad": ({"lambda_": np.array([0.1] * 5 + [np.nan]), "expansions": np.arange(1, G + 1)}, "game 5"),
}


@pytest.mark.parametrize("case", list(MALFORMED))
def test_malformed_per_game_arrays_raise_before_a_device_call(case, monkeypatch):
    from librubiks.cube.device import DeviceCubes
    from librubiks.solving.agents import AStar

    def no_device(*a, **k):
        raise AssertionError("the device was touched before the arrays were checked")
    monkeypatch.setattr(DeviceCubes, "of", classmethod(no_device))
    monkeypatch.setattr(AStar, "_batch_for", no_device)
    kwargs, names = MALFORMED[case]
    agent = AStar(None, lambda_=0.2, expansions=4)
    with pytest.raises(ValueError, match=names):
        agent.search_batch(np.zeros((G, 20), dtype=np.int8), None, 1000, **kwargs)


def test_well_formed_arrays_pass_the_check():
    from librubiks.solving.agents import AStar
    agent = AStar(None, lambda_=0.25, expansions=4)
    assert agent._per_game(G, None, None) is None
    lam, n_exp = agent._per_game(G, None, np.array([1.0, 2, 3, 4, 5, 6]))      # integral floats are integers
    assert lam.dtype == np.float64 and lam.tolist() == [0.25] * G and n_exp.dtype == np.int32 and n_exp.tolist() == [1, 2, 3, 4, 5, 6]
    lam, n_exp = agent._per_game(G, 0, None)
    assert lam.tolist() == [0.0] * G and n_exp.tolist() == [4] * G
    assert AStar.sweep_parameters == ("lambda_", "expansions")
