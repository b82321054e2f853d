"""
CPU checks of the 6x8x6 tables the library derives at compile time (csrc/rubiks_tables686.h): the 12 x 48 sticker permutation and
the bridge from the 20x24 codes, applied in NumPy and compared with the reference's own 6x8x6 states and outputs
(tests/golden/cube686_golden.npz, written by tests/golden/make_golden_686.py), plus the argument checks of the new entry points
(they fail before anything is launched, so they need no GPU).
"""
import ctypes
import os
import re

import numpy as np
import pytest

import conftest  # noqa: F401  (puts the package on sys.path)
from formula_weights import golden

RC_ERR_NULL, RC_ERR_ALIGN, RC_ERR_STRIDE, RC_ERR_RANGE = -1, -2, -3, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    return golden()


@pytest.fixture(scope="module")
def lib():
    from librubiks import _hip
    return _hip.load()


def test_from2024_gives_the_reference_state_for_every_pair(g):
    from librubiks.cube import cube686
    out = cube686.from2024(g["states2024"])
    assert out.shape == (1027, 6, 8, 6) and out.dtype == np.int8
    assert np.array_equal(out, g["states686"])
    assert np.array_equal(cube686.from2024(g["states2024"][100]), g["states686"][100])
    assert np.array_equal(cube686.from2024(g["states2024"][0]), cube686.get_solved())


def test_every_valid_state_writes_each_sticker_exactly_once(g):
    from librubiks.cube import cube686
    bridge = cube686.get_bridge_table()
    assert bridge.shape == (20, 24, 3, 2) and (bridge[8:, :, 2, 0] == 255).all() and (bridge[:8, :, :, 0] < 48).all()
    s = g["states2024"].astype(int)
    hits = np.zeros((len(s), 48), dtype=int)
    for i in range(20):
        for k in range(3 if i < 8 else 2):
            np.add.at(hits, (np.arange(len(s)), bridge[i, s[:, i], k, 0]), 1)
    assert (hits == 1).all()


def test_every_action_is_the_recorded_permutation(g):
    from librubiks.cube import cube686
    perm = cube686.get_perm_table()
    assert perm.shape == (12, 48)
    for a in range(12):
        assert sorted(perm[a]) == list(range(48)) and (perm[a] != np.arange(48)).sum() == 20   # 8 on the face, 12 around it
        assert np.array_equal(perm[a][perm[a ^ 1]], np.arange(48))                                # the other direction undoes it
    actions = 2 * g["mr_faces"].astype(int) + 1 - g["mr_dirs"].astype(int)
    assert set(actions) == set(range(12))
    colours = g["states686"].reshape(-1, 48, 6)
    out = colours[np.arange(len(colours))[:, None], perm[actions]]
    assert np.array_equal(out.reshape(g["mr_out"].shape), g["mr_out"])
    kids = colours[g["ex_idx"]][:, perm].reshape(-1, 6, 8, 6)     # [parent, action, sticker] = the 12-child expansion
    assert np.array_equal(kids, g["ex_children"])


def test_to2024_inverts_the_bridge(g):
    from librubiks.cube import cube686
    back = cube686.to2024(g["states686"])
    assert back.dtype == np.int8 and np.array_equal(back, g["states2024"])
    assert np.array_equal(cube686.to2024(cube686.from2024(g["states2024"])), g["states2024"])
    assert np.array_equal(cube686.to2024(g["mr_out"][7]), cube686.to2024(g["mr_out"][7:8])[0])
    bad = g["states686"][50].copy()
    bad[0, 0], bad[0, 1] = bad[0, 1].copy(), bad[0, 0].copy()      # a corner sticker and an edge sticker trade places
    if not np.array_equal(bad, g["states686"][50]):
        with pytest.raises(AssertionError):
            cube686.to2024(bad)


def test_as633_agrees_across_the_representations(g):
    from librubiks import cube
    from librubiks.cube import cube686
    for i in list(range(40)) + list(range(40, 1027, 29)):
        assert np.array_equal(cube686.as633(g["states686"][i]), g["as633"][i])
        assert np.array_equal(cube.as633(g["states2024"][i]), g["as633"][i])
    assert np.array_equal(cube686.as69(g["states686"][3]), g["as633"][3].reshape(6, 9))
    assert cube686.stringify(g["states686"][200]) == cube.stringify(g["states2024"][200])


def test_host_helpers(g):
    from librubiks.cube import cube686
    assert cube686.get_oh_shape() == 288 and cube686.shape() == (6, 8, 6) and cube686.get_is2024() is False
    assert np.array_equal(cube686.get_solved(), g["solved"]) and cube686.get_solved().dtype == np.int8
    assert cube686.get_solved() is not cube686.get_solved_instance()
    assert np.array_equal(cube686.repeat_state(g["states686"][40], 3), g["repeat_state"])
    assert cube686.repeat_state(g["solved"]).shape == (12, 6, 8, 6)


def test_header_declares_the_entry_points_with_their_reference_lines(lib):
    from librubiks import _hip
    header = open(os.path.join(ROOT, "include", "rubiks_hip.h")).read()
    names = ["rc686_get_perm_table", "rc686_get_bridge_table", "rc686_aos_to_soa", "rc686_soa_to_aos", "rc686_multi_rotate",
             "rc686_expand12", "rc686_expand12_flags", "rc686_is_solved", "rc686_as_oh_f32", "rc686_as_oh_bf16", "rc686_as_correct_f32",
             "rc686_apply_moves", "rc686_multi_rotate_aos", "rc686_is_solved_aos", "rc686_as_oh_aos_f32", "rc_2024_to_686",
             "rc_as_oh686_from2024_f32", "rc_as_oh686_from2024_bf16", "rc_as_correct_from2024_f32", "rc686_as_correct_oh_f32",
             "rc686_as_correct_oh_bf16"]
    for name in names:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in include/rubiks_hip.h"
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    section = header[header.index("the 6x8x6 representation (csrc/rubiks_env686.hip)"):]
    for cite in ("cube.py:349-361", "cube.py:363-369", "cube.py:372-380", "cube.py:85-89", "model.py:326"):
        assert cite in section
    assert lib.rc_abi_version() == 10   # symbols were only added


def test_entry_points_reject_bad_arguments_without_a_launch(lib):
    p, q = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000)
    odd = ctypes.c_void_p(0x10004)
    for fn in (lib.rc686_as_oh_f32, lib.rc686_as_oh_bf16, lib.rc686_as_correct_f32, lib.rc_as_oh686_from2024_f32,
               lib.rc_as_oh686_from2024_bf16, lib.rc_as_correct_from2024_f32):
        assert fn(None, q, 16, 16, None) == RC_ERR_NULL and fn(p, None, 16, 16, None) == RC_ERR_NULL
        assert fn(odd, q, 16, 16, None) == RC_ERR_ALIGN and fn(p, odd, 16, 16, None) == RC_ERR_ALIGN
        assert fn(p, q, 16, 24, None) == RC_ERR_ALIGN and fn(p, q, 17, 16, None) == RC_ERR_STRIDE
        assert fn(None, None, 0, 0, None) == 0                                # nothing to do
    assert lib.rc_2024_to_686(p, None, 16, 16, 16, None) == RC_ERR_NULL
    assert lib.rc_2024_to_686(p, q, 17, 32, 16, None) == RC_ERR_STRIDE
    assert lib.rc686_multi_rotate(p, None, q, 16, 16, 16, None) == RC_ERR_NULL
    assert lib.rc686_multi_rotate(p, odd, q, 16, 16, 16, None) == RC_ERR_ALIGN
    assert lib.rc686_multi_rotate(p, p, q, 33, 48, 32, None) == RC_ERR_STRIDE
    assert lib.rc686_expand12(p, q, 16, 16, 176, None) == RC_ERR_STRIDE       # 192 children per plane
    assert lib.rc686_expand12_flags(p, q, 16, 16, 192, None, q, None) == RC_ERR_NULL
    assert lib.rc686_expand12_flags(p, q, 16, 16, 192, odd, q, None) == RC_ERR_ALIGN
    assert lib.rc686_is_solved(p, None, 16, 16, None) == RC_ERR_NULL
    assert lib.rc686_apply_moves(p, None, 16, 16, 16, 3, None) == RC_ERR_NULL
    assert lib.rc686_apply_moves(p, q, 16, 16, 8, 3, None) == RC_ERR_STRIDE   # a row of moves shorter than the batch
    assert lib.rc686_aos_to_soa(odd, q, 16, 16, None) == RC_ERR_ALIGN and lib.rc686_soa_to_aos(p, None, 16, 16, None) == RC_ERR_NULL
    assert lib.rc686_multi_rotate_aos(p, p, p, 4, None) == RC_ERR_RANGE       # not in place
    assert lib.rc686_is_solved_aos(None, p, 4, None) == RC_ERR_NULL and lib.rc686_as_oh_aos_f32(p, None, 4, None) == RC_ERR_NULL
    assert lib.rc686_as_correct_oh_f32(None, q, 4, None) == RC_ERR_NULL
    assert lib.rc686_as_correct_oh_f32(ctypes.c_void_p(0x10002), q, 4, None) == RC_ERR_ALIGN
    assert lib.rc686_as_correct_oh_bf16(ctypes.c_void_p(0x10001), q, 4, None) == RC_ERR_ALIGN
    assert lib.rc686_get_perm_table(None) == RC_ERR_NULL and lib.rc686_get_bridge_table(None) == RC_ERR_NULL
