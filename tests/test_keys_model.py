"""
tests/keys_model.py, the NumPy restatement of the packed state keys (csrc/rubiks_keys.h), on the CPU: the packing and key_hash
against values worked out by hand, and the solved key, the child keys and the unpacking against oracle.cube.
"""
import numpy as np

import conftest  # noqa: F401  (puts the package on sys.path)
import astar_model as am
import keys_model as km
from oracle import cube as oc


def _scrambles() -> np.ndarray:
    np.random.seed(5)
    return np.array([oc.get_solved()] + [oc.scramble(d, True)[0] for d in (1, 2, 7, 20, 40)])


def test_packing_and_hash_are_the_headers():
    """Six 5-bit codes a word, and key_hash of csrc/rubiks_keys.h worked out step by step in Python integers."""
    state = np.arange(20, dtype=np.int8) + 3
    w = km.pack_keys(state[None])[0].tolist()
    assert w == [sum(int(state[6 * k + j]) << (5 * j) for j in range(6) if 6 * k + j < 20) for k in range(4)]
    M = (1 << 32) - 1
    h = (w[0] * 0x9E3779B1) & M
    h ^= h >> 15
    h = (h + w[1] * 0x85EBCA77) & M
    h ^= h >> 13
    h = (h + w[2] * 0xC2B2AE3D) & M
    h ^= h >> 16
    h = (h + w[3] * 0x27D4EB2F) & M
    h ^= h >> 15
    h = (h * 0x165667B1) & M
    h ^= h >> 16
    assert int(km.key_hash(np.array([w], dtype=np.uint32))[0]) == h
    assert int(km.home_cell(np.array([w], dtype=np.uint32), 512)[0]) == h & 511
    assert [am.min_hash_size(C) for C in (13, 63, 255, 1023, 2047, 31, 64)] == [32, 128, 512, 2048, 4096, 64, 256]


def test_the_solved_key_is_the_packed_solved_state():
    solved = oc.get_solved()
    assert km.SOLVED_KEY.dtype == np.uint32
    assert km.SOLVED_KEY.tolist() == [sum(int(solved[6 * k + j]) << (5 * j) for j in range(6) if 6 * k + j < 20) for k in range(4)]
    keys = km.pack_keys(_scrambles())
    assert ((keys == km.SOLVED_KEY).all(axis=1) == oc.multi_is_solved(_scrambles())).all()


def test_a_turned_key_is_the_packed_rotated_state():
    states = _scrambles()
    for a, (face, direction) in enumerate(oc.ACTION_SPACE):
        want = km.pack_keys(np.array([oc.rotate(s, face, direction) for s in states]))
        assert np.array_equal(km.turned_keys(km.pack_keys(states), np.full(len(states), a)), want), f"action {a}"
    # one action a key, in the order of expand12
    assert np.array_equal(km.turned_keys(np.repeat(km.pack_keys(states), 12, axis=0), np.tile(np.arange(12), len(states))),
                          km.pack_keys(oc.expand12(states)))


def test_unpacking_undoes_packing():
    from librubiks.solving.keys import unpack_keys
    states = np.concatenate([_scrambles(), np.arange(20, dtype=np.int8)[None] + 4, np.full((1, 20), 23, dtype=np.int8)])
    back = unpack_keys(km.pack_keys(states))
    assert back.dtype == np.int8 and np.array_equal(back, states)
