"""
The NumPy restatement of csrc/rubiks_keys.h that the search models and GPU tests share: the 5-bit packing of a cube state into four
words, key_hash, a key's home cell in a table, the key of a child, and the check of a linear-probing table.  NumPy and oracle.cube
only; tests/test_keys_model.py pins it to values worked out by hand and to oracle.cube.
"""
import numpy as np

from oracle import cube as oc


def pack_keys(states: np.ndarray) -> np.ndarray:
    """[n, 20] codes -> uint32 [n, 4]: 5 bits a code, six codes a word (cubies 0-5, 6-11, 12-17, 18-19)."""
    codes = states.astype(np.int64).astype(np.uint32) & np.uint32(31)
    w = np.zeros((len(states), 4), dtype=np.uint32)
    for j in range(20):
        w[:, j // 6] |= codes[:, j] << np.uint32(5 * (j % 6))
    return w


SOLVED_KEY = pack_keys(oc.get_solved()[None])[0]


def key_hash(w: np.ndarray) -> np.ndarray:
    """key_hash on uint32 [n, 4], modulo 2^32."""
    w = w.astype(np.uint32)
    with np.errstate(over="ignore"):
        h = w[:, 0] * np.uint32(0x9E3779B1)
        h ^= h >> np.uint32(15)
        h += w[:, 1] * np.uint32(0x85EBCA77)
        h ^= h >> np.uint32(13)
        h += w[:, 2] * np.uint32(0xC2B2AE3D)
        h ^= h >> np.uint32(16)
        h += w[:, 3] * np.uint32(0x27D4EB2F)
        h ^= h >> np.uint32(15)
        h *= np.uint32(0x165667B1)
        h ^= h >> np.uint32(16)
    return h


def home_cell(w: np.ndarray, cells: int) -> np.ndarray:
    """Where the probe for each key of uint32 [n, 4] starts in a table of `cells` (a power of two) cells: int64 [n]."""
    return (key_hash(w) & np.uint32(cells - 1)).astype(np.int64)


def turned_keys(w: np.ndarray, actions: np.ndarray) -> np.ndarray:
    """key_turned: the keys of uint32 [n, 4] after actions [n], code by code through oracle.cube's move table."""
    w, a = w.astype(np.uint32), np.asarray(actions).astype(np.int64)
    out = np.zeros_like(w)
    for j in range(20):
        code = (w[:, j // 6] >> np.uint32(5 * (j % 6))) & np.uint32(31)
        out[:, j // 6] |= oc._LUT[a, oc.KIND[j], code].astype(np.uint32) << np.uint32(5 * (j % 6))
    return out


def check_hash_table(table: np.ndarray, keys: np.ndarray, n: int):
    """The linear-probing table of a tree of n nodes (keys: its rows 0 .. n, packed): every filled slot names a node 1 .. n, each node
    exactly once, and each node sits on the probe from its home cell with no empty slot before it."""
    mask = len(table) - 1
    filled = np.flatnonzero(table)
    assert np.array_equal(np.sort(table[filled]), np.arange(1, n + 1))
    where = np.empty(n + 1, dtype=np.int64)
    where[table[filled]] = filled
    home = home_cell(keys[1:n + 1].view(np.uint32).reshape(-1, 4), len(table))
    for i in range(1, n + 1):
        h, s = int(home[i - 1]), int(where[i])
        steps = (s - h) & mask
        assert all(table[(h + j) & mask] != 0 for j in range(steps)), f"node {i}: an empty slot on its probe"
