"""
Packed node states on the host (NumPy only): what the search forests' `keys` arrays hold (csrc/rubiks_keys.h).
"""
import numpy as np


def unpack_keys(keys: np.ndarray) -> np.ndarray:
    """(n,4) uint32 packed states -> (n,20) int8 codes (6 codes of 5 bits per dword)."""
    keys = keys.astype(np.uint32).reshape(-1, 4)
    out = np.empty((len(keys), 20), dtype=np.int8)
    for j in range(20):
        out[:, j] = (keys[:, j // 6] >> np.uint32(5 * (j % 6))) & np.uint32(31)
    return out
