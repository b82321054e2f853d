"""
CPU checks of the entry points behind pattern mining (rc_patterns_begin, rc_patterns_extend, rc_patterns_close,
rc_patterns_level): the ABI version stays where callers built against it expect it (symbols were only added), the struct is the
ctypes mirror's size, argument errors are reported before anything is launched, and the host-only helpers -- workspace bytes, table
cells, the hash -- are the header's formulas, the Python module's and the model's.
"""
import ctypes

import pytest

import conftest  # noqa: F401  (puts the package on sys.path)
import patterns_model as pm

RC_ERR_NULL, RC_ERR_ALIGN, RC_ERR_RANGE = -1, -2, -4
ENTRY_POINTS = ("rc_patterns_begin", "rc_patterns_extend", "rc_patterns_close", "rc_patterns_level")
HELPERS = ("rc_patterns_struct_bytes", "rc_patterns_table_cells", "rc_patterns_workspace_bytes", "rc_patterns_hash")


@pytest.fixture(scope="module")
def lib():
    from librubiks import _hip
    from librubiks.analysis import pattern_mining  # noqa: F401  (registers the rc_patterns_* signatures)
    return _hip.load()


def _struct(**over):
    """A well-formed rc_patterns_t whose pointers name no memory: every call below must fail its checks before it would use them."""
    from librubiks.analysis.pattern_mining import POINTER_FIELDS, _PatternsStruct
    s = _PatternsStruct()
    s.n_seqs, s.width, s.level, s.min_count, s.total_positions, s.node_cells, s.seen_cells, s.out_cap = 4, 40, 2, 1, 100, 256, 256, 100
    for i, name in enumerate(POINTER_FIELDS):
        setattr(s, name, 0x1000 * (i + 1))
    for k, v in over.items():
        setattr(s, k, v)
    return s


def test_abi_version_stays_10_and_the_entry_points_exist(lib):
    from librubiks.analysis.pattern_mining import _PatternsStruct
    assert lib.rc_abi_version() == 10
    for name in ENTRY_POINTS + HELPERS:
        assert hasattr(lib, name)
    assert lib.rc_patterns_struct_bytes() == ctypes.sizeof(_PatternsStruct) == 4 * 4 + 4 * 8 + 13 * 8


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_every_entry_point_rejects_bad_arguments_without_a_launch(lib, name):
    from librubiks.analysis.pattern_mining import POINTER_FIELDS
    fn = getattr(lib, name)
    assert fn(None, None) == RC_ERR_NULL
    for field in POINTER_FIELDS:
        assert fn(ctypes.byref(_struct(**{field: None})), None) == RC_ERR_NULL
    for field, address in (("out_rows", 0xb008), ("counters", 0xc004), ("pos_off", 0x3004), ("node_keys", 0x7004), ("node_first", 0x9004),
                           ("seen_keys", 0xa004), ("lens", 0x2002), ("lane_seq", 0x4002), ("lane_state", 0x5002), ("lane_node", 0x6002),
                           ("node_count", 0x8002), ("status", 0xd002)):
        assert fn(ctypes.byref(_struct(**{field: address})), None) == RC_ERR_ALIGN, field
    bad = [dict(n_seqs=0), dict(width=0), dict(total_positions=0), dict(total_positions=1 << 40)]
    if name != "rc_patterns_begin":   # the level and the table sizes are the levels' arguments
        bad += [dict(level=1), dict(level=41), dict(node_cells=1), dict(node_cells=96), dict(seen_cells=0), dict(seen_cells=100), dict(node_cells=1 << 32)]
    for over in bad:
        assert fn(ctypes.byref(_struct(**over)), None) == RC_ERR_RANGE, over


def test_the_host_helpers_are_the_headers_formulas(lib):
    from librubiks.analysis import pattern_mining as mining
    r = lambda x: (x + 255) // 256 * 256   # noqa: E731
    for keys, cells in ((0, 2), (1, 2), (2, 4), (3, 8), (4, 8), (5, 16), (1000, 2048), (1024, 2048), (1025, 4096), (2 ** 31 + 5, 2 ** 33)):
        assert lib.rc_patterns_table_cells(keys) == cells == mining.table_cells(keys) == pm.table_cells(keys)
    for P in (1, 7, 1000, 175_001, 2_500_000, 2 ** 31 + 5):
        C = mining.table_cells(P)
        want = 3 * r(4 * P) + r(8 * C) + r(4 * C) + r(8 * C) + r(8 * C) + r(16 * P) + 256
        assert lib.rc_patterns_workspace_bytes(P) == want == mining.workspace_bytes(P) == pm.workspace_bytes(P)
    assert lib.rc_patterns_workspace_bytes(1 << 40) == 0 and lib.rc_patterns_table_cells(1 << 40) == 0
    # 28 bytes per position and 28 per cell, 2 .. 4 cells per position
    assert 84 <= mining.workspace_bytes(1 << 20) / (1 << 20) <= 85 and 139 <= mining.workspace_bytes((1 << 20) + 1) / (1 << 20) <= 141
    for key in (1, 0x101, (5 << 8) | 12, (77 << 32) | 3, (1 << 64) - 1):
        assert lib.rc_patterns_hash(key) == pm.hash64(key)
    assert (mining.OK, mining.BAD_ACTION, mining.FAILED, mining.NO_ROOM) == (pm.OK, pm.BAD_ACTION, pm.FAILED, pm.NO_ROOM) == (0, 1, 2, 3)
