"""
CPU checks of the entry points behind queue shortening (rc_shorten_index, rc_shorten_neighbours, rc_shorten_bfs, rc_shorten):
argument errors are reported before anything is launched, so they need no GPU; the ABI version stays where callers built against
it expect it (symbols were only added); and rc_shorten_workspace_bytes is the header's formula.
"""
import ctypes

import pytest

import conftest  # noqa: F401  (puts the package on sys.path)
import shorten_model as sm

RC_ERR_NULL, RC_ERR_ALIGN, RC_ERR_STRIDE, RC_ERR_RANGE = -1, -2, -3, -4
ENTRY_POINTS = ("rc_shorten_index", "rc_shorten_neighbours", "rc_shorten_bfs", "rc_shorten")


@pytest.fixture(scope="module")
def lib():
    from librubiks import _hip
    from librubiks.solving import shorten  # noqa: F401  (registers the rc_shorten_* signatures)
    return _hip.load()


def _struct(G=4, Q=40, W=40, max_len=30, stride=256, P=200, H=512, **over):
    """A well-formed rc_shorten_t whose pointers name no memory: every call below must fail its checks before it would use them."""
    from librubiks.solving.shorten import POINTER_FIELDS, _ShortenStruct
    s = _ShortenStruct()
    s.n_games, s.queue_width, s.out_width, s.max_len, s.stride, s.total_positions, s.total_hash_cells = G, Q, W, max_len, stride, P, H
    for i, name in enumerate(POINTER_FIELDS):
        setattr(s, name, 0x1000 * (i + 1))
    for k, v in over.items():
        setattr(s, k, v)
    return s


def _bad_structs():
    from librubiks.solving.shorten import MAX_LEN, POINTER_FIELDS
    out = [(_struct(**{name: None}), RC_ERR_NULL) for name in POINTER_FIELDS]
    out += [(_struct(roots_soa=0x1004), RC_ERR_ALIGN), (_struct(keys=0x7008), RC_ERR_ALIGN), (_struct(hash=0xd004), RC_ERR_ALIGN),
            (_struct(stride=264), RC_ERR_ALIGN), (_struct(pos_off=0x5004), RC_ERR_ALIGN), (_struct(hash_off=0x6004), RC_ERR_ALIGN),
            (_struct(lens=0x3002), RC_ERR_ALIGN), (_struct(ids=0x8002), RC_ERR_ALIGN), (_struct(nbr=0x9001), RC_ERR_ALIGN),
            (_struct(claim=0xa002), RC_ERR_ALIGN), (_struct(frontier_a=0xb002), RC_ERR_ALIGN), (_struct(frontier_b=0xc002), RC_ERR_ALIGN),
            (_struct(out_lens=0xf002), RC_ERR_ALIGN), (_struct(status=0x10002), RC_ERR_ALIGN),
            (_struct(G=300), RC_ERR_STRIDE),                                              # 300 games need 304 bytes per plane
            (_struct(G=0), RC_ERR_RANGE), (_struct(Q=0), RC_ERR_RANGE), (_struct(W=0), RC_ERR_RANGE),
            (_struct(max_len=41), RC_ERR_RANGE),                                          # longer than a queue row
            (_struct(Q=2 ** 31, max_len=MAX_LEN + 1), RC_ERR_RANGE),                      # parent << 4 | action would not fit an int32
            (_struct(P=0), RC_ERR_RANGE), (_struct(H=1), RC_ERR_RANGE), (_struct(P=1 << 40), RC_ERR_RANGE), (_struct(H=1 << 40), RC_ERR_RANGE)]
    return out


def test_abi_version_stays_10_and_the_entry_points_exist(lib):
    from librubiks.solving.shorten import _ShortenStruct
    assert lib.rc_abi_version() == 10
    for name in ENTRY_POINTS + ("rc_shorten_workspace_bytes", "rc_shorten_struct_bytes"):
        assert hasattr(lib, name)
    assert lib.rc_shorten_struct_bytes() == ctypes.sizeof(_ShortenStruct)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_every_entry_point_rejects_bad_arguments_without_a_launch(lib, name):
    fn = getattr(lib, name)
    assert fn(None, None) == RC_ERR_NULL
    for bad, code in _bad_structs():
        assert fn(ctypes.byref(bad), None) == code
    from librubiks.solving.shorten import MAX_LEN
    assert MAX_LEN == sm.MAX_LEN == (1 << 27) - 2


def test_workspace_bytes_is_the_headers_formula(lib):
    from librubiks.solving import shorten
    r = lambda x: (x + 255) // 256 * 256   # noqa: E731
    for P, H in ((1, 2), (7, 16), (1000, 4096), (175_001, 524_288), (2 ** 31 + 5, 2 ** 33)):
        want = r(16 * P) + r(4 * P) + r(48 * P) + r(8 * P) + 2 * r(4 * P) + r(4 * H)
        assert lib.rc_shorten_workspace_bytes(P, H) == want == shorten.workspace_bytes(P, H) == sm.workspace_bytes(P, H)
    assert lib.rc_shorten_workspace_bytes(1 << 40, 2) == 0 and lib.rc_shorten_workspace_bytes(1, 1 << 40) == 0
    # 84 bytes per position and 4 per cell, 2 .. 4 cells per position: the 90 - 100 B a position costs
    assert 92 <= shorten.workspace_bytes(1 << 20, 2 << 20) / (1 << 20) <= 100 >= shorten.workspace_bytes(1 << 20, 4 << 20) / (1 << 20)
