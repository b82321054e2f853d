"""
The eight-column form of the input layer (rc_first_layer_gather_f16, form 2 of rc_first_layer_gather_rows_f16) as a pipeline: a wave
keeps table reads in flight across the end of a state, has its codes in registers two passes ahead (the map entry three) and swaps one
group of four columns with its neighbour lane before it stores.  Whatever the pipeline does, a state's outputs are the bits of twenty
sequential fp32 additions behind the bias -- the torch model of tests/test_net_gpu.py::test_input_layer_as_a_sum_of_rows -- and the
bits the four-column form gives; rows that do not exist are never written, map entries that are stale never become an address.

PASS rows are one pass of a workgroup of the eight-column form (twelve waves of eight states; 64 with the eight waves the form had
before: both sets of boundaries are run), AHEAD the passes its codes are requested ahead of their use and MAP_AHEAD those of its map
entries; H = 4096 makes 64 column tiles and so 4 row groups, H = 64 one column tile and up to 256 row groups.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cube as oc  # noqa: E402  (checker only)

PASS, AHEAD, MAP_AHEAD, GROUPS = 96, 2, 3, 4
HALF_SENTINEL = 0x7BCD        # a finite half no test's outputs contain
STALE = 0x7FFFFFFF
N_MAX = PASS * GROUPS * (AHEAD + 2) + 5
NONE, RELU, ELU = 0, 1, 2


def _around(passes):
    """The row counts at which every row group has had `passes` passes, one less and one more, for either pass size."""
    return [rows * GROUPS * passes + d for rows in (64, PASS) for d in (-1, 0, 1)]


@pytest.fixture(scope="module")
def data():
    """States, tables and the torch model's sums for every test of the module, computed once and left unchanged."""
    rng = np.random.RandomState(11)
    s = np.tile(oc.get_solved(), (N_MAX, 1))
    for _ in range(25):
        s = oc.multi_rotate_actions(s, rng.randint(0, 12, N_MAX))
    g = torch.Generator().manual_seed(5)
    idx = torch.from_numpy(s.astype(np.int64)).cuda() + 24 * torch.arange(20, device="cuda")      # [n, 20] rows of W^T
    out = {"states": s, "idx": idx}
    for H in (64, 4096):
        Wt = (torch.randn(480, H, generator=g) * 0.4).cuda().contiguous()
        b = torch.randn(H, generator=g).cuda()
        out[H] = (Wt, b, _model(Wt, b, idx))
    return out


def _model(Wt, b, idx):
    acc = b.expand(idx.shape[0], Wt.shape[1]).clone()
    for j in range(20):
        acc = acc + Wt[idx[:, j]]                                            # the same fp32 additions, in the same order
    hi = acc.half()
    return torch.cat([hi, ((acc - hi.float()) * 2048.0).half()], 1).view(torch.int16)


def _word(n):
    return torch.tensor([n, 0, 0, 0], dtype=torch.int32, device="cuda")


def _rows_call(cubes, n, Wt, b, H, act, form, R=None, src=None, flag=None, extra_rows=3):
    """rc_first_layer_gather_rows_f16 into a sentinel-filled output of n + extra_rows rows; the identity map and R = n by default."""
    from librubiks import _hip
    out = torch.full((n + extra_rows, 2 * H), HALF_SENTINEL, dtype=torch.int16, device="cuda")
    src = torch.arange(n, dtype=torch.int32, device="cuda") if src is None else src
    _hip.check(_hip.lib().rc_first_layer_gather_rows_f16(cubes.soa.data_ptr(), n, cubes.stride, Wt.data_ptr(), b.data_ptr(), out.data_ptr(), H, act, 1.0,
                                                         flag.data_ptr() if flag is not None else None, _word(n if R is None else R).data_ptr(),
                                                         src.data_ptr(), form, None), "rc_first_layer_gather_rows_f16")
    return out


BOUNDARY_NS = [1, 7, 8, 9, 63, 64, 65, PASS - 1, PASS, PASS + 1] + _around(AHEAD) + [64 * GROUPS * (AHEAD + 2) + 5, N_MAX]


@pytest.mark.parametrize("n", BOUNDARY_NS)
def test_every_row_at_pass_and_pipeline_boundaries(data, n):
    """H = 4096 (4 row groups), the eight-column form forced: a partial pass, whole passes, the pass in which the codes requested in
    the prologue run out, the first one whose codes were requested in the loop, and two passes beyond with a ragged end."""
    from librubiks.cube import DeviceCubes
    H = 4096
    Wt, b, model = data[H]
    cubes = DeviceCubes.from_numpy(data["states"][:n])
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    for act in (NONE, RELU, ELU):
        narrow, wide = (_rows_call(cubes, n, Wt, b, H, act, form, flag=flag) for form in (1, 2))
        assert torch.equal(wide, narrow), (n, act)
        assert bool((wide[n:] == HALF_SENTINEL).all()), (n, act)
        if act == NONE:
            assert torch.equal(wide[:n], model[:n]), n
    assert int(flag.item()) == 0


@pytest.mark.parametrize("n", [1, 5, 300])
def test_workgroups_with_less_than_a_pass_and_without_rows(data, n):
    """H = 64: one column tile, so up to 256 row groups share n rows -- units of one wave's states, waves and workgroups without any."""
    from librubiks import _hip
    from librubiks.cube import DeviceCubes
    H = 64
    Wt, b, model = data[H]
    cubes = DeviceCubes.from_numpy(data["states"][:n])
    for act in (NONE, RELU, ELU):
        narrow, wide = (_rows_call(cubes, n, Wt, b, H, act, form) for form in (1, 2))
        plain = torch.full_like(wide, HALF_SENTINEL)
        _hip.check(_hip.lib().rc_first_layer_gather_f16(cubes.soa.data_ptr(), n, cubes.stride, Wt.data_ptr(), b.data_ptr(), plain.data_ptr(), H, act, 1.0,
                                                        None, None), "rc_first_layer_gather_f16")
        assert torch.equal(wide, narrow) and torch.equal(wide, plain), (n, act)
        assert bool((wide[n:] == HALF_SENTINEL).all()), (n, act)
        if act == NONE:
            assert torch.equal(wide[:n], model[:n]), n


@pytest.mark.parametrize("act", [ELU, RELU])
def test_packed_rows_with_stale_map_entries(data, act):
    """A map that permutes the states and drops a third of them; the entries beyond R hold 0x7fffffff and are stale by contract: they
    must never become an address, however far ahead the kernel requests its map entries -- R around the row counts at which the
    farthest request for a code (AHEAD passes on) and for a map entry (MAP_AHEAD passes on) first falls behind the last row.  Packed
    row r is row src[r] of the plain call, rows >= R keep what they held, R = 0 writes nothing."""
    from librubiks import _hip
    from librubiks.cube import DeviceCubes
    H, n = 4096, PASS * GROUPS * MAP_AHEAD + 48
    Wt, b, _ = data[H]
    cubes = DeviceCubes.from_numpy(data["states"][:n])
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3))
    kept = n - n // 3
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    plain = torch.empty((n, 2 * H), dtype=torch.int16, device="cuda")
    _hip.check(_hip.lib().rc_first_layer_gather_f16(cubes.soa.data_ptr(), n, cubes.stride, Wt.data_ptr(), b.data_ptr(), plain.data_ptr(), H, act, 1.0,
                                                    flag.data_ptr(), None), "rc_first_layer_gather_f16")
    for R in [0, 1, 8, 9, 64 * GROUPS * AHEAD + 3, PASS * GROUPS * AHEAD + 3] + _around(MAP_AHEAD) + [kept, n]:
        src = torch.full((n,), STALE, dtype=torch.int32)
        src[:R] = perm[:R].int()
        src = src.cuda()
        for form in (1, 2):
            out = _rows_call(cubes, n, Wt, b, H, act, form, R=R, src=src, flag=flag, extra_rows=0)
            assert torch.equal(out[:R], plain[perm[:R].cuda()]), (act, R, form)
            assert bool((out[R:] == HALF_SENTINEL).all()), (act, R, form)
    assert int(flag.item()) == 0


def _hot_states(m, hot):
    """m solved cubes, those listed in `hot` turned once; (cubie, code) of a table row that only the turned ones select."""
    s = np.tile(oc.get_solved(), (m, 1))
    turned = oc.multi_rotate_actions(s[:1].copy(), np.array([0]))[0]
    j = int(np.nonzero(turned != s[0])[0][0])
    s[list(hot)] = turned
    return s, 24 * j + int(turned[j])


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("n", [8 * 9 + 1, 8 * 64 + 1, 8 * 96 + 1])
def test_half_range_flag_follows_the_rows_that_exist(n, form):
    """Only the rows of one (cubie, code) leave half's range.  The flag rises when the one state that selects it is the last one --
    the last live lane of the last pass, whichever column it is in -- and stays down when the only states that select it lie
    behind row n - 1 in the planes: the lanes past the end compute the LAST state again and count for nothing."""
    from librubiks.cube import DeviceCubes
    H = 64
    b = torch.zeros(H, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    for column in (0, 31, 32, 63):
        s, row = _hot_states(n + 16, [n - 1])
        Wt = torch.full((480, H), 0.25, device="cuda")
        Wt[row, column] = 1.0e5
        _rows_call(DeviceCubes.from_numpy(s), n, Wt, b, H, ELU, form, flag=flag)
        assert int(flag.item()) == 1, column
        flag.zero_()
        s, row = _hot_states(n + 16, range(n, n + 16))
        out = _rows_call(DeviceCubes.from_numpy(s), n, Wt, b, H, ELU, form, flag=flag)
        assert int(flag.item()) == 0, column
        assert bool((out[:n].view(torch.float16)[:, :H] == 5.0).all())         # twenty rows of 0.25: every state that exists is in range
        _rows_call(DeviceCubes.from_numpy(s), n + 1, Wt, b, H, ELU, form, flag=flag)   # the control: one of them inside
        assert int(flag.item()) == 1, column
        flag.zero_()


@pytest.mark.parametrize("n", [5, 300])
def test_every_column_holds_its_own_sum_after_the_exchange(data, n):
    """W^T[r][c] = c + r / 1024 without activation: output column c of a state is 20 c + (sum of its rows) / 1024, exact in fp32 and
    in the [hi | lo] halves.  Two column groups stored in each other's place, or the halves of a pair swapped, show as another c."""
    from librubiks.cube import DeviceCubes
    H = 128
    r, c = torch.arange(480, dtype=torch.float32, device="cuda"), torch.arange(H, dtype=torch.float32, device="cuda")
    Wt = (c[None, :] + r[:, None] / 1024.0).contiguous()
    b = torch.zeros(H, device="cuda")
    idx = data["idx"][:n]
    cubes = DeviceCubes.from_numpy(data["states"][:n])
    for form in (1, 2):
        out = _rows_call(cubes, n, Wt, b, H, NONE, form)
        assert torch.equal(out[:n], _model(Wt, b, idx)), form
        halves = out[:n].view(torch.float16).double()
        y = halves[:, :H] + halves[:, H:] / 2048.0
        column = (y - idx.sum(1, keepdim=True).double() / 1024.0) / 20.0
        assert torch.equal(column, c.double().expand(n, H)), form
