"""
The 6x8x6 kernels (csrc/rubiks_env686.hip) against the reference's own outputs (tests/golden/cube686_golden.npz), bit for bit --
the one-hot and +-1 outputs too, since 0 and +-1 are exact in float32 and bfloat16.  Sizes 1, 15, 16, 17, 255, 256, 257 and 1 027
are the edges of a lane's 16 states and of the 64- and 256-state workgroup tiles; one size beyond 65 536 takes the large-batch
tiles, and one beyond 2^20 the non-temporal form of rc686_multi_rotate.  Covered: the sticker-plane kernels, the one-launch row-major forms behind the `cube686` functions, the bridge kernels from
the 20 code planes (whole batches and column windows), and the `cube686` scramblers against the reference's draws.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import conftest  # noqa: E402,F401
from formula_weights import golden  # noqa: E402

SIZES = (1, 15, 16, 17, 255, 256, 257, 1027)


@pytest.fixture(scope="module")
def g():
    return {k: v for k, v in golden().items()}


def _actions(g, n):
    a = (2 * g["mr_faces"][:n].astype(np.int64) + 1 - g["mr_dirs"][:n]).astype(np.uint8)
    buf = np.zeros((n + 15) // 16 * 16, dtype=np.uint8)
    buf[:n] = a
    return torch.from_numpy(buf).cuda()


def _bf16_exact(t, expected):
    assert t.dtype == torch.bfloat16
    return np.array_equal(t.float().cpu().numpy(), expected)


@pytest.mark.parametrize("n", SIZES)
def test_planes_form(g, n):
    from librubiks.cube import DeviceCubes686
    s = g["states686"][:n]
    cubes = DeviceCubes686.from_numpy(s)
    assert cubes.soa.shape[0] == 48 and np.array_equal(cubes.numpy(), s)                       # both boundary transposes
    colours = s.reshape(n, 48, 6).argmax(2)
    assert np.array_equal(cubes.soa[:, :n].cpu().numpy(), colours.T)
    assert np.array_equal(cubes.multi_rotate(_actions(g, n)).numpy(), g["mr_out"][:n])
    assert np.array_equal(cubes.numpy(), s)                                                    # out of place
    assert np.array_equal(cubes.is_solved().cpu().numpy(), g["is_solved"][:n])
    oh = cubes.as_oh(torch.float32)
    assert oh.shape == (n, 288) and np.array_equal(oh.cpu().numpy(), g["as_oh"][:n])
    assert _bf16_exact(cubes.as_oh(torch.bfloat16), g["as_oh"][:n])
    assert np.array_equal(cubes.as_correct().cpu().numpy(), g["as_correct"][:n])
    same = DeviceCubes686(cubes.soa.clone(), n)                                               # in and out may alias exactly
    same.multi_rotate(_actions(g, n), out=same)
    assert np.array_equal(same.numpy(), g["mr_out"][:n])


@pytest.mark.parametrize("n", SIZES)
def test_bridge_from_the_code_planes(g, n):
    from librubiks.cube import DeviceCubes
    cubes = DeviceCubes.from_numpy(g["states2024"][:n])
    assert np.array_equal(cubes.to686().numpy(), g["states686"][:n])
    assert np.array_equal(cubes.as_oh686(torch.float32).cpu().numpy(), g["as_oh"][:n])
    assert _bf16_exact(cubes.as_oh686(torch.bfloat16), g["as_oh"][:n])
    assert np.array_equal(cubes.as_correct686().cpu().numpy(), g["as_correct"][:n])
    out = torch.full((n, 288), 7.0, device="cuda")                                             # every element is written
    assert cubes.as_oh686(out=out) is out and np.array_equal(out.cpu().numpy(), g["as_oh"][:n])


@pytest.mark.parametrize("lo,n", [(16, 1), (16, 17), (256, 257), (1008, 19), (64, 963)])
def test_bridge_on_a_column_window(g, lo, n):
    from librubiks.cube import DeviceCubes
    from librubiks.cube.device import encode
    from librubiks.model import GenericNet
    cubes = DeviceCubes.from_numpy(g["states2024"])
    want = g["as_oh"][lo:lo + n]
    assert np.array_equal(cubes.as_oh686(torch.float32, lo=lo, n=n).cpu().numpy(), want)
    assert _bf16_exact(cubes.as_oh686(torch.bfloat16, lo=lo, n=n), want)
    assert np.array_equal(cubes.as_correct686(lo=lo, n=n).cpu().numpy(), g["as_correct"][lo:lo + n])

    class Net686(torch.nn.Module):
        class config:
            is2024 = False
    buf = torch.zeros((1027, 288), device="cuda")
    out = encode(GenericNet(Net686()), cubes, buf[:n], lo, n)                                   # the agents' helper, 6x8x6 engine
    assert out.data_ptr() == buf.data_ptr() and np.array_equal(out.cpu().numpy(), want)
    plain = encode(GenericNet(torch.nn.Identity()), cubes, None, lo, n)                          # ... and a 20x24 engine: rc_as_oh_f32
    assert plain.shape == (n, 480)
    assert np.array_equal(plain.cpu().numpy(), DeviceCubes.from_numpy(g["states2024"][lo:lo + n]).as_oh().cpu().numpy())
    with pytest.raises(AssertionError):
        cubes.as_oh686(lo=8, n=4)                                                              # a window starts at a multiple of 16


def test_expand12_and_its_flags(g):
    from librubiks.cube import DeviceCubes686
    for take in (64, 63, 17, 1):
        parents = g["states686"][g["ex_idx"][:take]]
        cubes = DeviceCubes686.from_numpy(parents)
        assert np.array_equal(cubes.expand12().numpy(), g["ex_children"][:12 * take])
        kids, pflags, cflags = cubes.expand12_flags()
        assert np.array_equal(kids.numpy(), g["ex_children"][:12 * take])
        assert np.array_equal(pflags.cpu().numpy(), g["is_solved"][g["ex_idx"][:take]])
        assert np.array_equal(cflags.cpu().numpy(), g["ex_children_solved"][:12 * take])
    assert g["ex_children_solved"].sum() == 24 and g["is_solved"][g["ex_idx"]].sum() == 4
    # more than one tile of parents (64 per workgroup), not a multiple of it
    many = g["states686"][:257]
    kids = DeviceCubes686.from_numpy(many).expand12().numpy().reshape(257, 12, 48, 6)
    from librubiks.cube import cube686
    want = many.reshape(257, 48, 6)[:, cube686.get_perm_table()]
    assert np.array_equal(kids, want)


def test_large_batch_tiles(g):
    """Beyond 65 536 states the encoders stage 256 states per workgroup instead of 64."""
    from librubiks.cube import DeviceCubes, DeviceCubes686
    reps = 65
    n = reps * 1027 - 5                                                                        # 66 750: no multiple of 16 or of a tile
    s20, s686 = np.tile(g["states2024"], (reps, 1))[:n], np.tile(g["states686"], (reps, 1, 1, 1))[:n]
    oh, correct = torch.from_numpy(np.tile(g["as_oh"], (reps, 1))[:n]).cuda(), torch.from_numpy(np.tile(g["as_correct"], (reps, 1, 1))[:n]).cuda()
    c20, c686 = DeviceCubes.from_numpy(s20), DeviceCubes686.from_numpy(s686)
    assert torch.equal(c20.as_oh686(torch.float32), oh) and torch.equal(c686.as_oh(torch.float32), oh)
    assert torch.equal(c20.as_oh686(torch.bfloat16).float(), oh) and torch.equal(c686.as_oh(torch.bfloat16).float(), oh)
    assert torch.equal(c20.as_correct686(), correct) and torch.equal(c686.as_correct(), correct)
    assert torch.equal(c20.to686().soa[:, :n], c686.soa[:, :n])
    assert torch.equal(c20.as_oh686(torch.float32, lo=1024, n=65600), oh[1024:1024 + 65600])
    assert np.array_equal(c686.numpy(), s686)
    assert np.array_equal(c686.is_solved().cpu().numpy(), np.tile(g["is_solved"], reps)[:n])


def test_multi_rotate_beyond_a_million_states(g):
    """From 2^20 states on rc686_multi_rotate streams with non-temporal accesses (another instantiation of the kernel)."""
    from librubiks.cube import DeviceCubes686
    reps = 1022
    n = reps * 1027 - 3                                                                        # 1 049 591
    assert n >= 1 << 20
    small, want = DeviceCubes686.from_numpy(g["states686"]), DeviceCubes686.from_numpy(g["mr_out"])
    big = DeviceCubes686.empty(n)
    big.soa[:, :n] = small.soa[:, :1027].repeat(1, reps)[:, :n]
    actions = torch.zeros((n + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
    actions[:n] = _actions(g, 1027)[:1027].repeat(reps)[:n]
    out = big.multi_rotate(actions)
    assert torch.equal(out.soa[:, :n], want.soa[:, :1027].repeat(1, reps)[:, :n])
    assert torch.equal(big.soa[:, :n], small.soa[:, :1027].repeat(1, reps)[:, :n])                 # out of place
    back = int((g["mr_out"].reshape(1027, 288) == g["solved"].reshape(288)).all(1).sum())          # one-move states moved back
    assert back > 0 and int(out.is_solved().sum()) == back * reps and int(big.is_solved().sum()) == 4 * reps


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_correctness_from_the_one_hot(g, dtype):
    from librubiks.cube import cube686
    for n in (1, 17, 1027):
        out = cube686.as_correct(torch.from_numpy(g["as_oh"][:n]).cuda().to(dtype))
        assert out.dtype == dtype and out.shape == (n, 6, 8)
        assert np.array_equal(out.float().cpu().numpy(), g["as_correct"][:n])
    broken = torch.from_numpy(g["as_oh"][:4]).cuda().to(dtype)
    broken[:, 5] = 1.0                                                                         # a second 1 on sticker 0: not its solved entry
    assert (cube686.as_correct(broken)[:, 0, 0] == -1).all()


@pytest.mark.parametrize("n", SIZES)
def test_module_functions_in_one_launch(g, n):
    from librubiks.cube import cube686
    s = g["states686"][:n]
    before = s.copy()
    out = cube686.multi_rotate(s, g["mr_faces"][:n], g["mr_dirs"][:n])
    assert out.dtype == np.int8 and np.array_equal(out, g["mr_out"][:n]) and np.array_equal(s, before)
    assert np.array_equal(cube686.multi_is_solved(s), g["is_solved"][:n]) and cube686.multi_is_solved(s).dtype == bool
    oh = cube686.as_oh(s)
    assert oh.is_cuda and oh.dtype == torch.float32 and np.array_equal(oh.cpu().numpy(), g["as_oh"][:n])
    assert np.array_equal(cube686.rotate(s[n - 1], g["mr_faces"][n - 1], g["mr_dirs"][n - 1]), g["mr_out"][n - 1])
    assert cube686.is_solved(s[0]) and cube686.is_solved(s[n - 1]) == bool(g["is_solved"][n - 1])


def test_module_functions_through_the_planes(g, monkeypatch):
    from librubiks.cube import cube686
    monkeypatch.setattr(cube686, "SMALL_CALL_686", 0)   # what batches beyond the one-launch limit take
    s = g["states686"]
    assert np.array_equal(cube686.multi_rotate(s, g["mr_faces"], g["mr_dirs"]), g["mr_out"])
    assert np.array_equal(cube686.multi_is_solved(s), g["is_solved"])
    assert np.array_equal(cube686.as_oh(s).cpu().numpy(), g["as_oh"])
    assert np.array_equal(cube686.as_oh(s[5]).cpu().numpy(), g["as_oh_single"])


def test_single_state_and_empty_calls(g):
    from librubiks.cube import cube686
    assert np.array_equal(cube686.as_oh(g["states686"][5]).cpu().numpy(), g["as_oh_single"])
    assert cube686.as_oh(g["states686"][:0]).shape == (0, 288) and cube686.multi_is_solved(g["states686"][:0]).shape == (0,)
    assert cube686.multi_rotate(g["states686"][:0], np.zeros(0, int), np.zeros(0, int)).shape == (0, 6, 8, 6)
    assert cube686.as_correct(cube686.as_oh(g["solved"])).eq(1).all()


@pytest.mark.parametrize("seed", [0, 42])
def test_scramblers_draw_like_the_reference(g, seed):
    from librubiks.cube import DeviceCubes686, cube686
    for depth in (10, 14):
        np.random.seed(seed)
        for i in range(8):
            s, f, d = cube686.scramble(depth, True)
            assert s.shape == (6, 8, 6) and s.dtype == np.int8
            assert np.array_equal(s, g[f"scr_s{seed}_d{depth}_states"][i])
            assert np.array_equal(f, g[f"scr_s{seed}_d{depth}_faces"][i]) and np.array_equal(d, g[f"scr_s{seed}_d{depth}_dirs"][i])
        np.random.seed(seed)
        cubes, f, d = cube686.scramble_batch(8, depth, True)
        assert np.array_equal(cubes.numpy(), g[f"scr_s{seed}_d{depth}_states"])
        # the same moves applied to sticker planes, row d of `moves` first
        acts = (2 * g[f"scr_s{seed}_d{depth}_faces"] + 1 - g[f"scr_s{seed}_d{depth}_dirs"]).astype(np.uint8)
        moves = np.full((depth + 1, 8), 12, dtype=np.uint8)                                     # a last row of 12s: no move
        moves[:depth] = acts.T
        moved = DeviceCubes686.solved(8).apply_moves(torch.from_numpy(moves).cuda())
        assert np.array_equal(moved.numpy(), g[f"scr_s{seed}_d{depth}_states"])
    for ws in (True, False):
        np.random.seed(seed)
        s, oh = cube686.sequence_scrambler(4, 10, ws)
        assert np.array_equal(s, g[f"seq_s{seed}_ws{int(ws)}_states"])
        assert oh.dtype == torch.float32 and np.array_equal(oh.cpu().numpy(), s.reshape(40, 288).astype(np.float32))
