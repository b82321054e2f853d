"""
The network kernels on PACKED rows (MCTSForest.pack_rows): a device word R says how many of the launch's rows exist, a device map
names the state / row slot behind each of them.  Every kernel must give the rows that exist the bits of its plain launch on the same
operands and touch no other row, whatever R is -- the launch shape (grid, tiles, K chunks) is the plain one's, chosen on the host
from the row bound.  And rc_mcts_row_map must be the exclusive scan of the listed trees' row counts, in list order.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HALF_SENTINEL, WORD_SENTINEL = 0x7BCD, 0x7FC12345   # a finite half / a NaN payload no kernel produces


def _split(v):
    hi = v.half()
    return hi, ((v - hi.double()) * 2048.0).half()


def _word(n):
    return torch.tensor([n, 0, 0, 0], dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("rows", [700, 1056])        # two row tiles (the last one short), three full ones
@pytest.mark.parametrize("k", [128, 256])
@pytest.mark.parametrize("n_out", [256, 512])
def test_hidden_layer_with_a_device_row_count_equals_the_plain_launch_on_the_rows_that_exist(n_out, k, rows):
    """rc_split_layer_f16 with rows_dev: whole K with [hi | lo] and fp32 outputs (352 x 256 and 352 x 128 tiles) and K cut into 2,
    3 or 4 chunks (352 x 256, 352 x 128 and 352 x 64 tiles; 3 k / 64 = 6 K-steps at k = 128 take 2 and 3 chunks, 12 at k = 256 take 2
    and 4).  R around one fragment row, around the even tile heights and at the launch's end: rows < R bit-equal to the plain
    launch, rows >= R of a pre-filled output untouched."""
    from librubiks.model import _layer_call
    g = torch.Generator().manual_seed(1000 * n_out + 10 * k + rows)
    x = torch.randn(rows, k, generator=g).double() * 0.7
    W = torch.randn(n_out, k, generator=g).double() / np.sqrt(k)
    b = torch.randn(n_out, generator=g).cuda()
    (xh, xl), (wh, wl) = _split(x), _split(W)
    a, w3 = torch.cat([xh, xl], 1).cuda(), torch.cat([wl, wh, wh], 1).cuda()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    common = dict(a=a, w=w3, n_rows=rows, n_out=n_out, k=k)
    kinds = [("halves", tile, 1) for tile in (1, 3)] + [("f32", tile, 1) for tile in (1, 3)] + \
            [("partials", tile, S) for tile in (1, 3, 7) for S in ((2, 3) if k == 128 else (2, 4))]
    Rs = sorted({1, 15, 16, 17, 320, 336, 337, 352, 353, rows - 1, rows})
    for kind, tile, S in kinds:
        if kind == "halves":
            make = lambda: torch.full((rows, 2 * n_out), HALF_SENTINEL, dtype=torch.int16, device="cuda")   # noqa: E731
            call = lambda out, **kw: _layer_call("rc_split_layer_f16", **common, bias=b, activation=2, alpha=1.0, out_hi_lo=out.view(torch.float16),   # noqa: E731
                                                 tile=tile, k_splits=1, range_flag=flag, **kw)
        elif kind == "f32":
            make = lambda: torch.full((rows, n_out), WORD_SENTINEL, dtype=torch.int32, device="cuda")   # noqa: E731
            call = lambda out, **kw: _layer_call("rc_split_layer_f16", **common, bias=b, activation=2, alpha=1.0, out_f32=out.view(torch.float32),   # noqa: E731
                                                 tile=tile, k_splits=1, **kw)
        else:
            make = lambda: torch.full((S, rows, n_out), WORD_SENTINEL, dtype=torch.int32, device="cuda")   # noqa: E731
            call = lambda out, **kw: _layer_call("rc_split_layer_f16", **common, out_partials=out.view(torch.float32), k_splits=S, tile=tile, **kw)   # noqa: E731
        plain = make()
        call(plain)
        rows_axis = plain.dim() - 2
        assert not bool((plain == (HALF_SENTINEL if kind == "halves" else WORD_SENTINEL)).all(rows_axis + 1).any()), "the plain launch writes every row"
        for R in Rs:
            out = make()
            call(out, rows_dev=_word(R))
            lo, hi = out.narrow(rows_axis, 0, R), out.narrow(rows_axis, R, rows - R)
            assert torch.equal(lo, plain.narrow(rows_axis, 0, R)), (kind, tile, S, R)
            assert bool((hi == (HALF_SENTINEL if kind == "halves" else WORD_SENTINEL)).all()), (kind, tile, S, R)
        out = make()
        call(out, rows_dev=_word(0))              # no row at all, and a count beyond the launch's rows
        assert bool((out == (HALF_SENTINEL if kind == "halves" else WORD_SENTINEL)).all())
        out = make()
        call(out, rows_dev=_word(rows + 1000))
        assert torch.equal(out, plain)
    assert int(flag.item()) == 0


def test_device_row_count_is_refused_where_no_kernel_reads_it():
    from librubiks import _hip
    from librubiks.model import _layer_call
    a = torch.zeros((64, 256), dtype=torch.float16, device="cuda")
    w3 = torch.zeros((256, 384), dtype=torch.float16, device="cuda")
    b = torch.zeros(256, device="cuda")
    out = torch.empty((64, 512), dtype=torch.float16, device="cuda")
    for tile in (2, 4, 5, 6):    # 176 x 128 and the four-wave tiles have no such form: an error, not a plain launch
        with pytest.raises(_hip.RubiksHipError):
            _layer_call("rc_split_layer_f16", a=a, w=w3, bias=b, n_rows=64, n_out=256, k=128, activation=2, alpha=1.0, out_hi_lo=out, tile=tile,
                        k_splits=1, rows_dev=_word(10))
    with pytest.raises(_hip.RubiksHipError):
        _layer_call("rc_gemm_layer_bf16", a=a.view(torch.bfloat16), w=w3.view(torch.bfloat16), bias=b, n_rows=64, n_out=256, k=128,
                    out_bf16=out.view(torch.bfloat16)[:, :256].contiguous(), rows_dev=_word(10))


@pytest.mark.parametrize("n", [64, 353])
def test_input_layer_with_a_map_gives_packed_row_r_the_bits_of_state_src_r(n):
    """rc_first_layer_gather_rows_f16 in both forms of the kernel (forced), with a map that permutes the states and drops a third
    of them: packed row r equals row src[r] of rc_first_layer_gather_f16, rows >= R keep what they held; R = 0 writes nothing."""
    from librubiks import _hip, cube
    lib = _hip.lib()
    H = 128
    g = torch.Generator().manual_seed(n)
    Wt = (torch.randn(480, H, generator=g) * 0.3).cuda()
    bias = torch.randn(H, generator=g).cuda()
    np.random.seed(n)
    cubes, _, _ = cube.scramble_batch(n, 15, True)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    plain = torch.empty((n, 2 * H), dtype=torch.float16, device="cuda")
    _hip.check(lib.rc_first_layer_gather_f16(cubes.soa.data_ptr(), n, cubes.stride, Wt.data_ptr(), bias.data_ptr(), plain.data_ptr(), H, 2, 1.0,
                                             flag.data_ptr(), None), "rc_first_layer_gather_f16")
    plain = plain.view(torch.int16)
    perm = torch.randperm(n, generator=g)
    for R in (n - n // 3, n, 1, 0):
        src = torch.full((n,), n + 7, dtype=torch.int32)      # entries beyond R are never read
        src[:R] = perm[:R].int()
        src = src.cuda()
        for form in (1, 2):
            out = torch.full((n, 2 * H), HALF_SENTINEL, dtype=torch.int16, device="cuda")
            _hip.check(lib.rc_first_layer_gather_rows_f16(cubes.soa.data_ptr(), n, cubes.stride, Wt.data_ptr(), bias.data_ptr(), out.data_ptr(), H, 2,
                                                          1.0, flag.data_ptr(), _word(R).data_ptr(), src.data_ptr(), form, None),
                       "rc_first_layer_gather_rows_f16")
            assert torch.equal(out[:R], plain[perm[:R].cuda()]), (R, form)
            assert bool((out[R:] == HALF_SENTINEL).all()), (R, form)
    args = (cubes.soa.data_ptr(), n, cubes.stride, Wt.data_ptr(), bias.data_ptr(), plain.data_ptr(), H, 2, 1.0, None)
    assert lib.rc_first_layer_gather_rows_f16(*args, _word(1).data_ptr(), None, 0, None) == -1      # a count without a map
    assert lib.rc_first_layer_gather_rows_f16(*args, _word(1).data_ptr(), src.data_ptr(), 3, None) == -4   # no such form
    assert int(flag.item()) == 0


@pytest.mark.parametrize("K", [512, 1024])
def test_head_scatters_the_rows_that_exist_to_their_slots_and_writes_no_other(K):
    """rc_head_split_rows_f32: row r < R of (c, c_corr) lands in row src[r] of the [n, 16] buffer with the bits rc_head_split_f32
    gives row r; slots no row maps to keep their sentinel.  rc_split_reduce_rows_f16 likewise stops at R."""
    from librubiks import _hip
    lib = _hip.lib()
    n, n_out = 353, 13
    g = torch.Generator().manual_seed(K)
    c, corr = torch.randn(n, K, generator=g).cuda(), (torch.randn(n, K, generator=g) * 100).cuda()
    bh, w, bo = torch.randn(K, generator=g).cuda(), (torch.randn(n_out, K, generator=g) / 30).cuda(), torch.randn(n_out, generator=g).cuda()
    plain = torch.empty((n, 16), device="cuda")
    args = (c.data_ptr(), corr.data_ptr(), 1.0 / 2048.0, n, K, bh.data_ptr(), 2, 1.0, w.data_ptr(), bo.data_ptr(), n_out)
    _hip.check(lib.rc_head_split_f32(*args, plain.data_ptr(), None), "rc_head_split_f32")
    plain = plain.view(torch.int32)
    perm = torch.randperm(n, generator=g).cuda()
    for R in (0, 1, 16, 17, 200, n):
        out = torch.full((n, 16), WORD_SENTINEL, dtype=torch.int32, device="cuda")
        src = perm.int().contiguous()
        _hip.check(lib.rc_head_split_rows_f32(*args, out.data_ptr(), _word(R).data_ptr(), src.data_ptr(), None), "rc_head_split_rows_f32")
        assert torch.equal(out[perm[:R]], plain[:R]), R
        assert bool((out[perm[R:]] == WORD_SENTINEL).all()), R
    assert lib.rc_head_split_rows_f32(*args, out.data_ptr(), None, src.data_ptr(), None) == -1
    # the reduce kernel: two partials, the first one a correction
    part = torch.stack([corr, c])
    whole_hl, whole_f = torch.empty((n, 2 * K), dtype=torch.float16, device="cuda"), torch.empty((n, K), device="cuda")
    red = (part.data_ptr(), n * K, 2, 1, n, K, bh.data_ptr(), None, 2, 1.0, None, None)
    _hip.check(lib.rc_split_reduce_f16(*red, whole_hl.data_ptr(), whole_f.data_ptr(), None, None), "rc_split_reduce_f16")
    for R in (0, 1, 200, n):
        hl = torch.full((n, 2 * K), HALF_SENTINEL, dtype=torch.int16, device="cuda")
        f = torch.full((n, K), WORD_SENTINEL, dtype=torch.int32, device="cuda")
        _hip.check(lib.rc_split_reduce_rows_f16(*red, hl.data_ptr(), f.data_ptr(), None, _word(R).data_ptr(), None), "rc_split_reduce_rows_f16")
        assert torch.equal(hl[:R], whole_hl.view(torch.int16)[:R]) and torch.equal(f[:R], whole_f.view(torch.int32)[:R]), R
        assert bool((hl[R:] == HALF_SENTINEL).all()) and bool((f[R:] == WORD_SENTINEL).all()), R


def test_row_map_is_the_exclusive_scan_of_the_listed_trees_counts():
    """rc_mcts_row_map against NumPy: every count 0 .. 11 (not expanded; the root phases' 11 and 2; 0 .. 12 new children, capped at
    the 11 row slots), every tree listed in order, then a shuffled shorter list padded with -1 to its launch size -- the counts follow
    their trees to the new positions."""
    from librubiks.solving import mcts_device as md
    B = 70
    forest = md.MCTSForest(B, 40, max_path=64)
    rng = np.random.default_rng(3)
    expanded = (rng.random(B) < 0.8).astype(np.uint8)
    phase = rng.choice([0, 0, 0, 1, 2, 16, 17, 18], size=B).astype(np.int32)     # (16: the "solved at the root" flag on top of a phase)
    new_mask = np.array([int(sum(1 << int(b) for b in rng.choice(12, size=int(rng.integers(0, 13)), replace=False))) for _ in range(B)], dtype=np.int32)
    new_mask[:13] = [(1 << i) - 1 for i in range(13)]        # every count once, whatever the draw
    expanded[:13], phase[:13] = 1, 0
    forest.expanded.copy_(torch.from_numpy(expanded))
    forest.phase.copy_(torch.from_numpy(phase))
    forest.new_mask.copy_(torch.from_numpy(new_mask))

    def count(t):
        if t < 0 or not expanded[t]:
            return 0
        ph = phase[t] & 15
        return 11 if ph == 1 else 2 if ph == 2 else min(bin(int(new_mask[t]) & 0xFFF).count("1"), 11)

    def check(listed):
        rows, first, src = forest.row_map()
        torch.cuda.synchronize()
        cnt = np.array([count(int(t)) for t in listed])
        off = np.concatenate([[0], np.cumsum(cnt)])
        assert len(listed) == forest.G and int(rows[0].item()) == off[-1]
        assert np.array_equal(first[:forest.G].cpu().numpy(), off[:-1])
        want = np.concatenate([md.ROWS * i + np.arange(c) for i, c in enumerate(cnt)] + [np.zeros(0, dtype=np.int64)])
        assert np.array_equal(src[:off[-1]].cpu().numpy(), want)
        return cnt

    cnt = check(np.arange(B))
    assert set(cnt[:13]) == set(range(12))
    trees = rng.permutation(B)[:40]
    forest.set_active(trees)
    assert forest.G == 64
    check(np.concatenate([trees, np.full(24, -1)]))
    forest.set_active(trees[::-1][:30])               # reordered and narrowed again: 32 positions, two pads
    assert forest.G == 32
    check(np.concatenate([trees[::-1][:30], np.full(2, -1)]))
    assert forest.lib.rc_mcts_row_map(ctypes.byref(forest.struct), None, forest.row_first.data_ptr(), forest.row_src.data_ptr(), None) == -1
    forest.close()
