"""
The epilogue contract of the network kernels, element by element (tests/netmath_model.py is the model):

    y = post_scale * act(acc + bias + residual) + post_shift,   hi = half(y),   lo = half((y - hi) 2^11),   flag iff !(|y| <= 65504)

Every entry point is driven through the C ABI so that the accumulator of output element (r, c) is EXACTLY the sweep value assigned to
it (identity weights, one-hot tables, selector rows): the model is then the only correct answer.  Without ELU the fp32 output equals
the model bit for bit (either rounding of the post-affine), bf16 outputs are its round-to-nearest-even; with ELU the same where
x > 0 and |y - alpha expm1(x)| <= alpha 2^-22 where x <= 0 (netmath_model.ELU_BOUND; bf16 outputs: plus half a bf16 ulp).  The halves
of a launch equal split(fp32 output of the same launch) bit for bit; the range flag rises exactly with an element beyond 65504 in a
row that exists.  alpha is 1.0, 0.37 and 2.5 throughout.  A failure names the element, its value and the stage that is off.
"""
import numpy as np
import pytest
import torch

import netmath_model as nm

pytestmark = pytest.mark.gpu

from oracle import cube as oc  # noqa: E402  (checker only)

ROWS, COLS = nm.ROWS, nm.COLS
ALPHAS = (1.0, 0.37, 2.5)
ACTS = [(0, 0.37), (1, 0.37)] + [(2, a) for a in ALPHAS]          # alpha must not touch identity / ReLU
ELU_MAX = {}                                                      # implementation -> measured max |y - alpha expm1(x)| / alpha
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _host(t, dtype=None):
    a = t.detach().cpu().contiguous()
    if a.dtype in (torch.float16, torch.bfloat16):
        a = a.view(torch.int16)
    a = a.numpy()
    if a.dtype == np.int16:
        a = a.view(np.uint16)
    return a if dtype is None else a.view(dtype)


def _lib():
    from librubiks import _hip
    return _hip, _hip.lib()


def _poison(shape, dtype):
    """NaN for fp32 buffers, 7.0 for halves and bf16 (as elsewhere in the suite)."""
    if dtype == torch.float32:
        return torch.full(shape, float("nan"), device="cuda")
    return torch.full(shape, 7.0, dtype=dtype, device="cuda")


def _untouched(t):
    return bool(torch.isnan(t).all()) if t.dtype == torch.float32 else bool((t == 7.0).all())


# ---- the model, per epilogue option ---------------------------------------------------------------------------------------------
class Epi:
    """Host side of one epilogue configuration for a [rows][cols] layer."""

    def __init__(self, rows, cols, full, seed=3, bf16=False):
        rng = np.random.RandomState(seed)
        self.full, self.bf16 = full, bf16
        if full:
            self.bias = rng.standard_normal(cols).astype(np.float32)
            self.ps = (rng.rand(cols) + 0.5).astype(np.float32) * np.where(np.arange(cols) % 5 == 0, -1, 1).astype(np.float32)
            self.pt = rng.standard_normal(cols).astype(np.float32)
            r = nm.sweep("finite", rows * cols, seed=seed + 1)[rng.permutation(rows * cols)].reshape(rows, cols)
            if bf16:
                self.res_bits = nm.bf16_rne(np.clip(r, -3e4, 3e4))
                self.res = (nm.bf16_value(self.res_bits),)
            else:
                self.res = nm.split(np.clip(r, -3e4, 3e4))
        else:
            self.bias = np.full(cols, -0.0, dtype=np.float32)       # x + -0 = x for every x, -0 included
            self.ps = self.pt = self.res = None

    def pre(self, acc):
        return nm.pre(acc, self.bias[None, :], *(self.res or ()))

    def dev(self):
        d = {"bias": _dev(self.bias)}
        if self.full:
            d["post_scale"], d["post_shift"] = _dev(self.ps), _dev(self.pt)
            d["residual"] = _dev(self.res_bits) if self.bf16 else _dev(np.concatenate(self.res, axis=1))
        return d


def _describe(x, got, idx, what):
    r = tuple(int(i) for i in idx)
    return f"{what}: element {r}, pre-activation {float(x[r])!r} (bits {int(x.view(np.uint32)[r]):#010x}), got {float(got[r])!r}"


def check_f32(got, x, code, alpha, epi, what, impl=None, rows=None):
    """got: the kernel's fp32 output; x: the model's pre-activation (fp32).  Raises with the first offending element."""
    if rows is not None:
        got, x = got[:rows], x[:rows]
    ps = epi.ps[None, :] if epi.full else None
    pt = epi.pt[None, :] if epi.full else None
    a = nm.act(x, code, alpha)
    exact = np.ones(x.shape, bool) if code != nm.ACT_ELU else (x > 0)
    a32 = np.where(exact, a, 0).astype(np.float32)
    c0, c1 = nm.affine(a32, ps, pt) if epi.full else (a32, a32)
    ok = nm.matches_either(got, c0, c1)
    if code == nm.ACT_RELU:
        ok |= (got == 0) & ((c0 == 0) | (c1 == 0))                 # fmaxf(-0, 0) may return either zero
    bad = exact & ~ok
    assert not bad.any(), _describe(x, got, np.argwhere(bad)[0], f"{what}: not the model's bits (stage: " + ("affine" if epi.full else "activation / sum") + ")")
    if code == nm.ACT_ELU:
        neg = ~exact
        nan = neg & np.isnan(x)
        assert np.isnan(got[nan]).all(), f"{what}: ELU of NaN is not NaN"
        neg &= ~nan
        with np.errstate(all="ignore"):
            if epi.full:
                ref = a * ps.astype(np.float64) + pt.astype(np.float64)
                bound = np.abs(ps) * alpha * nm.ELU_BOUND + 2.0 ** -23 * (np.abs(ps) * alpha + np.abs(pt))   # ELU's bound through s, two roundings
            else:
                ref, bound = a, np.full(x.shape, alpha * nm.ELU_BOUND)
            err = np.where(neg, np.abs(got.astype(np.float64) - ref), 0.0)
        if not epi.full and impl:
            ELU_MAX[impl] = max(ELU_MAX.get(impl, 0.0), float(err.max()) / alpha)
            print(f"{what}: ELU[{impl}] alpha={alpha}: max |y - alpha expm1(x)| = {err.max():.3e} (bound {alpha * nm.ELU_BOUND:.3e})")
        bad = neg & ~(err <= np.broadcast_to(bound, x.shape))
        assert not bad.any(), _describe(x, got, np.argwhere(bad)[0], f"{what}: ELU beyond alpha 2^-22 (err {err[bad].max():.3e})")


def check_split(hl, y, what, rows=None):
    """hl: [rows][2 cols] halves as uint16; y: the fp32 output of the same launch with the other output."""
    if rows is not None:
        hl, y = hl[:rows], y[:rows]
    cols = y.shape[1]
    hi, lo = nm.split(y)
    inside = ~nm.flag(y)
    bad = inside & ((hl[:, :cols] != hi) | (hl[:, cols:] != lo))
    if bad.any():
        r = tuple(int(i) for i in np.argwhere(bad)[0])
        stage = "hi" if hl[:, :cols][r] != hi[r] else "lo"
        raise AssertionError(f"{what}: split stage {stage}: element {r}, y = {float(y[r])!r} ({int(y.view(np.uint32)[r]):#010x}): got hi {int(hl[:, :cols][r]):#06x} lo "
                             f"{int(hl[:, cols:][r]):#06x}, model hi {int(hi[r]):#06x} lo {int(lo[r]):#06x}")
    return bool(nm.flag(y).any())


def check_bf16(got_bits, x, code, alpha, epi, what, impl=None):
    """got_bits: bf16 output bit patterns; exact = bf16_rne(model) where the model is exact, ELU's bound plus half a bf16 ulp elsewhere."""
    ps = epi.ps[None, :] if epi.full else None
    pt = epi.pt[None, :] if epi.full else None
    a = nm.act(x, code, alpha)
    exact = np.ones(x.shape, bool) if code != nm.ACT_ELU else (x > 0)
    a32 = np.where(exact, a, 0).astype(np.float32)
    c0, c1 = nm.affine(a32, ps, pt) if epi.full else (a32, a32)
    b0, b1 = nm.bf16_rne(c0), nm.bf16_rne(c1)
    gv = nm.bf16_value(got_bits)
    ok = (got_bits == b0) | (got_bits == b1) | (np.isnan(gv) & np.isnan(c0))
    if code == nm.ACT_RELU:
        ok |= (gv == 0) & (c0 == 0)
    bad = exact & ~ok
    assert not bad.any(), _describe(x, gv, np.argwhere(bad)[0], f"{what}: bf16 output is not the rounded model (want {int(b0[tuple(np.argwhere(bad)[0])]):#06x})")
    if code == nm.ACT_ELU:
        neg = ~exact & ~np.isnan(x)
        assert np.isnan(gv[~exact & np.isnan(x)]).all()
        with np.errstate(all="ignore"):
            if epi.full:
                ref = a * ps.astype(np.float64) + pt.astype(np.float64)
                bound = np.abs(ps) * alpha * nm.ELU_BOUND + 2.0 ** -23 * (np.abs(ps) * alpha + np.abs(pt))
            else:
                ref, bound = a, alpha * nm.ELU_BOUND
            bound = bound + nm.bf16_ulp(np.maximum(np.abs(ref), np.abs(gv.astype(np.float64)))) / 2
            err = np.where(neg, np.abs(gv.astype(np.float64) - ref), 0.0)
        if not epi.full and impl:
            over = np.where(neg, err - nm.bf16_ulp(np.maximum(np.abs(ref), np.abs(gv.astype(np.float64)))) / 2, 0.0).max()
            ELU_MAX[impl] = max(ELU_MAX.get(impl, 0.0), float(over) / alpha)
            print(f"{what}: ELU[{impl}] alpha={alpha}: max (|y - alpha expm1(x)| - half a bf16 ulp) = {over:.3e} (bound {alpha * nm.ELU_BOUND:.3e})")
        bad = neg & ~(err <= bound)
        assert not bad.any(), _describe(x, gv, np.argwhere(bad)[0], f"{what}: ELU beyond alpha 2^-22 + half a bf16 ulp")


# ---- carrier: the split GEMM with identity weights ----------------------------------------------------------------------------------
def _gemm_operands(k, n_out=COLS, rows=ROWS):
    """a = [hi | lo] of the carried sweep [rows][k], w = [0 | I | I] with I repeated down the outputs: acc[r][c] = v[r][c % k] exactly."""
    def make():
        hi, lo, v = (t.reshape(rows, k) for t in nm.carried_pairs(nm.sweep("finite", rows * k)))
        eye = np.zeros((n_out, k), dtype=np.float16)
        eye[np.arange(n_out), np.arange(n_out) % k] = 1.0
        w = np.concatenate([np.zeros_like(eye), eye, eye], axis=1)
        acc = v[:, np.arange(n_out) % k]
        assert np.array_equal(nm.joined(hi, lo), v.astype(np.float64))       # the pair holds the value exactly
        _CACHE[("pairs", k)] = (hi.view(np.float16).astype(np.float32)[:, np.arange(n_out) % k], lo.view(np.float16).astype(np.float32)[:, np.arange(n_out) % k])
        return acc, _dev(np.concatenate([hi, lo], axis=1)), _dev(w.view(np.uint16))
    return _cached(("gemm", k, n_out, rows), make)


def _epi(full, bf16=False, rows=ROWS, cols=COLS):
    def make():
        e = Epi(rows, cols, full, bf16=bf16)
        return e, e.dev()
    return _cached(("epi", full, bf16, rows, cols), make)


def _split_layer(a, w, e_dev, rows, n_out, k, code, alpha, tile, split_out, flag=None, rows_dev=None):
    from librubiks.model import _layer_call
    out = _poison((rows + 1, 2 * n_out), torch.float16) if split_out else _poison((rows + 1, n_out), torch.float32)
    kw = dict(e_dev)
    kw["out_hi_lo" if split_out else "out_f32"] = out
    if flag is not None:
        kw["range_flag"] = flag
    if rows_dev is not None:
        kw["rows_dev"] = rows_dev
    _layer_call("rc_split_layer_f16", a=a, w=w, n_rows=rows, n_out=n_out, k=k, activation=code, alpha=alpha, tile=tile, k_splits=1, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 6])
def test_split_layer_whole_k_every_tile(tile):
    """rc_split_layer_f16, whole K, k = n_out = 256, W_hi = I, W_lo = 0: acc = lo 2^-11 + hi = v exactly.  Tiles 1 .. 6, fp32 output against
    the model, halves against the split of that output, the flag against the model's, the guard row untouched."""
    acc, a, w = _gemm_operands(COLS)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    for full in (False, True):
        epi, e_dev = _epi(full)
        x = epi.pre(acc)
        for code, alpha in ACTS:
            what = f"rc_split_layer_f16 tile {tile} act {code} alpha {alpha} {'residual+affine' if full else 'plain'}"
            f32 = _split_layer(a, w, e_dev, ROWS, COLS, COLS, code, alpha, tile, False)
            assert _untouched(f32[ROWS]), what + ": wrote past the last row"
            y = _host(f32[:ROWS])
            check_f32(y, x, code, alpha, epi, what, impl="act_value (GEMM epilogue)")
            flag.zero_()
            hl = _split_layer(a, w, e_dev, ROWS, COLS, COLS, code, alpha, tile, True, flag=flag)
            assert _untouched(hl[ROWS]), what + ": wrote past the last row (halves)"
            want_flag = check_split(_host(hl[:ROWS]), y, what)
            assert int(flag.item()) == int(want_flag), what + ": range flag"


@pytest.mark.parametrize("tile", [1, 3])
@pytest.mark.parametrize("R", [1, 17, 336, 353])
def test_split_layer_with_a_device_row_count(tile, R):
    """The rows_dev forms: rows < R get the model's bits, rows >= R (and the guard row) stay untouched, the flag sees rows < R only."""
    acc, a, w = _gemm_operands(COLS)
    rows_dev = torch.tensor([R], dtype=torch.int32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    for full, (code, alpha) in ((False, (2, 0.37)), (True, (2, 2.5)), (True, (0, 0.37))):
        epi, e_dev = _epi(full)
        x = epi.pre(acc)
        what = f"rc_split_layer_f16 rows_dev R={R} tile {tile} act {code} alpha {alpha}"
        f32 = _split_layer(a, w, e_dev, ROWS, COLS, COLS, code, alpha, tile, False, rows_dev=rows_dev)
        assert _untouched(f32[R:]), what + ": a row >= R was written"
        y = _host(f32[:R])
        check_f32(y, x, code, alpha, epi, what, rows=R)
        flag.zero_()
        hl = _split_layer(a, w, e_dev, ROWS, COLS, COLS, code, alpha, tile, True, flag=flag, rows_dev=rows_dev)
        assert _untouched(hl[R:]), what + ": a row >= R was written (halves)"
        assert int(flag.item()) == int(check_split(_host(hl[:R]), y, what)), what + ": range flag"


# ---- the range flag's edge --------------------------------------------------------------------------------------------------------
def _edge_cases():
    """(name, value placed in ONE element, flag expected)."""
    up = np.nextafter(np.float32(65504.0), np.float32(np.inf))
    return [("65504", np.float32(65504.0), 0), ("-65504", np.float32(-65504.0), 0), ("next float above 65504", up, 1), ("next below -65504", -up, 1),
            ("+inf", np.float32(np.inf), 1), ("-inf", np.float32(-np.inf), 1), ("NaN", np.float32(np.nan), 1)]


def _tame(v):
    """The sweep with everything beyond +-65504 pulled onto it: the largest value IS 65504 and the flag must stay 0."""
    return np.clip(v, -65504.0, 65504.0).astype(np.float32)


@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 6])
def test_range_flag_edge_of_the_gemm_epilogue(tile):
    """65504 gives no flag; the next float, +-inf and NaN in a single element do (finite ones through the operand, the others through the
    skip connection: an infinite operand would meet the zeros of W); behind a device row count the element in row R raises nothing."""
    from librubiks.model import _layer_call
    acc, _, w = _gemm_operands(COLS)
    bias = torch.full((COLS,), -0.0, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.empty((ROWS + 1, 2 * COLS), dtype=torch.float16, device="cuda")
    base = _tame(acc)
    assert base.max() == 65504.0 and base.min() == -65504.0
    zero_res = np.zeros((ROWS, 2 * COLS), dtype=np.uint16)
    for name, val, want in [("the tame sweep", None, 0)] + _edge_cases():
        for r, c in ((0, 0), (ROWS - 1, COLS - 1), (200, 129)) if val is not None else ((0, 0),):
            v, res = base.copy(), zero_res.copy()
            if val is not None and np.isfinite(val):
                v[r, c] = val
            elif val is not None:
                res[r, c] = np.float16(val).view(np.uint16)
                v[r, c] = 1.0
            hi, lo = nm.split(v)
            a = _dev(np.concatenate([hi, lo], axis=1))
            for code in (0, 2):
                flag.zero_()
                _layer_call("rc_split_layer_f16", a=a, w=w, bias=bias, residual=_dev(res), n_rows=ROWS, n_out=COLS, k=COLS, activation=code, alpha=0.37,
                            tile=tile, k_splits=1, out_hi_lo=out, range_flag=flag)
                w_eff = 0 if (code == 2 and val is not None and val < 0) else want          # ELU of a large negative value is -alpha
                assert int(flag.item()) == w_eff, f"tile {tile} act {code}: {name} at ({r}, {c}): flag {int(flag.item())}, want {w_eff}"
    if tile in (1, 3):
        for R in (1, 17, 336):
            v = base.copy()
            v[R, 5] = np.nextafter(np.float32(65504.0), np.float32(np.inf))
            hi, lo = nm.split(v)
            a = _dev(np.concatenate([hi, lo], axis=1))
            for rr, want in ((R, 0), (R + 1, 1)):
                flag.zero_()
                o = _poison((ROWS + 1, 2 * COLS), torch.float16)
                _layer_call("rc_split_layer_f16", a=a, w=w, bias=bias, n_rows=ROWS, n_out=COLS, k=COLS, activation=0, alpha=1.0, tile=tile, k_splits=1,
                            out_hi_lo=o, range_flag=flag, rows_dev=torch.tensor([rr], dtype=torch.int32, device="cuda"))
                assert int(flag.item()) == want and _untouched(o[rr:]), (tile, R, rr)


# ---- carrier: K cut into chunks + the reduce kernels ---------------------------------------------------------------------------------
def _reduce(lib, part, stride, P, n_corr, rows, cols, e_dev, code, alpha, want_hl, want_f32, flag, rows_dev=None):
    from librubiks import _hip
    hl = _poison((rows + 1, 2 * cols), torch.float16) if want_hl else None
    f32 = _poison((rows + 1, cols), torch.float32) if want_f32 else None
    p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    args = (part.data_ptr(), stride, P, n_corr, rows, cols, e_dev["bias"].data_ptr(), p(e_dev.get("residual")), code, alpha, p(e_dev.get("post_scale")),
            p(e_dev.get("post_shift")), p(hl), p(f32), p(flag))
    if rows_dev is None:
        _hip.check(lib.rc_split_reduce_f16(*args, None), "rc_split_reduce_f16")
    else:
        _hip.check(lib.rc_split_reduce_rows_f16(*args, rows_dev.data_ptr(), None), "rc_split_reduce_rows_f16")
    torch.cuda.synchronize()
    return hl, f32


@pytest.mark.parametrize("tile,S", [(0, 2), (3, 2), (7, 2), (0, 3), (3, 3), (7, 3)])
def test_partials_and_reduce(tile, S):
    """out_partials with k = 128: k_splits = 2 puts the 2^-11 scaling inside chunk 1 (three K-steps per chunk), k_splits = 3 gives two
    correction chunks.  The partial sums are exact, so they are compared bit for bit; rc_split_reduce_f16 and its rows form then finish
    the layer under the full contract."""
    from librubiks.model import _layer_call
    _hip, lib = _lib()
    k = 128
    acc, a, w = _gemm_operands(k)
    hi, lo = _CACHE[("pairs", k)]                                   # the operand halves as fp32: acc = hi + lo / 2048 exactly
    col = (np.arange(COLS) % k)[None, :]
    zero = np.zeros_like(acc)
    if S == 2:      # chunk 0: K-steps 0 .. 2 = hi W_lo (0) and the first half of lo W_hi; chunk 1: the rest, scaled, plus hi W_hi
        want = [np.where(col < 64, lo, zero), np.where(col >= 64, lo * np.float32(1.0 / 2048.0), zero) + hi]
    else:           # chunks of two K-steps: hi W_lo = 0 | lo W_hi | hi W_hi
        want = [zero, lo, hi]
    n_corr = lib.rc_split_layer_corr_chunks(k, S)
    assert n_corr == S - 1
    part = _poison((S * ROWS + 1, COLS), torch.float32)
    _layer_call("rc_split_layer_f16", a=a, w=w, n_rows=ROWS, n_out=COLS, k=k, out_partials=part, k_splits=S, tile=tile)
    torch.cuda.synchronize()
    assert _untouched(part[S * ROWS]), "partials: wrote past the last chunk"
    got = _host(part[:S * ROWS]).reshape(S, ROWS, COLS)
    for p in range(S):
        bad = got[p] != want[p]
        assert not bad.any(), _describe(acc, got[p], np.argwhere(bad)[0], f"partials tile {tile} k_splits {S} chunk {p}")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    for full in (False, True):
        epi, e_dev = _epi(full)
        x = epi.pre(acc)
        for code, alpha in ACTS:
            what = f"rc_split_reduce_f16 behind tile {tile} k_splits {S} act {code} alpha {alpha} full={full}"
            flag.zero_()
            hl, f32 = _reduce(lib, part, ROWS * COLS, S, n_corr, ROWS, COLS, e_dev, code, alpha, True, True, flag)
            assert _untouched(hl[ROWS]) and _untouched(f32[ROWS]), what
            y = _host(f32[:ROWS])
            check_f32(y, x, code, alpha, epi, what, impl="expm1f (reduce)")
            assert int(flag.item()) == int(check_split(_host(hl[:ROWS]), y, what)), what + ": range flag"
    epi, e_dev = _epi(True)
    x = epi.pre(acc)
    for R in (1, 17, 336, 353):
        flag.zero_()
        hl, f32 = _reduce(lib, part, ROWS * COLS, S, n_corr, ROWS, COLS, e_dev, 2, 0.37, True, True, flag, rows_dev=torch.tensor([R], dtype=torch.int32, device="cuda"))
        assert _untouched(hl[R:]) and _untouched(f32[R:]), f"rc_split_reduce_rows_f16 R={R}: a row >= R was written"
        y = _host(f32[:R])
        check_f32(y, x, 2, 0.37, epi, f"rc_split_reduce_rows_f16 R={R}", rows=R)
        assert int(flag.item()) == int(check_split(_host(hl[:R]), y, f"rc_split_reduce_rows_f16 R={R}"))


def _raw_pair():
    """c = the raw sweep, c_corr = a second sweep times 2048 (corr_scale = 2^-11 returns it exactly): y = c + second, one fp32 addition."""
    def make():
        c = nm.sweep("raw").reshape(ROWS, COLS)
        second = nm.sweep("finite", seed=5)[np.random.RandomState(9).permutation(ROWS * COLS)].reshape(ROWS, COLS)
        second = np.where(np.arange(COLS)[None, :] % 2 == 0, np.float32(-0.0), second).astype(np.float32)    # even columns: c alone reaches the epilogue
        with np.errstate(all="ignore"):
            cc = second * np.float32(2048.0)
            acc = c + cc * np.float32(1.0 / 2048.0)
        return c, cc, acc
    return _cached("rawpair", make)


@pytest.mark.parametrize("P", [1, 2, 9])
def test_reduce_kernel_fed_directly(P):
    """rc_split_reduce_f16 on raw values (+-inf, NaN, -0, fp32 denormals): n_partials 1, 2 and 9 with the sweep in one main partial and
    the second sweep times 2048 in one correction partial, the others zero."""
    _hip, lib = _lib()
    c, cc, acc2 = _raw_pair()
    if P == 1:
        parts, n_corr, acc = [c], 0, c + np.float32(0.0)            # the kernel's sum starts at +0: -0 does not survive it
    elif P == 2:
        with np.errstate(all="ignore"):
            parts, n_corr, acc = [cc, c], 1, (cc + np.float32(0.0)) * np.float32(1.0 / 2048.0) + c
    else:
        z = np.zeros_like(c)
        parts, n_corr = [z, z, cc, z, z, z, z, c, z], 4
        with np.errstate(all="ignore"):
            acc = (cc + np.float32(0.0)) * np.float32(1.0 / 2048.0) + c + np.float32(0.0)
    part = _dev(np.stack(parts))
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    for full in (False, True):
        epi, e_dev = _epi(full)
        x = epi.pre(acc)
        for code, alpha in ACTS:
            what = f"rc_split_reduce_f16 n_partials {P} act {code} alpha {alpha} full={full}"
            flag.zero_()
            hl, f32 = _reduce(lib, part, ROWS * COLS, P, n_corr, ROWS, COLS, e_dev, code, alpha, True, True, flag)
            y = _host(f32[:ROWS])
            check_f32(y, x, code, alpha, epi, what, impl="expm1f (reduce)")
            assert int(flag.item()) == int(check_split(_host(hl[:ROWS]), y, what)) == 1, what + ": range flag"
            assert _untouched(hl[ROWS]) and _untouched(f32[ROWS])
    # the flag's edge, one element at a time; and behind a device row count
    epi, e_dev = _epi(False)
    base = _tame(np.nan_to_num(acc, nan=1.0))
    for name, val, want in [("the tame sweep", None, 0)] + _edge_cases():
        v = base.copy()
        if val is not None:
            v[ROWS - 1, COLS - 1] = val
        flag.zero_()
        part1 = _dev(np.stack([np.zeros_like(v)] * (P - 1) + [v]))
        _reduce(lib, part1, ROWS * COLS, P, 0, ROWS, COLS, e_dev, 0, 1.0, True, False, flag)
        assert int(flag.item()) == want, f"rc_split_reduce_f16 P={P}: {name}: flag {int(flag.item())}, want {want}"
        if val is not None and want:
            for R, w2 in ((ROWS - 1, 0), (ROWS, 1)):
                flag.zero_()
                hl, _ = _reduce(lib, part1, ROWS * COLS, P, 0, ROWS, COLS, e_dev, 0, 1.0, True, False, flag, rows_dev=torch.tensor([R], dtype=torch.int32, device="cuda"))
                assert int(flag.item()) == w2 and _untouched(hl[R:]), f"rc_split_reduce_rows_f16 P={P} R={R}: {name}"


def test_split_act_kernel_fed_directly():
    """rc_split_act_f16 (no residual, no affine, no flag): c alone and c + 2^-11 c_corr on raw values."""
    _hip, lib = _lib()
    c, cc, acc2 = _raw_pair()
    epi, e_dev = _epi(False)
    dc, dcc = _dev(c), _dev(cc)
    for with_corr in (False, True):
        x = epi.pre(acc2 if with_corr else c)
        for code, alpha in ACTS:
            what = f"rc_split_act_f16 corr={with_corr} act {code} alpha {alpha}"
            hl, f32 = _poison((ROWS + 1, 2 * COLS), torch.float16), _poison((ROWS + 1, COLS), torch.float32)
            _hip.check(lib.rc_split_act_f16(dc.data_ptr(), dcc.data_ptr() if with_corr else None, 1.0 / 2048.0, ROWS, COLS, e_dev["bias"].data_ptr(), code, alpha,
                                            hl.data_ptr(), f32.data_ptr(), None), "rc_split_act_f16")
            torch.cuda.synchronize()
            assert _untouched(hl[ROWS]) and _untouched(f32[ROWS]), what
            y = _host(f32[:ROWS])
            check_f32(y, x, code, alpha, epi, what, impl="expm1f (split_act)")
            check_split(_host(hl[:ROWS]), y, what)


# ---- carrier: the split head ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [512, 1024])
def test_split_head_reads_the_hidden_activation_through_selector_rows(K):
    """rc_head_split_f32 / ..._rows_f32 with w[o] = e_{32 o}, bias_o = 0: out[i][o] is y[i][32 o], the hidden activation the kernel never
    writes.  Finite values only (an infinite activation would meet the zeros of w); the sums add zeros, so -0 comes back as +0."""
    _hip, lib = _lib()
    n = ROWS * COLS // 16
    v = nm.sweep("finite").reshape(n, 16)
    second = nm.sweep("finite", seed=5)[np.random.RandomState(9).permutation(ROWS * COLS)].reshape(n, 16)
    second = np.where(np.arange(16)[None, :] % 2 == 0, np.float32(0.0), np.clip(second, -6e4, 6e4)).astype(np.float32)
    c, cc = np.zeros((n, K), dtype=np.float32), np.zeros((n, K), dtype=np.float32)
    c[:, ::32][:, :16], cc[:, ::32][:, :16] = v, second * np.float32(2048.0)
    with np.errstate(all="ignore"):
        acc = v + second
    w = np.zeros((16, K), dtype=np.float32)
    w[np.arange(16), 32 * np.arange(16)] = 1.0
    rng = np.random.RandomState(4)
    dc, dcc, dw, bo = _dev(c), _dev(cc), _dev(w), torch.zeros(16, device="cuda")
    R = n - 37
    src_map = rng.permutation(n).astype(np.int32)
    rows_dev, dmap = torch.tensor([R], dtype=torch.int32, device="cuda"), _dev(src_map)
    for full in (False, True):
        bias_h = np.full(K, -0.0, dtype=np.float32)
        if full:
            bias_h[::32] = rng.standard_normal(K // 32).astype(np.float32)
        epi = Epi(n, 16, False)
        epi.bias = bias_h[::32][:16].copy()
        x = epi.pre(acc)
        dbh = _dev(bias_h)
        for code, alpha in ACTS:
            what = f"rc_head_split_f32 K={K} act {code} alpha {alpha} bias={full}"
            out = _poison((n + 1, 16), torch.float32)
            _hip.check(lib.rc_head_split_f32(dc.data_ptr(), dcc.data_ptr(), 1.0 / 2048.0, n, K, dbh.data_ptr(), code, alpha, dw.data_ptr(), bo.data_ptr(), 16,
                                             out.data_ptr(), None), "rc_head_split_f32")
            torch.cuda.synchronize()
            assert _untouched(out[n]), what
            got = _host(out[:n]) + np.float32(0.0)
            with np.errstate(all="ignore"):
                xz = x + np.float32(0.0)                                    # -0 pre-activations: the head's sums return +0 for them
            check_f32(got, np.where(x == 0, xz, x), code, alpha, epi, what, impl="act_value (head)")
            mapped = _poison((n + 1, 16), torch.float32)
            _hip.check(lib.rc_head_split_rows_f32(dc.data_ptr(), dcc.data_ptr(), 1.0 / 2048.0, n, K, dbh.data_ptr(), code, alpha, dw.data_ptr(), bo.data_ptr(), 16,
                                                  mapped.data_ptr(), rows_dev.data_ptr(), dmap.data_ptr(), None), "rc_head_split_rows_f32")
            torch.cuda.synchronize()
            m = _host(mapped)
            assert np.array_equal(m[src_map[:R]].view(np.uint32), _host(out[:R]).view(np.uint32)), what + ": the rows form differs from the plain one"
            rest = np.ones(n + 1, bool)
            rest[src_map[:R]] = False
            assert np.isnan(m[rest]).all(), what + ": a row no packed row maps to was written"


# ---- carrier: the input layer ----------------------------------------------------------------------------------------------------------
def _states(n, seed):
    rng = np.random.RandomState(seed)
    s = np.tile(oc.get_solved(), (n, 1))
    for _ in range(30):
        s = oc.multi_rotate_actions(s, rng.randint(0, 12, n))
    return s


def _input_layer(H, kind):
    """Column c reads cubie c % 20 only: table row 24 j + code is zero in every column but those with c % 20 == j, where it holds the sweep
    value of (code, c).  y[i][c] = bias[c] + value(code of cubie c % 20 in state i, c)."""
    def make():
        s = _states(ROWS, 11)
        for j in range(20):
            assert len(set(s[:, j])) == 24, f"cubie {j}: not every code occurs"
        vals = nm.sweep(kind, 24 * H).reshape(24, H)
        if kind != "carried":
            vals = vals + np.float32(0.0)                             # no -0: 0 + -0 loses it
        table = np.zeros((480, H), dtype=np.float32)
        cj = np.arange(H) % 20
        for code in range(24):
            table[24 * cj + code, np.arange(H)] = vals[code]
        acc = vals[s[:, cj], np.arange(H)[None, :]]                   # [ROWS][H]
        return s, table, acc
    return _cached(("input", H, kind), make)


def _sample(v, n):
    """n of the sweep's values: the anchors' neighbourhoods, zeros, denormals and ties (its first 2 300 values) whole, the rest evenly thinned."""
    idx = np.concatenate([np.arange(2300), np.linspace(2300, v.size - 1, n - 2300).astype(np.int64)])
    return np.ascontiguousarray(v[idx])


def _table_acc(table, s):
    H = table.shape[1]
    cj = np.arange(H) % 20
    return table[24 * cj[None, :] + s[:, cj], np.arange(H)[None, :]]


@pytest.mark.parametrize("form", [0, 1, 2])
def test_input_layer_as_a_sum_of_rows_against_the_model(form):
    """rc_first_layer_gather_f16 (form 0) and both forms of rc_first_layer_gather_rows_f16, H = 4096: every one of the 24 x 4096 table values is
    a sweep value (raw: +-inf and NaN included -- the sum adds zeros to it), all 24 codes occur for every cubie."""
    from librubiks.cube import DeviceCubes
    _hip, lib = _lib()
    H = 4096
    s, table, acc = _input_layer(H, "raw")
    cubes = DeviceCubes.from_numpy(s)
    dt = _dev(table)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    rng = np.random.RandomState(2)
    R = ROWS - 16
    src_map = rng.permutation(ROWS).astype(np.int32)
    rows_dev, dmap = torch.tensor([R], dtype=torch.int32, device="cuda"), _dev(src_map)
    for full in (False, True):
        epi = Epi(ROWS, H, False)
        if full:
            epi.bias = rng.standard_normal(H).astype(np.float32)
        else:
            epi.bias = np.zeros(H, dtype=np.float32)
        x = epi.pre(acc)
        if form:
            x = x[src_map]
        db = _dev(epi.bias)
        for code, alpha in ACTS:
            what = f"rc_first_layer_gather form {form} act {code} alpha {alpha} bias={full}"
            out = _poison((ROWS + 1, 2 * H), torch.float16)
            flag.zero_()
            if form == 0:
                _hip.check(lib.rc_first_layer_gather_f16(cubes.soa.data_ptr(), ROWS, cubes.stride, dt.data_ptr(), db.data_ptr(), out.data_ptr(), H, code, alpha,
                                                         flag.data_ptr(), None), "rc_first_layer_gather_f16")
                rows = ROWS
            else:
                _hip.check(lib.rc_first_layer_gather_rows_f16(cubes.soa.data_ptr(), ROWS, cubes.stride, dt.data_ptr(), db.data_ptr(), out.data_ptr(), H, code, alpha,
                                                              flag.data_ptr(), rows_dev.data_ptr(), dmap.data_ptr(), form, None), "rc_first_layer_gather_rows_f16")
                rows = R
            torch.cuda.synchronize()
            assert _untouched(out[rows:]), what + ": a row that does not exist was written"
            hl = _host(out[:rows])
            # this kernel has no fp32 output: hi + lo 2^-11 carries y to 22 bits, so hi is compared bit for bit where the model is exact and the
            # pair against the model's pair; ELU's negative side within its bound plus the pair's own 2^-22 relative
            check_pair(hl, x[:rows], code, alpha, what, flag, impl="act_value (input layer, through the half pair)")


def check_pair(hl, x, code, alpha, what, flag, impl):
    cols = x.shape[1]
    a = nm.act(x, code, alpha)
    exact = np.ones(x.shape, bool) if code != nm.ACT_ELU else (x > 0)
    y = np.where(exact, a, 0).astype(np.float32)
    hi, lo = nm.split(y)
    inside = ~nm.flag(y) & exact
    ghi, glo = hl[:, :cols], hl[:, cols:]
    same = (ghi == hi) & (glo == lo)
    if code == nm.ACT_RELU:
        same |= (y == 0) & ((ghi & 0x7FFF) == 0) & ((glo & 0x7FFF) == 0)
    bad = inside & ~same
    if bad.any():
        r = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: split stage {'hi' if ghi[r] != hi[r] else 'lo'}: element {r}, pre-activation {float(x[r])!r}: got {int(ghi[r]):#06x} {int(glo[r]):#06x}, "
                             f"model {int(hi[r]):#06x} {int(lo[r]):#06x}")
    want_flag = bool(nm.flag(y)[exact].any())
    if code == nm.ACT_ELU:
        neg = ~exact & ~np.isnan(x)
        got = nm.joined(ghi, glo)
        with np.errstate(all="ignore"):
            err = np.where(neg, np.abs(got - a), 0.0)
            bound = alpha * nm.ELU_BOUND + 2.0 ** -21 * np.abs(a)           # the pair keeps 22 bits: two roundings of 2^-11 relative each
        ELU_MAX[impl] = max(ELU_MAX.get(impl, 0.0), float(err.max()) / alpha)
        print(f"{what}: ELU[{impl}] alpha={alpha}: max |hi + lo 2^-11 - alpha expm1(x)| = {err.max():.3e}")
        bad = neg & ~(err <= bound)
        assert not bad.any(), _describe(x, got.astype(np.float32), np.argwhere(bad)[0], f"{what}: ELU beyond its bound")
        want_flag |= bool(np.isnan(x).any())                                # NaN stays NaN through ELU; the negative side is within [-alpha, 0]
    if flag is not None:
        assert int(flag.item()) == int(want_flag), what + f": range flag {int(flag.item())}, model {int(want_flag)}"


def test_input_layer_on_the_matrix_cores_against_the_model():
    """rc_first_layer_split_flag_f16: hi / lo tables of the carried sweep (acc = hi + 2^-11 lo exactly), H = 4096."""
    from librubiks.cube import DeviceCubes
    _hip, lib = _lib()
    H = 4096
    s, table, _ = _input_layer(H, "carried")
    table = _tame(table)                                              # (a pair can hold 65520, but no table of pairs made by split has it)
    acc = _table_acc(table, s)
    cubes = DeviceCubes.from_numpy(s)
    thi, tlo = nm.split(np.ascontiguousarray(table.T))                # [H][480]
    assert np.array_equal(nm.joined(thi, tlo), table.T.astype(np.float64))
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    # The accumulators start at the bias and the matrix cores add the products to it with a rounding of their own, so bias + value is no
    # single fp32 addition: the sweep goes through the table with bias 0, then through the bias with a table of zeros (0 + bias is exact).
    for through_bias in (False, True):
        epi = Epi(ROWS, H, False)
        epi.bias = _sample(nm.sweep("carried"), H) if through_bias else np.zeros(H, dtype=np.float32)
        x = epi.pre(np.zeros_like(acc) if through_bias else acc)
        db = _dev(epi.bias)
        dhi, dlo = (_dev(np.zeros_like(thi)), _dev(np.zeros_like(tlo))) if through_bias else (_dev(thi), _dev(tlo))
        full = through_bias
        for code, alpha in ACTS:
            what = f"rc_first_layer_split_flag_f16 act {code} alpha {alpha} bias={full}"
            out = _poison((ROWS + 1, 2 * H), torch.float16)
            flag.zero_()
            _hip.check(lib.rc_first_layer_split_flag_f16(cubes.soa.data_ptr(), ROWS, cubes.stride, dhi.data_ptr(), dlo.data_ptr(), db.data_ptr(), out.data_ptr(), H,
                                                         code, alpha, flag.data_ptr(), None), "rc_first_layer_split_flag_f16")
            torch.cuda.synchronize()
            assert _untouched(out[ROWS]), what
            check_pair(_host(out[:ROWS]), x, code, alpha, what, flag, impl="act_value (input layer, through the half pair)")


def test_input_layer_range_flag_edge():
    """The input-layer kernels' flag: 65504 in the table gives none; the next float, +-inf and NaN in ONE table entry (one that a state reads) do."""
    from librubiks.cube import DeviceCubes
    _hip, lib = _lib()
    H = 256
    s = _states(ROWS, 11)
    cubes = DeviceCubes.from_numpy(s)
    base = _tame(nm.sweep("finite", 480 * H, seed=2).reshape(480, H) * (np.arange(H)[None, :] % 20 == (np.arange(480) // 24)[:, None]))
    bias = torch.zeros(H, device="cuda")
    out = torch.empty((ROWS, 2 * H), dtype=torch.float16, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ident, all_rows = torch.arange(ROWS, dtype=torch.int32, device="cuda"), torch.tensor([ROWS], dtype=torch.int32, device="cuda")
    j, c = 7, 47                                                       # column 47 reads cubie 7
    row = 24 * j + int(s[ROWS - 1, j])
    for name, val, want in [("the tame table", None, 0)] + _edge_cases():
        t = base.copy()
        t[24 * 3 + int(s[0, 3]), 3] = 65504.0
        if val is not None:
            t[row, c] = val
        dt = _dev(t)
        for code in (0, 2):
            for form in (0, 1, 2):
                flag.zero_()
                if form == 0:
                    rc = lib.rc_first_layer_gather_f16(cubes.soa.data_ptr(), ROWS, cubes.stride, dt.data_ptr(), bias.data_ptr(), out.data_ptr(), H, code, 0.37, flag.data_ptr(), None)
                else:
                    rc = lib.rc_first_layer_gather_rows_f16(cubes.soa.data_ptr(), ROWS, cubes.stride, dt.data_ptr(), bias.data_ptr(), out.data_ptr(), H, code, 0.37,
                                                            flag.data_ptr(), all_rows.data_ptr(), ident.data_ptr(), form, None)
                _hip.check(rc, "rc_first_layer_gather")
                w_eff = 0 if (code == 2 and val is not None and val < 0) else want      # ELU of a large negative value is -alpha
                assert int(flag.item()) == w_eff, f"gather form {form} act {code}: {name}: flag {int(flag.item())}, want {w_eff}"
        if val is None or np.isfinite(val):
            dthi, dtlo = (_dev(h) for h in nm.split(np.ascontiguousarray(t.T)))
            for code in (0, 2):
                flag.zero_()
                _hip.check(lib.rc_first_layer_split_flag_f16(cubes.soa.data_ptr(), ROWS, cubes.stride, dthi.data_ptr(), dtlo.data_ptr(), bias.data_ptr(),
                                                             out.data_ptr(), H, code, 0.37, flag.data_ptr(), None), "rc_first_layer_split_flag_f16")
                w_eff = 0 if (code == 2 and val is not None and val < 0) else want
                assert int(flag.item()) == w_eff, f"split_flag act {code}: {name}: flag {int(flag.item())}, want {w_eff}"


# ---- the bf16 kernels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [1, 3, 4])
def test_bf16_layer_kernel_against_the_model(tile):
    """rc_gemm_layer_bf16 with W = I: acc is the bf16 operand itself; with the bf16 skip connection y = acc + residual carries 16 significant
    bits and sits on bf16's ties.  Output = bf16_rne(model)."""
    from librubiks.model import _layer_call

    def make():
        v = nm.sweep("finite").reshape(ROWS, COLS)
        with np.errstate(all="ignore"):
            top = nm.bf16_value(nm.bf16_rne(v))
            top = np.where(np.isfinite(top), top, np.float32(0.0)).astype(np.float32)
            low = nm.bf16_value(nm.bf16_rne((v - top).astype(np.float32)))
        return top, low
    top, low = _cached("bf16gemm", make)
    a = _dev(nm.bf16_rne(top)).view(torch.bfloat16)
    w = torch.eye(COLS, dtype=torch.bfloat16, device="cuda")
    for mode in ("plain", "residual", "full"):
        epi = Epi(ROWS, COLS, mode == "full", bf16=True)
        kw = epi.dev()
        if mode == "residual":
            epi.res = (low,)
            kw["residual"] = _dev(nm.bf16_rne(low))
        x = epi.pre(top + np.float32(0.0))                         # (the accumulator starts at +0: a -0 operand comes out as +0)
        if mode == "residual":
            assert nm.classes(x)["bf16 tie, rounds down"].any() and nm.classes(x)["bf16 tie, rounds up"].any()
        for code, alpha in ACTS:
            what = f"rc_gemm_layer_bf16 tile {tile} {mode} act {code} alpha {alpha}"
            out = _poison((ROWS + 1, COLS), torch.bfloat16)
            _layer_call("rc_gemm_layer_bf16", a=a, w=w, n_rows=ROWS, n_out=COLS, k=COLS, activation=code, alpha=alpha, tile=tile, k_splits=1, out_bf16=out, **kw)
            torch.cuda.synchronize()
            assert _untouched(out[ROWS]), what
            check_bf16(_host(out[:ROWS]), x, code, alpha, epi, what, impl="act_value (bf16 GEMM epilogue)")


def test_inplace_activation_on_every_bf16_value():
    """rc_act_bf16_inplace on all 65 536 bf16 bit patterns, NaNs and infinities included."""
    _hip, lib = _lib()
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16).reshape(256, 256)
    x = nm.bf16_value(bits)
    epi = Epi(256, 256, False)
    for code, alpha in ACTS[1:]:
        t = _dev(bits)
        _hip.check(lib.rc_act_bf16_inplace(t.data_ptr(), 65536, code, alpha, None), "rc_act_bf16_inplace")
        torch.cuda.synchronize()
        check_bf16(_host(t), x, code, alpha, epi, f"rc_act_bf16_inplace act {code} alpha {alpha}", impl="exp - 1 (bf16 kernels)")


def test_bf16_head_reads_the_activation_through_selector_rows():
    """rc_head_bf16, K = 1024, w[o] = e_{32 o}: out[i][o] = bf16(act(x[i][32 o])) as a float, every finite bf16 value in x."""
    _hip, lib = _lib()
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    bits = bits[np.isfinite(nm.bf16_value(bits))]
    n = bits.size // 16
    bits = bits[:n * 16].reshape(n, 16)
    xin = np.zeros((n, 1024), dtype=np.uint16)
    xin[:, ::32][:, :16] = bits
    w = np.zeros((16, 1024), dtype=np.float32)
    w[np.arange(16), 32 * np.arange(16)] = 1.0
    dx, dw, bo = _dev(xin), _dev(nm.bf16_rne(w)), torch.zeros(16, device="cuda")
    x = nm.bf16_value(bits)
    epi = Epi(n, 16, False)
    for code, alpha in ACTS:
        what = f"rc_head_bf16 act {code} alpha {alpha}"
        out = _poison((n + 1, 16), torch.float32)
        _hip.check(lib.rc_head_bf16(dx.data_ptr(), n, 1024, dw.data_ptr(), bo.data_ptr(), 16, out.data_ptr(), code, alpha, None), "rc_head_bf16")
        torch.cuda.synchronize()
        assert _untouched(out[n]), what
        got = _host(out[:n])
        gb = nm.bf16_rne(got)
        assert np.array_equal(nm.bf16_value(gb).view(np.uint32), got.view(np.uint32)), what + ": an output that is no bf16 value"
        check_bf16(gb, x + np.float32(0.0), code, alpha, epi, what, impl="exp - 1 (bf16 kernels)")


@pytest.mark.parametrize("table", ["half", "bf16"])
def test_bf16_input_layer_against_the_model(table):
    """rc_first_layer_mfma_bf16, H = 4096, tables in IEEE half and in bf16: acc = the table value of (code, column), y = acc + bias in fp32."""
    from librubiks.cube import DeviceCubes
    _hip, lib = _lib()
    H = 4096
    s, tab, _ = _input_layer(H, "carried")
    tab = _tame(tab)
    with np.errstate(all="ignore"):
        if table == "half":
            tb = nm.split(np.ascontiguousarray(tab.T))[0]
            tv = tb.view(np.float16).astype(np.float32)
        else:
            tb = nm.bf16_rne(np.ascontiguousarray(tab.T))
            tv = nm.bf16_value(tb)
    acc = _table_acc(np.ascontiguousarray(tv.T), s)
    cubes = DeviceCubes.from_numpy(s)
    # (bias + value is summed on the matrix cores, with their rounding: the sweep goes through the table with bias 0, then through the
    #  fp32 bias with a table of zeros -- full fp32 values in front of the bf16 rounding)
    for through_bias in (False, True):
        epi = Epi(ROWS, H, False)
        epi.bias = (_sample(nm.sweep("finite"), H) + np.float32(0.0)) if through_bias else np.zeros(H, dtype=np.float32)
        x = epi.pre(np.zeros_like(acc) if through_bias else acc)
        db = _dev(epi.bias)
        dt = _dev(np.zeros_like(tb) if through_bias else tb)
        full = through_bias
        for code, alpha in ACTS:
            what = f"rc_first_layer_mfma_bf16 table {table} act {code} alpha {alpha} bias={full}"
            out = _poison((ROWS + 1, H), torch.bfloat16)
            _hip.check(lib.rc_first_layer_mfma_bf16(cubes.soa.data_ptr(), ROWS, cubes.stride, dt.data_ptr(), db.data_ptr(), out.data_ptr(), H, code, alpha,
                                                    int(table == "half"), None), "rc_first_layer_mfma_bf16")
            torch.cuda.synchronize()
            assert _untouched(out[ROWS]), what
            check_bf16(_host(out[:ROWS]), x, code, alpha, epi, what, impl="exp - 1 (bf16 kernels)")


# ---- engine level: alpha through model.py ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ["fc_small", "res_small"])
def test_engines_carry_alpha_through_every_layer_plan(arch):
    """ELU(alpha = 0.37) through SplitF32Net and the bf16 InferenceNet at 300, 5 632 and 11 264 rows (library or cut plan, K-cut plan,
    fused plan) against the float64 module, under the bounds of test_engines_at_every_launch_size_of_a_narrowing_search:
    split <= 1.25 e_fp32 + 2e-7 scale, bf16 <= 2e-2 scale."""
    import copy
    from test_net_gpu import _model, _res_model
    from librubiks import cube
    from librubiks.model import F32_SPLIT, InferenceNet, Model, ModelConfig, SplitF32Net, make_inference_net
    act = torch.nn.ELU(alpha=0.37)
    if arch == "fc_small":
        net = _model(act)
    else:
        torch.manual_seed(0)
        net = Model.create(ModelConfig(architecture=arch, activation_function=act)).eval()
        donor = _res_model()
        net.load_state_dict(donor.state_dict())           # the perturbed batch-norm statistics of _res_model
    assert any(isinstance(m, torch.nn.ELU) and m.alpha == 0.37 for m in net.modules())
    ref64 = copy.deepcopy(net).double()
    split, bf16 = make_inference_net(net, F32_SPLIT), make_inference_net(net, torch.bfloat16)
    assert isinstance(split, SplitF32Net) and isinstance(bf16, InferenceNet)
    np.random.seed(6)
    for n in (300, 5632, 11264):
        cubes, _, _ = cube.scramble_batch(n, 25, True)
        oh = cubes.as_oh(torch.float32)
        with torch.no_grad():
            p64, v64 = ref64(oh.double())
            p32, v32 = net(oh)
        v64, v32 = v64.reshape(-1), v32.reshape(-1)
        err = lambda p, v: max(float((p.double() - p64).abs().max()), float((v.double().reshape(-1) - v64).abs().max()))   # noqa: E731
        scale = max(1.0, float(p64.abs().max()), float(v64.abs().max()))
        e_f32 = err(p32, v32)
        e_split, e_bf = err(*split.forward_cubes(cubes)), err(*bf16.forward_cubes(cubes))
        assert not split.overflowed()
        print(f"{arch} alpha=0.37 n={n}: |out| <= {scale:.2f}; max |err| vs float64: split {e_split:.2e}, fp32 module {e_f32:.2e}, bf16 {e_bf:.2e}")
        assert e_split <= 1.25 * e_f32 + 2e-7 * scale, (n, e_split, e_f32)
        assert e_bf <= 2e-2 * scale, (n, e_bf)
    # alpha = 1 would not pass: the module with the default ELU is further from this one than a hundred times the bound
    with torch.no_grad():
        other = copy.deepcopy(net)
        for m in other.modules():
            if isinstance(m, torch.nn.ELU):
                m.alpha = 1.0
        p1, _ = other(oh)
    assert float((p1.double() - p64).abs().max()) > 100 * (1.25 * e_f32 + 2e-7 * scale)


def test_zz_measured_elu_maxima():
    """Prints the measured maximum per ELU implementation (of the tests above that ran in this session: the figures of DESIGN.md 3.3) and
    holds each to the bound; a figure taken through a half pair carries the pair's own rounding and was held to its bound where it was taken."""
    for impl, worst in sorted(ELU_MAX.items()):
        print(f"ELU[{impl}]: max |y - alpha expm1(x)| / alpha = {worst:.3e}  (bound {nm.ELU_BOUND:.3e})")
        assert worst <= nm.ELU_BOUND or "half pair" in impl, impl
