"""
A plain NumPy model of the contract that ends every layer of the network kernels (include/rubiks_hip.h, rc_split_layer_t):

    y  = post_scale * act(acc + bias + residual) + post_shift
    hi = half(y)                         (round to nearest even)
    lo = half((y - hi) * 2^11)
    *range_flag |= 1   iff   !(|y| <= 65504)

on fp32 arrays, in the kernels' order of operations, and `sweep()`: a deterministic set of fp32 values that sits on every edge
of that contract (ELU's switch points, ties of both 16-bit formats, subnormals, the rim of half's range).  tests/test_netmath_model.py
checks the model against itself on the CPU; tests/test_epilogue_gpu.py holds every kernel to it element by element.
"""
import numpy as np

F32 = np.float32
HALF_MAX = 65504.0
ACT_NONE, ACT_RELU, ACT_ELU = 0, 1, 2
ELU_BOUND = 2.0 ** -22          # |y - alpha expm1(x)| <= alpha * ELU_BOUND for x <= 0: 2.4 x the ~1e-7 rubiks_netmath.h states
ROWS, COLS = 353, 256           # one full 352-row tile plus one row; `sweep` fills exactly this matrix by default
_ANCHORS = (-0.35, -1.0, 65504.0, -65504.0, 65520.0, -65520.0, 2.0 ** -14, -2.0 ** -14, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, -2.0 ** -25)


def f32(x):
    return np.asarray(x, dtype=F32)


# ---- stages of the epilogue ------------------------------------------------------------------------------------------------
def pre(acc, bias, residual_hi=None, residual_lo=None):
    """acc + bias, then + (hi + lo / 2048) with the residual formed first: fp32 operations in the kernels' order.
    residual_hi / residual_lo: float16 arrays (or uint16 bit patterns); a bf16 residual is passed as fp32 in residual_hi alone."""
    with np.errstate(all="ignore"):
        y = f32(acc) + f32(bias)
        if residual_hi is not None:
            hi = _halves(residual_hi)
            r = hi if residual_lo is None else hi + _halves(residual_lo) * F32(1.0 / 2048.0)
            y = y + r
    return y


def _halves(h):
    h = np.asarray(h)
    if h.dtype == np.uint16:
        h = h.view(np.float16)
    return h.astype(F32)


def act(x, code, alpha=1.0):
    """Identity and ReLU exactly (fp32); ELU in float64 (returned as float64: the kernels are held to it within alpha * ELU_BOUND
    where x <= 0 and exactly where x > 0)."""
    x = f32(x)
    if code == ACT_NONE:
        return x
    if code == ACT_RELU:
        return np.where(x > 0, x, F32(0.0)).astype(F32)       # fmaxf(x, 0): NaN -> 0, -0 -> either zero (compare with ==)
    with np.errstate(all="ignore"):
        x64 = x.astype(np.float64)
        return np.where(x > 0, x64, float(alpha) * np.expm1(x64))


def affine(y, s, t):
    """y * s + t both ways a compiler may emit it: (fused, unfused) = (float64 product and sum rounded once, two fp32 roundings).
    A kernel may give either, chosen per element."""
    y, s, t = f32(y), f32(s), f32(t)
    with np.errstate(all="ignore"):
        fused = (y.astype(np.float64) * s.astype(np.float64) + t.astype(np.float64)).astype(F32)
        unfused = (y * s).astype(F32) + t
    return fused, unfused


def matches_either(got, a, b):
    """Elementwise: got equals a or b (NaN equals NaN; +0 equals -0 only where both candidates are zeros of either sign)."""
    got, a, b = f32(got), f32(a), f32(b)
    same = lambda u, v: (u.view(np.uint32) == v.view(np.uint32)) | (np.isnan(u) & np.isnan(v))   # noqa: E731
    return same(got, a) | same(got, b)


def split(y):
    """(hi, lo) as uint16 bit patterns: hi = half(y), lo = half((y - hi) * 2048), every step rounded to nearest even."""
    y = f32(y)
    with np.errstate(all="ignore"):
        hi = y.astype(np.float16)
        lo = ((y - hi.astype(F32)) * F32(2048.0)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def split_fma(y):
    """The form rubiks_netmath.h::split_pair computes: lo = half(fma(hi, -2^11, y * 2^11)), the fma rounded once to fp32."""
    y = f32(y)
    with np.errstate(all="ignore"):
        hi = y.astype(np.float16)
        t = y * F32(2048.0)
        l32 = (hi.astype(np.float64) * -2048.0 + t.astype(np.float64)).astype(F32)      # both products exact in float64, their sum too
        lo = l32.astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def joined(hi, lo):
    """float64 value hi + lo / 2048 of a split pair (bit patterns or float16)."""
    with np.errstate(all="ignore"):
        return _halves(hi).astype(np.float64) + _halves(lo).astype(np.float64) / 2048.0


def flag(y):
    with np.errstate(all="ignore"):
        return ~(np.abs(f32(y)) <= F32(HALF_MAX))


def bf16_rne(y):
    """fp32 -> bf16 bit patterns (uint16), round to nearest even; NaN stays NaN (quiet)."""
    u = f32(y).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(f32(y)), ((u >> 16) | 0x40).astype(np.uint16), r)


def bf16_value(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


def bf16_ulp(v):
    """Spacing of bf16 at |v| (float64; the subnormal spacing 2^-133 below 2^-126)."""
    a = np.abs(np.asarray(v, dtype=np.float64))
    with np.errstate(all="ignore"):
        e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    return 2.0 ** (np.maximum(np.where(a > 0, e, -126.0), -126.0) - 7)


# ---- rubiks_netmath.h::expm1_neg, emulated --------------------------------------------------------------------------------
def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + np.float64(c)).astype(F32)


def expm1_neg_emulated(x, switch=-0.35):
    """expm1_neg with fp32 roundings emulated through float64 and a correctly rounded exp: (polynomial branch, exp branch, selected)."""
    x = f32(x)
    p = np.full(x.shape, F32(1.0 / 40320.0), dtype=F32)
    for c in (F32(1.0 / 5040.0), F32(1.0 / 720.0), F32(1.0 / 120.0), F32(1.0 / 24.0), F32(1.0 / 6.0), F32(0.5), F32(1.0)):
        p = _fma32(p, x, c)
    with np.errstate(all="ignore"):
        poly = (p * x).astype(F32)
        ex = np.exp(x.astype(np.float64)).astype(F32) - F32(1.0)
    return poly, ex, np.where(x < F32(switch), ex, poly)


# ---- the sweep ----------------------------------------------------------------------------------------------------------------
def _around(v, ulps=64):
    c = np.array([v], dtype=F32).view(np.int32)[0]
    return (np.arange(c - ulps, c + ulps + 1, dtype=np.int64).astype(np.int32)).view(F32)


def half_midpoints():
    """Exact midpoints between adjacent halves, fp32-exact: normal binades 2^-14 .. 2^15 (every second) and the subnormal range; the
    lower neighbour's mantissa even (the tie rounds down) and odd (rounds up); both signs."""
    out = []
    mant = np.array([0, 1, 2, 3, 340, 341, 511, 512, 1022, 1023], dtype=np.float64)
    for e in range(-14, 16, 2):
        out.append((1024.0 + mant + 0.5) * 2.0 ** (e - 10))
    out.append((mant + 0.5) * 2.0 ** -24)                       # subnormal halves; (0 + 0.5) 2^-24 = 2^-25: hi = 0 by the tie
    m = np.concatenate(out)
    return np.concatenate([m, -m]).astype(F32)


def bf16_midpoints():
    mant = np.array([0, 1, 2, 3, 42, 43, 63, 64, 126, 127], dtype=np.float64)
    m = np.concatenate([(128.0 + mant + 0.5) * 2.0 ** (e - 7) for e in range(-40, 41, 5)])
    return np.concatenate([m, -m]).astype(F32)


def _raw_specials():
    parts = [_around(a) for a in _ANCHORS]
    parts.append(np.array([0.0, -0.0], dtype=F32))
    den = np.array([1, 2, 3, 1 << 10, (1 << 22) + 1, (1 << 23) - 1], dtype=np.uint32)
    parts += [den.view(F32), (den | np.uint32(0x80000000)).view(F32)]                       # fp32 denormals
    parts += [half_midpoints(), bf16_midpoints()]
    parts.append(-np.exp(np.linspace(np.log(2.0 ** -30), np.log(110.0), 4096)).astype(F32))   # exp underflows at -104: ELU = -alpha
    parts.append(np.array([-1e30, -104.0, -87.5, -88.0], dtype=F32))
    return np.concatenate(parts)


def sweep(kind="raw", n=ROWS * COLS, seed=0):
    """n fp32 values (default 353 x 256 = 90 368): the special values above, then Gaussians scaled by 1e-3, 1, 30 and 3000 in turn.
    kind "raw": with +-inf and NaN.  "finite": without.  "carried": only values a split pair holds exactly, v = hi + lo 2^-11 with hi
    finite -- each special value and Gaussian is replaced by what its split carries, which is checked to be an fp32 number."""
    assert kind in ("raw", "finite", "carried")
    s = _raw_specials()
    if kind == "raw":
        s = np.concatenate([s, np.array([np.inf, -np.inf, np.nan], dtype=F32)])
    assert s.size <= n, (s.size, n)
    rng = np.random.RandomState(seed)
    g = rng.standard_normal(n - s.size) * np.array([1e-3, 1.0, 30.0, 3000.0])[np.arange(n - s.size) % 4]
    v = np.concatenate([s, g.astype(F32)])
    if kind == "carried":
        v = carried(v)
    return v


def carried_pairs(v):
    """(hi, lo, value): the split pair of each v (bit patterns) and the fp32 number hi + lo / 2048 it carries.  Values whose hi is not
    finite (|v| >= 65520) are replaced by +-65504 first.  Asserts that every pair's value is an fp32 number.  (A pair can hold 65520 =
    65504 + 32768 / 2048, which is not the pair of any value: split(65520) has hi = inf.)"""
    v = f32(v)
    hi, lo = split(v)
    bad = ~np.isfinite(hi.view(np.float16))
    v = np.where(bad, np.copysign(F32(HALF_MAX), v), v).astype(F32)
    hi, lo = split(v)
    j = joined(hi, lo)
    assert np.array_equal(j.astype(F32).astype(np.float64), j), "a split pair that fp32 does not hold exactly"
    return hi, lo, j.astype(F32) + F32(0.0)          # (-0 becomes +0, as in an accumulator that starts at +0)


def carried(v):
    return carried_pairs(v)[2]


def classes(v):
    """Masks of the value classes a sweep must contain (tests assert that each is present)."""
    v = f32(v)
    a = np.abs(v.astype(np.float64))
    with np.errstate(all="ignore"):
        hf = v.astype(np.float16).astype(np.float64)
        hb = v.astype(np.float16).view(np.uint16)
        fin = np.isfinite(v) & np.isfinite(hf)
        e = np.floor(np.log2(np.where(fin & (a > 0), a, 1.0)))
        # a tie: an odd multiple of half the spacing of the 16-bit format at |v|; it rounds away from zero when the neighbour below is odd
        sp = np.where(a < 2.0 ** -14, 2.0 ** -24, 2.0 ** (e - 10))
        q = a / (sp / 2)
        tie = fin & (a > 0) & (q == np.floor(q)) & (np.floor(q) % 2 == 1)
        below = np.floor(a / sp) % 2 == 1
        bs = 2.0 ** (np.maximum(e, -126.0) - 7)
        bq = a / (bs / 2)
        btie = np.isfinite(v) & (a > 0) & (bq == np.floor(bq)) & (np.floor(bq) % 2 == 1)
        bbelow = np.floor(a / bs) % 2 == 1
    return {
        "half tie, rounds down (towards zero)": tie & ~below,
        "half tie, rounds up (away from zero)": tie & below,
        "half tie, subnormal": tie & (a < 2.0 ** -14),
        "hi subnormal": fin & (a < 2.0 ** -14) & (hf != 0),
        "hi zero, value not": fin & (hf == 0) & (a > 0),
        "2^-25: hi = 0 by the tie": a == 2.0 ** -25,
        "just above 2^-25: hi = 2^-24": (a > 2.0 ** -25) & (a < 2.0 ** -25 * 1.0001),
        "fp32 denormal": (a > 0) & (a < 2.0 ** -126),
        "+0": (v == 0) & ~np.signbit(v),
        "-0": (v == 0) & np.signbit(v),
        "65504": a == HALF_MAX,
        "next float above 65504": v == np.nextafter(F32(HALF_MAX), F32(np.inf)),
        "(65504, 65520): hi = 65504, flagged": (a > HALF_MAX) & (a < 65520.0),
        "ELU switch -0.35, both sides": (v >= np.nextafter(F32(-0.35), F32(-1))) & (v <= np.nextafter(F32(-0.35), F32(0))),
        "-1, both sides": (v >= np.nextafter(F32(-1), F32(-2))) & (v <= np.nextafter(F32(-1), F32(0))),
        "exp underflow (x < -104)": v < -104,
        "tiny negative (|x| < 2^-24)": (v < 0) & (a < 2.0 ** -24),
        "bf16 tie, rounds down": btie & ~bbelow,
        "bf16 tie, rounds up": btie & bbelow,
        "hi odd mantissa": fin & ((hb & 1) == 1),
    }


RAW_ONLY = ("fp32 denormal", "-0")      # a split pair carries neither (an accumulator that starts at +0 never returns -0)
