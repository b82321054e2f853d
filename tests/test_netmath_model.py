"""
CPU checks of tests/netmath_model.py, the NumPy model that tests/test_epilogue_gpu.py holds the network kernels' epilogues to: the
sweep contains every value class it promises and every carried value is exact, the subtract-then-scale split equals the fused form
of rubiks_netmath.h::split_pair, the round-to-nearest-even helpers give hand-written ties, and the emulated expm1_neg stays inside
what the header states.
"""
import numpy as np
import pytest

import netmath_model as nm


@pytest.mark.parametrize("kind", ["raw", "finite", "carried"])
def test_sweep_is_deterministic_and_holds_every_value_class(kind):
    v = nm.sweep(kind)
    assert v.dtype == np.float32 and v.shape == (nm.ROWS * nm.COLS,)
    assert np.array_equal(v.view(np.uint32), nm.sweep(kind).view(np.uint32))
    assert (np.isnan(v).any() and np.isinf(v).any()) == (kind == "raw")
    absent = set(nm.RAW_ONLY) | {"just above 2^-25: hi = 2^-24"} if kind == "carried" else set()   # (a pair rounds those onto the tie itself)
    for name, mask in nm.classes(v).items():
        assert bool(mask.any()) != (name in absent), (kind, name)
    for anchor in nm._ANCHORS:                          # every float within 64 ulp of each anchor
        if kind != "carried":
            assert np.isin(nm._around(anchor), v).all(), anchor
    for scale in (1e-3, 1.0, 30.0, 3000.0):             # the Gaussian bulk, each scale
        assert ((np.abs(v) > scale / 2) & (np.abs(v) < scale * 2)).sum() > 5000, scale


def test_carried_values_are_exactly_what_a_split_pair_holds():
    raw = nm.sweep("finite")
    v = nm.carried(raw)                                 # asserts float64(hi) + float64(lo) / 2048 == float32(that) for every value
    assert np.abs(v).max() == 65520.0                   # 65519.996 = 65504 + 32760 / 2048 whose lo rounds to 32768: a pair CAN hold 65520
    v = v[np.abs(v) < 65520.0]
    hi, lo = nm.split(v)
    assert np.isfinite(hi.view(np.float16)).all() and np.isfinite(lo.view(np.float16)).all()
    assert np.array_equal(nm.joined(hi, lo), v.astype(np.float64))          # a fixed point: the pair of a carried value IS the value
    assert np.array_equal(nm.carried(v).view(np.uint32), v.view(np.uint32))
    # the same for a dense set of other fp32 values: every split pair is an fp32 number
    rng = np.random.RandomState(1)
    bits = rng.randint(0, 2 ** 32, 800000, dtype=np.uint64).astype(np.uint32)
    x = bits.view(np.float32)
    x = x[np.isfinite(x) & (np.abs(x) < 65520.0)]
    nm.carried(x)
    assert nm.flag(np.float32(65504.0)) == False and nm.flag(np.nextafter(np.float32(65504.0), np.float32(np.inf))) == True   # noqa: E712
    assert nm.flag(np.float32(np.nan)) and nm.flag(np.float32(-np.inf)) and not nm.flag(np.float32(-65504.0))


def test_split_equals_the_fused_form_of_split_pair():
    """rubiks_netmath.h: "(y - hi) * 2^11 is formed as fma(hi, -2^11, y * 2^11): both products are exact and their difference is
    representable, so the single rounding returns exactly what the subtract-then-scale form returns"."""
    for kind in ("finite", "carried"):
        v = nm.sweep(kind)
        v = v[np.abs(v) < 65520.0]                      # beyond: hi = inf, lo = NaN both ways, the range flag's business
        a, b = nm.split(v), nm.split_fma(v)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # the claim fails where y * 2^11 underflows: fp32 denormals below 2^-137 lose bits in the product -- but lo rounds to 0 both ways
    den = nm.sweep("raw")
    den = den[(np.abs(den) < 2.0 ** -126)]
    assert np.array_equal(nm.split(den)[1] & 0x7FFF, np.zeros(den.size, np.uint16)) and np.array_equal(nm.split_fma(den)[1] & 0x7FFF, np.zeros(den.size, np.uint16))


def test_round_to_nearest_even_on_hand_written_ties():
    h = lambda x: int(nm.split(np.float32(x))[0])                 # noqa: E731
    assert h(1.0 + 2.0 ** -11) == 0x3C00                          # 1 + half an ulp: ties to the even 1.0
    assert h(1.0 + 3 * 2.0 ** -11) == 0x3C02                      # between 0x3C01 and 0x3C02: to the even one, upwards
    assert h(np.nextafter(np.float32(1.0 + 2.0 ** -11), np.float32(2))) == 0x3C01
    assert h(2.0 ** -25) == 0x0000 and h(np.nextafter(np.float32(2.0 ** -25), np.float32(1))) == 0x0001   # half the smallest subnormal
    assert h(3 * 2.0 ** -25) == 0x0002 and h(-3 * 2.0 ** -25) == 0x8002
    assert h(2.0 ** -14 - 2.0 ** -25) == 0x0400                   # between the largest subnormal (odd) and the smallest normal
    assert h(65504.0) == 0x7BFF and h(65519.996) == 0x7BFF and h(65520.0) == 0x7C00 and h(-65520.0) == 0xFC00
    hi, lo = nm.split(np.float32(1.0 + 2.0 ** -11))
    assert (int(hi), int(lo)) == (0x3C00, 0x3C00)                 # lo = 2^-11 * 2048 = 1.0
    hi, lo = nm.split(np.nextafter(np.float32(65504.0), np.float32(np.inf)))
    assert (int(hi), int(lo)) == (0x7BFF, 0x4800)                 # 65504 + 2^-8: lo = 8.0
    b = lambda x: int(nm.bf16_rne(np.float32(x)))                 # noqa: E731
    assert b(1.0 + 2.0 ** -8) == 0x3F80 and b(1.0 + 3 * 2.0 ** -8) == 0x3F82 and b(-(1.0 + 3 * 2.0 ** -8)) == 0xBF82
    assert b(np.nextafter(np.float32(1.0 + 2.0 ** -8), np.float32(2))) == 0x3F81
    assert b(3.3895314e38) == 0x7F7F and b(3.4e38) == 0x7F80      # the largest bf16; beyond its rounding boundary: inf
    assert b(np.inf) == 0x7F80 and b(-0.0) == 0x8000
    assert np.isnan(nm.bf16_value(nm.bf16_rne(np.float32(np.nan))))
    assert np.isnan(nm.bf16_value(nm.bf16_rne(np.array([0x7F800001], dtype=np.uint32).view(np.float32))))[0]   # a NaN whose payload would round away
    v = nm.sweep("finite")
    import torch
    assert np.array_equal(nm.bf16_rne(v).view(np.int16), torch.from_numpy(v).to(torch.bfloat16).view(torch.int16).numpy())


def test_affine_and_pre_follow_the_kernels_order():
    y, s, t = np.float32(1.0 + 2.0 ** -12), np.float32(1.0 + 2.0 ** -12), np.float32(-1.0)
    fused, unfused = nm.affine(y, s, t)
    assert float(fused) == 2.0 ** -11 + 2.0 ** -24 and float(unfused) == 2.0 ** -11          # the product's low bit survives only fused
    assert nm.matches_either(unfused, fused, unfused) and not nm.matches_either(np.float32(0.0), fused, unfused)
    # the residual is formed first: (acc + bias) + (hi + lo / 2048), not ((acc + bias) + hi) + lo / 2048
    acc, bias = np.float32(2.0 ** 24), np.float32(0.0)
    hi, lo = np.float16(1.0), np.float16(1024.0)                                             # 1 + 0.5
    assert float(nm.pre(acc, bias, hi, lo)) == 2.0 ** 24 + 2.0                               # 1.5 added at once rounds up to even
    assert float((acc + np.float32(1.0)) + np.float32(0.5)) == 2.0 ** 24                     # ... one at a time both are lost
    x = np.array([-1.0, -0.0, 0.0, 2.5, np.nan], dtype=np.float32)
    assert np.array_equal(nm.act(x, nm.ACT_RELU), np.array([0, 0, 0, 2.5, 0], dtype=np.float32))
    e = nm.act(x, nm.ACT_ELU, 0.37)
    assert e[0] == 0.37 * np.expm1(-1.0) and e[3] == 2.5 and np.isnan(e[4])
    assert nm.act(np.float32(-200.0), nm.ACT_ELU, 2.5) == -2.5


def test_emulated_expm1_neg_stays_inside_the_headers_statement():
    """rubiks_netmath.h states ~1e-7 absolute for expm1_neg.  With a correctly rounded exp the two sides' floors are printed; the
    GPU tests allow alpha * 2^-22 (2.4e-7) on top for v_exp_f32's ulp and the rounding of x * log2(e).  A switch point at -1
    instead of -0.35 costs the polynomial side its truncation error and must show."""
    xp = -np.linspace(0.0, 0.35, 400001).astype(np.float32)
    xe = -np.exp(np.linspace(np.log(0.35), np.log(110.0), 400001)).astype(np.float32)
    xe = xe[xe < np.float32(-0.35)]
    poly, _, sel_p = nm.expm1_neg_emulated(xp)
    _, ex, sel_e = nm.expm1_neg_emulated(xe)
    assert np.array_equal(sel_p, poly) and np.array_equal(sel_e, ex)
    floor_p = float(np.abs(poly - np.expm1(xp.astype(np.float64))).max())
    floor_e = float(np.abs(ex - np.expm1(xe.astype(np.float64))).max())
    print(f"expm1_neg emulated: polynomial side {floor_p:.2e}, exp side {floor_e:.2e} (header: ~1e-7; the GPU bound: {nm.ELU_BOUND:.2e})")
    assert floor_p <= 3.0e-8 and floor_e <= 6.0e-8           # half an ulp below 0.5 / half an ulp of exp below 1 + half an ulp of the difference
    x1 = -np.linspace(0.35, 1.0, 100001).astype(np.float32)
    moved = nm.expm1_neg_emulated(x1, switch=-1.0)[2]
    assert float(np.abs(moved - np.expm1(x1.astype(np.float64))).max()) > 10 * nm.ELU_BOUND   # 2.8e-6: the GPU bound catches a moved switch
    assert nm.expm1_neg_emulated(np.float32(-200.0))[2] == -1.0
