"""The primary ray's pixel coordinates uf = (x + ru) / w, vf = (y + rv) / h as
k_render_bins forms them (bih_pixdiv.h): with y = fl(1 / d) formed once,
q = fl(n y), r = fma(-q, d, n), result = fma(r, y, q) -- no division sequence.
DESIGN.md section 4.14 proves this the IEEE quotient for integer d up to 65536;
above that the kernel keeps the division.

Here the library's own host copy (bih_pixel_divide) and a numpy restatement
are compared with numpy's float32 division, on the numerators the kernel can
form and on contiguous blocks of floats where a rounding error would show
first: zero mismatches.  The bare product n y is wrong on the same inputs, so
the two fma are what is being tested.
"""
import ctypes as C

import numpy as np
import pytest

F32, F64, U32 = np.float32, np.float64, np.uint32
LIMIT = 65536                                  # kPixelDivideMax
WIDTHS = (1, 2, 3, 7, 208, 320, 333, 641, 1023, 1080, 1920, 2047, 2160, 3840, 4095, 65535, 65536)
ABOVE = LIMIT + 1
SAMPLE = 1 << 22
BLOCK = 1 << 18


def uniforms(words):
    """dev::xorwow_to_uniform (_curand_uniform) of u32 words, in f32."""
    return (words.astype(F32) * F32(2.3283064e-10) + F32(2.3283064e-10) / F32(2.0)).astype(F32)


R_LO, R_HI = uniforms(np.array([0, 0xFFFFFFFF], U32))


def block(start, count, down=False):
    """`count` consecutive floats from `start` (upwards, or downwards)."""
    b = np.array([start], F32).view(U32)[0].astype(np.int64)
    k = np.arange(count, dtype=np.int64)
    return (b - k if down else b + k).astype(U32).view(F32)


@pytest.fixture(scope="module")
def words():
    """The seeded sample: 2^22 pixel columns in [0, 1) of the width and 2^22
    draws, the smallest and the largest word among them."""
    rng = np.random.default_rng(14)
    frac = rng.random(SAMPLE)
    w = rng.integers(0, 2 ** 32, SAMPLE, dtype=np.uint64).astype(U32)
    w[:4] = (0, 0xFFFFFFFF, 1, 0xFFFFFF7F)
    return frac, w


def numerators(d, words):
    """Every kind of numerator of width d: fl(x + ru) of the sample (x < d;
    the first and last column with the smallest and largest ru among them),
    all floats just below d (and d itself, which x = d - 1 with ru = 1
    gives), around 1, and from the smallest numerator 2^-33 up."""
    frac, w = words
    x = np.minimum((frac * d).astype(np.int64), d - 1)
    x[:4] = (0, 0, d - 1, d - 1)
    ru = uniforms(w)
    assert ru[0] == R_LO and ru[1] == R_HI == F32(1.0) and R_LO == F32(2.0 ** -33)
    n = (x.astype(F32) + ru).astype(F32)
    parts = [n, block(F32(d), BLOCK, down=True), block(F32(1.0), BLOCK // 2), block(F32(1.0), BLOCK // 2, down=True),
             block(R_LO, BLOCK)]
    n = np.concatenate(parts)
    assert (n > 0).all() and np.isfinite(n).all()
    return np.ascontiguousarray(n)


def fma32(a, b, c):
    """fl(a b + c) on f32 arrays, one rounding.  a b is exact in f64 (48
    bits); TwoSum gives the f64 sum's error, which decides the only case where
    rounding the f64 sum to f32 would round twice: the f64 sum exactly half
    way between two floats."""
    p = a.astype(F64) * b.astype(F64)
    c = c.astype(F64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    out = s.astype(F32)
    lo = np.where(out.astype(F64) <= s, out, np.nextafter(out, F32(-np.inf)))
    hi = np.where(out.astype(F64) >= s, out, np.nextafter(out, F32(np.inf)))
    tie = (lo != hi) & (s == (lo.astype(F64) + hi.astype(F64)) / 2) & (err != 0)
    return np.where(tie, np.where(err > 0, hi, lo), out).astype(F32)


def restated(n, d):
    """bih_pixel_divide in numpy: (quotients, the bare product n y)."""
    df = F32(d)
    if d > LIMIT:
        return (n / df).astype(F32), None
    y = F32(1.0) / df
    q = (n * y).astype(F32)
    r = fma32(-q, np.full_like(n, df), n)
    return fma32(r, np.full_like(n, y), q), q


def library(bihrt, n, d):
    out = np.empty_like(n)
    flag = C.c_uint32(7)
    rc = bihrt._lib.load().bih_pixel_divide(d, n.ctypes.data, n.size, out.ctypes.data, C.byref(flag))
    assert rc == 0
    return out, flag.value


def test_fma_restatement():
    """fma32 against exact rational arithmetic on products that land on and
    next to rounding midpoints."""
    from fractions import Fraction
    rng = np.random.default_rng(2)
    a = rng.standard_normal(4000).astype(F32)
    b = rng.standard_normal(4000).astype(F32)
    c = (-(a.astype(F64) * b.astype(F64))).astype(F32)                 # heavy cancellation
    c[::2] = rng.standard_normal(2000).astype(F32)
    # exact ties (1 + 2^-24, and above an odd float), and sums whose f64
    # rounding lands on a tie: 2^20 + 2^-3 + 2^-4 (1 -+ 2^-46), where rounding
    # twice goes to the even neighbour and one rounding does not
    up, dn = F32(1.0) + F32(2.0 ** -23), F32(1.0) - F32(2.0 ** -23)
    q = F32(0.25)
    a = np.concatenate([a, np.array([2.0 ** -12, 2.0 ** -12, q * up, q * up, q * dn], F32)])
    b = np.concatenate([b, np.array([2.0 ** -12, 2.0 ** -12, q * dn, q * up, q * dn], F32)])
    c = np.concatenate([c, np.array([1.0, 1.0 + 2.0 ** -23, 2.0 ** 20 + 2.0 ** -3, 2.0 ** 20 + 2.0 ** -3,
                                     2.0 ** 20 + 2.0 ** -3], F32)])
    got = fma32(a, b, c)
    assert got[-3] != got[-2]                  # the two sides of the tie
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        g = float(got[i])
        lo, hi = float(np.nextafter(got[i], F32(-np.inf))), float(np.nextafter(got[i], F32(np.inf)))
        e = abs(Fraction(g) - exact)
        assert e <= abs(Fraction(lo) - exact) and e <= abs(Fraction(hi) - exact), i
        if e == abs(Fraction(lo) - exact) or e == abs(Fraction(hi) - exact):
            assert (int(got[i:i + 1].view(U32)[0]) & 1) == 0, i           # a tie goes to even


@pytest.mark.parametrize("d", WIDTHS)
def test_reciprocal_form_is_the_quotient(d, words, bihrt_mod):
    """Zero mismatches with float32 division, for the library's host copy and
    for the restatement; the bare product mismatches at every width that is
    no power of two (at a power of two y is exact, and so is n y)."""
    n = numerators(d, words)
    want = (n / F32(d)).astype(F32)
    got, flag = library(bihrt_mod, n, d)
    rst, bare = restated(n, d)
    bad_lib, bad_rst = int((got.view(U32) != want.view(U32)).sum()), int((rst.view(U32) != want.view(U32)).sum())
    bad_bare = int((bare.view(U32) != want.view(U32)).sum())
    print(f"d {d}: {n.size} numerators, mismatches library {bad_lib} restated {bad_rst} bare product {bad_bare} "
          f"({bad_bare / n.size:.3f})")
    assert flag == 1
    assert bad_lib == 0 and bad_rst == 0
    assert (bad_bare > 0) == (d & (d - 1) != 0), (d, bad_bare)


def test_above_the_limit_takes_the_division(words, bihrt_mod):
    """One above the proof's limit: the library reports the division, and its
    quotients are numpy's."""
    n = numerators(ABOVE, words)
    got, flag = library(bihrt_mod, n, ABOVE)
    assert flag == 0
    assert np.array_equal(got.view(U32), (n / F32(ABOVE)).astype(F32).view(U32))
    assert np.array_equal(restated(n, ABOVE)[0].view(U32), got.view(U32))
    # arguments
    L = bihrt_mod._lib.load()
    assert L.bih_pixel_divide(0, n.ctypes.data, 1, got.ctypes.data, None) != 0
    assert L.bih_pixel_divide(5, None, 1, got.ctypes.data, None) != 0
    assert L.bih_pixel_divide(5, None, 0, None, None) == 0
