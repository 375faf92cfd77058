"""Segment queries (BIH_QUERY_CLOSEST_WITHIN / BIH_QUERY_OCCLUDED_WITHIN,
DESIGN.md section 4.5.1): rays with a far end t_hi, bih_ray's last float.

Both queries are defined on the BIH_QUERY_CLOSEST result of the same {o, t_lo,
d}: that record counts when its t < t_hi (one strict f32 compare).  So the
expected values are tests/test_trace.py's `expected` (OracleTree.closest plus
its numpy f32 u, v) filtered by that compare in numpy f32; every comparison is
on bits.  The rays are test_trace's ray sets, answered by the oracle once.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import test_trace as tt
from test_trace import F32, FLT_MAX, assert_hits, balanced, bits, expected, ray_set, scene

CASES = ("0.5*t", "t", "nextafter(t)", "2*t")


def within(exp, t_hi):
    """The segment queries' answers from the closest records `exp`: (records of
    CLOSEST_WITHIN, bytes of OCCLUDED_WITHIN)."""
    import bihrt
    t_hi = np.broadcast_to(np.asarray(t_hi, F32), exp.shape)
    with np.errstate(invalid="ignore"):
        ok = (exp["prim"] != bihrt.NO_HIT) & (exp["t"] < t_hi)      # NaN: False
    rec = np.zeros(exp.shape[0], bihrt.HIT_DTYPE)
    rec["t"], rec["prim"] = FLT_MAX, bihrt.NO_HIT
    rec[ok] = exp[ok]
    return rec, ok.astype(np.uint8)


def case_t_hi(exp):
    """Each ray's t_hi, cycling over four cases of its own oracle t (0.5 t; t,
    which must not count; the next float above t, which must; 2 t); 1 for a
    miss.  The cycle runs over the hit rays (the k-th of them takes case k % 4:
    the sets aim every other ray at a triangle, so a cycle over all rays would
    leave two cases nearly empty).  Returns (t_hi, case index per ray)."""
    import bihrt
    t = exp["t"].astype(F32)
    case = (np.cumsum(exp["prim"] != bihrt.NO_HIT) - 1) % 4
    with np.errstate(over="ignore"):
        cand = np.stack([F32(0.5) * t, t, np.nextafter(t, F32(np.inf)), F32(2.0) * t], 1)
    t_hi = cand[np.arange(t.shape[0]), case].astype(F32)
    t_hi[exp["prim"] == bihrt.NO_HIT] = F32(1.0)
    return t_hi, case


@functools.lru_cache(maxsize=None)
def segment_set(name):
    """(rays with the four-case t_hi, the closest records, CLOSEST_WITHIN's
    records, OCCLUDED_WITHIN's bytes) of ray_set(name, "mixed"); read-only."""
    import bihrt
    rays0, exp = ray_set(name, "mixed")
    t_hi, case = case_t_hi(exp)
    rays = bihrt.pack_rays(rays0["o"], rays0["d"], rays0["t_lo"], t_hi)
    rec, occ = within(exp, t_hi)
    hit = exp["prim"] != bihrt.NO_HIT
    # by construction: each case holds a quarter of the hit rays, cases 0 and 1 are cut off
    for k in range(4):
        assert (case[hit] == k).sum() >= 0.10 * hit.sum(), (name, CASES[k])
    assert not occ[hit & (case < 2)].any() and occ[hit & (case >= 2)].all()
    for a in (rays, rec, occ):
        a.setflags(write=False)
    return rays, exp, rec, occ


class Dev(tt.Dev):
    """test_trace.Dev for any query: the segment queries' outputs are sized as
    their plain counterparts'."""

    def __init__(self, rays, query):
        import bihrt
        super().__init__(rays, query & ~bihrt.QUERY_T_HI)
        self.query = query


def dev_trace(g, rays, query):
    dv = Dev(rays, query)
    dv.launch(g)
    g.sync()
    return dv.result()


def check_both(g, rays, rec, occ, what):
    import bihrt
    assert_hits(dev_trace(g, rays, bihrt.QUERY_CLOSEST_WITHIN), rec, what)
    got = dev_trace(g, rays, bihrt.QUERY_OCCLUDED_WITHIN)
    bad = np.flatnonzero(got != occ)
    assert bad.size == 0, f"{what}: occluded differs at {bad[:8]} ({bad.size} rays)"


@pytest.fixture(scope="module", autouse=True)
def _free_trees():
    yield
    while tt._trees:
        tt._trees.popitem()[1].close()


# --- CPU ------------------------------------------------------------------------

def test_struct_and_constants(bihrt_mod):
    R = bihrt_mod.Ray
    assert C.sizeof(R) == 32 and R.t_hi.offset == 28 and R.reserved.offset == 28 and R.d.offset == 16
    dt = bihrt_mod.RAY_DTYPE
    assert dt.itemsize == 32 and dt.fields["t_hi"][1] == 28 and dt.fields["reserved"][1] == 28
    assert dt.fields["t_lo"][1] == 12 and dt.fields["d"][1] == 16
    assert (bihrt_mod.QUERY_T_HI, bihrt_mod.QUERY_CLOSEST_WITHIN, bihrt_mod.QUERY_OCCLUDED_WITHIN) == (0x10, 0x10, 0x11)
    r = R()
    r.t_hi = 2.5
    assert r.reserved == 2.5
    import os
    hdr = open(os.path.join(tt.ROOT, "include", "bih.h")).read()
    assert "#define BIH_QUERY_T_HI      0x10u" in hdr and "#define BIH_ABI_VERSION 4" in hdr
    assert "bih_trace" in bihrt_mod._lib.exported_symbols_from_header()


def test_device_free_error_codes(bihrt_mod):
    """The two codes pass the argument checks; everything else stays invalid.
    A stand-in tree pointer is never dereferenced on these paths."""
    L = bihrt_mod._lib.load()
    INVALID, TOO_LARGE = -1, -6
    buf = (C.c_char * 96)()
    base = (C.addressof(buf) + 15) & ~15
    p, fake, odd = C.c_void_p(base), C.c_void_p(base), C.c_void_p(base + 4)
    for call in (lambda *a: L.bih_trace_device(*a, None), L.bih_trace):
        for q in (0x10, 0x11):
            assert call(fake, None, 0, q, None) == 0             # accepted; nothing to do
            assert call(fake, p, 0, q, p) == 0
            assert call(None, p, 1, q, p) == INVALID
            assert call(fake, None, 1, q, p) == INVALID
            assert call(fake, p, 1, q, None) == INVALID
            assert call(fake, p, (1 << 30) + 1, q, p) == TOO_LARGE
        for q in (0x12, 0x20, 3, 2, 7, 0x13, 0x30, 0x110, 0xFFFFFFFF):
            assert call(fake, p, 0, q, p) == INVALID, hex(q)
            assert call(fake, p, 1 << 40, q, p) == INVALID, hex(q)   # (before TOO_LARGE)
    # the device entry moves hit records as 16-byte words
    assert L.bih_trace_device(fake, p, 1, 0x10, odd, None) == INVALID
    assert L.bih_trace_device(fake, odd, 1, 0x11, p, None) == INVALID


def test_pack_rays_t_hi(bihrt_mod):
    o = np.arange(15, dtype=F32).reshape(5, 3)
    d = -o
    plain = bihrt_mod.pack_rays(o, d, 0.25)
    assert not bits(plain["t_hi"]).any() and not bits(plain["reserved"]).any()
    assert not plain.view(np.uint32).reshape(5, 8)[:, 7].any()
    one = bihrt_mod.pack_rays(o, d, 0.25, 3.5)
    assert (one.view(F32).reshape(5, 8)[:, 7] == 3.5).all() and (one["reserved"] == 3.5).all()
    th = np.array([1, 2, np.inf, np.nan, -0.0], F32)
    many = bihrt_mod.pack_rays(o, d, np.arange(5, dtype=F32), th)
    raw = many.view(F32).reshape(5, 8)
    assert np.array_equal(bits(raw[:, 7]), bits(th)) and np.array_equal(raw[:, 3], np.arange(5, dtype=F32))
    assert np.array_equal(raw[:, 0:3], o) and np.array_equal(raw[:, 4:7], d)
    assert many.tobytes() == np.ascontiguousarray(many).view(np.uint8).tobytes() and many.nbytes == 160


def test_filter_rule():
    """The checker's own rule on hand-made records: strict, NaN-safe."""
    import bihrt
    exp = np.zeros(6, bihrt.HIT_DTYPE)
    exp["t"], exp["prim"] = [1, 1, 1, 1, FLT_MAX, 1], [3, 3, 3, 3, bihrt.NO_HIT, 3]
    rec, occ = within(exp, np.array([0.5, 1.0, np.nextafter(F32(1), F32(2)), np.inf, np.inf, np.nan], F32))
    assert occ.tolist() == [0, 0, 1, 1, 0, 0]
    assert rec["prim"].tolist() == [bihrt.NO_HIT] * 2 + [3, 3] + [bihrt.NO_HIT] * 2 and rec["t"][0] == FLT_MAX


# --- GPU ------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["soup20k", "cornell", "dup_all"])
def test_four_cases(name, gpu, bihrt_mod):
    """t_hi at 0.5 t, t (strict: no hit), the next float above t (hit) and 2 t,
    with t_lo cycling {0, 1e-4, 0.25}; dup_all is one leaf (the walk's prologue
    answers).  n around the wave size too."""
    rays, exp, rec, occ = segment_set(name)
    balanced(exp)
    g = tt.tree(name)
    check_both(g, rays, rec, occ, name)
    for n in (1, 63, 65):
        check_both(g, rays[:n], rec[:n], occ[:n], f"{name} n={n}")


@pytest.mark.gpu
def test_unbounded_equals_plain_queries(gpu, bihrt_mod):
    """t_hi = FLT_MAX and +inf: byte for byte QUERY_OCCLUDED / QUERY_CLOSEST."""
    rays0, exp = ray_set("soup20k", "mixed")
    g = tt.tree("soup20k")
    plain = tt.dev_trace(g, rays0, bihrt_mod.QUERY_CLOSEST)
    plain_occ = tt.dev_trace(g, rays0, bihrt_mod.QUERY_OCCLUDED)
    assert_hits(plain, exp, "closest")
    for far in (FLT_MAX, F32(np.inf)):
        rays = bihrt_mod.pack_rays(rays0["o"], rays0["d"], rays0["t_lo"], far)
        got = dev_trace(g, rays, bihrt_mod.QUERY_CLOSEST_WITHIN)
        assert got.tobytes() == plain.tobytes(), far
        assert np.array_equal(dev_trace(g, rays, bihrt_mod.QUERY_OCCLUDED_WITHIN), plain_occ), far


@pytest.mark.gpu
def test_nan_and_empty_segments(gpu, bihrt_mod):
    """NaN t_hi and t_hi <= t_lo (equal, below, zero, negative, -inf): 0 and
    the miss record for every ray."""
    rays0, exp = ray_set("soup20k", "mixed")
    balanced(exp)
    g = tt.tree("soup20k")
    tlo = rays0["t_lo"]
    for what, t_hi in (("nan", np.full(tlo.shape, np.nan, F32)), ("t_lo", tlo), ("0", np.zeros_like(tlo)),
                       ("-1", np.full(tlo.shape, -1, F32)), ("-inf", np.full(tlo.shape, -np.inf, F32)),
                       ("below t_lo", np.nextafter(tlo, F32(-np.inf)))):
        rays = bihrt_mod.pack_rays(rays0["o"], rays0["d"], tlo, t_hi)
        rec, occ = within(exp, t_hi)
        assert not occ.any(), what                     # (the rule itself says so: t > t_lo >= t_hi)
        got = dev_trace(g, rays, bihrt_mod.QUERY_CLOSEST_WITHIN)
        assert_hits(got, rec, what)
        assert (got["t"] == FLT_MAX).all() and not bits(got["u"]).any() and not bits(got["v"]).any(), what
        assert not dev_trace(g, rays, bihrt_mod.QUERY_OCCLUDED_WITHIN).any(), what


@pytest.mark.gpu
def test_old_queries_do_not_read_the_field(gpu, bihrt_mod):
    """Garbage in the last float leaves QUERY_CLOSEST and QUERY_OCCLUDED unchanged."""
    rays0, exp = ray_set("soup20k", "mixed")
    g = tt.tree("soup20k")
    junk = np.resize(np.array([np.nan, -1.0, 0.0, 1e-30, np.inf, -np.inf, 3.0], F32), rays0.shape[0])
    rays = bihrt_mod.pack_rays(rays0["o"], rays0["d"], rays0["t_lo"], junk)
    assert_hits(tt.dev_trace(g, rays, bihrt_mod.QUERY_CLOSEST), exp, "closest, junk t_hi")
    occ = tt.dev_trace(g, rays, bihrt_mod.QUERY_OCCLUDED)
    assert np.array_equal(occ, (exp["prim"] != bihrt_mod.NO_HIT).astype(np.uint8))


@pytest.mark.gpu
def test_stack_spill_instantiation(gpu, bihrt_mod):
    """Two stack slots on chip, the rest in memory: the same results."""
    rays, exp, rec, occ = segment_set("soup20k")
    g = bihrt_mod.GPUArrayManager(scene("soup20k")[0])
    g.set_param(bihrt_mod.PARAM_TRACE_LDS_SLOTS, 2)
    check_both(g, rays, rec, occ, "2 slots")
    g.set_param(bihrt_mod.PARAM_TRACE_LDS_SLOTS, 0)
    check_both(g, rays, rec, occ, "default again")
    g.close()


@pytest.mark.gpu
def test_non_finite_rays(gpu, bihrt_mod):
    """test_trace.odd_rays (zero, NaN, Inf and 1e38 directions and origins)
    with finite t_hi: the oracle-derived rule."""
    tris, ot = scene("soup3k1")
    o, d = tt.gen(tris, ot, 512, 15)
    odd = tt.odd_rays(o, d)
    exp = expected("soup3k1", o, d, 0.0)
    balanced(exp)
    t_hi, _ = case_t_hi(exp)
    t_hi[odd] = np.resize(np.array([1.0, 1e30, 0.5], F32), odd.size)
    rec, occ = within(exp, t_hi)
    assert occ.any() and not occ[odd].any()
    check_both(tt.tree("soup3k1"), bihrt_mod.pack_rays(o, d, 0.0, t_hi), rec, occ, "non-finite")


@pytest.mark.gpu
def test_host_entry_and_allocations(gpu, bihrt_mod):
    """bih_trace equals bih_trace_device; after the first trace of a tree a
    second one, of either new query, allocates nothing."""
    rays, exp, rec, occ = segment_set("soup20k")
    g = bihrt_mod.GPUArrayManager(scene("soup20k")[0])
    got = g.trace(rays["o"], rays["d"], rays["t_lo"], bihrt_mod.QUERY_CLOSEST_WITHIN, t_hi=rays["t_hi"])
    assert sorted(got) == ["prim", "t", "u", "v"]
    for f in ("t", "u", "v", "prim"):
        assert np.array_equal(bits(got[f]), bits(rec[f])), f
    first = g.info()
    hocc = g.trace(rays["o"], rays["d"], rays["t_lo"], bihrt_mod.QUERY_OCCLUDED_WITHIN, t_hi=rays["t_hi"])
    assert hocc.dtype == np.uint8 and np.array_equal(hocc, occ)
    one = g.trace(rays["o"][:64], rays["d"][:64], rays["t_lo"][:64], bihrt_mod.QUERY_OCCLUDED_WITHIN, t_hi=np.inf)
    assert np.array_equal(one, (exp["prim"][:64] != bihrt_mod.NO_HIT).astype(np.uint8))
    check_both(g, rays, rec, occ, "device entry")
    after = g.info()
    assert after.device_allocs == first.device_allocs and after.device_bytes == first.device_bytes
    g.close()
