"""Ray queries (bih_trace / bih_trace_device): closest
hit and occlusion for caller-supplied rays, against the oracle's
traverse_closest (OracleTree.closest) and its any-hit flag (OracleTree.trace).

The expected hit record of a ray is built from the oracle alone: t and the
sorted position from OracleTree.closest, prim = tri_idx[position], and u, v
from this file's numpy f32 restatement of the reference's triangle test
(`restate`), which a CPU test pins against ob_mt bit for bit.  Each (scene,
ray set) is answered by the oracle once and shared by the tests that use it.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, edge_scenes

F32 = np.float32
FLT_MAX = np.finfo(F32).max
SRC = os.path.join(ROOT, "tests", "c", "trace_smoke.c")
LIBDIR = os.path.join(ROOT, "bih-gpu-raytracer_amd", "lib")


def gen(tris, ot, n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = ot.scene_lo.astype(np.float64), ot.scene_hi.astype(np.float64)
    o = rng.uniform(lo - 1.0, hi + 1.0, (n, 3)).astype(F32)
    tgt = rng.uniform(lo, hi, (n, 3))
    k = rng.integers(0, tris.shape[0], n)
    a = rng.uniform(0, 1, (n, 2)); s = np.sqrt(a[:, 0])
    T = tris[k].astype(np.float64)
    pt = (1 - s)[:, None] * T[:, 0:3] + (s * (1 - a[:, 1]))[:, None] * T[:, 3:6] + (s * a[:, 1])[:, None] * T[:, 6:9]
    tgt[1::2] = pt[1::2]                       # every other ray aims at a triangle
    d = (tgt.astype(F32) - o).astype(F32)
    d[::16, 0] = 0.0; d[8::16, 1] = -0.0; d[4::32, 1:] = 0.0   # axis-parallel, signed zero
    return o, d


def restate(tri, o, d):
    """RayTriangleIntersection's t, u, v (CUDAKernels.cu:17-50) for triangles
    tri (n, 9) and rays o, d (n, 3), every operation a separately rounded f32
    one in the oracle's order: dot = (x + y) + z, inv = 1.0f / det."""
    tri, o, d = (np.ascontiguousarray(x, F32) for x in (tri, o, d))

    def dot(a, b):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]

    def cross(x, y):
        return np.stack([x[:, 1] * y[:, 2] - y[:, 1] * x[:, 2],
                         x[:, 2] * y[:, 0] - y[:, 2] * x[:, 0],
                         x[:, 0] * y[:, 1] - y[:, 0] * x[:, 1]], 1)

    with np.errstate(all="ignore"):
        v0 = tri[:, 0:3]
        e1, e2 = tri[:, 3:6] - v0, tri[:, 6:9] - v0
        p = cross(d, e2)
        inv = F32(1.0) / dot(e1, p)
        s = o - v0
        u = dot(s, p) * inv
        q = cross(s, e1)
        v = dot(d, q) * inv
        t = dot(e2, q) * inv
    assert t.dtype == F32 and u.dtype == F32 and v.dtype == F32
    return t, u, v


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(tris, OracleTree) of an edge scene, or of the soups the tests use."""
    import bihrt
    import oracle
    if name == "soup20k":
        tris = bihrt.scenes.soup(20000, seed=2)
    elif name.startswith("soup3k"):
        tris = bihrt.scenes.soup(3000, seed=int(name[6:] or 1))
    else:
        tris = edge_scenes()[name]
    tris = np.ascontiguousarray(tris, F32).reshape(-1, 9)
    return tris, oracle.OracleTree(tris)


def expected(name, o, d, tlo):
    """The oracle's hit records (HIT_DTYPE) of rays (o, d, tlo) in scene `name`."""
    return expected_of(*scene(name), o, d, tlo)


def expected_of(tris, ot, o, d, tlo):
    """The same for the soup `tris` and its OracleTree `ot`."""
    import bihrt
    n = o.shape[0]
    tlo = np.broadcast_to(np.asarray(tlo, F32), (n,))
    t = np.empty(n, F32)
    idx = np.empty(n, np.int64)
    for k in range(n):
        t[k], idx[k] = ot.closest(o[k], d[k], float(tlo[k]))
    hit = idx >= 0
    exp = np.zeros(n, bihrt.HIT_DTYPE)
    exp["t"] = t
    exp["prim"] = bihrt.NO_HIT
    assert (t[~hit] == FLT_MAX).all()
    if hit.any():
        prim = ot.tri_idx[idx[hit]]
        rt, ru, rv = restate(tris[prim], o[hit], d[hit])
        assert np.array_equal(bits(rt), bits(t[hit])), "the restated t is not the oracle's"
        exp["u"][hit], exp["v"][hit], exp["prim"][hit] = ru, rv, prim
    return exp


def balanced(exp):
    """A ray set that degenerates must fail, not pass vacuously."""
    import bihrt
    share = float((exp["prim"] != bihrt.NO_HIT).mean())
    assert 0.10 <= share <= 0.90, f"hit share {share:.3f}"


@functools.lru_cache(maxsize=None)
def ray_set(name, kind):
    """(rays as RAY_DTYPE, expected HIT_DTYPE) -- computed once per process.
    edge:   2048 rays of gen(seed=11), t_lo = 0
    mixed:  4096 + 37 rays of gen(seed=12), t_lo cycling {0, 1e-4, 0.25}
    bounce: rays leaving the hit points of `mixed` in random directions, t_lo = 1e-4
    two:    1024 rays of gen(seed=14), t_lo = 0 (second stream / rebuilt soup)"""
    import bihrt
    tris, ot = scene(name)
    if kind == "edge":
        o, d = gen(tris, ot, 2048, 11)
        tlo = np.zeros(2048, F32)
    elif kind == "mixed":
        o, d = gen(tris, ot, 4096 + 37, 12)
        tlo = np.resize(np.array([0.0, 1e-4, 0.25], F32), o.shape[0])
    elif kind == "two":
        o, d = gen(tris, ot, 1024, 14)
        tlo = np.zeros(1024, F32)
    else:
        r0, e0 = ray_set(name, "mixed")
        hit = e0["prim"] != bihrt.NO_HIT
        o = (r0["o"][hit] + e0["t"][hit][:, None] * r0["d"][hit]).astype(F32)
        d = np.random.default_rng(13).uniform(-1.0, 1.0, o.shape).astype(F32)
        tlo = np.full(o.shape[0], 1e-4, F32)
    rays = bihrt.pack_rays(o, d, tlo)
    exp = expected(name, o, d, tlo)
    rays.setflags(write=False)
    exp.setflags(write=False)
    return rays, exp


def assert_hits(got, exp, what=""):
    for f in ("t", "u", "v"):
        bad = np.flatnonzero(bits(got[f]) != bits(exp[f]))
        assert bad.size == 0, f"{what}: {f} differs at {bad[:8]} ({bad.size} rays)"
    bad = np.flatnonzero(got["prim"] != exp["prim"])
    assert bad.size == 0, f"{what}: prim differs at {bad[:8]} ({bad.size} rays)"


class Dev:
    """Device copies of a ray array and its result buffer (torch tensors)."""

    def __init__(self, rays, query):
        import bihrt
        import torch
        self.n, self.query = rays.shape[0], query
        self.closest = query == bihrt.QUERY_CLOSEST
        self.rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).cuda()
        self.out = torch.full((self.n * (16 if self.closest else 1),), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def launch(self, g, stream=None):
        g.trace_device(self.rays.data_ptr(), self.n, self.out.data_ptr(), self.query, stream)

    def result(self):
        import bihrt
        a = self.out.cpu().numpy()
        return a.view(bihrt.HIT_DTYPE) if self.closest else a


def dev_trace(g, rays, query):
    dv = Dev(rays, query)
    dv.launch(g)
    g.sync()
    return dv.result()


_trees = {}


def tree(name):
    """The scene's GPU tree, shared by the tests of this module."""
    import bihrt
    if name not in _trees:
        _trees[name] = bihrt.GPUArrayManager(scene(name)[0])
    return _trees[name]


@pytest.fixture(scope="module", autouse=True)
def _free_trees():
    yield
    while _trees:
        _trees.popitem()[1].close()


# --- CPU ------------------------------------------------------------------------

def test_struct_sizes(bihrt_mod):
    assert C.sizeof(bihrt_mod.Ray) == 32 and C.sizeof(bihrt_mod.Hit) == 16
    assert bihrt_mod.RAY_DTYPE.itemsize == 32 and bihrt_mod.HIT_DTYPE.itemsize == 16
    assert bihrt_mod.Ray.t_lo.offset == 12 and bihrt_mod.Ray.d.offset == 16 and bihrt_mod.Hit.prim.offset == 12
    assert (bihrt_mod.QUERY_CLOSEST, bihrt_mod.QUERY_OCCLUDED, bihrt_mod.NO_HIT) == (0, 1, 0xFFFFFFFF)
    assert bihrt_mod.PARAM_TRACE_LDS_SLOTS == 8


def test_device_free_error_codes(bihrt_mod):
    """The argument checks come before the tree or a device is touched: a
    stand-in tree pointer is never dereferenced on these paths."""
    L = bihrt_mod._lib.load()
    INVALID, TOO_LARGE = -1, -6
    buf = (C.c_char * 64)()
    p = C.c_void_p(C.addressof(buf))
    fake = C.c_void_p(C.addressof(buf))
    for call in (lambda *a: L.bih_trace_device(*a, None), L.bih_trace):
        assert call(None, p, 1, 0, p) == INVALID                 # NULL tree, checked first
        assert call(None, None, 0, 7, None) == INVALID
        assert call(fake, None, 1, 0, p) == INVALID              # rays missing
        assert call(fake, p, 1, 1, None) == INVALID              # out missing
        assert call(fake, p, 1, 2, p) == INVALID                 # unknown query
        assert call(fake, p, (1 << 30) + 1, 0, p) == TOO_LARGE
        assert call(fake, p, 1 << 40, 1, p) == TOO_LARGE
        assert call(fake, None, 0, 0, None) == 0                 # nothing to do
        assert call(fake, p, 0, 1, p) == 0


def test_restatement_reproduces_ob_mt(oracle_mod, bihrt_mod):
    """The checker's own u, v arithmetic: its t equals ob_mt's bit for bit on
    the hit triangles of one ray set (so its u, v are the same expressions'
    values, which the oracle does not return)."""
    tris, ot = scene("soup3k1")
    o, d = gen(tris, ot, 1024, 21)
    hits = 0
    for k in range(o.shape[0]):
        t, i = ot.closest(o[k], d[k], 0.0)
        if i < 0:
            continue
        tri = tris[ot.tri_idx[i]]
        ok, tm = oracle_mod.mt(tri, o[k], d[k])
        rt, ru, rv = restate(tri[None], o[k][None], d[k][None])
        assert ok and bits(F32(tm)) == bits(F32(t)) == bits(rt)[0]
        assert 0.0 <= ru[0] <= 1.0 and 0.0 <= rv[0] and ru[0] + rv[0] <= 1.0
        hits += 1
    assert 0.10 * o.shape[0] <= hits <= 0.90 * o.shape[0]


def _build_c(tmp_path) -> str:
    exe = str(tmp_path / "trace_smoke")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic",
                    "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                    "-L", LIBDIR, "-lbih_amd", "-Wl,-rpath," + LIBDIR,
                    "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    return exe


def test_c_caller_error_paths(tmp_path, bihrt_mod):
    bihrt_mod._lib.load()
    exe = _build_c(tmp_path)
    r = subprocess.run([exe, "--errors"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and r.stdout.count("ok ") >= 7, r.stdout


# --- GPU ------------------------------------------------------------------------

EDGE = ["one_tri", "two_tris", "dup_all", "clustered", "flat_z", "signed_zero", "cornell", "dodeca",
        "bih1_dodeca"]


def test_edge_list_is_complete():
    assert sorted(EDGE) == sorted(edge_scenes())


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE)
def test_closest_edge_scenes(name, gpu, bihrt_mod):
    """1, 3: t bits, prim, u and v bits, the exact miss record; the occlusion flag
    is (closest prim != NO_HIT) and the oracle's any-hit flag (t_lo = 0)."""
    import oracle
    rays, exp = ray_set(name, "edge")
    balanced(exp)
    g = tree(name)
    got = dev_trace(g, rays, bihrt_mod.QUERY_CLOSEST)
    assert_hits(got, exp, name)
    miss = got[exp["prim"] == bihrt_mod.NO_HIT]
    assert (miss["t"] == FLT_MAX).all() and not bits(miss["u"]).any() and not bits(miss["v"]).any()
    occ = dev_trace(g, rays, bihrt_mod.QUERY_OCCLUDED)
    assert np.array_equal(occ, (got["prim"] != bihrt_mod.NO_HIT).astype(np.uint8))
    any_hit = scene(name)[1].trace(rays["o"], rays["d"], mode=oracle.MODE_GPU_ANYHIT)[0]
    assert np.array_equal(occ, any_hit)


@pytest.mark.gpu
def test_closest_mixed_t_lo(gpu, bihrt_mod):
    """2, 3: per-ray t_lo in {0, 1e-4, 0.25}, and rays that start on a surface
    (t_lo = 1e-4), where the interval clamp decides the answer."""
    g = tree("soup20k")
    for kind in ("mixed", "bounce"):
        rays, exp = ray_set("soup20k", kind)
        balanced(exp)
        got = dev_trace(g, rays, bihrt_mod.QUERY_CLOSEST)
        assert_hits(got, exp, kind)
        occ = dev_trace(g, rays, bihrt_mod.QUERY_OCCLUDED)
        assert np.array_equal(occ, (exp["prim"] != bihrt_mod.NO_HIT).astype(np.uint8)), kind
    # the surface rays really depend on t_lo: many answer differently at t_lo = 0
    rays, exp = ray_set("soup20k", "bounce")
    k = 512
    at0 = expected("soup20k", rays["o"][:k], rays["d"][:k], 0.0)
    differ = float((at0["prim"] != exp["prim"][:k]).mean())
    assert differ >= 0.05, differ


@pytest.mark.gpu
def test_counts_and_refill(gpu, bihrt_mod):
    """4: n around the wave size, then a batch larger than the persistent grid's
    lane count (CUs x 32 blocks x 64 lanes, bih_trace.hip), so that lanes
    refill: the oracle-checked batch tiled must give its results tiled."""
    import torch
    g = tree("soup20k")
    rays, exp = ray_set("soup20k", "mixed")
    assert rays.shape[0] == 4133
    for n in (0, 1, 63, 64, 65, 4133):
        assert_hits(dev_trace(g, rays[:n], bihrt_mod.QUERY_CLOSEST), exp[:n], f"n={n}")
        occ = dev_trace(g, rays[:n], bihrt_mod.QUERY_OCCLUDED)
        assert np.array_equal(occ, (exp["prim"][:n] != bihrt_mod.NO_HIT).astype(np.uint8)), n
    lanes = torch.cuda.get_device_properties(0).multi_processor_count * 32 * 64
    reps = lanes // 4133 + 2
    big = np.tile(rays, reps)
    assert big.shape[0] > lanes + 4133
    got = dev_trace(g, big, bihrt_mod.QUERY_CLOSEST)
    assert_hits(got, np.tile(exp, reps), "tiled")
    occ = dev_trace(g, big, bihrt_mod.QUERY_OCCLUDED)
    assert np.array_equal(occ, np.tile((exp["prim"] != bihrt_mod.NO_HIT).astype(np.uint8), reps))


def stack_depth(ot, o, d):
    """Entries the walk of a ray that hits nothing has on its stack at most
    (TraverseTree's decisions from the oracle's arrays, f32; with no hit there
    is no culling, so the closest walk is the reference walk)."""
    with np.errstate(all="ignore"):
        inv = F32(1.0) / d
        sg = inv < 0
        box = (ot.scene_lo, ot.scene_hi)
        tmin, tmax = F32(-np.inf), F32(np.inf)
        for ax in range(3):
            t0 = (box[int(sg[ax])][ax] - o[ax]) * inv[ax]
            t1 = (box[1 - int(sg[ax])][ax] - o[ax]) * inv[ax]
            if ax and (tmin > t1 or t0 > tmax):
                return 0
            tmin, tmax = (t0, t1) if ax == 0 else (max(tmin, t0), min(tmax, t1))
        stack, cur, deepest = [], 0, 0
        while ot.U > 1:
            ax = ot.axis[cur]
            nr = int(sg[ax])
            t = [(ot.clip[cur][k] - o[ax]) * inv[ax] for k in (0, 1)]
            A, B = tmin < t[nr], tmax < t[1 - nr]
            (cn, cf), (ln, lf) = ot.children[cur][[nr, 1 - nr]], ot.is_leaf[cur][[nr, 1 - nr]]
            pop = False
            if B and (not A or ln):
                pop = True
            elif A and B:
                cur, tmax = cn, t[nr]
            elif not A:
                pop = bool(lf)
                if not pop:
                    cur, tmin = cf, t[1 - nr]
            elif ln and lf:
                pop = True
            elif lf:
                cur, tmax = cn, t[nr]
            elif ln:
                cur, tmin = cf, t[1 - nr]
            else:
                stack.append((cf, t[1 - nr], tmax))
                deepest = max(deepest, len(stack))
                cur, tmax = cn, t[nr]
            if pop:
                if not stack:
                    break
                cur, tmin, tmax = stack.pop()
    return deepest


@pytest.mark.gpu
def test_stack_spill_instantiation(gpu, bihrt_mod):
    """5: two stack slots on chip, the rest in memory: the same results."""
    rays, exp = ray_set("soup20k", "mixed")
    balanced(exp)
    # the set does reach the memory part: most missing rays stack 3 entries or more
    miss = np.flatnonzero((exp["prim"] == bihrt_mod.NO_HIT) & (rays["t_lo"] == 0))[:200]
    depth = np.array([stack_depth(scene("soup20k")[1], rays["o"][k], rays["d"][k]) for k in miss])
    assert miss.size == 200 and (depth >= 3).sum() >= 100, np.bincount(depth)
    g = bihrt_mod.GPUArrayManager(scene("soup20k")[0])
    base = dev_trace(g, rays, bihrt_mod.QUERY_CLOSEST)
    base_occ = dev_trace(g, rays, bihrt_mod.QUERY_OCCLUDED)
    g.set_param(bihrt_mod.PARAM_TRACE_LDS_SLOTS, 2)
    got = dev_trace(g, rays, bihrt_mod.QUERY_CLOSEST)
    occ = dev_trace(g, rays, bihrt_mod.QUERY_OCCLUDED)
    assert_hits(got, exp, "2 slots")
    assert_hits(got, base, "2 slots vs default")
    assert np.array_equal(occ, base_occ)
    assert np.array_equal(occ, (exp["prim"] != bihrt_mod.NO_HIT).astype(np.uint8))
    with pytest.raises(bihrt_mod.BihError):
        g.set_param(bihrt_mod.PARAM_TRACE_LDS_SLOTS, 3)
    g.set_param(bihrt_mod.PARAM_TRACE_LDS_SLOTS, 0)
    assert_hits(dev_trace(g, rays, bihrt_mod.QUERY_CLOSEST), exp, "default again")
    g.close()


def odd_rays(o, d):
    """Zero, NaN, +-Inf and 1e38 directions, NaN and Inf origins, scattered
    among ordinary rays; returns the indices of the odd ones."""
    nan, inf = F32(np.nan), F32(np.inf)
    odd = {5: ("d", [0, 0, 0]), 21: ("d", [nan, nan, nan]), 37: ("d", [inf, inf, inf]),
           53: ("d", [-inf, -inf, -inf]), 69: ("d", [1e38, 1e38, 1e38]), 85: ("o", [nan, nan, nan]),
           101: ("o", [inf, inf, inf]), 117: ("o", [-inf, 0.5, 0.5]), 133: ("d", [-0.0, 0.0, -0.0]),
           149: ("d", [-1e38, 1e38, -1e38])}
    for k, (what, val) in odd.items():
        (o if what == "o" else d)[k] = np.array(val, F32)
    return np.array(sorted(odd))


@pytest.mark.gpu
def test_non_finite_rays(gpu, bihrt_mod):
    """6: legal input; every ray equals the oracle, and the odd ones miss."""
    tris, ot = scene("soup3k1")
    o, d = gen(tris, ot, 512, 15)
    odd = odd_rays(o, d)
    exp = expected("soup3k1", o, d, 0.0)
    balanced(exp)
    assert (exp["prim"][odd] == bihrt_mod.NO_HIT).all()
    rays = bihrt_mod.pack_rays(o, d, 0.0)
    g = tree("soup3k1")
    assert_hits(dev_trace(g, rays, bihrt_mod.QUERY_CLOSEST), exp, "non-finite")
    occ = dev_trace(g, rays, bihrt_mod.QUERY_OCCLUDED)
    assert np.array_equal(occ, (exp["prim"] != bihrt_mod.NO_HIT).astype(np.uint8))


@pytest.mark.gpu
def test_empty_scene(gpu, bihrt_mod):
    """A tree of no triangles (U = 0): every ray gets the miss record."""
    g = bihrt_mod.GPUArrayManager(np.zeros((0, 9), F32))
    rays, _ = ray_set("cornell", "edge")
    got = dev_trace(g, rays[:130], bihrt_mod.QUERY_CLOSEST)
    assert (got["t"] == FLT_MAX).all() and (got["prim"] == bihrt_mod.NO_HIT).all()
    assert not bits(got["u"]).any() and not bits(got["v"]).any()
    assert not dev_trace(g, rays[:130], bihrt_mod.QUERY_OCCLUDED).any()
    g.close()


@pytest.mark.gpu
def test_rebuild_ordering(gpu, bihrt_mod):
    """7: a trace on a second stream after rebuild() sees the new soup's tree."""
    import torch
    old, new = scene("soup3k1")[0], scene("soup3k2")[0]
    soup = torch.from_numpy(old.copy()).cuda()
    torch.cuda.synchronize()
    g = bihrt_mod.GPUArrayManager.from_device(soup.data_ptr(), old.shape[0])
    rays0, exp0 = ray_set("soup3k1", "two")
    rays1, exp1 = ray_set("soup3k2", "two")
    balanced(exp0)
    balanced(exp1)
    d0, d1 = Dev(rays0, bihrt_mod.QUERY_CLOSEST), Dev(rays1, bihrt_mod.QUERY_CLOSEST)
    d0.launch(g)
    g.sync()                      # (the caller's duty: the soup is not rewritten under a build or trace)
    soup.copy_(torch.from_numpy(new))
    torch.cuda.synchronize()
    g.rebuild()
    s2 = torch.cuda.Stream()
    d1.launch(g, s2.cuda_stream)
    s2.synchronize()
    assert_hits(d0.result(), exp0, "before the rebuild")
    assert_hits(d1.result(), exp1, "after the rebuild")
    g.close()


@pytest.mark.gpu
def test_two_streams(gpu, bihrt_mod):
    """8: two traces of one tree issued back to back on two streams."""
    import torch
    g = tree("soup20k")
    ra, ea = ray_set("soup20k", "mixed")
    rb, eb = ray_set("soup20k", "bounce")
    da, db = Dev(ra, bihrt_mod.QUERY_CLOSEST), Dev(rb, bihrt_mod.QUERY_CLOSEST)
    oa = Dev(ra, bihrt_mod.QUERY_OCCLUDED)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    da.launch(g, sa.cuda_stream)
    db.launch(g, sb.cuda_stream)
    oa.launch(g, sa.cuda_stream)
    sa.synchronize()
    sb.synchronize()
    assert_hits(da.result(), ea, "stream a")
    assert_hits(db.result(), eb, "stream b")
    assert np.array_equal(oa.result(), (ea["prim"] != bihrt_mod.NO_HIT).astype(np.uint8))


@pytest.mark.gpu
def test_renders_undisturbed(gpu, bihrt_mod):
    """9: a trace between two frames moves no pixel and no RNG state."""
    tris, ot = scene("cornell")
    g = bihrt_mod.GPUArrayManager(tris)
    r = bihrt_mod.Renderer(g, 64, 64)
    rays, exp = ray_set("cornell", "edge")
    f0 = r.render(0)
    got = dev_trace(g, rays, bihrt_mod.QUERY_CLOSEST)
    f1 = r.render(1)
    assert_hits(got, exp, "between frames")
    assert np.array_equal(f0, ot.render(64, 64, frame=0)[0])
    assert np.array_equal(f1, ot.render(64, 64, frame=1)[0])
    g.close()


@pytest.mark.gpu
def test_host_entry(gpu, bihrt_mod):
    """10: bih_trace (numpy in, numpy out) equals bih_trace_device."""
    g = tree("soup20k")
    rays, exp = ray_set("soup20k", "mixed")
    got = g.trace(rays["o"], rays["d"], rays["t_lo"])
    dev = dev_trace(g, rays, bihrt_mod.QUERY_CLOSEST)
    assert sorted(got) == ["prim", "t", "u", "v"] and got["prim"].dtype == np.uint32
    for f in ("t", "u", "v", "prim"):
        assert np.array_equal(np.ascontiguousarray(got[f]).view(np.uint32),
                              np.ascontiguousarray(dev[f]).view(np.uint32)), f
    assert_hits(dev, exp, "device")
    occ = g.trace(rays["o"], rays["d"], rays["t_lo"], query=bihrt_mod.QUERY_OCCLUDED)
    assert occ.dtype == np.uint8
    assert np.array_equal(occ, dev_trace(g, rays, bihrt_mod.QUERY_OCCLUDED))
    # a scalar t_lo, and an empty batch
    k = 64
    one = g.trace(rays["o"][:k], rays["d"][:k], 0.25)
    assert np.array_equal(one["prim"], expected("soup20k", rays["o"][:k], rays["d"][:k], 0.25)["prim"])
    assert g.trace(np.zeros((0, 3), F32), np.zeros((0, 3), F32))["t"].shape == (0,)


@pytest.mark.gpu
def test_steady_state_allocations(gpu, bihrt_mod):
    """11: the cursor and the spill area are sized by the grid: a second trace,
    and a larger third one, allocate nothing."""
    g = bihrt_mod.GPUArrayManager(scene("soup3k1")[0])
    rays, exp = ray_set("soup3k1", "two")
    before = g.info()
    dev_trace(g, rays, bihrt_mod.QUERY_CLOSEST)
    first = g.info()
    assert first.device_allocs > before.device_allocs and first.device_bytes > before.device_bytes
    dev_trace(g, rays, bihrt_mod.QUERY_OCCLUDED)
    got = dev_trace(g, np.tile(rays, 5), bihrt_mod.QUERY_CLOSEST)
    after = g.info()
    assert after.device_allocs == first.device_allocs and after.device_bytes == first.device_bytes
    assert_hits(got, np.tile(exp, 5), "larger batch")
    g.close()


@pytest.mark.gpu
def test_c_caller_traces(tmp_path, gpu, bihrt_mod):
    """12: tests/c/trace_smoke.c -- bih_build + bih_trace from strict C11."""
    exe = _build_c(tmp_path)
    tris = scene("soup3k1")[0]
    rays, exp = ray_set("soup3k1", "two")
    balanced(exp)
    sp, rp, hp = tmp_path / "scene.f32", tmp_path / "rays.bin", tmp_path / "hits.bin"
    tris.tofile(sp)
    rays.tofile(rp)
    n = rays.shape[0]
    r = subprocess.run([exe, str(sp), str(tris.shape[0]), str(rp), str(n), str(hp)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "trace_smoke OK" in r.stdout, r.stdout + r.stderr
    raw = np.fromfile(hp, np.uint8)
    assert raw.size == n * 17
    assert_hits(raw[:n * 16].view(bihrt_mod.HIT_DTYPE), exp, "C caller")
    assert np.array_equal(raw[n * 16:], (exp["prim"] != bihrt_mod.NO_HIT).astype(np.uint8))
