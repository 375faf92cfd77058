"""G-buffer render (bih_render_gbuffer / bih_render_gbuffer_device, DESIGN.md
section 4.5.2): the closest hit of every primary sample of a frame and the
pixel planes resolved from them.

Expected values come from the oracle alone.  The rays are this file's numpy
f32 restatement of the camera formula on oracle.rng_uniforms (a CPU test pins
their hit flags against ob_render_whitted's per-sample depths); t and the
sorted position come from OracleTree.closest, prim = tri_idx[position], u and
v from a copy of tests/test_trace.py's `restate`, and the pixel planes from
numpy f32 on those.  Every comparison is on bits.  Each (scene, camera, shape,
frame) is answered by the oracle once and shared by the tests that use it.
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
SEED = 1984
SRC = os.path.join(ROOT, "tests", "c", "gbuffer_smoke.c")
LIBDIR = os.path.join(ROOT, "bih-gpu-raytracer_amd", "lib")
K1, K2 = (0.35, 0.25, -1.0), (-0.6, 0.4, 0.7)
KS = {"K1": K1, "K2": K2}
PLANES = ("depth", "prim", "bary", "normal", "coverage")
EDGE = ["one_tri", "two_tris", "dup_all", "clustered", "flat_z", "signed_zero", "cornell", "dodeca",
        "bih1_dodeca"]
SPARSE = ("clustered", "flat_z", "signed_zero")   # hit share below 10 % under both cameras: bits only
# Other test modules' scenes (name -> () -> soup) and cameras (name -> (w, h) ->
# float32[12]) for scene(), camera() and expected(): tests/test_cameras.py
EXTRA_SCENES, EXTRA_CAMERAS = {}, {}


def framing(lo, hi, w, h, k, fill=0.75):
    """A camera that frames the scene box from direction k (f64, cast to f32)."""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    c = (lo + hi) / 2; r = max(np.linalg.norm(hi - lo) / 2, 1e-3)
    k = np.asarray(k, float); k /= np.linalg.norm(k)
    o = c + 2.5 * r * k; f = (c - o) / np.linalg.norm(c - o)
    rt = np.cross([0, 1.0, 0], f); rt /= np.linalg.norm(rt); up = np.cross(f, rt)
    hh = fill / 2.5; hw = hh * w / h
    return np.concatenate([o, o + f - rt * hw - up * hh, 2 * hw * rt, 2 * hh * up]).astype(np.float32)


def restate(tri, o, d):
    """RayTriangleIntersection's t, u, v (CUDAKernels.cu:17-50), every operation
    a separately rounded f32 one in the oracle's order (tests/test_trace.py)."""
    tri, o, d = (np.ascontiguousarray(x, F32) for x in (tri, o, d))

    def dot(a, b):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]

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


def cross(x, y):
    """glm::cross, f32."""
    return np.stack([x[:, 1] * y[:, 2] - y[:, 1] * x[:, 2],
                     x[:, 2] * y[:, 0] - y[:, 2] * x[:, 0],
                     x[:, 0] * y[:, 1] - y[:, 0] * x[:, 1]], 1)


def normals(tri):
    """cross(e1, e2) / len of triangles (n, 9), each operation one f32 op."""
    tri = np.ascontiguousarray(tri, F32)
    with np.errstate(all="ignore"):
        v0 = tri[:, 0:3]
        n = cross(tri[:, 3:6] - v0, tri[:, 6:9] - v0)
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        out = n / ln[:, None]
    assert out.dtype == F32
    return out


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == F32 else x


@functools.lru_cache(maxsize=None)
def scene(name):
    """(tris, OracleTree) of an edge scene, or of the soups the tests use."""
    import bihrt
    import oracle
    if name in EXTRA_SCENES:
        tris = EXTRA_SCENES[name]()
    elif name == "soup20k":
        tris = bihrt.scenes.soup(20000, seed=2, half=0.05)
    elif name.startswith("soup3k"):
        tris = bihrt.scenes.soup(3000, seed=int(name[6:] or 1), half=0.08)
    else:
        tris = edge_scenes()[name]
    tris = np.ascontiguousarray(tris, F32).reshape(-1, 9)
    return tris, oracle.OracleTree(tris)


def camera(name, kname, w, h):
    if kname in EXTRA_CAMERAS:
        return np.ascontiguousarray(EXTRA_CAMERAS[kname](w, h), F32)
    ot = scene(name)[1]
    return framing(ot.scene_lo, ot.scene_hi, w, h, KS[kname])


@functools.lru_cache(maxsize=None)
def frame_uniforms(w, h, spp, frame, seed=SEED):
    """(h, w, 2*spp) f32: draws 2*spp*frame .. of XORWOW subsequence y*w + x; read-only."""
    import oracle
    r = np.empty((h, w, 2 * spp), F32)
    for y in range(h):
        for x in range(w):
            r[y, x] = oracle.rng_uniforms(seed, y * w + x, 2 * spp, skip=2 * spp * frame)
    r.setflags(write=False)
    return r


def frame_rays(cam, w, h, spp, frame, seed=SEED):
    """Directions (h, w, spp, 3) f32 of the frame's samples: r0, r1 = draws
    2*spp*frame + 2s (+ 1) of XORWOW subsequence y*w + x; u = (x + r0) / w,
    v = (y + r1) / h; d = ((lower_left + u*horizontal) + v*vertical) - origin."""
    r = frame_uniforms(w, h, spp, frame, seed)
    cam = np.asarray(cam, F32)
    xs = np.arange(w, dtype=F32)[None, :, None]
    ys = np.arange(h, dtype=F32)[:, None, None]
    u = (xs + r[:, :, 0::2]) / F32(w)
    v = (ys + r[:, :, 1::2]) / F32(h)
    d = np.stack([((cam[3 + a] + u * cam[6 + a]) + v * cam[9 + a]) - cam[a] for a in range(3)], -1)
    assert d.dtype == F32 and d.shape == (h, w, spp, 3)
    return d


@functools.lru_cache(maxsize=None)
def expected(name, kname, w, h, spp, frame):
    """The oracle's G-buffer of the whole frame: "hits" (h*w*spp HIT_DTYPE) and
    the pixel planes shaped as render_gbuffer's; read-only, computed once."""
    import bihrt
    tris, ot = scene(name)
    cam = camera(name, kname, w, h)
    d = frame_rays(cam, w, h, spp, frame).reshape(-1, 3)
    n = d.shape[0]
    o = np.broadcast_to(cam[0:3], (n, 3))
    t = np.empty(n, F32)
    idx = np.empty(n, np.int64)
    for k in range(n):
        t[k], idx[k] = ot.closest(cam[0:3], d[k], 0.0)
    hit = idx >= 0
    hits = np.zeros(n, bihrt.HIT_DTYPE)
    hits["t"] = t
    hits["prim"] = bihrt.NO_HIT
    assert (t[~hit] == FLT_MAX).all()
    nrm = np.zeros((n, 3), F32)
    if hit.any():
        prim = ot.tri_idx[idx[hit]]
        rt, ru, rv = restate(tris[prim], o[hit], d[hit])
        assert np.array_equal(bits(rt), bits(t[hit])), "the restated t is not the oracle's"
        hits["u"][hit], hits["v"][hit], hits["prim"][hit] = ru, rv, prim
        nrm[hit] = normals(tris[prim])
    # the representative sample: the hit sample of smallest (t bits, s)
    P = w * h
    key = np.where(hit, (bits(t).astype(np.uint64) << np.uint64(32)) | np.tile(np.arange(spp, dtype=np.uint64), P),
                   np.uint64(0xFFFFFFFFFFFFFFFF)).reshape(P, spp)
    rep = np.arange(P) * spp + key.argmin(1)       # (argmin: the first of equal keys, and those differ by s)
    cov = hit.reshape(P, spp).sum(1).astype(np.uint32)
    any_hit = cov > 0
    assert np.array_equal(any_hit, hit[rep])
    out = {"hits": hits,
           "depth": hits["t"][rep].reshape(h, w),
           "prim": hits["prim"][rep].reshape(h, w),
           "bary": np.stack([hits["u"][rep], hits["v"][rep]], 1).reshape(h, w, 2),
           "normal": nrm[rep].reshape(h, w, 3),
           "coverage": cov.reshape(h, w)}
    assert (out["depth"][~any_hit.reshape(h, w)] == FLT_MAX).all() and not bits(out["bary"])[~any_hit.reshape(h, w)].any()
    for a in out.values():
        a.setflags(write=False)
    return out


def share(exp):
    import bihrt
    return float((exp["hits"]["prim"] != bihrt.NO_HIT).mean())


def balanced(name, exp):
    """A frame that degenerates must fail, not pass vacuously."""
    s = share(exp)
    if name in SPARSE:
        assert s > 0, "no sample hits"
    else:
        assert 0.10 <= s <= 0.90, f"hit share {s:.3f}"


def rows_of(exp, w, spp, ys):
    """The expected planes of global rows ys (local row order)."""
    ys = np.asarray(ys)
    out = {k: exp[k][ys] for k in PLANES}
    out["hits"] = exp["hits"].reshape(-1, w * spp)[ys].reshape(-1)
    return out


def assert_planes(got, exp, what="", names=PLANES + ("hits",)):
    for name in names:
        g, e = got[name], exp[name]
        assert g.shape == e.shape and g.dtype == e.dtype, f"{what}: {name} {g.shape} {g.dtype}"
        if name == "hits":
            for f in ("t", "u", "v", "prim"):
                bad = np.flatnonzero(bits(g[f]) != bits(e[f]))
                assert bad.size == 0, f"{what}: hits.{f} differs at {bad[:8]} ({bad.size} samples)"
        else:
            bad = np.argwhere(bits(g) != bits(e))
            assert bad.size == 0, f"{what}: {name} differs at {bad[:4].tolist()} ({bad.shape[0]} values)"


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


def renderer(g, name, kname, w, h, spp):
    import bihrt
    return bihrt.Renderer(g, w, h, spp=spp, seed=SEED, camera=bihrt.Camera.from_list(camera(name, kname, w, h)))


class DevPlanes:
    """Device planes (torch tensors prefilled with 0xAB) of a G-buffer call."""
    SIZE = {"depth": 4, "prim": 4, "bary": 8, "normal": 12, "coverage": 4}

    def __init__(self, nrows, w, spp, names=PLANES + ("hits",)):
        import torch
        self.nrows, self.w, self.spp, self.names = nrows, w, spp, names
        P = nrows * w
        self.t = {k: torch.full((P * (16 * spp if k == "hits" else self.SIZE[k]),), 0xAB, dtype=torch.uint8,
                                device="cuda") for k in PLANES + ("hits",)}
        torch.cuda.synchronize()

    def launch(self, r, frame, rows=None, stream=None):
        r.render_gbuffer_device({k: self.t[k].data_ptr() for k in self.names}, frame, rows, stream)

    def result(self):
        """Every plane (also the ones not asked for), shaped as render_gbuffer's."""
        import bihrt
        out = {}
        for k, ten in self.t.items():
            a = ten.cpu().numpy()
            if k == "hits":
                out[k] = a.view(bihrt.HIT_DTYPE)
            else:
                dt, n = bihrt.GBUFFER_PLANES[k]
                out[k] = a.view(dt).reshape((self.nrows, self.w) + ((n,) if n > 1 else ()))
        return out


def dev_gbuffer(r, frame, rows=None, names=PLANES + ("hits",)):
    nrows = rows.nrows if rows is not None else r.h
    dv = DevPlanes(nrows, r.w, r.spp, names)
    dv.launch(r, frame, rows)
    r.sync()
    return dv.result()


# --- CPU ------------------------------------------------------------------------

def test_edge_list_is_complete():
    assert sorted(EDGE) == sorted(edge_scenes())


@pytest.mark.parametrize("name,w,h,spp", [("cornell", 48, 32, 4), ("soup3k", 48, 32, 4),
                                          ("cornell", 37, 29, 3), ("soup3k", 37, 29, 3)])
def test_ray_restatement_matches_oracle(name, w, h, spp, oracle_mod, bihrt_mod):
    """The checker's own rays: their hit flags equal ob_render_whitted's
    per-sample depths > 0 (the oracle's own primary rays of that frame)."""
    tris, ot = scene(name)
    exp = expected(name, "K1", w, h, spp, 1)
    flags = exp["hits"]["prim"] != bihrt_mod.NO_HIT
    dep = ot.render_whitted(w, h, spp=spp, frame=1, seed=SEED, cam=camera(name, "K1", w, h), depths=True)[2]
    assert np.array_equal(flags, dep > 0)
    assert 0.10 <= flags.mean() <= 0.90, flags.mean()
    # the pixel planes are consistent with the samples
    hit = exp["prim"] != bihrt_mod.NO_HIT
    assert np.array_equal(hit, exp["coverage"] > 0) and exp["coverage"].max() <= spp
    ln = np.linalg.norm(exp["normal"].astype(np.float64), axis=-1)
    assert np.allclose(ln[hit], 1.0, atol=1e-6) and not ln[~hit].any()
    partial = ((exp["coverage"] > 0) & (exp["coverage"] < spp)).mean()
    assert partial > 0.01, partial


def test_struct_layout(bihrt_mod):
    G = bihrt_mod.GBuffer
    assert C.sizeof(G) == 6 * C.sizeof(C.c_void_p)
    assert [f[0] for f in G._fields_] == ["hits", "depth", "prim", "bary", "normal", "coverage"]
    assert [getattr(G, f).offset for f, _ in G._fields_] == [k * C.sizeof(C.c_void_p) for k in range(6)]
    assert bihrt_mod.PARAM_GBUFFER_MASK == 9
    assert sorted(bihrt_mod.GBUFFER_PLANES) == sorted(PLANES)


def test_device_free_error_codes(bihrt_mod):
    """The argument checks come, in the header's order, before the tree or a
    device is touched: a stand-in tree pointer is never dereferenced."""
    L = bihrt_mod._lib.load()
    INVALID, TOO_LARGE = -1, -6
    raw = (C.c_char * 96)()
    base = (C.addressof(raw) + 15) & ~15
    fake = C.c_void_p(base)
    cam = bihrt_mod.Camera()
    G, R = bihrt_mod.GBuffer, bihrt_mod.Rows
    depth, hits, none = G(depth=base), G(hits=base), G()
    odd = G(hits=base + 4, depth=base)
    for entry in (lambda *a: L.bih_render_gbuffer_device(*a, None), L.bih_render_gbuffer):
        def call(t, c, w, h, spp, rows, g):
            return entry(t, C.byref(c) if c is not None else None, w, h, spp, 0, SEED,
                         C.byref(rows) if rows is not None else None, C.byref(g) if g is not None else None)
        assert call(None, cam, 8, 8, 4, None, depth) == INVALID           # 1: NULL tree, camera, planes
        assert call(fake, None, 8, 8, 4, None, depth) == INVALID
        assert call(fake, cam, 8, 8, 4, None, None) == INVALID
        for whs in ((0, 8, 4), (8, 0, 4), (8, 8, 0)):                     # 2
            assert call(fake, cam, *whs, None, depth) == INVALID
        assert call(fake, cam, 8, 8, 65, None, depth) == INVALID          # 3: the call's limit
        assert call(fake, cam, 1 << 16, 1 << 16, 65, None, depth) == INVALID   # (before TOO_LARGE)
        assert call(fake, cam, 8, 8, 4, None, none) == INVALID            # 4: all planes NULL
        assert call(fake, cam, 1 << 16, 1 << 16, 1, None, none) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 4, 0, 1), depth) == INVALID  # 5: rows
        assert call(fake, cam, 8, 8, 4, R(0, 4, 2, 0), depth) == INVALID
        assert call(fake, cam, 8, 8, 4, R(6, 4, 4, 1), depth) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 8, 4, 2), depth) == INVALID
        assert call(fake, cam, 1 << 16, 1 << 16, 1, R(1 << 16, 1, 1, 1), depth) == INVALID   # (before TOO_LARGE)
        assert call(fake, cam, 1 << 16, 1 << 16, 1, None, depth) == TOO_LARGE   # 6
        assert call(fake, cam, 1 << 15, 1 << 15, 4, None, odd) == TOO_LARGE     # (before the alignment)
        assert call(fake, cam, 8, 8, 4, None, odd) == INVALID             # 7: misaligned hits
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), odd) == INVALID    # (before nrows == 0)
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), hits) == 0         # 8: nothing to do
        assert call(fake, cam, 8, 8, 64, R(3, 0, 0, 0), depth) == 0


def _build_c(tmp_path) -> str:
    exe = str(tmp_path / "gbuffer_smoke")
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
    assert "FAIL" not in r.stdout and r.stdout.count("ok ") >= 11, r.stdout


# --- GPU ------------------------------------------------------------------------

def both_masks(g, run, exp, what):
    """`run()` with the bins' hit mask (the default) and with every sample walked."""
    import bihrt
    try:
        for m in (1, 0):
            g.set_param(bihrt.PARAM_GBUFFER_MASK, m)
            assert_planes(run(), exp, f"{what} mask={m}")
    finally:
        g.set_param(bihrt.PARAM_GBUFFER_MASK, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE)
def test_edge_scenes(name, gpu, bihrt_mod):
    """Every plane and `hits` of all nine edge scenes (one-leaf trees among
    them) at 48x32x4, frame 1, camera K2, with the mask and without."""
    exp = expected(name, "K2", 48, 32, 4, 1)
    balanced(name, exp)
    g = tree(name)
    r = renderer(g, name, "K2", 48, 32, 4)
    both_masks(g, lambda: dev_gbuffer(r, 1), exp, name)
    miss = exp["hits"]["prim"] == bihrt_mod.NO_HIT
    assert miss.any() and (exp["hits"]["t"][miss] == FLT_MAX).all()


@pytest.mark.gpu
def test_shapes(gpu, bihrt_mod):
    """Partial tiles, every tile shape (spp 1, 2, 4, .. 64), one pixel per wave,
    and spp that are no power of two."""
    g = tree("cornell")
    for w, h, spp in ((1, 1, 1), (37, 29, 1), (37, 29, 4), (16, 8, 16), (8, 8, 64), (37, 29, 3), (20, 12, 5),
                      (37, 29, 2), (37, 29, 8), (20, 12, 32)):
        exp = expected("cornell", "K1", w, h, spp, 1)
        if (w, h) != (1, 1):
            balanced("cornell", exp)
        r = renderer(g, "cornell", "K1", w, h, spp)
        both_masks(g, lambda: dev_gbuffer(r, 1), exp, f"{w}x{h}x{spp}")


@pytest.mark.gpu
def test_soup_depth_complexity(gpu, bihrt_mod):
    """Many triangles behind one another (about a third of the pixels are
    partially covered), frames 0 and 3; once more with two stack slots on chip,
    the rest of the stack in memory."""
    g = tree("soup20k")
    r = renderer(g, "soup20k", "K1", 96, 64, 4)
    for frame in (0, 3):
        exp = expected("soup20k", "K1", 96, 64, 4, frame)
        balanced("soup20k", exp)
        partial = ((exp["coverage"] > 0) & (exp["coverage"] < 4)).mean()
        assert partial > 0.2 and np.unique(exp["prim"]).size > 1000, (partial, np.unique(exp["prim"]).size)
        both_masks(g, lambda: dev_gbuffer(r, frame), exp, f"frame {frame}")
    g.set_param(bihrt_mod.PARAM_TRACE_LDS_SLOTS, 2)
    try:
        both_masks(g, lambda: dev_gbuffer(r, 3), expected("soup20k", "K1", 96, 64, 4, 3), "2 slots")
    finally:
        g.set_param(bihrt_mod.PARAM_TRACE_LDS_SLOTS, 0)


@pytest.mark.gpu
def test_rows_and_bands(gpu, bihrt_mod):
    """Rows {4, 8, 4, 2} (tile-aligned bands: the mask serves) and {5, 7, 7, 1}
    (not aligned) of a 48x32 frame equal the same rows of the full frame."""
    exp = expected("cornell", "K1", 48, 32, 4, 1)
    g = tree("cornell")
    r = renderer(g, "cornell", "K1", 48, 32, 4)
    for rows, ys in ((bihrt_mod.Rows(4, 8, 4, 2), [4, 5, 6, 7, 12, 13, 14, 15]),
                     (bihrt_mod.Rows(5, 7, 7, 1), list(range(5, 12)))):
        sub = rows_of(exp, 48, 4, ys)
        assert 0.10 <= (sub["hits"]["prim"] != bihrt_mod.NO_HIT).mean() <= 0.90
        both_masks(g, lambda: dev_gbuffer(r, 1, rows), sub, f"rows {ys[0]}..")
        host = r.render_gbuffer(1, rows, hits=True)
        assert_planes(host, sub, "host entry rows")


@pytest.mark.gpu
def test_plane_subsets(gpu, bihrt_mod):
    """Each plane alone, and `hits` alone, gives the bits of all planes
    together; planes that were not asked for stay untouched (0xAB)."""
    exp = expected("cornell", "K1", 48, 32, 4, 1)
    g = tree("cornell")
    r = renderer(g, "cornell", "K1", 48, 32, 4)
    for name in PLANES + ("hits",):
        got = dev_gbuffer(r, 1, names=(name,))
        assert_planes(got, exp, f"{name} alone", names=(name,))
        for other in PLANES + ("hits",):
            if other != name:
                assert (np.ascontiguousarray(got[other]).view(np.uint8) == 0xAB).all(), (name, other)


@pytest.mark.gpu
def test_grid_larger_than_persistent_grid(gpu, bihrt_mod):
    """More tiles (9216) than the persistent grid has waves (waves take two
    tiles at a time, 16 waves per CU: bih_gbuffer.hip), so that waves come back
    for more: every sample's hit flag equals the oracle's per-sample depth > 0,
    coverage their per-pixel sum, and the colour computed from coverage the
    oracle's render."""
    import torch
    w, h, spp = 512, 288, 4
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert (w // 4) * (h // 4) > cus * 32 and (w // 4) * (h // 4) // 2 > cus * 16
    tris, ot = scene("cornell")
    cam = camera("cornell", "K1", w, h)
    g = tree("cornell")
    r = renderer(g, "cornell", "K1", w, h, spp)
    got = dev_gbuffer(r, 1)
    dep = ot.render_whitted(w, h, spp=spp, frame=1, seed=SEED, cam=cam, depths=True)[2]
    flags = got["hits"]["prim"] != bihrt_mod.NO_HIT
    assert np.array_equal(flags, dep > 0) and 0.10 <= flags.mean() <= 0.90
    cov = flags.reshape(h, w, spp).sum(-1).astype(np.uint32)
    assert np.array_equal(got["coverage"], cov)
    assert np.array_equal(got["prim"] != bihrt_mod.NO_HIT, cov > 0)
    # Color (CUDAKernels.cu:384-388) summed in sample order, / spp, clamp + rgbToInt: f32
    col = np.zeros((h, w, 3), F32)
    for s in range(spp):
        f = flags.reshape(h, w, spp)[:, :, s]
        col += np.where(f[..., None], np.array([255, 255, 0], F32), np.array([20, 20, 40], F32))
    col = np.clip(col / F32(spp), F32(0), F32(255)).astype(np.int32).astype(np.uint32)
    img = (col[..., 2] << 16) | (col[..., 1] << 8) | col[..., 0]
    assert np.array_equal(img, ot.render(w, h, spp=spp, frame=1, seed=SEED, cam=cam)[0])


@pytest.mark.gpu
def test_matches_trace_device(gpu, bihrt_mod):
    """The `hits` plane equals bih_trace_device(CLOSEST) on the restated rays."""
    import torch
    w, h, spp = 48, 32, 4
    exp = expected("soup3k", "K1", w, h, spp, 1)
    balanced("soup3k", exp)
    cam = camera("soup3k", "K1", w, h)
    d = frame_rays(cam, w, h, spp, 1).reshape(-1, 3)
    rays = bihrt_mod.pack_rays(np.broadcast_to(cam[0:3], d.shape), d, 0.0)
    g = tree("soup3k")
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    d_out = torch.zeros(rays.shape[0] * 16, dtype=torch.uint8, device="cuda")
    g.trace_device(d_rays.data_ptr(), rays.shape[0], d_out.data_ptr(), bihrt_mod.QUERY_CLOSEST)
    g.sync()
    traced = d_out.cpu().numpy().view(bihrt_mod.HIT_DTYPE)
    got = dev_gbuffer(renderer(g, "soup3k", "K1", w, h, spp), 1)
    assert_planes({"hits": traced}, exp, "trace", names=("hits",))
    assert_planes(got, {"hits": traced}, "gbuffer vs trace", names=("hits",))
    assert_planes(got, exp, "gbuffer")


@pytest.mark.gpu
def test_renders_undisturbed(gpu, bihrt_mod):
    """render f=0, gbuffer f=2, render f=2, render f=3, gbuffer f=3: every
    image is the oracle's and every plane is right."""
    w, h, spp = 48, 32, 4
    tris, ot = scene("cornell")
    cam = camera("cornell", "K1", w, h)
    g = bihrt_mod.GPUArrayManager(tris)
    r = renderer(g, "cornell", "K1", w, h, spp)
    f0 = r.render(0)
    g2 = r.render_gbuffer(2, hits=True)
    f2 = r.render(2)
    f3 = r.render(3)
    g3 = r.render_gbuffer(3, hits=True)
    for f, img in ((0, f0), (2, f2), (3, f3)):
        assert np.array_equal(img, ot.render(w, h, spp=spp, frame=f, seed=SEED, cam=cam)[0]), f
    assert_planes(g2, expected("cornell", "K1", w, h, spp, 2), "frame 2")
    assert_planes(g3, expected("cornell", "K1", w, h, spp, 3), "frame 3")
    g.close()


@pytest.mark.gpu
def test_rebuild_ordering(gpu, bihrt_mod):
    """A G-buffer render on a second stream after rebuild() sees the new soup's tree."""
    import torch
    w, h, spp = 48, 32, 4
    old, new = scene("soup3k")[0], scene("soup3k2")[0]
    soup = torch.from_numpy(old.copy()).cuda()
    torch.cuda.synchronize()
    g = bihrt_mod.GPUArrayManager.from_device(soup.data_ptr(), old.shape[0])
    exp0, exp1 = expected("soup3k", "K1", w, h, spp, 1), expected("soup3k2", "K1", w, h, spp, 1)
    balanced("soup3k", exp0)
    balanced("soup3k2", exp1)
    assert not np.array_equal(exp0["prim"], exp1["prim"])
    r0, r1 = renderer(g, "soup3k", "K1", w, h, spp), renderer(g, "soup3k2", "K1", w, h, spp)
    d0, d1 = DevPlanes(h, w, spp), DevPlanes(h, w, spp)
    d0.launch(r0, 1)
    g.sync()                      # (the caller's duty: the soup is not rewritten under a build or render)
    soup.copy_(torch.from_numpy(new))
    torch.cuda.synchronize()
    g.rebuild()
    s2 = torch.cuda.Stream()
    d1.launch(r1, 1, stream=s2.cuda_stream)
    s2.synchronize()
    assert_planes(d0.result(), exp0, "before the rebuild")
    assert_planes(d1.result(), exp1, "after the rebuild")
    g.close()


@pytest.mark.gpu
def test_two_streams(gpu, bihrt_mod):
    """Two G-buffer renders of one tree issued back to back on two streams,
    and a trace behind them on the first."""
    import torch
    w, h, spp = 48, 32, 4
    g = tree("soup3k")
    r = renderer(g, "soup3k", "K1", w, h, spp)
    ea, eb = expected("soup3k", "K1", w, h, spp, 1), expected("soup3k", "K1", w, h, spp, 2)
    da, db, dc = DevPlanes(h, w, spp), DevPlanes(h, w, spp), DevPlanes(h, w, spp)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    da.launch(r, 1, stream=sa.cuda_stream)
    db.launch(r, 2, stream=sb.cuda_stream)
    dc.launch(r, 1, stream=sa.cuda_stream)
    sa.synchronize()
    sb.synchronize()
    assert_planes(da.result(), ea, "stream a")
    assert_planes(db.result(), eb, "stream b")
    assert_planes(dc.result(), ea, "stream a again")


@pytest.mark.gpu
def test_host_entry_equals_device_entry(gpu, bihrt_mod):
    exp = expected("soup3k", "K1", 48, 32, 4, 1)
    g = tree("soup3k")
    r = renderer(g, "soup3k", "K1", 48, 32, 4)
    host = r.render_gbuffer(1, hits=True)
    assert sorted(host) == sorted(PLANES + ("hits",)) and r.frame == 2
    assert_planes(host, dev_gbuffer(r, 1), "host vs device")
    assert_planes(host, exp, "host")
    only = r.render_gbuffer(1, planes=("depth", "coverage"))
    assert sorted(only) == ["coverage", "depth"]
    assert_planes(only, exp, "two planes", names=("depth", "coverage"))


@pytest.mark.gpu
def test_steady_state_allocations(gpu, bihrt_mod):
    """After the first call of a shape further calls allocate nothing, with
    the mask and without."""
    tris = scene("soup3k")[0]
    for m in (1, 0):
        g = bihrt_mod.GPUArrayManager(tris)
        g.set_param(bihrt_mod.PARAM_GBUFFER_MASK, m)
        r = renderer(g, "soup3k", "K1", 48, 32, 4)
        before = g.info()
        dev_gbuffer(r, 0)
        first = g.info()
        assert first.device_allocs > before.device_allocs and first.device_bytes > before.device_bytes
        for f in (2, 5, 1):
            got = dev_gbuffer(r, f)
        after = g.info()
        assert after.device_allocs == first.device_allocs and after.device_bytes == first.device_bytes, m
        assert_planes(got, expected("soup3k", "K1", 48, 32, 4, 1), f"mask={m}")
        g.close()


@pytest.mark.gpu
def test_c_caller(tmp_path, gpu, bihrt_mod):
    """tests/c/gbuffer_smoke.c -- bih_build + bih_render_gbuffer from strict C11
    (cornell, 64x48, the reference camera): the planes equal render_gbuffer's."""
    exe = _build_c(tmp_path)
    tris = scene("cornell")[0]
    w, h, spp = 64, 48, 4
    sp, op = tmp_path / "scene.f32", tmp_path / "planes.bin"
    tris.tofile(sp)
    r = subprocess.run([exe, str(sp), str(tris.shape[0]), str(w), str(h), str(spp), "0", str(op)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "gbuffer_smoke OK" in r.stdout, r.stdout + r.stderr
    ref = bihrt_mod.Renderer(tree("cornell"), w, h, spp=spp).render_gbuffer(0, hits=True)
    assert (ref["coverage"] > 0).any()
    raw = np.fromfile(op, np.uint8)
    P = w * h
    assert raw.size == P * (16 * spp + 4 + 4 + 8 + 12 + 4)
    off = 0
    for name, size in (("hits", 16 * spp), ("depth", 4), ("prim", 4), ("bary", 8), ("normal", 12), ("coverage", 4)):
        part = raw[off:off + P * size]
        off += P * size
        assert np.array_equal(part, np.ascontiguousarray(ref[name]).view(np.uint8).reshape(-1)), name


@pytest.mark.gpu
def test_app_writes_npz(tmp_path, gpu, bihrt_mod):
    """python -m bihrt --gbuffer: one .npz of the planes per written frame,
    equal to render_gbuffer's (cornell, 64x48, one frame)."""
    from bihrt.app import main
    out, gb = tmp_path / "f%02d.ppm", tmp_path / "g%02d.npz"
    assert main(["--scene", "cornell", "--width", "64", "--height", "48", "--frames", "1",
                 "--out", str(out), "--gbuffer", str(gb)]) == 0
    assert os.path.exists(tmp_path / "f00.ppm")
    ref = bihrt_mod.Renderer(tree("cornell"), 64, 48).render_gbuffer(0)
    with np.load(tmp_path / "g00.npz") as z:
        assert sorted(z.files) == sorted(PLANES)
        for name in PLANES:
            assert z[name].dtype == ref[name].dtype and np.array_equal(bits(z[name]), bits(ref[name])), name
    assert (ref["coverage"] > 0).any()
