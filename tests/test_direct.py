"""Direct-lighting render (bih_render_direct / bih_render_direct_device,
DESIGN.md section 4.5.3): per primary sample the directional lights that reach
its hit point, and the pixel's irradiance and grey shade.

Expected values come from the oracle alone.  The samples' hits are
tests/test_gbuffer.py's `expected` (OracleTree.closest on the restated primary
rays); the hit point, the normal and every c_k are numpy f32 in the header's
order; a facing pair is occluded when OracleTree.closest(P, L, 1e-4) finds a
triangle; the sums are numpy f32, accumulated sequentially.  Every comparison
is on bits.  Each (scene, camera, shape, frame, lights) is answered once and
shared by the tests that use it.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import test_gbuffer as tg
from conftest import ROOT
from test_gbuffer import (EDGE, F32, LIBDIR, SEED, bits, camera, expected, frame_rays, normals,  # noqa: F401
                          renderer, scene, tree)

SRC = os.path.join(ROOT, "tests", "c", "direct_smoke.c")
T_LO = 1e-4                      # BIH_SHADOW_T_LO
MISS_SHADE = 0x00281414
NAMES = ("lit", "irradiance", "rgba")
CONVEX = ("dodeca", "bih1_dodeca")          # no facing pair can be occluded
# Under camera K1 these are not hit at all (every lit word 0, every pixel the miss
# shade); under K2 all of them are, the first three by 19-21 % of the samples
K1_UNHIT = ("one_tri", "two_tris", "dup_all", "clustered")


def fib_lights(K):
    """K Fibonacci directions over the whole sphere (half of them behind any
    normal), f64 cast to f32; weights (1 + k%3) / K."""
    import bihrt
    i = np.arange(K, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / K
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    r = np.sqrt(1.0 - z * z)
    out = np.zeros(K, bihrt.LIGHT_DTYPE)
    out["dir"] = np.stack([r * np.cos(phi), z, r * np.sin(phi)], 1).astype(F32)
    out["weight"] = ((1 + np.arange(K) % 3) / K).astype(F32)
    return out


def oracle_occluded(ot):
    def fn(P, L):
        return np.array([ot.closest(P[k], L[k], T_LO)[1] >= 0 for k in range(P.shape[0])], bool)
    return fn


def restate(tris, cam, hits, d, lights, occluded, spp):
    """The header's direct lighting of samples with hit records `hits`
    (HIT_DTYPE, prim in file order) and primary directions d (n, 3): lit, the
    pixel planes (flat), and the facing and occluded (sample, light) masks.
    occluded(P, L) answers the shadow rays of the facing pairs."""
    import bihrt
    L, wgt = np.ascontiguousarray(lights["dir"], F32), np.ascontiguousarray(lights["weight"], F32)
    K, n = L.shape[0], hits.shape[0]
    hit = hits["prim"] != bihrt.NO_HIT
    with np.errstate(all="ignore"):
        P = cam[0:3][None, :] + hits["t"][:, None] * d            # one multiply, then one add
        nrm = np.zeros((n, 3), F32)
        nrm[hit] = normals(tris[hits["prim"][hit]])
        c = (nrm[:, 0:1] * L[None, :, 0] + nrm[:, 1:2] * L[None, :, 1]) + nrm[:, 2:3] * L[None, :, 2]
        assert P.dtype == F32 and c.dtype == F32 and c.shape == (n, K)
        facing = hit[:, None] & (c > 0)
        si, ki = np.nonzero(facing)
        occ = np.zeros((n, K), bool)
        if si.size:
            occ[si, ki] = occluded(P[si], L[ki])
        litb = facing & ~occ
        lit = np.zeros(n, np.uint64)
        e = np.zeros(n, F32)
        for k in range(K):                                        # k ascending over the lit bits
            lit |= litb[:, k].astype(np.uint64) << np.uint64(k)
            e = np.where(litb[:, k], e + wgt[k] * c[:, k], e)
        e = e.reshape(-1, spp)
        acc = e[:, 0]
        for s in range(1, spp):
            acc = acc + e[:, s]
        E = acc / F32(spp)
        assert E.dtype == F32
        g = np.fmax(F32(0), np.fmin(F32(255), F32(255) * E)).astype(np.int32).astype(np.uint32)
    rgba = np.where(hit.reshape(-1, spp).any(1), g | (g << 8) | (g << 16), np.uint32(MISS_SHADE)).astype(np.uint32)
    out = {"lit": lit, "irradiance": E, "rgba": rgba, "hit": hit, "facing": facing, "occ": occ}
    for a in out.values():
        a.setflags(write=False)
    return out


def expect_with(name, kname, w, h, spp, frame, lights):
    tris, ot = scene(name)
    cam = camera(name, kname, w, h)
    d = frame_rays(cam, w, h, spp, frame).reshape(-1, 3)
    return restate(tris, cam, expected(name, kname, w, h, spp, frame)["hits"], d, lights, oracle_occluded(ot), spp)


@functools.lru_cache(maxsize=None)
def expect(name, kname, w, h, spp, frame, K):
    """The oracle's direct lighting of the whole frame under fib_lights(K); read-only, computed once."""
    return expect_with(name, kname, w, h, spp, frame, fib_lights(K))


def shares(exp):
    """(hit share of samples, facing share of (hit sample, light) pairs, occluded share of facing pairs)."""
    pairs = exp["hit"].sum() * exp["facing"].shape[1]
    return (float(exp["hit"].mean()), float(exp["facing"].sum() / max(pairs, 1)),
            float(exp["occ"].sum() / max(exp["facing"].sum(), 1)))


def balanced(exp, what):
    """A frame that degenerates must fail, not pass vacuously."""
    hs, fs, os_ = shares(exp)
    assert 0.10 <= hs <= 0.90, f"{what}: hit share {hs:.3f}"
    assert 0.30 <= fs <= 0.70, f"{what}: facing share {fs:.3f}"
    assert 0.10 <= os_ <= 0.90, f"{what}: occluded share of facing pairs {os_:.3f}"


def rows_of(exp, w, spp, ys):
    """The expected planes of global rows ys (local row order)."""
    ys = np.asarray(ys)
    return {"lit": exp["lit"].reshape(-1, w * spp)[ys].reshape(-1),
            "irradiance": exp["irradiance"].reshape(-1, w)[ys], "rgba": exp["rgba"].reshape(-1, w)[ys]}


def assert_direct(got, exp, what="", names=NAMES):
    for name in names:
        g, e = got[name], np.asarray(exp[name]).reshape(got[name].shape)
        assert g.dtype == e.dtype, f"{what}: {name} {g.dtype}"
        bad = np.argwhere(bits(g) != bits(e))
        assert bad.size == 0, f"{what}: {name} differs at {bad[:4].tolist()} ({bad.shape[0]} values)"


@pytest.fixture(scope="module", autouse=True)
def _free_trees():
    yield
    while tg._trees:
        tg._trees.popitem()[1].close()


class DevDirect:
    """Device planes (torch tensors prefilled with 0xAB) of a direct-lighting call."""

    def __init__(self, nrows, w, spp, names=NAMES):
        import torch
        self.nrows, self.w, self.spp, self.names = nrows, w, spp, names
        P = nrows * w
        self.t = {k: torch.full((P * (8 * spp if k == "lit" else 4),), 0xAB, dtype=torch.uint8, device="cuda")
                  for k in NAMES}
        torch.cuda.synchronize()

    def launch(self, r, lights, frame, rows=None, stream=None):
        r.render_direct_device({k: self.t[k].data_ptr() for k in self.names}, lights, frame, rows, stream)

    def result(self):
        """Every plane (also the ones not asked for), shaped as render_direct's."""
        import bihrt
        out = {}
        for k, ten in self.t.items():
            dt, per = bihrt.DIRECT_PLANES[k]
            a = ten.cpu().numpy().view(dt)
            out[k] = a.reshape(self.nrows, self.w) if per else a
        return out


def dev_direct(r, lights, frame, rows=None, names=NAMES):
    nrows = rows.nrows if rows is not None else r.h
    dv = DevDirect(nrows, r.w, r.spp, names)
    dv.launch(r, lights, frame, rows)
    r.sync()
    return dv.result()


def gpu_occluded(g):
    """bih_trace_device(OCCLUDED) on the restated shadow rays."""
    def fn(P, L):
        import bihrt
        import torch
        rays = bihrt.pack_rays(P, L, F32(T_LO))
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        d_out = torch.full((rays.shape[0],), 0xAB, dtype=torch.uint8, device="cuda")
        g.trace_device(d_rays.data_ptr(), rays.shape[0], d_out.data_ptr(), bihrt.QUERY_OCCLUDED)
        g.sync()
        out = d_out.cpu().numpy()
        assert ((out == 0) | (out == 1)).all()
        return out == 1
    return fn


# --- CPU ------------------------------------------------------------------------

def test_struct_layout(bihrt_mod):
    Lt, D = bihrt_mod.Light, bihrt_mod.Direct
    assert C.sizeof(Lt) == 16 and Lt.dir.offset == 0 and Lt.weight.offset == 12
    assert bihrt_mod.LIGHT_DTYPE.itemsize == 16 and bihrt_mod.LIGHT_DTYPE.fields["weight"][1] == 12
    assert C.sizeof(D) == 3 * C.sizeof(C.c_void_p)
    assert [f[0] for f in D._fields_] == ["lit", "irradiance", "rgba"]
    assert [getattr(D, f).offset for f, _ in D._fields_] == [k * C.sizeof(C.c_void_p) for k in range(3)]
    assert bihrt_mod.MAX_LIGHTS == 64 and sorted(bihrt_mod.DIRECT_PLANES) == sorted(NAMES)
    assert F32(bihrt_mod.SHADOW_T_LO) == F32(T_LO)
    hdr = open(os.path.join(ROOT, "include", "bih.h")).read()
    assert "#define BIH_MAX_LIGHTS   64" in hdr and "#define BIH_SHADOW_T_LO  1e-4f" in hdr
    assert "#define BIH_ABI_VERSION 4" in hdr


def test_device_free_error_codes(bihrt_mod):
    """The argument checks come, in the header's order, before the tree or a
    device is touched: a stand-in tree pointer is never dereferenced."""
    L = bihrt_mod._lib.load()
    INVALID, TOO_LARGE = -1, -6
    raw = (C.c_char * 96)()
    base = (C.addressof(raw) + 15) & ~15
    fake = C.c_void_p(base)
    cam = bihrt_mod.Camera()
    D, R = bihrt_mod.Direct, bihrt_mod.Rows
    sun = (bihrt_mod.Light * 1)()
    sun[0].dir[1], sun[0].weight = 1.0, 1.0
    rgba, lit, none = D(rgba=base), D(lit=base), D()
    odd = D(lit=base + 4, rgba=base)
    for entry in (lambda *a: L.bih_render_direct_device(*a, None), L.bih_render_direct):
        def call(t, c, w, h, spp, rows, lights, k, d):
            return entry(t, C.byref(c) if c is not None else None, w, h, spp, 0, SEED,
                         C.byref(rows) if rows is not None else None,
                         C.cast(lights, C.c_void_p) if lights is not None else None, k,
                         C.byref(d) if d is not None else None)
        # 1: the G-buffer's checks, in its order
        assert call(None, cam, 8, 8, 4, None, sun, 1, rgba) == INVALID
        assert call(fake, None, 8, 8, 4, None, sun, 1, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, None, sun, 1, None) == INVALID
        for whs in ((0, 8, 4), (8, 0, 4), (8, 8, 0)):
            assert call(fake, cam, *whs, None, sun, 1, rgba) == INVALID
        assert call(fake, cam, 8, 8, 65, None, sun, 1, rgba) == INVALID
        assert call(fake, cam, 1 << 16, 1 << 16, 65, None, sun, 1, rgba) == INVALID   # (before TOO_LARGE)
        assert call(fake, cam, 8, 8, 4, None, sun, 1, none) == INVALID             # all three planes NULL
        assert call(fake, cam, 1 << 16, 1 << 16, 1, None, sun, 1, none) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 4, 0, 1), sun, 1, rgba) == INVALID     # rows
        assert call(fake, cam, 8, 8, 4, R(0, 4, 2, 0), sun, 1, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, R(6, 4, 4, 1), sun, 1, rgba) == INVALID
        assert call(fake, cam, 1 << 16, 1 << 16, 1, None, sun, 1, rgba) == TOO_LARGE
        assert call(fake, cam, 1 << 16, 1 << 16, 1, None, None, 0, odd) == TOO_LARGE   # (before 2 and 3)
        # 2: the lights
        assert call(fake, cam, 8, 8, 4, None, None, 1, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, None, sun, 0, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, None, sun, 65, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), sun, 0, rgba) == INVALID     # (before nrows == 0)
        # 3: lit's alignment
        assert call(fake, cam, 8, 8, 4, None, sun, 1, odd) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), sun, 1, odd) == INVALID      # (before nrows == 0)
        # 4: nothing to do
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), sun, 1, lit) == 0
        assert call(fake, cam, 8, 8, 64, R(3, 0, 0, 0), sun, 64, rgba) == 0
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), sun, 1, D(lit=base + 8)) == 0   # 8-byte alignment suffices


def _build_c(tmp_path) -> str:
    exe = str(tmp_path / "direct_smoke")
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
    assert "FAIL" not in r.stdout and r.stdout.count("ok ") == 13, r.stdout


def test_sky_dome(bihrt_mod):
    """k unit directions on the upper hemisphere whose weights make a horizontal
    unoccluded surface sum to 1; the sun is prepended."""
    for k in (1, 8, 63):
        sky = bihrt_mod.scenes.sky_dome(k)
        assert sky.dtype == bihrt_mod.LIGHT_DTYPE and sky.shape == (k,)
        d = sky["dir"].astype(np.float64)
        assert (d[:, 1] > 0).all() and np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-6)
        assert abs((sky["weight"].astype(np.float64) * d[:, 1]).sum() - 1.0) < 1e-5      # n = +y: c_k = dir.y
        assert np.unique(np.round(d, 5), axis=0).shape[0] == k
    both = bihrt_mod.scenes.sky_dome(8, sun=(1.0, 2.0, 2.0))
    assert both.shape == (9,) and np.allclose(both["dir"][0], [1 / 3, 2 / 3, 2 / 3], atol=1e-6)
    assert both["weight"][0] == 1.0 and np.array_equal(both[1:], bihrt_mod.scenes.sky_dome(8))
    with pytest.raises(ValueError):
        bihrt_mod.scenes.sky_dome(0)


def test_app_options_need_direct(bihrt_mod):
    """--sun and --sky without --direct are an error, not ignored (before any device is used)."""
    from bihrt.app import main
    for extra in (["--sun", "0,1,0"], ["--sky", "4"]):
        with pytest.raises(SystemExit):
            main(["--scene", "cornell", "--frames", "1"] + extra)
    with pytest.raises(SystemExit):
        main(["--scene", "cornell", "--direct", "d.ppm", "--sky", "0"])          # no light at all


def test_origin_triangle_cannot_block(oracle_mod, bihrt_mod):
    """A check of the checker: the restated shadow rays of soup3k (48x32x4,
    frame 1) answer identically at t_lo = 1e-4 whether the originating triangle
    is in the soup or removed from it: a facing light has det < 0 on the
    triangle it leaves, so that triangle never blocks its own ray."""
    w, h, spp, K = 48, 32, 4, 8
    tris, ot = scene("soup3k")
    exp = expect("soup3k", "K1", w, h, spp, 1, K)
    balanced(exp, "soup3k")
    cam = camera("soup3k", "K1", w, h)
    hits = expected("soup3k", "K1", w, h, spp, 1)["hits"]
    d = frame_rays(cam, w, h, spp, 1).reshape(-1, 3)
    with np.errstate(all="ignore"):               # (a miss has t = FLT_MAX; only hit samples are used)
        P = cam[0:3][None, :] + hits["t"][:, None] * d
    L = fib_lights(K)["dir"]
    si, ki = np.nonzero(exp["facing"])
    prim = hits["prim"][si]
    # det of the originating triangle under its facing lights: negative, all of them
    t3 = tris[prim].astype(np.float64)
    e1, e2 = t3[:, 3:6] - t3[:, 0:3], t3[:, 6:9] - t3[:, 0:3]
    det = np.einsum("ij,ij->i", e1, np.cross(L[ki].astype(np.float64), e2))
    assert (det < 0).all()
    checked = 0
    for p in np.unique(prim):
        sel = np.flatnonzero(prim == p)
        without = oracle_mod.OracleTree(np.delete(tris, p, axis=0))
        for j in sel:
            a = ot.closest(P[si[j]], L[ki[j]], T_LO)[1] >= 0
            assert a == bool(exp["occ"][si[j], ki[j]])
            assert a == (without.closest(P[si[j]], L[ki[j]], T_LO)[1] >= 0), (p, j)
            checked += 1
    assert checked == si.size and checked > 1000


# --- GPU ------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kname", ["K1", "K2"])
@pytest.mark.parametrize("name", EDGE)
def test_edge_scenes(name, kname, gpu, bihrt_mod):
    """All nine edge scenes at 48x32x4, K = 8, frame 1, under camera K1 and
    under K2, which hits every one of them (test_gbuffer.py's camera): the
    one-leaf trees one_tri and dup_all cast shadow rays only there.  cornell
    also with every primary sample walked."""
    exp = expect(name, kname, 48, 32, 4, 1, 8)
    lit_pairs = exp["facing"] & ~exp["occ"]
    if name == "cornell":
        balanced(exp, name)
    elif name in CONVEX:
        assert exp["hit"].any() and exp["facing"].any() and not exp["occ"].any()
    elif kname == "K1" and name in K1_UNHIT:
        assert not exp["hit"].any() and (exp["rgba"] == MISS_SHADE).all()     # (bits only; K2 casts their rays)
    elif name in K1_UNHIT[:3]:
        # as test_gbuffer.balanced; parallel or identical triangles: no facing pair is occluded
        assert 0.10 <= exp["hit"].mean() <= 0.90 and exp["facing"].any() and not exp["occ"].any()
    elif name == "clustered":
        assert exp["hit"].any() and exp["facing"].any() and exp["occ"].any()
    else:
        assert exp["hit"].any() and exp["facing"].any()
    if kname == "K2":
        assert lit_pairs.any() and (exp["lit"] != 0).any(), "no shadow ray is unoccluded"
    g = tree(name)
    r = renderer(g, name, kname, 48, 32, 4)
    lights = fib_lights(8)
    assert_direct(dev_direct(r, lights, 1), exp, f"{name} {kname}")
    if name == "cornell":
        g.set_param(bihrt_mod.PARAM_GBUFFER_MASK, 0)
        try:
            assert_direct(dev_direct(r, lights, 1), exp, name + " mask=0")
        finally:
            g.set_param(bihrt_mod.PARAM_GBUFFER_MASK, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,spp,K,kname", [(1, 1, 1, 1, "K1"), (37, 29, 3, 5, "K2"), (8, 8, 64, 3, "K1"),
                                             (37, 29, 1, 33, "K1"), (16, 8, 16, 64, "K1"), (20, 12, 5, 7, "K1")])
def test_shapes(w, h, spp, K, kname, gpu, bihrt_mod):
    """One sample; partial tiles and waves; spp that is no power of two; a
    pixel per wave; masks that cross bit 31/32 and reach bit 63."""
    exp = expect("soup20k", kname, w, h, spp, 1, K)
    if (w, h, spp, K) in ((37, 29, 3, 5), (16, 8, 16, 64)):
        balanced(exp, f"{w}x{h}x{spp} K={K}")
    elif (w, h) != (1, 1):
        assert exp["hit"].any() and exp["facing"].any() and (exp["facing"] & ~exp["occ"]).any()
    if K > 32:
        assert (exp["lit"] >> np.uint64(32)).any() and (exp["lit"] & np.uint64(0xFFFFFFFF)).any()
    if K == 64:
        assert (exp["lit"] >> np.uint64(63)).any()
    r = renderer(tree("soup20k"), "soup20k", kname, w, h, spp)
    assert_direct(dev_direct(r, fib_lights(K), 1), exp, f"{w}x{h}x{spp} K={K}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["soup20k", "soup3k"])
def test_soups(name, gpu, bihrt_mod):
    """Deep shadow walks: a third of the samples hit, two fifths of soup20k's
    facing pairs are occluded; soup20k once more with two stack slots on chip."""
    exp = expect(name, "K1", 48, 32, 4, 1, 8)
    balanced(exp, name)
    g = tree(name)
    r = renderer(g, name, "K1", 48, 32, 4)
    assert_direct(dev_direct(r, fib_lights(8), 1), exp, name)
    if name == "soup20k":
        g.set_param(bihrt_mod.PARAM_TRACE_LDS_SLOTS, 2)
        try:
            assert_direct(dev_direct(r, fib_lights(8), 1), exp, "2 slots")
        finally:
            g.set_param(bihrt_mod.PARAM_TRACE_LDS_SLOTS, 0)


@pytest.mark.gpu
def test_matches_trace_device(gpu, bihrt_mod):
    """Composition: `lit` equals bih_trace_device(OCCLUDED) on the restated
    shadow rays, GPU against GPU, and both equal the oracle."""
    w, h, spp, K = 48, 32, 4, 8
    exp = expect("soup3k", "K1", w, h, spp, 1, K)
    balanced(exp, "soup3k")
    tris = scene("soup3k")[0]
    cam = camera("soup3k", "K1", w, h)
    g = tree("soup3k")
    d = frame_rays(cam, w, h, spp, 1).reshape(-1, 3)
    traced = restate(tris, cam, expected("soup3k", "K1", w, h, spp, 1)["hits"], d, fib_lights(K), gpu_occluded(g), spp)
    assert np.array_equal(traced["occ"], exp["occ"])
    got = dev_direct(renderer(g, "soup3k", "K1", w, h, spp), fib_lights(K), 1)
    assert_direct(got, traced, "direct vs trace")
    assert_direct(got, exp, "direct vs oracle")


@pytest.mark.gpu
def test_grid_larger_than_persistent_grid(gpu, bihrt_mod):
    """96x96x4 on soup20k with K = 64: more (listed sample, light) items than
    the persistent grid has lanes, so lanes come back for more.  Expected: the
    G-buffer's hits and bih_trace_device's occlusion flags (both pinned by their
    own tests) through the restatement; the oracle would take too long here."""
    import torch
    w, h, spp, K = 96, 96, 4, 64
    tris = scene("soup20k")[0]
    cam = camera("soup20k", "K1", w, h)
    g = tree("soup20k")
    r = renderer(g, "soup20k", "K1", w, h, spp)
    hits = r.render_gbuffer(1, planes=(), hits=True)["hits"]
    d = frame_rays(cam, w, h, spp, 1).reshape(-1, 3)
    exp = restate(tris, cam, hits, d, fib_lights(K), gpu_occluded(g), spp)
    balanced(exp, "large grid")
    listed = int(exp["facing"].any(1).sum())
    lanes = torch.cuda.get_device_properties(0).multi_processor_count * 32 * 64
    assert listed * K > lanes, (listed, lanes)
    assert_direct(dev_direct(r, fib_lights(K), 1), exp, "large grid")


@pytest.mark.gpu
def test_rows_and_bands(gpu, bihrt_mod):
    """Rows {4, 8, 4, 2} (interleaved bands) and {5, 7, 7, 1} (not tile-aligned)
    of a 48x32 frame equal the same rows of the full frame; host entry too."""
    exp = expect("soup20k", "K1", 48, 32, 4, 1, 8)
    r = renderer(tree("soup20k"), "soup20k", "K1", 48, 32, 4)
    for rows, ys in ((bihrt_mod.Rows(4, 8, 4, 2), [4, 5, 6, 7, 12, 13, 14, 15]),
                     (bihrt_mod.Rows(5, 7, 7, 1), list(range(5, 12)))):
        sub = rows_of(exp, 48, 4, ys)
        assert (sub["lit"] != 0).any() and (sub["lit"] == 0).any()
        assert_direct(dev_direct(r, fib_lights(8), 1, rows), sub, f"rows {ys[0]}..")
        assert_direct(r.render_direct(fib_lights(8), 1, rows), sub, "host entry rows")


@pytest.mark.gpu
def test_plane_subsets(gpu, bihrt_mod):
    """Each plane alone gives the bits of all planes together; planes that were
    not asked for stay untouched (0xAB)."""
    exp = expect("soup20k", "K1", 48, 32, 4, 1, 8)
    r = renderer(tree("soup20k"), "soup20k", "K1", 48, 32, 4)
    for name in NAMES:
        got = dev_direct(r, fib_lights(8), 1, names=(name,))
        assert_direct(got, exp, f"{name} alone", names=(name,))
        for other in NAMES:
            if other != name:
                assert (np.ascontiguousarray(got[other]).view(np.uint8) == 0xAB).all(), (name, other)


@pytest.mark.gpu
def test_odd_lights(gpu, bihrt_mod):
    """Zero, NaN and Inf directions, zero and negative weights, duplicate
    lights: every bit and sum equals the restatement."""
    w, h, spp = 48, 32, 4
    base = fib_lights(8)
    odd = np.zeros(14, bihrt_mod.LIGHT_DTYPE)
    odd[:4] = base[[0, 1, 2, 3]]
    odd[4] = base[1]                                   # a duplicate
    odd[5] = ((0, 0, 0), 1.0)                          # zero: never facing
    odd[6] = ((np.nan, 1, 0), 1.0)                     # NaN: never facing
    odd[7] = ((np.inf, 0, 0), 0.25)                    # Inf: c = +-inf or NaN
    odd[8] = ((0, -np.inf, np.inf), 0.25)
    odd[9] = (tuple(base["dir"][2]), 0.0)              # zero weight
    odd[10] = (tuple(base["dir"][1]), -0.5)            # negative weight
    odd[11] = (tuple(base["dir"][3]), -0.0)
    odd[12] = base[5]
    odd[13] = ((0, 1e-30, 0), 1e30)                    # tiny direction, huge weight
    exp = expect_with("soup20k", "K1", w, h, spp, 1, odd)
    assert not exp["facing"][:, 5].any() and not exp["facing"][:, 6].any()
    assert exp["facing"][:, 7].any() and exp["facing"][:, 13].any()
    assert np.array_equal(exp["facing"][:, 4], exp["facing"][:, 1]) and np.array_equal(exp["occ"][:, 4], exp["occ"][:, 1])
    lit = exp["facing"] & ~exp["occ"]
    assert lit[:, 9].any() and lit[:, 10].any() and lit[:, 4].any()
    r = renderer(tree("soup20k"), "soup20k", "K1", w, h, spp)
    assert_direct(dev_direct(r, odd, 1), exp, "odd lights")


@pytest.mark.gpu
def test_renders_undisturbed(gpu, bihrt_mod):
    """render f=0, direct f=2, render f=2, render f=3, direct f=3: every image
    is the oracle's and every plane is right."""
    w, h, spp = 48, 32, 4
    tris, ot = scene("cornell")
    cam = camera("cornell", "K1", w, h)
    g = bihrt_mod.GPUArrayManager(tris)
    r = renderer(g, "cornell", "K1", w, h, spp)
    lights = fib_lights(8)
    f0 = r.render(0)
    d2 = r.render_direct(lights, 2)
    f2 = r.render(2)
    f3 = r.render(3)
    d3 = r.render_direct(lights, 3)
    assert r.frame == 4
    for f, img in ((0, f0), (2, f2), (3, f3)):
        assert np.array_equal(img, ot.render(w, h, spp=spp, frame=f, seed=SEED, cam=cam)[0]), f
    assert_direct(d2, expect("cornell", "K1", w, h, spp, 2, 8), "frame 2")
    assert_direct(d3, expect("cornell", "K1", w, h, spp, 3, 8), "frame 3")
    g.close()


@pytest.mark.gpu
def test_rebuild_ordering(gpu, bihrt_mod):
    """A direct-lighting render on a second stream after rebuild() sees the new soup's tree."""
    import torch
    w, h, spp = 48, 32, 4
    old, new = scene("soup3k")[0], scene("soup3k2")[0]
    soup = torch.from_numpy(old.copy()).cuda()
    torch.cuda.synchronize()
    g = bihrt_mod.GPUArrayManager.from_device(soup.data_ptr(), old.shape[0])
    exp0, exp1 = expect("soup3k", "K1", w, h, spp, 1, 8), expect("soup3k2", "K1", w, h, spp, 1, 8)
    balanced(exp0, "soup3k")
    balanced(exp1, "soup3k2")
    assert not np.array_equal(exp0["lit"], exp1["lit"])
    r0, r1 = renderer(g, "soup3k", "K1", w, h, spp), renderer(g, "soup3k2", "K1", w, h, spp)
    d0, d1 = DevDirect(h, w, spp), DevDirect(h, w, spp)
    d0.launch(r0, fib_lights(8), 1)
    g.sync()                      # (the caller's duty: the soup is not rewritten under a build or render)
    soup.copy_(torch.from_numpy(new))
    torch.cuda.synchronize()
    g.rebuild()
    s2 = torch.cuda.Stream()
    d1.launch(r1, fib_lights(8), 1, stream=s2.cuda_stream)
    s2.synchronize()
    assert_direct(d0.result(), exp0, "before the rebuild")
    assert_direct(d1.result(), exp1, "after the rebuild")
    g.close()


@pytest.mark.gpu
def test_two_streams(gpu, bihrt_mod):
    """Two direct-lighting renders of one tree issued back to back on two
    streams with different lights, and a third behind them on the first."""
    import torch
    w, h, spp = 48, 32, 4
    g = tree("soup3k")
    r = renderer(g, "soup3k", "K1", w, h, spp)
    ea, eb = expect("soup3k", "K1", w, h, spp, 1, 8), expect("soup3k", "K1", w, h, spp, 2, 5)
    da, db, dc = DevDirect(h, w, spp), DevDirect(h, w, spp), DevDirect(h, w, spp)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    da.launch(r, fib_lights(8), 1, stream=sa.cuda_stream)
    db.launch(r, fib_lights(5), 2, stream=sb.cuda_stream)
    dc.launch(r, fib_lights(8), 1, stream=sa.cuda_stream)
    sa.synchronize()
    sb.synchronize()
    assert_direct(da.result(), ea, "stream a")
    assert_direct(db.result(), eb, "stream b")
    assert_direct(dc.result(), ea, "stream a again")


@pytest.mark.gpu
def test_host_entry_equals_device_entry(gpu, bihrt_mod):
    exp = expect("soup3k", "K1", 48, 32, 4, 1, 8)
    r = renderer(tree("soup3k"), "soup3k", "K1", 48, 32, 4)
    host = r.render_direct(fib_lights(8), 1)
    assert sorted(host) == sorted(NAMES) and r.frame == 2
    assert host["lit"].shape == (48 * 32 * 4,) and host["rgba"].shape == (32, 48)
    assert_direct(host, dev_direct(r, fib_lights(8), 1), "host vs device")
    assert_direct(host, exp, "host")
    only = r.render_direct(fib_lights(8).view(F32).reshape(-1, 4), 1, planes=("irradiance",))   # (k, 4) rows
    assert sorted(only) == ["irradiance"]
    assert_direct(only, exp, "one plane", names=("irradiance",))


@pytest.mark.gpu
def test_steady_state_allocations(gpu, bihrt_mod):
    """After the first call of a shape and light count further calls allocate nothing."""
    tris = scene("soup3k")[0]
    g = bihrt_mod.GPUArrayManager(tris)
    r = renderer(g, "soup3k", "K1", 48, 32, 4)
    before = g.info()
    dev_direct(r, fib_lights(8), 0)
    first = g.info()
    assert first.device_allocs > before.device_allocs
    assert first.device_bytes >= before.device_bytes + 48 * 32 * 4 * 28
    for f in (2, 5, 1):
        got = dev_direct(r, fib_lights(8), f, names=("lit", "rgba") if f == 5 else NAMES)
    after = g.info()
    assert after.device_allocs == first.device_allocs and after.device_bytes == first.device_bytes
    assert_direct(got, expect("soup3k", "K1", 48, 32, 4, 1, 8), "steady state")
    # the tree's own lit words (8 bytes per sample) come with the first call that passes no `lit`
    got = dev_direct(r, fib_lights(8), 1, names=("irradiance",))
    own = g.info()
    assert own.device_allocs == after.device_allocs + 1 and own.device_bytes == after.device_bytes + 48 * 32 * 4 * 8
    for f in (3, 1):
        got = dev_direct(r, fib_lights(8), f, names=("irradiance", "rgba"))
    last = g.info()
    assert last.device_allocs == own.device_allocs and last.device_bytes == own.device_bytes
    assert_direct(got, expect("soup3k", "K1", 48, 32, 4, 1, 8), "own lit words", names=("irradiance", "rgba"))
    g.close()


@pytest.mark.gpu
def test_c_caller(tmp_path, gpu, bihrt_mod):
    """tests/c/direct_smoke.c -- bih_build + bih_render_direct from strict C11
    (cornell, 64x48, the reference camera, a sky and a sun): the planes equal
    render_direct's."""
    exe = _build_c(tmp_path)
    tris = scene("cornell")[0]
    w, h, spp = 64, 48, 4
    lights = bihrt_mod.scenes.sky_dome(8, sun=(0.3, 1.0, -0.4))
    sp, lp, op = tmp_path / "scene.f32", tmp_path / "lights.f32", tmp_path / "planes.bin"
    tris.tofile(sp)
    lights.tofile(lp)
    r = subprocess.run([exe, str(sp), str(tris.shape[0]), str(w), str(h), str(spp), "0", str(lp),
                        str(lights.shape[0]), str(op)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "direct_smoke OK" in r.stdout, r.stdout + r.stderr
    ref = bihrt_mod.Renderer(tree("cornell"), w, h, spp=spp).render_direct(lights, 0)
    assert (ref["lit"] != 0).any() and (ref["irradiance"] > 0).any()
    raw = np.fromfile(op, np.uint8)
    P = w * h
    assert raw.size == P * (8 * spp + 4 + 4)
    off = 0
    for name, size in (("lit", 8 * spp), ("irradiance", 4), ("rgba", 4)):
        part = raw[off:off + P * size]
        off += P * size
        assert np.array_equal(part, np.ascontiguousarray(ref[name]).view(np.uint8).reshape(-1)), name


@pytest.mark.gpu
def test_app_writes_ppm(tmp_path, gpu, bihrt_mod):
    """python -m bihrt --direct: one PPM of the rgba plane per written frame,
    equal to render_direct's under sky_dome(8, sun) (cornell, 64x48, one frame)."""
    from bihrt.app import main
    out, dr = tmp_path / "f%02d.ppm", tmp_path / "d%02d.ppm"
    assert main(["--scene", "cornell", "--width", "64", "--height", "48", "--frames", "1",
                 "--out", str(out), "--direct", str(dr), "--sun", "0.3,1,-0.4", "--sky", "8"]) == 0
    assert os.path.exists(tmp_path / "f00.ppm")
    lights = bihrt_mod.scenes.sky_dome(8, sun=(0.3, 1.0, -0.4))
    ref = bihrt_mod.Renderer(tree("cornell"), 64, 48).render_direct(lights, 0, planes=("rgba",))["rgba"]
    want = tmp_path / "want.ppm"
    bihrt_mod.write_ppm(str(want), ref)
    assert open(tmp_path / "d00.ppm", "rb").read() == open(want, "rb").read()
    grey = bihrt_mod.unpack_rgba(ref)[..., 0]
    assert np.unique(grey).size > 4 and (ref == MISS_SHADE).any()
    # App.run without lights: the plain sky
    from bihrt.app import App
    app = App(64, 48)
    app.load_models(scene("cornell")[0])
    app.run(1, direct_pattern=str(tmp_path / "sky.ppm"))
    sky = bihrt_mod.Renderer(tree("cornell"), 64, 48).render_direct(bihrt_mod.scenes.sky_dome(8), 0, planes=("rgba",))
    bihrt_mod.write_ppm(str(want), sky["rgba"])
    assert open(tmp_path / "sky.ppm", "rb").read() == open(want, "rb").read()
    app.arrays.close()
