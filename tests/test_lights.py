"""Direct lighting with point lights (bih_render_lights /
bih_render_lights_device): lamps at a position next to
the directional lights of bih_render_direct.  A triangle behind a lamp does not
shadow it.

Expected values come from the oracle alone, as tests/test_direct.py's, whose
structure `restate` extends here: the samples' hits are test_gbuffer's
`expected`; P, the normal, L = Q - P, every c, r2, len and term are numpy f32
in the header's order; a facing (sample, lamp) pair is occluded when
OracleTree.closest(P, L, 1e-4) finds a triangle with t < 1.0f (the rule of
BIH_QUERY_OCCLUDED_WITHIN with t_hi = 1); directional pairs as test_direct.
Planes are compared on bits; IEEE 754 leaves the sign and payload of a
generated NaN open, so a NaN irradiance is compared as NaN.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import test_direct as td
import test_gbuffer as tg
from conftest import ROOT
from test_direct import MISS_SHADE, NAMES, T_LO, DevDirect, fib_lights, rows_of
from test_gbuffer import EDGE, F32, LIBDIR, SEED, bits, camera, expected, frame_rays, normals, renderer, scene, tree

SRC = os.path.join(ROOT, "tests", "c", "lights_smoke.c")
NO_DIR = fib_lights(5)[:0]


def lamps_of(name, k=8, scale=0.6):
    import bihrt
    ot = scene(name)[1]
    return bihrt.scenes.lamps(ot.scene_lo, ot.scene_hi, k, scale)


def oracle_segment(ot):
    """(P, L) -> (blocked before the lamp, blocked only at or beyond it)."""
    def fn(P, L):
        before, beyond = np.zeros(P.shape[0], bool), np.zeros(P.shape[0], bool)
        for k in range(P.shape[0]):
            t, idx = ot.closest(P[k], L[k], T_LO)
            before[k] = idx >= 0 and F32(t) < F32(1.0)
            beyond[k] = idx >= 0 and not before[k]
        return before, beyond
    return fn


def gpu_segment(g):
    """bih_trace_device(OCCLUDED_WITHIN, t_hi = 1) on the restated lamp rays."""
    def fn(P, L):
        import bihrt
        import torch
        rays = bihrt.pack_rays(P, L, F32(T_LO), F32(1.0))
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        d_out = torch.full((rays.shape[0],), 0xAB, dtype=torch.uint8, device="cuda")
        g.trace_device(d_rays.data_ptr(), rays.shape[0], d_out.data_ptr(), bihrt.QUERY_OCCLUDED_WITHIN)
        g.sync()
        out = d_out.cpu().numpy()
        assert ((out == 0) | (out == 1)).all()
        return out == 1, np.zeros(out.shape, bool)
    return fn


def restate(tris, cam, hits, d, dir_lights, lamps, occluded, segment, spp):
    """The header's lighting of samples with hit records `hits` and primary
    directions d under dir_lights (LIGHT_DTYPE) then lamps (POINT_LIGHT_DTYPE):
    lit, the pixel planes (flat), and for the lamps the facing / blocked-before
    / blocked-beyond-only (sample, lamp) masks."""
    import bihrt
    Ld, wd = np.ascontiguousarray(dir_lights["dir"], F32), np.ascontiguousarray(dir_lights["weight"], F32)
    Q, wp = np.ascontiguousarray(lamps["pos"], F32), np.ascontiguousarray(lamps["weight"], F32)
    Kd, Kp, n = Ld.shape[0], Q.shape[0], hits.shape[0]
    hit = hits["prim"] != bihrt.NO_HIT
    with np.errstate(all="ignore"):
        P = cam[0:3][None, :] + hits["t"][:, None] * d            # one multiply, then one add
        nrm = np.zeros((n, 3), F32)
        nrm[hit] = normals(tris[hits["prim"][hit]])
        cd = (nrm[:, 0:1] * Ld[None, :, 0] + nrm[:, 1:2] * Ld[None, :, 1]) + nrm[:, 2:3] * Ld[None, :, 2]
        L = Q[None, :, :] - P[:, None, :]                         # (n, Kp, 3)
        cp = (nrm[:, 0:1] * L[:, :, 0] + nrm[:, 1:2] * L[:, :, 1]) + nrm[:, 2:3] * L[:, :, 2]
        r2 = (L[:, :, 0] * L[:, :, 0] + L[:, :, 1] * L[:, :, 1]) + L[:, :, 2] * L[:, :, 2]
        ln = np.sqrt(r2)
        term = (wp[None, :] * (cp / ln)) / r2
        assert P.dtype == F32 and cd.dtype == F32 and L.dtype == F32 and term.dtype == F32 and ln.dtype == F32
        fd = hit[:, None] & (cd > 0)
        od = np.zeros((n, Kd), bool)
        si, ki = np.nonzero(fd)
        if si.size:
            od[si, ki] = occluded(P[si], Ld[ki])
        facing = hit[:, None] & (cp > 0)
        before, beyond = np.zeros((n, Kp), bool), np.zeros((n, Kp), bool)
        si, ki = np.nonzero(facing)
        if si.size:
            before[si, ki], beyond[si, ki] = segment(P[si], L[si, ki])
        lit = np.zeros(n, np.uint64)
        e = np.zeros(n, F32)
        for k in range(Kd):                                       # k ascending: directional lights first
            on = fd[:, k] & ~od[:, k]
            lit |= on.astype(np.uint64) << np.uint64(k)
            e = np.where(on, e + wd[k] * cd[:, k], e)
        for j in range(Kp):
            on = facing[:, j] & ~before[:, j]
            lit |= on.astype(np.uint64) << np.uint64(Kd + j)
            e = np.where(on, e + term[:, j], e)
        e = e.reshape(-1, spp)
        acc = e[:, 0]
        for s in range(1, spp):
            acc = acc + e[:, s]
        E = acc / F32(spp)
        assert E.dtype == F32
        g = np.fmax(F32(0), np.fmin(F32(255), F32(255) * E)).astype(np.int32).astype(np.uint32)
    rgba = np.where(hit.reshape(-1, spp).any(1), g | (g << 8) | (g << 16), np.uint32(MISS_SHADE)).astype(np.uint32)
    out = {"lit": lit, "irradiance": E, "rgba": rgba, "hit": hit, "facing": facing, "before": before,
           "beyond": beyond, "P": P}
    for a in out.values():
        a.setflags(write=False)
    return out


def expect_with(name, kname, w, h, spp, frame, dir_lights, lamps, segment=None):
    tris, ot = scene(name)
    cam = camera(name, kname, w, h)
    d = frame_rays(cam, w, h, spp, frame).reshape(-1, 3)
    return restate(tris, cam, expected(name, kname, w, h, spp, frame)["hits"], d, dir_lights, lamps,
                   td.oracle_occluded(ot), segment or oracle_segment(ot), spp)


@functools.lru_cache(maxsize=None)
def expect(name, kname, w, h, spp, frame, Kd, Kp, scale=0.6):
    """The oracle's lighting of the whole frame under fib_lights(Kd) and
    lamps(scene box, Kp, scale); read-only, computed once."""
    return expect_with(name, kname, w, h, spp, frame, fib_lights(Kd) if Kd else NO_DIR, lamps_of(name, Kp, scale))


def classes(exp):
    """(hit share; facing share of (hit sample, lamp) pairs; of the facing pairs
    the shares blocked before the lamp / only beyond it / not at all)."""
    f = max(int(exp["facing"].sum()), 1)
    pairs = max(int(exp["hit"].sum()) * exp["facing"].shape[1], 1)
    b, y = float(exp["before"].sum() / f), float(exp["beyond"].sum() / f)
    return float(exp["hit"].mean()), float(exp["facing"].sum() / pairs), b, y, 1.0 - b - y


def three_classes(exp, what):
    """A frame that degenerates must fail, not pass vacuously."""
    hs, fs, b, y, none = classes(exp)
    assert 0.10 <= hs <= 0.90, f"{what}: hit share {hs:.3f}"
    assert b >= 0.10 and y >= 0.10 and none >= 0.10, f"{what}: before {b:.3f}, beyond-only {y:.3f}, none {none:.3f}"


def canon(a):
    """Bits of a plane, every NaN as one NaN."""
    a = np.ascontiguousarray(a)
    if a.dtype != F32:
        return a
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def assert_lights(got, exp, what="", names=NAMES):
    for name in names:
        g, e = got[name], np.asarray(exp[name]).reshape(got[name].shape)
        assert g.dtype == e.dtype, f"{what}: {name} {g.dtype}"
        bad = np.argwhere(canon(g) != canon(e))
        assert bad.size == 0, f"{what}: {name} differs at {bad[:4].tolist()} ({bad.shape[0]} values)"


class DevLights(DevDirect):
    def launch(self, r, dir_lights, lamps, frame, rows=None, stream=None):
        r.render_lights_device({k: self.t[k].data_ptr() for k in self.names}, dir_lights, lamps, frame, rows, stream)


def dev_lights(r, dir_lights, lamps, frame, rows=None, names=NAMES):
    nrows = rows.nrows if rows is not None else r.h
    dv = DevLights(nrows, r.w, r.spp, names)
    dv.launch(r, dir_lights, lamps, frame, rows)
    r.sync()
    return dv.result()


@pytest.fixture(scope="module", autouse=True)
def _free_trees():
    yield
    while tg._trees:
        tg._trees.popitem()[1].close()


# --- CPU ------------------------------------------------------------------------

def test_struct_layout(bihrt_mod):
    PL = bihrt_mod.PointLight
    assert C.sizeof(PL) == 16 and PL.pos.offset == 0 and PL.weight.offset == 12
    dt = bihrt_mod.POINT_LIGHT_DTYPE
    assert dt.itemsize == 16 and dt.fields["pos"][1] == 0 and dt.fields["weight"][1] == 12
    packed = bihrt_mod.pack_point_lights([[1, 2, 3, 4], [5, 6, 7, 8]])
    assert packed.dtype == dt and packed.shape == (2,) and packed["weight"].tolist() == [4, 8]
    assert bihrt_mod.pack_point_lights(packed) is not None and bihrt_mod.pack_point_lights(packed).shape == (2,)
    names = bihrt_mod._lib.exported_symbols_from_header()
    assert "bih_render_lights" in names and "bih_render_lights_device" in names and "bih_trace" in names
    hdr = open(os.path.join(ROOT, "include", "bih.h")).read()
    assert "#define BIH_ABI_VERSION 4" in hdr and "typedef struct bih_point_light" in hdr


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
    lamp = (bihrt_mod.PointLight * 1)()
    lamp[0].pos[1], lamp[0].weight = 1.0, 1.0
    rgba, lit, none = D(rgba=base), D(lit=base), D()
    odd = D(lit=base + 4, rgba=base)
    for entry in (lambda *a: L.bih_render_lights_device(*a, None), L.bih_render_lights):
        def call(t, c, w, h, spp, rows, dl, kd, pl, kp, d):
            return entry(t, C.byref(c) if c is not None else None, w, h, spp, 0, SEED,
                         C.byref(rows) if rows is not None else None,
                         C.cast(dl, C.c_void_p) if dl is not None else None, kd,
                         C.cast(pl, C.c_void_p) if pl is not None else None, kp,
                         C.byref(d) if d is not None else None)
        # 1: the G-buffer's checks, in its order
        assert call(None, cam, 8, 8, 4, None, sun, 1, lamp, 1, rgba) == INVALID
        assert call(fake, None, 8, 8, 4, None, sun, 1, lamp, 1, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, None, sun, 1, lamp, 1, None) == INVALID
        assert call(fake, cam, 8, 8, 65, None, sun, 1, lamp, 1, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, None, sun, 1, lamp, 1, none) == INVALID        # all planes NULL
        assert call(fake, cam, 8, 8, 4, R(6, 4, 4, 1), sun, 1, lamp, 1, rgba) == INVALID
        assert call(fake, cam, 1 << 16, 1 << 16, 1, None, None, 0, None, 0, odd) == TOO_LARGE   # (before 2 and 3)
        # 2: the lights
        assert call(fake, cam, 8, 8, 4, None, None, 0, None, 0, rgba) == INVALID      # 0 + 0
        assert call(fake, cam, 8, 8, 4, None, sun, 0, lamp, 0, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, None, sun, 33, lamp, 32, rgba) == INVALID     # 65 together
        assert call(fake, cam, 8, 8, 4, None, sun, 65, None, 0, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, None, sun, 0xFFFFFFFF, lamp, 2, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, None, None, 1, lamp, 1, rgba) == INVALID      # NULL with a count
        assert call(fake, cam, 8, 8, 4, None, sun, 1, None, 1, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), None, 0, None, 0, rgba) == INVALID   # (before nrows == 0)
        # 3: lit's alignment
        assert call(fake, cam, 8, 8, 4, None, sun, 1, lamp, 1, odd) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), None, 0, lamp, 1, odd) == INVALID    # (before nrows == 0)
        # 4: nothing to do
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), sun, 1, lamp, 1, lit) == 0
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), None, 0, lamp, 1, rgba) == 0
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), sun, 1, None, 0, rgba) == 0
        assert call(fake, cam, 8, 8, 64, R(3, 0, 0, 0), sun, 32, lamp, 32, rgba) == 0


def test_lamps(bihrt_mod):
    """k Fibonacci points on the ellipsoid centre + scale * half_extent * u_i,
    u_i test_direct.fib_lights' directions; f32; deterministic."""
    lo, hi = np.array([-1.0, 0.0, 2.0]), np.array([3.0, 1.0, 4.0])
    for k in (1, 8, 64):
        a = bihrt_mod.scenes.lamps(lo, hi, k)
        assert a.dtype == bihrt_mod.POINT_LIGHT_DTYPE and a.shape == (k,)
        assert a.tobytes() == bihrt_mod.scenes.lamps(lo.astype(F32), hi.astype(F32), k).tobytes()
        u = (a["pos"].astype(np.float64) - [1.0, 0.5, 3.0]) / (0.6 * np.array([2.0, 0.5, 1.0]))
        assert np.allclose(np.linalg.norm(u, axis=1), 1.0, atol=1e-5)
        assert np.allclose(u, fib_lights(k)["dir"], atol=1e-5)
        assert np.allclose(a["weight"], (4.0 + 0.25 + 1.0) / k)
    b = bihrt_mod.scenes.lamps(lo, hi, 4, scale=2.0, weight=0.5)
    assert (b["weight"] == 0.5).all()
    assert np.allclose(b["pos"] - F32([1.0, 0.5, 3.0]), 2.0 * np.array([2.0, 0.5, 1.0]) * fib_lights(4)["dir"], atol=1e-5)
    with pytest.raises(ValueError):
        bihrt_mod.scenes.lamps(lo, hi, 0)


def test_app_lamp_options(bihrt_mod):
    """--lamp without --direct, a malformed lamp and more than 64 lights are
    errors, before any device is used."""
    from bihrt.app import main
    base = ["--scene", "cornell", "--frames", "1"]
    for extra in (["--lamp", "0,1,0"],
                  ["--direct", "d.ppm", "--lamp", "0,1"],
                  ["--direct", "d.ppm", "--lamp", "0,1,x"],
                  ["--direct", "d.ppm", "--lamp", "0,1,2,3,4"],
                  ["--direct", "d.ppm", "--sky", "64", "--lamp", "0,1,0"],
                  ["--direct", "d.ppm", "--sky", "62", "--sun", "0,1,0", "--lamp", "0,1,0", "--lamp", "1,1,1,2"]):
        with pytest.raises(SystemExit):
            main(base + extra)


def _build_c(tmp_path) -> str:
    exe = str(tmp_path / "lights_smoke")
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
    assert "FAIL" not in r.stdout and r.stdout.count("ok ") == 15, r.stdout


def test_header_is_cxx17(tmp_path):
    """bih_ray's anonymous union: the header still compiles as C++17."""
    src = tmp_path / "hdr.cpp"
    src.write_text('#include "bih.h"\nstatic_assert(sizeof(bih_ray) == 32, "");\n'
                   "int main() { bih_ray r{}; r.t_hi = 1.0f; return r.reserved == 1.0f ? 0 : 1; }\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only",
                    "-I", os.path.join(ROOT, "include"), str(src)], check=True)


# --- GPU ------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name,kname", [("soup20k", "K2"), ("soup3k", "K2"), ("cornell", "K1")])
def test_three_classes(name, kname, gpu, bihrt_mod):
    """8 lamps inside the scene box at 48x32x4: of the facing pairs at least a
    tenth each is blocked before the lamp, blocked only beyond it (an any-hit
    shadow ray would call it shadowed; it is lit) and not blocked at all.
    soup20k once more with two stack slots on chip."""
    exp = expect(name, kname, 48, 32, 4, 1, 0, 8)
    three_classes(exp, name)
    lit_pairs = exp["facing"] & ~exp["before"]
    assert (lit_pairs & exp["beyond"]).any()
    g = tree(name)
    r = renderer(g, name, kname, 48, 32, 4)
    assert_lights(dev_lights(r, None, lamps_of(name), 1), exp, f"{name} {kname}")
    if name == "soup20k":
        g.set_param(bihrt_mod.PARAM_TRACE_LDS_SLOTS, 2)
        try:
            assert_lights(dev_lights(r, None, lamps_of(name), 1), exp, "2 slots")
        finally:
            g.set_param(bihrt_mod.PARAM_TRACE_LDS_SLOTS, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE)
def test_edge_scenes(name, gpu, bihrt_mod):
    """Every edge scene under K2, bits only; the convex dodecahedra hold the
    lamps of scale 0.6 inside (no facing pair): bih1_dodeca also with lamps
    outside (scale 2), where pairs face and none is blocked, as in two_tris."""
    for scale in (0.6, 2.0) if name == "bih1_dodeca" else (0.6,):
        exp = expect(name, "K2", 48, 32, 4, 1, 0, 8, scale)
        assert exp["hit"].any()
        if name in ("dodeca", "bih1_dodeca") and scale == 0.6:
            assert not exp["facing"].any() and not exp["lit"].any()
        if (name == "bih1_dodeca" and scale == 2.0) or name == "two_tris":
            assert classes(exp)[1] >= 0.10 and not exp["before"].any() and not exp["beyond"].any()
            assert exp["lit"].any()
        r = renderer(tree(name), name, "K2", 48, 32, 4)
        assert_lights(dev_lights(r, None, lamps_of(name, 8, scale), 1), exp, f"{name} scale {scale}")


@pytest.mark.gpu
def test_mixed_lights(gpu, bihrt_mod):
    """5 directional + 3 point lights: bits 0..4 are bih_render_direct's under
    the 5, bits 5..7 the 3 lamps' alone (n_dir = 0); the sum runs over both in
    bit order; n_point = 0 is bih_render_direct byte for byte."""
    w, h, spp = 48, 32, 4
    exp = expect("soup20k", "K2", w, h, spp, 1, 5, 3)
    assert (exp["lit"] & np.uint64(0x1F)).any() and (exp["lit"] >> np.uint64(5)).any()
    assert not (exp["lit"] >> np.uint64(8)).any()
    r = renderer(tree("soup20k"), "soup20k", "K2", w, h, spp)
    dl, pl = fib_lights(5), lamps_of("soup20k", 3)
    got = dev_lights(r, dl, pl, 1)
    assert_lights(got, exp, "5 + 3")
    only_dir = td.dev_direct(r, dl, 1)
    only_point = dev_lights(r, NO_DIR, pl, 1)
    assert_lights(only_point, expect("soup20k", "K2", w, h, spp, 1, 0, 3), "n_dir = 0")
    assert np.array_equal(got["lit"] & np.uint64(0x1F), only_dir["lit"])
    assert np.array_equal(got["lit"] >> np.uint64(5), only_point["lit"])
    no_point = dev_lights(r, dl, None, 1)
    for name in NAMES:
        assert no_point[name].tobytes() == only_dir[name].tobytes(), name
    assert (no_point["irradiance"] != got["irradiance"]).any()


@pytest.mark.gpu
def test_bit_63(gpu, bihrt_mod):
    """61 + 3 lights: the last lamp is bit 63."""
    w, h, spp = 16, 8, 16
    exp = expect("soup20k", "K1", w, h, spp, 1, 61, 3)
    assert (exp["lit"] >> np.uint64(63)).any() and (exp["lit"] & np.uint64(0xFFFFFFFF)).any()
    assert ((exp["lit"] >> np.uint64(32)) & np.uint64(0x1FFFFFFF)).any()
    r = renderer(tree("soup20k"), "soup20k", "K1", w, h, spp)
    assert_lights(dev_lights(r, fib_lights(61), lamps_of("soup20k", 3), 1), exp, "61 + 3")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,spp", [(1, 1, 1), (37, 29, 3), (8, 8, 64)])
def test_shapes(w, h, spp, gpu, bihrt_mod):
    """One sample; partial tiles and waves with an spp that is no power of two; a pixel per wave."""
    exp = expect("soup20k", "K2", w, h, spp, 1, 2, 3)
    if (w, h) != (1, 1):
        assert exp["hit"].any() and exp["facing"].any() and exp["before"].any() and (exp["lit"] >> np.uint64(2)).any()
    r = renderer(tree("soup20k"), "soup20k", "K2", w, h, spp)
    assert_lights(dev_lights(r, fib_lights(2), lamps_of("soup20k", 3), 1), exp, f"{w}x{h}x{spp}")


@pytest.mark.gpu
def test_rows_bands_planes_and_host_entry(gpu, bihrt_mod):
    """Interleaved bands and rows that are not tile-aligned equal the same rows
    of the full frame, through both entries; each plane alone gives the bits of
    all together and leaves the others untouched; no call after the first of
    the shape allocates."""
    w, h, spp = 48, 32, 4
    exp = expect("soup20k", "K2", w, h, spp, 1, 5, 3)
    g = tree("soup20k")
    r = renderer(g, "soup20k", "K2", w, h, spp)
    dl, pl = fib_lights(5), lamps_of("soup20k", 3)
    host = r.render_lights(dl, pl, 1)
    assert sorted(host) == sorted(NAMES) and host["lit"].shape == (w * h * spp,) and host["rgba"].shape == (h, w)
    assert_lights(host, exp, "host entry")
    assert_lights(host, dev_lights(r, dl, pl, 1, names=("irradiance",)), "own lit words", names=("irradiance",))
    first = g.info()
    for rows, ys in ((bihrt_mod.Rows(4, 8, 4, 2), [4, 5, 6, 7, 12, 13, 14, 15]),
                     (bihrt_mod.Rows(5, 7, 7, 1), list(range(5, 12)))):
        sub = rows_of(exp, w, spp, ys)
        assert (sub["lit"] != 0).any() and (sub["lit"] == 0).any()
        assert_lights(dev_lights(r, dl, pl, 1, rows), sub, f"rows {ys[0]}..")
        assert_lights(r.render_lights(dl, pl, 1, rows), sub, "host entry rows")
    for name in NAMES:
        got = dev_lights(r, dl, pl, 1, names=(name,))
        assert_lights(got, exp, f"{name} alone", names=(name,))
        for other in NAMES:
            if other != name:
                assert (np.ascontiguousarray(got[other]).view(np.uint8) == 0xAB).all(), (name, other)
    assert_lights(dev_lights(r, dl, lamps_of("soup20k", 3, 0.9), 2), expect_with(
        "soup20k", "K2", w, h, spp, 2, dl, lamps_of("soup20k", 3, 0.9)), "other frame, other lamps")
    after = g.info()
    assert after.device_allocs == first.device_allocs and after.device_bytes == first.device_bytes


@pytest.mark.gpu
def test_matches_trace_device(gpu, bihrt_mod):
    """Composition: `lit` equals bih_trace_device(OCCLUDED_WITHIN, t_hi = 1) on
    the restated lamp rays, GPU against GPU, and both equal the oracle."""
    w, h, spp = 48, 32, 4
    exp = expect("soup3k", "K2", w, h, spp, 1, 0, 8)
    three_classes(exp, "soup3k")
    g = tree("soup3k")
    traced = expect_with("soup3k", "K2", w, h, spp, 1, NO_DIR, lamps_of("soup3k"), gpu_segment(g))
    assert np.array_equal(traced["before"], exp["before"])
    got = dev_lights(renderer(g, "soup3k", "K2", w, h, spp), None, lamps_of("soup3k"), 1)
    assert_lights(got, traced, "lights vs trace")
    assert_lights(got, exp, "lights vs oracle")


@pytest.mark.gpu
def test_odd_lamps(gpu, bihrt_mod):
    """A lamp exactly at a hit point (L = 0 there: never lit), NaN and Inf
    positions, zero and negative weights, duplicate lamps."""
    w, h, spp = 48, 32, 4
    base = lamps_of("soup20k", 8)
    plain = expect("soup20k", "K2", w, h, spp, 1, 0, 8)
    at = int(np.flatnonzero(plain["facing"].any(1))[7])           # a hit sample that lamps face
    odd = np.zeros(12, bihrt_mod.POINT_LIGHT_DTYPE)
    odd[:3] = base[:3]
    odd[3] = base[1]                                              # a duplicate
    odd[4] = (tuple(plain["P"][at]), 1.0)                         # at a hit point
    odd[5] = ((np.nan, 0, 0), 1.0)                                # NaN: never facing
    odd[6] = ((np.inf, 0, 0), 0.25)                               # Inf: c = +-inf or NaN
    odd[7] = ((0, -np.inf, np.inf), 0.25)
    odd[8] = (tuple(base["pos"][2]), 0.0)                         # zero weight
    odd[9] = (tuple(base["pos"][0]), -0.5)                        # negative weight
    odd[10] = (tuple(base["pos"][1]), -0.0)
    odd[11] = base[5]
    exp = expect_with("soup20k", "K2", w, h, spp, 1, NO_DIR, odd)
    lit = exp["facing"] & ~exp["before"]
    assert not exp["facing"][at, 4] and exp["facing"][:, 4].any() and not exp["facing"][:, 5].any()
    assert np.array_equal(lit[:, 3], lit[:, 1]) and lit[:, 3].any()
    assert lit[:, 8].any() and lit[:, 9].any() and lit[:, 11].any()
    r = renderer(tree("soup20k"), "soup20k", "K2", w, h, spp)
    assert_lights(dev_lights(r, None, odd, 1), exp, "odd lamps")


@pytest.mark.gpu
def test_renders_undisturbed(gpu, bihrt_mod):
    """render f=0, lights f=2, render f=2, render f=3, lights f=3: every image
    is the oracle's and every plane is right."""
    w, h, spp = 48, 32, 4
    tris, ot = scene("cornell")
    cam = camera("cornell", "K1", w, h)
    g = bihrt_mod.GPUArrayManager(tris)
    r = renderer(g, "cornell", "K1", w, h, spp)
    pl = lamps_of("cornell", 3)
    f0 = r.render(0)
    d2 = r.render_lights(None, pl, 2)
    f2 = r.render(2)
    f3 = r.render(3)
    d3 = r.render_lights(None, pl, 3)
    assert r.frame == 4
    for f, img in ((0, f0), (2, f2), (3, f3)):
        assert np.array_equal(img, ot.render(w, h, spp=spp, frame=f, seed=SEED, cam=cam)[0]), f
    assert_lights(d2, expect("cornell", "K1", w, h, spp, 2, 0, 3), "frame 2")
    assert_lights(d3, expect("cornell", "K1", w, h, spp, 3, 0, 3), "frame 3")
    g.close()


@pytest.mark.gpu
def test_rebuild_ordering_and_two_streams(gpu, bihrt_mod):
    """Two calls of one tree back to back on two streams with different lamps;
    then a call on a second stream after rebuild() sees the new soup's tree."""
    import torch
    w, h, spp = 48, 32, 4
    old, new = scene("soup3k")[0], scene("soup3k2")[0]
    soup = torch.from_numpy(old.copy()).cuda()
    torch.cuda.synchronize()
    g = bihrt_mod.GPUArrayManager.from_device(soup.data_ptr(), old.shape[0])
    ea, eb = expect("soup3k", "K2", w, h, spp, 1, 0, 8), expect("soup3k", "K2", w, h, spp, 2, 2, 3)
    e1 = expect("soup3k2", "K2", w, h, spp, 1, 0, 8)
    assert not np.array_equal(ea["lit"], e1["lit"])
    r0, r1 = renderer(g, "soup3k", "K2", w, h, spp), renderer(g, "soup3k2", "K2", w, h, spp)
    da, db, dc, d1 = (DevLights(h, w, spp) for _ in range(4))
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    da.launch(r0, None, lamps_of("soup3k", 8), 1, stream=sa.cuda_stream)
    db.launch(r0, fib_lights(2), lamps_of("soup3k", 3), 2, stream=sb.cuda_stream)
    dc.launch(r0, None, lamps_of("soup3k", 8), 1, stream=sa.cuda_stream)
    sa.synchronize()
    sb.synchronize()
    g.sync()                      # (the caller's duty: the soup is not rewritten under a build or render)
    soup.copy_(torch.from_numpy(new))
    torch.cuda.synchronize()
    g.rebuild()
    d1.launch(r1, None, lamps_of("soup3k2", 8), 1, stream=sb.cuda_stream)
    sb.synchronize()
    assert_lights(da.result(), ea, "stream a")
    assert_lights(db.result(), eb, "stream b")
    assert_lights(dc.result(), ea, "stream a again")
    assert_lights(d1.result(), e1, "after the rebuild")
    g.close()


@pytest.mark.gpu
def test_c_caller(tmp_path, gpu, bihrt_mod):
    """tests/c/lights_smoke.c -- bih_build + bih_render_lights from strict C11
    (cornell, 64x48, the reference camera, a sky and lamps): render_lights' planes."""
    exe = _build_c(tmp_path)
    tris = scene("cornell")[0]
    w, h, spp = 64, 48, 4
    dl, pl = bihrt_mod.scenes.sky_dome(4), lamps_of("cornell", 3)
    sp, lp, pp, op = (tmp_path / n for n in ("scene.f32", "dir.f32", "lamps.f32", "planes.bin"))
    tris.tofile(sp)
    dl.tofile(lp)
    pl.tofile(pp)
    r = subprocess.run([exe, str(sp), str(tris.shape[0]), str(w), str(h), str(spp), "0", str(lp), str(dl.shape[0]),
                        str(pp), str(pl.shape[0]), str(op)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "lights_smoke OK" in r.stdout, r.stdout + r.stderr
    ref = bihrt_mod.Renderer(tree("cornell"), w, h, spp=spp).render_lights(dl, pl, 0)
    assert (ref["lit"] >> np.uint64(4)).any() and (ref["irradiance"] > 0).any()
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
    """python -m bihrt --direct --lamp: the PPM of render_lights' rgba plane
    under the sky and the lamps (cornell, 64x48, one frame); --sky 0: lamps only."""
    from bihrt.app import main
    want = tmp_path / "want.ppm"
    rr = bihrt_mod.Renderer(tree("cornell"), 64, 48)
    lamps = np.array([[0.0, 0.5, 0.0, 1.0], [0.3, -0.2, 0.4, 0.5]], F32)
    for sky, dl in ((["--sky", "4"], bihrt_mod.scenes.sky_dome(4)), (["--sky", "0"], None)):
        dr = tmp_path / ("d%s.ppm" % sky[1])
        assert main(["--scene", "cornell", "--width", "64", "--height", "48", "--frames", "1", "--direct", str(dr),
                     "--lamp", "0,0.5,0", "--lamp", "0.3,-0.2,0.4,0.5"] + sky) == 0
        ref = rr.render_lights(dl, lamps, 0, planes=("rgba",))["rgba"]
        bihrt_mod.write_ppm(str(want), ref)
        assert open(dr, "rb").read() == open(want, "rb").read()
        assert np.unique(bihrt_mod.unpack_rgba(ref)[..., 0]).size > 4
