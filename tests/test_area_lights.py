"""Direct lighting with area lights (bih_render_area_lights /
bih_render_area_lights_device / bih_area_light_sample, DESIGN.md section
4.5.5): parallelogram panels next to the directional and point lights of
bih_render_lights, one shadow ray per (sample, panel) to a hashed point of the
panel -- soft shadows.

Expected values come from the oracle alone, as tests/test_lights.py's, whose
`restate` this one extends: the hash is numpy uint32 (wrapping), the panel
point Q, L = Q - P, nl, c, g and the term are numpy f32 in the header's order;
a facing (sample, panel) pair is blocked when OracleTree.closest(P, L, 1e-4)
finds a triangle with t < 1.0f.  Planes are compared on bits, NaN as NaN.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import test_direct as td
import test_gbuffer as tg
import test_lights as tl
from conftest import ROOT
from test_direct import MISS_SHADE, NAMES, DevDirect, fib_lights, rows_of
from test_gbuffer import EDGE, F32, LIBDIR, SEED, camera, expected, frame_rays, normals, renderer, scene, tree
from test_lights import NO_DIR, assert_lights, lamps_of

SRC = os.path.join(ROOT, "tests", "c", "area_smoke.c")
U32 = np.uint32
W, H, SPP = 48, 32, 4


# --- the header's sample point, restated ------------------------------------------

def mix(x):
    x = np.atleast_1d(x).astype(U32)
    x = x ^ (x >> U32(16))
    x = x * U32(0x7feb352d)
    x = x ^ (x >> U32(15))
    x = x * U32(0x846ca68b)
    return x ^ (x >> U32(16))


def sample_ab(seed, gp, fs, j):
    """(a, b) f32 of area light j for global pixels gp and counters fs = frame*spp + s (u32 arrays)."""
    h = mix(U32(seed & 0xFFFFFFFF))
    h = mix(h ^ U32(seed >> 32))
    h = mix(h ^ np.asarray(gp, U32))
    h = mix(h ^ np.asarray(fs, U32))
    h = mix(h ^ U32(j))
    ha, hb = mix(h + U32(0x9E3779B9)), mix(h + U32(0x3C6EF372))
    a = (ha >> U32(8)).astype(F32) * F32(2.0 ** -24)
    b = (hb >> U32(8)).astype(F32) * F32(2.0 ** -24)
    assert a.dtype == F32 and (a >= 0).all() and (a < 1).all() and (b >= 0).all() and (b < 1).all()
    return a, b


def sample_points(panel, j, seed, gp, fs):
    """Q (n, 3) f32: (C + a*U) + b*V per component."""
    a, b = sample_ab(seed, gp, fs, j)
    Cn, U, V = (np.asarray(panel[k], F32) for k in ("corner", "edge_u", "edge_v"))
    with np.errstate(all="ignore"):
        Q = (Cn[None, :] + a[:, None] * U[None, :]) + b[:, None] * V[None, :]
    assert Q.dtype == F32
    return Q


def panel_normal(panel):
    U, V = np.asarray(panel["edge_u"], F32), np.asarray(panel["edge_v"], F32)
    with np.errstate(all="ignore"):
        return np.array([U[1] * V[2] - V[1] * U[2], U[2] * V[0] - V[2] * U[0], U[0] * V[1] - V[0] * U[1]], F32)


def restate(tris, cam, hits, d, dir_lights, lamps, panels, occluded, segment, spp, gp, frame, seed=SEED):
    """The header's lighting of samples with hit records `hits`, primary
    directions d and global pixels gp (sample i is sample i % spp of its pixel)
    under dir_lights, then lamps, then panels: lit, the pixel planes (flat), and
    per panel the masks facing / blocked / c > 0 but rejected by g <= 0."""
    import bihrt
    Ld, wd = np.ascontiguousarray(dir_lights["dir"], F32), np.ascontiguousarray(dir_lights["weight"], F32)
    Qp, wp = np.ascontiguousarray(lamps["pos"], F32), np.ascontiguousarray(lamps["weight"], F32)
    Kd, Kp, Ka, n = Ld.shape[0], Qp.shape[0], panels.shape[0], hits.shape[0]
    hit = hits["prim"] != bihrt.NO_HIT
    s = np.arange(n) % spp
    fs = ((frame * spp + s) & 0xFFFFFFFF).astype(U32)
    with np.errstate(all="ignore"):
        P = cam[0:3][None, :] + hits["t"][:, None] * d            # one multiply, then one add
        nrm = np.zeros((n, 3), F32)
        nrm[hit] = normals(tris[hits["prim"][hit]])
        cd = (nrm[:, 0:1] * Ld[None, :, 0] + nrm[:, 1:2] * Ld[None, :, 1]) + nrm[:, 2:3] * Ld[None, :, 2]
        fd = hit[:, None] & (cd > 0)
        od = np.zeros((n, Kd), bool)
        si, ki = np.nonzero(fd)
        if si.size:
            od[si, ki] = occluded(P[si], Ld[ki])
        Lp = Qp[None, :, :] - P[:, None, :]
        cp = (nrm[:, 0:1] * Lp[:, :, 0] + nrm[:, 1:2] * Lp[:, :, 1]) + nrm[:, 2:3] * Lp[:, :, 2]
        r2p = (Lp[:, :, 0] * Lp[:, :, 0] + Lp[:, :, 1] * Lp[:, :, 1]) + Lp[:, :, 2] * Lp[:, :, 2]
        termp = (wp[None, :] * (cp / np.sqrt(r2p))) / r2p
        fp = hit[:, None] & (cp > 0)
        bp = np.zeros((n, Kp), bool)
        si, ki = np.nonzero(fp)
        if si.size:
            bp[si, ki] = segment(P[si], Lp[si, ki])[0]
        # the panels
        La = np.zeros((n, Ka, 3), F32)
        ca, ga, terma = np.zeros((n, Ka), F32), np.zeros((n, Ka), F32), np.zeros((n, Ka), F32)
        for j in range(Ka):
            Q = sample_points(panels[j], j, seed, gp, fs)
            L = Q - P
            nl = panel_normal(panels[j])
            c = (nrm[:, 0] * L[:, 0] + nrm[:, 1] * L[:, 1]) + nrm[:, 2] * L[:, 2]
            g = -((nl[0] * L[:, 0] + nl[1] * L[:, 1]) + nl[2] * L[:, 2])
            r2 = (L[:, 0] * L[:, 0] + L[:, 1] * L[:, 1]) + L[:, 2] * L[:, 2]
            ln = np.sqrt(r2)
            term = ((F32(panels[j]["weight"]) * (c / ln)) * (g / ln)) / r2
            assert L.dtype == F32 and c.dtype == F32 and g.dtype == F32 and term.dtype == F32 and ln.dtype == F32
            La[:, j], ca[:, j], ga[:, j], terma[:, j] = L, c, g, term
        facing = hit[:, None] & (ca > 0) & (ga > 0)
        reject = hit[:, None] & (ca > 0) & ~(ga > 0)
        blocked = np.zeros((n, Ka), bool)
        si, ki = np.nonzero(facing)
        if si.size:
            blocked[si, ki] = segment(P[si], La[si, ki])[0]
        lit = np.zeros(n, np.uint64)
        e = np.zeros(n, F32)
        for k in range(Kd):                                       # ascending over the lit bits
            on = fd[:, k] & ~od[:, k]
            lit |= on.astype(np.uint64) << np.uint64(k)
            e = np.where(on, e + wd[k] * cd[:, k], e)
        for i in range(Kp):
            on = fp[:, i] & ~bp[:, i]
            lit |= on.astype(np.uint64) << np.uint64(Kd + i)
            e = np.where(on, e + termp[:, i], e)
        for j in range(Ka):
            on = facing[:, j] & ~blocked[:, j]
            lit |= on.astype(np.uint64) << np.uint64(Kd + Kp + j)
            e = np.where(on, e + terma[:, j], e)
        e = e.reshape(-1, spp)
        acc = e[:, 0]
        for k in range(1, spp):
            acc = acc + e[:, k]
        E = acc / F32(spp)
        assert E.dtype == F32 and P.dtype == F32
        g8 = np.fmax(F32(0), np.fmin(F32(255), F32(255) * E)).astype(np.int32).astype(np.uint32)
    rgba = np.where(hit.reshape(-1, spp).any(1), g8 | (g8 << 8) | (g8 << 16), np.uint32(MISS_SHADE)).astype(np.uint32)
    out = {"lit": lit, "irradiance": E, "rgba": rgba, "hit": hit, "facing": facing, "blocked": blocked,
           "reject": reject, "P": P, "L": La}
    for a in out.values():
        a.setflags(write=False)
    return out


def none_of(dtype):
    return np.zeros(0, dtype)


def expect_with(name, kname, w, h, spp, frame, dir_lights, lamps, panels, segment=None):
    import bihrt
    tris, ot = scene(name)
    cam = camera(name, kname, w, h)
    d = frame_rays(cam, w, h, spp, frame).reshape(-1, 3)
    gp = (np.arange(w * h * spp) // spp).astype(U32)             # whole frame: local pixel = y*w + x
    return restate(tris, cam, expected(name, kname, w, h, spp, frame)["hits"], d,
                   dir_lights if dir_lights is not None else NO_DIR,
                   lamps if lamps is not None else none_of(bihrt.POINT_LIGHT_DTYPE),
                   bihrt.pack_area_lights(panels), td.oracle_occluded(ot), segment or tl.oracle_segment(ot),
                   spp, gp, frame)


def panels_of(name):
    import bihrt
    if name == "cornell":
        return bihrt.scenes.cornell_panel()
    ot = scene(name)[1]
    return bihrt.scenes.panels(ot.scene_lo, ot.scene_hi)


@functools.lru_cache(maxsize=None)
def expect(name, kname, w, h, spp, frame, Kd=0, Kp=0):
    """The oracle's lighting of the whole frame under fib_lights(Kd), lamps(scene
    box, Kp) and panels_of(name); read-only, computed once."""
    return expect_with(name, kname, w, h, spp, frame, fib_lights(Kd) if Kd else None,
                       lamps_of(name, Kp) if Kp else None, panels_of(name))


def penumbra(exp, j, spp):
    """Pixels where some but not all facing samples of panel j are lit."""
    f = exp["facing"][:, j].reshape(-1, spp)
    on = (exp["facing"][:, j] & ~exp["blocked"][:, j]).reshape(-1, spp)
    return int(((on.sum(1) > 0) & (on.sum(1) < f.sum(1))).sum())


def figures(exp, spp):
    """Per panel (blocked share of facing pairs, penumbra pixels, emitter-side rejects)."""
    return [(float(exp["blocked"][:, j].sum() / max(int(exp["facing"][:, j].sum()), 1)), penumbra(exp, j, spp),
             int(exp["reject"][:, j].sum())) for j in range(exp["facing"].shape[1])]


def soft_classes(exp, spp, what):
    """A frame that degenerates must fail, not pass vacuously."""
    hs = float(exp["hit"].mean())
    assert 0.10 <= hs <= 0.90, f"{what}: hit share {hs:.3f}"
    for j, (b, pen, rej) in enumerate(figures(exp, spp)):
        assert 0.10 <= b <= 0.90, f"{what} panel {j}: blocked share {b:.3f}"
        assert pen >= 8, f"{what} panel {j}: {pen} penumbra pixels"
        assert rej >= 16, f"{what} panel {j}: {rej} emitter-side rejects"


class DevArea(DevDirect):
    def launch(self, r, dir_lights, lamps, panels, frame, rows=None, stream=None):
        r.render_area_lights_device({k: self.t[k].data_ptr() for k in self.names}, dir_lights, lamps, panels, frame,
                                    rows, stream)


def dev_area(r, dir_lights, lamps, panels, frame, rows=None, names=NAMES):
    nrows = rows.nrows if rows is not None else r.h
    dv = DevArea(nrows, r.w, r.spp, names)
    dv.launch(r, dir_lights, lamps, panels, frame, rows)
    r.sync()
    return dv.result()


@pytest.fixture(scope="module", autouse=True)
def _free_trees():
    yield
    while tg._trees:
        tg._trees.popitem()[1].close()


# --- CPU ------------------------------------------------------------------------

def test_struct_layout(bihrt_mod):
    A, S = bihrt_mod.AreaLight, bihrt_mod.LightSet
    assert C.sizeof(A) == 48
    assert [getattr(A, f).offset for f in ("corner", "weight", "edge_u", "reserved0", "edge_v", "reserved1")] == \
        [0, 12, 16, 28, 32, 44]
    p = C.sizeof(C.c_void_p)
    assert [getattr(S, f).offset for f in ("dir", "n_dir", "point", "n_point", "area", "n_area")] == \
        [0, p, 2 * p, 3 * p, 4 * p, 5 * p] and C.sizeof(S) == 6 * p
    dt = bihrt_mod.AREA_LIGHT_DTYPE
    assert dt.itemsize == 48
    assert [dt.fields[f][1] for f in ("corner", "weight", "edge_u", "reserved0", "edge_v", "reserved1")] == \
        [0, 12, 16, 28, 32, 44]
    packed = bihrt_mod.pack_area_lights([[1, 2, 3, 4, 5, 6, 7, 8, 9, 10], [0] * 9 + [2]])
    assert packed.dtype == dt and packed.shape == (2,) and packed["weight"].tolist() == [10, 2]
    assert packed["corner"][0].tolist() == [1, 2, 3] and packed["edge_u"][0].tolist() == [4, 5, 6]
    assert packed["edge_v"][0].tolist() == [7, 8, 9] and (packed["reserved0"] == 0).all()
    assert bihrt_mod.pack_area_lights(packed).tobytes() == packed.tobytes()
    assert bihrt_mod.pack_area_lights(packed[0]).shape == (1,)
    assert bihrt_mod.MAX_AREA_LIGHTS == 16


def test_header_symbols_exported(bihrt_mod):
    names = bihrt_mod._lib.exported_symbols_from_header()
    L = bihrt_mod._lib.load()
    for sym in ("bih_render_area_lights", "bih_render_area_lights_device", "bih_area_light_sample"):
        assert sym in names and getattr(L, sym) is not None, sym
    hdr = open(os.path.join(ROOT, "include", "bih.h")).read()
    assert "#define BIH_ABI_VERSION 4" in hdr and "#define BIH_MAX_AREA_LIGHTS 16" in hdr
    assert "typedef struct bih_area_light" in hdr and "typedef struct bih_light_set" in hdr
    assert L.bih_abi_version() == 4


def test_sample_equals_the_hash(bihrt_mod):
    """bih_area_light_sample is the header's hash and Q on bits: 4096 draws of
    (seed, pixel, frame, spp, s, j), seeds with high bits set and frame*spp
    products that wrap among them."""
    L = bihrt_mod._lib.load()
    rng = np.random.default_rng(5)
    panels = np.zeros(4, bihrt_mod.AREA_LIGHT_DTYPE)
    panels[0] = bihrt_mod.scenes.cornell_panel()[0]
    panels[1] = bihrt_mod.scenes.panels([-1.0, 0.0, 2.0], [3.0, 1.0, 4.0])[1]
    panels[2] = ((1e3, -2e-3, 7.25), 1.0, (0.3, 0.7, -0.1), 0.0, (-5.0, 0.125, 9.0), 0.0)
    panels[3] = ((0.1, 0.2, 0.3), 1.0, (1e-8, 1e8, 3.0), 0.0, (np.inf, 1.0, np.nan), 0.0)
    seeds = [1984, 0, 0xFFFFFFFFFFFFFFFF, 0x8000000000000001, 0xDEADBEEF00000000, 0x123456789ABCDEF0]
    n, q = 4096, (C.c_float * 3)()
    wraps = 0
    for k in range(n):
        seed = seeds[k % len(seeds)]
        spp = int(rng.integers(1, 65))
        frame = int(rng.integers(0, 1 << 32)) if k % 3 else int(rng.integers(0, 8))
        s, j, pix = int(rng.integers(0, spp)), int(rng.integers(0, 16)), int(rng.integers(0, 1 << 32))
        if k % 64 == 0:
            pix = 0xFFFFFFFF
        wraps += frame * spp + s >= 1 << 32
        lt = panels[k % 4:k % 4 + 1]
        assert L.bih_area_light_sample(C.c_void_p(lt.ctypes.data), j, seed, pix, frame, spp, s, q) == 0
        fs = (frame * spp + s) & 0xFFFFFFFF
        want = sample_points(lt[0], j, seed, np.array([pix], U32), np.array([fs], U32))[0]
        got = np.array(q[:], F32)
        assert tl.canon(got).tolist() == tl.canon(want).tolist(), (k, seed, pix, frame, spp, s, j)
    assert wraps > 1000
    # the Python mirror, and the point lies on the panel
    got = bihrt_mod.area_light_sample(panels[0], 3, 1984, 77, 1, 4, 2)
    a, b = sample_ab(1984, np.array([77], U32), np.array([6], U32), 3)
    assert got.dtype == F32 and got.tolist() == [F32(0.1) + a[0] * F32(0.6), F32(0.98), F32(1.0) + b[0] * F32(0.6)]
    assert bihrt_mod.area_light_sample(panels[0], 3, 1984, 77, 1, 4, 3).tolist() != got.tolist()
    # errors
    lt = panels[:1]
    ptr = C.c_void_p(lt.ctypes.data)
    assert L.bih_area_light_sample(None, 0, 1, 0, 0, 4, 0, q) == -1
    assert L.bih_area_light_sample(ptr, 0, 1, 0, 0, 4, 0, None) == -1
    assert L.bih_area_light_sample(ptr, 0, 1, 0, 0, 0, 0, q) == -1
    assert L.bih_area_light_sample(ptr, 0, 1, 0, 0, 4, 4, q) == -1
    assert L.bih_area_light_sample(ptr, 0, 1, 0, 0, 4, 3, q) == 0
    with pytest.raises(bihrt_mod.BihError):
        bihrt_mod.area_light_sample(panels[0], 0, 1, 0, 0, 4, 4)


def test_device_free_error_codes(bihrt_mod):
    """The argument checks come, in the header's order, before the tree or a
    device is touched: a stand-in tree pointer is never dereferenced."""
    L = bihrt_mod._lib.load()
    INVALID, TOO_LARGE = -1, -6
    raw = (C.c_char * 96)()
    base = (C.addressof(raw) + 15) & ~15
    fake = C.c_void_p(base)
    cam = bihrt_mod.Camera()
    D, R, S = bihrt_mod.Direct, bihrt_mod.Rows, bihrt_mod.LightSet
    sun = (bihrt_mod.Light * 1)()
    sun[0].dir[1], sun[0].weight = 1.0, 1.0
    lamp = (bihrt_mod.PointLight * 1)()
    lamp[0].pos[1], lamp[0].weight = 1.0, 1.0
    pan = (bihrt_mod.AreaLight * 1)()
    pan[0].edge_u[0], pan[0].edge_v[2], pan[0].weight = 1.0, 1.0, 1.0
    ps, pl, pp = (C.cast(x, C.c_void_p) for x in (sun, lamp, pan))

    def ls(d, kd, p, kp, a, ka):
        return S(d, kd, p, kp, a, ka)
    full = ls(ps, 1, pl, 1, pp, 1)
    rgba, lit, none = D(rgba=base), D(lit=base), D()
    odd = D(lit=base + 4, rgba=base)
    for entry in (lambda *a: L.bih_render_area_lights_device(*a, None), L.bih_render_area_lights):
        def call(t, c, w, h, spp, rows, s, d):
            return entry(t, C.byref(c) if c is not None else None, w, h, spp, 0, SEED,
                         C.byref(rows) if rows is not None else None,
                         C.byref(s) if s is not None else None, C.byref(d) if d is not None else None)
        # 1: the G-buffer's checks, in its order
        assert call(None, cam, 8, 8, 4, None, full, rgba) == INVALID
        assert call(fake, None, 8, 8, 4, None, full, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, None, full, None) == INVALID
        assert call(fake, cam, 8, 8, 65, None, full, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, None, full, none) == INVALID              # all planes NULL
        assert call(fake, cam, 8, 8, 4, R(6, 4, 4, 1), full, rgba) == INVALID
        assert call(fake, cam, 1 << 16, 1 << 16, 1, None, None, odd) == TOO_LARGE   # (before 2 and 3)
        # 2: the lights
        assert call(fake, cam, 8, 8, 4, None, None, rgba) == INVALID               # lights == NULL
        assert call(fake, cam, 8, 8, 4, None, ls(None, 0, None, 0, None, 0), rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, None, ls(ps, 0, pl, 0, pp, 0), rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, None, ls(ps, 33, pl, 31, pp, 1), rgba) == INVALID   # 65 together
        assert call(fake, cam, 8, 8, 4, None, ls(ps, 0xFFFFFFFF, pl, 1, pp, 1), rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, None, ls(ps, 1, pl, 1, pp, 17), rgba) == INVALID    # n_area > 16
        assert call(fake, cam, 8, 8, 4, None, ls(None, 0, None, 0, pp, 17), rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, None, ls(None, 1, pl, 1, pp, 1), rgba) == INVALID   # NULL with a count
        assert call(fake, cam, 8, 8, 4, None, ls(ps, 1, None, 1, pp, 1), rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, None, ls(ps, 1, pl, 1, None, 1), rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), None, rgba) == INVALID      # (before nrows == 0)
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), ls(None, 0, None, 0, None, 1), rgba) == INVALID
        # 3: lit's alignment
        assert call(fake, cam, 8, 8, 4, None, full, odd) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), ls(None, 0, None, 0, pp, 1), odd) == INVALID
        # 4: nothing to do
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, lit) == 0
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), ls(None, 0, None, 0, pp, 1), rgba) == 0
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), ls(ps, 1, None, 0, None, 0), rgba) == 0
        assert call(fake, cam, 8, 8, 64, R(3, 0, 0, 0), ls(ps, 46, pl, 2, pp, 16), rgba) == 0


def test_panels(bihrt_mod):
    """scenes.panels: two panels of 0.6 x 0.6 of the box's x-z extent, 0.2 hy
    above the centre facing down and below it facing up; f64 rounded to f32."""
    lo, hi = np.array([-1.0, 0.0, 2.0]), np.array([3.0, 1.0, 4.0])
    c, h = np.array([1.0, 0.5, 3.0]), np.array([2.0, 0.5, 1.0])
    p = bihrt_mod.scenes.panels(lo, hi)
    assert p.dtype == bihrt_mod.AREA_LIGHT_DTYPE and p.shape == (2,)
    assert p.tobytes() == bihrt_mod.scenes.panels(lo.astype(F32), hi.astype(F32)).tobytes()
    eu, ev = np.array([0.6 * h[0], 0, 0]), np.array([0, 0, 0.6 * h[2]])
    assert np.array_equal(p["corner"][0], (c - [0.3 * h[0], -0.2 * h[1], 0.3 * h[2]]).astype(F32))
    assert np.array_equal(p["corner"][1], (c - [0.3 * h[0], 0.2 * h[1], 0.3 * h[2]]).astype(F32))
    assert np.array_equal(p["edge_u"][0], eu.astype(F32)) and np.array_equal(p["edge_v"][0], ev.astype(F32))
    assert np.array_equal(p["edge_u"][1], ev.astype(F32)) and np.array_equal(p["edge_v"][1], eu.astype(F32))
    assert panel_normal(p[0])[1] < 0 and panel_normal(p[1])[1] > 0      # down, up
    assert not panel_normal(p[0])[[0, 2]].any() and not panel_normal(p[1])[[0, 2]].any()
    assert (p["weight"] > 0).all() and p["weight"][0] == p["weight"][1]
    assert (bihrt_mod.scenes.panels(lo, hi, weight=0.5)["weight"] == 0.5).all()
    assert (p["reserved0"] == 0).all() and (p["reserved1"] == 0).all()
    q = bihrt_mod.scenes.cornell_panel()
    assert q.dtype == bihrt_mod.AREA_LIGHT_DTYPE and q.shape == (1,)
    assert q["corner"][0].tolist() == [F32(0.1), F32(0.98), F32(1.0)]
    assert q["edge_u"][0].tolist() == [F32(0.6), 0, 0] and q["edge_v"][0].tolist() == [0, 0, F32(0.6)]
    assert panel_normal(q[0])[1] < 0
    # the lamp quad's outline, one centimetre below it
    lamp = bihrt_mod.scenes.cornell()[-2:].reshape(-1, 3)
    assert lamp[:, 0].min() == F32(0.1) and lamp[:, 0].max() == F32(0.7) and lamp[:, 2].min() == F32(1.0)
    assert lamp[:, 2].max() == F32(1.6) and np.allclose(lamp[:, 1] - q["corner"][0][1], 0.01, atol=1e-6)


def test_app_panel_options(bihrt_mod):
    """--panel without --direct, a malformed panel, more than 16 panels and
    more than 64 lights are errors, before any device is used."""
    from bihrt.app import main
    base = ["--scene", "cornell", "--frames", "1"]
    ok = "0.1,0.98,1,0.6,0,0,0,0,0.6"
    for extra in (["--panel", ok],
                  ["--direct", "d.ppm", "--panel", "0,1,0"],
                  ["--direct", "d.ppm", "--panel", ok + ",x"],
                  ["--direct", "d.ppm", "--panel", ok + ",1,2"],
                  ["--direct", "d.ppm", "--panel", ok[:-4]],
                  ["--direct", "d.ppm", "--sky", "1"] + ["--panel", ok] * 17,
                  ["--direct", "d.ppm", "--sky", "64", "--panel", ok],
                  ["--direct", "d.ppm", "--sky", "61", "--sun", "0,1,0", "--lamp", "0,1,0", "--panel", ok,
                   "--panel", ok + ",2"]):
        with pytest.raises(SystemExit):
            main(base + extra)


def _build_c(tmp_path) -> str:
    exe = str(tmp_path / "area_smoke")
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
    assert "FAIL" not in r.stdout and r.stdout.count("ok ") == 17, r.stdout


def test_header_is_cxx17(tmp_path):
    src = tmp_path / "hdr.cpp"
    src.write_text('#include "bih.h"\nstatic_assert(sizeof(bih_area_light) == 48, "");\n'
                   "int main() { bih_area_light a{}; bih_light_set s{}; s.area = &a; s.n_area = 1;\n"
                   "  float q[3]; return bih_area_light_sample(s.area, 0, 1, 0, 0, 1, 0, q) == BIH_OK ? 0 : 1; }\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only",
                    "-I", os.path.join(ROOT, "include"), str(src)], check=True)


# --- GPU ------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name,kname", [("soup20k", "K2"), ("soup3k", "K2"), ("cornell", "K1")])
def test_classes(name, kname, gpu, bihrt_mod):
    """The two panels of the scene box (cornell: its ceiling lamp) at 48x32x4:
    blocked and open pairs, penumbra pixels and emitter-side rejects are all
    there; the planes on bits.  soup20k once more with two stack slots on chip."""
    exp = expect(name, kname, W, H, SPP, 1)
    print(name, "hit share %.3f" % exp["hit"].mean(), "(blocked share, penumbra pixels, rejects):", figures(exp, SPP))
    if name == "cornell":
        assert penumbra(exp, 0, SPP) >= 16 and exp["blocked"].any()
    else:
        soft_classes(exp, SPP, name)
    g = tree(name)
    r = renderer(g, name, kname, W, H, SPP)
    assert_lights(dev_area(r, None, None, panels_of(name), 1), exp, f"{name} {kname}")
    if name == "soup20k":
        g.set_param(bihrt_mod.PARAM_TRACE_LDS_SLOTS, 2)
        try:
            assert_lights(dev_area(r, None, None, panels_of(name), 1), exp, "2 slots")
        finally:
            g.set_param(bihrt_mod.PARAM_TRACE_LDS_SLOTS, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE)
def test_edge_scenes(name, gpu, bihrt_mod):
    """Every edge scene under K2 with the panels of its box, bits only."""
    exp = expect(name, "K2", W, H, SPP, 1)
    assert exp["hit"].any()
    r = renderer(tree(name), name, "K2", W, H, SPP)
    assert_lights(dev_area(r, None, None, panels_of(name), 1), exp, name)


@pytest.mark.gpu
def test_mixed_lights(gpu, bihrt_mod):
    """3 directional + 2 point + 2 area lights: the low 5 bits are
    bih_render_lights' under the first five, the top 2 the panels' alone; the
    sum runs over all in bit order; n_area = 0 is bih_render_lights byte for byte."""
    exp = expect("soup20k", "K2", W, H, SPP, 1, 3, 2)
    assert (exp["lit"] & np.uint64(7)).any() and ((exp["lit"] >> np.uint64(3)) & np.uint64(3)).any()
    assert (exp["lit"] >> np.uint64(5)).any() and not (exp["lit"] >> np.uint64(7)).any()
    r = renderer(tree("soup20k"), "soup20k", "K2", W, H, SPP)
    dl, pl, al = fib_lights(3), lamps_of("soup20k", 2), panels_of("soup20k")
    got = dev_area(r, dl, pl, al, 1)
    assert_lights(got, exp, "3 + 2 + 2")
    five = tl.dev_lights(r, dl, pl, 1)
    only_area = dev_area(r, None, None, al, 1)
    assert_lights(only_area, expect("soup20k", "K2", W, H, SPP, 1), "area alone")
    assert np.array_equal(got["lit"] & np.uint64(0x1F), five["lit"])
    assert np.array_equal(got["lit"] >> np.uint64(5), only_area["lit"])
    no_area = dev_area(r, dl, pl, None, 1)
    for name in NAMES:
        assert no_area[name].tobytes() == five[name].tobytes(), name
    assert (no_area["irradiance"] != got["irradiance"]).any()
    only_dir = dev_area(r, dl, None, None, 1)
    assert only_dir["lit"].tobytes() == td.dev_direct(r, dl, 1)["lit"].tobytes()


@pytest.mark.gpu
def test_bit_63(gpu, bihrt_mod):
    """46 + 2 + 16 lights at 16x8x16: the last panel is bit 63."""
    w, h, spp = 16, 8, 16
    two = panels_of("soup20k")
    al = np.zeros(16, bihrt_mod.AREA_LIGHT_DTYPE)
    for j in range(16):
        al[j] = two[j % 2]
        al[j]["corner"][1] += F32(0.01 * (j // 2))
    dl, pl = fib_lights(46), lamps_of("soup20k", 2)
    exp = expect_with("soup20k", "K1", w, h, spp, 1, dl, pl, al)
    assert (exp["lit"] >> np.uint64(63)).any() and (exp["lit"] & np.uint64(0xFFFFFFFF)).any()
    assert ((exp["lit"] >> np.uint64(48)) & np.uint64(0x7FFF)).any()
    r = renderer(tree("soup20k"), "soup20k", "K1", w, h, spp)
    assert_lights(dev_area(r, dl, pl, al, 1), exp, "46 + 2 + 16")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,spp", [(1, 1, 1), (37, 29, 3), (8, 8, 64), (16, 8, 16)])
def test_shapes(w, h, spp, gpu, bihrt_mod):
    """One sample; partial tiles and waves with an spp that is no power of two; a pixel per wave; four pixels per wave."""
    exp = expect("soup20k", "K2", w, h, spp, 1, 1, 1)
    if (w, h) != (1, 1):
        assert exp["hit"].any() and exp["facing"].any() and exp["blocked"].any() and (exp["lit"] >> np.uint64(2)).any()
    r = renderer(tree("soup20k"), "soup20k", "K2", w, h, spp)
    assert_lights(dev_area(r, fib_lights(1), lamps_of("soup20k", 1), panels_of("soup20k"), 1), exp, f"{w}x{h}x{spp}")


@pytest.mark.gpu
def test_rows_bands_planes_and_host_entry(gpu, bihrt_mod):
    """Interleaved bands and rows that are not tile-aligned equal the same rows
    of the full frame, through both entries (the hash takes the GLOBAL pixel);
    each plane alone gives the bits of all together and leaves the others
    untouched; no call after the first of the shape allocates."""
    exp = expect("soup20k", "K2", W, H, SPP, 1, 3, 2)
    g = tree("soup20k")
    r = renderer(g, "soup20k", "K2", W, H, SPP)
    dl, pl, al = fib_lights(3), lamps_of("soup20k", 2), panels_of("soup20k")
    host = r.render_area_lights(dl, pl, al, 1)
    assert sorted(host) == sorted(NAMES) and host["lit"].shape == (W * H * SPP,) and host["rgba"].shape == (H, W)
    assert_lights(host, exp, "host entry")
    assert_lights(host, dev_area(r, dl, pl, al, 1, names=("irradiance",)), "own lit words", names=("irradiance",))
    first = g.info()
    for rows, ys in ((bihrt_mod.Rows(4, 8, 4, 2), [4, 5, 6, 7, 12, 13, 14, 15]),
                     (bihrt_mod.Rows(5, 7, 7, 1), list(range(5, 12)))):
        sub = rows_of(exp, W, SPP, ys)
        assert ((sub["lit"] >> np.uint64(5)) != 0).any() and (sub["lit"] == 0).any()
        assert_lights(dev_area(r, dl, pl, al, 1, rows), sub, f"rows {ys[0]}..")
        assert_lights(r.render_area_lights(dl, pl, al, 1, rows), sub, "host entry rows")
    for name in NAMES:
        got = dev_area(r, dl, pl, al, 1, names=(name,))
        assert_lights(got, exp, f"{name} alone", names=(name,))
        for other in NAMES:
            if other != name:
                assert (np.ascontiguousarray(got[other]).view(np.uint8) == 0xAB).all(), (name, other)
    after = g.info()
    assert after.device_allocs == first.device_allocs and after.device_bytes == first.device_bytes


@pytest.mark.gpu
def test_frames(gpu, bihrt_mod):
    """Frames 1 and 2 use other panel points (and other primary rays): each is the oracle's."""
    e1, e2 = expect("soup3k", "K2", W, H, SPP, 1), expect("soup3k", "K2", W, H, SPP, 2)
    assert not np.array_equal(e1["lit"], e2["lit"])
    r = renderer(tree("soup3k"), "soup3k", "K2", W, H, SPP)
    al = panels_of("soup3k")
    assert_lights(dev_area(r, None, None, al, 1), e1, "frame 1")
    assert_lights(dev_area(r, None, None, al, 2), e2, "frame 2")
    assert_lights(dev_area(r, None, None, al, 1), e1, "frame 1 again")


@pytest.mark.gpu
def test_matches_trace_device(gpu, bihrt_mod):
    """Composition: `lit` equals bih_trace_device(OCCLUDED_WITHIN, t_hi = 1) on
    the restated rays, GPU against GPU, and both equal the oracle."""
    exp = expect("soup3k", "K2", W, H, SPP, 1)
    soft_classes(exp, SPP, "soup3k")
    g = tree("soup3k")
    traced = expect_with("soup3k", "K2", W, H, SPP, 1, None, None, panels_of("soup3k"), tl.gpu_segment(g))
    assert np.array_equal(traced["blocked"], exp["blocked"])
    got = dev_area(renderer(g, "soup3k", "K2", W, H, SPP), None, None, panels_of("soup3k"), 1)
    assert_lights(got, traced, "area vs trace")
    assert_lights(got, exp, "area vs oracle")


@pytest.mark.gpu
def test_odd_panels(gpu, bihrt_mod):
    """Zero-area and degenerate panels, NaN and Inf corners, zero and negative
    weights, a duplicate, a panel whose corner is a hit point, and a panel seen
    only from behind (no bit is ever set for it)."""
    two = panels_of("soup20k")
    plain = expect("soup20k", "K2", W, H, SPP, 1)
    ot = scene("soup20k")[1]
    at = int(np.flatnonzero(plain["facing"].any(1))[7])           # a hit sample that a panel faces
    odd = np.zeros(12, bihrt_mod.AREA_LIGHT_DTYPE)
    odd[0], odd[1] = two[0], two[1]
    odd[2] = two[0]                                               # a duplicate (its hash differs: j = 2)
    odd[3] = two[0]
    odd[3]["edge_u"] = 0                                          # zero area: nl = 0
    odd[4] = two[1]
    odd[4]["edge_v"] = 2 * odd[4]["edge_u"]                       # U parallel to V: nl = 0
    odd[5] = two[0]
    odd[5]["corner"] = (np.nan, 0, 0)                             # NaN: never facing
    odd[6] = two[1]
    odd[6]["corner"] = (0, -np.inf, 0)                            # Inf
    odd[7] = two[0]
    odd[7]["weight"] = 0.0
    odd[8] = two[1]
    odd[8]["weight"] = -0.5
    odd[9] = two[0]
    odd[9]["corner"] = plain["P"][at]                             # a corner at a hit point
    hi_y = float(ot.scene_hi[1]) + 1.0
    odd[10] = two[1]                                              # above everything, facing up: seen from behind
    odd[10]["corner"][1] = hi_y
    odd[11] = two[1]
    exp = expect_with("soup20k", "K2", W, H, SPP, 1, None, None, odd)
    lit = exp["facing"] & ~exp["blocked"]
    for j in (3, 4, 5, 10):
        assert not exp["facing"][:, j].any() and not ((exp["lit"] >> np.uint64(j)) & np.uint64(1)).any(), j
    assert exp["reject"][:, 10].sum() >= 16
    assert lit[:, 2].any() and not np.array_equal(lit[:, 2], lit[:, 0])
    assert lit[:, 7].any() and lit[:, 8].any() and lit[:, 9].any() and lit[:, 11].any()
    r = renderer(tree("soup20k"), "soup20k", "K2", W, H, SPP)
    got = dev_area(r, None, None, odd, 1)
    assert_lights(got, exp, "odd panels")
    for j in (3, 4, 5, 10):
        assert not ((got["lit"] >> np.uint64(j)) & np.uint64(1)).any(), j


@pytest.mark.gpu
def test_renders_undisturbed(gpu, bihrt_mod):
    """render f=0, area f=2, render f=2, render f=3, area f=3: every image is
    the oracle's and every plane is right (the panel points take no XORWOW draw)."""
    tris, ot = scene("cornell")
    cam = camera("cornell", "K1", W, H)
    g = bihrt_mod.GPUArrayManager(tris)
    r = renderer(g, "cornell", "K1", W, H, SPP)
    al = panels_of("cornell")
    f0 = r.render(0)
    d2 = r.render_area_lights(None, None, al, 2)
    f2 = r.render(2)
    f3 = r.render(3)
    d3 = r.render_area_lights(None, None, al, 3)
    assert r.frame == 4
    for f, img in ((0, f0), (2, f2), (3, f3)):
        assert np.array_equal(img, ot.render(W, H, spp=SPP, frame=f, seed=SEED, cam=cam)[0]), f
    assert_lights(d2, expect("cornell", "K1", W, H, SPP, 2), "frame 2")
    assert_lights(d3, expect("cornell", "K1", W, H, SPP, 3), "frame 3")
    g.close()


@pytest.mark.gpu
def test_rebuild_ordering_and_two_streams(gpu, bihrt_mod):
    """Two calls of one tree back to back on two streams with different lights;
    then a call on a second stream after rebuild() sees the new soup's tree."""
    import torch
    old, new = scene("soup3k")[0], scene("soup3k2")[0]
    soup = torch.from_numpy(old.copy()).cuda()
    torch.cuda.synchronize()
    g = bihrt_mod.GPUArrayManager.from_device(soup.data_ptr(), old.shape[0])
    ea, eb = expect("soup3k", "K2", W, H, SPP, 1), expect("soup3k", "K2", W, H, SPP, 2, 1, 1)
    e1 = expect("soup3k2", "K2", W, H, SPP, 1)
    assert not np.array_equal(ea["lit"], e1["lit"])
    r0, r1 = renderer(g, "soup3k", "K2", W, H, SPP), renderer(g, "soup3k2", "K2", W, H, SPP)
    da, db, dc, d1 = (DevArea(H, W, SPP) for _ in range(4))
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    da.launch(r0, None, None, panels_of("soup3k"), 1, stream=sa.cuda_stream)
    db.launch(r0, fib_lights(1), lamps_of("soup3k", 1), panels_of("soup3k"), 2, stream=sb.cuda_stream)
    dc.launch(r0, None, None, panels_of("soup3k"), 1, stream=sa.cuda_stream)
    sa.synchronize()
    sb.synchronize()
    g.sync()                      # (the caller's duty: the soup is not rewritten under a build or render)
    soup.copy_(torch.from_numpy(new))
    torch.cuda.synchronize()
    g.rebuild()
    d1.launch(r1, None, None, panels_of("soup3k2"), 1, stream=sb.cuda_stream)
    sb.synchronize()
    assert_lights(da.result(), ea, "stream a")
    assert_lights(db.result(), eb, "stream b")
    assert_lights(dc.result(), ea, "stream a again")
    assert_lights(d1.result(), e1, "after the rebuild")
    g.close()


@pytest.mark.gpu
def test_c_caller(tmp_path, gpu, bihrt_mod):
    """tests/c/area_smoke.c -- bih_build + bih_render_area_lights from strict
    C11 (cornell, 64x48, the reference camera, a sky, lamps and the ceiling
    panel): render_area_lights' planes."""
    exe = _build_c(tmp_path)
    tris = scene("cornell")[0]
    w, h, spp = 64, 48, 4
    dl, pl, al = bihrt_mod.scenes.sky_dome(2), lamps_of("cornell", 2), bihrt_mod.scenes.cornell_panel(4.0)
    sp, lp, pp, ap, op = (tmp_path / n for n in ("scene.f32", "dir.f32", "lamps.f32", "area.f32", "planes.bin"))
    tris.tofile(sp)
    dl.tofile(lp)
    pl.tofile(pp)
    al.tofile(ap)
    r = subprocess.run([exe, str(sp), str(tris.shape[0]), str(w), str(h), str(spp), "0", str(lp), str(dl.shape[0]),
                        str(pp), str(pl.shape[0]), str(ap), str(al.shape[0]), str(op)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "area_smoke OK" in r.stdout, r.stdout + r.stderr
    ref = bihrt_mod.Renderer(tree("cornell"), w, h, spp=spp).render_area_lights(dl, pl, al, 0)
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
    """python -m bihrt --direct --panel: the PPM of render_area_lights' rgba
    plane under the sky, a lamp and the panel (cornell, 64x48, one frame);
    --sky 0: the panel only."""
    from bihrt.app import main
    want = tmp_path / "want.ppm"
    rr = bihrt_mod.Renderer(tree("cornell"), 64, 48)
    panel = np.array([[0.1, 0.98, 1.0, 0.6, 0, 0, 0, 0, 0.6, 4.0]], F32)
    lamp = np.array([[0.0, 0.5, 0.0, 1.0]], F32)
    for sky, dl, lamps in ((["--sky", "4", "--lamp", "0,0.5,0"], bihrt_mod.scenes.sky_dome(4), lamp),
                           (["--sky", "0"], None, None)):
        dr = tmp_path / ("d%s.ppm" % sky[1])
        assert main(["--scene", "cornell", "--width", "64", "--height", "48", "--frames", "1", "--direct", str(dr),
                     "--panel", "0.1,0.98,1,0.6,0,0,0,0,0.6,4"] + sky) == 0
        ref = rr.render_area_lights(dl, lamps, panel, 0, planes=("rgba",))["rgba"]
        bihrt_mod.write_ppm(str(want), ref)
        assert open(dr, "rb").read() == open(want, "rb").read()
        assert np.unique(bihrt_mod.unpack_rgba(ref)[..., 0]).size > 4
