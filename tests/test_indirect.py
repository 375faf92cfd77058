"""One-bounce indirect lighting with a sky term (bih_render_indirect /
bih_render_indirect_device / bih_bounce_sample): per
hit sample one hashed, cosine-distributed bounce ray, its closest hit lit by
the call's lights under bih_render_area_lights' rules; an escaped bounce ray
collects the sky.

Expected values come from the oracle alone: the hash is numpy uint32
(wrapping), the bounce direction B, the hit points and both levels' lighting
are numpy f32 in the header's order; the bounce record is
OracleTree.closest(P, B, 1e-4) with u and v restated (test_trace.restate); the
shadow rays are test_direct.oracle_occluded and test_lights.oracle_segment.
Planes are compared on bits, NaN as NaN.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import test_area_lights as ta
import test_direct as td
import test_gbuffer as tg
import test_lights as tl
import test_trace as tt
from conftest import ROOT
from test_area_lights import U32, panels_of
from test_direct import MISS_SHADE, fib_lights
from test_gbuffer import EDGE, F32, LIBDIR, SEED, camera, expected, frame_rays, normals, renderer, scene, tree
from test_lights import NO_DIR, canon, lamps_of

SRC = os.path.join(ROOT, "tests", "c", "indirect_smoke.c")
W, H, SPP = 48, 32, 4
NAMES = ("lit", "bounce", "lit2", "irradiance", "rgba")
SIZE = {"lit": 8, "bounce": 16, "lit2": 8}          # bytes per sample; the others 4 per pixel
ALBEDO, SKY = 0.5, 0.25
T_LO = 1e-4
FLT_MAX = float(np.finfo(F32).max)
SLOT = 0x80000000
C1, C3, C5, C7, C9 = (F32(float.fromhex(x)) for x in
                      ("0x1.921fb6p+0", "-0x1.4abbcep-1", "0x1.466bc6p-4", "-0x1.32d2ccp-8", "0x1.507834p-13"))


# --- the header, restated ---------------------------------------------------------

def taylor_sin(x):
    x2 = x * x
    return ((((C9 * x2 + C7) * x2 + C5) * x2 + C3) * x2 + C1) * x


def sphere_points(seed, gp, fs):
    """(w (n, 3), q, z): the unit-sphere point of the header for global pixels gp
    and counters fs = frame*spp + s (u32 arrays)."""
    a, b = ta.sample_ab(seed, gp, fs, SLOT)
    with np.errstate(all="ignore"):
        z = F32(1.0) - F32(2.0) * a
        r = np.sqrt(np.fmax(F32(0.0), F32(1.0) - z * z))
        b4 = F32(4.0) * b
        q = b4.astype(np.int32)
        f = b4 - q.astype(F32)
        sn, cs = taylor_sin(f), taylor_sin(F32(1.0) - f)
        cx = np.select([q == 0, q == 1, q == 2], [cs, -sn, -cs], sn)
        sx = np.select([q == 0, q == 1, q == 2], [sn, cs, -sn], -cs)
        w = np.stack([r * cx, r * sx, z], 1)
    assert w.dtype == F32 and ((q >= 0) & (q <= 3)).all()
    return w, q, z


def bounce_dirs(seed, gp, fs, nrm):
    """B (n, 3) f32 = n + w."""
    with np.errstate(all="ignore"):
        B = np.asarray(nrm, F32) + sphere_points(seed, gp, fs)[0]
    assert B.dtype == F32
    return B


def light_level(P, nrm, on, dir_lights, lamps, panels, occluded, segment, seed, gp, fs):
    """bih_render_area_lights' lit word and per-sample sum of the points P with
    normals nrm (rows with `on` False: no point, lit 0 and sum 0) under
    dir_lights, then lamps, then panels; the panels' Q from (gp, fs)."""
    Ld, wd = np.ascontiguousarray(dir_lights["dir"], F32), np.ascontiguousarray(dir_lights["weight"], F32)
    Qp, wp = np.ascontiguousarray(lamps["pos"], F32), np.ascontiguousarray(lamps["weight"], F32)
    Kd, Kp, Ka, n = Ld.shape[0], Qp.shape[0], panels.shape[0], P.shape[0]
    lit, e = np.zeros(n, np.uint64), np.zeros(n, F32)
    with np.errstate(all="ignore"):
        cd = (nrm[:, 0:1] * Ld[None, :, 0] + nrm[:, 1:2] * Ld[None, :, 1]) + nrm[:, 2:3] * Ld[None, :, 2]
        fd = on[:, None] & (cd > 0)
        od = np.zeros((n, Kd), bool)
        si, ki = np.nonzero(fd)
        if si.size:
            od[si, ki] = occluded(P[si], Ld[ki])
        for k in range(Kd):
            lit_k = fd[:, k] & ~od[:, k]
            lit |= lit_k.astype(np.uint64) << np.uint64(k)
            e = np.where(lit_k, e + wd[k] * cd[:, k], e)
        for i in range(Kp):
            L = Qp[i][None, :] - P
            c = (nrm[:, 0] * L[:, 0] + nrm[:, 1] * L[:, 1]) + nrm[:, 2] * L[:, 2]
            r2 = (L[:, 0] * L[:, 0] + L[:, 1] * L[:, 1]) + L[:, 2] * L[:, 2]
            term = (wp[i] * (c / np.sqrt(r2))) / r2
            f = on & (c > 0)
            blocked = np.zeros(n, bool)
            if f.any():
                blocked[f] = segment(P[f], L[f])[0]
            lit_k = f & ~blocked
            lit |= lit_k.astype(np.uint64) << np.uint64(Kd + i)
            e = np.where(lit_k, e + term, e)
        for j in range(Ka):
            L = ta.sample_points(panels[j], j, seed, gp, fs) - P
            nl = ta.panel_normal(panels[j])
            c = (nrm[:, 0] * L[:, 0] + nrm[:, 1] * L[:, 1]) + nrm[:, 2] * L[:, 2]
            g = -((nl[0] * L[:, 0] + nl[1] * L[:, 1]) + nl[2] * L[:, 2])
            r2 = (L[:, 0] * L[:, 0] + L[:, 1] * L[:, 1]) + L[:, 2] * L[:, 2]
            ln = np.sqrt(r2)
            term = ((F32(panels[j]["weight"]) * (c / ln)) * (g / ln)) / r2
            f = on & (c > 0) & (g > 0)
            blocked = np.zeros(n, bool)
            if f.any():
                blocked[f] = segment(P[f], L[f])[0]
            lit_k = f & ~blocked
            lit |= lit_k.astype(np.uint64) << np.uint64(Kd + Kp + j)
            e = np.where(lit_k, e + term, e)
    assert e.dtype == F32
    return lit, e


def oracle_closest(name):
    """(P, B) -> HIT_DTYPE records of {o = P, t_lo = 1e-4, d = B}: OracleTree.closest,
    prim in file order, u and v restated (and t, which must be the oracle's)."""
    import bihrt
    tris, ot = scene(name)

    def fn(P, B):
        n = P.shape[0]
        t, idx = np.empty(n, F32), np.empty(n, np.int64)
        for k in range(n):
            t[k], idx[k] = ot.closest(P[k], B[k], T_LO)
        hit = idx >= 0
        out = np.zeros(n, bihrt.HIT_DTYPE)
        out["t"], out["prim"] = t, bihrt.NO_HIT
        assert (t[~hit] == F32(FLT_MAX)).all()
        if hit.any():
            prim = ot.tri_idx[idx[hit]]
            rt, ru, rv = tt.restate(tris[prim], P[hit], B[hit])
            assert np.array_equal(rt.view(np.uint32), t[hit].view(np.uint32)), "the restated t is not the oracle's"
            out["u"][hit], out["v"][hit], out["prim"][hit] = ru, rv, prim
        return out
    return fn


def restate(name, kname, w, h, spp, frame, dir_lights, lamps, panels, albedo, sky, closest=None, seed=SEED):
    """The header's five planes of the whole frame (flat), and the masks."""
    import bihrt
    tris, ot = scene(name)
    cam = camera(name, kname, w, h)
    d = frame_rays(cam, w, h, spp, frame).reshape(-1, 3)
    hits = expected(name, kname, w, h, spp, frame)["hits"]
    dl = dir_lights if dir_lights is not None else NO_DIR
    lp = lamps if lamps is not None else np.zeros(0, bihrt.POINT_LIGHT_DTYPE)
    pan = bihrt.pack_area_lights(panels if panels is not None else np.zeros((0, 10), F32))
    occluded, segment = td.oracle_occluded(ot), tl.oracle_segment(ot)
    closest = closest or oracle_closest(name)
    n = hits.shape[0]
    hit = hits["prim"] != bihrt.NO_HIT
    gp = (np.arange(n) // spp).astype(U32)                       # whole frame: local pixel = y*w + x
    fs = ((frame * spp + np.arange(n) % spp) & 0xFFFFFFFF).astype(U32)
    with np.errstate(all="ignore"):
        P = cam[0:3][None, :] + hits["t"][:, None] * d           # one multiply, then one add
        nrm = np.zeros((n, 3), F32)
        nrm[hit] = normals(tris[hits["prim"][hit]])
        lit, e_dir = light_level(P, nrm, hit, dl, lp, pan, occluded, segment, seed, gp, fs)
        B = bounce_dirs(seed, gp, fs, nrm)
        bounce = np.zeros(n, bihrt.HIT_DTYPE)
        bounce["t"], bounce["prim"] = FLT_MAX, bihrt.NO_HIT
        if hit.any():
            bounce[hit] = closest(P[hit], B[hit])
        hit2 = bounce["prim"] != bihrt.NO_HIT
        assert not (hit2 & ~hit).any()
        P2 = P + bounce["t"][:, None] * B
        nrm2 = np.zeros((n, 3), F32)
        nrm2[hit2] = normals(tris[bounce["prim"][hit2]])
        lit2, e2 = light_level(P2, nrm2, hit2, dl, lp, pan, occluded, segment, seed, gp, fs)
        e_ind = np.where(hit2, F32(albedo) * e2, F32(sky))
        e_s = np.where(hit, e_dir + e_ind, F32(0.0)).reshape(-1, spp)
        acc = e_s[:, 0]
        for k in range(1, spp):
            acc = acc + e_s[:, k]
        E = acc / F32(spp)
        assert E.dtype == F32 and P2.dtype == F32 and e_s.dtype == F32
        g8 = np.fmax(F32(0), np.fmin(F32(255), F32(255) * E)).astype(np.int32).astype(np.uint32)
    rgba = np.where(hit.reshape(-1, spp).any(1), g8 | (g8 << 8) | (g8 << 16), np.uint32(MISS_SHADE)).astype(np.uint32)
    out = {"lit": lit, "bounce": bounce, "lit2": lit2, "irradiance": E, "rgba": rgba, "hit": hit, "hit2": hit2,
           "P": P, "B": B, "nrm": nrm}
    for a in out.values():
        a.setflags(write=False)
    return out


def lights_of(name):
    return fib_lights(2), None, panels_of(name)


@functools.lru_cache(maxsize=None)
def expect(name, kname, w, h, spp, frame, albedo=ALBEDO, sky=SKY, lit=True):
    """The restatement under fib_lights(2) + panels_of(name) (lit False: no
    lights at all); read-only, computed once."""
    dl, lp, pan = lights_of(name) if lit else (None, None, None)
    return restate(name, kname, w, h, spp, frame, dl, lp, pan, albedo, sky)


def figures(exp, spp):
    """(bounce-hit share of hit samples, share of bounce hits with lit2 != 0,
    pixels with both escaped and stopped bounce rays)."""
    hit, hit2 = exp["hit"], exp["hit2"]
    esc = (hit & ~hit2).reshape(-1, spp).any(1)
    stop = hit2.reshape(-1, spp).any(1)
    return (float(hit2.sum() / max(int(hit.sum()), 1)),
            float((exp["lit2"][hit2] != 0).sum() / max(int(hit2.sum()), 1)), int((esc & stop).sum()))


def cplane(a):
    """Bits of a plane (a record plane field by field), every NaN as one NaN."""
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        return np.stack([canon(np.ascontiguousarray(a[f])).astype(np.uint32) for f in a.dtype.names], -1)
    return canon(a)


def assert_planes(got, exp, what="", names=NAMES):
    for name in names:
        g, e = got[name], np.asarray(exp[name]).reshape(got[name].shape)
        assert g.dtype == e.dtype, f"{what}: {name} {g.dtype}"
        bad = np.argwhere(cplane(g) != cplane(e))
        assert bad.size == 0, f"{what}: {name} differs at {bad[:4].tolist()} ({bad.shape[0]} values)"


def rows_of(exp, w, spp, ys):
    """The expected planes of global rows ys (local row order)."""
    ys = np.asarray(ys)
    out = {k: exp[k].reshape(-1, w * spp)[ys].reshape(-1) for k in ("lit", "bounce", "lit2")}
    out.update({k: exp[k].reshape(-1, w)[ys] for k in ("irradiance", "rgba")})
    return out


class Dev:
    """Device planes (torch tensors prefilled with 0xAB) of an indirect-lighting call."""

    def __init__(self, nrows, w, spp, names=NAMES):
        import torch
        self.nrows, self.w, self.spp, self.names = nrows, w, spp, names
        P = nrows * w
        self.t = {k: torch.full((P * (SIZE[k] * spp if k in SIZE else 4),), 0xAB, dtype=torch.uint8, device="cuda")
                  for k in NAMES}
        torch.cuda.synchronize()

    def launch(self, r, dl, lp, pan, bounce, frame, rows=None, stream=None):
        r.render_indirect_device({k: self.t[k].data_ptr() for k in self.names}, dl, lp, pan, bounce, frame, rows,
                                 stream)

    def result(self):
        """Every plane (also the ones not asked for), shaped as render_indirect's."""
        import bihrt
        out = {}
        for k, ten in self.t.items():
            dt, per = bihrt.INDIRECT_PLANES[k]
            a = ten.cpu().numpy().view(dt)
            out[k] = a.reshape(self.nrows, self.w) if per else a
        return out


def dev_indirect(r, dl, lp, pan, frame, rows=None, names=NAMES, bounce=(ALBEDO, SKY)):
    nrows = rows.nrows if rows is not None else r.h
    dv = Dev(nrows, r.w, r.spp, names)
    dv.launch(r, dl, lp, pan, bounce, frame, rows)
    r.sync()
    return dv.result()


@pytest.fixture(scope="module", autouse=True)
def _free_trees():
    yield
    while tg._trees:
        tg._trees.popitem()[1].close()


# --- CPU ------------------------------------------------------------------------

def test_struct_layout(bihrt_mod):
    Bn, I = bihrt_mod.Bounce, bihrt_mod.Indirect
    assert C.sizeof(Bn) == 8 and Bn.albedo.offset == 0 and Bn.sky.offset == 4
    p = C.sizeof(C.c_void_p)
    assert [f[0] for f in I._fields_] == list(NAMES) and C.sizeof(I) == 5 * p
    assert [getattr(I, f).offset for f in NAMES] == [k * p for k in range(5)]
    assert bihrt_mod.INDIRECT == NAMES and list(bihrt_mod.INDIRECT_PLANES) == list(NAMES)
    assert bihrt_mod.INDIRECT_PLANES["bounce"][0] == bihrt_mod.HIT_DTYPE and bihrt_mod.BOUNCE_SLOT == SLOT


def test_header_symbols_exported(bihrt_mod):
    names = bihrt_mod._lib.exported_symbols_from_header()
    L = bihrt_mod._lib.load()
    for sym in ("bih_render_indirect", "bih_render_indirect_device", "bih_bounce_sample"):
        assert sym in names and getattr(L, sym) is not None, sym
    hdr = open(os.path.join(ROOT, "include", "bih.h")).read()
    assert "#define BIH_ABI_VERSION 4" in hdr and "#define BIH_BOUNCE_SLOT 0x80000000u" in hdr
    assert "typedef struct bih_bounce" in hdr and "typedef struct bih_indirect" in hdr
    assert L.bih_abi_version() == 4


def _header_compiles(tmp_path, cc, std, ext):
    src = tmp_path / ("hdr." + ext)
    src.write_text('#include "bih.h"\n'
                   "int main(void) { bih_bounce b = {0.5f, 0.25f}; bih_indirect p = {0, 0, 0, 0, 0};\n"
                   "  float n[3] = {0, 0, 1}, d[3]; (void)b; (void)p; (void)BIH_BOUNCE_SLOT;\n"
                   "  return bih_bounce_sample(1, 0, 0, 1, 0, n, d) == BIH_OK ? 0 : 1; }\n")
    subprocess.run([cc, "-std=" + std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only",
                    "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_header_is_c11_and_cxx17(tmp_path):
    _header_compiles(tmp_path, "gcc", "c11", "c")
    _header_compiles(tmp_path, "g++", "c++17", "cpp")


def test_device_free_error_codes(bihrt_mod):
    """The argument checks come, in the header's order, before the tree or a
    device is touched: a stand-in tree pointer is never dereferenced."""
    L = bihrt_mod._lib.load()
    INVALID, TOO_LARGE = -1, -6
    raw = (C.c_char * 96)()
    base = (C.addressof(raw) + 15) & ~15
    fake = C.c_void_p(base)
    cam = bihrt_mod.Camera()
    I, R, S, Bn = bihrt_mod.Indirect, bihrt_mod.Rows, bihrt_mod.LightSet, bihrt_mod.Bounce
    sun = (bihrt_mod.Light * 1)()
    sun[0].dir[1], sun[0].weight = 1.0, 1.0
    lamp = (bihrt_mod.PointLight * 1)()
    pan = (bihrt_mod.AreaLight * 1)()
    ps, pl, pp = (C.cast(x, C.c_void_p) for x in (sun, lamp, pan))
    full, empty = S(ps, 1, pl, 1, pp, 1), S(None, 0, None, 0, None, 0)
    bn = Bn(0.5, 0.25)
    rgba, none = I(rgba=base), I()
    for entry in (lambda *a: L.bih_render_indirect_device(*a, None), L.bih_render_indirect):
        def call(t, c, w, h, spp, rows, s, b, d):
            return entry(t, C.byref(c) if c is not None else None, w, h, spp, 0, SEED,
                         C.byref(rows) if rows is not None else None, C.byref(s) if s is not None else None,
                         C.byref(b) if b is not None else None, C.byref(d) if d is not None else None)
        # 1: the G-buffer's checks, in its order
        assert call(None, cam, 8, 8, 4, None, full, bn, rgba) == INVALID
        assert call(fake, None, 8, 8, 4, None, full, bn, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, None, full, bn, None) == INVALID
        assert call(fake, cam, 0, 8, 4, None, full, bn, rgba) == INVALID
        assert call(fake, cam, 8, 8, 65, None, full, bn, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, None, full, bn, none) == INVALID               # all five planes NULL
        assert call(fake, cam, 8, 8, 4, R(6, 4, 4, 1), full, bn, rgba) == INVALID
        assert call(fake, cam, 1 << 16, 1 << 16, 1, None, S(ps, 65, None, 0, None, 0), None,
                    I(lit=base + 4)) == TOO_LARGE                                      # (before 2, 3 and 4)
        # 2: the lights: NULL and empty are legal, the rest as bih_render_area_lights
        assert call(fake, cam, 8, 8, 4, None, S(ps, 33, pl, 31, pp, 1), bn, rgba) == INVALID   # 65 together
        assert call(fake, cam, 8, 8, 4, None, S(ps, 0xFFFFFFFF, pl, 1, pp, 1), bn, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, None, S(ps, 1, pl, 1, pp, 17), bn, rgba) == INVALID    # n_area > 16
        assert call(fake, cam, 8, 8, 4, None, S(None, 1, pl, 1, pp, 1), bn, rgba) == INVALID   # NULL with a count
        assert call(fake, cam, 8, 8, 4, None, S(ps, 1, None, 1, pp, 1), bn, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), S(ps, 1, pl, 1, None, 1), bn, rgba) == INVALID
        # 3: bounce == NULL; the alignments
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, None, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), None, None, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, bn, I(lit=base + 4, rgba=base)) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, bn, I(lit2=base + 4, rgba=base)) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, bn, I(bounce=base + 8)) == INVALID
        # 4: nothing to do -- each single plane, no lights at all
        for d in (I(lit=base), I(bounce=base), I(lit2=base + 8), I(irradiance=base + 4), rgba):
            assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, bn, d) == 0
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), None, bn, rgba) == 0
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), empty, bn, rgba) == 0
        assert call(fake, cam, 8, 8, 64, R(3, 0, 0, 0), S(ps, 46, pl, 2, pp, 16), bn, rgba) == 0


@functools.lru_cache(maxsize=None)
def _samples():
    """200,000 (seed, gp, frame, spp, s) draws: several seeds, frames and spp."""
    rng = np.random.default_rng(7)
    n = 200000
    seeds = [1984, 0, 0xFFFFFFFFFFFFFFFF, 0x8000000000000001, 0xDEADBEEF00000000]
    spps = [1, 3, 4, 16, 64]
    frames = [0, 1, 2, 77, 0xFFFFFFFF]
    k = np.arange(n)
    seed = np.array(seeds, np.uint64)[k % 5]
    spp = np.array(spps)[(k // 5) % 5]
    frame = np.array(frames, np.uint64)[(k // 25) % 5]
    s = rng.integers(0, 1 << 30, n) % spp
    gp = rng.integers(0, 1 << 32, n).astype(U32)
    fs = ((frame * spp.astype(np.uint64) + s.astype(np.uint64)) & np.uint64(0xFFFFFFFF)).astype(U32)
    return seed, gp, frame, spp, s, fs


def _restated_w(nrm):
    """(B, q, z) of _samples() for the normal nrm, seed by seed."""
    seed, gp, frame, spp, s, fs = _samples()
    B = np.zeros((gp.shape[0], 3), F32)
    q, z = np.zeros(gp.shape[0], np.int32), np.zeros(gp.shape[0], F32)
    for sd in np.unique(seed):
        m = seed == sd
        w, q[m], z[m] = sphere_points(int(sd), gp[m], fs[m])
        with np.errstate(all="ignore"):
            B[m] = np.asarray(nrm, F32)[None, :] + w
    return B, q, z


def test_bounce_sample_equals_the_hash(bihrt_mod):
    """bih_bounce_sample is the header's B on bits over 200,000 hashed samples;
    all four quadrants and both signs of z occur."""
    L = bihrt_mod._lib.load()
    seed, gp, frame, spp, s, fs = _samples()
    nrm = np.array([0.3, -0.5, 0.8], F32)
    want, q, z = _restated_w(nrm)
    assert sorted(np.unique(q).tolist()) == [0, 1, 2, 3] and (z > 0).any() and (z < 0).any()
    nn, d = (C.c_float * 3)(*nrm.tolist()), (C.c_float * 3)()
    got = np.empty((gp.shape[0], 3), F32)
    fn = L.bih_bounce_sample
    for k in range(gp.shape[0]):
        assert fn(int(seed[k]), int(gp[k]), int(frame[k]), int(spp[k]), int(s[k]), nn, d) == 0
        got[k] = d[:]
    bad = np.argwhere(canon(got) != canon(want))
    assert bad.size == 0, (bad[:4].tolist(), bad.shape[0])
    # the Python mirror and the errors
    one = bihrt_mod.bounce_sample(1984, 77, 1, 4, 2, nrm)
    assert one.dtype == F32 and one.tolist() == bounce_dirs(1984, np.array([77], U32), np.array([6], U32), nrm)[0].tolist()
    assert fn(1, 0, 0, 4, 0, None, d) == -1 and fn(1, 0, 0, 4, 0, nn, None) == -1
    assert fn(1, 0, 0, 0, 0, nn, d) == -1 and fn(1, 0, 0, 4, 4, nn, d) == -1 and fn(1, 0, 0, 4, 3, nn, d) == 0
    with pytest.raises(bihrt_mod.BihError):
        bihrt_mod.bounce_sample(1, 0, 0, 4, 4, nrm)


def test_bounce_distribution():
    """n = (0, 0, 1): B is cosine-distributed (mean cosine 2/3, standard error
    5e-4 at 200,000 samples) and w lies on the unit sphere."""
    nrm = np.array([0, 0, 1], F32)
    B = _restated_w(nrm)[0].astype(np.float64)
    w = B - nrm[None, :].astype(np.float64)
    assert np.abs(np.linalg.norm(w, axis=1) - 1.0).max() <= 1e-5
    ln = np.linalg.norm(B, axis=1)
    mean = float((B[ln > 0, 2] / ln[ln > 0]).mean())
    print("mean cosine %.5f" % mean)
    assert abs(mean - 2.0 / 3.0) <= 0.003


def test_app_bounce_options(bihrt_mod):
    """--bounce without --direct and malformed values are errors, before any device is used."""
    from bihrt.app import main
    base = ["--scene", "cornell", "--frames", "1"]
    for extra in (["--bounce", "0.5"],
                  ["--direct", "d.ppm", "--bounce", "x"],
                  ["--direct", "d.ppm", "--bounce", "0.5,0.25,1"],
                  ["--direct", "d.ppm", "--bounce", ""]):
        with pytest.raises(SystemExit):
            main(base + extra)


def _build_c(tmp_path) -> str:
    exe = str(tmp_path / "indirect_smoke")
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
    assert "FAIL" not in r.stdout and r.stdout.count("ok ") == 8, r.stdout


# --- GPU ------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name,kname", [("cornell", "K1"), ("soup3k", "K2"), ("soup20k", "K2")])
def test_classes(name, kname, gpu, bihrt_mod):
    """fib_lights(2) + the scene's panels, albedo 0.5, sky 0.25 at 48x32x4: stopped
    and escaped bounce rays, lit and dark bounce hits are all there (asserted on
    the restatement); the five planes on bits.  soup20k once more with two
    stack slots on chip (the spill stack is used)."""
    exp = expect(name, kname, W, H, SPP, 1)
    share, lit2, both = figures(exp, SPP)
    print(name, "bounce-hit share %.3f, lit2 share %.3f, mixed pixels %d" % (share, lit2, both))
    assert 0.10 <= share <= 0.90, share
    assert 0.10 <= lit2 <= 0.90, lit2
    assert both >= 8, both
    g = tree(name)
    r = renderer(g, name, kname, W, H, SPP)
    dl, lp, pan = lights_of(name)
    assert_planes(dev_indirect(r, dl, lp, pan, 1), exp, f"{name} {kname}")
    if name == "soup20k":
        g.set_param(bihrt_mod.PARAM_TRACE_LDS_SLOTS, 2)
        try:
            assert_planes(dev_indirect(r, dl, lp, pan, 1), exp, "2 slots")
        finally:
            g.set_param(bihrt_mod.PARAM_TRACE_LDS_SLOTS, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE)
def test_edge_scenes(name, gpu, bihrt_mod):
    """Every edge scene under K2, bits only; dodeca is convex and one-sided: every bounce ray escapes."""
    exp = expect(name, "K2", W, H, SPP, 1)
    assert exp["hit"].any()
    if name == "dodeca":
        assert not exp["hit2"].any()
    r = renderer(tree(name), name, "K2", W, H, SPP)
    dl, lp, pan = lights_of(name)
    got = dev_indirect(r, dl, lp, pan, 1)
    assert_planes(got, exp, name)
    if name == "dodeca":
        assert (got["bounce"]["prim"] == bihrt_mod.NO_HIT).all() and not got["lit2"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,spp", [(1, 1, 1), (37, 29, 3), (8, 8, 64), (16, 8, 16)])
def test_shapes(w, h, spp, gpu, bihrt_mod):
    """One sample; partial tiles and waves with an spp that is no power of two; a pixel per wave; four pixels per wave."""
    exp = expect("soup20k", "K2", w, h, spp, 1)
    if (w, h) != (1, 1):
        assert exp["hit2"].any() and (exp["hit"] & ~exp["hit2"]).any() and exp["lit2"].any()
    r = renderer(tree("soup20k"), "soup20k", "K2", w, h, spp)
    dl, lp, pan = lights_of("soup20k")
    assert_planes(dev_indirect(r, dl, lp, pan, 1), exp, f"{w}x{h}x{spp}")


@pytest.mark.gpu
def test_more_hit_samples_than_the_persistent_grid(gpu, bihrt_mod):
    """A frame whose hit samples exceed the persistent grid x 64 lanes, so that
    the bounce walk's waves come back for more: its planes equal the same frame
    assembled from bands of 32 rows, each far below the grid (gp is global, so
    bands reassemble; the small shapes above tie a band to the oracle)."""
    import torch
    w, h, spp = 768, 512, 4
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    g = tree("cornell")
    r = renderer(g, "cornell", "K1", w, h, spp)
    dl, lp, pan = lights_of("cornell")
    nhit = int((tg.dev_gbuffer(r, 1)["hits"]["prim"] != bihrt_mod.NO_HIT).sum())
    assert nhit > cus * 32 * 64, (nhit, cus)
    full = dev_indirect(r, dl, lp, pan, 1)
    assert (full["bounce"]["prim"] != bihrt_mod.NO_HIT).any() and full["lit2"].any()
    band = 32
    assert w * band * spp < cus * 32 * 64
    for y0 in range(0, h, band):
        part = dev_indirect(r, dl, lp, pan, 1, bihrt_mod.Rows(y0, band, band, 1))
        for k in ("lit", "bounce", "lit2"):
            want = full[k].reshape(h, w * spp)[y0:y0 + band].reshape(-1)
            assert part[k].tobytes() == want.tobytes(), (k, y0)
        for k in ("irradiance", "rgba"):
            assert part[k].tobytes() == full[k][y0:y0 + band].tobytes(), (k, y0)


@pytest.mark.gpu
def test_rows_bands_planes_and_host_entry(gpu, bihrt_mod):
    """Interleaved bands and rows that are not tile-aligned equal the same rows
    of the full frame, through both entries (the hash takes the GLOBAL pixel);
    each plane alone gives the bits of all together and leaves the others
    untouched; no call after the first of the shape allocates, and a fresh
    tree's first call takes at least the header's scratch per sample."""
    exp = expect("soup20k", "K2", W, H, SPP, 1)
    g = tree("soup20k")
    r = renderer(g, "soup20k", "K2", W, H, SPP)
    dl, lp, pan = lights_of("soup20k")
    host = r.render_indirect(dl, lp, pan, (ALBEDO, SKY), 1)
    assert sorted(host) == sorted(NAMES) and host["bounce"].shape == (W * H * SPP,) and host["rgba"].shape == (H, W)
    assert_planes(host, exp, "host entry")
    for name in NAMES:                       # (first: a call without lit / lit2 grows the tree's own words)
        got = dev_indirect(r, dl, lp, pan, 1, names=(name,))
        assert_planes(got, exp, f"{name} alone", names=(name,))
        for other in NAMES:
            if other != name:
                assert (np.ascontiguousarray(got[other]).view(np.uint8) == 0xAB).all(), (name, other)
    first = g.info()
    for rows, ys in ((bihrt_mod.Rows(4, 8, 4, 2), [4, 5, 6, 7, 12, 13, 14, 15]),
                     (bihrt_mod.Rows(5, 7, 7, 1), list(range(5, 12)))):
        sub = rows_of(exp, W, SPP, ys)
        assert (sub["bounce"]["prim"] != bihrt_mod.NO_HIT).any() and (sub["lit2"] != 0).any()
        assert_planes(dev_indirect(r, dl, lp, pan, 1, rows), sub, f"rows {ys[0]}..")
        assert_planes(r.render_indirect(dl, lp, pan, (ALBEDO, SKY), 1, rows), sub, "host entry rows")
    for name in NAMES:
        assert_planes(dev_indirect(r, dl, lp, pan, 1, names=(name,)), exp, f"{name} alone", names=(name,))
    assert_planes(r.render_indirect(dl, lp, pan, (ALBEDO, SKY), 1, planes=("irradiance",)), exp, "host, one plane",
                  names=("irradiance",))
    after = g.info()
    assert after.device_allocs == first.device_allocs and after.device_bytes == first.device_bytes
    # a fresh tree's first five-plane call: the header's 28 + 20 + 9 bytes of scratch per sample
    fresh = bihrt_mod.GPUArrayManager(scene("soup20k")[0])
    rf = renderer(fresh, "soup20k", "K2", W, H, SPP)
    before = fresh.info()
    assert_planes(dev_indirect(rf, dl, lp, pan, 1), exp, "fresh tree")
    assert fresh.info().device_bytes >= before.device_bytes + W * H * SPP * 57
    fresh.close()


@pytest.mark.gpu
def test_composition(gpu, bihrt_mod):
    """`bounce` equals bih_trace_device(CLOSEST) on the restated rays, GPU
    against GPU; `lit` is bih_render_area_lights' lit; with albedo = 0 and sky =
    0 on cornell irradiance and rgba are bih_render_area_lights' byte for byte."""
    import bihrt
    g = tree("soup3k")
    exp = expect("soup3k", "K2", W, H, SPP, 1)

    def gpu_closest(P, B):
        return tt.dev_trace(g, bihrt.pack_rays(P, B, F32(T_LO)), bihrt.QUERY_CLOSEST)
    dl, lp, pan = lights_of("soup3k")
    traced = restate("soup3k", "K2", W, H, SPP, 1, dl, lp, pan, ALBEDO, SKY, closest=gpu_closest)
    assert_planes(traced, exp, "trace_device vs oracle", names=("bounce",))
    r = renderer(g, "soup3k", "K2", W, H, SPP)
    got = dev_indirect(r, dl, lp, pan, 1)
    assert_planes(got, traced, "indirect vs trace")
    area = ta.dev_area(r, dl, lp, pan, 1)
    assert got["lit"].tobytes() == area["lit"].tobytes()
    assert got["lit"].tobytes() == dev_indirect(r, dl, lp, pan, 1, bounce=(7.0, -3.0))["lit"].tobytes()
    rc = renderer(tree("cornell"), "cornell", "K1", W, H, SPP)
    dl, lp, pan = lights_of("cornell")
    zero = dev_indirect(rc, dl, lp, pan, 1, bounce=(0.0, 0.0))
    area = ta.dev_area(rc, dl, lp, pan, 1)
    for name in ("lit", "irradiance", "rgba"):
        assert zero[name].tobytes() == area[name].tobytes(), name
    assert (area["irradiance"] > 0).any() and (zero["bounce"]["prim"] != bihrt.NO_HIT).any()


@pytest.mark.gpu
def test_sky_only(gpu, bihrt_mod):
    """No lights, sky = 1: irradiance = escaped bounce rays / spp exactly, lit =
    lit2 = 0 -- the ambient-occlusion render; NULL, None and empty sets agree."""
    exp = expect("soup20k", "K2", W, H, SPP, 1, 0.5, 1.0, False)
    esc = (exp["hit"] & ~exp["hit2"]).reshape(-1, SPP).sum(1)
    assert np.array_equal(exp["irradiance"], (esc.astype(F32) / F32(SPP))) and (esc > 0).any() and (esc < SPP).any()
    assert not exp["lit"].any() and not exp["lit2"].any()
    r = renderer(tree("soup20k"), "soup20k", "K2", W, H, SPP)
    got = dev_indirect(r, None, None, None, 1, bounce=(0.5, 1.0))
    assert_planes(got, exp, "sky only")
    assert not got["lit"].any() and not got["lit2"].any()
    # lights == NULL through the C entry
    L = bihrt_mod._lib.load()
    dv = Dev(H, W, SPP)
    ip = bihrt_mod.Indirect(**{k: dv.t[k].data_ptr() for k in NAMES})
    bn = bihrt_mod.Bounce(0.5, 1.0)
    assert L.bih_render_indirect_device(r.arrays.handle, C.byref(r.camera), W, H, SPP, 1, SEED, None, None,
                                        C.byref(bn), C.byref(ip), None) == 0
    r.sync()
    assert_planes(dv.result(), exp, "lights == NULL")


@pytest.mark.gpu
def test_frames(gpu, bihrt_mod):
    """Frames 0, 1 and 2 give different bounce records, each the restatement's."""
    es = [expect("soup3k", "K2", W, H, SPP, f) for f in (0, 1, 2)]
    assert not np.array_equal(es[0]["bounce"], es[1]["bounce"]) and not np.array_equal(es[1]["bounce"], es[2]["bounce"])
    r = renderer(tree("soup3k"), "soup3k", "K2", W, H, SPP)
    dl, lp, pan = lights_of("soup3k")
    for f in (0, 1, 2, 1):
        assert_planes(dev_indirect(r, dl, lp, pan, f), es[f], f"frame {f}")


@pytest.mark.gpu
def test_renders_undisturbed(gpu, bihrt_mod):
    """render f=0, indirect f=2, render f=2, area f=2, render f=3, indirect f=3:
    every image is the oracle's and every plane is right (the bounce takes no
    XORWOW draw)."""
    tris, ot = scene("cornell")
    cam = camera("cornell", "K1", W, H)
    g = bihrt_mod.GPUArrayManager(tris)
    r = renderer(g, "cornell", "K1", W, H, SPP)
    dl, lp, pan = lights_of("cornell")
    a_before = r.render_area_lights(dl, lp, pan, 2)
    f0 = r.render(0)
    d2 = r.render_indirect(dl, lp, pan, (ALBEDO, SKY), 2)
    f2 = r.render(2)
    a_after = r.render_area_lights(dl, lp, pan, 2)
    f3 = r.render(3)
    d3 = r.render_indirect(dl, lp, pan, (ALBEDO, SKY), 3)
    assert r.frame == 4
    for f, img in ((0, f0), (2, f2), (3, f3)):
        assert np.array_equal(img, ot.render(W, H, spp=SPP, frame=f, seed=SEED, cam=cam)[0]), f
    for name in ("lit", "irradiance", "rgba"):
        assert a_before[name].tobytes() == a_after[name].tobytes(), name
    assert a_after["lit"].tobytes() == d2["lit"].tobytes()
    assert_planes(d2, expect("cornell", "K1", W, H, SPP, 2), "frame 2")
    assert_planes(d3, expect("cornell", "K1", W, H, SPP, 3), "frame 3")
    g.close()


@pytest.mark.gpu
def test_rebuild_ordering_and_two_streams(gpu, bihrt_mod):
    """Two calls of one tree back to back on two streams with different frames;
    then a call on a second stream after rebuild() sees the new soup's tree."""
    import torch
    old, new = scene("soup3k")[0], scene("soup3k2")[0]
    soup = torch.from_numpy(old.copy()).cuda()
    torch.cuda.synchronize()
    g = bihrt_mod.GPUArrayManager.from_device(soup.data_ptr(), old.shape[0])
    ea, eb = expect("soup3k", "K2", W, H, SPP, 1), expect("soup3k", "K2", W, H, SPP, 2)
    e1 = expect("soup3k2", "K2", W, H, SPP, 1)
    assert not np.array_equal(ea["bounce"], e1["bounce"])
    r0, r1 = renderer(g, "soup3k", "K2", W, H, SPP), renderer(g, "soup3k2", "K2", W, H, SPP)
    da, db, dc, d1 = (Dev(H, W, SPP) for _ in range(4))
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    bn = (ALBEDO, SKY)
    da.launch(r0, *lights_of("soup3k"), bn, 1, stream=sa.cuda_stream)
    db.launch(r0, *lights_of("soup3k"), bn, 2, stream=sb.cuda_stream)
    dc.launch(r0, *lights_of("soup3k"), bn, 1, stream=sa.cuda_stream)
    sa.synchronize()
    sb.synchronize()
    g.sync()                      # (the caller's duty: the soup is not rewritten under a build or render)
    soup.copy_(torch.from_numpy(new))
    torch.cuda.synchronize()
    g.rebuild()
    d1.launch(r1, *lights_of("soup3k2"), bn, 1, stream=sb.cuda_stream)
    sb.synchronize()
    assert_planes(da.result(), ea, "stream a")
    assert_planes(db.result(), eb, "stream b")
    assert_planes(dc.result(), ea, "stream a again")
    assert_planes(d1.result(), e1, "after the rebuild")
    g.close()


@pytest.mark.gpu
def test_c_caller(tmp_path, gpu, bihrt_mod):
    """tests/c/indirect_smoke.c -- bih_build + bih_render_indirect from strict
    C11 (cornell, 64x48, the reference camera, a sky, lamps and the ceiling
    panel): render_indirect's planes."""
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
                        str(pp), str(pl.shape[0]), str(ap), str(al.shape[0]), "0.5", "0.25", str(op)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "indirect_smoke OK" in r.stdout, r.stdout + r.stderr
    ref = bihrt_mod.Renderer(tree("cornell"), w, h, spp=spp).render_indirect(dl, pl, al, (0.5, 0.25), 0)
    assert ref["lit2"].any() and (ref["bounce"]["prim"] != bihrt_mod.NO_HIT).any()
    raw = np.fromfile(op, np.uint8)
    P = w * h
    assert raw.size == P * (32 * spp + 8)
    off = 0
    for name, size in (("lit", 8 * spp), ("bounce", 16 * spp), ("lit2", 8 * spp), ("irradiance", 4), ("rgba", 4)):
        part = raw[off:off + P * size]
        off += P * size
        assert np.array_equal(part, np.ascontiguousarray(ref[name]).view(np.uint8).reshape(-1)), name


@pytest.mark.gpu
def test_app_writes_ppm(tmp_path, gpu, bihrt_mod):
    """python -m bihrt --direct --bounce: the PPM of render_indirect's rgba plane
    with the panel and a lamp, and alone (sky only)."""
    from bihrt.app import main
    want = tmp_path / "want.ppm"
    rr = bihrt_mod.Renderer(tree("cornell"), 64, 48)
    panel = np.array([[0.1, 0.98, 1.0, 0.6, 0, 0, 0, 0, 0.6, 4.0]], F32)
    lamp = np.array([[0.0, 0.5, 0.0, 1.0]], F32)
    for tag, extra, lights, bn in (
            ("lit", ["--sky", "0", "--lamp", "0,0.5,0", "--panel", "0.1,0.98,1,0.6,0,0,0,0,0.6,4", "--bounce", "0.5,0.25"],
             (None, lamp, panel), (0.5, 0.25)),
            ("ao", ["--sky", "0", "--bounce", "0.5,1"], (None, None, None), (0.5, 1.0)),
            ("dflt", ["--bounce", "0.5"], (None, None, None), (0.5, 1.0))):
        dr = tmp_path / ("d%s.ppm" % tag)
        assert main(["--scene", "cornell", "--width", "64", "--height", "48", "--frames", "1", "--direct", str(dr)]
                    + extra) == 0
        ref = rr.render_indirect(*lights, bn, 0, planes=("rgba",))["rgba"]
        bihrt_mod.write_ppm(str(want), ref)
        assert open(dr, "rb").read() == open(want, "rb").read(), tag
        assert np.unique(bihrt_mod.unpack_rgba(ref)[..., 0]).size > 2
