"""Multi-bounce paths (bih_render_path / bih_render_path_device /
bih_path_sample): bih_render_indirect carried on for
1 .. 8 levels, a sample's path going on from each bounce hit until a ray escapes
(it collects the sky) or the last level is reached.

Expected values come from the oracle alone: per level the sphere point with the
level's hash slot (numpy uint32, wrapping), test_indirect.oracle_closest for
the bounce record and test_indirect.light_level for the lit word and the sum,
then the header's forward accumulation in numpy f32.  The levels are restated
once per scene to depth 8; a call of n_bounces levels takes the first n_bounces
of them.  Planes are compared on bits, NaN as NaN (test_indirect.cplane).
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
import test_indirect as ti
import test_lights as tl
import test_trace as tt
from conftest import ROOT
from test_area_lights import U32
from test_direct import MISS_SHADE
from test_gbuffer import EDGE, F32, LIBDIR, SEED, camera, expected, frame_rays, normals, renderer, scene, tree
from test_indirect import ALBEDO, FLT_MAX, SKY, SLOT, T_LO, cplane, lights_of
from test_lights import NO_DIR, canon, lamps_of

SRC = os.path.join(ROOT, "tests", "c", "path_smoke.c")
W, H, SPP = 48, 32, 4
NAMES = ("lit", "bounces", "lits", "irradiance", "rgba")
SIZE = {"lit": 8, "bounces": 16, "lits": 8}         # bytes per sample (and level); the others 4 per pixel
LEVELS = ("bounces", "lits")                        # one plane per level
MAXB = 8
FRAME = 0        # the classes' frame: the one whose counts the conditions of check_class were set on


# --- the header, restated ---------------------------------------------------------

def sphere_points(seed, gp, fs, level):
    """w (n, 3) f32: test_indirect.sphere_points with the hash's last mix taking
    the slot BIH_BOUNCE_SLOT + (level - 1), wrapping."""
    a, b = ta.sample_ab(seed, gp, fs, (SLOT + level - 1) & 0xFFFFFFFF)
    with np.errstate(all="ignore"):
        z = F32(1.0) - F32(2.0) * a
        r = np.sqrt(np.fmax(F32(0.0), F32(1.0) - z * z))
        b4 = F32(4.0) * b
        q = b4.astype(np.int32)
        f = b4 - q.astype(F32)
        sn, cs = ti.taylor_sin(f), ti.taylor_sin(F32(1.0) - f)
        cx = np.select([q == 0, q == 1, q == 2], [cs, -sn, -cs], sn)
        sx = np.select([q == 0, q == 1, q == 2], [sn, cs, -sn], -cs)
        w = np.stack([r * cx, r * sx, z], 1)
    assert w.dtype == F32 and ((q >= 0) & (q <= 3)).all()
    return w


def path_dirs(seed, gp, fs, level, nrm):
    """B_level (n, 3) f32 = n + w."""
    with np.errstate(all="ignore"):
        B = np.asarray(nrm, F32) + sphere_points(seed, gp, fs, level)
    assert B.dtype == F32
    return B


def restate_levels(name, kname, w, h, spp, frame, dir_lights, lamps, panels, levels=MAXB, closest=None, seed=SEED):
    """The header's levels 0 .. `levels` of the whole frame, before any sum:
    "lit", "e0", "hit" of level 0; lists (index k-1 = level k) "bounces", "lits",
    "e", "alive" and the rays "P" (origins), "B" (directions) of level k."""
    import bihrt
    tris, ot = scene(name)
    cam = camera(name, kname, w, h)
    d = frame_rays(cam, w, h, spp, frame).reshape(-1, 3)
    hits = expected(name, kname, w, h, spp, frame)["hits"]
    dl = dir_lights if dir_lights is not None else NO_DIR
    lp = lamps if lamps is not None else np.zeros(0, bihrt.POINT_LIGHT_DTYPE)
    pan = bihrt.pack_area_lights(panels if panels is not None else np.zeros((0, 10), F32))
    occluded, segment = td.oracle_occluded(ot), tl.oracle_segment(ot)
    closest = closest or ti.oracle_closest(name)
    n = hits.shape[0]
    hit = hits["prim"] != bihrt.NO_HIT
    gp = (np.arange(n) // spp).astype(U32)                       # whole frame: local pixel = y*w + x
    fs = ((frame * spp + np.arange(n) % spp) & 0xFFFFFFFF).astype(U32)
    out = {"hit": hit, "bounces": [], "lits": [], "e": [], "alive": [], "P": [], "B": []}
    with np.errstate(all="ignore"):
        P = cam[0:3][None, :] + hits["t"][:, None] * d           # one multiply, then one add
        nrm = np.zeros((n, 3), F32)
        nrm[hit] = normals(tris[hits["prim"][hit]])
        out["lit"], out["e0"] = ti.light_level(P, nrm, hit, dl, lp, pan, occluded, segment, seed, gp, fs)
        alive = hit
        for k in range(1, levels + 1):
            B = path_dirs(seed, gp, fs, k, nrm)
            rec = np.zeros(n, bihrt.HIT_DTYPE)
            rec["t"], rec["prim"] = FLT_MAX, bihrt.NO_HIT
            if alive.any():
                rec[alive] = closest(P[alive], B[alive])
            stopped = rec["prim"] != bihrt.NO_HIT
            assert not (stopped & ~alive).any()
            out["P"].append(P)
            out["B"].append(B)
            P = P + rec["t"][:, None] * B
            nrm = np.zeros((n, 3), F32)
            nrm[stopped] = normals(tris[rec["prim"][stopped]])
            lits, e = ti.light_level(P, nrm, stopped, dl, lp, pan, occluded, segment, seed, gp, fs)
            assert P.dtype == F32 and e.dtype == F32
            out["bounces"].append(rec)
            out["lits"].append(lits)
            out["e"].append(e)
            out["alive"].append(stopped)
            alive = stopped
    for v in out.values():
        for a in (v if isinstance(v, list) else [v]):
            a.setflags(write=False)
    return out


_levels = {}


def levels_of(name, kname, w, h, spp, frame, lit=True, levels=MAXB):
    """restate_levels to a depth of at least `levels` under fib_lights(2) +
    panels_of(name) (lit False: no lights at all); read-only, computed once
    (a deeper restatement serves a shallower request: level k does not depend
    on the levels after it)."""
    key = (name, kname, w, h, spp, frame, lit)
    if key not in _levels or len(_levels[key]["alive"]) < levels:
        dl, lp, pan = lights_of(name) if lit else (None, None, None)
        _levels[key] = restate_levels(name, kname, w, h, spp, frame, dl, lp, pan, levels)
    return _levels[key]


def planes_of(lv, spp, n_bounces, albedo=ALBEDO, sky=SKY):
    """The five planes of a call of n_bounces levels: the forward accumulation
    in f32 over the restated levels."""
    hit = lv["hit"]
    albedo, sky = F32(albedo), F32(sky)
    with np.errstate(all="ignore"):
        thr = F32(1.0)
        acc = np.where(hit, lv["e0"], F32(0.0))
        before = hit
        for k in range(1, n_bounces + 1):
            alive = lv["alive"][k - 1]
            acc = np.where(before & ~alive, acc + thr * sky, acc)          # an escape: thr_{k-1} * sky
            thr = thr * albedo
            acc = np.where(alive, acc + thr * lv["e"][k - 1], acc)
            before = alive
        assert acc.dtype == F32 and isinstance(thr, F32)
        e_s = acc.reshape(-1, spp)
        tot = e_s[:, 0]
        for k in range(1, spp):
            tot = tot + e_s[:, k]
        E = tot / F32(spp)
        g8 = np.fmax(F32(0), np.fmin(F32(255), F32(255) * E)).astype(np.int32).astype(np.uint32)
    rgba = np.where(hit.reshape(-1, spp).any(1), g8 | (g8 << 8) | (g8 << 16), np.uint32(MISS_SHADE)).astype(np.uint32)
    return {"lit": lv["lit"], "bounces": np.stack(lv["bounces"][:n_bounces]), "lits": np.stack(lv["lits"][:n_bounces]),
            "irradiance": E, "rgba": rgba}


def counts(lv):
    """(hit samples, live paths per level, escapes per level, live bounce hits with a non-zero lit word per level)."""
    before, live, esc, lit = lv["hit"], [], [], []
    for alive, lits in zip(lv["alive"], lv["lits"]):
        live.append(int(alive.sum()))
        esc.append(int((before & ~alive).sum()))
        lit.append(int((lits[alive] != 0).sum()))
        before = alive
    return int(lv["hit"].sum()), live, esc, lit


def assert_planes(got, exp, what="", names=NAMES):
    for name in names:
        g, e = got[name], np.asarray(exp[name]).reshape(got[name].shape)
        assert g.dtype == e.dtype, f"{what}: {name} {g.dtype}"
        bad = np.argwhere(cplane(g) != cplane(e))
        assert bad.size == 0, f"{what}: {name} differs at {bad[:4].tolist()} ({bad.shape[0]} values)"


def rows_of(exp, w, spp, ys):
    """The expected planes of global rows ys (local row order)."""
    ys = np.asarray(ys)
    nb = exp["bounces"].shape[0]
    out = {"lit": exp["lit"].reshape(-1, w * spp)[ys].reshape(-1)}
    out.update({k: exp[k].reshape(nb, -1, w * spp)[:, ys].reshape(nb, -1) for k in LEVELS})
    out.update({k: exp[k].reshape(-1, w)[ys] for k in ("irradiance", "rgba")})
    return out


class Dev:
    """Device planes (torch tensors prefilled with 0xAB) of a path call."""

    def __init__(self, nrows, w, spp, n_bounces, names=NAMES):
        import torch
        self.nrows, self.w, self.spp, self.nb, self.names = nrows, w, spp, n_bounces, names
        P = nrows * w
        self.t = {k: torch.full((P * (SIZE[k] * spp * (n_bounces if k in LEVELS else 1) if k in SIZE else 4),), 0xAB,
                                dtype=torch.uint8, device="cuda") for k in NAMES}
        torch.cuda.synchronize()

    def launch(self, r, dl, lp, pan, bounce, frame, rows=None, stream=None):
        r.render_path_device({k: self.t[k].data_ptr() for k in self.names}, dl, lp, pan, bounce, self.nb, frame, rows,
                             stream)

    def result(self):
        """Every plane (also the ones not asked for), shaped as render_path's."""
        import bihrt
        out = {}
        for k, ten in self.t.items():
            dt, per = bihrt.PATH_PLANES[k]
            a = ten.cpu().numpy().view(dt)
            out[k] = a.reshape(self.nrows, self.w) if per > 0 else (a.reshape(self.nb, -1) if per < 0 else a)
        return out


def dev_path(r, dl, lp, pan, n_bounces, frame, rows=None, names=NAMES, bounce=(ALBEDO, SKY)):
    nrows = rows.nrows if rows is not None else r.h
    dv = Dev(nrows, r.w, r.spp, n_bounces, names)
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
    Pt = bihrt_mod.Path
    p = C.sizeof(C.c_void_p)
    assert [f[0] for f in Pt._fields_] == list(NAMES) and C.sizeof(Pt) == 5 * p
    assert [getattr(Pt, f).offset for f in NAMES] == [k * p for k in range(5)]
    assert bihrt_mod.PATH == NAMES and list(bihrt_mod.PATH_PLANES) == list(NAMES)
    assert bihrt_mod.PATH_PLANES["bounces"][0] == bihrt_mod.HIT_DTYPE and bihrt_mod.MAX_BOUNCES == MAXB
    for name in ("Path", "PATH", "PATH_PLANES", "MAX_BOUNCES", "path_sample"):
        assert name in bihrt_mod.__all__, name
    assert hasattr(bihrt_mod.Renderer, "render_path") and hasattr(bihrt_mod.Renderer, "render_path_device")


def test_header_symbols_exported(bihrt_mod):
    names = bihrt_mod._lib.exported_symbols_from_header()
    L = bihrt_mod._lib.load()
    for sym in ("bih_render_path", "bih_render_path_device", "bih_path_sample"):
        assert sym in names and getattr(L, sym) is not None, sym
    hdr = open(os.path.join(ROOT, "include", "bih.h")).read()
    assert "#define BIH_ABI_VERSION 4" in hdr and "#define BIH_MAX_BOUNCES 8" in hdr
    assert "typedef struct bih_path" in hdr
    assert L.bih_abi_version() == 4


def _header_compiles(tmp_path, cc, std, ext):
    src = tmp_path / ("hdr." + ext)
    src.write_text('#include "bih.h"\n'
                   "int main(void) { bih_path p = {0, 0, 0, 0, 0};\n"
                   "  float n[3] = {0, 0, 1}, d[3]; (void)p; (void)BIH_MAX_BOUNCES;\n"
                   "  return bih_path_sample(1, 0, 0, 1, 0, 2, n, d) == BIH_OK ? 0 : 1; }\n")
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
    I, R, S, Bn = bihrt_mod.Path, bihrt_mod.Rows, bihrt_mod.LightSet, bihrt_mod.Bounce
    sun = (bihrt_mod.Light * 1)()
    sun[0].dir[1], sun[0].weight = 1.0, 1.0
    lamp = (bihrt_mod.PointLight * 1)()
    pan = (bihrt_mod.AreaLight * 1)()
    ps, pl, pp = (C.cast(x, C.c_void_p) for x in (sun, lamp, pan))
    full, empty = S(ps, 1, pl, 1, pp, 1), S(None, 0, None, 0, None, 0)
    bn = Bn(0.5, 0.25)
    rgba, none = I(rgba=base), I()
    for entry in (lambda *a: L.bih_render_path_device(*a, None), L.bih_render_path):
        def call(t, c, w, h, spp, rows, s, b, d, nb=2):
            return entry(t, C.byref(c) if c is not None else None, w, h, spp, 0, SEED,
                         C.byref(rows) if rows is not None else None, C.byref(s) if s is not None else None,
                         C.byref(b) if b is not None else None, nb, C.byref(d) if d is not None else None)
        # 1: the G-buffer's checks, in its order
        assert call(None, cam, 8, 8, 4, None, full, bn, rgba) == INVALID
        assert call(fake, None, 8, 8, 4, None, full, bn, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, None, full, bn, None) == INVALID
        assert call(fake, cam, 0, 8, 4, None, full, bn, rgba) == INVALID
        assert call(fake, cam, 8, 8, 65, None, full, bn, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, None, full, bn, none) == INVALID               # all five planes NULL
        assert call(fake, cam, 8, 8, 4, R(6, 4, 4, 1), full, bn, rgba) == INVALID
        assert call(fake, cam, 1 << 16, 1 << 16, 1, None, S(ps, 65, None, 0, None, 0), None,
                    I(lit=base + 4), 0) == TOO_LARGE                                   # (before 2, 3 and 4)
        # 2: the lights: NULL and empty are legal, the rest as bih_render_area_lights
        assert call(fake, cam, 8, 8, 4, None, S(ps, 33, pl, 31, pp, 1), bn, rgba) == INVALID   # 65 together
        assert call(fake, cam, 8, 8, 4, None, S(ps, 0xFFFFFFFF, pl, 1, pp, 1), bn, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, None, S(ps, 1, pl, 1, pp, 17), bn, rgba) == INVALID    # n_area > 16
        assert call(fake, cam, 8, 8, 4, None, S(None, 1, pl, 1, pp, 1), bn, rgba) == INVALID   # NULL with a count
        assert call(fake, cam, 8, 8, 4, None, S(ps, 1, None, 1, pp, 1), bn, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), S(ps, 1, pl, 1, None, 1), bn, rgba) == INVALID
        # 3: lit's alignment; bounce == NULL; n_bounces; the level planes' alignments
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, bn, I(lit=base + 4, rgba=base)) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, None, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), None, None, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, bn, rgba, 0) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, bn, rgba, MAXB + 1) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, bn, rgba, 0xFFFFFFFF) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, bn, I(lits=base + 4, rgba=base)) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, bn, I(bounces=base + 8)) == INVALID
        # 4: nothing to do -- each single plane, every legal n_bounces, no lights at all
        for d in (I(lit=base), I(bounces=base), I(lits=base + 8), I(irradiance=base + 4), rgba):
            assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, bn, d) == 0
        for nb in range(1, MAXB + 1):
            assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, bn, rgba, nb) == 0
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), None, bn, rgba) == 0
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), empty, bn, rgba) == 0
        assert call(fake, cam, 8, 8, 64, R(3, 0, 0, 0), S(ps, 46, pl, 2, pp, 16), bn, rgba, MAXB) == 0


def test_path_sample_equals_the_hash(bihrt_mod):
    """bih_path_sample is the header's B_k on bits for levels 1 .. 8 over
    104,000 hashed samples; level 1 is bih_bounce_sample; levels 1 and 2 of one
    sample differ."""
    L = bihrt_mod._lib.load()
    seed, gp, frame, spp, s, fs = (a[:13000] for a in ti._samples())
    nrm = np.array([0.3, -0.5, 0.8], F32)
    nn, d = (C.c_float * 3)(*nrm.tolist()), (C.c_float * 3)()
    fn = L.bih_path_sample
    got = {}
    for level in range(1, MAXB + 1):
        want = np.zeros((gp.shape[0], 3), F32)
        for sd in np.unique(seed):
            m = seed == sd
            want[m] = path_dirs(int(sd), gp[m], fs[m], level, nrm)
        g = np.empty((gp.shape[0], 3), F32)
        for k in range(gp.shape[0]):
            assert fn(int(seed[k]), int(gp[k]), int(frame[k]), int(spp[k]), int(s[k]), level, nn, d) == 0
            g[k] = d[:]
        bad = np.argwhere(canon(g) != canon(want))
        assert bad.size == 0, (level, bad[:4].tolist(), bad.shape[0])
        got[level] = g
    one = np.empty((gp.shape[0], 3), F32)
    for k in range(gp.shape[0]):
        assert L.bih_bounce_sample(int(seed[k]), int(gp[k]), int(frame[k]), int(spp[k]), int(s[k]), nn, d) == 0
        one[k] = d[:]
    assert got[1].tobytes() == one.tobytes()
    for a in range(1, MAXB + 1):
        for b in range(a + 1, MAXB + 1):
            assert (got[a] != got[b]).any(1).all(), (a, b)
    # the Python mirror and the errors
    two = bihrt_mod.path_sample(1984, 77, 1, 4, 2, 2, nrm)
    assert two.dtype == F32 and two.tolist() == path_dirs(1984, np.array([77], U32), np.array([6], U32), 2, nrm)[0].tolist()
    assert bihrt_mod.path_sample(1984, 77, 1, 4, 2, 1, nrm).tolist() == bihrt_mod.bounce_sample(1984, 77, 1, 4, 2, nrm).tolist()
    assert fn(1, 0, 0, 4, 0, 1, None, d) == -1 and fn(1, 0, 0, 4, 0, 1, nn, None) == -1
    assert fn(1, 0, 0, 0, 0, 1, nn, d) == -1 and fn(1, 0, 0, 4, 4, 1, nn, d) == -1 and fn(1, 0, 0, 4, 3, 1, nn, d) == 0
    assert fn(1, 0, 0, 4, 0, 0, nn, d) == -1 and fn(1, 0, 0, 4, 0, MAXB + 1, nn, d) == -1 and fn(1, 0, 0, 4, 0, MAXB, nn, d) == 0
    with pytest.raises(bihrt_mod.BihError):
        bihrt_mod.path_sample(1, 0, 0, 4, 0, 0, nrm)


def test_app_bounces_options(bihrt_mod):
    """--bounces without --bounce, out of range or malformed is an error, before any device is used."""
    from bihrt.app import main
    base = ["--scene", "cornell", "--frames", "1"]
    for extra in (["--bounces", "2"],
                  ["--direct", "d.ppm", "--bounces", "2"],
                  ["--direct", "d.ppm", "--bounce", "0.5", "--bounces", "0"],
                  ["--direct", "d.ppm", "--bounce", "0.5", "--bounces", "9"],
                  ["--direct", "d.ppm", "--bounce", "0.5", "--bounces", "x"]):
        with pytest.raises(SystemExit):
            main(base + extra)


def _build_c(tmp_path) -> str:
    exe = str(tmp_path / "path_smoke")
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
    assert "FAIL" not in r.stdout and r.stdout.count("ok ") == 9, r.stdout


# --- GPU ------------------------------------------------------------------------

CLASSES = [("cornell", "K1"), ("soup3k", "K2"), ("soup20k", "K2")]


def check_class(name, lv):
    """The conditions the classes stand for, on the restatement."""
    nhit, live, esc, lit = counts(lv)
    print(name, "hit samples", nhit, "live", live, "escapes", esc, "lit words", lit)
    if name == "cornell":
        assert min(lit) >= 898, lit
        assert live[7] >= 0.25 * nhit, (live, nhit)
        assert min(esc) >= 50 and min(lit) >= 300, (esc, lit)
    elif name == "soup3k":
        assert live[0] > 0 and 0 in live[:7], live          # every kernel runs on an empty list
    else:
        assert 1 <= live[7] <= 64, live                     # a last level that does not fill one wave


@pytest.mark.gpu
@pytest.mark.parametrize("n_bounces", [1, 2, 3, 8])
@pytest.mark.parametrize("name,kname", CLASSES)
def test_classes(name, kname, n_bounces, gpu, bihrt_mod):
    """fib_lights(2) + the scene's panels, albedo 0.5, sky 0.25 at 48x32x4; 1:
    bih_render_indirect's planes, 2: the first buffer swap, 3: both parities,
    8: the limit.  The five planes on bits."""
    lv = levels_of(name, kname, W, H, SPP, FRAME)
    check_class(name, lv)
    r = renderer(tree(name), name, kname, W, H, SPP)
    dl, lp, pan = lights_of(name)
    assert_planes(dev_path(r, dl, lp, pan, n_bounces, FRAME), planes_of(lv, SPP, n_bounces), f"{name} {kname} {n_bounces}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,kname", CLASSES)
def test_identity_with_indirect(name, kname, gpu, bihrt_mod):
    """n_bounces = 1: all five planes are bih_render_indirect_device's bytes on
    the same tree; lit is bih_render_area_lights' at n_bounces = 3."""
    r = renderer(tree(name), name, kname, W, H, SPP)
    dl, lp, pan = lights_of(name)
    ind = ti.dev_indirect(r, dl, lp, pan, FRAME)
    got = dev_path(r, dl, lp, pan, 1, FRAME)
    assert (ind["bounce"]["prim"] != bihrt_mod.NO_HIT).any() and ind["lit2"].any() and (ind["irradiance"] > 0).any()
    for a, b in zip(NAMES, ti.NAMES):
        assert got[a].tobytes() == ind[b].tobytes(), a
    area = ta.dev_area(r, dl, lp, pan, FRAME)
    assert dev_path(r, dl, lp, pan, 3, FRAME)["lit"].tobytes() == area["lit"].tobytes()


@pytest.mark.gpu
def test_composition(gpu, bihrt_mod):
    """Levels 2 and 3's bounces planes equal bih_trace_device(CLOSEST) on the
    rays restated from the level before, GPU against GPU."""
    import bihrt
    g = tree("soup20k")
    lv = levels_of("soup20k", "K2", W, H, SPP, FRAME)
    r = renderer(g, "soup20k", "K2", W, H, SPP)
    dl, lp, pan = lights_of("soup20k")
    got = dev_path(r, dl, lp, pan, 3, FRAME)
    for k in (2, 3):
        before = lv["alive"][k - 2]
        assert before.sum() >= 100
        want = np.zeros(before.shape[0], bihrt.HIT_DTYPE)
        want["t"], want["prim"] = FLT_MAX, bihrt.NO_HIT
        want[before] = tt.dev_trace(g, bihrt.pack_rays(lv["P"][k - 1][before], lv["B"][k - 1][before], F32(T_LO)),
                                    bihrt.QUERY_CLOSEST)
        assert (want["prim"] != bihrt.NO_HIT).any()
        assert np.array_equal(cplane(got["bounces"][k - 1]), cplane(want)), k


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE)
def test_edge_scenes(name, gpu, bihrt_mod):
    """Every edge scene under K2 at n_bounces = 3, bits only; dodeca is convex
    and one-sided: every path ends at level 1."""
    lv = levels_of(name, "K2", W, H, SPP, FRAME, True, 3)
    assert lv["hit"].any()
    if name == "dodeca":
        assert not lv["alive"][0].any()
    r = renderer(tree(name), name, "K2", W, H, SPP)
    dl, lp, pan = lights_of(name)
    got = dev_path(r, dl, lp, pan, 3, FRAME)
    assert_planes(got, planes_of(lv, SPP, 3), name)
    if name == "dodeca":
        assert (got["bounces"]["prim"] == bihrt_mod.NO_HIT).all() and not got["lits"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,spp", [(1, 1, 1), (37, 29, 3), (8, 8, 64), (16, 8, 16)])
def test_shapes(w, h, spp, gpu, bihrt_mod):
    """One sample; partial tiles and waves with an spp that is no power of two; a pixel per wave; four pixels per wave."""
    lv = levels_of("soup20k", "K2", w, h, spp, 1, True, 2)
    if (w, h) != (1, 1):
        assert lv["alive"][1].any() and (lv["alive"][0] & ~lv["alive"][1]).any() and lv["lits"][1].any()
    r = renderer(tree("soup20k"), "soup20k", "K2", w, h, spp)
    dl, lp, pan = lights_of("soup20k")
    assert_planes(dev_path(r, dl, lp, pan, 2, 1), planes_of(lv, spp, 2), f"{w}x{h}x{spp}")


@pytest.mark.gpu
def test_more_hit_samples_than_the_persistent_grid(gpu, bihrt_mod):
    """A frame whose hit samples exceed the persistent grid x 64 lanes, so that
    the walk's waves come back for more at n_bounces = 3: its planes equal the
    same frame assembled from bands of 32 rows, each far below the grid (gp is
    global, so bands reassemble), and sampled rows equal the restatement.
    (768 x 576: at 768 x 512 soup20k's 511,255 hit samples stay 2.5 % below the
    256 x 32 x 64 lanes of an MI355X's grid.)"""
    import torch
    w, h, spp = 768, 576, 4
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    g = tree("soup20k")
    r = renderer(g, "soup20k", "K2", w, h, spp)
    dl, lp, pan = lights_of("soup20k")
    nhit = int((tg.dev_gbuffer(r, FRAME)["hits"]["prim"] != bihrt_mod.NO_HIT).sum())
    assert nhit > cus * 32 * 64, (nhit, cus)
    full = dev_path(r, dl, lp, pan, 3, FRAME)
    assert (full["bounces"][2]["prim"] != bihrt_mod.NO_HIT).any() and full["lits"][2].any()
    band = 32
    assert w * band * spp < cus * 32 * 64
    for y0 in range(0, h, band):
        part = dev_path(r, dl, lp, pan, 3, FRAME, bihrt_mod.Rows(y0, band, band, 1))
        want = rows_of(full, w, spp, list(range(y0, y0 + band)))
        for k in NAMES:
            assert part[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), (k, y0)
    # sampled rows against the restatement: the header's levels of those rows alone
    ys = [3, 287, 288, 573]
    sub = restate_rows("soup20k", "K2", w, h, spp, FRAME, ys, 3)
    assert sub["bounces"].shape == (3, len(ys) * w * spp) and (sub["bounces"][2]["prim"] != bihrt_mod.NO_HIT).any()
    assert_planes(rows_of(full, w, spp, ys), sub, "sampled rows")


def restate_rows(name, kname, w, h, spp, frame, ys, n_bounces):
    """planes_of for the global rows ys of a frame too large to restate whole:
    the primary hits of those rows from the oracle's closest walk, then the
    levels with the rows' global pixels."""
    import bihrt
    import oracle
    tris, ot = scene(name)
    cam = camera(name, kname, w, h)
    r = np.stack([np.stack([oracle.rng_uniforms(SEED, y * w + x, 2 * spp, skip=2 * spp * frame) for x in range(w)])
                  for y in ys]).astype(F32)                         # (rows, w, 2*spp): frame_rays' draws
    xs = np.arange(w, dtype=F32)[None, :, None]
    yy = np.asarray(ys, F32)[:, None, None]
    u = (xs + r[:, :, 0::2]) / F32(w)
    v = (yy + r[:, :, 1::2]) / F32(h)
    d = np.stack([((cam[3 + a] + u * cam[6 + a]) + v * cam[9 + a]) - cam[a] for a in range(3)], -1).reshape(-1, 3)
    assert d.dtype == F32
    n = d.shape[0]
    o = np.broadcast_to(cam[0:3], (n, 3)).astype(F32)
    t, idx = np.empty(n, F32), np.empty(n, np.int64)
    for k in range(n):
        t[k], idx[k] = ot.closest(o[k], d[k], 0.0)
    hit = idx >= 0
    dl, lp, pan = lights_of(name)
    pan = bihrt.pack_area_lights(pan)
    occluded, segment = td.oracle_occluded(ot), tl.oracle_segment(ot)
    closest = ti.oracle_closest(name)
    gp = np.concatenate([(y * w + np.arange(w * spp) // spp) for y in ys]).astype(U32)
    fs = ((frame * spp + np.arange(n) % spp) & 0xFFFFFFFF).astype(U32)
    lv = {"hit": hit, "bounces": [], "lits": [], "e": [], "alive": []}
    with np.errstate(all="ignore"):
        P = cam[0:3][None, :] + t[:, None] * d
        nrm = np.zeros((n, 3), F32)
        nrm[hit] = normals(tris[ot.tri_idx[idx[hit]]])
        lv["lit"], lv["e0"] = ti.light_level(P, nrm, hit, dl, np.zeros(0, bihrt.POINT_LIGHT_DTYPE), pan, occluded,
                                             segment, SEED, gp, fs)
        alive = hit
        for k in range(1, n_bounces + 1):
            B = path_dirs(SEED, gp, fs, k, nrm)
            rec = np.zeros(n, bihrt.HIT_DTYPE)
            rec["t"], rec["prim"] = FLT_MAX, bihrt.NO_HIT
            if alive.any():
                rec[alive] = closest(P[alive], B[alive])
            alive = rec["prim"] != bihrt.NO_HIT
            P = P + rec["t"][:, None] * B
            nrm = np.zeros((n, 3), F32)
            nrm[alive] = normals(tris[rec["prim"][alive]])
            lits, e = ti.light_level(P, nrm, alive, dl, np.zeros(0, bihrt.POINT_LIGHT_DTYPE), pan, occluded, segment,
                                     SEED, gp, fs)
            lv["bounces"].append(rec)
            lv["lits"].append(lits)
            lv["e"].append(e)
            lv["alive"].append(alive)
    out = planes_of(lv, spp, n_bounces)
    out["irradiance"], out["rgba"] = out["irradiance"].reshape(len(ys), w), out["rgba"].reshape(len(ys), w)
    return out


@pytest.mark.gpu
def test_two_stack_slots(gpu, bihrt_mod):
    """soup20k at n_bounces = 3 with two stack slots on chip (the spill stack is used)."""
    lv = levels_of("soup20k", "K2", W, H, SPP, FRAME)
    g = tree("soup20k")
    r = renderer(g, "soup20k", "K2", W, H, SPP)
    dl, lp, pan = lights_of("soup20k")
    g.set_param(bihrt_mod.PARAM_TRACE_LDS_SLOTS, 2)
    try:
        assert_planes(dev_path(r, dl, lp, pan, 3, FRAME), planes_of(lv, SPP, 3), "2 slots")
    finally:
        g.set_param(bihrt_mod.PARAM_TRACE_LDS_SLOTS, 0)


@pytest.mark.gpu
def test_rows_bands_planes_and_host_entry(gpu, bihrt_mod):
    """Interleaved bands and rows that are not tile-aligned equal the same rows
    of the full frame, through both entries; each plane alone gives the bits of
    all together and leaves the others untouched (prefilled with 0xAB); no call
    after the first of the shape allocates."""
    nb = 3
    exp = planes_of(levels_of("soup20k", "K2", W, H, SPP, FRAME), SPP, nb)
    g = tree("soup20k")
    r = renderer(g, "soup20k", "K2", W, H, SPP)
    dl, lp, pan = lights_of("soup20k")
    host = r.render_path(dl, lp, pan, (ALBEDO, SKY), nb, FRAME)
    assert sorted(host) == sorted(NAMES) and host["bounces"].shape == (nb, W * H * SPP)
    assert host["lits"].shape == (nb, W * H * SPP) and host["rgba"].shape == (H, W)
    assert_planes(host, exp, "host entry")
    for name in NAMES:                       # (first: a call without lit / lits grows the tree's own words)
        got = dev_path(r, dl, lp, pan, nb, FRAME, names=(name,))
        assert_planes(got, exp, f"{name} alone", names=(name,))
        for other in NAMES:
            if other != name:
                assert (np.ascontiguousarray(got[other]).view(np.uint8) == 0xAB).all(), (name, other)
    first = g.info()
    for rows, ys in ((bihrt_mod.Rows(4, 8, 4, 2), [4, 5, 6, 7, 12, 13, 14, 15]),
                     (bihrt_mod.Rows(5, 7, 7, 1), list(range(5, 12)))):
        sub = rows_of(exp, W, SPP, ys)
        assert (sub["bounces"][nb - 1]["prim"] != bihrt_mod.NO_HIT).any() and (sub["lits"][1] != 0).any()
        assert_planes(dev_path(r, dl, lp, pan, nb, FRAME, rows), sub, f"rows {ys[0]}..")
        assert_planes(r.render_path(dl, lp, pan, (ALBEDO, SKY), nb, FRAME, rows), sub, "host entry rows")
    for name in NAMES:
        assert_planes(dev_path(r, dl, lp, pan, nb, FRAME, names=(name,)), exp, f"{name} alone", names=(name,))
    assert_planes(r.render_path(dl, lp, pan, (ALBEDO, SKY), nb, FRAME, planes=("irradiance",)), exp, "host, one plane",
                  names=("irradiance",))
    after = g.info()
    assert after.device_allocs == first.device_allocs and after.device_bytes == first.device_bytes


@pytest.mark.gpu
@pytest.mark.parametrize("n_bounces", [1, 3, 8])
def test_sky_only(n_bounces, gpu, bihrt_mod):
    """No lights, albedo 1, sky 0.25: irradiance is exactly 0.25 x (paths that
    escape at a level <= n_bounces) / spp, counted from the restated bounces."""
    lv = levels_of("soup20k", "K2", W, H, SPP, FRAME, False)
    exp = planes_of(lv, SPP, n_bounces, 1.0, 0.25)
    esc = (lv["hit"] & ~lv["alive"][n_bounces - 1]).reshape(-1, SPP).sum(1)
    assert np.array_equal(exp["irradiance"], F32(0.25) * esc.astype(F32) / F32(SPP)) and (esc > 0).any() and (esc < SPP).any()
    assert not exp["lit"].any() and not exp["lits"].any()
    r = renderer(tree("soup20k"), "soup20k", "K2", W, H, SPP)
    got = dev_path(r, None, None, None, n_bounces, FRAME, bounce=(1.0, 0.25))
    assert_planes(got, exp, "sky only")
    assert np.array_equal(got["irradiance"].reshape(-1), F32(0.25) * esc.astype(F32) / F32(SPP))


@pytest.mark.gpu
def test_frames(gpu, bihrt_mod):
    """Frames 0, 1 and 2 give different bounce records at every level, each the restatement's."""
    ls = [levels_of("soup20k", "K2", W, H, SPP, f, True, 3) for f in (0, 1, 2)]
    for k in range(3):
        assert not np.array_equal(ls[0]["bounces"][k], ls[1]["bounces"][k])
        assert not np.array_equal(ls[1]["bounces"][k], ls[2]["bounces"][k])
    r = renderer(tree("soup20k"), "soup20k", "K2", W, H, SPP)
    dl, lp, pan = lights_of("soup20k")
    for f in (0, 1, 2, 1):
        assert_planes(dev_path(r, dl, lp, pan, 3, f), planes_of(ls[f], SPP, 3), f"frame {f}")


@pytest.mark.gpu
def test_renders_undisturbed(gpu, bihrt_mod):
    """render f=0, path f=2, render f=2, indirect f=2, render f=3, path f=3:
    every image is the oracle's, the indirect call before and after is the same
    and every plane is right (no level takes an XORWOW draw)."""
    tris, ot = scene("cornell")
    cam = camera("cornell", "K1", W, H)
    g = bihrt_mod.GPUArrayManager(tris)
    r = renderer(g, "cornell", "K1", W, H, SPP)
    dl, lp, pan = lights_of("cornell")
    i_before = r.render_indirect(dl, lp, pan, (ALBEDO, SKY), 2)
    f0 = r.render(0)
    d2 = r.render_path(dl, lp, pan, (ALBEDO, SKY), 3, 2)
    f2 = r.render(2)
    i_after = r.render_indirect(dl, lp, pan, (ALBEDO, SKY), 2)
    f3 = r.render(3)
    d3 = r.render_path(dl, lp, pan, (ALBEDO, SKY), 2, 3)
    assert r.frame == 4
    for f, img in ((0, f0), (2, f2), (3, f3)):
        assert np.array_equal(img, ot.render(W, H, spp=SPP, frame=f, seed=SEED, cam=cam)[0]), f
    for name in ti.NAMES:
        assert i_before[name].tobytes() == i_after[name].tobytes(), name
    ti.assert_planes(i_after, ti.expect("cornell", "K1", W, H, SPP, 2), "indirect, frame 2")
    assert_planes(d2, planes_of(levels_of("cornell", "K1", W, H, SPP, 2, True, 3), SPP, 3), "frame 2")
    assert_planes(d3, planes_of(levels_of("cornell", "K1", W, H, SPP, 3, True, 3), SPP, 2), "frame 3")
    g.close()


@pytest.mark.gpu
def test_rebuild_ordering_and_two_streams(gpu, bihrt_mod):
    """Two calls of one tree back to back on two streams with different frames
    and depths; then a call on a second stream after rebuild() sees the new
    soup's tree."""
    import torch
    old, new = scene("soup3k")[0], scene("soup3k2")[0]
    soup = torch.from_numpy(old.copy()).cuda()
    torch.cuda.synchronize()
    g = bihrt_mod.GPUArrayManager.from_device(soup.data_ptr(), old.shape[0])
    ea = planes_of(levels_of("soup3k", "K2", W, H, SPP, 1, True, 3), SPP, 3)
    eb = planes_of(levels_of("soup3k", "K2", W, H, SPP, 2, True, 3), SPP, 2)
    e1 = planes_of(levels_of("soup3k2", "K2", W, H, SPP, 1, True, 3), SPP, 3)
    assert not np.array_equal(ea["bounces"], e1["bounces"])
    r0, r1 = renderer(g, "soup3k", "K2", W, H, SPP), renderer(g, "soup3k2", "K2", W, H, SPP)
    da, db, dc, d1 = Dev(H, W, SPP, 3), Dev(H, W, SPP, 2), Dev(H, W, SPP, 3), Dev(H, W, SPP, 3)
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
    """tests/c/path_smoke.c -- bih_build + bih_render_path from strict C11
    (cornell, 64x48, the reference camera, a sky, lamps and the ceiling panel,
    3 bounces): render_path's planes."""
    exe = _build_c(tmp_path)
    tris = scene("cornell")[0]
    w, h, spp, nb = 64, 48, 4, 3
    dl, pl, al = bihrt_mod.scenes.sky_dome(2), lamps_of("cornell", 2), bihrt_mod.scenes.cornell_panel(4.0)
    sp, lp, pp, ap, op = (tmp_path / n for n in ("scene.f32", "dir.f32", "lamps.f32", "area.f32", "planes.bin"))
    tris.tofile(sp)
    dl.tofile(lp)
    pl.tofile(pp)
    al.tofile(ap)
    r = subprocess.run([exe, str(sp), str(tris.shape[0]), str(w), str(h), str(spp), "0", str(lp), str(dl.shape[0]),
                        str(pp), str(pl.shape[0]), str(ap), str(al.shape[0]), "0.5", "0.25", str(nb), str(op)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "path_smoke OK" in r.stdout, r.stdout + r.stderr
    ref = bihrt_mod.Renderer(tree("cornell"), w, h, spp=spp).render_path(dl, pl, al, (0.5, 0.25), nb, 0)
    assert ref["lits"][nb - 1].any() and (ref["bounces"][nb - 1]["prim"] != bihrt_mod.NO_HIT).any()
    raw = np.fromfile(op, np.uint8)
    P = w * h
    assert raw.size == P * (8 * spp + 24 * spp * nb + 8)
    off = 0
    for name, size in (("lit", 8 * spp), ("bounces", 16 * spp * nb), ("lits", 8 * spp * nb), ("irradiance", 4),
                       ("rgba", 4)):
        part = raw[off:off + P * size]
        off += P * size
        assert np.array_equal(part, np.ascontiguousarray(ref[name]).view(np.uint8).reshape(-1)), name


@pytest.mark.gpu
def test_app_writes_ppm(tmp_path, gpu, bihrt_mod):
    """python -m bihrt --direct --bounce --bounces: the PPM of render_path's rgba
    plane with the panel and a lamp; without --bounces it is render_indirect's."""
    from bihrt.app import main
    want = tmp_path / "want.ppm"
    rr = bihrt_mod.Renderer(tree("cornell"), 64, 48)
    panel = np.array([[0.1, 0.98, 1.0, 0.6, 0, 0, 0, 0, 0.6, 4.0]], F32)
    lamp = np.array([[0.0, 0.5, 0.0, 1.0]], F32)
    common = ["--scene", "cornell", "--width", "64", "--height", "48", "--frames", "1", "--sky", "0", "--lamp",
              "0,0.5,0", "--panel", "0.1,0.98,1,0.6,0,0,0,0,0.6,4", "--bounce", "0.5,0.25"]
    shades = {}
    for nb in (None, 1, 4):
        dr = tmp_path / ("d%s.ppm" % nb)
        assert main(common + ["--direct", str(dr)] + (["--bounces", str(nb)] if nb else [])) == 0
        if nb:
            ref = rr.render_path(None, lamp, panel, (0.5, 0.25), nb, 0, planes=("rgba",))["rgba"]
        else:
            ref = rr.render_indirect(None, lamp, panel, (0.5, 0.25), 0, planes=("rgba",))["rgba"]
        bihrt_mod.write_ppm(str(want), ref)
        shades[nb] = open(dr, "rb").read()
        assert shades[nb] == open(want, "rb").read(), nb
        assert np.unique(bihrt_mod.unpack_rgba(ref)[..., 0]).size > 2
    assert shades[None] == shades[1] and shades[1] != shades[4]
