"""Mirror materials (bih_material.kind, bih_render_path_spec /
bih_render_path_spec_device): bih_render_path_rgb with
a material kind that steers the path -- a sample that lands on a
BIH_MAT_MIRROR material goes on along the reflection of the ray that found it
and gathers no light there.

Expected values come from the oracle alone: test_path.restate_levels carried on
with the incoming direction D, the level's ray picked per sample (the
reflection R behind a mirror hit, test_path.path_dirs behind a diffuse one),
mirror hits masked out of test_indirect.light_level's `on`, then
test_path_rgb.planes_rgb's accumulation.  Planes are compared on bits, NaN as
NaN (test_indirect.cplane).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_direct as td
import test_gbuffer as tg
import test_indirect as ti
import test_lights as tl
import test_path as tp
import test_path_rgb as trgb
from conftest import ROOT
from test_area_lights import U32
from test_gbuffer import EDGE, F32, LIBDIR, SEED, camera, expected, frame_rays, normals, renderer, scene, tree
from test_indirect import FLT_MAX, cplane, lights_of
from test_lights import NO_DIR
from test_path import CLASSES, FRAME, H, MAXB, SPP, W
from test_path_rgb import NAMES, SKY3, assert_planes, ids_of, planes_rgb, rows_of

SRC = os.path.join(ROOT, "tests", "c", "path_spec_smoke.c")
DIFFUSE, MIRROR = 0, 1
MIRROR_MATERIAL = 2          # the fixture: test_path_rgb's five materials, this one a mirror


def palette(kinds="fixture"):
    """test_path_rgb's palette with material 2 a mirror ("fixture"), every kind
    zeroed ("zero"), every material a mirror ("mirror"), or material 2 of kind 2 ("bad")."""
    pal = trgb.palette().copy()
    pal["kind"] = {"fixture": [0, 0, 1, 0, 0], "zero": [0] * 5, "mirror": [1] * 5, "bad": [0, 0, 2, 0, 0]}[kinds]
    return pal


# --- the header, restated ---------------------------------------------------------

def reflect(D, nrm):
    """R (n, 3) f32: dn = (D.x*n.x + D.y*n.y) + D.z*n.z; k2 = 2*dn; R[c] = D[c] - k2*n[c]; and dn."""
    with np.errstate(all="ignore"):
        dn = (D[:, 0] * nrm[:, 0] + D[:, 1] * nrm[:, 1]) + D[:, 2] * nrm[:, 2]
        k2 = F32(2.0) * dn
        R = D - k2[:, None] * nrm
    assert R.dtype == F32 and dn.dtype == F32
    return R, dn


def restate_spec(name, kname, w, h, spp, frame, dir_lights, lamps, panels, tri_kind, levels=MAXB, seed=SEED):
    """test_path.restate_levels with a kind per file-order triangle (tri_kind):
    the same keys, the rays "B" being the reflection behind a mirror hit, and
    "kind0", "prim0" of level 0, the list "kind" (index k-1 = level k: the kind
    of the level's hit, 0 where there is none), "dn" (index k = level k: D_k . n_k)."""
    import bihrt
    tris, ot = scene(name)
    cam = camera(name, kname, w, h)
    D = np.ascontiguousarray(frame_rays(cam, w, h, spp, frame).reshape(-1, 3), F32)
    hits = expected(name, kname, w, h, spp, frame)["hits"]
    dl = dir_lights if dir_lights is not None else NO_DIR
    lp = lamps if lamps is not None else np.zeros(0, bihrt.POINT_LIGHT_DTYPE)
    pan = bihrt.pack_area_lights(panels if panels is not None else np.zeros((0, 10), F32))
    occluded, segment = td.oracle_occluded(ot), tl.oracle_segment(ot)
    closest = ti.oracle_closest(name)
    tri_kind = np.asarray(tri_kind, np.uint32)
    n = hits.shape[0]
    hit = hits["prim"] != bihrt.NO_HIT
    gp = (np.arange(n) // spp).astype(U32)
    fs = ((frame * spp + np.arange(n) % spp) & 0xFFFFFFFF).astype(U32)
    out = {"hit": hit, "prim0": hits["prim"], "bounces": [], "lits": [], "e": [], "alive": [], "P": [], "B": [],
           "kind": [], "dn": []}
    with np.errstate(all="ignore"):
        P = cam[0:3][None, :] + hits["t"][:, None] * D
        nrm = np.zeros((n, 3), F32)
        nrm[hit] = normals(tris[hits["prim"][hit]])
        kind = np.where(hit, tri_kind[np.where(hit, hits["prim"], 0)], 0).astype(np.uint32)
        out["kind0"] = kind
        out["lit"], out["e0"] = ti.light_level(P, nrm, hit & (kind != MIRROR), dl, lp, pan, occluded, segment, seed,
                                               gp, fs)
        alive, prim = hit, hits["prim"]
        for k in range(1, levels + 1):
            R, dn = reflect(D, nrm)
            B = np.where((kind == MIRROR)[:, None], R, tp.path_dirs(seed, gp, fs, k, nrm))
            assert B.dtype == F32
            rec = np.zeros(n, bihrt.HIT_DTYPE)
            rec["t"], rec["prim"] = FLT_MAX, bihrt.NO_HIT
            if alive.any():
                rec[alive] = closest(P[alive], B[alive])
            stopped = rec["prim"] != bihrt.NO_HIT
            assert not (stopped & ~alive).any()
            mir = alive & (kind == MIRROR)
            assert not (mir & stopped & (rec["prim"] == prim)).any(), "a reflected ray stopped on its own triangle"
            out["P"].append(P)
            out["B"].append(B)
            out["dn"].append(np.where(alive, dn, F32(0)))
            P = P + rec["t"][:, None] * B
            D = B
            nrm = np.zeros((n, 3), F32)
            nrm[stopped] = normals(tris[rec["prim"][stopped]])
            kind = np.where(stopped, tri_kind[np.where(stopped, rec["prim"], 0)], 0).astype(np.uint32)
            lits, e = ti.light_level(P, nrm, stopped & (kind != MIRROR), dl, lp, pan, occluded, segment, seed, gp, fs)
            assert P.dtype == F32 and e.dtype == F32
            out["bounces"].append(rec)
            out["lits"].append(lits)
            out["e"].append(e)
            out["alive"].append(stopped)
            out["kind"].append(kind)
            alive, prim = stopped, rec["prim"]
        out["dn"].append(np.where(alive, reflect(D, nrm)[1], F32(0)))
    for v in out.values():
        for a in (v if isinstance(v, list) else [v]):
            a.setflags(write=False)
    return out


_levels = {}


def levels_of(name, kname, w, h, spp, frame, kinds="fixture", lit=True, levels=MAXB):
    """restate_spec under fib_lights(2) + panels_of(name) (lit False: no lights)
    with triangle i's material i % 5 of palette(kinds); read-only, computed once
    (a deeper restatement serves a shallower request)."""
    key = (name, kname, w, h, spp, frame, kinds, lit)
    if key not in _levels or len(_levels[key]["alive"]) < levels:
        dl, lp, pan = lights_of(name) if lit else (None, None, None)
        tri_kind = palette(kinds)["kind"][ids_of(scene(name)[0].shape[0])]
        _levels[key] = restate_spec(name, kname, w, h, spp, frame, dl, lp, pan, tri_kind, levels)
    return _levels[key]


def expect(name, kname, w, h, spp, frame, n_bounces, kinds="fixture", lit=True, sky=SKY3, levels=MAXB):
    lv = levels_of(name, kname, w, h, spp, frame, kinds, lit, max(levels, n_bounces))
    return planes_rgb(lv, lv["prim0"], spp, n_bounces, palette(kinds), ids_of(scene(name)[0].shape[0]), sky)


def counts(lv):
    """(mirror hits at level 0, at levels >= 1, mirror hits followed by another
    mirror hit, mirror hits whose reflected ray escapes, mirror hits followed by
    a diffuse hit with a non-zero lit word), levels 1 .. 8 summed."""
    kinds = [lv["kind0"]] + list(lv["kind"])
    alive = [lv["hit"]] + list(lv["alive"])
    m0 = int((alive[0] & (kinds[0] == MIRROR)).sum())
    deeper = sum(int((alive[k] & (kinds[k] == MIRROR)).sum()) for k in range(1, len(kinds)))
    chain = esc = lit = 0
    for k in range(1, len(kinds)):
        before = alive[k - 1] & (kinds[k - 1] == MIRROR)
        chain += int((before & alive[k] & (kinds[k] == MIRROR)).sum())
        esc += int((before & ~alive[k]).sum())
        lit += int((before & alive[k] & (kinds[k] == DIFFUSE) & (lv["lits"][k - 1] != 0)).sum())
    return m0, deeper, chain, esc, lit


def check_class(name, kname):
    """The conditions the fixture stands for, on the restatement: a fixture that
    stops exercising the feature fails here."""
    lv = levels_of(name, kname, W, H, SPP, FRAME)
    m0, deeper, chain, esc, lit = counts(lv)
    print(name, "mirror hits at level 0", m0, "at levels >= 1", deeper, "mirror to mirror", chain,
          "reflected rays that escape", esc, "lit diffuse successors", lit)
    assert m0 >= 100 and deeper >= 20 and esc >= 100 and lit >= 20, (m0, deeper, esc, lit)
    if name in ("cornell", "soup20k"):
        assert chain >= 20, chain
    kinds = [lv["kind0"]] + list(lv["kind"])
    alive = [lv["hit"]] + list(lv["alive"])
    for k in range(len(kinds)):
        on = alive[k] & (kinds[k] == MIRROR)
        assert not (lv["dn"][k][on] >= 0).any(), f"an accepted mirror hit with dn >= 0 at level {k}"
    assert np.isfinite(expect(name, kname, W, H, SPP, FRAME, MAXB)["acc"]).all()


class Dev(trgb.Dev):
    """test_path_rgb.Dev, launching the mirror call (spec False: the colour call)."""

    def __init__(self, *a, spec=True, **kw):
        super().__init__(*a, **kw)
        self.spec = spec

    def launch(self, r, dl, lp, pan, sky, frame, rows=None, stream=None):
        call = r.render_path_spec_device if self.spec else r.render_path_rgb_device
        call({k: self.t[k].data_ptr() for k in self.names}, dl, lp, pan, sky, self.nb, frame, rows, stream)


def dev_spec(r, dl, lp, pan, n_bounces, frame, rows=None, names=NAMES, sky=SKY3, spec=True):
    nrows = rows.nrows if rows is not None else r.h
    dv = Dev(nrows, r.w, r.spp, n_bounces, names, spec=spec)
    dv.launch(r, dl, lp, pan, sky, frame, rows)
    r.sync()
    return dv.result()


def with_materials(name, kinds="fixture"):
    """The scene's shared tree with palette(kinds), triangle i material i % 5."""
    g = tree(name)
    g.set_materials(palette(kinds), ids_of(scene(name)[0].shape[0]))
    return g


def same(a, b, what=""):
    for k in NAMES:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.fixture(scope="module", autouse=True)
def _free_trees():
    yield
    while tg._trees:
        tg._trees.popitem()[1].close()


# --- CPU ------------------------------------------------------------------------

def test_layouts(bihrt_mod):
    M, dt = bihrt_mod.Material, bihrt_mod.MATERIAL_DTYPE
    assert C.sizeof(M) == 32 and M.kind.offset == 12 and M.kind.size == 4 and M.reserved0.offset == 12
    assert M.albedo.offset == 0 and M.emission.offset == 16 and M.reserved1.offset == 28
    assert dt.itemsize == 32 and dt.fields["kind"][0] == np.uint32 and dt.fields["kind"][1] == 12
    assert dt.fields["reserved0"][1] == 12 and dt.fields["albedo"][1] == 0 and dt.fields["emission"][1] == 16
    assert dt.fields["reserved1"][1] == 28
    assert bihrt_mod.MAT_DIFFUSE == 0 and bihrt_mod.MAT_MIRROR == 1
    for name in ("MAT_DIFFUSE", "MAT_MIRROR"):
        assert name in bihrt_mod.__all__, name
    for name in ("render_path_spec", "render_path_spec_device"):
        assert hasattr(bihrt_mod.Renderer, name), name
    six = bihrt_mod.pack_materials([(1, 2, 3, 4, 5, 6)])
    assert six.dtype == dt and six.view(F32).tolist() == [1, 2, 3, 0, 4, 5, 6, 0] and six["kind"].tolist() == [0]
    seven = bihrt_mod.pack_materials([(1, 2, 3, 4, 5, 6, 1), (.5, .5, .5, 0, 0, 0, 0)])
    assert seven["kind"].tolist() == [1, 0] and seven.view(np.uint32)[3] == 1 and seven.view(np.uint32)[11] == 0
    assert seven.view(F32)[[0, 1, 2, 4, 5, 6, 7]].tolist() == [1, 2, 3, 4, 5, 6, 0]
    assert bihrt_mod.pack_materials(seven).tobytes() == seven.tobytes()
    m = M()
    m.kind = 1
    assert bytes(m)[12:16] == b"\x01\x00\x00\x00"
    assert palette()["kind"].tolist() == [0, 0, 1, 0, 0] and palette().view(F32).reshape(5, 8)[:, :3].tolist() == \
        trgb.palette()["albedo"].tolist()


def test_header_symbols_exported(bihrt_mod):
    names = bihrt_mod._lib.exported_symbols_from_header()
    L = bihrt_mod._lib.load()
    for sym in ("bih_render_path_spec", "bih_render_path_spec_device"):
        assert sym in names and getattr(L, sym) is not None, sym
    hdr = open(os.path.join(ROOT, "include", "bih.h")).read()
    assert "#define BIH_ABI_VERSION 4" in hdr and "#define BIH_MAT_DIFFUSE 0u" in hdr
    assert "#define BIH_MAT_MIRROR  1u" in hdr and "union { float reserved0; uint32_t kind; }" in hdr
    assert "Materials and sky never\n *    steer a path" in hdr          # bih_render_path_rgb's guarantee stands
    assert L.bih_abi_version() == 4


def _header_compiles(tmp_path, cc, std, ext):
    src = tmp_path / ("hdr." + ext)
    src.write_text('#include "bih.h"\n'
                   "int main(void) { bih_material m = {{1, 1, 1}, 0, {0, 0, 0}, 0};\n"
                   "  bih_path_rgb p = {0, 0, 0, 0, 0}; float sky[3] = {0, 0, 0}; (void)BIH_MAT_DIFFUSE;\n"
                   "  if (m.kind != BIH_MAT_DIFFUSE) return 1;\n"
                   "  m.kind = BIH_MAT_MIRROR;\n"
                   "  return bih_render_path_spec(0, 0, 1, 1, 1, 0, 1, 0, 0, sky, 1, &p) == BIH_ERR_INVALID &&\n"
                   "         sizeof m == 32 && sizeof m.kind == 4 ? 0 : 1; }\n")
    subprocess.run([cc, "-std=" + std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only",
                    "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_header_is_c11_and_cxx17(tmp_path):
    _header_compiles(tmp_path, "gcc", "c11", "c")
    _header_compiles(tmp_path, "g++", "c++17", "cpp")


def test_device_free_error_codes(bihrt_mod):
    """bih_render_path_rgb's checks in its order, before the tree or a device is
    touched: a stand-in tree pointer is never dereferenced."""
    L = bihrt_mod._lib.load()
    INVALID, TOO_LARGE = -1, -6
    raw = (C.c_char * 96)()
    base = (C.addressof(raw) + 15) & ~15
    fake = C.c_void_p(base)
    cam = bihrt_mod.Camera()
    I, R, S = bihrt_mod.PathRgb, bihrt_mod.Rows, bihrt_mod.LightSet
    sun = (bihrt_mod.Light * 1)()
    sun[0].dir[1], sun[0].weight = 1.0, 1.0
    lamp = (bihrt_mod.PointLight * 1)()
    pan = (bihrt_mod.AreaLight * 1)()
    ps, pl, pp = (C.cast(x, C.c_void_p) for x in (sun, lamp, pan))
    full, empty = S(ps, 1, pl, 1, pp, 1), S(None, 0, None, 0, None, 0)
    sky = (C.c_float * 3)(*SKY3)
    rgba, none = I(rgba=base), I()
    for entry in (lambda *a: L.bih_render_path_spec_device(*a, None), L.bih_render_path_spec):
        def call(t, c, w, h, spp, rows, s, sk, d, nb=2):
            return entry(t, C.byref(c) if c is not None else None, w, h, spp, 0, SEED,
                         C.byref(rows) if rows is not None else None, C.byref(s) if s is not None else None,
                         sk, nb, C.byref(d) if d is not None else None)
        # 1: the G-buffer's checks, in its order
        assert call(None, cam, 8, 8, 4, None, full, sky, rgba) == INVALID
        assert call(fake, None, 8, 8, 4, None, full, sky, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, None, full, sky, None) == INVALID
        assert call(fake, cam, 0, 8, 4, None, full, sky, rgba) == INVALID
        assert call(fake, cam, 8, 8, 65, None, full, sky, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, None, full, sky, none) == INVALID               # all five planes NULL
        assert call(fake, cam, 8, 8, 4, R(6, 4, 4, 1), full, sky, rgba) == INVALID
        assert call(fake, cam, 1 << 16, 1 << 16, 1, None, S(ps, 65, None, 0, None, 0), None,
                    I(lit=base + 4), 0) == TOO_LARGE                                   # (before 2, 3 and 4)
        # 2: the lights
        assert call(fake, cam, 8, 8, 4, None, S(ps, 33, pl, 31, pp, 1), sky, rgba) == INVALID   # 65 together
        assert call(fake, cam, 8, 8, 4, None, S(ps, 1, pl, 1, pp, 17), sky, rgba) == INVALID    # n_area > 16
        assert call(fake, cam, 8, 8, 4, None, S(None, 1, pl, 1, pp, 1), sky, rgba) == INVALID   # NULL with a count
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), S(ps, 1, pl, 1, None, 1), sky, rgba) == INVALID
        # 3: lit's alignment; sky == NULL; n_bounces; the level planes' alignments
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, sky, I(lit=base + 4, rgba=base)) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, None, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, sky, rgba, 0) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, sky, rgba, MAXB + 1) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, sky, I(lits=base + 4, rgba=base)) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, sky, I(bounces=base + 8)) == INVALID
        # 4: nothing to do: the tree (no tree at all) is never dereferenced
        for d in (I(lit=base), I(bounces=base), I(lits=base + 8), I(radiance=base + 4), rgba):
            assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, sky, d) == 0
        for nb in range(1, MAXB + 1):
            assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, sky, rgba, nb) == 0
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), None, sky, rgba) == 0
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), empty, sky, rgba) == 0
        assert call(fake, cam, 8, 8, 64, R(3, 0, 0, 0), S(ps, 46, pl, 2, pp, 16), sky, rgba, MAXB) == 0


def test_app_mirror_options(bihrt_mod):
    """--mirror without --colour (or with a --colour that is itself an error) is
    an error, before any device is used."""
    from bihrt.app import main
    base = ["--scene", "cornell", "--frames", "1"]
    for extra in (["--mirror"],
                  ["--direct", "d.ppm", "--mirror"],
                  ["--direct", "d.ppm", "--bounce", "0.5", "--bounces", "2", "--mirror"],
                  ["--direct", "d.ppm", "--bounce", "0.5", "--colour", "--mirror"]):
        with pytest.raises(SystemExit):
            main(base + extra)
    with pytest.raises(SystemExit):
        main(["--scene", "torus", "--frames", "1", "--direct", "d.ppm", "--bounce", "0.5", "--bounces", "2",
              "--colour", "--mirror"])


def test_cornell_mirror_materials(bihrt_mod):
    pal, ids = bihrt_mod.scenes.cornell_mirror_materials()
    base, base_ids = bihrt_mod.scenes.cornell_materials()
    assert pal.dtype == bihrt_mod.MATERIAL_DTYPE and pal.shape == (5,) and pal[:4].tobytes() == base.tobytes()
    assert pal["kind"].tolist() == [0, 0, 0, 0, 1] and pal["albedo"][4].tolist() == [F32(.9)] * 3
    assert not pal["emission"][4].any()
    mirrors = [0, 1] + list(range(10, 20))
    assert np.flatnonzero(ids == 4).tolist() == mirrors and ids.dtype == np.uint32 and ids.shape == (32,)
    rest = np.setdiff1d(np.arange(32), mirrors)
    assert np.array_equal(ids[rest], base_ids[rest])


def _build_c(tmp_path) -> str:
    exe = str(tmp_path / "path_spec_smoke")
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


@pytest.mark.parametrize("name,kname", CLASSES)
def test_restatement_identity_and_conditions(name, kname, bihrt_mod):
    """The test's own reference against the existing one: with every kind zero
    it gives test_path_rgb.expect's planes at 1, 3 and 8 levels; and the
    conditions the fixture stands for hold."""
    for nb in (1, 3, 8):
        old = trgb.expect(name, kname, W, H, SPP, FRAME, nb)
        new = expect(name, kname, W, H, SPP, FRAME, nb, "zero")
        for k in NAMES + ("acc",):
            assert np.array_equal(cplane(new[k]), cplane(old[k])), (nb, k)
    check_class(name, kname)


# --- GPU ------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n_bounces", [1, 2, 3, 8])
@pytest.mark.parametrize("name,kname", CLASSES)
def test_classes(name, kname, n_bounces, gpu, bihrt_mod):
    """The fixture at 48x32x4 under fib_lights(2) + the scene's panels: the five planes on bits."""
    exp = expect(name, kname, W, H, SPP, FRAME, n_bounces)
    r = renderer(with_materials(name), name, kname, W, H, SPP)
    dl, lp, pan = lights_of(name)
    assert_planes(dev_spec(r, dl, lp, pan, n_bounces, FRAME), exp, f"{name} {kname} {n_bounces}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,kname", CLASSES)
def test_identity_and_the_old_call_ignores_kind(name, kname, gpu, bihrt_mod):
    """With every kind zeroed all five planes are bih_render_path_rgb_device's
    bytes at 1, 3 and 8 levels, GPU against GPU; and bih_render_path_rgb_device
    on the mirror palette equals itself on the zeroed one, while the mirror
    call does not."""
    r = renderer(with_materials(name, "zero"), name, kname, W, H, SPP)
    dl, lp, pan = lights_of(name)
    rgb = {}
    for nb in (1, 3, 8):
        rgb[nb] = dev_spec(r, dl, lp, pan, nb, FRAME, spec=False)
        assert rgb[nb]["radiance"].any() and rgb[nb]["lits"].any()
        same(dev_spec(r, dl, lp, pan, nb, FRAME), rgb[nb], f"all diffuse, {nb}")
    with_materials(name)
    same(dev_spec(r, dl, lp, pan, 3, FRAME, spec=False), rgb[3], "the colour call on the mirror palette")
    got = dev_spec(r, dl, lp, pan, 3, FRAME)
    for k in ("lit", "bounces", "lits", "radiance"):
        assert got[k].tobytes() != rgb[3][k].tobytes(), k


@pytest.mark.gpu
def test_all_mirror(gpu, bihrt_mod):
    """Every material a mirror: lit and lits are zero, the call equals itself
    with no lights, radiance is emission and sky only (the restatement with no
    lights), and some path runs along mirrors to the last level."""
    name, kname, nb = "soup3k", "K2", 3
    lv = levels_of(name, kname, W, H, SPP, FRAME, "mirror", False, nb)
    assert lv["alive"][0].any() and not any(a.any() for a in lv["lits"]) and not lv["lit"].any()
    exp = expect(name, kname, W, H, SPP, FRAME, nb, "mirror", False)
    r = renderer(with_materials(name, "mirror"), name, kname, W, H, SPP)
    dl, lp, pan = lights_of(name)
    got = dev_spec(r, dl, lp, pan, nb, FRAME)
    assert not got["lit"].any() and not got["lits"].any() and got["radiance"].any()
    same(got, dev_spec(r, None, None, None, nb, FRAME), "no lights")
    assert_planes(got, exp, "all mirror")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,spp", [(1, 1, 1), (40, 24, 1), (8, 8, 64), (37, 29, 3)])
def test_shapes(w, h, spp, gpu, bihrt_mod):
    """One sample; 1 spp; 64 spp on a small image (a pixel per wave); a width
    that is no multiple of the tile with an spp that is no power of two."""
    lv = levels_of("soup20k", "K2", w, h, spp, 1, levels=2)
    if (w, h) != (1, 1):
        assert (lv["hit"] & (lv["kind0"] == MIRROR)).any() and lv["alive"][1].any()
    exp = expect("soup20k", "K2", w, h, spp, 1, 2, levels=2)
    r = renderer(with_materials("soup20k"), "soup20k", "K2", w, h, spp)
    dl, lp, pan = lights_of("soup20k")
    assert_planes(dev_spec(r, dl, lp, pan, 2, 1), exp, f"{w}x{h}x{spp}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE)
def test_edge_scenes(name, gpu, bihrt_mod):
    """Every edge scene under K2 at n_bounces = 3; ids i % 5, material 2 a mirror."""
    exp = expect(name, "K2", W, H, SPP, FRAME, 3, levels=3)
    r = renderer(with_materials(name), name, "K2", W, H, SPP)
    dl, lp, pan = lights_of(name)
    assert_planes(dev_spec(r, dl, lp, pan, 3, FRAME), exp, name)


@pytest.mark.gpu
def test_two_stack_slots(gpu, bihrt_mod):
    """soup20k at n_bounces = 3 with two stack slots on chip: the walk's second instantiation."""
    exp = expect("soup20k", "K2", W, H, SPP, FRAME, 3)
    g = with_materials("soup20k")
    r = renderer(g, "soup20k", "K2", W, H, SPP)
    dl, lp, pan = lights_of("soup20k")
    g.set_param(bihrt_mod.PARAM_TRACE_LDS_SLOTS, 2)
    try:
        assert_planes(dev_spec(r, dl, lp, pan, 3, FRAME), exp, "2 slots")
    finally:
        g.set_param(bihrt_mod.PARAM_TRACE_LDS_SLOTS, 0)


@pytest.mark.gpu
def test_rows_bands_planes_host_entry_and_memory(gpu, bihrt_mod):
    """Interleaved bands and rows that are not tile-aligned equal the same rows
    of the full frame, through both entries; each plane alone gives the bits of
    all together and leaves the others untouched; the call's scratch (16 bytes
    per sample next to the colour call's) is counted in bih_tree_info, and no
    call after the first of the shape allocates."""
    nb = 3
    S = W * H * SPP
    exp = expect("soup20k", "K2", W, H, SPP, FRAME, nb)
    tris = scene("soup20k")[0]
    g = bihrt_mod.GPUArrayManager(tris)
    g.set_materials(palette(), ids_of(tris.shape[0]))
    r = renderer(g, "soup20k", "K2", W, H, SPP)
    dl, lp, pan = lights_of("soup20k")
    dev_spec(r, dl, lp, pan, nb, FRAME, spec=False)                    # the colour call's scratch first
    before = g.info()
    assert_planes(dev_spec(r, dl, lp, pan, nb, FRAME), exp, "device entry")
    mid = g.info()
    assert mid.device_allocs == before.device_allocs + 1 and mid.device_bytes == before.device_bytes + 16 * S
    host = r.render_path_spec(dl, lp, pan, SKY3, nb, FRAME)
    assert sorted(host) == sorted(NAMES) and host["bounces"].shape == (nb, S)
    assert host["radiance"].shape == (H, W, 3) and host["rgba"].shape == (H, W)
    assert_planes(host, exp, "host entry")
    for name in NAMES:                       # (first: a call without lit / lits grows the tree's own words)
        got = dev_spec(r, dl, lp, pan, nb, FRAME, names=(name,))
        assert_planes(got, exp, f"{name} alone", names=(name,))
        for other in NAMES:
            if other != name:
                assert (np.ascontiguousarray(got[other]).view(np.uint8) == 0xAB).all(), (name, other)
    first = g.info()
    for rows, ys in ((bihrt_mod.Rows(4, 8, 4, 2), [4, 5, 6, 7, 12, 13, 14, 15]),
                     (bihrt_mod.Rows(5, 7, 7, 1), list(range(5, 12)))):
        sub = rows_of(exp, W, SPP, ys)
        assert (sub["bounces"][nb - 1]["prim"] != bihrt_mod.NO_HIT).any() and (sub["lits"][1] != 0).any()
        assert_planes(dev_spec(r, dl, lp, pan, nb, FRAME, rows), sub, f"rows {ys[0]}..")
        assert_planes(r.render_path_spec(dl, lp, pan, SKY3, nb, FRAME, rows), sub, "host entry rows")
    assert_planes(r.render_path_spec(dl, lp, pan, SKY3, nb, FRAME, planes=("radiance",)), exp, "host, one plane",
                  names=("radiance",))
    assert_planes(dev_spec(r, dl, lp, pan, nb, FRAME), exp, "again")
    after = g.info()
    assert after.device_allocs == first.device_allocs and after.device_bytes == first.device_bytes
    g.close()


@pytest.mark.gpu
def test_bad_kind(gpu, bihrt_mod):
    """A palette with kind 2 is accepted by set_materials; the mirror call gives
    BIH_ERR_INVALID through both entries while bih_render_path_rgb still renders
    it; a good palette afterwards renders."""
    name = "soup3k"
    tris = scene(name)[0]
    g = bihrt_mod.GPUArrayManager(tris)
    r = renderer(g, name, "K2", W, H, SPP)
    dl, lp, pan = lights_of(name)
    g.set_materials(palette("bad"), ids_of(tris.shape[0]))
    with pytest.raises(bihrt_mod.BihError):
        dev_spec(r, dl, lp, pan, 2, FRAME)
    with pytest.raises(bihrt_mod.BihError):
        r.render_path_spec(dl, lp, pan, SKY3, 2, FRAME)
    assert_planes(dev_spec(r, dl, lp, pan, 2, FRAME, spec=False), trgb.expect(name, "K2", W, H, SPP, FRAME, 2),
                  "the colour call")
    g.set_materials(palette(), ids_of(tris.shape[0]))
    assert_planes(dev_spec(r, dl, lp, pan, 2, FRAME), expect(name, "K2", W, H, SPP, FRAME, 2), "a good palette")
    g.close()


@pytest.mark.gpu
def test_renders_undisturbed(gpu, bihrt_mod):
    """bih_render, bih_render_path and bih_render_path_rgb before and after
    mirror calls give the same bytes, and the mirror calls between them are right."""
    name, kname = "cornell", "K1"
    tris, ot = scene(name)
    cam = camera(name, kname, W, H)
    g = bihrt_mod.GPUArrayManager(tris)
    g.set_materials(palette(), ids_of(tris.shape[0]))
    r = renderer(g, name, kname, W, H, SPP)
    dl, lp, pan = lights_of(name)
    bn = (ti.ALBEDO, ti.SKY)
    p_before = r.render_path(dl, lp, pan, bn, 3, 2)
    c_before = r.render_path_rgb(dl, lp, pan, SKY3, 3, 2)
    f0 = r.render(0)
    s2 = r.render_path_spec(dl, lp, pan, SKY3, 3, 2)
    f2 = r.render(2)
    p_after = r.render_path(dl, lp, pan, bn, 3, 2)
    c_after = r.render_path_rgb(dl, lp, pan, SKY3, 3, 2)
    f3 = r.render(3)
    s3 = r.render_path_spec(dl, lp, pan, SKY3, 2, 3)
    assert r.frame == 4
    for f, img in ((0, f0), (2, f2), (3, f3)):
        assert np.array_equal(img, ot.render(W, H, spp=SPP, frame=f, seed=SEED, cam=cam)[0]), f
    for k in tp.NAMES:
        assert p_before[k].tobytes() == p_after[k].tobytes(), k
    same(c_before, c_after, "the colour call")
    assert_planes(c_after, trgb.expect(name, kname, W, H, SPP, 2, 3, levels=3), "colour, frame 2")
    assert_planes(s2, expect(name, kname, W, H, SPP, 2, 3, levels=3), "frame 2")
    assert_planes(s3, expect(name, kname, W, H, SPP, 3, 2, levels=3), "frame 3")
    g.close()


@pytest.mark.gpu
def test_rebuild_ordering_and_two_streams(gpu, bihrt_mod):
    """Mirror calls of one tree back to back on two streams with different
    frames and depths; one enqueued right before a rebuild renders the old
    soup's tree, one on a second stream after it the new soup's."""
    import torch
    old, new = scene("soup3k")[0], scene("soup3k2")[0]
    soup = torch.from_numpy(old.copy()).cuda()
    torch.cuda.synchronize()
    g = bihrt_mod.GPUArrayManager.from_device(soup.data_ptr(), old.shape[0])
    g.set_materials(palette(), ids_of(old.shape[0]))
    ea = expect("soup3k", "K2", W, H, SPP, 1, 3, levels=3)
    eb = expect("soup3k", "K2", W, H, SPP, 2, 2, levels=3)
    e1 = expect("soup3k2", "K2", W, H, SPP, 1, 3, levels=3)
    assert not np.array_equal(cplane(ea["radiance"]), cplane(e1["radiance"]))
    r0, r1 = renderer(g, "soup3k", "K2", W, H, SPP), renderer(g, "soup3k2", "K2", W, H, SPP)
    da, db, dc, dd, d1 = Dev(H, W, SPP, 3), Dev(H, W, SPP, 2), Dev(H, W, SPP, 3), Dev(H, W, SPP, 3), Dev(H, W, SPP, 3)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    da.launch(r0, *lights_of("soup3k"), SKY3, 1, stream=sa.cuda_stream)
    db.launch(r0, *lights_of("soup3k"), SKY3, 2, stream=sb.cuda_stream)
    dc.launch(r0, *lights_of("soup3k"), SKY3, 1, stream=sa.cuda_stream)
    sa.synchronize()
    sb.synchronize()
    g.sync()
    # enqueued before a rebuild of the unchanged soup: the rebuild orders after it
    dd.launch(r0, *lights_of("soup3k"), SKY3, 1, stream=sa.cuda_stream)
    g.rebuild()
    sa.synchronize()
    g.sync()                      # (the caller's duty: the soup is not rewritten under a build or render)
    soup.copy_(torch.from_numpy(new))
    torch.cuda.synchronize()
    g.rebuild()
    d1.launch(r1, *lights_of("soup3k2"), SKY3, 1, stream=sb.cuda_stream)
    sb.synchronize()
    assert_planes(da.result(), ea, "stream a")
    assert_planes(db.result(), eb, "stream b")
    assert_planes(dc.result(), ea, "stream a again")
    assert_planes(dd.result(), ea, "before the rebuild")
    assert_planes(d1.result(), e1, "after the rebuild")
    g.close()


@pytest.mark.gpu
def test_c_caller(tmp_path, gpu, bihrt_mod):
    """tests/c/path_spec_smoke.c -- bih_build + bih_tree_set_materials +
    bih_render_path_spec from strict C11 (cornell with its mirror materials,
    64x48x4, the reference camera, a sky dome, 3 bounces): its checksum is the
    one of the device entry's planes."""
    exe = _build_c(tmp_path)
    tris = scene("cornell")[0]
    w, h, spp, nb = 64, 48, 4, 3
    dl = bihrt_mod.scenes.sky_dome(2)
    pal, ids = bihrt_mod.scenes.cornell_mirror_materials()
    sp, lp, mp, ip = (tmp_path / n for n in ("scene.f32", "dir.f32", "mat.bin", "ids.u32"))
    tris.tofile(sp)
    dl.tofile(lp)
    mp.write_bytes(pal.tobytes())
    ids.tofile(ip)
    r = subprocess.run([exe, str(sp), str(tris.shape[0]), str(w), str(h), str(spp), "0", str(lp), str(dl.shape[0]),
                        str(mp), str(pal.shape[0]), str(ip), "0.25", "0.3", "0.4", str(nb)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "path_spec_smoke OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
    g = bihrt_mod.GPUArrayManager(tris)
    g.set_materials(pal, ids)
    ref = dev_spec(bihrt_mod.Renderer(g, w, h, spp=spp), dl, None, None, nb, 0)
    g.close()
    assert ref["lits"][nb - 1].any() and ref["radiance"].any()
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("checksum ")]
    assert len(line) == 1 and int(line[0].split()[1], 16) == trgb.checksum(ref), (line, hex(trgb.checksum(ref)))


@pytest.mark.gpu
def test_app_writes_ppm(tmp_path, gpu, bihrt_mod):
    """python -m bihrt --scene cornell --direct --bounce A,S --bounces 3 --colour
    --mirror: the PPM of render_path_spec's rgba plane with
    cornell_mirror_materials(); it is not the --colour image."""
    from bihrt.app import main
    out, plain, want = tmp_path / "m.ppm", tmp_path / "c.ppm", tmp_path / "want.ppm"
    common = ["--scene", "cornell", "--width", "64", "--height", "48", "--frames", "1", "--bounce", "0.5,0.25",
              "--bounces", "3", "--colour"]
    assert main(common + ["--direct", str(out), "--mirror"]) == 0
    assert main(common + ["--direct", str(plain)]) == 0
    g = bihrt_mod.GPUArrayManager(bihrt_mod.scenes.cornell())
    g.set_materials(*bihrt_mod.scenes.cornell_mirror_materials())
    ref = bihrt_mod.Renderer(g, 64, 48).render_path_spec(None, None, None, (.25, .25, .25), 3, 0,
                                                         planes=("rgba",))["rgba"]
    g.close()
    bihrt_mod.write_ppm(str(want), ref)
    assert open(out, "rb").read() == open(want, "rb").read()
    assert open(out, "rb").read() != open(plain, "rb").read()
