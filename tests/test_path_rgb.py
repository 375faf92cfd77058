"""Colour paths (bih_tree_set_materials, bih_render_path_rgb /
bih_render_path_rgb_device): bih_render_path with a
material per triangle -- albedo and emission, R G B -- and an RGB sky.

Expected values: the levels come from test_path.levels_of (the oracle alone),
the material of level 0's hit from test_gbuffer.expected's prim, the one of
level k's from the restated bounce record's prim; then the header's forward
accumulation per channel in numpy f32.  Planes are compared on bits, NaN as
NaN (test_indirect.cplane).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_gbuffer as tg
import test_indirect as ti
import test_path as tp
from conftest import ROOT
from test_direct import MISS_SHADE
from test_gbuffer import EDGE, F32, LIBDIR, SEED, camera, expected, renderer, scene, tree
from test_indirect import cplane, lights_of
from test_path import CLASSES, FRAME, H, LEVELS, MAXB, SPP, W, levels_of

SRC = os.path.join(ROOT, "tests", "c", "path_rgb_smoke.c")
NAMES = ("lit", "bounces", "lits", "radiance", "rgba")
SIZE = {"lit": 8, "bounces": 16, "lits": 8}         # bytes per sample (and level); radiance 12, rgba 4 per pixel
# the fixture: five materials, the last one emissive; triangle i (file order) has material i % 5
ALBEDO5 = [(.73, .71, .68), (.63, .065, .05), (.14, .45, .091), (.3, .5, .9), (.78, .78, .78)]
EMISSION5 = [(0, 0, 0)] * 4 + [(1.7, 1.3, .6)]
EMISSIVE = 4
SKY3 = (.25, .3, .4)
WHITE = [(1, 1, 1, 0, 0, 0)]

# soup3k in reverse file order: the same triangles, every file position another one's
tg.EXTRA_SCENES.setdefault("soup3k_rev", lambda: np.ascontiguousarray(scene("soup3k")[0][::-1]))


def palette():
    import bihrt
    return bihrt.pack_materials([a + e for a, e in zip(ALBEDO5, EMISSION5)])


def ids_of(n):
    return (np.arange(n) % 5).astype(np.uint32)


def rotated(pal):
    """R -> G -> B -> R in every material."""
    out = pal.copy()
    out["albedo"], out["emission"] = np.roll(pal["albedo"], 1, 1), np.roll(pal["emission"], 1, 1)
    return out


# --- the header, restated ---------------------------------------------------------

def planes_rgb(lv, prim0, spp, n_bounces, pal, ids, sky):
    """The five planes of a call of n_bounces levels over the restated levels lv
    (test_path.levels_of), prim0 the primary hits' prim (file order): the
    forward accumulation per channel in f32; "acc": the samples' sums (n, 3)."""
    import bihrt
    pal = bihrt.pack_materials(pal)
    alb, em = np.ascontiguousarray(pal["albedo"], F32), np.ascontiguousarray(pal["emission"], F32)
    ids = np.zeros(1 << 20, np.uint32) if ids is None else np.asarray(ids, np.uint32)
    sky = np.asarray(sky, F32).reshape(1, 3)
    hit = lv["hit"]
    with np.errstate(all="ignore"):
        m = ids[np.where(hit, prim0, 0)]
        acc = np.where(hit[:, None], em[m], F32(0.0))
        thr = alb[m]
        acc = np.where(hit[:, None], acc + thr * lv["e0"][:, None], acc)
        before = hit
        for k in range(1, n_bounces + 1):
            alive = lv["alive"][k - 1]
            m = ids[np.where(alive, lv["bounces"][k - 1]["prim"], 0)]
            acc = np.where((before & ~alive)[:, None], acc + thr * sky, acc)     # an escape: thr_{k-1} * sky
            acc = np.where(alive[:, None], acc + thr * em[m], acc)
            thr = np.where(alive[:, None], thr * alb[m], thr)
            acc = np.where(alive[:, None], acc + thr * lv["e"][k - 1][:, None], acc)
            before = alive
        assert acc.dtype == F32 and thr.dtype == F32
        e_s = acc.reshape(-1, spp, 3)
        tot = e_s[:, 0]
        for k in range(1, spp):
            tot = tot + e_s[:, k]
        E = tot / F32(spp)
        assert E.dtype == F32
        g8 = np.fmax(F32(0), np.fmin(F32(255), F32(255) * E)).astype(np.int32).astype(np.uint32)
    shade = g8[:, 0] | (g8[:, 1] << 8) | (g8[:, 2] << 16)
    rgba = np.where(hit.reshape(-1, spp).any(1), shade, np.uint32(MISS_SHADE)).astype(np.uint32)
    return {"lit": lv["lit"], "bounces": np.stack(lv["bounces"][:n_bounces]), "lits": np.stack(lv["lits"][:n_bounces]),
            "radiance": E, "rgba": rgba, "acc": acc}


def expect(name, kname, w, h, spp, frame, n_bounces, pal=None, ids="mod5", sky=SKY3, levels=MAXB):
    lv = levels_of(name, kname, w, h, spp, frame, True, levels)
    prim0 = expected(name, kname, w, h, spp, frame)["hits"]["prim"]
    n_tris = scene(name)[0].shape[0]
    return planes_rgb(lv, prim0, spp, n_bounces, palette() if pal is None else pal,
                      ids_of(n_tris) if isinstance(ids, str) else ids, sky)


def check_class(name, kname):
    """The conditions the fixture stands for, on the restatement."""
    import bihrt
    lv = levels_of(name, kname, W, H, SPP, FRAME)
    tp.check_class(name, lv)
    prim0 = expected(name, kname, W, H, SPP, FRAME)["hits"]["prim"]
    exp = expect(name, kname, W, H, SPP, FRAME, MAXB)
    acc = exp["acc"]
    differ = (acc[:, 0] != acc[:, 1]) & (acc[:, 1] != acc[:, 2]) & (acc[:, 0] != acc[:, 2])
    px = exp["rgba"]
    r, g, b = px & 0xFF, (px >> 8) & 0xFF, (px >> 16) & 0xFF
    coloured = ~((r == g) & (g == b)) & lv["hit"].reshape(-1, SPP).any(1)          # (the miss shade is no colour)
    ids = ids_of(scene(name)[0].shape[0])
    on1 = lv["alive"][0]
    lamp1 = int((ids[lv["bounces"][0]["prim"][on1]] == EMISSIVE).sum())
    lamp0 = int((ids[prim0[lv["hit"]]] == EMISSIVE).sum())
    print(name, "samples whose channels differ pairwise", int(differ.sum()), "coloured pixels", int(coloured.sum()),
          "emissive hits at level 1", lamp1, "at level 0", lamp0)
    assert differ.sum() >= 1000 and coloured.sum() >= 400 and lamp1 >= 20 and lamp0 >= 20
    assert np.isfinite(acc).all() and bihrt.NO_HIT not in prim0[lv["hit"]]


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
    out["radiance"] = exp["radiance"].reshape(-1, w, 3)[ys]
    out["rgba"] = exp["rgba"].reshape(-1, w)[ys]
    return out


class Dev:
    """Device planes (torch tensors prefilled with 0xAB) of a colour path call."""

    def __init__(self, nrows, w, spp, n_bounces, names=NAMES):
        import torch
        self.nrows, self.w, self.spp, self.nb, self.names = nrows, w, spp, n_bounces, names
        P = nrows * w
        size = {k: SIZE[k] * spp * (n_bounces if k in LEVELS else 1) for k in SIZE}
        size.update(radiance=12, rgba=4)
        self.t = {k: torch.full((P * size[k],), 0xAB, dtype=torch.uint8, device="cuda") for k in NAMES}
        torch.cuda.synchronize()

    def launch(self, r, dl, lp, pan, sky, frame, rows=None, stream=None):
        r.render_path_rgb_device({k: self.t[k].data_ptr() for k in self.names}, dl, lp, pan, sky, self.nb, frame, rows,
                                 stream)

    def result(self):
        """Every plane (also the ones not asked for), shaped as render_path_rgb's."""
        import bihrt
        out = {}
        for k, ten in self.t.items():
            dt, per = bihrt.PATH_RGB_PLANES[k]
            a = ten.cpu().numpy().view(dt)
            out[k] = (a.reshape((self.nrows, self.w) + ((per,) if per > 1 else ())) if per > 0 else
                      (a.reshape(self.nb, -1) if per < 0 else a))
        return out


def dev_rgb(r, dl, lp, pan, n_bounces, frame, rows=None, names=NAMES, sky=SKY3):
    nrows = rows.nrows if rows is not None else r.h
    dv = Dev(nrows, r.w, r.spp, n_bounces, names)
    dv.launch(r, dl, lp, pan, sky, frame, rows)
    r.sync()
    return dv.result()


def with_materials(name, pal=None, ids="mod5"):
    """The scene's shared tree with the fixture's materials (or the ones given)."""
    g = tree(name)
    g.set_materials(palette() if pal is None else pal,
                    ids_of(scene(name)[0].shape[0]) if isinstance(ids, str) else ids)
    return g


@pytest.fixture(scope="module", autouse=True)
def _free_trees():
    yield
    while tg._trees:
        tg._trees.popitem()[1].close()


# --- CPU ------------------------------------------------------------------------

def test_struct_layout(bihrt_mod):
    M, Pt = bihrt_mod.Material, bihrt_mod.PathRgb
    p = C.sizeof(C.c_void_p)
    assert C.sizeof(M) == 32 and M.albedo.offset == 0 and M.emission.offset == 16
    assert bihrt_mod.MATERIAL_DTYPE.itemsize == 32 and bihrt_mod.MATERIAL_DTYPE.fields["emission"][1] == 16
    assert [f[0] for f in Pt._fields_] == list(NAMES) and C.sizeof(Pt) == 5 * p
    assert [getattr(Pt, f).offset for f in NAMES] == [k * p for k in range(5)]
    assert bihrt_mod.PATH_RGB == NAMES and list(bihrt_mod.PATH_RGB_PLANES) == list(NAMES)
    assert bihrt_mod.PATH_RGB_PLANES["radiance"] == (np.float32, 3) and bihrt_mod.MAX_MATERIALS == 65536
    for name in ("MATERIAL_DTYPE", "Material", "PathRgb", "PATH_RGB", "PATH_RGB_PLANES", "MAX_MATERIALS",
                 "pack_materials"):
        assert name in bihrt_mod.__all__, name
    for name in ("render_path_rgb", "render_path_rgb_device"):
        assert hasattr(bihrt_mod.Renderer, name), name
    assert hasattr(bihrt_mod.GPUArrayManager, "set_materials")
    pal = bihrt_mod.pack_materials([(1, 2, 3, 4, 5, 6)])
    assert pal.dtype == bihrt_mod.MATERIAL_DTYPE and pal.view(F32).tolist() == [1, 2, 3, 0, 4, 5, 6, 0]
    assert bihrt_mod.pack_materials(pal).tobytes() == pal.tobytes()


def test_header_symbols_exported(bihrt_mod):
    names = bihrt_mod._lib.exported_symbols_from_header()
    L = bihrt_mod._lib.load()
    for sym in ("bih_tree_set_materials", "bih_render_path_rgb", "bih_render_path_rgb_device"):
        assert sym in names and getattr(L, sym) is not None, sym
    hdr = open(os.path.join(ROOT, "include", "bih.h")).read()
    assert "#define BIH_ABI_VERSION 4" in hdr and "#define BIH_MAX_MATERIALS 65536" in hdr
    assert "typedef struct bih_material" in hdr and "typedef struct bih_path_rgb" in hdr
    assert L.bih_abi_version() == 4


def _header_compiles(tmp_path, cc, std, ext):
    src = tmp_path / ("hdr." + ext)
    src.write_text('#include "bih.h"\n'
                   "int main(void) { bih_path_rgb p = {0, 0, 0, 0, 0};\n"
                   "  bih_material m = {{1, 1, 1}, 0, {0, 0, 0}, 0}; (void)p; (void)BIH_MAX_MATERIALS;\n"
                   "  return bih_tree_set_materials(0, &m, 1, 0) == BIH_ERR_INVALID && sizeof m == 32 ? 0 : 1; }\n")
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
    I, R, S = bihrt_mod.PathRgb, bihrt_mod.Rows, bihrt_mod.LightSet
    sun = (bihrt_mod.Light * 1)()
    sun[0].dir[1], sun[0].weight = 1.0, 1.0
    lamp = (bihrt_mod.PointLight * 1)()
    pan = (bihrt_mod.AreaLight * 1)()
    ps, pl, pp = (C.cast(x, C.c_void_p) for x in (sun, lamp, pan))
    full, empty = S(ps, 1, pl, 1, pp, 1), S(None, 0, None, 0, None, 0)
    sky = (C.c_float * 3)(*SKY3)
    rgba, none = I(rgba=base), I()
    for entry in (lambda *a: L.bih_render_path_rgb_device(*a, None), L.bih_render_path_rgb):
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
        # 2: the lights: NULL and empty are legal, the rest as bih_render_area_lights
        assert call(fake, cam, 8, 8, 4, None, S(ps, 33, pl, 31, pp, 1), sky, rgba) == INVALID   # 65 together
        assert call(fake, cam, 8, 8, 4, None, S(ps, 1, pl, 1, pp, 17), sky, rgba) == INVALID    # n_area > 16
        assert call(fake, cam, 8, 8, 4, None, S(None, 1, pl, 1, pp, 1), sky, rgba) == INVALID   # NULL with a count
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), S(ps, 1, pl, 1, None, 1), sky, rgba) == INVALID
        # 3: lit's alignment; sky == NULL; n_bounces; the level planes' alignments
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, sky, I(lit=base + 4, rgba=base)) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, None, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), None, None, rgba) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, sky, rgba, 0) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, sky, rgba, MAXB + 1) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, sky, rgba, 0xFFFFFFFF) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, sky, I(lits=base + 4, rgba=base)) == INVALID
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, sky, I(bounces=base + 8)) == INVALID
        # 4: nothing to do -- each single plane (radiance at 4 bytes), every legal n_bounces, no lights at all;
        #    the tree (which has no materials: it is no tree) is never dereferenced
        for d in (I(lit=base), I(bounces=base), I(lits=base + 8), I(radiance=base + 4), rgba):
            assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, sky, d) == 0
        for nb in range(1, MAXB + 1):
            assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), full, sky, rgba, nb) == 0
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), None, sky, rgba) == 0
        assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), empty, sky, rgba) == 0
        assert call(fake, cam, 8, 8, 64, R(3, 0, 0, 0), S(ps, 46, pl, 2, pp, 16), sky, rgba, MAXB) == 0


def test_set_materials_null_tree(bihrt_mod):
    L = bihrt_mod._lib.load()
    pal = palette()
    ids = ids_of(4)
    assert L.bih_tree_set_materials(None, pal.ctypes.data, 5, ids.ctypes.data) == -1
    assert L.bih_tree_set_materials(None, None, 0, None) == -1


def test_app_colour_options(bihrt_mod):
    """--colour without --bounces, or with a scene that has no built-in
    materials, is an error, before any device is used."""
    from bihrt.app import main
    for argv in (["--scene", "cornell", "--frames", "1", "--colour"],
                 ["--scene", "cornell", "--frames", "1", "--direct", "d.ppm", "--colour"],
                 ["--scene", "cornell", "--frames", "1", "--direct", "d.ppm", "--bounce", "0.5", "--colour"],
                 ["--scene", "torus", "--frames", "1", "--direct", "d.ppm", "--bounce", "0.5", "--bounces", "2",
                  "--colour"],
                 ["--scene", "soup:1000", "--frames", "1", "--direct", "d.ppm", "--bounce", "0.5", "--bounces", "2",
                  "--colour"],
                 ["--obj", "no_such.obj", "--frames", "1", "--direct", "d.ppm", "--bounce", "0.5", "--bounces", "2",
                  "--colour"]):
        with pytest.raises(SystemExit):
            main(argv)


def _build_c(tmp_path) -> str:
    exe = str(tmp_path / "path_rgb_smoke")
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
    """The test's own reference against the existing one: one white material and
    a grey sky give test_path.planes_of(albedo 1, sky 0.25) in every channel at
    1, 3 and 8 levels; and the conditions the fixture stands for hold."""
    lv = levels_of(name, kname, W, H, SPP, FRAME)
    for nb in (1, 3, 8):
        grey = tp.planes_of(lv, SPP, nb, albedo=1.0, sky=0.25)
        for ids in (None, "mod5"):
            pal = WHITE if ids is None else WHITE * 5
            rgb = expect(name, kname, W, H, SPP, FRAME, nb, pal, ids, (.25, .25, .25))
            for c in range(3):
                assert np.array_equal(cplane(rgb["radiance"][:, c]), cplane(grey["irradiance"])), (nb, c)
            assert np.array_equal(rgb["rgba"], grey["rgba"]) and rgb["bounces"].tobytes() == grey["bounces"].tobytes()
    check_class(name, kname)


def test_cornell_materials(bihrt_mod):
    pal, ids = bihrt_mod.scenes.cornell_materials()
    tris = bihrt_mod.scenes.cornell()
    assert pal.dtype == bihrt_mod.MATERIAL_DTYPE and ids.shape == (32,) == (tris.shape[0],) and ids.dtype == np.uint32
    assert ids.max() < pal.shape[0]
    emissive = pal["emission"][ids].any(1)
    assert np.flatnonzero(emissive).tolist() == [30, 31]
    red, green, white = pal["albedo"][ids[6]], pal["albedo"][ids[8]], pal["albedo"][ids[0]]
    assert (tris[6:8, 0::3] == -1.0).all() and (tris[8:10, 0::3] == F32(1.9)).all()      # the left and right walls
    assert red[0] > 4 * red[1] and red[0] > 4 * red[2] and green[1] > 2 * green[0] and green[1] > 2 * green[2]
    assert white[0] == white[1] == white[2]
    for k in list(range(0, 6)) + list(range(10, 30)):                    # back wall, floor, ceiling, blocks
        assert np.array_equal(pal["albedo"][ids[k]], white), k
    assert ids[6] == ids[7] and ids[8] == ids[9] and ids[30] == ids[31]


# --- GPU ------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n_bounces", [1, 2, 3, 8])
@pytest.mark.parametrize("name,kname", CLASSES)
def test_classes(name, kname, n_bounces, gpu, bihrt_mod):
    """The fixture at 48x32x4 under fib_lights(2) + the scene's panels: the five planes on bits."""
    exp = expect(name, kname, W, H, SPP, FRAME, n_bounces)
    r = renderer(with_materials(name), name, kname, W, H, SPP)
    dl, lp, pan = lights_of(name)
    assert_planes(dev_rgb(r, dl, lp, pan, n_bounces, FRAME), exp, f"{name} {kname} {n_bounces}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,kname", CLASSES)
def test_identity_with_path(name, kname, gpu, bihrt_mod):
    """One white material and sky (.25, .25, .25): every channel of radiance, and
    rgba, are bih_render_path_device's bytes with bounce (1.0, .25) on the same
    tree at 1, 3 and 8 levels; under the fixture's palette lit, bounces and
    lits are its bytes at 3."""
    g = tree(name)
    r = renderer(g, name, kname, W, H, SPP)
    dl, lp, pan = lights_of(name)
    g.set_materials(WHITE)
    for nb in (1, 3, 8):
        grey = tp.dev_path(r, dl, lp, pan, nb, FRAME, bounce=(1.0, 0.25))
        got = dev_rgb(r, dl, lp, pan, nb, FRAME, sky=(.25, .25, .25))
        assert (grey["irradiance"] > 0).any()
        for c in range(3):
            assert np.ascontiguousarray(got["radiance"][..., c]).tobytes() == grey["irradiance"].tobytes(), (nb, c)
        for k in ("rgba", "lit", "bounces", "lits"):
            assert got[k].tobytes() == grey[k].tobytes(), (nb, k)
    with_materials(name)
    grey = tp.dev_path(r, dl, lp, pan, 3, FRAME)
    got = dev_rgb(r, dl, lp, pan, 3, FRAME)
    for k in ("lit", "bounces", "lits"):
        assert got[k].tobytes() == grey[k].tobytes(), k
    assert got["rgba"].tobytes() != grey["rgba"].tobytes()


@pytest.mark.gpu
def test_channels_are_independent(gpu, bihrt_mod):
    """R -> G -> B -> R in every material and in sky: radiance rotates the same way, byte for byte."""
    name = "soup20k"
    g = with_materials(name)
    r = renderer(g, name, "K2", W, H, SPP)
    dl, lp, pan = lights_of(name)
    a = dev_rgb(r, dl, lp, pan, 3, FRAME)
    g.set_materials(rotated(palette()), ids_of(scene(name)[0].shape[0]))
    b = dev_rgb(r, dl, lp, pan, 3, FRAME, sky=tuple(np.roll(SKY3, 1)))
    ra = a["radiance"]
    assert (ra[..., 0] != ra[..., 1]).any() and (ra[..., 1] != ra[..., 2]).any()
    assert np.ascontiguousarray(np.roll(ra, 1, -1)).tobytes() == b["radiance"].tobytes()
    for k in ("lit", "bounces", "lits"):
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,spp", [(1, 1, 1), (37, 29, 3), (8, 8, 64), (16, 8, 16)])
def test_shapes(w, h, spp, gpu, bihrt_mod):
    """One sample; partial tiles and waves with an spp that is no power of two; a pixel per wave; four pixels per wave."""
    exp = expect("soup20k", "K2", w, h, spp, 1, 2, levels=2)
    r = renderer(with_materials("soup20k"), "soup20k", "K2", w, h, spp)
    dl, lp, pan = lights_of("soup20k")
    assert_planes(dev_rgb(r, dl, lp, pan, 2, 1), exp, f"{w}x{h}x{spp}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE)
def test_edge_scenes(name, gpu, bihrt_mod):
    """Every edge scene under K2 at n_bounces = 3; ids i % 5 (one_tri: material 0 only)."""
    n_tris = scene(name)[0].shape[0]
    ids = ids_of(n_tris)
    assert ids.max() == min(n_tris, 5) - 1
    exp = expect(name, "K2", W, H, SPP, FRAME, 3, levels=3)
    r = renderer(with_materials(name), name, "K2", W, H, SPP)
    dl, lp, pan = lights_of(name)
    assert_planes(dev_rgb(r, dl, lp, pan, 3, FRAME), exp, name)


@pytest.mark.gpu
def test_material_lifetime(gpu, bihrt_mod):
    """No materials: BIH_ERR_INVALID; a replacing set is followed (albedo 0
    everywhere: radiance is level 0's emission alone); a rebuild of the
    unchanged soup keeps the bytes; cleared: BIH_ERR_INVALID again.  The
    checks of set_materials leave the earlier set in place."""
    name, nb = "soup3k", 2
    tris = scene(name)[0]
    g = bihrt_mod.GPUArrayManager(tris)
    r = renderer(g, name, "K2", W, H, SPP)
    dl, lp, pan = lights_of(name)
    ids = ids_of(tris.shape[0])
    with pytest.raises(bihrt_mod.BihError):
        dev_rgb(r, dl, lp, pan, nb, FRAME)
    before = g.info()
    g.set_materials(palette(), ids)
    mid = g.info()
    assert mid.device_allocs == before.device_allocs + 2
    assert mid.device_bytes == before.device_bytes + 5 * 32 + 4 * tris.shape[0]
    assert_planes(dev_rgb(r, dl, lp, pan, nb, FRAME), expect(name, "K2", W, H, SPP, FRAME, nb), "first set")
    # a bad id, a count without a palette, ids without a palette: INVALID, and the set stays
    L = bihrt_mod._lib.load()
    bad = ids.copy()
    bad[-1] = 5
    pal = palette()
    assert L.bih_tree_set_materials(g.handle, pal.ctypes.data, 5, bad.ctypes.data) == -1
    assert L.bih_tree_set_materials(g.handle, pal.ctypes.data, 65537, ids.ctypes.data) == -1
    assert L.bih_tree_set_materials(g.handle, None, 5, ids.ctypes.data) == -1
    assert L.bih_tree_set_materials(g.handle, pal.ctypes.data, 0, None) == -1
    assert L.bih_tree_set_materials(g.handle, None, 0, ids.ctypes.data) == -1
    assert_planes(dev_rgb(r, dl, lp, pan, nb, FRAME), expect(name, "K2", W, H, SPP, FRAME, nb), "after the errors")
    # the replacing set: black surfaces, every material emits its own colour
    black = bihrt_mod.pack_materials([(0, 0, 0) + a for a in ALBEDO5])
    g.set_materials(black, ids)
    got = dev_rgb(r, dl, lp, pan, nb, FRAME)
    assert_planes(got, expect(name, "K2", W, H, SPP, FRAME, nb, black), "replaced")
    prim0 = expected(name, "K2", W, H, SPP, FRAME)["hits"]["prim"]
    hit = prim0 != bihrt_mod.NO_HIT
    em = np.where(hit[:, None], black["emission"][ids[np.where(hit, prim0, 0)]], F32(0)).reshape(-1, SPP, 3)
    tot = em[:, 0]
    for k in range(1, SPP):
        tot = tot + em[:, k]
    assert np.array_equal(got["radiance"].reshape(-1, 3), tot / F32(SPP)) and got["radiance"].any()
    # NULL ids: material 0 everywhere
    g.set_materials(palette()[3:4])
    assert_planes(dev_rgb(r, dl, lp, pan, nb, FRAME), expect(name, "K2", W, H, SPP, FRAME, nb, palette()[3:4], None),
                  "material 0 everywhere")
    g.set_materials(palette(), ids)
    a = dev_rgb(r, dl, lp, pan, nb, FRAME)
    g.rebuild()
    b = dev_rgb(r, dl, lp, pan, nb, FRAME)
    for k in NAMES:
        assert a[k].tobytes() == b[k].tobytes(), k
    with_them = g.info()
    g.set_materials(None)
    assert g.info().device_bytes == with_them.device_bytes - (5 * 32 + 4 * tris.shape[0])
    with pytest.raises(bihrt_mod.BihError):
        dev_rgb(r, dl, lp, pan, nb, FRAME)
    g.close()


@pytest.mark.gpu
def test_rebuild_with_a_changed_soup(gpu, bihrt_mod):
    """A bih_build_device tree with materials; the device soup is overwritten
    with the same triangles in reverse file order and the tree rebuilt, with no
    new set_materials: ids are by file position, so the planes are the
    restatement of the reversed soup with the same id array."""
    import torch
    old, new = scene("soup3k")[0], scene("soup3k_rev")[0]
    assert np.array_equal(old[::-1], new)
    ids = ids_of(old.shape[0])
    assert (ids != ids[::-1]).mean() > 0.7          # (3000 % 5 == 0: i and n-1-i differ by 4 mod 5)
    soup = torch.from_numpy(old.copy()).cuda()
    torch.cuda.synchronize()
    g = bihrt_mod.GPUArrayManager.from_device(soup.data_ptr(), old.shape[0])
    g.set_materials(palette(), ids)
    dl, lp, pan = lights_of("soup3k")
    r0 = renderer(g, "soup3k", "K2", W, H, SPP)
    e0 = expect("soup3k", "K2", W, H, SPP, FRAME, 2)
    assert_planes(dev_rgb(r0, dl, lp, pan, 2, FRAME), e0, "before")
    g.sync()
    soup.copy_(torch.from_numpy(new))
    torch.cuda.synchronize()
    g.rebuild()
    r1 = renderer(g, "soup3k_rev", "K2", W, H, SPP)
    e1 = expect("soup3k_rev", "K2", W, H, SPP, FRAME, 2)
    assert not np.array_equal(cplane(e0["radiance"]), cplane(e1["radiance"]))
    assert_planes(dev_rgb(r1, *lights_of("soup3k_rev"), 2, FRAME), e1, "after the rebuild")
    g.close()


@pytest.mark.gpu
def test_two_stack_slots(gpu, bihrt_mod):
    """soup20k at n_bounces = 3 with two stack slots on chip (the spill stack is used)."""
    exp = expect("soup20k", "K2", W, H, SPP, FRAME, 3)
    g = with_materials("soup20k")
    r = renderer(g, "soup20k", "K2", W, H, SPP)
    dl, lp, pan = lights_of("soup20k")
    g.set_param(bihrt_mod.PARAM_TRACE_LDS_SLOTS, 2)
    try:
        assert_planes(dev_rgb(r, dl, lp, pan, 3, FRAME), exp, "2 slots")
    finally:
        g.set_param(bihrt_mod.PARAM_TRACE_LDS_SLOTS, 0)


@pytest.mark.gpu
def test_rows_bands_planes_and_host_entry(gpu, bihrt_mod):
    """Interleaved bands and rows that are not tile-aligned equal the same rows
    of the full frame, through both entries; each plane alone gives the bits of
    all together and leaves the others untouched (prefilled with 0xAB); no call
    after the first of the shape allocates."""
    nb = 3
    exp = expect("soup20k", "K2", W, H, SPP, FRAME, nb)
    g = with_materials("soup20k")
    r = renderer(g, "soup20k", "K2", W, H, SPP)
    dl, lp, pan = lights_of("soup20k")
    host = r.render_path_rgb(dl, lp, pan, SKY3, nb, FRAME)
    assert sorted(host) == sorted(NAMES) and host["bounces"].shape == (nb, W * H * SPP)
    assert host["radiance"].shape == (H, W, 3) and host["rgba"].shape == (H, W)
    assert_planes(host, exp, "host entry")
    for name in NAMES:                       # (first: a call without lit / lits grows the tree's own words)
        got = dev_rgb(r, dl, lp, pan, nb, FRAME, names=(name,))
        assert_planes(got, exp, f"{name} alone", names=(name,))
        for other in NAMES:
            if other != name:
                assert (np.ascontiguousarray(got[other]).view(np.uint8) == 0xAB).all(), (name, other)
    first = g.info()
    for rows, ys in ((bihrt_mod.Rows(4, 8, 4, 2), [4, 5, 6, 7, 12, 13, 14, 15]),
                     (bihrt_mod.Rows(5, 7, 7, 1), list(range(5, 12)))):
        sub = rows_of(exp, W, SPP, ys)
        assert (sub["bounces"][nb - 1]["prim"] != bihrt_mod.NO_HIT).any() and (sub["lits"][1] != 0).any()
        assert_planes(dev_rgb(r, dl, lp, pan, nb, FRAME, rows), sub, f"rows {ys[0]}..")
        assert_planes(r.render_path_rgb(dl, lp, pan, SKY3, nb, FRAME, rows), sub, "host entry rows")
    for name in NAMES:
        assert_planes(dev_rgb(r, dl, lp, pan, nb, FRAME, names=(name,)), exp, f"{name} alone", names=(name,))
    assert_planes(r.render_path_rgb(dl, lp, pan, SKY3, nb, FRAME, planes=("radiance",)), exp, "host, one plane",
                  names=("radiance",))
    after = g.info()
    assert after.device_allocs == first.device_allocs and after.device_bytes == first.device_bytes


@pytest.mark.gpu
def test_renders_undisturbed(gpu, bihrt_mod):
    """bih_render, bih_render_path and bih_render_indirect before and after a
    colour call give the same bytes, and the colour calls between them are right."""
    name, kname = "cornell", "K1"
    tris, ot = scene(name)
    cam = camera(name, kname, W, H)
    g = bihrt_mod.GPUArrayManager(tris)
    g.set_materials(palette(), ids_of(tris.shape[0]))
    r = renderer(g, name, kname, W, H, SPP)
    dl, lp, pan = lights_of(name)
    bn = (ti.ALBEDO, ti.SKY)
    i_before = r.render_indirect(dl, lp, pan, bn, 2)
    p_before = r.render_path(dl, lp, pan, bn, 3, 2)
    f0 = r.render(0)
    c2 = r.render_path_rgb(dl, lp, pan, SKY3, 3, 2)
    f2 = r.render(2)
    i_after = r.render_indirect(dl, lp, pan, bn, 2)
    p_after = r.render_path(dl, lp, pan, bn, 3, 2)
    f3 = r.render(3)
    c3 = r.render_path_rgb(dl, lp, pan, SKY3, 2, 3)
    assert r.frame == 4
    for f, img in ((0, f0), (2, f2), (3, f3)):
        assert np.array_equal(img, ot.render(W, H, spp=SPP, frame=f, seed=SEED, cam=cam)[0]), f
    for k in ti.NAMES:
        assert i_before[k].tobytes() == i_after[k].tobytes(), k
    for k in tp.NAMES:
        assert p_before[k].tobytes() == p_after[k].tobytes(), k
    tp.assert_planes(p_after, tp.planes_of(levels_of(name, kname, W, H, SPP, 2, True, 3), SPP, 3), "path, frame 2")
    assert_planes(c2, expect(name, kname, W, H, SPP, 2, 3, levels=3), "frame 2")
    assert_planes(c3, expect(name, kname, W, H, SPP, 3, 2, levels=3), "frame 3")
    g.close()


@pytest.mark.gpu
def test_rebuild_ordering_and_two_streams(gpu, bihrt_mod):
    """Colour calls of one tree back to back on two streams with different
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


def checksum(planes):
    """path_rgb_smoke.c's: the sum, modulo 2^64, of (i + 1) * word_i over the planes' 32-bit words."""
    words = np.concatenate([np.ascontiguousarray(planes[k]).view(np.uint32).reshape(-1) for k in NAMES])
    with np.errstate(over="ignore"):
        return int((np.arange(1, words.size + 1, dtype=np.uint64) * words.astype(np.uint64)).sum(dtype=np.uint64))


@pytest.mark.gpu
def test_c_caller(tmp_path, gpu, bihrt_mod):
    """tests/c/path_rgb_smoke.c -- bih_build + bih_tree_set_materials +
    bih_render_path_rgb from strict C11 (cornell with its materials, 64x48x4,
    the reference camera, a sky dome, 3 bounces): its checksum is the one of the
    device entry's planes."""
    exe = _build_c(tmp_path)
    tris = scene("cornell")[0]
    w, h, spp, nb = 64, 48, 4, 3
    dl = bihrt_mod.scenes.sky_dome(2)
    pal, ids = bihrt_mod.scenes.cornell_materials()
    sp, lp, mp, ip = (tmp_path / n for n in ("scene.f32", "dir.f32", "mat.bin", "ids.u32"))
    tris.tofile(sp)
    dl.tofile(lp)
    pal.tofile(mp)
    ids.tofile(ip)
    r = subprocess.run([exe, str(sp), str(tris.shape[0]), str(w), str(h), str(spp), "0", str(lp), str(dl.shape[0]),
                        str(mp), str(pal.shape[0]), str(ip), "0.25", "0.3", "0.4", str(nb)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "path_rgb_smoke OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
    g = bihrt_mod.GPUArrayManager(tris)
    g.set_materials(pal, ids)
    ref = dev_rgb(bihrt_mod.Renderer(g, w, h, spp=spp), dl, None, None, nb, 0)
    g.close()
    rad = ref["radiance"]
    assert (rad[..., 0] != rad[..., 1]).any() and ref["lits"][nb - 1].any()
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("checksum ")]
    assert len(line) == 1 and int(line[0].split()[1], 16) == checksum(ref), (line, hex(checksum(ref)))


@pytest.mark.gpu
def test_app_writes_ppm(tmp_path, gpu, bihrt_mod):
    """python -m bihrt --scene cornell --direct --bounce A,S --bounces 3 --colour:
    the PPM of render_path_rgb's rgba plane with cornell_materials(), sky
    (S, S, S), the lamp by emission and no other light; red and green show."""
    from bihrt.app import main
    out, want = tmp_path / "c.ppm", tmp_path / "want.ppm"
    assert main(["--scene", "cornell", "--width", "64", "--height", "48", "--frames", "1", "--direct", str(out),
                 "--bounce", "0.5,0.25", "--bounces", "3", "--colour"]) == 0
    g = bihrt_mod.GPUArrayManager(bihrt_mod.scenes.cornell())
    g.set_materials(*bihrt_mod.scenes.cornell_materials())
    ref = bihrt_mod.Renderer(g, 64, 48).render_path_rgb(None, None, None, (.25, .25, .25), 3, 0,
                                                        planes=("rgba",))["rgba"]
    g.close()
    bihrt_mod.write_ppm(str(want), ref)
    assert open(out, "rb").read() == open(want, "rb").read()
    px = bihrt_mod.unpack_rgba(ref).reshape(-1, 4).astype(int)
    assert (px[:, 0] > px[:, 1] + 40).any() and (px[:, 1] > px[:, 0] + 40).any()     # a red and a green wall
