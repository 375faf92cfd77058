"""The denoiser (bih_denoise / bih_denoise_device): the
edge-avoiding a-trous filter over a colour render's radiance, guided by the
G-buffer's depth and normal.

Expected values come from `restate`, a numpy restatement of the header kept
here: f32 throughout (asserted), np.fmax / np.fmin (which return the non-NaN
operand, as fmaxf does), vectorised over pixels with a loop over the 25 taps in
the header's order.  Planes are compared on bits, NaN as NaN
(test_indirect.cplane).  The class input is the oracle's: cornell under K1 at
48 x 32 x 4, 3 bounces, frame 0 of test_path_rgb.expect with the guides of
test_gbuffer.expected.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import test_gbuffer as tg
import test_path_rgb as trgb
from conftest import ROOT
from test_direct import MISS_SHADE
from test_gbuffer import F32, FLT_MAX, LIBDIR, SEED, camera, expected, renderer, scene, tree
from test_indirect import cplane, lights_of
from test_path import FRAME, H, SPP, W
from test_path_rgb import SKY3

SRC = os.path.join(ROOT, "tests", "c", "denoise_smoke.c")
NAME, KNAME, NB = "cornell", "K1", 3        # the class input
CLASS = (3, 5, 1.0, 0.05)                   # the params its conditions were counted under
NAMES = ("radiance", "rgba")
KERN = np.array([0.375, 0.25, 0.0625], F32)


# --- the header, restated ---------------------------------------------------------

def positions(cam, w, h, depth):
    """Pos (h, w, 3) f32: origin + depth * d, d the G-buffer's ray through the pixel centre."""
    cam = np.asarray(cam, F32)
    xs = np.arange(w, dtype=F32)[None, :]
    ys = np.arange(h, dtype=F32)[:, None]
    with np.errstate(all="ignore"):
        u = (xs + F32(0.5)) / F32(w)
        v = (ys + F32(0.5)) / F32(h)
        pos = np.stack([cam[a] + depth * (((cam[3 + a] + u * cam[6 + a]) + v * cam[9 + a]) - cam[a])
                        for a in range(3)], -1)
    assert pos.dtype == F32 and pos.shape == (h, w, 3)
    return pos


def support(x):
    """g(x) = t*t, t = fmaxf(0, 1 - x)."""
    t = np.fmax(F32(0), F32(1) - x)
    return t * t


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def restate(cam, w, h, params, radiance, depth, normal, counts=None):
    """The header's C_passes (h, w, 3) f32 and rgba (h, w) u32.  counts (a dict):
    receives, over the non-centre taps inside the image between two valid
    pixels, "taps" and how many have wn == 0, wn > 0 with wp == 0, both > 0 with
    wc == 0, and 0 < w < k."""
    passes, squarings, sigma_colour, sigma_plane = params
    col = np.ascontiguousarray(radiance, F32).reshape(h, w, 3).copy()
    depth = np.ascontiguousarray(depth, F32).reshape(h, w)
    nrm = np.ascontiguousarray(normal, F32).reshape(h, w, 3)
    with np.errstate(all="ignore"):
        valid = depth < F32(FLT_MAX)
    pos = positions(cam, w, h, depth)
    sigma_plane = F32(sigma_plane)
    if counts is not None:
        counts.update(taps=0, wn0=0, wp0=0, wc0=0, partial=0)
    with np.errstate(all="ignore"):
        for i in range(passes):
            s = 1 << i
            sc = np.ldexp(F32(sigma_colour), -i)
            assert sc.dtype == F32
            sc2 = sc * sc
            tot = np.zeros((h, w, 3), F32)
            wsum = np.zeros((h, w), F32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    k = KERN[abs(dx)] * KERN[abs(dy)]
                    if dx == 0 and dy == 0:
                        tot = tot + k * col
                        wsum = wsum + k
                        continue
                    ox, oy = dx * s, dy * s
                    x0, x1, y0, y1 = max(0, -ox), min(w, w - ox), max(0, -oy), min(h, h - oy)
                    if x0 >= x1 or y0 >= y1:
                        continue
                    p = (slice(y0, y1), slice(x0, x1))
                    q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                    m = np.fmax(F32(0), dot3(nrm[p], nrm[q]))
                    for _ in range(squarings):
                        m = m * m
                    wp = support(np.abs(dot3(nrm[p], pos[q] - pos[p])) / sigma_plane)
                    dc = col[q] - col[p]
                    wc = support(dot3(dc, dc) / sc2)
                    wt = ((k * m) * wp) * wc
                    assert wt.dtype == F32 and k.dtype == F32
                    both = valid[p] & valid[q]
                    on = both & (wt > 0)
                    tot[p] = np.where(on[..., None], tot[p] + wt[..., None] * col[q], tot[p])
                    wsum[p] = np.where(on, wsum[p] + wt, wsum[p])
                    if counts is not None:
                        counts["taps"] += int(both.sum())
                        counts["wn0"] += int((both & (m == 0)).sum())
                        counts["wp0"] += int((both & (m > 0) & (wp == 0)).sum())
                        counts["wc0"] += int((both & (m > 0) & (wp > 0) & (wc == 0)).sum())
                        counts["partial"] += int((both & (wt > 0) & (wt < k)).sum())
            col = np.where(valid[..., None], tot / wsum[..., None], col)
            assert col.dtype == F32
        g8 = np.fmax(F32(0), np.fmin(F32(255), F32(255) * col)).astype(np.int32).astype(np.uint32)
    shade = g8[..., 0] | (g8[..., 1] << 8) | (g8[..., 2] << 16)
    rgba = np.where(valid, shade, np.uint32(MISS_SHADE)).astype(np.uint32)
    return {"radiance": col, "rgba": rgba}


@functools.lru_cache(maxsize=None)
def class_input(frame=FRAME):
    """(cam, radiance (H, W, 3), depth, normal) of the class frame; read-only."""
    cam = camera(NAME, KNAME, W, H)
    rad = np.ascontiguousarray(trgb.expect(NAME, KNAME, W, H, SPP, frame, NB, levels=NB)["radiance"], F32)
    rad = rad.reshape(H, W, 3)
    gb = expected(NAME, KNAME, W, H, SPP, frame)
    rad.setflags(write=False)
    return cam, rad, gb["depth"], gb["normal"]


@functools.lru_cache(maxsize=None)
def class_expect(params):
    cam, rad, depth, nrm = class_input()
    out = restate(cam, W, H, params, rad, depth, nrm)
    for a in out.values():
        a.setflags(write=False)
    return out


def synthetic(w, h, seed, invalid=0.25, cam_of=(NAME, KNAME)):
    """Seeded guides of a w x h frame: unit normals scattered about +z, depths in
    [1, 1.5), colours in [0, 2), `invalid` of the pixels at the G-buffer's miss values."""
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(h, w, 3)) * 0.4 + np.array([0.0, 0.0, 1.0])
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F32)
    depth = (1.0 + 0.5 * rng.random((h, w))).astype(F32)
    rad = (2.0 * rng.random((h, w, 3))).astype(F32)
    miss = rng.random((h, w)) < invalid
    depth[miss] = FLT_MAX
    n[miss] = 0
    return camera(*cam_of, w, h), rad, depth, n


def centre_only(rad):
    """What a valid pixel none of whose other taps contributes comes out as: (k*C)/k."""
    k = KERN[0] * KERN[0]
    with np.errstate(all="ignore"):
        out = (k * np.asarray(rad, F32)) / k
    assert out.dtype == F32
    return out


def assert_planes(got, exp, what="", names=NAMES):
    for name in names:
        g, e = got[name], np.asarray(exp[name]).reshape(got[name].shape)
        assert g.dtype == e.dtype, f"{what}: {name} {g.dtype}"
        bad = np.argwhere(cplane(g) != cplane(e))
        assert bad.size == 0, f"{what}: {name} differs at {bad[:4].tolist()} ({bad.shape[0]} values)"


class Dev:
    """The device planes of a denoise call (torch tensors; the outputs prefilled with 0xAB)."""

    def __init__(self, w, h, rad, depth, nrm):
        import torch
        self.w, self.h = w, h
        self.src = [torch.from_numpy(np.ascontiguousarray(a, F32).reshape(-1).copy()).cuda() for a in (rad, depth, nrm)]
        self.t = {"radiance": torch.full((w * h * 12,), 0xAB, dtype=torch.uint8, device="cuda"),
                  "rgba": torch.full((w * h * 4,), 0xAB, dtype=torch.uint8, device="cuda")}
        torch.cuda.synchronize()

    def launch(self, r, params, names=NAMES, stream=None, inplace=False):
        ptrs = {k: self.t[k].data_ptr() for k in names}
        if inplace:
            ptrs["radiance"] = self.src[0].data_ptr()
        r.denoise_device(ptrs, self.src[0].data_ptr(), self.src[1].data_ptr(), self.src[2].data_ptr(), params, stream)

    def result(self, inplace=False):
        rad = self.src[0].cpu().numpy() if inplace else self.t["radiance"].cpu().numpy().view(F32)
        return {"radiance": rad.reshape(self.h, self.w, 3),
                "rgba": self.t["rgba"].cpu().numpy().view(np.uint32).reshape(self.h, self.w)}


def dev_denoise(r, rad, depth, nrm, params, names=NAMES, inplace=False):
    dv = Dev(r.w, r.h, rad, depth, nrm)
    dv.launch(r, params, names, inplace=inplace)
    r.sync()
    return dv.result(inplace)


def renderer_of(w, h, cam):
    import bihrt
    return bihrt.Renderer(tree(NAME), w, h, spp=SPP, seed=SEED, camera=bihrt.Camera.from_list(cam))


def run_both(w, h, cam, rad, depth, nrm, params, what):
    """The device entry against the restatement; returns the restatement."""
    exp = restate(cam, w, h, params, rad, depth, nrm)
    assert_planes(dev_denoise(renderer_of(w, h, cam), rad, depth, nrm, params), exp, what)
    return exp


@pytest.fixture(scope="module", autouse=True)
def _free_trees():
    yield
    while tg._trees:
        tg._trees.popitem()[1].close()


# --- CPU ------------------------------------------------------------------------

def test_struct_layout(bihrt_mod):
    D = bihrt_mod.DENOISE_PARAMS
    assert D is bihrt_mod.DenoiseParams and issubclass(D, C.Structure) and C.sizeof(D) == 16
    assert [(n, getattr(D, n).offset, getattr(D, n).size) for n, _ in D._fields_] == \
        [("passes", 0, 4), ("normal_squarings", 4, 4), ("sigma_colour", 8, 4), ("sigma_plane", 12, 4)]
    assert D._fields_[0][1] is C.c_uint32 and D._fields_[1][1] is C.c_uint32
    assert D._fields_[2][1] is C.c_float and D._fields_[3][1] is C.c_float
    d = bihrt_mod.denoise_params()
    assert (d.passes, d.normal_squarings, d.sigma_colour, d.sigma_plane) == (3, 5, 2.0, F32(0.05))
    assert bihrt_mod.DENOISE_DEFAULTS == (3, 5, 2.0, 0.05)
    d = bihrt_mod.denoise_params((8, 0, 1.5))
    assert (d.passes, d.normal_squarings, d.sigma_colour, d.sigma_plane) == (8, 0, 1.5, F32(0.05))
    assert bihrt_mod.denoise_params(d) is d
    assert bytes(D(1, 2, 1.0, 2.0)) == np.array([1, 2], np.uint32).tobytes() + np.array([1, 2], F32).tobytes()
    assert (bihrt_mod.DENOISE_MAX_PASSES, bihrt_mod.DENOISE_MAX_SQUARINGS, bihrt_mod.DENOISE_MAX_PIXELS) == \
        (8, 8, 1 << 28)
    assert bihrt_mod.DENOISE_PLANES == {"radiance": (np.float32, 3), "rgba": (np.uint32, 1)}
    for name in ("DENOISE_PARAMS", "DENOISE_DEFAULTS", "DENOISE_PLANES", "denoise_params"):
        assert name in bihrt_mod.__all__, name
    for name in ("denoise", "denoise_device"):
        assert hasattr(bihrt_mod.Renderer, name), name


def test_header_symbols_exported(bihrt_mod):
    names = bihrt_mod._lib.exported_symbols_from_header()
    L = bihrt_mod._lib.load()
    for sym in ("bih_denoise", "bih_denoise_device"):
        assert sym in names and getattr(L, sym) is not None, sym
    hdr = open(os.path.join(ROOT, "include", "bih.h")).read()
    assert "#define BIH_ABI_VERSION 4" in hdr and "#define BIH_DENOISE_MAX_PASSES 8" in hdr
    assert "#define BIH_DENOISE_MAX_SQUARINGS 8" in hdr and "#define BIH_DENOISE_MAX_PIXELS (1u << 28)" in hdr
    assert "bih_denoise*" in hdr.split("error codes")[0]          # the "added since" list
    assert L.bih_abi_version() == 4


def _header_compiles(tmp_path, cc, std, ext):
    src = tmp_path / ("hdr." + ext)
    src.write_text('#include "bih.h"\n'
                   "int main(void) { bih_denoise_params p = {3, 5, 2.0f, 0.05f}; float x[3] = {0, 0, 0};\n"
                   "  return bih_denoise(0, 0, 1, 1, &p, x, x, x, x, 0) == BIH_ERR_INVALID && sizeof p == 16 &&\n"
                   "         bih_denoise_device(0, 0, 1, 1, &p, x, x, x, x, 0, 0) == BIH_ERR_INVALID ? 0 : 1; }\n")
    subprocess.run([cc, "-std=" + std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only",
                    "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_header_is_c11_and_cxx17(tmp_path):
    _header_compiles(tmp_path, "gcc", "c11", "c")
    _header_compiles(tmp_path, "g++", "c++17", "cpp")


def test_device_free_error_codes(bihrt_mod):
    """Both entries' checks in the header's order, before the tree or a device
    is touched: a stand-in tree pointer is never dereferenced."""
    L = bihrt_mod._lib.load()
    INVALID, TOO_LARGE = -1, -6
    raw = (C.c_char * 96)()
    base = (C.addressof(raw) + 15) & ~15
    fake = C.c_void_p(base)
    cam = bihrt_mod.Camera()
    D = bihrt_mod.DENOISE_PARAMS
    good = D(3, 5, 2.0, 0.05)
    for entry in (lambda *a: L.bih_denoise_device(*a, None), L.bih_denoise):
        def call(t, c, w, h, p, rad=base, depth=base, nrm=base, out=base, rgba=base):
            return entry(t, C.byref(c) if c is not None else None, w, h, C.byref(p) if p is not None else None,
                         rad, depth, nrm, out, rgba)
        # 1: NULL tree, camera, params (each before everything after it)
        assert call(None, cam, 8, 8, good) == INVALID
        assert call(fake, None, 8, 8, good) == INVALID
        assert call(fake, cam, 8, 8, None) == INVALID
        # 2: an empty frame
        assert call(fake, cam, 0, 8, good) == INVALID and call(fake, cam, 8, 0, good) == INVALID
        # 3, 4: passes, squarings -- before 5, a frame that is too large
        for p in (D(0, 5, 2.0, 0.05), D(9, 5, 2.0, 0.05), D(3, 9, 2.0, 0.05)):
            assert call(fake, cam, 8, 8, p) == INVALID
            assert call(fake, cam, 1 << 16, 1 << 16, p) == INVALID
        # 5: w*h > 2^28 (no wrap at 2^32) -- before 6 and 7, the planes
        assert call(fake, cam, 1 << 16, 1 << 16, good) == TOO_LARGE
        assert call(fake, cam, 1 << 14, (1 << 14) + 1, good, None, None, None, None, None) == TOO_LARGE
        assert call(fake, cam, (1 << 28) + 1, 1, good, rad=None) == TOO_LARGE
        # 6: an input missing -- before 7
        for k in ("rad", "depth", "nrm"):
            assert call(fake, cam, 8, 8, good, **{k: None}) == INVALID
            assert call(fake, cam, 8, 8, good, out=None, rgba=None, **{k: None}) == INVALID
        assert call(fake, cam, 1 << 14, 1 << 14, good, nrm=None) == INVALID      # 2^28 pixels are not too many
        # 7: no output
        assert call(fake, cam, 8, 8, good, out=None, rgba=None) == INVALID
        # every limit itself passes the checks it belongs to (the next one stops the call)
        for p in (D(1, 0, 0.0, 0.0), D(8, 8, float("inf"), float("nan"))):
            assert call(fake, cam, 1 << 14, 1 << 14, p, out=None, rgba=None) == INVALID
            assert call(fake, cam, 1 << 14, (1 << 14) + 1, p) == TOO_LARGE


def test_app_denoise_options(bihrt_mod):
    """--denoise without --colour, or with a bad value, is an argument error
    before any device is used."""
    from bihrt.app import main
    base = ["--scene", "cornell", "--frames", "1"]
    colour = ["--direct", "d.ppm", "--bounce", "0.5", "--bounces", "2", "--colour"]
    for extra in (["--denoise"],
                  ["--direct", "d.ppm", "--denoise"],
                  ["--direct", "d.ppm", "--bounce", "0.5", "--bounces", "2", "--denoise", "3"],
                  colour + ["--denoise", "0"],
                  colour + ["--denoise", "9"],
                  colour + ["--denoise", "2.5"],
                  colour + ["--denoise", "x"],
                  colour + ["--denoise", "3,1,0.05,7"]):
        with pytest.raises(SystemExit):
            main(base + extra)


def _build_c(tmp_path) -> str:
    exe = str(tmp_path / "denoise_smoke")
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


def test_restatement_conditions(bihrt_mod):
    """The conditions the class input stands for, on the restatement: every
    branch of a tap's weight is taken often, nearly every valid pixel changes,
    every output is finite, and with the default params the filtered frame is
    closer to the 64-spp mean of frames 1 .. 16 than the raw frame is."""
    cam, rad, depth, nrm = class_input()
    valid = depth < FLT_MAX
    c = {}
    out = restate(cam, W, H, CLASS, rad, depth, nrm, c)
    changed = int((cplane(out["radiance"]) != cplane(rad)).any(-1)[valid].sum())
    print("valid pixels", int(valid.sum()), "changed", changed, "taps", c)
    assert c["wn0"] >= 1000 and c["wp0"] >= 1000 and c["wc0"] >= 1000 and c["partial"] >= 1000, c
    assert c["wn0"] + c["wp0"] + c["wc0"] + c["partial"] <= c["taps"]
    assert int(valid.sum()) == 929 and changed >= 900
    assert np.isfinite(out["radiance"]).all() and np.isfinite(rad).all()
    assert np.array_equal(cplane(out["radiance"])[~valid], cplane(rad)[~valid]) and (~valid).any()
    assert (out["rgba"][~valid] == MISS_SHADE).all() and (out["rgba"][valid] != MISS_SHADE).any()
    # the default params against the 64-spp yardstick, over the hit pixels
    d = bihrt_mod.denoise_params()
    default = (d.passes, d.normal_squarings, d.sigma_colour, d.sigma_plane)
    assert default == (3, 5, 2.0, F32(0.05))
    truth = np.mean([class_input(f)[1].astype(np.float64) for f in range(1, 17)], 0)
    den = restate(cam, W, H, default, rad, depth, nrm)["radiance"]
    mse_raw = float(((rad - truth)[valid] ** 2).mean())
    mse_den = float(((den - truth)[valid] ** 2).mean())
    print("mean squared error against the mean of frames 1..16: raw", mse_raw, "denoised", mse_den)
    assert mse_den < mse_raw


# --- GPU ------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("passes", [1, 2, 3, 8])
def test_class_input(passes, gpu, bihrt_mod):
    """The oracle's frame at 48 x 32: at 8 passes the steps of passes 5 .. 8
    (32 .. 128) exceed the image in y, those of passes 6 .. 8 in x as well."""
    cam, rad, depth, nrm = class_input()
    params = (passes,) + CLASS[1:]
    exp = class_expect(params)
    assert (cplane(exp["radiance"]) != cplane(rad)).any()
    assert_planes(dev_denoise(renderer(tree(NAME), NAME, KNAME, W, H, SPP), rad, depth, nrm, params), exp,
                  f"{passes} passes")


@pytest.mark.gpu
def test_off_block_size(gpu, bihrt_mod):
    """67 x 45 (no multiple of a block's 32 x 8 pixels, several blocks each way), 4 passes, a quarter invalid."""
    w, h = 67, 45
    cam, rad, depth, nrm = synthetic(w, h, 1)
    exp = run_both(w, h, cam, rad, depth, nrm, (4, 1, 1.5, 1.0), "67x45")
    valid = depth < FLT_MAX
    assert (cplane(exp["radiance"]) != cplane(rad)).any(-1)[valid].mean() > 0.9


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (3, 70)])
def test_small_shapes(w, h, gpu, bihrt_mod):
    """Images smaller than a block, than 5 x 5 and than the stencil's reach."""
    cam, rad, depth, nrm = synthetic(w, h, 2, invalid=0.0)
    exp = run_both(w, h, cam, rad, depth, nrm, (3, 1, 4.0, 1.0), f"{w}x{h}")
    if (w, h) == (1, 1):
        assert np.array_equal(cplane(exp["radiance"]), cplane(centre_only(rad)))
    else:
        assert (cplane(exp["radiance"]) != cplane(rad)).any()


@pytest.mark.gpu
def test_no_valid_pixel_and_a_single_one(gpu, bihrt_mod):
    w, h = 40, 12
    cam, rad, depth, nrm = synthetic(w, h, 3, invalid=1.0)
    assert not (depth < FLT_MAX).any()
    exp = run_both(w, h, cam, rad, depth, nrm, (3, 1, 4.0, 1.0), "all invalid")
    assert np.array_equal(cplane(exp["radiance"]), cplane(rad)) and (exp["rgba"] == MISS_SHADE).all()
    depth = depth.copy()
    depth[7, 33] = 1.25
    nrm[7, 33] = (0, 0, 1)
    exp = run_both(w, h, cam, rad, depth, nrm, (3, 1, 4.0, 1.0), "one valid pixel")
    only = rad.copy()
    only[7, 33] = centre_only(centre_only(centre_only(rad[7, 33])))
    assert np.array_equal(cplane(exp["radiance"]), cplane(only))
    assert (exp["rgba"] != MISS_SHADE).sum() == 1 and exp["rgba"][7, 33] != MISS_SHADE


@pytest.mark.gpu
def test_non_finite_values_stay_where_they_are(gpu, bihrt_mod):
    """NaN, +inf and -inf in radiance, depth and normal at fixed pixels of a
    synthetic frame: the planes on bits, and a non-finite colour comes out on
    its own pixel and on no other."""
    w, h = 45, 33
    cam, rad, depth, nrm = synthetic(w, h, 4)
    nan, inf = F32("nan"), F32("inf")
    depth[2:31:4, 3:44:5] = 1.25                                   # the pixels below and some neighbours are valid
    for k, (y, x, v) in enumerate([(2, 3, nan), (6, 8, inf), (10, 13, -inf), (14, 18, nan), (18, 23, inf)]):
        rad[y, x, k % 3] = v
    for y, x, v in [(22, 28, nan), (26, 33, inf), (30, 38, -inf)]:
        depth[y, x] = v
    nrm[2, 23, 0] = nan
    bad_in = ~np.isfinite(rad).all(-1)
    assert bad_in.sum() == 5 and (depth[bad_in] < FLT_MAX).all()
    exp = run_both(w, h, cam, rad, depth, nrm, (4, 1, 1.5, 1.0), "non-finite")
    assert np.array_equal(~np.isfinite(exp["radiance"]).all(-1), bad_in)
    valid = depth < FLT_MAX
    assert (cplane(exp["radiance"]) != cplane(rad)).any(-1)[valid & ~bad_in].mean() > 0.9
    # an infinity in a normal is a guide's, not a colour's: wn = +inf where n_p . n_q is, the tap's weight is
    # +inf and inf / inf is NaN at the pixels whose stencil reaches it -- the header's arithmetic, on bits
    nrm[6, 28, 1], nrm[10, 33, 2] = inf, -inf
    exp = run_both(w, h, cam, rad, depth, nrm, (4, 1, 1.5, 1.0), "infinities in normals")
    spread = ~np.isfinite(exp["radiance"]).all(-1) & ~bad_in
    assert spread.any() and not spread[6, 28] and not spread[10, 33] and (depth[spread] < FLT_MAX).all()


@pytest.mark.gpu
@pytest.mark.parametrize("params", [(2, 5, float("inf"), 0.05), (2, 5, 0.0, 0.05), (2, 5, 1.0, float("inf")),
                                    (2, 5, 1.0, 0.0), (2, 0, 1.0, 0.05), (2, 8, 1.0, 0.05)])
def test_sigmas_and_squarings(params, gpu, bihrt_mod):
    """Each sigma at +inf (the term is off) and at 0 (the centre tap alone:
    nothing changes); 0 and 8 normal squarings."""
    cam, rad, depth, nrm = class_input()
    exp = class_expect(params)
    valid = depth < FLT_MAX
    alone = np.where(valid[..., None], centre_only(centre_only(rad)), rad)       # two passes of the centre tap alone
    unchanged = np.array_equal(cplane(exp["radiance"]), cplane(alone))
    assert unchanged == (0.0 in params[2:])
    for other in ((2, 5, 1.0, 0.05),):
        if params != other and not unchanged:
            assert not np.array_equal(cplane(exp["radiance"]), cplane(class_expect(other)["radiance"]))
    assert_planes(dev_denoise(renderer(tree(NAME), NAME, KNAME, W, H, SPP), rad, depth, nrm, params), exp, str(params))


@pytest.mark.gpu
def test_outputs_alone_in_place_and_host_entry(gpu, bihrt_mod):
    """Each output alone gives the bits of both together and leaves the other
    untouched; radiance_out == radiance works in place; the host entry equals
    the device entry."""
    cam, rad, depth, nrm = class_input()
    exp = class_expect(CLASS)
    r = renderer(tree(NAME), NAME, KNAME, W, H, SPP)
    for name, other in (NAMES, NAMES[::-1]):
        got = dev_denoise(r, rad, depth, nrm, CLASS, names=(name,))
        assert_planes(got, exp, f"{name} alone", names=(name,))
        assert (np.ascontiguousarray(got[other]).view(np.uint8) == 0xAB).all(), other
    assert_planes(dev_denoise(r, rad, depth, nrm, CLASS, inplace=True), exp, "in place")
    got = dev_denoise(r, rad, depth, nrm, CLASS, names=("radiance",), inplace=True)
    assert_planes(got, exp, "in place, radiance alone", names=("radiance",))
    host = r.denoise(rad, depth, nrm, CLASS)
    assert sorted(host) == sorted(NAMES) and host["radiance"].shape == (H, W, 3) and host["rgba"].shape == (H, W)
    assert_planes(host, exp, "host entry")
    for name in NAMES:
        one = r.denoise(rad, depth, nrm, CLASS, planes=(name,))
        assert list(one) == [name]
        assert_planes(one, exp, f"host entry, {name} alone", names=(name,))
    assert_planes(r.denoise(rad, depth, nrm), class_expect((3, 5, 2.0, 0.05)), "host entry, default params")


@pytest.mark.gpu
def test_end_to_end_on_one_stream(gpu, bihrt_mod):
    """render_path_spec_device -> render_gbuffer_device -> denoise_device on one
    stream, nothing waited for in between: the restatement of the oracle's
    planes.  (Every kind of test_path_rgb's palette is diffuse, so the mirror
    call's radiance is the colour call's, test_path_rgb.expect's.)"""
    import torch
    cam, rad, depth, nrm = class_input()
    exp = class_expect(CLASS)
    g = trgb.with_materials(NAME)
    r = renderer(g, NAME, KNAME, W, H, SPP)
    dl, lp, pan = lights_of(NAME)
    P = W * H
    d_rad = torch.full((3 * P,), -7.0, dtype=torch.float32, device="cuda")
    d_depth = torch.full((P,), -7.0, dtype=torch.float32, device="cuda")
    d_nrm = torch.full((3 * P,), -7.0, dtype=torch.float32, device="cuda")
    d_rgba = torch.zeros(P, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    r.render_path_spec_device({"radiance": d_rad.data_ptr()}, dl, lp, pan, SKY3, NB, FRAME, stream=s.cuda_stream)
    r.render_gbuffer_device({"depth": d_depth.data_ptr(), "normal": d_nrm.data_ptr()}, FRAME, stream=s.cuda_stream)
    r.denoise_device({"radiance": d_rad.data_ptr(), "rgba": d_rgba.data_ptr()}, d_rad.data_ptr(), d_depth.data_ptr(),
                     d_nrm.data_ptr(), CLASS, stream=s.cuda_stream)
    r.sync(s.cuda_stream)
    assert np.array_equal(cplane(d_depth.cpu().numpy().reshape(H, W)), cplane(depth))
    assert np.array_equal(cplane(d_nrm.cpu().numpy().reshape(H, W, 3)), cplane(nrm))
    got = {"radiance": d_rad.cpu().numpy().reshape(H, W, 3), "rgba": d_rgba.cpu().numpy().view(np.uint32).reshape(H, W)}
    assert_planes(got, exp, "end to end")


@pytest.mark.gpu
def test_two_streams_memory_and_steady_state(gpu, bihrt_mod):
    """Denoise calls of one tree back to back on two streams with different
    inputs and params (they share the record planes: each orders after the one
    before it); the scratch is 64 bytes per pixel in bih_tree_info, one
    allocation, and no call after the first of the shape allocates."""
    import torch
    w, h = 67, 45
    g = bihrt_mod.GPUArrayManager(scene(NAME)[0])
    ins = [synthetic(w, h, 10 + k) for k in range(3)]
    prm = [(4, 1, 1.5, 1.0), (2, 0, 4.0, 2.0), (3, 2, 1.0, 1.0)]
    exps = [restate(c[0], w, h, p, *c[1:]) for c, p in zip(ins, prm)]
    r = bihrt_mod.Renderer(g, w, h, spp=SPP, seed=SEED, camera=bihrt_mod.Camera.from_list(ins[0][0]))
    before = g.info()
    assert_planes(dev_denoise(r, *ins[0][1:], prm[0]), exps[0], "first call")
    first = g.info()
    assert first.device_allocs == before.device_allocs + 1 and first.device_bytes == before.device_bytes + 64 * w * h
    devs = [Dev(w, h, *c[1:]) for c in ins] + [Dev(w, h, *ins[0][1:])]
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    for dv, p, st in zip(devs, prm + prm[:1], (sa, sb, sa, sb)):
        dv.launch(r, p, stream=st.cuda_stream)
    sa.synchronize()
    sb.synchronize()
    for dv, e, k in zip(devs, exps + exps[:1], range(4)):
        assert_planes(dv.result(), e, f"call {k}")
    c = synthetic(16, 9, 20)
    small = bihrt_mod.Renderer(g, 16, 9, spp=SPP, seed=SEED, camera=bihrt_mod.Camera.from_list(c[0]))
    assert_planes(dev_denoise(small, *c[1:], prm[0]), restate(c[0], 16, 9, prm[0], *c[1:]), "a smaller frame")
    after = g.info()
    assert after.device_allocs == first.device_allocs and after.device_bytes == first.device_bytes
    host = r.denoise(*ins[1][1:], prm[1])                      # the host entry's planes: one more allocation, once
    assert_planes(host, exps[1], "host entry")
    staged = g.info()
    assert staged.device_allocs == after.device_allocs + 1
    assert staged.device_bytes == after.device_bytes + sum((k * w * h + 15) & ~15 for k in (12, 4, 12, 12, 4))
    assert_planes(r.denoise(*ins[2][1:], prm[2]), exps[2], "host entry again")
    last = g.info()
    assert last.device_allocs == staged.device_allocs and last.device_bytes == staged.device_bytes
    g.close()


@pytest.mark.gpu
def test_renders_undisturbed(gpu, bihrt_mod):
    """bih_render and bih_render_path_rgb before and after denoise calls give
    the same bytes (the call draws no random number and takes no render slot),
    and the denoise between them is right."""
    cam, rad, depth, nrm = class_input()
    tris, ot = scene(NAME)
    g = bihrt_mod.GPUArrayManager(tris)
    g.set_materials(trgb.palette(), trgb.ids_of(tris.shape[0]))
    r = renderer(g, NAME, KNAME, W, H, SPP)
    dl, lp, pan = lights_of(NAME)
    c_before = r.render_path_rgb(dl, lp, pan, SKY3, NB, FRAME)
    f0 = r.render(0)
    den = r.denoise(c_before["radiance"], depth, nrm, CLASS)
    f1 = r.render(1)
    c_after = r.render_path_rgb(dl, lp, pan, SKY3, NB, FRAME)
    f2 = r.render(2)
    for f, img in ((0, f0), (1, f1), (2, f2)):
        assert np.array_equal(img, ot.render(W, H, spp=SPP, frame=f, seed=SEED, cam=cam)[0]), f
    for k in trgb.NAMES:
        assert c_before[k].tobytes() == c_after[k].tobytes(), k
    assert np.array_equal(cplane(c_before["radiance"]), cplane(rad))
    assert_planes(den, class_expect(CLASS), "between the renders")
    g.close()


def checksum(planes):
    """tests/c/denoise_smoke.c's: the sum of (i + 1) * word_i over radiance, then rgba."""
    words = np.concatenate([np.ascontiguousarray(planes[k]).reshape(-1).view(np.uint32) for k in NAMES])
    i = np.arange(1, words.size + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int((i * words.astype(np.uint64)).sum(dtype=np.uint64))


@pytest.mark.gpu
def test_c_caller(tmp_path, gpu, bihrt_mod):
    """tests/c/denoise_smoke.c -- bih_build + bih_denoise from strict C11 on the
    planes of a 64 x 48 x 4 cornell frame under the reference camera (3 bounces,
    the scene's own materials): its checksum is the device entry's."""
    exe = _build_c(tmp_path)
    tris = bihrt_mod.scenes.cornell()
    w, h, prm = 64, 48, (3, 5, 2.0, 0.05)
    g = bihrt_mod.GPUArrayManager(tris)
    g.set_materials(*bihrt_mod.scenes.cornell_materials())
    r = bihrt_mod.Renderer(g, w, h, spp=SPP)
    rad = r.render_path_rgb(None, None, None, (.25, .25, .25), NB, 0, planes=("radiance",))["radiance"]
    gb = r.render_gbuffer(0, planes=("depth", "normal"))
    ref = dev_denoise(r, rad, gb["depth"], gb["normal"], prm)
    g.close()
    assert (cplane(ref["radiance"]) != cplane(rad)).any() and (ref["rgba"] != MISS_SHADE).any()
    paths = [tmp_path / n for n in ("scene.f32", "rad.f32", "depth.f32", "normal.f32")]
    for p, a in zip(paths, (tris, rad, gb["depth"], gb["normal"])):
        np.ascontiguousarray(a, F32).tofile(p)
    run = subprocess.run([exe, str(paths[0]), str(tris.shape[0]), str(w), str(h)] + [str(p) for p in paths[1:]] +
                         [str(prm[0]), str(prm[1]), repr(prm[2]), repr(prm[3])],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "denoise_smoke OK" in run.stdout and "FAIL" not in run.stdout, run.stdout + run.stderr
    line = [ln for ln in run.stdout.splitlines() if ln.startswith("checksum ")]
    assert len(line) == 1 and int(line[0].split()[1], 16) == checksum(ref), (line, hex(checksum(ref)))


@pytest.mark.gpu
def test_app_writes_denoised_ppm(tmp_path, gpu, bihrt_mod):
    """python -m bihrt --scene cornell --direct --bounce A,S --bounces 3 --colour
    --denoise 2,1.5: the PPM of Renderer.denoise's rgba over the frame's radiance
    and render_gbuffer's depth and normal; it is not the raw --colour image."""
    from bihrt.app import main
    out, plain, want = tmp_path / "d.ppm", tmp_path / "c.ppm", tmp_path / "want.ppm"
    common = ["--scene", "cornell", "--width", "64", "--height", "48", "--frames", "1", "--bounce", "0.5,0.25",
              "--bounces", "3", "--colour"]
    assert main(common + ["--direct", str(out), "--denoise", "2,1.5"]) == 0
    assert main(common + ["--direct", str(plain)]) == 0
    g = bihrt_mod.GPUArrayManager(bihrt_mod.scenes.cornell())
    g.set_materials(*bihrt_mod.scenes.cornell_materials())
    r = bihrt_mod.Renderer(g, 64, 48)
    rad = r.render_path_rgb(None, None, None, (.25, .25, .25), 3, 0, planes=("radiance",))["radiance"]
    gb = r.render_gbuffer(0, planes=("depth", "normal"))
    ref = r.denoise(rad, gb["depth"], gb["normal"], (2, 5, 1.5, 0.05), planes=("rgba",))["rgba"]
    g.close()
    bihrt_mod.write_ppm(str(want), ref)
    assert open(out, "rb").read() == open(want, "rb").read()
    assert open(out, "rb").read() != open(plain, "rb").read()
