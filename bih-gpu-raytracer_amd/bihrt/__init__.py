"""bihrt -- Python host side of the MI355X BIH ray tracer.

Mirrors the reference's host interface for the hot path
(rehakvoj1/BIH-GPU-Raytracer, BIH_Raytracer/BIH_Raytracer/src):

  GPUArrayManager  (GPUArrayManager.h:6-56)  -> bihrt.GPUArrayManager: owns the
                   scene soup and the BIH on one device (bih_build/bih_rebuild)
  Renderer.Init / Render / Launch_cudaRender (Renderer.h:18-27) ->
                   bihrt.Renderer: camera, framebuffer, persistent RNG state,
                   render(g_odata) per frame

Everything runs through libbih_amd.so (HIP, gfx950); there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import scenes  # noqa: F401
from ._lib import (PARAM_BINS_CAP, PARAM_FORCE_FALLBACK, PARAM_ITEM_TILES, PARAM_PAIR_CAP, PARAM_STATIC_SOUP,
                   PARAM_TEST_ALLOC_FAIL, PARAM_TRACE_LDS_SLOTS, PARAM_WHITTED_COUNTERS, PARAM_GBUFFER_MASK,
                   AREA_LIGHT_DTYPE, MAX_AREA_LIGHTS, AreaLight, LightSet, BOUNCE_SLOT, Bounce, Indirect,
                   MAX_BOUNCES, Path, MATERIAL_DTYPE, MAX_MATERIALS, Material, PathRgb, MAT_DIFFUSE, MAT_MIRROR,
                   DENOISE_PARAMS, DENOISE_DEFAULTS, DENOISE_MAX_PASSES, DENOISE_MAX_SQUARINGS, DENOISE_MAX_PIXELS,
                   DenoiseParams,
                   NO_HIT, LIGHT_DTYPE, POINT_LIGHT_DTYPE, MAX_LIGHTS, SHADOW_T_LO, QUERY_CLOSEST, QUERY_OCCLUDED,
                   QUERY_T_HI, QUERY_CLOSEST_WITHIN, QUERY_OCCLUDED_WITHIN, PointLight, Direct, GBuffer, Hit, Light, Ray, TRAVERSE_ANYHIT,
                   TRAVERSE_REFERENCE, BihError, Camera, Framebuffer, Rows, Scene, TreeInfo, check, load)
from . import _lib

SCREEN_WIDTH, SCREEN_HEIGHT, RAYS_PER_PIXEL, SEED = 640, 480, 4, 1984   # Constants.h:4-8, :458


def device_count() -> int:
    return load().bih_device_count()


def camera_reference(w: int, h: int) -> Camera:
    cam = Camera()
    check(load().bih_camera_reference(w, h, C.byref(cam)), "bih_camera_reference")
    return cam


def camera_ray_bound(cam: Camera) -> np.ndarray:
    """bih_camera_ray_bound: per-component bound of |D| over the camera's
    primary rays (host only; sizes the any-hit walk's miss-proof boxes)."""
    out = (C.c_float * 3)()
    check(load().bih_camera_ray_bound(C.byref(cam), out), "bih_camera_ray_bound")
    return np.array(out[:], np.float32)


# numpy views of bih_ray / bih_hit arrays (`reserved` and `t_hi`: two names of the last float)
RAY_DTYPE = np.dtype({"names": ["o", "t_lo", "d", "reserved", "t_hi"],
                      "formats": [(np.float32, 3), np.float32, (np.float32, 3), np.float32, np.float32],
                      "offsets": [0, 12, 16, 28, 28], "itemsize": 32})
HIT_DTYPE = np.dtype([("t", np.float32), ("u", np.float32), ("v", np.float32), ("prim", np.uint32)])


# G-buffer pixel planes (bih_gbuffer): name -> (dtype, components per pixel)
GBUFFER_PLANES = {"depth": (np.float32, 1), "prim": (np.uint32, 1), "bary": (np.float32, 2),
                  "normal": (np.float32, 3), "coverage": (np.uint32, 1)}


# the planes of a direct-lighting render (bih_direct): name -> (dtype, values
# per pixel; 0: one per sample); lights are LIGHT_DTYPE arrays (bih_light)
DIRECT_PLANES = {"lit": (np.uint64, 0), "irradiance": (np.float32, 1), "rgba": (np.uint32, 1)}


# the planes of an indirect-lighting render (bih_indirect), as DIRECT_PLANES;
# "bounce" holds HIT_DTYPE records
INDIRECT_PLANES = {"lit": (np.uint64, 0), "bounce": (HIT_DTYPE, 0), "lit2": (np.uint64, 0),
                   "irradiance": (np.float32, 1), "rgba": (np.uint32, 1)}
INDIRECT = tuple(INDIRECT_PLANES)


# the planes of a path render (bih_path), as INDIRECT_PLANES; values per pixel
# -1: one per sample and level ("bounces" and "lits", level-major)
PATH_PLANES = {"lit": (np.uint64, 0), "bounces": (HIT_DTYPE, -1), "lits": (np.uint64, -1),
               "irradiance": (np.float32, 1), "rgba": (np.uint32, 1)}
PATH = tuple(PATH_PLANES)


# the planes of a colour path render (bih_path_rgb), as PATH_PLANES; "radiance"
# holds R, G, B per pixel
PATH_RGB_PLANES = {"lit": (np.uint64, 0), "bounces": (HIT_DTYPE, -1), "lits": (np.uint64, -1),
                   "radiance": (np.float32, 3), "rgba": (np.uint32, 1)}
PATH_RGB = tuple(PATH_RGB_PLANES)


# the outputs of a denoise call (bih_denoise*): name -> (dtype, values per pixel)
DENOISE_PLANES = {"radiance": (np.float32, 3), "rgba": (np.uint32, 1)}


def denoise_params(params=None) -> DenoiseParams:
    """A bih_denoise_params from None (DENOISE_DEFAULTS: 3 passes, 5 normal
    squarings, sigma_colour 2.0, sigma_plane 0.05), a DenoiseParams, or a
    sequence (passes[, normal_squarings[, sigma_colour[, sigma_plane]]])."""
    if isinstance(params, DenoiseParams):
        return params
    v = list(params) if params is not None else []
    v += list(DENOISE_DEFAULTS[len(v):])
    return DenoiseParams(int(v[0]), int(v[1]), float(v[2]), float(v[3]))


def _rows_ref(rows: Rows | None):
    """The bih_rows * argument of an optional Rows (NULL: the whole image)."""
    return C.byref(rows) if rows is not None else None


def _device_planes(st, known, ptrs: dict):
    """Fills the plane struct `st` (GBuffer, Direct) from {name: device pointer};
    KeyError on a name not in `known`."""
    for name, ptr in ptrs.items():
        if name not in known:
            raise KeyError(name)
        setattr(st, name, ptr or None)
    return st


def pack_lights(lights) -> np.ndarray:
    """(k,) LIGHT_DTYPE array (bih_light records) of a LIGHT_DTYPE array or of
    (k, 4) rows {dir.x, dir.y, dir.z, weight}."""
    a = np.asarray(lights)
    if a.dtype != LIGHT_DTYPE:
        a = np.ascontiguousarray(a, np.float32).reshape(-1, 4).view(LIGHT_DTYPE).reshape(-1)
    return np.ascontiguousarray(a).reshape(-1)


def pack_point_lights(lights) -> np.ndarray:
    """(k,) POINT_LIGHT_DTYPE array (bih_point_light records) of such an array or
    of (k, 4) rows {pos.x, pos.y, pos.z, weight}."""
    a = np.asarray(lights)
    if a.dtype != POINT_LIGHT_DTYPE:
        a = np.ascontiguousarray(a, np.float32).reshape(-1, 4).view(POINT_LIGHT_DTYPE).reshape(-1)
    return np.ascontiguousarray(a).reshape(-1)


def pack_area_lights(lights) -> np.ndarray:
    """(k,) AREA_LIGHT_DTYPE array (bih_area_light records) of such an array or
    of (k, 10) rows {corner, edge_u, edge_v, weight}."""
    a = np.asarray(lights)
    if a.dtype != AREA_LIGHT_DTYPE:
        rows = np.ascontiguousarray(a, np.float32).reshape(-1, 10)
        a = np.zeros(rows.shape[0], AREA_LIGHT_DTYPE)
        a["corner"], a["edge_u"], a["edge_v"], a["weight"] = rows[:, 0:3], rows[:, 3:6], rows[:, 6:9], rows[:, 9]
    return np.ascontiguousarray(a).reshape(-1)


def pack_materials(materials) -> np.ndarray:
    """(k,) MATERIAL_DTYPE array (bih_material records) of such an array or of
    (k, 6) rows {albedo R G B, emission R G B}, or (k, 7) rows with the kind
    (MAT_DIFFUSE, MAT_MIRROR) as the seventh value."""
    a = np.asarray(materials)
    if a.dtype != MATERIAL_DTYPE:
        rows = np.ascontiguousarray(a, np.float32)
        rows = rows.reshape(-1, 7 if rows.ndim == 2 and rows.shape[1] == 7 else 6)
        a = np.zeros(rows.shape[0], MATERIAL_DTYPE)
        a["albedo"], a["emission"] = rows[:, 0:3], rows[:, 3:6]
        if rows.shape[1] == 7:
            a["kind"] = rows[:, 6].astype(np.uint32)
    return np.ascontiguousarray(a).reshape(-1)


def area_light_sample(light, j: int, seed: int, pixel: int, frame: int, spp: int, s: int) -> np.ndarray:
    """bih_area_light_sample (host only): the point (3,) float32 of area light
    j -- `light`, one AREA_LIGHT_DTYPE record or a 10-float row -- that sample s
    of global pixel `pixel` = y*w + x uses in frame `frame` at spp samples."""
    lt = pack_area_lights(light)
    if lt.shape[0] != 1:
        raise ValueError("area_light_sample takes one light")
    q = (C.c_float * 3)()
    check(load().bih_area_light_sample(C.c_void_p(lt.ctypes.data), j, seed, pixel, frame, spp, s, q),
          "bih_area_light_sample")
    return np.array(q[:], np.float32)


def bounce_sample(seed: int, pixel: int, frame: int, spp: int, s: int, n) -> np.ndarray:
    """bih_bounce_sample (host only): the bounce direction B (3,) float32 that
    sample s of global pixel `pixel` = y*w + x uses in frame `frame` at spp
    samples for the normal n."""
    nn = (C.c_float * 3)(*[float(x) for x in np.asarray(n, np.float32).reshape(3)])
    d = (C.c_float * 3)()
    check(load().bih_bounce_sample(seed, pixel, frame, spp, s, nn, d), "bih_bounce_sample")
    return np.array(d[:], np.float32)


def path_sample(seed: int, pixel: int, frame: int, spp: int, s: int, level: int, n) -> np.ndarray:
    """bih_path_sample (host only): the direction B_k (3,) float32 of level
    `level` = k (1 .. MAX_BOUNCES) of a path, as bounce_sample; level 1 is
    bounce_sample's."""
    nn = (C.c_float * 3)(*[float(x) for x in np.asarray(n, np.float32).reshape(3)])
    d = (C.c_float * 3)()
    check(load().bih_path_sample(seed, pixel, frame, spp, s, level, nn, d), "bih_path_sample")
    return np.array(d[:], np.float32)


def pack_rays(orig, dirs, t_lo=0.0, t_hi=None) -> np.ndarray:
    """(n,) RAY_DTYPE array (bih_ray records) of origins, directions and t_lo;
    t_hi (a scalar or (n,), for the segment queries) goes into the last float,
    which stays 0 when it is not given."""
    orig = np.asarray(orig, np.float32).reshape(-1, 3)
    dirs = np.asarray(dirs, np.float32).reshape(-1, 3)
    if orig.shape != dirs.shape:
        raise ValueError("orig and dirs must hold the same number of rays")
    rays = np.zeros(orig.shape[0], RAY_DTYPE)
    rays["o"], rays["d"] = orig, dirs
    rays["t_lo"] = np.broadcast_to(np.asarray(t_lo, np.float32), (orig.shape[0],))
    if t_hi is not None:
        rays["t_hi"] = np.broadcast_to(np.asarray(t_hi, np.float32), (orig.shape[0],))
    return rays


class GPUArrayManager:
    """Scene + BIH on one device.  `tris` is a float32 (n, 9) soup."""

    def __init__(self, tris: np.ndarray, device: int = 0):
        self.tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
        self.scene = Scene(self.tris.shape[0], self.tris.ctypes.data)
        self.device = device
        self._tree = C.c_void_p()
        check(load().bih_build(C.byref(self.scene), device, C.byref(self._tree)), "bih_build")

    @classmethod
    def from_device(cls, ptr: int, n_tris: int, device: int = 0, stream: int | None = None):
        """Builds from a device-resident soup (e.g. a torch tensor's data_ptr())."""
        self = cls.__new__(cls)
        self.tris, self.scene, self.device = None, None, device
        self._tree = C.c_void_p()
        check(load().bih_build_device(C.c_void_p(ptr), n_tris, device, C.c_void_p(stream or 0),
                                      C.byref(self._tree)), "bih_build_device")
        return self

    @property
    def handle(self):
        return self._tree

    def rebuild(self):
        check(load().bih_rebuild(self._tree), "bih_rebuild")

    def info(self) -> TreeInfo:
        inf = TreeInfo()
        check(load().bih_tree_get_info(self._tree, C.byref(inf)), "bih_tree_get_info")
        return inf

    def set_param(self, param: int, value: int):
        """bih_tree_set_param (PARAM_*): work-order and test knobs; none changes a pixel."""
        check(load().bih_tree_set_param(self._tree, param, value), "bih_tree_set_param")

    def set_materials(self, materials, tri_material=None):
        """bih_tree_set_materials (synchronous; host arrays, copied): the tree's
        palette -- MATERIAL_DTYPE records or (k, 6) rows {albedo, emission} (or (k, 7)
        with the kind, which render_path_spec alone honours) -- and
        per triangle in file order the index of its material (None: every
        triangle uses material 0).  materials None or empty: the tree's
        materials are removed.  Ids stay valid across rebuild()."""
        pal = pack_materials(materials) if materials is not None else np.zeros(0, MATERIAL_DTYPE)
        ids = np.ascontiguousarray(tri_material, np.uint32).reshape(-1) if tri_material is not None else None
        if ids is not None and ids.shape[0] != self.info().n_tris:
            raise ValueError("tri_material holds one id per triangle")
        check(load().bih_tree_set_materials(self._tree, C.c_void_p(pal.ctypes.data) if pal.shape[0] else None,
                                            pal.shape[0], C.c_void_p(ids.ctypes.data) if ids is not None else None),
              "bih_tree_set_materials")

    def reserve(self, w: int, h: int, spp: int, rows: Rows | None = None, max_frames: int = 1):
        """bih_reserve: size every per-call buffer of renders of this shape (calls
        of up to max_frames frames) now, so that a frame loop allocates nothing."""
        check(load().bih_reserve(self._tree, w, h, spp, _rows_ref(rows), max_frames), "bih_reserve")

    def bins_stats(self):
        """Frustum bins of the current camera and image (bih_bins_get_stats)."""
        from ._lib import BinsStats
        st = BinsStats()
        check(load().bih_bins_get_stats(self._tree, C.byref(st)), "bih_bins_get_stats")
        return st

    def bins_solid_masks(self):
        """(sure words [tiles_y, tiles_x] uint16, solid tile count) of the
        current camera's bins (bih_bins_solid_masks; diagnostic)."""
        st = self.bins_stats()
        out = np.zeros((st.tiles_y, st.tiles_x), np.uint16)
        n = C.c_uint32(0)
        check(load().bih_bins_solid_masks(self._tree, out.ctypes.data_as(C.POINTER(C.c_uint16)), out.size,
                                          C.byref(n)), "bih_bins_solid_masks")
        return out, int(n.value)

    def export(self, which: int, dtype) -> np.ndarray:
        n = C.c_size_t(0)
        check(load().bih_tree_export(self._tree, which, None, C.byref(n)), "bih_tree_export")
        out = np.zeros(n.value // np.dtype(dtype).itemsize, dtype)
        check(load().bih_tree_export(self._tree, which, out.ctypes.data, C.byref(n)), "bih_tree_export")
        return out

    def trace(self, orig, dirs, t_lo=0.0, query: int = QUERY_CLOSEST, t_hi=None):
        """Ray queries for host rays (bih_trace; synchronous).  orig, dirs: (n, 3)
        float32; t_lo: a scalar or (n,).  QUERY_CLOSEST returns a dict of `t`, `u`,
        `v` (float32) and `prim` (uint32 file-order triangle, NO_HIT on a miss);
        QUERY_OCCLUDED a uint8 array (1: some triangle is hit).  The segment
        queries QUERY_CLOSEST_WITHIN / QUERY_OCCLUDED_WITHIN answer the same for
        hits with t < t_hi (a scalar or (n,)) only."""
        rays = pack_rays(orig, dirs, t_lo, t_hi)
        n = rays.shape[0]
        closest = (query & ~QUERY_T_HI) == QUERY_CLOSEST
        out = np.zeros(n, HIT_DTYPE if closest else np.uint8)
        check(load().bih_trace(self._tree, C.c_void_p(rays.ctypes.data), n, query,
                               C.c_void_p(out.ctypes.data)), "bih_trace")
        if not closest:
            return out
        return {k: np.ascontiguousarray(out[k]) for k in ("t", "u", "v", "prim")}

    def trace_device(self, rays_ptr: int, n: int, out_ptr: int, query: int = QUERY_CLOSEST,
                     stream: int | None = None):
        """Asynchronous ray queries on device memory (bih_trace_device): n bih_ray
        (32 bytes each, see pack_rays) at rays_ptr, results to out_ptr (16-byte
        bih_hit per ray, or one byte per ray for QUERY_OCCLUDED)."""
        check(load().bih_trace_device(self._tree, C.c_void_p(rays_ptr), n, query, C.c_void_p(out_ptr),
                                      C.c_void_p(stream or 0)), "bih_trace_device")

    def sync(self, stream: int | None = None):
        check(load().bih_sync(self._tree, C.c_void_p(stream or 0)), "bih_sync")

    def arrays(self) -> dict:
        """Canonical arrays under the oracle's names (OracleTree attributes)."""
        a = {
            "morton": self.export(_lib.ARR_MORTON_SORTED, np.uint32),
            "tri_idx": self.export(_lib.ARR_TRI_INDEX, np.uint32),
            "unique_mc": self.export(_lib.ARR_UNIQUE_MC, np.uint32),
            "dup_cnt": self.export(_lib.ARR_DUP_COUNT, np.uint32),
            "first_idx": self.export(_lib.ARR_FIRST_IDX, np.int32),
            "leaf_parent": self.export(_lib.ARR_LEAF_PARENT, np.int32),
            "clip": self.export(_lib.ARR_CLIP, np.float32).reshape(-1, 2),
            "axis": self.export(_lib.ARR_AXIS, np.int32),
            "children": self.export(_lib.ARR_CHILDREN, np.int32).reshape(-1, 2),
            "is_leaf": self.export(_lib.ARR_IS_LEAF, np.uint8).reshape(-1, 2),
            "parent": self.export(_lib.ARR_PARENT, np.int32),
            "lo": self.export(_lib.ARR_TRI_LO, np.float32).reshape(-1, 3),
            "hi": self.export(_lib.ARR_TRI_HI, np.float32).reshape(-1, 3),
        }
        inf = self.info()
        a["scene_lo"] = np.array(inf.scene_lo[:], np.float32)
        a["scene_hi"] = np.array(inf.scene_hi[:], np.float32)
        return a

    def close(self):
        if getattr(self, "_tree", None) and self._tree.value:
            load().bih_free(self._tree)
            self._tree = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Renderer:
    """Per-frame renderer over a GPUArrayManager (Renderer::Render, Renderer.cpp:415)."""

    def __init__(self, arrays: GPUArrayManager, w: int = SCREEN_WIDTH, h: int = SCREEN_HEIGHT,
                 spp: int = RAYS_PER_PIXEL, seed: int = SEED, camera: Camera | None = None):
        self.arrays, self.w, self.h, self.spp, self.seed = arrays, w, h, spp, seed
        self.camera = camera if camera is not None else camera_reference(w, h)
        self.frame = 0

    def render(self, frame: int | None = None, rows: tuple[int, int] | None = None,
               out: np.ndarray | None = None) -> np.ndarray:
        """One frame into a host (h, w) uint32 image (0x00BBGGRR, row 0 = bottom).
        `out`: a caller-owned C-contiguous (nrows, w) uint32 framebuffer to render
        into (a frame loop reuses it; see host_register)."""
        f = self.frame if frame is None else frame
        row0, nrows = rows if rows is not None else (0, self.h)
        if out is None:
            out = np.zeros((nrows, self.w), np.uint32)
        elif out.shape != (nrows, self.w) or out.dtype != np.uint32 or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous ({nrows}, {self.w}) uint32 array")
        fb = Framebuffer(self.w, self.h, self.spp, f, self.seed, out.ctypes.data)
        sc = C.byref(self.arrays.scene) if self.arrays.scene is not None else None
        if rows is None:
            check(load().bih_render(sc, self.arrays.handle, C.byref(self.camera), C.byref(fb)), "bih_render")
        else:
            check(load().bih_render_rows(sc, self.arrays.handle, C.byref(self.camera), C.byref(fb),
                                         row0, nrows), "bih_render_rows")
        self.frame = f + 1
        return out

    def render_device(self, out_ptr: int, frame: int, rows: Rows | None = None,
                      traverse: int = TRAVERSE_ANYHIT, stats_ptr: int | None = None,
                      stream: int | None = None):
        """Asynchronous device-resident render into out_ptr (u32, nrows*w)."""
        check(load().bih_render_device(self.arrays.handle, C.byref(self.camera), self.w, self.h,
                                       self.spp, frame, self.seed, _rows_ref(rows), traverse,
                                       C.c_void_p(out_ptr), C.c_void_p(stats_ptr or 0),
                                       C.c_void_p(stream or 0)), "bih_render_device")

    def render_device_frames(self, out_ptr: int, frame0: int, nframes: int, out_stride: int,
                             rows: Rows | None = None, stream: int | None = None):
        """Frames frame0 .. frame0+nframes-1 (any-hit) in one call
        (bih_render_device_frames); frame j at out_ptr + 4*j*out_stride bytes."""
        check(load().bih_render_device_frames(self.arrays.handle, C.byref(self.camera), self.w, self.h,
                                              self.spp, frame0, nframes, self.seed, _rows_ref(rows),
                                              C.c_void_p(out_ptr), out_stride, C.c_void_p(stream or 0)),
              "bih_render_device_frames")

    def render_whitted(self, frame: int | None = None) -> np.ndarray:
        """Config C4: one frame of 8-bounce mirror rays (bih_render_whitted) into a
        host (h, w) uint32 image."""
        f = self.frame if frame is None else frame
        out = np.zeros((self.h, self.w), np.uint32)
        fb = Framebuffer(self.w, self.h, self.spp, f, self.seed, out.ctypes.data)
        sc = C.byref(self.arrays.scene) if self.arrays.scene is not None else None
        check(load().bih_render_whitted(sc, self.arrays.handle, C.byref(self.camera), C.byref(fb)),
              "bih_render_whitted")
        self.frame = f + 1
        return out

    def render_whitted_device(self, out_ptr: int, frame: int, rows: Rows | None = None,
                              hits_ptr: int | None = None, stream: int | None = None):
        """Asynchronous C4 render into out_ptr (u32, nrows*w); hits_ptr (optional,
        u32 per sample) receives each sample's hit count along its mirror path."""
        check(load().bih_render_whitted_device(self.arrays.handle, C.byref(self.camera), self.w, self.h,
                                               self.spp, frame, self.seed, _rows_ref(rows),
                                               C.c_void_p(out_ptr), C.c_void_p(hits_ptr or 0),
                                               C.c_void_p(stream or 0)), "bih_render_whitted_device")

    def render_gbuffer(self, frame: int | None = None, rows: Rows | None = None,
                       planes=("depth", "prim", "bary", "normal", "coverage"), hits: bool = False) -> dict:
        """One frame's G-buffer into host arrays (bih_render_gbuffer; synchronous):
        a dict of the pixel planes asked for (GBUFFER_PLANES), shaped (nrows, w) or
        (nrows, w, k), from each pixel's hit sample of smallest (t, s); with
        `hits` also "hits", (nrows*w*spp,) HIT_DTYPE, sample = local pixel * spp + s.
        A pixel without a hit holds FLT_MAX, NO_HIT, zeros and coverage 0."""
        f = self.frame if frame is None else frame
        nrows = rows.nrows if rows is not None else self.h
        out, gb = {}, GBuffer()
        for name in planes:
            dt, k = GBUFFER_PLANES[name]
            out[name] = np.zeros((nrows, self.w) + ((k,) if k > 1 else ()), dt)
            setattr(gb, name, out[name].ctypes.data)
        if hits:
            out["hits"] = np.zeros(nrows * self.w * self.spp, HIT_DTYPE)
            gb.hits = out["hits"].ctypes.data
        check(load().bih_render_gbuffer(self.arrays.handle, C.byref(self.camera), self.w, self.h, self.spp, f,
                                        self.seed, _rows_ref(rows), C.byref(gb)),
              "bih_render_gbuffer")
        self.frame = f + 1
        return out

    def render_gbuffer_device(self, ptrs: dict, frame: int, rows: Rows | None = None, stream: int | None = None):
        """Asynchronous G-buffer render into device memory (bih_render_gbuffer_device):
        ptrs maps plane names ("hits", "depth", "prim", "bary", "normal", "coverage")
        to device pointers; planes left out are not written."""
        gb = _device_planes(GBuffer(), ("hits", *GBUFFER_PLANES), ptrs)
        check(load().bih_render_gbuffer_device(self.arrays.handle, C.byref(self.camera), self.w, self.h, self.spp,
                                               frame, self.seed, _rows_ref(rows),
                                               C.byref(gb), C.c_void_p(stream or 0)), "bih_render_gbuffer_device")

    def _host_planes(self, st, table, planes, rows, n_bounces: int = 0):
        """Zeroed host arrays of the planes asked for, by name, shaped as their
        *_PLANES table says (values per pixel k > 0: (nrows, w) or (nrows, w, k);
        0: one per sample; -1: (n_bounces, samples)), and the plane struct `st`
        (Direct, Indirect, Path, PathRgb) pointing at them."""
        nrows = rows.nrows if rows is not None else self.h
        S = nrows * self.w * self.spp
        out = {}
        for name in planes:
            dt, k = table[name]
            shape = (nrows, self.w) + ((k,) if k > 1 else ()) if k > 0 else ((n_bounces, S) if k < 0 else S)
            out[name] = np.zeros(shape, dt)
            setattr(st, name, out[name].ctypes.data)
        return out, st

    def render_direct(self, lights, frame: int | None = None, rows: Rows | None = None,
                      planes=("lit", "irradiance", "rgba")) -> dict:
        """One frame's direct lighting into host arrays (bih_render_direct;
        synchronous).  lights: a LIGHT_DTYPE array or (k, 4) rows {dir, weight},
        k <= MAX_LIGHTS, dir towards the light (scenes.sky_dome makes a sky).
        Returns a dict of the planes asked for (DIRECT_PLANES): "lit"
        (nrows*w*spp,) uint64, bit k = light k reaches sample p*spp + s;
        "irradiance" (nrows, w) float32; "rgba" (nrows, w) uint32 grey."""
        f = self.frame if frame is None else frame
        lt = pack_lights(lights)
        out, dp = self._host_planes(Direct(), DIRECT_PLANES, planes, rows)
        check(load().bih_render_direct(self.arrays.handle, C.byref(self.camera), self.w, self.h, self.spp, f,
                                       self.seed, _rows_ref(rows),
                                       C.c_void_p(lt.ctypes.data), lt.shape[0], C.byref(dp)), "bih_render_direct")
        self.frame = f + 1
        return out

    def render_direct_device(self, ptrs: dict, lights, frame: int, rows: Rows | None = None,
                             stream: int | None = None):
        """Asynchronous direct-lighting render into device memory
        (bih_render_direct_device): ptrs maps plane names ("lit", "irradiance",
        "rgba") to device pointers; planes left out are not written.  lights is
        host memory (as render_direct's), copied by the call."""
        dp = _device_planes(Direct(), DIRECT_PLANES, ptrs)
        lt = pack_lights(lights)
        check(load().bih_render_direct_device(self.arrays.handle, C.byref(self.camera), self.w, self.h, self.spp,
                                              frame, self.seed, _rows_ref(rows),
                                              C.c_void_p(lt.ctypes.data), lt.shape[0], C.byref(dp),
                                              C.c_void_p(stream or 0)), "bih_render_direct_device")

    def _lights_args(self, dir_lights, point_lights):
        dl = pack_lights(dir_lights if dir_lights is not None else np.zeros((0, 4), np.float32))
        pl = pack_point_lights(point_lights if point_lights is not None else np.zeros((0, 4), np.float32))
        return (dl, pl, C.c_void_p(dl.ctypes.data if dl.shape[0] else 0), dl.shape[0],
                C.c_void_p(pl.ctypes.data if pl.shape[0] else 0), pl.shape[0])

    def render_lights(self, dir_lights, point_lights, frame: int | None = None, rows: Rows | None = None,
                      planes=("lit", "irradiance", "rgba")) -> dict:
        """render_direct with point lights next to the directional ones
        (bih_render_lights; synchronous).  dir_lights as render_direct's lights,
        point_lights a POINT_LIGHT_DTYPE array or (k, 4) rows {pos, weight}
        (scenes.lamps makes some); either may be None or empty, together 1 ..
        MAX_LIGHTS.  Bit k of "lit" is directional light k, bit len(dir_lights)
        + j point light j, which a triangle behind it does not shadow."""
        f = self.frame if frame is None else frame
        dl, pl, dptr, nd, pptr, npt = self._lights_args(dir_lights, point_lights)
        out, dp = self._host_planes(Direct(), DIRECT_PLANES, planes, rows)
        check(load().bih_render_lights(self.arrays.handle, C.byref(self.camera), self.w, self.h, self.spp, f,
                                       self.seed, _rows_ref(rows),
                                       dptr, nd, pptr, npt, C.byref(dp)), "bih_render_lights")
        self.frame = f + 1
        return out

    def render_lights_device(self, ptrs: dict, dir_lights, point_lights, frame: int, rows: Rows | None = None,
                             stream: int | None = None):
        """Asynchronous render_lights into device memory (bih_render_lights_device);
        ptrs as render_direct_device's.  Both light arrays are host memory, copied
        by the call."""
        dp = _device_planes(Direct(), DIRECT_PLANES, ptrs)
        dl, pl, dptr, nd, pptr, npt = self._lights_args(dir_lights, point_lights)
        check(load().bih_render_lights_device(self.arrays.handle, C.byref(self.camera), self.w, self.h, self.spp,
                                              frame, self.seed, _rows_ref(rows),
                                              dptr, nd, pptr, npt, C.byref(dp), C.c_void_p(stream or 0)),
              "bih_render_lights_device")

    def _light_set(self, dir_lights, point_lights, area_lights):
        dl, pl, dptr, nd, pptr, npt = self._lights_args(dir_lights, point_lights)
        al = pack_area_lights(area_lights if area_lights is not None else np.zeros((0, 10), np.float32))
        ls = LightSet(dptr, nd, pptr, npt, C.c_void_p(al.ctypes.data if al.shape[0] else 0), al.shape[0])
        return (dl, pl, al), ls   # (the arrays stay alive as long as the first element does)

    def _host_call(self, fn: str, st, table, planes, lights, extra, frame, rows, n_bounces: int = 0) -> dict:
        """A host entry that takes a bih_light_set: `fn` names the C function, `st`
        and `table` are its plane struct and *_PLANES, `lights` the three light
        arrays, `extra` its arguments between the light set and the planes."""
        f = self.frame if frame is None else frame
        keep, ls = self._light_set(*lights)
        out, st = self._host_planes(st, table, planes, rows, n_bounces)
        check(getattr(load(), fn)(self.arrays.handle, C.byref(self.camera), self.w, self.h, self.spp, f, self.seed,
                                  _rows_ref(rows), C.byref(ls), *extra, C.byref(st)), fn)
        del keep
        self.frame = f + 1
        return out

    def _device_call(self, fn: str, st, table, ptrs: dict, lights, extra, frame, rows, stream):
        """The device entry next to _host_call's: ptrs maps plane names to device pointers."""
        st = _device_planes(st, table, ptrs)
        keep, ls = self._light_set(*lights)
        check(getattr(load(), fn)(self.arrays.handle, C.byref(self.camera), self.w, self.h, self.spp, frame, self.seed,
                                  _rows_ref(rows), C.byref(ls), *extra, C.byref(st), C.c_void_p(stream or 0)), fn)
        del keep

    def render_area_lights(self, dir_lights, point_lights, area_lights, frame: int | None = None,
                           rows: Rows | None = None, planes=("lit", "irradiance", "rgba")) -> dict:
        """render_lights with area lights (soft shadows) next to the others
        (bih_render_area_lights; synchronous).  area_lights: an AREA_LIGHT_DTYPE
        array or (k, 10) rows {corner, edge_u, edge_v, weight}, k <=
        MAX_AREA_LIGHTS (scenes.panels makes two); any of the three may be None
        or empty, together 1 .. MAX_LIGHTS.  Bit len(dir_lights) +
        len(point_lights) + j of "lit" is area light j: per sample one shadow
        ray to a point of the panel (area_light_sample)."""
        return self._host_call("bih_render_area_lights", Direct(), DIRECT_PLANES, planes,
                               (dir_lights, point_lights, area_lights), (), frame, rows)

    def render_area_lights_device(self, ptrs: dict, dir_lights, point_lights, area_lights, frame: int,
                                  rows: Rows | None = None, stream: int | None = None):
        """Asynchronous render_area_lights into device memory
        (bih_render_area_lights_device); ptrs as render_direct_device's.  The
        light arrays are host memory, copied by the call."""
        self._device_call("bih_render_area_lights_device", Direct(), DIRECT_PLANES, ptrs,
                          (dir_lights, point_lights, area_lights), (), frame, rows, stream)

    @staticmethod
    def _bounce(bounce) -> Bounce:
        """A Bounce of a Bounce or of (albedo, sky)."""
        return bounce if isinstance(bounce, Bounce) else Bounce(float(bounce[0]), float(bounce[1]))

    def render_indirect(self, dir_lights, point_lights, area_lights, bounce, frame: int | None = None,
                        rows: Rows | None = None, planes=INDIRECT) -> dict:
        """render_area_lights plus one bounce of indirect light and a sky term
        (bih_render_indirect; synchronous).  bounce: a Bounce or (albedo, sky).
        All three light arrays may be None or empty: the sky-only
        (ambient-occlusion) render.  Returns a dict of the planes asked for
        (INDIRECT_PLANES): "lit" and "lit2" (nrows*w*spp,) uint64 of the primary
        and the bounce hit, "bounce" (nrows*w*spp,) HIT_DTYPE, the bounce ray's
        closest hit, "irradiance" (nrows, w) float32, "rgba" (nrows, w) uint32."""
        return self._host_call("bih_render_indirect", Indirect(), INDIRECT_PLANES, planes,
                               (dir_lights, point_lights, area_lights), (C.byref(self._bounce(bounce)),), frame, rows)

    def render_indirect_device(self, ptrs: dict, dir_lights, point_lights, area_lights, bounce, frame: int,
                               rows: Rows | None = None, stream: int | None = None):
        """Asynchronous render_indirect into device memory
        (bih_render_indirect_device): ptrs maps plane names (INDIRECT_PLANES) to
        device pointers; planes left out are not written.  The light arrays and
        bounce are host memory, copied by the call."""
        self._device_call("bih_render_indirect_device", Indirect(), INDIRECT_PLANES, ptrs,
                          (dir_lights, point_lights, area_lights),
                          (C.byref(self._bounce(bounce)),), frame, rows, stream)

    def render_path(self, dir_lights, point_lights, area_lights, bounce, n_bounces: int, frame: int | None = None,
                    rows: Rows | None = None, planes=PATH) -> dict:
        """render_indirect carried on for n_bounces (1 .. MAX_BOUNCES) levels
        (bih_render_path; synchronous): a sample's path goes on from each bounce
        hit until a ray escapes or level n_bounces is reached.  Returns a dict
        of the planes asked for (PATH_PLANES): "lit" (nrows*w*spp,) uint64 of
        the primary hit, "bounces" (n_bounces, nrows*w*spp) HIT_DTYPE and "lits"
        (n_bounces, nrows*w*spp) uint64, row k-1 level k's bounce records and
        lit words, "irradiance" (nrows, w) float32, "rgba" (nrows, w) uint32.
        With n_bounces = 1 they are render_indirect's planes."""
        return self._host_call("bih_render_path", Path(), PATH_PLANES, planes,
                               (dir_lights, point_lights, area_lights),
                               (C.byref(self._bounce(bounce)), n_bounces), frame, rows, n_bounces)

    def render_path_device(self, ptrs: dict, dir_lights, point_lights, area_lights, bounce, n_bounces: int,
                           frame: int, rows: Rows | None = None, stream: int | None = None):
        """Asynchronous render_path into device memory (bih_render_path_device):
        ptrs maps plane names (PATH_PLANES) to device pointers; planes left out
        are not written.  The light arrays and bounce are host memory, copied by
        the call."""
        self._device_call("bih_render_path_device", Path(), PATH_PLANES, ptrs,
                          (dir_lights, point_lights, area_lights),
                          (C.byref(self._bounce(bounce)), n_bounces), frame, rows, stream)

    @staticmethod
    def _sky3(sky):
        return (C.c_float * 3)(*[float(x) for x in np.asarray(sky, np.float32).reshape(3)])

    def render_path_rgb(self, dir_lights, point_lights, area_lights, sky, n_bounces: int, frame: int | None = None,
                        rows: Rows | None = None, planes=PATH_RGB) -> dict:
        """render_path with the tree's materials (GPUArrayManager.set_materials)
        and an RGB sky, a 3-vector (bih_render_path_rgb; synchronous).  Returns
        a dict of the planes asked for (PATH_RGB_PLANES): "lit", "bounces",
        "lits" and "rgba" as render_path's, "radiance" (nrows, w, 3) float32."""
        return self._host_call("bih_render_path_rgb", PathRgb(), PATH_RGB_PLANES, planes,
                               (dir_lights, point_lights, area_lights),
                               (self._sky3(sky), n_bounces), frame, rows, n_bounces)

    def render_path_rgb_device(self, ptrs: dict, dir_lights, point_lights, area_lights, sky, n_bounces: int,
                               frame: int, rows: Rows | None = None, stream: int | None = None):
        """Asynchronous render_path_rgb into device memory
        (bih_render_path_rgb_device): ptrs maps plane names (PATH_RGB_PLANES) to
        device pointers; planes left out are not written.  The light arrays and
        sky are host memory, copied by the call."""
        self._device_call("bih_render_path_rgb_device", PathRgb(), PATH_RGB_PLANES, ptrs,
                          (dir_lights, point_lights, area_lights), (self._sky3(sky), n_bounces), frame, rows, stream)

    def render_path_spec(self, dir_lights, point_lights, area_lights, sky, n_bounces: int, frame: int | None = None,
                         rows: Rows | None = None, planes=PATH_RGB) -> dict:
        """render_path_rgb honouring the materials' kinds: a path that lands on a
        MAT_MIRROR material goes on along the reflection and gathers no light
        there (bih_render_path_spec; synchronous).  The planes are
        render_path_rgb's."""
        return self._host_call("bih_render_path_spec", PathRgb(), PATH_RGB_PLANES, planes,
                               (dir_lights, point_lights, area_lights),
                               (self._sky3(sky), n_bounces), frame, rows, n_bounces)

    def render_path_spec_device(self, ptrs: dict, dir_lights, point_lights, area_lights, sky, n_bounces: int,
                                frame: int, rows: Rows | None = None, stream: int | None = None):
        """Asynchronous render_path_spec into device memory
        (bih_render_path_spec_device), as render_path_rgb_device."""
        self._device_call("bih_render_path_spec_device", PathRgb(), PATH_RGB_PLANES, ptrs,
                          (dir_lights, point_lights, area_lights), (self._sky3(sky), n_bounces), frame, rows, stream)

    def denoise(self, radiance, depth, normal, params=None, planes=("radiance", "rgba")) -> dict:
        """The edge-avoiding a-trous filter over a whole frame's host planes
        (bih_denoise; synchronous): `radiance` (h, w, 3) float32 as
        render_path_rgb's or render_path_spec's, `depth` (h, w) and `normal`
        (h, w, 3) as render_gbuffer's under this renderer's camera.  params: see
        denoise_params (default 3 passes, 5 normal squarings, sigma_colour 2.0,
        sigma_plane 0.05; sigma_plane is in scene units, the distance of a tap from
        the centre's tangent plane at which its weight reaches 0).  Returns a
        dict of the planes asked for (DENOISE_PLANES): "radiance" (h, w, 3)
        float32, "rgba" (h, w) uint32.  Pixels the G-buffer missed pass through."""
        prm = denoise_params(params)
        src = [np.ascontiguousarray(a, np.float32) for a in (radiance, depth, normal)]
        for a, k in zip(src, (3, 1, 3)):
            if a.size != self.h * self.w * k:
                raise ValueError(f"a plane of {a.size} values for a {self.w} x {self.h} frame")
        out, ptr = {}, {"radiance": None, "rgba": None}
        for name in planes:
            dt, k = DENOISE_PLANES[name]
            out[name] = np.zeros((self.h, self.w) + ((k,) if k > 1 else ()), dt)
            ptr[name] = out[name].ctypes.data
        check(load().bih_denoise(self.arrays.handle, C.byref(self.camera), self.w, self.h, C.byref(prm),
                                 src[0].ctypes.data, src[1].ctypes.data, src[2].ctypes.data, ptr["radiance"],
                                 ptr["rgba"]), "bih_denoise")
        return out

    def denoise_device(self, ptrs: dict, radiance_ptr: int, depth_ptr: int, normal_ptr: int, params=None,
                       stream: int | None = None):
        """Asynchronous denoise of device planes (bih_denoise_device): ptrs maps
        "radiance" and "rgba" (DENOISE_PLANES) to the output device pointers, an
        output left out is not written; ptrs["radiance"] may be radiance_ptr (in
        place).  The call runs on `stream` and is not ordered after renders on
        other streams: that is the caller's."""
        for name in ptrs:
            if name not in DENOISE_PLANES:
                raise KeyError(name)
        prm = denoise_params(params)
        check(load().bih_denoise_device(self.arrays.handle, C.byref(self.camera), self.w, self.h, C.byref(prm),
                                        C.c_void_p(radiance_ptr or 0), C.c_void_p(depth_ptr or 0),
                                        C.c_void_p(normal_ptr or 0), C.c_void_p(ptrs.get("radiance") or 0),
                                        C.c_void_p(ptrs.get("rgba") or 0), C.c_void_p(stream or 0)),
              "bih_denoise_device")

    def whitted_work(self) -> dict:
        """Per bounce d = 0..8 of the last Whitted render (run with
        PARAM_WHITTED_COUNTERS on): rays traced, BIH nodes entered, triangles
        tested (bih_whitted_work)."""
        n = 9
        rays, nodes, tris = (C.c_uint32 * n)(), (C.c_uint64 * n)(), (C.c_uint64 * n)()
        check(load().bih_whitted_work(self.arrays.handle, rays, nodes, tris), "bih_whitted_work")
        return {"rays": list(rays), "nodes": list(nodes), "tris": list(tris)}

    def render_history(self, n: int) -> np.ndarray:
        """(n, 3) ms {kernel start, kernel end, end of the render's work} of the
        last n renders (issued with set_timing on), after the oldest one's kernel
        start (bih_render_history)."""
        t = (C.c_double * (3 * n))()
        check(load().bih_render_history(self.arrays.handle, n, t), "bih_render_history")
        return np.array(t[:], np.float64).reshape(n, 3)

    def sync(self, stream: int | None = None):
        check(load().bih_sync(self.arrays.handle, C.c_void_p(stream or 0)), "bih_sync")

    def set_timing(self, on: bool = True):
        """Record device-time events around every render (bih_set_timing)."""
        check(load().bih_set_timing(self.arrays.handle, 1 if on else 0), "bih_set_timing")

    def last_render_ms(self) -> float:
        ms = C.c_double(0.0)
        check(load().bih_last_render_ms(self.arrays.handle, C.byref(ms)), "bih_last_render_ms")
        return ms.value

    def last_render_times(self) -> tuple[float, float]:
        """(main render kernel ms, ms of the render call's device work after it:
        k_render_fallback for frustum-bin renders)."""
        k, t = C.c_double(0.0), C.c_double(0.0)
        check(load().bih_last_render_times(self.arrays.handle, C.byref(k), C.byref(t)),
              "bih_last_render_times")
        return k.value, t.value


def host_register(arr: np.ndarray):
    """Page-locks a host framebuffer (bih_host_register) so that bih_render's
    device-to-host copy into it runs at DMA rate; host_unregister before it is
    freed."""
    check(load().bih_host_register(C.c_void_p(arr.ctypes.data), arr.nbytes), "bih_host_register")


def host_unregister(arr: np.ndarray):
    check(load().bih_host_unregister(C.c_void_p(arr.ctypes.data)), "bih_host_unregister")


def load_obj(path: str) -> np.ndarray:
    """Wavefront OBJ -> float32 (n, 9) soup in file order (bih_scene_load_obj;
    Model::LoadModel + App::LoadModels flattening, Model.cpp:10-95,
    App.cpp:65-121).  Raises BihError (BIH_ERR_IO / BIH_ERR_PARSE with the line)."""
    sc = Scene()
    line = C.c_uint32(0)
    rc = load().bih_scene_load_obj(os.fsencode(path), C.byref(sc), C.byref(line))
    if rc != _lib.BIH_OK:
        raise BihError(rc, f"bih_scene_load_obj({path!r})" + (f" line {line.value}" if line.value else ""))
    try:
        if sc.n_tris == 0:
            return np.zeros((0, 9), np.float32)
        return np.ctypeslib.as_array(C.cast(sc.v, C.POINTER(C.c_float)), (sc.n_tris, 9)).copy()
    finally:
        load().bih_scene_free(C.byref(sc))


class Model:
    """Model(path) (Model.h / Model.cpp:6-8): the triangles of one OBJ file."""

    def __init__(self, path: str):
        self.path = path
        self.triangles = load_obj(path)

    def __len__(self):
        return self.triangles.shape[0]


def unpack_rgba(img: np.ndarray) -> np.ndarray:
    """0x00BBGGRR -> (..., 4) uint8 RGBA (alpha byte as stored, 0)."""
    return img.astype("<u4").view(np.uint8).reshape(img.shape + (4,))


def write_ppm(path: str, img: np.ndarray):
    """PPM (P6) with row 0 at the bottom, as the GL quad shows it."""
    rgb = unpack_rgba(img)[::-1, :, :3]
    h, w = img.shape
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(np.ascontiguousarray(rgb).tobytes())


__all__ = ["GPUArrayManager", "Renderer", "Model", "load_obj", "host_register", "host_unregister", "Camera", "Rows", "BihError", "camera_reference",
           "camera_ray_bound", "device_count", "unpack_rgba", "write_ppm", "scenes", "TRAVERSE_ANYHIT",
           "TRAVERSE_REFERENCE", "PARAM_ITEM_TILES", "PARAM_PAIR_CAP", "PARAM_BINS_CAP", "PARAM_FORCE_FALLBACK",
           "PARAM_WHITTED_COUNTERS", "PARAM_STATIC_SOUP", "PARAM_TEST_ALLOC_FAIL", "PARAM_TRACE_LDS_SLOTS",
           "PARAM_GBUFFER_MASK", "GBuffer", "GBUFFER_PLANES", "QUERY_CLOSEST", "QUERY_OCCLUDED", "NO_HIT", "Ray", "Hit", "RAY_DTYPE", "HIT_DTYPE", "pack_rays",
           "Light", "Direct", "LIGHT_DTYPE", "DIRECT_PLANES", "MAX_LIGHTS", "SHADOW_T_LO", "pack_lights",
           "QUERY_T_HI", "QUERY_CLOSEST_WITHIN", "QUERY_OCCLUDED_WITHIN", "PointLight", "POINT_LIGHT_DTYPE",
           "pack_point_lights", "AreaLight", "LightSet", "AREA_LIGHT_DTYPE", "MAX_AREA_LIGHTS",
           "pack_area_lights", "area_light_sample", "Bounce", "Indirect", "INDIRECT", "INDIRECT_PLANES",
           "BOUNCE_SLOT", "bounce_sample", "Path", "PATH", "PATH_PLANES", "MAX_BOUNCES", "path_sample",
           "MATERIAL_DTYPE", "Material", "PathRgb", "PATH_RGB", "PATH_RGB_PLANES", "MAX_MATERIALS", "pack_materials",
           "MAT_DIFFUSE", "MAT_MIRROR", "DENOISE_PARAMS", "DenoiseParams", "DENOISE_DEFAULTS", "DENOISE_PLANES",
           "DENOISE_MAX_PASSES", "DENOISE_MAX_SQUARINGS", "DENOISE_MAX_PIXELS", "denoise_params"]
