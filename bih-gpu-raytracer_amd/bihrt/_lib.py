"""ctypes binding of libbih_amd.so (include/bih.h).

The library is built in-tree (`make -C bih-gpu-raytracer_amd`, or
__graft_entry__.build()).  There is no CPU fallback: if the shared object is
missing, loading raises, and every render/build call needs a HIP device.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPO_DIR = os.path.dirname(PKG_DIR)
LIB_PATH = os.environ.get("BIH_LIB") or os.path.join(PKG_DIR, "lib", "libbih_amd.so")
HEADER_PATH = os.path.join(REPO_DIR, "include", "bih.h")

BIH_OK = 0
ERRORS = {
    -1: "BIH_ERR_INVALID", -2: "BIH_ERR_NO_DEVICE", -3: "BIH_ERR_HIP", -4: "BIH_ERR_OOM",
    -5: "BIH_ERR_NONFINITE", -6: "BIH_ERR_TOO_LARGE", -7: "BIH_ERR_MISMATCH",
    -8: "BIH_ERR_IO", -9: "BIH_ERR_PARSE",
}
TRAVERSE_ANYHIT, TRAVERSE_REFERENCE = 0, 1
PARAM_ITEM_TILES, PARAM_PAIR_CAP, PARAM_BINS_CAP, PARAM_FORCE_FALLBACK, PARAM_WHITTED_COUNTERS = 1, 2, 3, 4, 5   # bih_tree_set_param
PARAM_STATIC_SOUP = 6
PARAM_TEST_ALLOC_FAIL = 7   # tests: the next allocating build fails at its k-th allocation
PARAM_TRACE_LDS_SLOTS = 8   # tests: 2 = ray queries keep only 2 stack slots per lane on chip
PARAM_GBUFFER_MASK = 9      # tests / A-B: 0 = G-buffer renders walk every sample (no bins hit mask)
QUERY_CLOSEST, QUERY_OCCLUDED = 0, 1   # bih_trace / bih_trace_device
QUERY_T_HI = 0x10                      # flag: the ray ends at its t_hi (segment queries)
QUERY_CLOSEST_WITHIN, QUERY_OCCLUDED_WITHIN = QUERY_CLOSEST | QUERY_T_HI, QUERY_OCCLUDED | QUERY_T_HI
NO_HIT = 0xFFFFFFFF
MAX_RAYS = 1 << 30
MAX_LIGHTS = 64           # bih_render_direct*: one bit each of a sample's lit word
LIGHT_DTYPE = np.dtype([("dir", np.float32, 3), ("weight", np.float32)])   # numpy view of a bih_light array
POINT_LIGHT_DTYPE = np.dtype([("pos", np.float32, 3), ("weight", np.float32)])   # ... of a bih_point_light array
SHADOW_T_LO = 1e-4        # BIH_SHADOW_T_LO
BOUNCE_SLOT = 0x80000000  # BIH_BOUNCE_SLOT: the hash slot of the bounce direction
MAX_BOUNCES = 8           # BIH_MAX_BOUNCES: levels of a path (bih_render_path*)
MAX_MATERIALS = 65536     # BIH_MAX_MATERIALS: records of a tree's palette (bih_tree_set_materials)
MAT_DIFFUSE = 0           # BIH_MAT_DIFFUSE: a Lambertian surface (the bits of reserved0 = +0.0)
MAT_MIRROR = 1            # BIH_MAT_MIRROR: a mirror tinted by albedo (bih_render_path_spec*)
# numpy view of a bih_material array; "kind" (uint32) overlaps "reserved0": one word, two names
MATERIAL_DTYPE = np.dtype({"names": ["albedo", "reserved0", "emission", "reserved1", "kind"],
                           "formats": [(np.float32, 3), np.float32, (np.float32, 3), np.float32, np.uint32],
                           "offsets": [0, 12, 16, 28, 12], "itemsize": 32})
DENOISE_MAX_PASSES = 8        # BIH_DENOISE_MAX_PASSES
DENOISE_MAX_SQUARINGS = 8     # BIH_DENOISE_MAX_SQUARINGS
DENOISE_MAX_PIXELS = 1 << 28  # BIH_DENOISE_MAX_PIXELS
MAX_AREA_LIGHTS = 16      # bih_render_area_lights*: area lights of one call
AREA_LIGHT_DTYPE = np.dtype([("corner", np.float32, 3), ("weight", np.float32),       # numpy view of a
                             ("edge_u", np.float32, 3), ("reserved0", np.float32),    # bih_area_light array
                             ("edge_v", np.float32, 3), ("reserved1", np.float32)])
(ARR_MORTON_SORTED, ARR_TRI_INDEX, ARR_UNIQUE_MC, ARR_DUP_COUNT, ARR_FIRST_IDX, ARR_LEAF_PARENT,
 ARR_CLIP, ARR_AXIS, ARR_CHILDREN, ARR_IS_LEAF, ARR_PARENT, ARR_TRI_LO, ARR_TRI_HI) = range(13)


class BihError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        self.code = code
        name = ERRORS.get(code, str(code))
        msg = strerror(code) if _lib is not None else name
        super().__init__(f"{what}: {name} ({msg})" if what else f"{name} ({msg})")


class Scene(C.Structure):
    _fields_ = [("n_tris", C.c_uint32), ("v", C.c_void_p)]


class Camera(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("lower_left", C.c_float * 3),
                ("horizontal", C.c_float * 3), ("vertical", C.c_float * 3)]

    def as_list(self):
        return list(self.origin) + list(self.lower_left) + list(self.horizontal) + list(self.vertical)

    @classmethod
    def from_list(cls, v):
        c = cls()
        v = [float(x) for x in v]
        for i in range(3):
            c.origin[i], c.lower_left[i] = v[i], v[3 + i]
            c.horizontal[i], c.vertical[i] = v[6 + i], v[9 + i]
        return c


class Framebuffer(C.Structure):
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("spp", C.c_uint32), ("frame", C.c_uint32),
                ("seed", C.c_uint64), ("rgba", C.c_void_p)]


class Rows(C.Structure):
    _fields_ = [("row0", C.c_uint32), ("nrows", C.c_uint32), ("band_h", C.c_uint32),
                ("band_step", C.c_uint32)]


class _RayEnd(C.Union):
    _fields_ = [("reserved", C.c_float), ("t_hi", C.c_float)]


class Ray(C.Structure):
    """bih_ray (32 bytes); the last float is `reserved` or `t_hi` (one member)."""
    _anonymous_ = ("_end",)
    _fields_ = [("o", C.c_float * 3), ("t_lo", C.c_float), ("d", C.c_float * 3), ("_end", _RayEnd)]


class Hit(C.Structure):
    """bih_hit (16 bytes)."""
    _fields_ = [("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("prim", C.c_uint32)]


class GBuffer(C.Structure):
    """bih_gbuffer: six plane pointers, any of them NULL (not written)."""
    _fields_ = [("hits", C.c_void_p), ("depth", C.c_void_p), ("prim", C.c_void_p), ("bary", C.c_void_p),
                ("normal", C.c_void_p), ("coverage", C.c_void_p)]


class Light(C.Structure):
    """bih_light (16 bytes): a directional light, dir towards the light."""
    _fields_ = [("dir", C.c_float * 3), ("weight", C.c_float)]


class PointLight(C.Structure):
    """bih_point_light (16 bytes): a lamp at pos."""
    _fields_ = [("pos", C.c_float * 3), ("weight", C.c_float)]


class AreaLight(C.Structure):
    """bih_area_light (48 bytes): a parallelogram corner + a*edge_u + b*edge_v that
    emits to the side cross(edge_u, edge_v) points to; weight = its radiance."""
    _fields_ = [("corner", C.c_float * 3), ("weight", C.c_float), ("edge_u", C.c_float * 3),
                ("reserved0", C.c_float), ("edge_v", C.c_float * 3), ("reserved1", C.c_float)]


class LightSet(C.Structure):
    """bih_light_set: the three light arrays of bih_render_area_lights* (host memory)."""
    _fields_ = [("dir", C.c_void_p), ("n_dir", C.c_uint32), ("point", C.c_void_p), ("n_point", C.c_uint32),
                ("area", C.c_void_p), ("n_area", C.c_uint32)]


class Direct(C.Structure):
    """bih_direct: three plane pointers, any of them NULL (not written)."""
    _fields_ = [("lit", C.c_void_p), ("irradiance", C.c_void_p), ("rgba", C.c_void_p)]


class Bounce(C.Structure):
    """bih_bounce (8 bytes): the bounced light's diffuse reflectance and the
    irradiance an escaped bounce ray collects."""
    _fields_ = [("albedo", C.c_float), ("sky", C.c_float)]


class Indirect(C.Structure):
    """bih_indirect: five plane pointers, any of them NULL (not written)."""
    _fields_ = [("lit", C.c_void_p), ("bounce", C.c_void_p), ("lit2", C.c_void_p), ("irradiance", C.c_void_p),
                ("rgba", C.c_void_p)]


class Path(C.Structure):
    """bih_path: five plane pointers, any of them NULL (not written); bounces and
    lits hold one plane per level."""
    _fields_ = [("lit", C.c_void_p), ("bounces", C.c_void_p), ("lits", C.c_void_p), ("irradiance", C.c_void_p),
                ("rgba", C.c_void_p)]


class _MaterialWord(C.Union):
    _fields_ = [("reserved0", C.c_float), ("kind", C.c_uint32)]


class Material(C.Structure):
    """bih_material: diffuse reflectance and emitted radiance, R G B, and the
    kind (MAT_*; one word with reserved0) (32 bytes)."""
    _anonymous_ = ("word",)
    _fields_ = [("albedo", C.c_float * 3), ("word", _MaterialWord), ("emission", C.c_float * 3),
                ("reserved1", C.c_float)]


class PathRgb(C.Structure):
    """bih_path_rgb: bih_path's planes with radiance (three floats per pixel) in
    the place of irradiance."""
    _fields_ = [("lit", C.c_void_p), ("bounces", C.c_void_p), ("lits", C.c_void_p), ("radiance", C.c_void_p),
                ("rgba", C.c_void_p)]


class DenoiseParams(C.Structure):
    """bih_denoise_params (16 bytes): passes 1..8 (pass i uses step 1 << i),
    normal_squarings 0..8, sigma_colour (pass 0's colour support; halves every
    pass), sigma_plane (scene units: distance from the centre's tangent plane)."""
    _fields_ = [("passes", C.c_uint32), ("normal_squarings", C.c_uint32), ("sigma_colour", C.c_float),
                ("sigma_plane", C.c_float)]


DENOISE_PARAMS = DenoiseParams          # the ctypes mirror of bih_denoise_params
DENOISE_DEFAULTS = (3, 5, 2.0, 0.05)    # passes, normal_squarings, sigma_colour, sigma_plane


class BinsStats(C.Structure):
    _fields_ = [("usable", C.c_uint32), ("tiles_x", C.c_uint32), ("tiles_y", C.c_uint32),
                ("list_entries", C.c_uint64), ("global_entries", C.c_uint32)]


class TreeInfo(C.Structure):
    _fields_ = [("n_tris", C.c_uint32), ("n_unique", C.c_uint32), ("scene_lo", C.c_float * 3),
                ("scene_hi", C.c_float * 3), ("device", C.c_int), ("device_bytes", C.c_uint64),
                ("build_ms", C.c_double), ("device_allocs", C.c_uint64)]


_lib = None


def exported_symbols_from_header(path: str = HEADER_PATH):
    """Function names declared in include/bih.h."""
    src = open(path).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w[\w\s\*]*?\b(bih_\w+)\s*\(", src, re.M)))


def load():
    """Loads the in-tree shared object (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError(f"{LIB_PATH} not built: run `make -C bih-gpu-raytracer_amd` "
                      "(or __graft_entry__.build())")
    # One HIP runtime per process: the torch wheel bundles its own
    # libamdhip64 (soname libamdhip64.so.7, NEEDED as "libamdhip64.so"), so
    # if torch is present it is loaded first and libbih_amd.so binds to that
    # same runtime instead of pulling in a second copy from /opt/rocm.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    L.bih_abi_version.restype = i32
    L.bih_device_count.restype = i32
    L.bih_strerror.argtypes = [i32]
    L.bih_strerror.restype = C.c_char_p
    L.bih_camera_reference.argtypes = [u32, u32, C.POINTER(Camera)]
    L.bih_camera_ray_bound.argtypes = [C.POINTER(Camera), C.POINTER(C.c_float)]
    L.bih_pixel_divide.argtypes = [u32, vp, C.c_size_t, vp, C.POINTER(u32)]
    L.bih_scene_load_obj.argtypes = [C.c_char_p, C.POINTER(Scene), C.POINTER(u32)]
    L.bih_scene_free.argtypes = [C.POINTER(Scene)]
    L.bih_scene_free.restype = None
    L.bih_build.argtypes = [C.POINTER(Scene), i32, C.POINTER(vp)]
    L.bih_build_device.argtypes = [vp, u32, i32, vp, C.POINTER(vp)]
    L.bih_rebuild.argtypes = [vp]
    L.bih_free.argtypes = [vp]
    L.bih_free.restype = None
    L.bih_tree_get_info.argtypes = [vp, C.POINTER(TreeInfo)]
    L.bih_tree_export.argtypes = [vp, i32, vp, C.POINTER(C.c_size_t)]
    L.bih_render.argtypes = [C.POINTER(Scene), vp, C.POINTER(Camera), C.POINTER(Framebuffer)]
    L.bih_render_rows.argtypes = [C.POINTER(Scene), vp, C.POINTER(Camera), C.POINTER(Framebuffer),
                                  u32, u32]
    L.bih_render_device.argtypes = [vp, C.POINTER(Camera), u32, u32, u32, u32, u64,
                                    C.POINTER(Rows), u32, vp, vp, vp]
    L.bih_sync.argtypes = [vp, vp]
    L.bih_render_device_frames.argtypes = [vp, C.POINTER(Camera), u32, u32, u32, u32, u32, u64,
                                           C.POINTER(Rows), vp, u64, vp]
    L.bih_render_whitted_device.argtypes = [vp, C.POINTER(Camera), u32, u32, u32, u32, u64,
                                            C.POINTER(Rows), vp, vp, vp]
    L.bih_render_whitted.argtypes = [C.POINTER(Scene), vp, C.POINTER(Camera), C.POINTER(Framebuffer)]
    L.bih_last_render_ms.argtypes = [vp, C.POINTER(C.c_double)]
    L.bih_set_timing.argtypes = [vp, i32]
    L.bih_last_render_times.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.bih_bins_get_stats.argtypes = [vp, C.POINTER(BinsStats)]
    L.bih_bins_solid_masks.argtypes = [vp, C.POINTER(C.c_uint16), C.c_size_t, C.POINTER(u32)]
    L.bih_reserve.argtypes = [vp, u32, u32, u32, C.POINTER(Rows), u32]
    L.bih_tree_set_param.argtypes = [vp, i32, u64]
    L.bih_whitted_work.argtypes = [vp, C.POINTER(u32), C.POINTER(u64), C.POINTER(u64)]
    L.bih_host_register.argtypes = [vp, C.c_size_t]
    L.bih_host_unregister.argtypes = [vp]
    L.bih_render_history.argtypes = [vp, u32, C.POINTER(C.c_double)]
    L.bih_trace_device.argtypes = [vp, vp, u64, u32, vp, vp]
    L.bih_trace.argtypes = [vp, vp, u64, u32, vp]
    L.bih_render_gbuffer_device.argtypes = [vp, C.POINTER(Camera), u32, u32, u32, u32, u64, C.POINTER(Rows),
                                            C.POINTER(GBuffer), vp]
    L.bih_render_gbuffer.argtypes = [vp, C.POINTER(Camera), u32, u32, u32, u32, u64, C.POINTER(Rows),
                                     C.POINTER(GBuffer)]
    L.bih_render_direct_device.argtypes = [vp, C.POINTER(Camera), u32, u32, u32, u32, u64, C.POINTER(Rows),
                                           vp, u32, C.POINTER(Direct), vp]
    L.bih_render_direct.argtypes = [vp, C.POINTER(Camera), u32, u32, u32, u32, u64, C.POINTER(Rows),
                                    vp, u32, C.POINTER(Direct)]
    L.bih_render_lights_device.argtypes = [vp, C.POINTER(Camera), u32, u32, u32, u32, u64, C.POINTER(Rows),
                                           vp, u32, vp, u32, C.POINTER(Direct), vp]
    L.bih_render_lights.argtypes = [vp, C.POINTER(Camera), u32, u32, u32, u32, u64, C.POINTER(Rows),
                                    vp, u32, vp, u32, C.POINTER(Direct)]
    L.bih_render_area_lights_device.argtypes = [vp, C.POINTER(Camera), u32, u32, u32, u32, u64, C.POINTER(Rows),
                                                C.POINTER(LightSet), C.POINTER(Direct), vp]
    L.bih_render_area_lights.argtypes = [vp, C.POINTER(Camera), u32, u32, u32, u32, u64, C.POINTER(Rows),
                                         C.POINTER(LightSet), C.POINTER(Direct)]
    L.bih_area_light_sample.argtypes = [vp, u32, u64, u32, u32, u32, u32, C.POINTER(C.c_float)]
    L.bih_render_indirect_device.argtypes = [vp, C.POINTER(Camera), u32, u32, u32, u32, u64, C.POINTER(Rows),
                                             C.POINTER(LightSet), C.POINTER(Bounce), C.POINTER(Indirect), vp]
    L.bih_render_indirect.argtypes = [vp, C.POINTER(Camera), u32, u32, u32, u32, u64, C.POINTER(Rows),
                                      C.POINTER(LightSet), C.POINTER(Bounce), C.POINTER(Indirect)]
    L.bih_bounce_sample.argtypes = [u64, u32, u32, u32, u32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.bih_render_path_device.argtypes = [vp, C.POINTER(Camera), u32, u32, u32, u32, u64, C.POINTER(Rows),
                                         C.POINTER(LightSet), C.POINTER(Bounce), u32, C.POINTER(Path), vp]
    L.bih_render_path.argtypes = [vp, C.POINTER(Camera), u32, u32, u32, u32, u64, C.POINTER(Rows),
                                  C.POINTER(LightSet), C.POINTER(Bounce), u32, C.POINTER(Path)]
    L.bih_path_sample.argtypes = [u64, u32, u32, u32, u32, u32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.bih_tree_set_materials.argtypes = [vp, vp, u32, vp]
    L.bih_render_path_rgb_device.argtypes = [vp, C.POINTER(Camera), u32, u32, u32, u32, u64, C.POINTER(Rows),
                                             C.POINTER(LightSet), C.POINTER(C.c_float), u32, C.POINTER(PathRgb), vp]
    L.bih_render_path_rgb.argtypes = [vp, C.POINTER(Camera), u32, u32, u32, u32, u64, C.POINTER(Rows),
                                      C.POINTER(LightSet), C.POINTER(C.c_float), u32, C.POINTER(PathRgb)]
    L.bih_render_path_spec_device.argtypes = L.bih_render_path_rgb_device.argtypes
    L.bih_render_path_spec.argtypes = L.bih_render_path_rgb.argtypes
    L.bih_denoise_device.argtypes = [vp, C.POINTER(Camera), u32, u32, C.POINTER(DenoiseParams), vp, vp, vp, vp, vp, vp]
    L.bih_denoise.argtypes = [vp, C.POINTER(Camera), u32, u32, C.POINTER(DenoiseParams), vp, vp, vp, vp, vp]
    for name in ("bih_camera_reference", "bih_camera_ray_bound", "bih_pixel_divide", "bih_scene_load_obj", "bih_build", "bih_build_device", "bih_rebuild",
                 "bih_tree_get_info", "bih_tree_export", "bih_render", "bih_render_rows",
                 "bih_render_device", "bih_sync", "bih_last_render_ms", "bih_last_render_times", "bih_set_timing",
                 "bih_render_whitted_device", "bih_render_whitted", "bih_render_device_frames",
                 "bih_bins_get_stats", "bih_bins_solid_masks", "bih_reserve", "bih_tree_set_param", "bih_whitted_work",
                 "bih_host_register", "bih_host_unregister", "bih_render_history", "bih_trace_device", "bih_trace",
                 "bih_render_gbuffer_device", "bih_render_gbuffer", "bih_render_direct_device", "bih_render_direct",
                 "bih_render_lights_device", "bih_render_lights", "bih_render_area_lights_device",
                 "bih_render_area_lights", "bih_area_light_sample", "bih_render_indirect_device",
                 "bih_render_indirect", "bih_bounce_sample", "bih_render_path_device", "bih_render_path",
                 "bih_path_sample", "bih_tree_set_materials", "bih_render_path_rgb_device", "bih_render_path_rgb",
                 "bih_render_path_spec_device", "bih_render_path_spec", "bih_denoise_device", "bih_denoise"):
        getattr(L, name).restype = i32
    _lib = L
    return L


def strerror(code: int) -> str:
    return load().bih_strerror(code).decode()


def check(rc: int, what: str = ""):
    if rc != BIH_OK:
        raise BihError(rc, what)
    return rc
