"""The camera catalogue of tests/test_cameras.py: cameras inside, across and
far from the scene, one per camera-dependent branch of the frustum bins
(k_bin_fp, bin_camera, build_bins: DESIGN.md, "Camera classes under test").

A plain helper module: no test lives here.  Cameras are float32 arrays of 12
(origin, lower_left, horizontal, vertical), built in f64 and cast once.
"""
import functools

import numpy as np

F32 = np.float32
W, H = 96, 64                     # the catalogue's image unless a test says otherwise
BACKGROUND = 0x281414             # a pixel whose samples all miss (20, 20, 40)
GLOBAL_MAX = 4096                 # kBinGlobalMax (bih_internal.h)


def look(o, f, w, h, hh=0.5, up=(0, 1, 0), plane=1.0):
    """A pinhole camera at o looking along f: half height hh of the image
    plane at distance `plane`, half width hh * w / h."""
    o, f, up = (np.asarray(x, np.float64) for x in (o, f, up))
    f = f / np.linalg.norm(f)
    rt = np.cross(up, f)
    rt /= np.linalg.norm(rt)
    u = np.cross(f, rt)
    hw = hh * w / h
    return np.concatenate([o, o + plane * f - rt * hw - u * hh, 2 * hw * rt, 2 * hh * u]).astype(F32)


def basis(f, up=(0, 1, 0)):
    """(f, rt, u) of look(), f64."""
    f, up = np.asarray(f, np.float64), np.asarray(up, np.float64)
    f = f / np.linalg.norm(f)
    rt = np.cross(up, f)
    rt /= np.linalg.norm(rt)
    return f, rt, np.cross(f, rt)


DIAG_O, DIAG_F = (1.3, .1, 1), (-.5, .3, -.8)


def _mirrored(c):
    c = c.copy()
    c[3:6] += c[6:9]
    c[6:9] = -c[6:9]
    return c


def _sheared(c):
    c = c.copy()
    c[6:9] += F32(0.3) * c[9:12]
    c[3:6] += F32(0.2) * c[9:12] - F32(0.15) * c[6:9]
    return c


def _zero_horizontal(c):
    c = c.copy()
    c[6:9] = 0
    return c


# name -> (scene, camera(w, h)); scene "A" = soup(20000, seed=3), "C" = cornell()
CATALOGUE = {
    "inside_z": ("A", lambda w, h: look((1.3, 0, 1), (0, 0, 1), w, h)),
    "inside_diag": ("A", lambda w, h: look(DIAG_O, DIAG_F, w, h)),
    "mirrored": ("A", lambda w, h: _mirrored(look(DIAG_O, DIAG_F, w, h))),
    "sheared": ("A", lambda w, h: _sheared(look(DIAG_O, DIAG_F, w, h))),
    "wide174": ("A", lambda w, h: look(DIAG_O, DIAG_F, w, h, hh=20)),
    "wide_nobins": ("A", lambda w, h: look(DIAG_O, DIAG_F, w, h, hh=2000)),
    "plane_through_origin": ("A", lambda w, h: look(DIAG_O, DIAG_F, w, h, plane=0.0)),
    "zero_horizontal": ("A", lambda w, h: _zero_horizontal(look(DIAG_O, DIAG_F, w, h))),
    "away": ("A", lambda w, h: look((1.3, 0, -.5), (0, 0, -1), w, h)),
    "tele": ("A", lambda w, h: look((1.3, 0, -2000), (0, 0, 1), w, h, hh=3e-4)),
    "tele_off": ("A", lambda w, h: look((801.3, 500, -2000), (-800, -500, 2001), w, h, hh=3e-4)),
    "at_edge": ("A", lambda w, h: look((0, 0, 1), (1, .1, .05), w, h)),
    "cornell_back": ("C", lambda w, h: look((.4, 0, 1.2), (-.5, .2, -1), w, h)),
    "cornell_in": ("C", lambda w, h: look((.4, 0, .3), (.2, -.1, 1), w, h, hh=.7)),
}
SCENE_A = [k for k, v in CATALOGUE.items() if v[0] == "A"]
DEGENERATE = ("wide_nobins", "plane_through_origin", "zero_horizontal")   # bin_camera returns false
STRADDLING = ("inside_z", "inside_diag", "mirrored", "sheared")            # origin deep inside scene A


def camera(name, w=W, h=H):
    """The catalogue camera `name` for a w x h image (a fresh float32[12])."""
    return CATALOGUE[name][1](w, h)


def scene_of(name):
    return CATALOGUE[name][0]


@functools.lru_cache(maxsize=None)
def scene(name):
    """Scene "A", "B" (A plus the band on inside_diag's eye plane) or "C": float32 (n, 9), read-only."""
    from bihrt import scenes
    if name == "A":
        t = scenes.soup(20000, seed=3)
    elif name == "B":
        t = np.concatenate([scene("A"), band()])
    else:
        t = scenes.cornell()
    t = np.ascontiguousarray(t, F32).reshape(-1, 9)
    t.setflags(write=False)
    return t


def band(n=24000):
    """n tiny triangles whose centroids lie on the eye plane of inside_diag,
    0.3 .. 0.9 from the origin: at depth 0, outside every finite field of view,
    and with vertices on both sides of the plane."""
    rng = np.random.default_rng(5)
    _, rt, u = basis(DIAG_F)
    r = rng.uniform(0.3, 0.9, n)
    a = rng.uniform(0, 2 * np.pi, n)
    c = np.asarray(DIAG_O, np.float64) + r[:, None] * (np.cos(a)[:, None] * rt + np.sin(a)[:, None] * u)
    v = c[:, None, :] + rng.uniform(-0.01, 0.01, (n, 3, 3))
    return v.reshape(n, 9).astype(F32)


def plane_terms(cam):
    """(A, n, A.n) in f64 as bin_camera forms them, before its flip of n."""
    c = np.asarray(cam, F32).astype(np.float64)
    A = c[3:6] - c[0:3]
    n = np.cross(c[6:9], c[9:12])
    return A, n, float(A @ n)


def classify(tris, cam):
    """(alive, alive and straddling, alive and behind) of raw f64 vertices:
    alive = front-facing to the origin (e2 . ((O - v0) x e1) > 0, the sign
    RayTriangleIntersection's culling takes for every ray from O); straddling =
    vertex depths (v - O) . n not all of one sign; n = h x v, flipped to A . n >= 0."""
    t = np.asarray(tris, F32).astype(np.float64).reshape(-1, 3, 3)
    O = np.asarray(cam, F32).astype(np.float64)[0:3]
    _, n, an = plane_terms(cam)
    if an < 0:
        n = -n
    e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    alive = np.einsum("ij,ij->i", e2, np.cross(O - t[:, 0], e1)) > 0
    depth = (t - O) @ n
    front, behind = (depth > 0).all(1), (depth < 0).all(1)
    return int(alive.sum()), int((alive & ~front & ~behind).sum()), int((alive & behind).sum())


def hit_share(img):
    """Share of the pixels with at least one hit sample."""
    return float((np.asarray(img) != BACKGROUND).mean())
