"""Deterministic synthetic scenes for the BASELINE.json configs.

Scenes are flat triangle soups: float32 arrays of shape (n, 9) holding
v0, v1, v2 per triangle in "file order" -- the layout App::LoadModels builds
(reference src/App.cpp:108-121).  Every generator is counter-based
(splitmix64), so this container and the GPU box produce identical bytes.

C1 cornell():   32-tri Cornell box (5 walls, 2 blocks x 5 faces, light).
C2 torus():     ~70k-tri closed torus (procedural stand-in: the Stanford
                Bunny is not available offline).
C3 soup():      1M random-triangle soup, centroids U([0,2.667]x[-1,1]x[0,2]),
                vertices = centroid + U(-0.02,0.02)^3, seed 1.
"""
from __future__ import annotations

import numpy as np

from ._lib import AREA_LIGHT_DTYPE, LIGHT_DTYPE, POINT_LIGHT_DTYPE

_GOLD = np.uint64(0x9E3779B97F4A7C15)


def splitmix64(seed: int, start: int, count: int) -> np.ndarray:
    """Outputs start..start+count-1 of splitmix64 seeded with `seed`."""
    k = np.arange(start + 1, start + count + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + k * _GOLD
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def uniform01(seed: int, start: int, count: int) -> np.ndarray:
    """24-bit uniforms in [0,1), exact in float32 and float64."""
    return (splitmix64(seed, start, count) >> np.uint64(40)).astype(np.float64) * (2.0 ** -24)


def soup(n: int = 1_000_000, seed: int = 1, lo=(0.0, -1.0, 0.0), size=(2.6666667, 2.0, 2.0),
         half: float = 0.02) -> np.ndarray:
    """Random triangle soup (config C3/C5).  12 uniforms per triangle:
    3 for the centroid, then 9 for the vertex offsets (v0.xyz, v1.xyz, v2.xyz)."""
    u = uniform01(seed, 0, 12 * n).reshape(n, 12)
    c = np.asarray(lo, np.float64) + u[:, 0:3] * np.asarray(size, np.float64)
    off = (u[:, 3:12] * (2.0 * half) - half).reshape(n, 3, 3)
    v = c[:, None, :] + off
    return np.ascontiguousarray(v.reshape(n, 9).astype(np.float32))


def _quad(a, b, c, d):
    """Two CCW triangles (a,b,c), (a,c,d) of the quad a-b-c-d."""
    return [a + b + c, a + c + d]


def cornell() -> np.ndarray:
    """32 triangles: 5 walls x2, 2 blocks x 5 faces x2, ceiling light x2.
    Front faces (CCW seen from inside) point into the box, towards the
    reference camera at (2,0,-2) looking down +z (MT culls back faces)."""
    x0, x1, y0, y1, z0, z1 = -1.0, 1.9, -1.0, 1.0, 0.0, 2.4
    P = lambda x, y, z: [x, y, z]  # noqa: E731
    tris = []
    # back wall z=z1, normal -z (faces the camera)
    tris += _quad(P(x0, y0, z1), P(x0, y1, z1), P(x1, y1, z1), P(x1, y0, z1))
    # floor y=y0, normal +y
    tris += _quad(P(x0, y0, z0), P(x0, y0, z1), P(x1, y0, z1), P(x1, y0, z0))
    # ceiling y=y1, normal -y
    tris += _quad(P(x0, y1, z0), P(x1, y1, z0), P(x1, y1, z1), P(x0, y1, z1))
    # left wall x=x0, normal +x
    tris += _quad(P(x0, y0, z0), P(x0, y1, z0), P(x0, y1, z1), P(x0, y0, z1))
    # right wall x=x1, normal -x
    tris += _quad(P(x1, y0, z0), P(x1, y0, z1), P(x1, y1, z1), P(x1, y1, z0))

    def block(cx, cz, hw, hgt, rot):
        cs, sn = np.cos(rot), np.sin(rot)

        def p(dx, y, dz):
            return [cx + cs * dx - sn * dz, y, cz + sn * dx + cs * dz]
        a, b, c, d = (-hw, -hw), (hw, -hw), (hw, hw), (-hw, hw)
        yb, yt = y0, y0 + hgt
        out = []
        # top, normal +y
        out += _quad(p(a[0], yt, a[1]), p(d[0], yt, d[1]), p(c[0], yt, c[1]), p(b[0], yt, b[1]))
        # four sides, outward normals
        for (u0, u1) in ((a, b), (b, c), (c, d), (d, a)):
            out += _quad(p(u0[0], yb, u0[1]), p(u1[0], yb, u1[1]), p(u1[0], yt, u1[1]), p(u0[0], yt, u0[1]))
        return out
    tris += block(-0.2, 1.6, 0.35, 1.2, 0.3)
    tris += block(0.9, 0.9, 0.3, 0.6, -0.3)
    # light, just below the ceiling, normal -y
    ly = y1 - 0.01
    tris += _quad(P(0.1, ly, 1.0), P(0.7, ly, 1.0), P(0.7, ly, 1.6), P(0.1, ly, 1.6))
    v = np.asarray(tris, np.float64).astype(np.float32)
    assert v.shape == (32, 9), v.shape
    return np.ascontiguousarray(v)


def torus(nu: int = 263, nv: int = 132, R: float = 1.0, r: float = 0.35,
          center=(0.3, 0.0, 1.5), tilt: float = 0.6) -> np.ndarray:
    """Closed torus, 2*nu*nv triangles (69,432 at the defaults), outward CCW."""
    iu, iv = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    th = 2 * np.pi * np.arange(nu + 1) / nu
    ph = 2 * np.pi * np.arange(nv + 1) / nv
    T, Pm = np.meshgrid(th, ph, indexing="ij")
    X = (R + r * np.cos(Pm)) * np.cos(T)
    Y = (R + r * np.cos(Pm)) * np.sin(T)
    Z = r * np.sin(Pm)
    ct, st = np.cos(tilt), np.sin(tilt)
    Y, Z = ct * Y - st * Z, st * Y + ct * Z
    pts = np.stack([X + center[0], Y + center[1], Z + center[2]], -1)
    a = pts[iu, iv]
    b = pts[iu + 1, iv]
    c = pts[iu + 1, iv + 1]
    d = pts[iu, iv + 1]
    t1 = np.concatenate([a, b, c], -1)
    t2 = np.concatenate([a, c, d], -1)
    v = np.stack([t1, t2], 2).reshape(-1, 9)
    return np.ascontiguousarray(v.astype(np.float32))


def dodecahedron(start=None, variant: int = 0) -> np.ndarray:
    """Regular dodecahedron, circumradius 1, 12 pentagons fan-triangulated
    (assimp aiProcess_Triangulate, reference src/Model.cpp:13) -> 36 tris.
    `start[f]` picks the fan apex of face f (0..4); variant selects one of the
    two standard axis orientations."""
    phi = (1 + 5 ** 0.5) / 2
    s = 1 / 3 ** 0.5
    V = []
    for x in (-1, 1):
        for y in (-1, 1):
            for z in (-1, 1):
                V.append((x, y, z))
    a, b = 1 / phi, phi
    if variant == 1:
        a, b = b, a
    for i in (-1, 1):
        for j in (-1, 1):
            V.append((0, i * a, j * b))
            V.append((i * a, j * b, 0))
            V.append((i * b, 0, j * a))
    V = np.asarray(V, np.float64) * s
    faces = _dodeca_faces(V)
    if start is None:
        start = [0] * 12
    tris = []
    for f, st in zip(faces, start):
        f = list(f[st:]) + list(f[:st])
        for k in range(1, 4):
            tris.append(np.concatenate([V[f[0]], V[f[k]], V[f[k + 1]]]))
    return np.ascontiguousarray(np.asarray(tris).astype(np.float32)), faces, V


# Fan apex per face (variant 1) of the one triangulation, out of 5^12 per
# orientation and vertex precision, whose BIH reproduces the reference's own
# tree dump node for node (BIH1.txt:1-348; search: tests/golden/
# make_bih1_soup.py, record: tests/golden/bih1_dodecahedron.json).
BIH1_APEX = (1, 4, 4, 0, 3, 3, 3, 1, 3, 0, 4, 1)


def dodecahedron_bih1() -> np.ndarray:
    """The reference's 36-triangle dodecahedron (the mesh behind BIH1.txt),
    recovered by exhaustive search; 36 x 9 float32."""
    return dodecahedron(start=BIH1_APEX, variant=1)[0]


def _dodeca_faces(V):
    """12 pentagonal faces as CCW (outward) vertex cycles."""
    d = np.linalg.norm(V[:, None] - V[None], axis=-1)
    edge = np.min(d[d > 1e-9])
    adj = np.abs(d - edge) < 1e-6
    seen, out = set(), []
    for i in range(len(V)):
        nb = np.nonzero(adj[i])[0]
        for a_ in range(len(nb)):
            for b_ in range(a_ + 1, len(nb)):
                j, k = nb[a_], nb[b_]
                nrm = np.cross(V[j] - V[i], V[k] - V[i])
                nrm /= np.linalg.norm(nrm)
                if np.dot(nrm, V[i]) < 0:
                    nrm = -nrm
                on = np.nonzero(np.abs((V - V[i]) @ nrm) < 1e-6)[0]
                key = frozenset(int(x) for x in on)
                if len(on) != 5 or key in seen:
                    continue
                seen.add(key)
                cen = V[on].mean(0)
                e0 = V[on[0]] - cen
                e0 /= np.linalg.norm(e0)
                e1 = np.cross(nrm, e0)
                ang = np.arctan2((V[on] - cen) @ e1, (V[on] - cen) @ e0)
                out.append([int(x) for x in on[np.argsort(ang)]])
    assert len(out) == 12, len(out)
    return out


def write_obj(path: str, tris: np.ndarray, shared: bool = False):
    """Writes a soup as Wavefront OBJ (numpy's shortest round-trip float32
    repr per coordinate).  shared=False: three `v` lines + one `f` per triangle;
    shared=True: identical vertices are written once and referenced by index."""
    tris = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    with open(path, "w") as f:
        f.write(f"# {tris.shape[0]} triangles\no soup\n")
        if not shared:
            for t in tris:
                for p in t:
                    f.write("v %s %s %s\n" % tuple(str(x) for x in p))
            for i in range(tris.shape[0]):
                f.write("f %d %d %d\n" % (3 * i + 1, 3 * i + 2, 3 * i + 3))
            return
        verts, idx = np.unique(tris.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
        for p in verts.view(np.float32):
            f.write("v %s %s %s\n" % tuple(str(x) for x in p))
        for t in idx.reshape(-1, 3):
            f.write("f %d %d %d\n" % tuple(int(k) + 1 for k in t))


def sky_dome(k: int, sun=None) -> np.ndarray:
    """Directional lights of a uniform sky for Renderer.render_direct: k
    Fibonacci directions on the upper (+y) hemisphere, (k,) float32 records
    {dir[3], weight} (bihrt.LIGHT_DTYPE), unit length.  The weights make a
    horizontal unoccluded surface (normal +y) sum to 1: weight = 1 / sum(dir.y).
    sun: an optional (x, y, z) direction towards the sun, normalised and
    prepended with weight 1 (k + 1 lights)."""
    if k < 1:
        raise ValueError("sky_dome needs at least one direction")
    i = np.arange(k, dtype=np.float64) + 0.5
    y = i / k                                     # uniform in height: uniform on the hemisphere
    r = np.sqrt(np.maximum(0.0, 1.0 - y * y))
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    out = np.zeros((k, 4), np.float64)
    out[:, 0], out[:, 1], out[:, 2] = r * np.cos(phi), y, r * np.sin(phi)
    out[:, 3] = 1.0 / y.sum()
    if sun is not None:
        s = np.asarray(sun, np.float64).reshape(3)
        n = np.linalg.norm(s)
        if not n > 0:
            raise ValueError("sun direction must be non-zero")
        out = np.concatenate([[[*(s / n), 1.0]], out])
    return np.ascontiguousarray(out, np.float32).view(LIGHT_DTYPE).reshape(-1)


def lamps(lo, hi, k: int, scale: float = 0.6, weight=None) -> np.ndarray:
    """Point lights for Renderer.render_lights: k lamps on an ellipsoid inside
    (scale < 1) or around the box [lo, hi] -- centre + scale * half_extent * u_i,
    u_i = k Fibonacci points over the whole unit sphere -- as (k,) float32
    records {pos[3], weight} (bihrt.POINT_LIGHT_DTYPE); computed in f64.
    weight: of each lamp; default |half_extent|^2 / k, which makes a surface
    that faces the lamps from about a half-diagonal away sum to the order of 1."""
    if k < 1:
        raise ValueError("lamps needs at least one lamp")
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    centre, half = (lo + hi) / 2.0, (hi - lo) / 2.0
    i = np.arange(k, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / k
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    r = np.sqrt(1.0 - z * z)
    u = np.stack([r * np.cos(phi), z, r * np.sin(phi)], 1)
    out = np.zeros((k, 4), np.float64)
    out[:, :3] = centre + scale * half * u
    out[:, 3] = float(half @ half) / k if weight is None else float(weight)
    return np.ascontiguousarray(out, np.float32).view(POINT_LIGHT_DTYPE).reshape(-1)


def _panel_rows(rows) -> np.ndarray:
    out = np.zeros(len(rows), AREA_LIGHT_DTYPE)
    for k, (corner, u, v, w) in enumerate(rows):
        out[k]["corner"], out[k]["edge_u"], out[k]["edge_v"] = corner, u, v
        out[k]["weight"] = w
    return out


def panels(lo, hi, weight=None) -> np.ndarray:
    """Area lights for Renderer.render_area_lights: two horizontal panels
    inside the box [lo, hi] of centre c and half extent h, as (2,) float32
    records (bihrt.AREA_LIGHT_DTYPE); computed in f64, then rounded.  The first
    {c - (0.3hx, -0.2hy, 0.3hz), U = (0.6hx, 0, 0), V = (0, 0, 0.6hz)} lies above
    the centre and faces down (cross(U, V) points to -y); the second
    {c - (0.3hx, 0.2hy, 0.3hz), U = (0, 0, 0.6hz), V = (0.6hx, 0, 0)} lies below
    it and faces up.  weight: each panel's radiance; default |h|^2 / area, which
    makes a surface that faces a panel from about a half-diagonal away get the
    order of 1."""
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    c, h = (lo + hi) / 2.0, (hi - lo) / 2.0
    area = 0.36 * h[0] * h[2]
    w = (float(h @ h) / area if area > 0 else 0.0) if weight is None else float(weight)
    eu, ev = np.array([0.6 * h[0], 0.0, 0.0]), np.array([0.0, 0.0, 0.6 * h[2]])
    return _panel_rows([(c - np.array([0.3 * h[0], -0.2 * h[1], 0.3 * h[2]]), eu, ev, w),
                        (c - np.array([0.3 * h[0], 0.2 * h[1], 0.3 * h[2]]), ev, eu, w)])


def cornell_panel(weight: float = 1.0) -> np.ndarray:
    """cornell()'s ceiling lamp as an area light: the lamp quad's outline one
    centimetre below it (geometry coincident with a panel may or may not shadow
    it), facing down; (1,) bihrt.AREA_LIGHT_DTYPE."""
    return _panel_rows([((0.1, 0.98, 1.0), (0.6, 0.0, 0.0), (0.0, 0.0, 0.6), weight)])


def cornell_materials():
    """cornell()'s colours for GPUArrayManager.set_materials: a palette
    (4,) bihrt.MATERIAL_DTYPE -- 0 white (floor, ceiling, back wall, blocks),
    1 red (left wall), 2 green (right wall), 3 the lamp quad (triangles 30 and
    31), which emits (17, 12, 4) -- and the (32,) uint32 material of each
    triangle in file order."""
    from . import pack_materials
    pal = pack_materials([(0.73, 0.73, 0.73, 0, 0, 0), (0.65, 0.05, 0.05, 0, 0, 0), (0.12, 0.45, 0.15, 0, 0, 0),
                          (0.78, 0.78, 0.78, 17.0, 12.0, 4.0)])
    ids = np.zeros(32, np.uint32)
    ids[6:8], ids[8:10], ids[30:32] = 1, 2, 3
    return pal, ids


def cornell_mirror_materials():
    """cornell_materials() with a fifth material, a mirror (albedo (.9, .9, .9),
    no emission, bihrt.MAT_MIRROR), on the back wall (triangles 0 and 1) and the
    tall block (10 .. 19), for Renderer.render_path_spec; (5,)
    bihrt.MATERIAL_DTYPE and the (32,) uint32 ids."""
    from . import MAT_MIRROR, MATERIAL_DTYPE, pack_materials
    base, ids = cornell_materials()
    pal = np.zeros(5, MATERIAL_DTYPE)       # (np.concatenate would repack the overlapping fields)
    pal[:4], pal[4:] = base, pack_materials([(0.9, 0.9, 0.9, 0, 0, 0, MAT_MIRROR)])
    ids[0:2], ids[10:20] = 4, 4
    return pal, ids
