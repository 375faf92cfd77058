"""Solid tiles: tiles of the frustum bins in which every sample of every pixel
provably hits whatever its jitter (csrc/bih_bins.hip: sure_mask, k_queue_class;
csrc/bih_bound.h: sure_applies).  k_render_bins writes them as constants, so a
wrong proof shows as a full pixel where the oracle has a partial one.

CPU: the scene's guard by the oracle alone, and the sure bound restated in
numpy (the thresholds of edge_pretest and sure_mask op for op, next to
tests/test_bin_pretest.py's restatement of the pre-test): every pixel it calls
sure has the numpy-f32 intersector accept every attainable sample.  That is the
acceptance half of the proof; the reachability half (plan bit, slab bit) needs
the tree and is checked on the GPU against the oracle's walk.

GPU: the sure words read back against the oracle, render parity in ring,
stamped, band and cut-tile launches, the A/B knob, staleness, the mask path
(Whitted, G-buffer) and the counter build's "bin-items" line.  The same file is
the script of the child processes (knob, counters).
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np

if __name__ == "__main__":      # a child process: the tests' own directory, then as conftest sets the paths
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pytest

import camera_cases as cc
from conftest import ROOT
from test_bin_pretest import (E, _bin_camera, _edge_margin, _f32_up, _pretest_coeffs, _refined_bounds,
                              _scene_on_rays)
from test_cameras import SEED, cam_of, diff, to_camera
from test_miss_box import F, _barycentric_bounds, _camera_dir, _mt, _offset_cameras, _tri_prim

W, H, SPP = 320, 208, 4
NT = (W // 4) * (H // 4)            # 4160 tiles
FULL = 0x00FFFF
GUARD = (609, 407, 3144)            # tiles full in every pixel of frames 0-3, mixed, background (the oracle)
FC_LIB = os.path.join(ROOT, "bih-gpu-raytracer_amd", "lib", "variants", "libbih_amd_fc.so")
GAP = 64
R_LO, R_HI = F(2.3283064e-10) / F(2), F(1.0)      # xorwow_to_uniform's smallest and largest value


@functools.lru_cache(maxsize=None)
def soup(seed=1):
    from bihrt import scenes
    t = np.ascontiguousarray(scenes.soup(8000, seed=seed, half=0.2), np.float32).reshape(-1, 9)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def otree(seed=1):
    import oracle
    return oracle.OracleTree(soup(seed))


def camera(name, w, h):
    return np.asarray(cam_of(name, w, h), F)


@functools.lru_cache(maxsize=None)
def oracle_frame(seed, name, w, h, frame):
    img = otree(seed).render(w, h, spp=SPP, frame=frame, seed=SEED, cam=camera(name, w, h))[0]
    img.setflags(write=False)
    return img


def tiles_of(img, value):
    """(tiles_y, tiles_x) bool: every pixel of the 4 x 4 tile equals `value` (whole tiles only)."""
    h, w = img.shape
    return (img[:h - h % 4, :w - w % 4].reshape(h // 4, 4, w // 4, 4) == value).all(axis=(1, 3))


@functools.lru_cache(maxsize=None)
def oracle_classes(seed=1, name="reference"):
    """(full, background) tile masks over frames 0-3 of the scene."""
    imgs = [oracle_frame(seed, name, W, H, f) for f in range(4)]
    full = np.logical_and.reduce([tiles_of(i, FULL) for i in imgs])
    bg = np.logical_and.reduce([tiles_of(i, cc.BACKGROUND) for i in imgs])
    return full, bg


# --- the sure bound, restated -----------------------------------------------------

def _sure_record(e1, e2, s, tn, dm, cam):
    """k_bin_fp's sure thresholds: (K, S, eligible) -- the pre-test's
    coefficient triples, the three thresholds f32_up(1.01 (2.02 a_j U + 2 M))
    and where sure_applies (acceptance only: no plan, no slab bit here)."""
    n, an, dn_lb = _bin_camera(cam)
    cam64 = np.asarray(cam, np.float64)
    O, llc, h, vert = cam64[:3], cam64[3:6], cam64[6:9], cam64[9:12]
    a0, b0, c0 = _barycentric_bounds(e1, e2, s, dm)
    a, b, c, take = _refined_bounds(e1, e2, s, tn, dm, cam)
    e164, e264, s64 = (x.astype(np.float64) for x in (e1, e2, s))
    as_, ae1 = np.abs(s64), np.abs(e164)
    Q = np.stack([as_[:, 1] * ae1[:, 2] + ae1[:, 1] * as_[:, 2], as_[:, 2] * ae1[:, 0] + ae1[:, 2] * as_[:, 0],
                  as_[:, 0] * ae1[:, 1] + ae1[:, 0] * as_[:, 1]], 1)
    et = 8.0 * E * np.einsum("ij,ij->i", np.abs(e264), Q)

    def depths(a_, b_, c_):
        a_, b_, c_ = (x.astype(np.float64) for x in (a_, b_, c_))
        cu, cv = [-a_, 1.0 + b_ + c_, -a_], [-b_, -b_, 1.0 + a_ + c_]
        d, front = [], np.ones(len(a_), bool)
        for j in range(3):
            X = cu[j][:, None] * e164 + cv[j][:, None] * e264 - s64
            d.append(X @ n)
            front &= d[-1] > 1e-9 * np.linalg.norm(X, axis=1) * np.linalg.norm(n)
        return np.max(d, 0), np.min(d, 0), front

    maxd0, _, _ = depths(a0, b0, c0)
    _, mind, front = depths(a, b, c)
    tn64 = tn.astype(np.float64)
    L = 0.99 * (tn64 - et) * dn_lb / maxd0
    U = np.where(mind > 0, 1.01 * (tn64 + et) * (2.0 * an - dn_lb) / np.where(mind > 0, mind, 1.0), np.inf)
    U = np.where(U == U, U, np.inf)
    elig = take & front & (np.where(take, L, 0).astype(F) >= F(2e-6)) & (U < 1e6) & (tn > F(1e-30)) & \
        (tn < F(1e30)) & ((a + b) + c < F(0.5))
    # edge_pretest's M per edge (the coefficient triples are _pretest_coeffs')
    K = _pretest_coeffs(e1, e2, s, a, b, c, cam)
    A = llc - O
    delta = 8.0 * E * (np.abs(llc) + np.abs(h) + np.abs(vert) + np.abs(O))
    Nu, Nd, Qx = np.cross(e264, s64), np.cross(e264, e164), np.cross(s64, e164)
    a6, b6, c6 = (x.astype(np.float64)[:, None] for x in (a, b, c))
    S = []
    for g, aj in zip([Nu + a6 * Nd, Qx + b6 * Nd, (1.0 + c6) * Nd - Nu - Qx], (a6, b6, c6)):
        K0, Ku, Kv = g @ A, g @ h, g @ vert
        M = 4.0 * (np.abs(g) @ delta + 8.0 * E * (np.abs(K0) + np.abs(Ku) + np.abs(Kv)) + 1e-30)
        S.append(_f32_up(1.01 * (2.02 * aj[:, 0] * np.where(elig, U, 0.0) + 2.0 * _f32_up(M).astype(np.float64))))
    elig &= (S[0] < F(1e30)) & (S[1] < F(1e30)) & (S[2] < F(1e30))
    return K, S, elig


SURE_Q = 2                          # kSureQ (bih_internal.h): sub-rectangles per pixel side
SURE_N = 4 * SURE_Q


def _sure_mask(K, S, bx, by, w, h):
    """sure_mask (bih_bins.hip) of 4 x 4 tiles, op for op in f32: (n, SURE_N,
    SURE_N) bool, [sub-row, sub-column] of the tile's grid of sub-rectangles."""
    pad, step = F(2.0 ** -20), F(1.0) / F(SURE_Q)
    iw, ih = F(1.0) / F(w), F(1.0) / F(h)
    x = (bx[:, None] * SURE_N + np.arange(SURE_N)[None, :]).astype(F) * step
    y = (by[:, None] * SURE_N + np.arange(SURE_N)[None, :]).astype(F) * step
    ua, ub = x * iw - pad, (x + step) * iw + pad
    va, vb = y * ih - pad, (y + step) * ih + pad
    ok = np.ones((len(bx), SURE_N, SURE_N), bool)
    with np.errstate(all="ignore"):
        for (K0, Ku, Kv), st in zip(K, S):
            K0, Ku, Kv = (np.asarray(z, F)[:, None] for z in (K0, Ku, Kv))
            T = _edge_margin(K0, Ku, Kv) + np.asarray(st, F)[:, None]
            cu = K0 + np.fmin(Ku * ua, Ku * ub)
            cv = np.fmin(Kv * va, Kv * vb)
            ok &= (cu[:, None, :] + cv[:, :, None]) > T[:, :, None]
    return ok


def pixel_samples(x, y, w, h, rng, interior=6, ru=(0.0, 1.0), rv=(0.0, 1.0)):
    """(uf, vf) f32 arrays (len(x), k): the samples of pixels (x, y) the claim is
    checked on, for jitters ru in [ru[0], ru[1]] and rv alike (scalars or arrays
    per pixel; the lower ends clipped to the smallest uniform): the four
    corners of the attainable range uf = fl(fl(x + ru) / w), their nextafter
    neighbours inward, and seeded interior samples."""
    x, y = np.asarray(x).astype(F)[:, None], np.asarray(y).astype(F)[:, None]
    n = len(x)
    lo_u, hi_u = (np.broadcast_to(np.asarray(z, F), (n,))[:, None] for z in ru)
    lo_v, hi_v = (np.broadcast_to(np.asarray(z, F), (n,))[:, None] for z in rv)
    lo_u, lo_v = np.maximum(lo_u, R_LO), np.maximum(lo_v, R_LO)
    cu = np.concatenate([lo_u, lo_u, hi_u, hi_u], 1)
    cv = np.concatenate([lo_v, hi_v, lo_v, hi_v], 1)
    uf = ((x + cu).astype(F) / F(w)).astype(F)
    vf = ((y + cv).astype(F) / F(h)).astype(F)
    inf = np.array([1, 1, -1, -1], F)[None, :] * F(np.inf)
    ui = np.nextafter(uf, np.broadcast_to(inf, uf.shape)).astype(F)
    vi = np.nextafter(vf, np.broadcast_to(np.array([1, -1, 1, -1], F)[None, :] * F(np.inf), vf.shape)).astype(F)
    r1 = (lo_u + (hi_u - lo_u) * rng.random((n, interior)).astype(F)).astype(F)
    r2 = (lo_v + (hi_v - lo_v) * rng.random((n, interior)).astype(F)).astype(F)
    um = ((x + np.clip(r1, lo_u, hi_u)).astype(F) / F(w)).astype(F)
    vm = ((y + np.clip(r2, lo_v, hi_v)).astype(F) / F(h)).astype(F)
    return np.concatenate([uf, ui, um], 1), np.concatenate([vf, vi, vm], 1)


def restated_pixel_words(tris, cam, dmax, w, h):
    """(tiles_y, tiles_x) int: the sure pixels of every 4 x 4 tile by the numpy
    restatement's acceptance half alone (every triangle taken to carry the
    plan and slab bits), a pixel sure when all its sub-rectangles are, each by
    some triangle.  A superset of what the device may classify."""
    tris = np.asarray(tris, F).reshape(-1, 9)
    v = [tris[:, 0:3], tris[:, 3:6], tris[:, 6:9]]
    e1, e2 = (v[1] - v[0]).astype(F), (v[2] - v[0]).astype(F)
    s, q, tn = _tri_prim(v[0], e1, e2, np.asarray(cam[:3], F))
    idx = np.flatnonzero(tn > 0)
    e1, e2, s, tn = e1[idx], e2[idx], s[idx], tn[idx]
    dm = np.broadcast_to(np.asarray(dmax, F), e1.shape)
    with np.errstate(all="ignore"):
        K, S, elig = _sure_record(e1, e2, s, tn, dm, cam)
    O, llc, hh, vv = (np.asarray(cam, np.float64)[3 * k:3 * k + 3] for k in range(4))
    n = np.cross(hh, vv)
    px, py = [], []
    for vk in v:
        d = vk[idx].astype(np.float64) - O
        Y = d * (((llc - O) @ n) / (d @ n))[:, None] - (llc - O)
        px.append((Y @ hh) / (hh @ hh) * w)
        py.append((Y @ vv) / (vv @ vv) * h)
    px, py = np.stack(px, 1), np.stack(py, 1)
    tx, ty = -(-w // 4), -(-h // 4)
    # a sure sub-rectangle lies inside the triangle: the tiles of its vertices' bounding box, one more around
    bx0 = np.clip(np.floor(px.min(1) / 4).astype(np.int64) - 1, 0, tx - 1)
    bx1 = np.clip(np.floor(px.max(1) / 4).astype(np.int64) + 1, 0, tx - 1)
    by0 = np.clip(np.floor(py.min(1) / 4).astype(np.int64) - 1, 0, ty - 1)
    by1 = np.clip(np.floor(py.max(1) / 4).astype(np.int64) + 1, 0, ty - 1)
    on = elig & np.isfinite(px).all(1) & np.isfinite(py).all(1)
    nx, ny = bx1 - bx0 + 1, by1 - by0 + 1
    cover = np.zeros((ty, tx, SURE_N, SURE_N), bool)
    for dy in range(int(ny[on].max())):
        for dx in range(int(nx[on].max())):
            sel = np.flatnonzero(on & (dx < nx) & (dy < ny))
            if len(sel):
                bx, by = bx0[sel] + dx, by0[sel] + dy
                ok = _sure_mask([tuple(k[sel] for k in K3) for K3 in K], [st[sel] for st in S], bx, by, w, h)
                np.logical_or.at(cover, (by, bx), ok)
    pix = cover.reshape(ty, tx, 4, SURE_Q, 4, SURE_Q).all(axis=(3, 5)).reshape(ty, tx, 16)
    return (pix.astype(np.int64) << np.arange(16)[None, None, :]).sum(-1)


# --- CPU ------------------------------------------------------------------------

def test_guard(oracle_mod):
    """The scene by the oracle alone: tiles full in every pixel of frames 0-3,
    mixed, and background -- the GPU tests cannot be vacuous."""
    full, bg = oracle_classes()
    counts = (int(full.sum()), int((~full & ~bg).sum()), int(bg.sum()))
    print("full, mixed, background tiles:", counts)
    assert counts == GUARD and sum(counts) == NT


def _claim(cam, dmax, wh, v0, v1, v2, u, v, rng):
    """Every sub-rectangle of a pixel the restated bound calls sure for a
    triangle: the f32 intersector accepts all its samples.  Returns (triangles
    with the thresholds, sure sub-rectangles, rays)."""
    w, h = wh
    O = np.asarray(cam[:3], F)
    v0, v1, v2 = (np.asarray(x, F) for x in (v0, v1, v2))
    e1, e2 = (v1 - v0).astype(F), (v2 - v0).astype(F)
    s, q, tn = _tri_prim(v0, e1, e2, O)
    dm = np.broadcast_to(np.asarray(dmax, F), e1.shape)
    with np.errstate(all="ignore"):
        K, S, elig = _sure_record(e1, e2, s, tn, dm, cam)
    elig &= tn > 0
    # the tile of the ray the triangle was placed on, or a neighbour
    bx = np.clip((u.astype(np.float64) * w).astype(np.int64) // 4 + rng.integers(-1, 2, len(u)), 0, (w - 1) // 4)
    by = np.clip((v.astype(np.float64) * h).astype(np.int64) // 4 + rng.integers(-1, 2, len(u)), 0, (h - 1) // 4)
    ti, sy, sx = np.nonzero(_sure_mask(K, S, bx, by, w, h) & elig[:, None, None])
    x, y = bx[ti] * 4 + sx // SURE_Q, by[ti] * 4 + sy // SURE_Q
    keep = (x < w) & (y < h)
    ti, x, y, sx, sy = ti[keep], x[keep], y[keep], sx[keep], sy[keep]
    # the jitters that put a sample into this sub-rectangle of its pixel
    jx, jy = (sx % SURE_Q).astype(np.float64), (sy % SURE_Q).astype(np.float64)
    uf, vf = pixel_samples(x, y, w, h, rng, ru=(jx / SURE_Q, (jx + 1) / SURE_Q), rv=(jy / SURE_Q, (jy + 1) / SURE_Q))
    k = uf.shape[1]
    rep = np.repeat(ti, k)
    D = _camera_dir(cam, uf.reshape(-1), vf.reshape(-1))
    with np.errstate(all="ignore"):
        hit, _ = _mt(e1[rep], e2[rep], s[rep], q[rep], tn[rep], D)
    assert hit.all(), (int((~hit).sum()), len(hit))
    return int(elig.sum()), len(ti), len(hit)


def test_sure_pixels_accept_every_sample(bihrt_mod):
    """Near-edge-on and oblique triangles on the rays of the reference-shaped
    cameras far from the origin (test_miss_box's offset cameras), and the
    bench's soup shape under the reference camera."""
    rng = np.random.default_rng(41)
    tri = pix = rays = 0
    for cam in _offset_cameras()[:3]:
        dmax = bihrt_mod.camera_ray_bound(bihrt_mod.Camera.from_list(cam.tolist()))
        for edge_on in (True, False):
            t, p, r = _claim(cam, dmax, (1920, 1080), *_scene_on_rays(cam, 40_000, rng, edge_on), rng)
            print(f"origin {cam[:3]} edge-on {edge_on}: {t} triangles with thresholds, {p} sure sub-rectangles, {r} rays")
            tri, pix, rays = tri + t, pix + p, rays + r
    # the bench's soup at 1080p and the tests' at 320 x 208
    for (w, h), half, n in (((1920, 1080), 0.02, 60_000), ((W, H), 0.2, 8_000)):
        cam = np.asarray(bihrt_mod.camera_reference(w, h).as_list(), F)
        dmax = bihrt_mod.camera_ray_bound(bihrt_mod.Camera.from_list(cam.tolist()))
        c = np.stack([rng.uniform(0, 2.6667, n), rng.uniform(-1, 1, n), rng.uniform(0, 2, n)], 1)
        vtx = c[:, None, :] + rng.uniform(-half, half, (n, 3, 3))
        O, llc, hh, vv = (cam[3 * k:3 * k + 3].astype(np.float64) for k in range(4))
        d = vtx.mean(1) - O
        Y = d * ((llc - O)[2] / d[:, 2])[:, None] - (llc - O)
        u = np.clip(Y[:, 0] / hh[0], 0, 1).astype(F)
        vq = np.clip(Y[:, 1] / vv[1], 0, 1).astype(F)
        t, p, r = _claim(cam, dmax, (w, h), vtx[:, 0], vtx[:, 1], vtx[:, 2], u, vq, rng)
        print(f"soup half {half} at {w}x{h}: {t} triangles with thresholds, {p} sure sub-rectangles, {r} rays")
        assert p > 1000, (w, h, p)
        tri, pix, rays = tri + t, pix + p, rays + r
    assert tri > 20_000 and pix > 20_000 and rays > 200_000, (tri, pix, rays)


def test_sure_mask_is_inside_the_pixel_mask(bihrt_mod):
    """A pixel with a sure sub-rectangle passes the pre-test (its bit of
    pixel_mask is set): the thresholds are positive, so min > T + S over a part
    of the pixel's rectangle implies max >= -T over the whole."""
    from test_bin_pretest import _pixel_mask
    rng = np.random.default_rng(5)
    cam = np.asarray(bihrt_mod.camera_reference(W, H).as_list(), F)
    dmax = bihrt_mod.camera_ray_bound(bihrt_mod.Camera.from_list(cam.tolist()))
    v0, v1, v2, u, v = _scene_on_rays(cam, 20_000, rng, False)
    v0, v1, v2 = (np.asarray(x, F) for x in (v0, v1, v2))
    e1, e2 = (v1 - v0).astype(F), (v2 - v0).astype(F)
    s, q, tn = _tri_prim(v0, e1, e2, cam[:3])
    dm = np.broadcast_to(np.asarray(dmax, F), e1.shape)
    with np.errstate(all="ignore"):
        K, S, elig = _sure_record(e1, e2, s, tn, dm, cam)
    assert all((st[elig] > 0).all() for st in S)
    bx = (u.astype(np.float64) * W).astype(np.int64).clip(0, W - 1) // 4
    by = (v.astype(np.float64) * H).astype(np.int64).clip(0, H - 1) // 4
    ok = _sure_mask(K, S, bx, by, W, H) & elig[:, None, None]
    pix = ok.reshape(-1, 4, SURE_Q, 4, SURE_Q).any(axis=(2, 4)).reshape(-1, 16)      # pixels with a sure sub-rectangle
    sm = (pix.astype(np.int64) << np.arange(16)[None, :]).sum(1)
    assert (sm & ~_pixel_mask(K, bx, by, W, H)).max() == 0 and (sm != 0).sum() > 100     # (not vacuous)


# --- GPU ------------------------------------------------------------------------

def rows_ys(rows, h):
    if rows is None:
        return np.arange(h)
    r = np.arange(rows.nrows)
    return rows.row0 + (r // rows.band_h) * rows.band_h * rows.band_step + r % rows.band_h


def plan_rows(bihrt, name):
    from bihrt.tiling import band_rows
    if name == "bands":
        return band_rows(H, 4, 1, 2)            # rank 1 of 2's aligned 4-row bands
    if name == "cut":
        # one band, 208 rows tall, of which the image has 206: band and start lie on tile rows, so the bins
        # serve the call, and the last tile row is cut at the image's bottom edge
        return bihrt.Rows(0, 206, 208, 1)
    if name == "cut_top":
        return bihrt.Rows(0, 204, 204, 1)       # whole tile rows of the 322 x 206 image: the bins serve them
    return None


# name -> (w, h, [(first frame, frames, stream)])
PLANS = {
    "ring": (W, H, [(0, 16, 0), (16, 1, 1), (17, 1, 2), (18, 1, 1), (19, 1, 2)]),
    "stamped": (W, H, [(16 * k, 16, 0) for k in range(5)]),
    "bands": (W, H, [(0, 16, 0)]),
    "cut": (322, 206, [(0, 16, 0)]),            # tiles cut at both edges, through the bins (plan_rows)
    "cut_top": (322, 206, [(0, 16, 0)]),        # its first 204 rows through the bins: tiles cut at the right edge
}


def run_plan(bihrt, name):
    """The plan's calls under the reference camera on a fresh tree: per call
    the first and last frame (nrows, w) u32, and the tree's solid count after."""
    import torch
    w, h, calls = PLANS[name]
    rows = plan_rows(bihrt, name)
    nrows = rows.nrows if rows is not None else h
    P = nrows * w
    stride = P + GAP
    g = bihrt.GPUArrayManager(soup())
    bufs = [torch.full((n * stride,), -1, dtype=torch.int32, device="cuda") for _, n, _ in calls]
    streams = {k: torch.cuda.Stream() for k in sorted({c[2] for c in calls} - {0})}
    torch.cuda.synchronize()
    r = bihrt.Renderer(g, w, h, spp=SPP, seed=SEED, camera=to_camera(bihrt, camera("reference", w, h)))
    for (first, n, sk), buf in zip(calls, bufs):
        st = streams[sk].cuda_stream if sk else None
        if n == 1:
            r.render_device(buf.data_ptr(), first, rows=rows, stream=st)
        else:
            r.render_device_frames(buf.data_ptr(), first, n, stride, rows=rows, stream=st)
        if sk:
            streams[sk].synchronize()
    r.sync()
    torch.cuda.synchronize()
    out = []
    for (_, n, _), buf in zip(calls, bufs):
        b = buf.cpu().numpy().view(np.uint32).reshape(n, stride)
        assert (b[:, P:] == 0xFFFFFFFF).all(), (name, "stride gap written")
        out.append(np.stack([b[0, :P].reshape(nrows, w), b[n - 1, :P].reshape(nrows, w)]))
    n_solid = g.bins_solid_masks()[1]
    g.close()
    return out, n_solid


@pytest.fixture(scope="module")
def default_frames(gpu, bihrt_mod):
    """Every plan once on the default library: {plan: (frames per call, solid count)}."""
    return {name: run_plan(bihrt_mod, name) for name in PLANS}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PLANS))
def test_render_parity(name, gpu, bihrt_mod, default_frames):
    """All rows of the first and last frame of each call equal the oracle: a
    16-frame call and one-frame calls alternating two streams (ring), five
    calls on one stream (stamped from the fourth), rank 1 of 2's aligned 4-row
    bands, the 322 x 206 image (one band taller than the image, so that the
    bins serve it: tiles cut at the right and at the bottom edge) and its first
    204 rows."""
    w, h, calls = PLANS[name]
    ys = rows_ys(plan_rows(bihrt_mod, name), h)
    frames, n_solid = default_frames[name]
    for (first, n, _), got in zip(calls, frames):
        for j, f in ((0, first), (1, first + n - 1)):
            ref = oracle_frame(1, "reference", w, h, f)[ys]
            assert np.array_equal(got[j], ref), (name, f, diff(got[j], ref))
    assert n_solid > 0, name


@pytest.mark.gpu
def test_knob_changes_no_pixel(gpu, bihrt_mod, default_frames, tmp_path):
    """The same calls in a child process with BIH_SOLID_TILES=0: bit-equal
    frames, and nothing is classified."""
    out = tmp_path / "frames.npz"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "knob", str(out)],
                       env=dict(os.environ, BIH_SOLID_TILES="0"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = np.load(out)
    for name, (_, _, calls) in PLANS.items():
        assert int(got[name + "_solid"]) == 0, name
        for k in range(len(calls)):
            a, b = got[f"{name}_{k}"], default_frames[name][0][k]
            assert np.array_equal(a, b), (name, k, diff(a, b))


@pytest.mark.gpu
def test_masks_against_the_oracle(gpu, bihrt_mod, oracle_mod):
    """The sure words read back: every solid tile is full in every pixel of
    the oracle's frames 0-3 and some tile is solid; the device's sure pixels
    are among those of the numpy restatement; the oracle's walk reports a
    hit for the corner, inward-neighbour and interior samples of up to 2000
    sure pixels; an inside camera (a non-empty global list) and 16 spp
    classify nothing."""
    g = bihrt_mod.GPUArrayManager(soup())
    cam = camera("reference", W, H)
    r = bihrt_mod.Renderer(g, W, H, spp=SPP, seed=SEED, camera=to_camera(bihrt_mod, cam))
    img = r.render(0)
    assert np.array_equal(img, oracle_frame(1, "reference", W, H, 0))
    words, n_solid = g.bins_solid_masks()
    full, bg = oracle_classes()
    solid = words == 0xFFFF
    print(f"solid tiles {n_solid} of the oracle's {int(full.sum())} always-full, sure pixels "
          f"{int(np.unpackbits(words.view(np.uint8)).sum())}")
    assert words.shape == full.shape and n_solid == int(solid.sum()) > 0
    assert not (solid & ~full).any(), int((solid & ~full).sum())
    assert not (words[bg] != 0).any()
    # the device's thresholds and sure_mask against their restatement: the device adds the plan and slab
    # bits, so its sure pixels are among the restatement's
    dmax = bihrt_mod.camera_ray_bound(to_camera(bihrt_mod, cam))
    rest = restated_pixel_words(soup(), cam, dmax, W, H)
    extra = words.astype(np.int64) & ~rest
    print(f"restated (acceptance only) sure pixels {int(sum(((rest >> b) & 1).sum() for b in range(16)))}")
    assert not extra.any(), (int((extra != 0).sum()), np.argwhere(extra != 0)[:4].tolist())
    ty, tx, bit = np.nonzero((words[:, :, None] >> np.arange(16)[None, None, :]) & 1)
    rng = np.random.default_rng(7)
    pick = rng.permutation(len(ty))[:2000]
    x, y = tx[pick] * 4 + bit[pick] % 4, ty[pick] * 4 + bit[pick] // 4
    # a sure pixel is full in every frame of the oracle
    for f in range(4):
        assert (oracle_frame(1, "reference", W, H, f)[y, x] == FULL).all(), f
    uf, vf = pixel_samples(x, y, W, H, rng, interior=2)
    D = _camera_dir(cam, uf.reshape(-1), vf.reshape(-1))
    hit = otree().trace(np.broadcast_to(cam[:3], D.shape), D)[0]
    assert hit.all(), (int((hit == 0).sum()), len(hit))
    # an inside camera: a non-empty global list, every tile live
    inside = cc.camera("inside_diag", W, H)
    r.camera = to_camera(bihrt_mod, inside)
    img = r.render(0)
    assert np.array_equal(img, otree().render(W, H, spp=SPP, frame=0, seed=SEED, cam=inside)[0])
    st = g.bins_stats()
    assert st.usable and st.global_entries > 0
    words, n_solid = g.bins_solid_masks()
    assert n_solid == 0 and not words.any()
    # 16 spp: 2 x 2-pixel tiles, no pixel masks
    r16 = bihrt_mod.Renderer(g, W, H, spp=16, seed=SEED, camera=to_camera(bihrt_mod, cam))
    img = r16.render(0)
    assert np.array_equal(img, otree().render(W, H, spp=16, frame=0, seed=SEED, cam=cam)[0])
    words, n_solid = g.bins_solid_masks()
    assert n_solid == 0 and not words.any()
    g.close()


@pytest.mark.gpu
def test_staleness(gpu, bihrt_mod):
    """In sequence, each step equal to the oracle of its own soup and camera:
    camera A, a moved camera, A again, a rebuild from another soup of the same
    size, a BINS_CAP too small (unusable bins: nothing solid) and back."""
    import torch
    n = 4
    dev = torch.from_numpy(soup(1).copy()).cuda()
    torch.cuda.synchronize()
    g = bihrt_mod.GPUArrayManager.from_device(dev.data_ptr(), len(soup(1)))
    r = bihrt_mod.Renderer(g, W, H, spp=SPP, seed=SEED)
    steps = [("reference", None, 1), ("moved2", None, 1), ("reference", None, 1), ("reference", None, 3),
             ("reference", 1000, 3), ("reference", 0, 3)]
    stride = H * W + GAP
    solids = []
    for k, (cam, cap, seed) in enumerate(steps):
        if cap is not None:
            g.set_param(bihrt_mod.PARAM_BINS_CAP, cap)
        if k and seed != steps[k - 1][2]:
            g.sync()
            dev.copy_(torch.from_numpy(soup(seed).copy()))
            torch.cuda.synchronize()
            g.rebuild()
        buf = torch.full((n * stride,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r.camera = to_camera(bihrt_mod, camera(cam, W, H))
        r.render_device_frames(buf.data_ptr(), n * k, n, stride)
        r.sync()
        b = buf.cpu().numpy().view(np.uint32).reshape(n, stride)
        for j in (0, n - 1):
            got, ref = b[j, :H * W].reshape(H, W), oracle_frame(seed, cam, W, H, n * k + j)
            assert np.array_equal(got, ref), (k, cam, seed, n * k + j, diff(got, ref))
        solids.append((bool(g.bins_stats().usable), g.bins_solid_masks()[1]))
    print("usable, solid per step:", solids)
    assert [u for u, _ in solids] == [True, True, True, True, False, True], solids
    assert all(s > 0 for (u, s) in solids if u) and solids[4][1] == 0
    assert solids[0][1] == solids[2][1] and solids[3][1] == solids[5][1]
    # a stale word would show: tiles always full under one soup are not under the other
    full1, full3 = oracle_classes(1)[0], oracle_classes(3)[0]
    assert (full1 & ~full3).any() and (full3 & ~full1).any()
    g.close()


@pytest.mark.gpu
def test_mask_path(gpu, bihrt_mod, oracle_mod):
    """One Whitted frame and one G-buffer frame of the scene (their primary
    pass takes the bins' hit masks): the Whitted image equals the oracle's;
    the G-buffer's per-sample hit flags equal the oracle's primary hits and its
    coverage plane their count per pixel."""
    g = bihrt_mod.GPUArrayManager(soup())
    cam = camera("reference", W, H)
    r = bihrt_mod.Renderer(g, W, H, spp=SPP, seed=SEED, camera=to_camera(bihrt_mod, cam))
    ref, _, dep = otree().render_whitted(W, H, spp=SPP, frame=1, seed=SEED, cam=cam, depths=True)
    img = r.render_whitted(1)
    assert np.array_equal(img, ref), diff(img, ref)
    gb = r.render_gbuffer(1, planes=("prim", "coverage"), hits=True)
    flags = gb["hits"]["prim"] != bihrt_mod.NO_HIT
    assert np.array_equal(flags, dep > 0), diff(flags, dep > 0)
    cov = (dep > 0).reshape(H, W, SPP).sum(-1)
    assert np.array_equal(gb["coverage"].astype(np.int64), cov)
    assert g.bins_solid_masks()[1] > 0 and (cov == SPP).mean() > 0.05
    g.close()


def _field(line, key):
    return int(re.search(r"(?<![\w-])" + re.escape(key) + r" (\d+)", line).group(1))


@pytest.mark.gpu
def test_counter_build_counts_solid_tiles(gpu):
    """The counter build, one 16-frame call: `solid` of the "bin-items" line
    equals the read-back count, tile-frames = live x 16, bg-tile-frames =
    (4160 - live) x 16 (solid tiles among them), and no plan disagrees with the
    root-path check."""
    assert os.path.exists(FC_LIB), "no counter build (lib/variants/libbih_amd_fc.so)"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "counters"],
                       env=dict(os.environ, BIH_LIB=FC_LIB), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stderr.splitlines()
    items = [ln for ln in lines if ln.startswith("bin-items")][-1]
    counters = [ln for ln in lines if ln.startswith("bin-counters")][-1]
    readback = int([ln for ln in lines if ln.startswith("solid-readback")][-1].split()[1])
    print(items)
    live, solid = _field(items, "live"), _field(items, "solid")
    full, bg = oracle_classes()
    assert solid == readback > 0
    assert NT - int(bg.sum()) <= live + solid <= NT      # (a tile with a hit has a list; a listed tile need not be hit)
    assert _field(items, "nframes") == 16 and _field(items, "tile-frames") == live * 16
    assert _field(items, "bg-tile-frames") == (NT - live) * 16
    assert _field(counters, "plan-disagrees") == 0


# --- the children -----------------------------------------------------------------

def _child(argv):
    import bihrt
    if argv[0] == "knob":
        out = {}
        for name in PLANS:
            frames, n_solid = run_plan(bihrt, name)
            out[name + "_solid"] = n_solid
            for k, f in enumerate(frames):
                out[f"{name}_{k}"] = f
        np.savez(argv[1], **out)
    elif argv[0] == "counters":
        import torch
        g = bihrt.GPUArrayManager(soup())
        stride = H * W + GAP
        buf = torch.full((16 * stride,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r = bihrt.Renderer(g, W, H, spp=SPP, seed=SEED, camera=to_camera(bihrt, camera("reference", W, H)))
        r.render_device_frames(buf.data_ptr(), 0, 16, stride)
        r.sync()
        sys.stderr.write(f"solid-readback {g.bins_solid_masks()[1]}\n")
        g.close()
    else:
        raise SystemExit("usage: test_solid_tiles.py knob OUT.npz | counters")


if __name__ == "__main__":
    _child(sys.argv[1:])
