#!/usr/bin/env python3
"""Path-render rate (bih_render_path_device: 1 .. --bounces levels) on the 1M
soup at 1920 x 1080 x 4 with the reference camera under scenes.panels(scene
box), albedo 0.5, sky 0.25: tools/indirect_rate.py's setup.  HIP events after
warm-up, one process, one stream; median, min and max of --reps runs of one
and the same frame:

  (1) one level   bih_render_path_device at n_bounces = 1 against
                  bih_render_indirect_device, all five planes each, the two
                  calls alternated run by run;
  (2) per level   bih_render_path_device at n_bounces = 1 .. --bounces, all five
                  planes and irradiance only; level k's added time is the median
                  at k minus the median at k - 1.  Next to it the composed route
                  of that level: bih_trace_device(CLOSEST) of the level's rays
                  plus bih_trace_device(OCCLUDED_WITHIN, t_hi = 1) of its facing
                  (bounce hit, panel) pairs, both ray sets prepared in device
                  memory outside the timer (the route leaves out the hashes, the
                  ray generation, the lists and the sums).

Per level also the call's own counts (live paths, escapes, non-zero lit words)
from its planes and the route's ray counts.  The route's hit points are rebuilt
level by level in torch, the call's are o + t*d in the kernels: the same points
to rounding, so the counts agree closely, not bit for bit.
Prints one JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bih-gpu-raytracer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from area_rate import mix, panel_points  # noqa: E402

F32, U32 = np.float32, np.uint32
C1, C3, C5, C7, C9 = (F32(float.fromhex(x)) for x in
                      ("0x1.921fb6p+0", "-0x1.4abbcep-1", "0x1.466bc6p-4", "-0x1.32d2ccp-8", "0x1.507834p-13"))


def sphere_points(seed, gp, fs, level):
    """include/bih.h's unit-sphere point of level `level` for global pixels gp and counters fs (u32 arrays)."""
    h = mix(U32(seed & 0xFFFFFFFF))
    h = mix(h ^ U32(seed >> 32))
    h = mix(mix(mix(h ^ gp) ^ fs) ^ U32((0x80000000 + level - 1) & 0xFFFFFFFF))
    a = (mix(h + U32(0x9E3779B9)) >> U32(8)).astype(F32) * F32(2.0 ** -24)
    b = (mix(h + U32(0x3C6EF372)) >> U32(8)).astype(F32) * F32(2.0 ** -24)
    z = F32(1.0) - F32(2.0) * a
    r = np.sqrt(np.fmax(F32(0.0), F32(1.0) - z * z))
    b4 = F32(4.0) * b
    q = b4.astype(np.int32)
    f = b4 - q.astype(F32)

    def S(x):
        x2 = x * x
        return ((((C9 * x2 + C7) * x2 + C5) * x2 + C3) * x2 + C1) * x
    sn, cs = S(f), S(F32(1.0) - f)
    cx = np.select([q == 0, q == 1, q == 2], [cs, -sn, -cs], sn)
    sx = np.select([q == 0, q == 1, q == 2], [sn, cs, -sn], -cs)
    return np.stack([r * cx, r * sx, z], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--albedo", type=float, default=0.5)
    ap.add_argument("--sky", type=float, default=0.25)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bihrt
    assert bihrt.device_count() > 0, "no HIP device"
    assert 1 <= a.bounces <= bihrt.MAX_BOUNCES
    w, h, spp, frame, nb = a.width, a.height, 4, 1, a.bounces
    P, n = w * h, w * h * spp
    s = torch.cuda.Stream()
    tris = bihrt.scenes.soup(a.tris, seed=1)
    d_soup = torch.from_numpy(tris).cuda()
    torch.cuda.synchronize()
    g = bihrt.GPUArrayManager.from_device(d_soup.data_ptr(), tris.shape[0], stream=s.cuda_stream)
    r = bihrt.Renderer(g, w, h, spp=spp, camera=bihrt.camera_reference(w, h))
    info = g.info()
    panels = bihrt.scenes.panels(info.scene_lo[:], info.scene_hi[:])
    K = panels.shape[0]
    bounce = (a.albedo, a.sky)

    def run(launch):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        launch()
        e1.record(s)
        s.synchronize()
        return e0.elapsed_time(e1)

    def stats(ms):
        return [round(float(np.median(ms)), 3), round(float(min(ms)), 3), round(float(max(ms)), 3)]

    def timed(*launches):
        """[median, min, max] device ms of each launch on stream s, the launches alternated run by run."""
        for _ in range(a.warmup):
            for launch in launches:
                launch()
        s.synchronize()
        ms = [[] for _ in launches]
        for _ in range(a.reps):
            for k, launch in enumerate(launches):
                ms[k].append(run(launch))
        return [stats(m) for m in ms]

    res = {"tool": "path_rate", "tris": int(tris.shape[0]), "image": [w, h, spp], "samples": n, "panels": K,
           "frame": frame, "albedo": a.albedo, "sky": a.sky, "warmup": a.warmup, "reps": a.reps, "bounces": nb,
           "ms": "median, min, max"}

    lit = torch.zeros(n, dtype=torch.int64, device="cuda")
    lits = torch.zeros(nb * n, dtype=torch.int64, device="cuda")
    brec = torch.zeros(nb * n * 16, dtype=torch.uint8, device="cuda")
    irr = torch.zeros(P, dtype=torch.float32, device="cuda")
    rgba = torch.zeros(P, dtype=torch.int32, device="cuda")
    five_i = {"lit": lit.data_ptr(), "bounce": brec.data_ptr(), "lit2": lits.data_ptr(), "irradiance": irr.data_ptr(),
              "rgba": rgba.data_ptr()}
    five_p = {"lit": lit.data_ptr(), "bounces": brec.data_ptr(), "lits": lits.data_ptr(), "irradiance": irr.data_ptr(),
              "rgba": rgba.data_ptr()}

    def indirect():
        r.render_indirect_device(five_i, None, None, panels, bounce, frame, stream=s.cuda_stream)

    def path(k, ptrs):
        return lambda: r.render_path_device(ptrs, None, None, panels, bounce, k, frame, stream=s.cuda_stream)

    # (1) one level against the one-bounce call, alternated
    ti, tp = timed(indirect, path(1, five_p))
    res["indirect_ms"], res["path1_ms"] = ti, tp
    res["path1_minus_indirect_ms"] = round(tp[0] - ti[0], 3)
    res["indirect_spread_ms"], res["path1_spread_ms"] = round(ti[2] - ti[1], 3), round(tp[2] - tp[1], 3)

    # (2) per level: all five planes, and irradiance only
    res["path_ms"] = {"1": tp}
    for k in range(2, nb + 1):
        res["path_ms"][str(k)] = timed(path(k, five_p))[0]
    res["path_irradiance_ms"] = {str(k): timed(path(k, {"irradiance": irr.data_ptr()}))[0] for k in range(1, nb + 1)}
    res["mean_irradiance"] = round(float(irr.mean()), 5)
    for key in ("path_ms", "path_irradiance_ms"):
        res[key.replace("_ms", "_level_ms")] = {str(k): round(res[key][str(k)][0] - res[key][str(k - 1)][0], 3)
                                               for k in range(2, nb + 1)}

    # the call's own counts, from the planes of the deepest all-planes run
    path(nb, five_p)()
    s.synchronize()
    prims = brec.view(torch.int32).reshape(nb, n, 4)[:, :, 3]
    live = [int((prims[k] != -1).sum()) for k in range(nb)]
    gb = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    r.render_gbuffer_device({"hits": gb.data_ptr()}, frame, stream=s.cuda_stream)
    s.synchronize()
    rec = gb.view(torch.float32).reshape(n, 4)
    prim = gb.view(torch.int32).reshape(n, 4)[:, 3]
    idx = (prim != -1).nonzero().squeeze(1)
    res["hit_samples"] = int(idx.shape[0])
    res["live"] = live
    res["escaped"] = [b - c for b, c in zip([res["hit_samples"]] + live[:-1], live)]
    res["lit_words"] = [int((lits.reshape(nb, n)[k] != 0).sum()) for k in range(nb)]

    # the composed route, level by level
    def normals_of(pr):
        tri = d_soup.reshape(-1, 9)[pr.long()]
        e1, e2 = tri[:, 3:6] - tri[:, 0:3], tri[:, 6:9] - tri[:, 0:3]
        nrm = torch.cross(e1, e2, dim=1)
        return tri, e1, e2, nrm / nrm.norm(dim=1, keepdim=True)

    tri, e1, e2, nrm = normals_of(prim[idx])
    pt = tri[:, 0:3] + rec[idx, 1:2] * e1 + rec[idx, 2:3] * e2
    del tri, e1, e2, gb
    res["route_rays"], res["route_shadow_rays"], res["route_closest_ms"], res["route_within_ms"] = [], [], [], []
    res["route_ms"] = []
    for k in range(1, nb + 1):
        i_host = idx.cpu().numpy()
        gp, fs = (i_host // spp).astype(U32), ((frame * spp + i_host % spp) & 0xFFFFFFFF).astype(U32)
        m1 = int(idx.shape[0])
        B = nrm + torch.from_numpy(sphere_points(r.seed, gp, fs, k)).cuda()
        rays1 = torch.zeros((max(m1, 1), 8), dtype=torch.float32, device="cuda")
        rays1[:m1, 0:3], rays1[:m1, 3], rays1[:m1, 4:7] = pt, bihrt.SHADOW_T_LO, B
        out1 = torch.zeros(max(m1, 1) * 16, dtype=torch.uint8, device="cuda")

        def closest():
            g.trace_device(rays1.data_ptr(), m1, out1.data_ptr(), bihrt.QUERY_CLOSEST, s.cuda_stream)

        closest()
        s.synchronize()
        t2 = out1.view(torch.float32).reshape(-1, 4)[:m1, 0:1]
        prim2 = out1.view(torch.int32).reshape(-1, 4)[:m1, 3]
        i2 = (prim2 != -1).nonzero().squeeze(1)
        pt = pt[i2] + t2[i2] * B[i2]
        nrm = normals_of(prim2[i2])[3]
        idx = idx[i2]
        i2_host = i2.cpu().numpy()
        parts = []
        for j in range(K):
            Q = torch.from_numpy(panel_points(panels[j], j, r.seed, gp[i2_host], fs[i2_host])).cuda()
            U, V = (torch.from_numpy(np.ascontiguousarray(panels[j][c])).cuda() for c in ("edge_u", "edge_v"))
            nl = torch.cross(U, V, dim=0)
            L = Q - pt
            c, ge = (nrm * L).sum(1), -(L * nl[None, :]).sum(1)
            si = ((c > 0) & (ge > 0)).nonzero().squeeze(1)
            part = torch.zeros((int(si.shape[0]), 8), dtype=torch.float32, device="cuda")
            part[:, 0:3], part[:, 3], part[:, 4:7], part[:, 7] = pt[si], bihrt.SHADOW_T_LO, L[si], 1.0
            parts.append(part)
        rays2 = torch.cat(parts)
        m2 = int(rays2.shape[0])
        flags = torch.zeros(max(m2, 1), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def within():
            g.trace_device(rays2.data_ptr(), m2, flags.data_ptr(), bihrt.QUERY_OCCLUDED_WITHIN, s.cuda_stream)

        def route():
            closest()
            within()

        tc, tw, tr = timed(closest, within, route)
        res["route_rays"].append(m1)
        res["route_shadow_rays"].append(m2)
        res["route_closest_ms"].append(tc)
        res["route_within_ms"].append(tw)
        res["route_ms"].append(tr)
        del rays1, out1, rays2, flags, parts, B
    res["route_live"] = res["route_rays"][1:] + [int(idx.shape[0])]
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        d = os.path.dirname(a.out)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
