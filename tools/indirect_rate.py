#!/usr/bin/env python3
"""Indirect-lighting rate (bih_render_indirect_device: one bounce and a sky
term) on the 1M soup at 1920 x 1080 x 4 with the reference camera under
scenes.panels(scene box), HIP events after warm-up, one process, one stream.
Median and min of --reps runs of one and the same frame:

  (a) area      bih_render_area_lights_device with the same set, all three
                planes: the direct light the call starts from;
  (b) route     the composed route: that area call, plus
                bih_trace_device(CLOSEST) of the same bounce rays, plus a second
                lighting pass, bih_trace_device(OCCLUDED_WITHIN, t_hi = 1) on
                the facing (bounce hit, panel) pairs' rays.  Both ray sets are
                prepared in device memory outside the timer (the figure leaves
                out the read-backs, the hashes, the ray generation and the
                sums that route needs);
  (c) indirect  bih_render_indirect_device, all five planes, and irradiance only.

Also timed alone: the two traces, which give the per-ray rates.  The route's
hit points are rebuilt from the records' barycentrics, the call's are o + t*d:
the same points to rounding, so the ray counts agree closely, not bit for bit;
the call's own counts (bounce hits, lit2 words) are printed next to the route's.
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


def sphere_points(seed, gp, fs):
    """include/bih.h's unit-sphere point of the bounce for global pixels gp and counters fs (u32 arrays)."""
    h = mix(U32(seed & 0xFFFFFFFF))
    h = mix(h ^ U32(seed >> 32))
    h = mix(mix(mix(h ^ gp) ^ fs) ^ U32(0x80000000))
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bihrt
    assert bihrt.device_count() > 0, "no HIP device"
    w, h, spp, frame = a.width, a.height, 4, 1
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

    def timed(launch):
        """Median / min / max device ms of `launch` on stream s."""
        for _ in range(a.warmup):
            launch()
        s.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            launch()
            e1.record(s)
            s.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    res = {"tool": "indirect_rate", "tris": int(tris.shape[0]), "image": [w, h, spp], "samples": n, "panels": K,
           "frame": frame, "albedo": a.albedo, "sky": a.sky, "warmup": a.warmup, "reps": a.reps}

    def record(label, t):
        res[f"{label}_ms"], res[f"{label}_min_ms"], res[f"{label}_max_ms"] = (round(x, 3) for x in t)

    def normals_of(prim):
        tri = d_soup.reshape(-1, 9)[prim.long()]
        e1, e2 = tri[:, 3:6] - tri[:, 0:3], tri[:, 6:9] - tri[:, 0:3]
        nrm = torch.cross(e1, e2, dim=1)
        return tri, e1, e2, nrm / nrm.norm(dim=1, keepdim=True)

    # the bounce rays of the frame, in device memory
    hits = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    r.render_gbuffer_device({"hits": hits.data_ptr()}, frame, stream=s.cuda_stream)
    s.synchronize()
    rec = hits.view(torch.float32).reshape(n, 4)
    prim = hits.view(torch.int32).reshape(n, 4)[:, 3]
    idx = (prim != -1).nonzero().squeeze(1)
    m1 = int(idx.shape[0])
    tri, e1, e2, nrm = normals_of(prim[idx])
    pt = tri[:, 0:3] + rec[idx, 1:2] * e1 + rec[idx, 2:3] * e2
    i_host = idx.cpu().numpy()
    gp, fs = (i_host // spp).astype(U32), ((frame * spp + i_host % spp) & 0xFFFFFFFF).astype(U32)
    B = nrm + torch.from_numpy(sphere_points(r.seed, gp, fs)).cuda()
    rays1 = torch.zeros((m1, 8), dtype=torch.float32, device="cuda")
    rays1[:, 0:3], rays1[:, 3], rays1[:, 4:7] = pt, bihrt.SHADOW_T_LO, B
    out1 = torch.zeros(m1 * 16, dtype=torch.uint8, device="cuda")
    res["hit_share"] = round(m1 / n, 4)
    res["bounce_rays"] = m1

    def closest():
        g.trace_device(rays1.data_ptr(), m1, out1.data_ptr(), bihrt.QUERY_CLOSEST, s.cuda_stream)

    closest()
    s.synchronize()
    # the second lighting pass' rays: the facing (bounce hit, panel) pairs
    t2 = out1.view(torch.float32).reshape(m1, 4)[:, 0:1]
    prim2 = out1.view(torch.int32).reshape(m1, 4)[:, 3]
    i2 = (prim2 != -1).nonzero().squeeze(1)
    res["route_bounce_hits"] = int(i2.shape[0])
    pt2 = pt[i2] + t2[i2] * B[i2]
    nrm2 = normals_of(prim2[i2])[3]
    i2_host = i2.cpu().numpy()
    parts = []
    for j in range(K):
        Q = torch.from_numpy(panel_points(panels[j], j, r.seed, gp[i2_host], fs[i2_host])).cuda()
        U, V = (torch.from_numpy(np.ascontiguousarray(panels[j][k])).cuda() for k in ("edge_u", "edge_v"))
        nl = torch.cross(U, V, dim=0)
        L = Q - pt2
        c, ge = (nrm2 * L).sum(1), -(L * nl[None, :]).sum(1)
        si = ((c > 0) & (ge > 0)).nonzero().squeeze(1)
        part = torch.zeros((int(si.shape[0]), 8), dtype=torch.float32, device="cuda")
        part[:, 0:3], part[:, 3], part[:, 4:7], part[:, 7] = pt2[si], bihrt.SHADOW_T_LO, L[si], 1.0
        parts.append(part)
    rays2 = torch.cat(parts)
    m2 = int(rays2.shape[0])
    flags = torch.zeros(max(m2, 1), dtype=torch.uint8, device="cuda")
    res["second_pass_rays"] = m2
    del tri, e1, e2, nrm, pt, B, rec, parts, pt2, nrm2
    torch.cuda.synchronize()

    def within():
        g.trace_device(rays2.data_ptr(), m2, flags.data_ptr(), bihrt.QUERY_OCCLUDED_WITHIN, s.cuda_stream)

    lit = torch.zeros(n, dtype=torch.int64, device="cuda")
    lit2 = torch.zeros(n, dtype=torch.int64, device="cuda")
    brec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    irr = torch.zeros(P, dtype=torch.float32, device="cuda")
    rgba = torch.zeros(P, dtype=torch.int32, device="cuda")
    three = {"lit": lit.data_ptr(), "irradiance": irr.data_ptr(), "rgba": rgba.data_ptr()}
    five = dict(three, bounce=brec.data_ptr(), lit2=lit2.data_ptr())

    def area():
        r.render_area_lights_device(three, None, None, panels, frame, stream=s.cuda_stream)

    def route():
        area()
        closest()
        within()

    def indirect(ptrs):
        return lambda: r.render_indirect_device(ptrs, None, None, panels, bounce, frame, stream=s.cuda_stream)

    record("area", timed(area))
    res["direct_mean_irradiance"] = round(float(irr.mean()), 5)
    record("route", timed(route))
    record("closest_trace", timed(closest))
    record("within_trace", timed(within))
    record("indirect", timed(indirect(five)))
    res["bounce_hits"] = int((brec.view(torch.int32).reshape(n, 4)[:, 3] != -1).sum())
    res["lit2_samples"] = int((lit2 != 0).sum())
    res["mean_irradiance"] = round(float(irr.mean()), 5)
    record("indirect_irradiance", timed(indirect({"irradiance": irr.data_ptr()})))
    record("sky_only", timed(lambda: r.render_indirect_device({"irradiance": irr.data_ptr()}, None, None, None,
                                                               bounce, frame, stream=s.cuda_stream)))
    for k in ("area", "route"):
        res[f"indirect_over_{k}"] = round(res["indirect_ms"] / res[f"{k}_ms"], 3)
    for k in ("area", "route", "indirect"):
        res[f"{k}_spread_ms"] = round(res[f"{k}_max_ms"] - res[f"{k}_min_ms"], 3)
    res["closest_mrays_per_s"] = round(m1 / res["closest_trace_ms"] / 1e3, 1)
    res["within_mrays_per_s"] = round(m2 / max(res["within_trace_ms"], 1e-6) / 1e3, 1)
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
