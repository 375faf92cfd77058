#!/usr/bin/env python3
"""Area-light rate (bih_render_area_lights_device, soft shadows) on the 1M soup
at 1920 x 1080 x 4 with the reference camera under scenes.panels(scene box),
HIP events after warm-up, one process, one stream.  Median and min of --reps
runs of one and the same frame:

  (a) route    the only route before the call: a G-buffer launch (hits) plus
               bih_trace_device(OCCLUDED_WITHIN, t_hi = 1) on the facing
               (sample, panel) pairs' rays, which are prepared in device memory
               outside the timer (the figure leaves out the read-back, the
               hash, the ray generation and the reduction that route needs);
  (b) area     bih_render_area_lights_device, `lit` only, and all three planes.

Also timed alone: the G-buffer launch (`hits`) and the trace, which give the
per-ray rates.  Ray counts per class: hit samples, (hit sample, panel) pairs
whose surface faces the point (c > 0), of those the pairs rejected by the
emitter's side (g <= 0), the facing pairs (= shadow rays), and of those the
blocked ones.

The route's panel points are the header's hash, restated here in numpy u32;
its hit points are rebuilt from the records' barycentrics ((1-u-v) v0 + u v1 +
v v2), the call's are o + t*d: the same points to rounding, so the facing pairs
are the same and the lit shares agree closely, not bit for bit.
Prints one JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bih-gpu-raytracer_amd"))

F32, U32 = np.float32, np.uint32


def mix(x):
    x = np.atleast_1d(x).astype(U32)
    x = x ^ (x >> U32(16))
    x = x * U32(0x7feb352d)
    x = x ^ (x >> U32(15))
    x = x * U32(0x846ca68b)
    return x ^ (x >> U32(16))


def panel_points(panel, j, seed, gp, fs):
    """include/bih.h's sample point of area light j for global pixels gp and counters fs (u32 arrays)."""
    h = mix(U32(seed & 0xFFFFFFFF))
    h = mix(h ^ U32(seed >> 32))
    h = mix(mix(mix(h ^ gp) ^ fs) ^ U32(j))
    a = (mix(h + U32(0x9E3779B9)) >> U32(8)).astype(F32) * F32(2.0 ** -24)
    b = (mix(h + U32(0x3C6EF372)) >> U32(8)).astype(F32) * F32(2.0 ** -24)
    c, u, v = (np.asarray(panel[k], F32) for k in ("corner", "edge_u", "edge_v"))
    return (c[None, :] + a[:, None] * u[None, :]) + b[:, None] * v[None, :]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
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

    res = {"tool": "area_rate", "tris": int(tris.shape[0]), "image": [w, h, spp], "samples": n, "panels": K,
           "frame": frame, "warmup": a.warmup, "reps": a.reps}

    def record(label, t):
        res[f"{label}_ms"], res[f"{label}_min_ms"], res[f"{label}_max_ms"] = (round(x, 3) for x in t)

    # the facing pairs' rays of the frame, in device memory
    hits = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    r.render_gbuffer_device({"hits": hits.data_ptr()}, frame, stream=s.cuda_stream)
    s.synchronize()
    rec = hits.view(torch.float32).reshape(n, 4)
    prim = hits.view(torch.int32).reshape(n, 4)[:, 3]
    hit = prim != -1
    res["hit_share"] = round(float(hit.float().mean()), 4)
    idx = hit.nonzero().squeeze(1)
    tri = d_soup.reshape(-1, 9)[prim[idx].long()]
    v0, e1, e2 = tri[:, 0:3], tri[:, 3:6] - tri[:, 0:3], tri[:, 6:9] - tri[:, 0:3]
    u, v = rec[idx, 1:2], rec[idx, 2:3]
    pt = v0 + u * e1 + v * e2
    nrm = torch.cross(e1, e2, dim=1)
    nrm = nrm / nrm.norm(dim=1, keepdim=True)
    i_host = idx.cpu().numpy()
    gp, fs = (i_host // spp).astype(U32), ((frame * spp + i_host % spp) & 0xFFFFFFFF).astype(U32)
    parts, counts = [], {"surface_facing_pairs": 0, "emitter_side_rejects": 0}
    for j in range(K):
        Q = torch.from_numpy(panel_points(panels[j], j, r.seed, gp, fs)).cuda()
        U, V = (torch.from_numpy(np.ascontiguousarray(panels[j][k])).cuda() for k in ("edge_u", "edge_v"))
        nl = torch.cross(U, V, dim=0)
        L = Q - pt
        c, ge = (nrm * L).sum(1), -(L * nl[None, :]).sum(1)
        counts["surface_facing_pairs"] += int((c > 0).sum())
        counts["emitter_side_rejects"] += int(((c > 0) & ~(ge > 0)).sum())
        si = ((c > 0) & (ge > 0)).nonzero().squeeze(1)
        part = torch.zeros((int(si.shape[0]), 8), dtype=torch.float32, device="cuda")
        part[:, 0:3], part[:, 3], part[:, 4:7], part[:, 7] = pt[si], bihrt.SHADOW_T_LO, L[si], 1.0
        parts.append(part)
    rays = torch.cat(parts)
    m = int(rays.shape[0])
    flags = torch.zeros(m, dtype=torch.uint8, device="cuda")
    del tri, v0, e1, e2, u, v, pt, nrm, rec, parts
    torch.cuda.synchronize()
    res["hit_samples"] = int(idx.shape[0])
    res.update(counts)
    res["shadow_rays"] = m
    res["facing_share"] = round(m / max(int(idx.shape[0]) * K, 1), 4)

    def gbuffer():
        r.render_gbuffer_device({"hits": hits.data_ptr()}, frame, stream=s.cuda_stream)

    def within():
        g.trace_device(rays.data_ptr(), m, flags.data_ptr(), bihrt.QUERY_OCCLUDED_WITHIN, s.cuda_stream)

    def route():
        gbuffer()
        within()

    lit = torch.zeros(n, dtype=torch.int64, device="cuda")
    irr = torch.zeros(P, dtype=torch.float32, device="cuda")
    rgba = torch.zeros(P, dtype=torch.int32, device="cuda")

    def area(ptrs):
        return lambda: r.render_area_lights_device(ptrs, None, None, panels, frame, stream=s.cuda_stream)

    record("route", timed(route))
    res["blocked_rays"] = int((flags == 1).sum())
    res["blocked_share"] = round(res["blocked_rays"] / max(m, 1), 4)
    record("hits", timed(gbuffer))
    record("within_trace", timed(within))
    record("lit", timed(area({"lit": lit.data_ptr()})))
    bitsum = sum(int(((lit >> k) & 1).sum()) for k in range(K))
    res["lit_share"] = round(bitsum / max(m, 1), 4)
    res["trace_lit_share"] = round(float((flags == 0).float().mean()), 4)
    assert int((lit >> K).ne(0).sum()) == 0, "bits above the lights"
    record("planes", timed(area({"lit": lit.data_ptr(), "irradiance": irr.data_ptr(), "rgba": rgba.data_ptr()})))
    res["mean_irradiance"] = round(float(irr.mean()), 5)
    for k in ("lit", "planes"):
        res[f"{k}_over_route"] = round(res[f"{k}_ms"] / res["route_ms"], 3)
    res["route_spread_ms"] = round(res["route_max_ms"] - res["route_min_ms"], 3)
    res["lit_spread_ms"] = round(res["lit_max_ms"] - res["lit_min_ms"], 3)
    res["within_mrays_per_s"] = round(m / res["within_trace_ms"] / 1e3, 1)
    res["area_mrays_per_s"] = round(m / max(res["lit_ms"] - res["hits_ms"], 1e-6) / 1e3, 1)
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
