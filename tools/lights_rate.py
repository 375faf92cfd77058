#!/usr/bin/env python3
"""Point-light rate (bih_render_lights_device, segment queries) on the 1M soup
at 1920 x 1080 x 4 with the reference camera under scenes.lamps(scene box, 8),
HIP events after warm-up, one process, one stream.  Median and min of --reps
runs of one and the same frame:

  (a) closest  the only route before the segment queries: a G-buffer launch
               (hits) plus bih_trace_device(CLOSEST) on the facing (sample,
               lamp) pairs' rays, which are prepared in device memory outside
               the timer; the compare of each record's t with 1 is outside the
               timer too (the figure leaves out the read-back, the ray
               generation, the compare and the reduction that route needs);
  (b) within   the same launch plus the same rays through
               bih_trace_device(OCCLUDED_WITHIN), t_hi = 1;
  (c) lights   bih_render_lights_device, `lit` only, and all three planes.

Also timed alone: the G-buffer launch (`hits`) and the two traces, which give
the per-ray rates.  From (a)'s records: the shares of the facing pairs blocked
before the lamp, blocked only at or beyond it, and not blocked.

(a)'s hit points are rebuilt from the records' barycentrics ((1-u-v) v0 + u v1
+ v v2), the call's are o + t*d: the same points to rounding, so the facing
pairs are the same and the lit shares agree closely, not bit for bit.
Prints one JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bih-gpu-raytracer_amd"))

F32 = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--lamps", type=int, default=8)
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
    lamps = bihrt.scenes.lamps(info.scene_lo[:], info.scene_hi[:], a.lamps)
    K = lamps.shape[0]

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

    res = {"tool": "lights_rate", "tris": int(tris.shape[0]), "image": [w, h, spp], "samples": n, "lamps": K,
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
    Q = torch.from_numpy(np.ascontiguousarray(lamps["pos"])).cuda()
    L = Q[None, :, :] - pt[:, None, :]
    facing = (nrm[:, None, :] * L).sum(2) > 0
    si, ki = facing.nonzero(as_tuple=True)
    m = int(si.shape[0])
    rays = torch.zeros((m, 8), dtype=torch.float32, device="cuda")
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = pt[si], bihrt.SHADOW_T_LO, L[si, ki], 1.0
    recs = torch.zeros(m * 16, dtype=torch.uint8, device="cuda")
    flags = torch.zeros(m, dtype=torch.uint8, device="cuda")
    del tri, v0, e1, e2, u, v, pt, nrm, rec, L, facing
    torch.cuda.synchronize()
    res["shadow_rays"] = m
    res["facing_share"] = round(m / max(int(idx.shape[0]) * K, 1), 4)

    def gbuffer():
        r.render_gbuffer_device({"hits": hits.data_ptr()}, frame, stream=s.cuda_stream)

    def closest():
        g.trace_device(rays.data_ptr(), m, recs.data_ptr(), bihrt.QUERY_CLOSEST, s.cuda_stream)

    def within():
        g.trace_device(rays.data_ptr(), m, flags.data_ptr(), bihrt.QUERY_OCCLUDED_WITHIN, s.cuda_stream)

    def route_a():
        gbuffer()
        closest()

    def route_b():
        gbuffer()
        within()

    lit = torch.zeros(n, dtype=torch.int64, device="cuda")
    irr = torch.zeros(P, dtype=torch.float32, device="cuda")
    rgba = torch.zeros(P, dtype=torch.int32, device="cuda")

    def lights(ptrs):
        return lambda: r.render_lights_device(ptrs, None, lamps, frame, stream=s.cuda_stream)

    record("closest_route", timed(route_a))
    t = recs.view(torch.float32).reshape(m, 4)[:, 0]
    blocker = recs.view(torch.int32).reshape(m, 4)[:, 3] != -1
    before = blocker & (t < 1.0)
    res["before_share"] = round(float(before.float().mean()), 4)
    res["beyond_only_share"] = round(float((blocker & ~before).float().mean()), 4)
    res["none_share"] = round(float((~blocker).float().mean()), 4)
    record("within_route", timed(route_b))
    assert bool((flags == before.to(torch.uint8)).all()), "OCCLUDED_WITHIN differs from CLOSEST's t < 1"
    record("hits", timed(gbuffer))
    record("closest_trace", timed(closest))
    record("within_trace", timed(within))
    record("lit", timed(lights({"lit": lit.data_ptr()})))
    bitsum = sum(int(((lit >> k) & 1).sum()) for k in range(K))
    res["lit_share"] = round(bitsum / max(m, 1), 4)
    res["trace_lit_share"] = round(float((flags == 0).float().mean()), 4)
    assert int((lit >> K).ne(0).sum()) == 0, "bits above the lights"
    record("planes", timed(lights({"lit": lit.data_ptr(), "irradiance": irr.data_ptr(), "rgba": rgba.data_ptr()})))
    res["mean_irradiance"] = round(float(irr.mean()), 5)
    for k in ("within_route", "lit", "planes"):
        res[f"{k}_over_closest_route"] = round(res[f"{k}_ms"] / res["closest_route_ms"], 3)
    res["closest_route_spread_ms"] = round(res["closest_route_max_ms"] - res["closest_route_min_ms"], 3)
    res["closest_trace_spread_ms"] = round(res["closest_trace_max_ms"] - res["closest_trace_min_ms"], 3)
    res["within_trace_faster_beyond_spread"] = bool(
        res["within_trace_ms"] + res["closest_trace_spread_ms"] < res["closest_trace_ms"])
    res["closest_mrays_per_s"] = round(m / res["closest_trace_ms"] / 1e3, 1)
    res["within_mrays_per_s"] = round(m / res["within_trace_ms"] / 1e3, 1)
    res["lights_mrays_per_s"] = round(m / max(res["lit_ms"] - res["hits_ms"], 1e-6) / 1e3, 1)
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
