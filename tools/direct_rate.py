#!/usr/bin/env python3
"""Direct-lighting render rate (bih_render_direct_device) on the 1M soup at
1920 x 1080 x 4 with the reference camera under scenes.sky_dome(8, sun), HIP
events after warm-up, one process, one stream.  Median and min of --reps runs
of one and the same frame:

  (a) compose  the route a caller has without the call:
               bih_render_gbuffer_device(hits) + bih_trace_device(OCCLUDED) on
               the facing (sample, light) pairs' rays, which are prepared in
               device memory outside the timer (so the figure leaves out the
               read-back, the ray generation and the reduction that route also
               needs);
  (b) lit      bih_render_direct_device, `lit` only;
  (c) planes   bih_render_direct_device, all three planes.

Also timed alone: the G-buffer launch of (a) (`hits`) and its trace (`trace`),
which give the per-ray rates: shadow rays per second of the trace, and of the
call's own kernels ((b) minus `hits`).

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
SUN = (0.3, 1.0, -0.4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--sky", type=int, default=8)
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
    lights = bihrt.scenes.sky_dome(a.sky, SUN)
    K = lights.shape[0]

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

    res = {"tool": "direct_rate", "tris": int(tris.shape[0]), "image": [w, h, spp], "samples": n, "lights": K,
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
    L = torch.from_numpy(np.ascontiguousarray(lights["dir"])).cuda()
    facing = (nrm @ L.T) > 0
    si, ki = facing.nonzero(as_tuple=True)
    m = int(si.shape[0])
    rays = torch.zeros((m, 8), dtype=torch.float32, device="cuda")
    rays[:, 0:3], rays[:, 3], rays[:, 4:7] = pt[si], bihrt.SHADOW_T_LO, L[ki]
    flags = torch.zeros(m, dtype=torch.uint8, device="cuda")
    del tri, v0, e1, e2, u, v, pt, nrm, rec
    torch.cuda.synchronize()
    res["shadow_rays"] = m
    res["facing_share"] = round(m / max(int(idx.shape[0]) * K, 1), 4)

    def gbuffer():
        r.render_gbuffer_device({"hits": hits.data_ptr()}, frame, stream=s.cuda_stream)

    def trace():
        g.trace_device(rays.data_ptr(), m, flags.data_ptr(), bihrt.QUERY_OCCLUDED, s.cuda_stream)

    def compose():
        gbuffer()
        trace()

    lit = torch.zeros(n, dtype=torch.int64, device="cuda")
    irr = torch.zeros(P, dtype=torch.float32, device="cuda")
    rgba = torch.zeros(P, dtype=torch.int32, device="cuda")

    def direct(ptrs):
        return lambda: r.render_direct_device(ptrs, lights, frame, stream=s.cuda_stream)

    record("compose", timed(compose))
    res["compose_lit_share"] = round(float((flags == 0).float().mean()), 4)
    record("hits", timed(gbuffer))
    record("trace", timed(trace))
    record("lit", timed(direct({"lit": lit.data_ptr()})))
    bitsum = sum(int(((lit >> k) & 1).sum()) for k in range(K))
    res["lit_share"] = round(bitsum / max(m, 1), 4)
    assert int((lit >> K).ne(0).sum()) == 0, "bits above n_lights"
    record("planes", timed(direct({"lit": lit.data_ptr(), "irradiance": irr.data_ptr(), "rgba": rgba.data_ptr()})))
    res["mean_irradiance"] = round(float(irr.mean()), 5)
    for k in ("lit", "planes"):
        res[f"{k}_over_compose"] = round(res[f"{k}_ms"] / res["compose_ms"], 3)
    res["compose_spread_ms"] = round(res["compose_max_ms"] - res["compose_min_ms"], 3)
    res["lit_within_spread"] = bool(res["lit_ms"] <= res["compose_ms"] + res["compose_spread_ms"])
    res["trace_mrays_per_s"] = round(m / res["trace_ms"] / 1e3, 1)
    res["direct_mrays_per_s"] = round(m / max(res["lit_ms"] - res["hits_ms"], 1e-6) / 1e3, 1)
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
