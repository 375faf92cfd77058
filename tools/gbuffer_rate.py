#!/usr/bin/env python3
"""G-buffer render rate (bih_render_gbuffer_device) on the 1M soup at
1920 x 1080 x 4 with the reference camera, HIP events after warm-up, one
process, one stream.  Median and min of --reps runs of

  (a) trace      bih_trace_device(CLOSEST) on the camera's jittered rays
                 materialised in device memory (one per sample, pixel order; the
                 figure leaves out the ray generation that route also needs);
  (b) hits       bih_render_gbuffer_device, `hits` only, every sample walked
                 (PARAM_GBUFFER_MASK = 0);
  (c) hits_mask  as (b) with the frustum bins' hit mask;
  (d) planes     the five pixel planes only, with the mask.

(a)'s jitter is numpy's, (b)-(d)'s the frame's XORWOW draws: the same
distribution, so the hit shares agree to three digits, not bit for bit.
Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bih-gpu-raytracer_amd"))

F32 = np.float32


def camera_rays(cam, w, h, spp, seed):
    """D = ((lower_left + u*horizontal) + v*vertical) - origin in f32 (Camera.cu:18-20)."""
    rng = np.random.default_rng(seed)
    y, x, _ = np.meshgrid(np.arange(h, dtype=F32), np.arange(w, dtype=F32), np.arange(spp), indexing="ij")
    n = w * h * spp
    u = ((x.reshape(n) + rng.uniform(0, 1, n).astype(F32)) / F32(w)).astype(F32)
    v = ((y.reshape(n) + rng.uniform(0, 1, n).astype(F32)) / F32(h)).astype(F32)
    c = np.array(cam.as_list(), F32)
    o, ll, hor, ver = c[0:3], c[3:6], c[6:9], c[9:12]
    d = ((ll[None, :] + u[:, None] * hor[None, :]) + v[:, None] * ver[None, :]) - o[None, :]
    return np.broadcast_to(o, (n, 3)), d.astype(F32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    import bihrt
    assert bihrt.device_count() > 0, "no HIP device"
    w, h, spp = a.width, a.height, 4
    P, n = w * h, w * h * spp
    s = torch.cuda.Stream()
    tris = bihrt.scenes.soup(a.tris, seed=1)
    d_soup = torch.from_numpy(tris).cuda()
    torch.cuda.synchronize()
    g = bihrt.GPUArrayManager.from_device(d_soup.data_ptr(), tris.shape[0], stream=s.cuda_stream)
    cam = bihrt.camera_reference(w, h)
    r = bihrt.Renderer(g, w, h, spp=spp, camera=cam)

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

    res = {"tool": "gbuffer_rate", "tris": int(tris.shape[0]), "image": [w, h, spp], "rays": n,
           "warmup": a.warmup, "reps": a.reps}

    def record(label, t):
        res[f"{label}_ms"], res[f"{label}_min_ms"], res[f"{label}_max_ms"] = (round(x, 3) for x in t)

    o, d = camera_rays(cam, w, h, spp, 7)
    rays = torch.from_numpy(bihrt.pack_rays(o, d, 0.0).view(np.uint8)).cuda()
    hits = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    record("trace", timed(lambda: g.trace_device(rays.data_ptr(), n, hits.data_ptr(), bihrt.QUERY_CLOSEST, s.cuda_stream)))
    res["trace_hit_share"] = round(float((hits.cpu().numpy().view(bihrt.HIT_DTYPE)["prim"] != bihrt.NO_HIT).mean()), 4)
    del rays
    frame = [0]

    def gbuffer(ptrs):
        def launch():
            r.render_gbuffer_device(ptrs, frame[0], stream=s.cuda_stream)
            frame[0] += 1
        return launch

    hits.zero_()
    g.set_param(bihrt.PARAM_GBUFFER_MASK, 0)
    record("hits", timed(gbuffer({"hits": hits.data_ptr()})))
    prim = hits.cpu().numpy().view(bihrt.HIT_DTYPE)["prim"].copy()
    res["hits_hit_share"] = round(float((prim != bihrt.NO_HIT).mean()), 4)
    last = frame[0] - 1
    g.set_param(bihrt.PARAM_GBUFFER_MASK, 1)
    record("hits_mask", timed(gbuffer({"hits": hits.data_ptr()})))
    # the mask changes no record: the last unmasked frame once more
    r.render_gbuffer_device({"hits": hits.data_ptr()}, last, stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(hits.cpu().numpy().view(bihrt.HIT_DTYPE)["prim"], prim), "the mask changed a record"
    planes = {k: torch.zeros(P * sz, dtype=torch.uint8, device="cuda")
              for k, sz in (("depth", 4), ("prim", 4), ("bary", 8), ("normal", 12), ("coverage", 4))}
    record("planes", timed(gbuffer({k: t.data_ptr() for k, t in planes.items()})))
    res["planes_covered_share"] = round(float((planes["coverage"].cpu().numpy().view(np.uint32) > 0).mean()), 4)
    for k in ("hits", "hits_mask", "planes"):
        res[f"{k}_over_trace"] = round(res[f"{k}_ms"] / res["trace_ms"], 3)
    res["trace_spread_ms"] = round(res["trace_max_ms"] - res["trace_min_ms"], 3)
    res["hits_within_bar"] = bool(res["hits_ms"] <= res["trace_ms"] + res["trace_spread_ms"])
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
