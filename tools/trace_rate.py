#!/usr/bin/env python3
"""Ray-query rate (bih_trace_device) on the 1M soup, HIP events after warm-up.

Two ray sets of 1920 x 1080 x 4 rays each:
  coherent    the reference camera's rays, one per sample, jittered inside
              their pixel (u = (x + r) / w, r uniform), in pixel order;
  incoherent  the test suite's generator (tests/test_trace.py gen): origins in
              the scene box grown by 1, half of the rays aimed at a random
              triangle, half at a random point of the box.
For comparison the same image through bih_render_device with
BIH_TRAVERSE_REFERENCE (the exhaustive reference walk; spp 4, so the same ray
count), timed the same way in the same process.  Prints one JSON line.
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


def scattered_rays(tris, lo, hi, n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    o = rng.uniform(lo - 1.0, hi + 1.0, (n, 3)).astype(F32)
    tgt = rng.uniform(lo, hi, (n, 3))
    k = rng.integers(0, tris.shape[0], n)
    a = rng.uniform(0, 1, (n, 2))
    s = np.sqrt(a[:, 0])
    T = tris[k[1::2]].astype(np.float64)
    s1, a1 = s[1::2], a[1::2, 1]
    tgt[1::2] = (1 - s1)[:, None] * T[:, 0:3] + (s1 * (1 - a1))[:, None] * T[:, 3:6] + (s1 * a1)[:, None] * T[:, 6:9]
    return o, (tgt.astype(F32) - o).astype(F32)


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
    n = w * h * spp
    s = torch.cuda.Stream()
    tris = bihrt.scenes.soup(a.tris, seed=1)
    d_soup = torch.from_numpy(tris).cuda()
    torch.cuda.synchronize()
    g = bihrt.GPUArrayManager.from_device(d_soup.data_ptr(), tris.shape[0], stream=s.cuda_stream)
    inf = g.info()
    cam = bihrt.camera_reference(w, h)

    def timed(launch):
        """Median / min device ms of `launch` on stream s."""
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
        return float(np.median(ms)), float(min(ms))

    res = {"tool": "trace_rate", "tris": int(tris.shape[0]), "image": [w, h, spp], "rays": n,
           "warmup": a.warmup, "reps": a.reps}
    sets = {"coherent": camera_rays(cam, w, h, spp, 7),
            "incoherent": scattered_rays(tris, np.array(inf.scene_lo[:], F32), np.array(inf.scene_hi[:], F32), n, 11)}
    for name, (o, d) in sets.items():
        rays = torch.from_numpy(bihrt.pack_rays(o, d, 0.0).view(np.uint8)).cuda()
        hits = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        occ = torch.zeros(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for q, out, label in ((bihrt.QUERY_CLOSEST, hits, "closest"), (bihrt.QUERY_OCCLUDED, occ, "occluded")):
            med, lo = timed(lambda: g.trace_device(rays.data_ptr(), n, out.data_ptr(), q, s.cuda_stream))
            res[f"{name}_{label}_ms"] = round(med, 3)
            res[f"{name}_{label}_min_ms"] = round(lo, 3)
            res[f"{name}_{label}_mrays_s"] = round(n / med / 1e3, 1)
        prim = hits.cpu().numpy().view(bihrt.HIT_DTYPE)["prim"]
        res[f"{name}_hit_share"] = round(float((prim != bihrt.NO_HIT).mean()), 4)
        assert np.array_equal(occ.cpu().numpy() != 0, prim != bihrt.NO_HIT), "occlusion flag differs from closest"
        del rays, hits, occ
    # the reference-walk render of the same image (exhaustive walk of every sample)
    r = bihrt.Renderer(g, w, h, spp=spp, camera=cam)
    img = torch.zeros(w * h, dtype=torch.int32, device="cuda")
    frame = [0]

    def render():
        r.render_device(img.data_ptr(), frame[0], traverse=bihrt.TRAVERSE_REFERENCE, stream=s.cuda_stream)
        frame[0] += 1

    med, lo = timed(render)
    res["reference_walk_render_ms"] = round(med, 3)
    res["reference_walk_render_min_ms"] = round(lo, 3)
    res["reference_walk_render_mrays_s"] = round(n / med / 1e3, 1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
