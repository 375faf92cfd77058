#!/usr/bin/env python3
"""Mirror-path rate (bih_render_path_spec_device: 1 .. --bounces levels) on
the 1M soup at 1920 x 1080 x 4 with the reference camera under
scenes.panels(scene box): tools/path_rgb_rate.py's setup -- five materials (the
last one emissive), triangle i taking material i % 5, the sky (0.25, 0.3,
0.4).  HIP events after warm-up, one process, one stream; median, min and max
of --reps runs of one and the same frame.

Per n_bounces = 1 .. --bounces four calls are alternated run by run on one
tree, all five planes each:
  spec_diffuse: the mirror call with every kind BIH_MAT_DIFFUSE;
  spec_mirror:  the mirror call with material 2 a mirror (a fifth of the soup);
  colour:       bih_render_path_rgb_device, the yardstick of the machinery's cost;
  grey:         bih_render_path_device at albedo 0.5, sky 0.25.
The palette is switched with bih_tree_set_materials (synchronous, host) before
the timed launch, outside the events.  "spec_minus_colour_ms" is the
difference of the spec_diffuse and colour medians, "spread_ms" the larger max -
min of the two.  Prints one JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bih-gpu-raytracer_amd"))

ALBEDO5 = [(.73, .71, .68), (.63, .065, .05), (.14, .45, .091), (.3, .5, .9), (.78, .78, .78)]
EMISSION5 = [(0, 0, 0)] * 4 + [(1.7, 1.3, .6)]
SKY3 = (.25, .3, .4)


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
    ids = (np.arange(tris.shape[0]) % 5).astype(np.uint32)
    pal = {False: bihrt.pack_materials([al + em for al, em in zip(ALBEDO5, EMISSION5)])}
    pal[True] = pal[False].copy()
    pal[True]["kind"][2] = bihrt.MAT_MIRROR
    g.set_materials(pal[False], ids)
    r = bihrt.Renderer(g, w, h, spp=spp, camera=bihrt.camera_reference(w, h))
    info = g.info()
    panels = bihrt.scenes.panels(info.scene_lo[:], info.scene_hi[:])
    bounce = (a.albedo, a.sky)

    lit = torch.zeros(n, dtype=torch.int64, device="cuda")
    lits = torch.zeros(nb * n, dtype=torch.int64, device="cuda")
    brec = torch.zeros(nb * n * 16, dtype=torch.uint8, device="cuda")
    irr = torch.zeros(P, dtype=torch.float32, device="cuda")
    rad = torch.zeros(3 * P, dtype=torch.float32, device="cuda")
    rgba = torch.zeros(P, dtype=torch.int32, device="cuda")
    five_p = {"lit": lit.data_ptr(), "bounces": brec.data_ptr(), "lits": lits.data_ptr(), "irradiance": irr.data_ptr(),
              "rgba": rgba.data_ptr()}
    five_c = {"lit": lit.data_ptr(), "bounces": brec.data_ptr(), "lits": lits.data_ptr(), "radiance": rad.data_ptr(),
              "rgba": rgba.data_ptr()}

    def grey(k):
        return lambda: r.render_path_device(five_p, None, None, panels, bounce, k, frame, stream=s.cuda_stream)

    def colour(k):
        return lambda: r.render_path_rgb_device(five_c, None, None, panels, SKY3, k, frame, stream=s.cuda_stream)

    def spec(k, mirror):
        def launch():
            r.render_path_spec_device(five_c, None, None, panels, SKY3, k, frame, stream=s.cuda_stream)
        launch.before = lambda: g.set_materials(pal[mirror], ids)     # (synchronous: ends before the events)
        return launch

    def run(launch):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        getattr(launch, "before", lambda: None)()
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
                run(launch)
        ms = [[] for _ in launches]
        for _ in range(a.reps):
            for k, launch in enumerate(launches):
                ms[k].append(run(launch))
        return [stats(m) for m in ms]

    res = {"tool": "path_spec_rate", "tris": int(tris.shape[0]), "image": [w, h, spp], "samples": n,
           "panels": int(panels.shape[0]), "frame": frame, "materials": 5, "mirror_material": 2, "sky": list(SKY3),
           "grey_albedo": a.albedo, "grey_sky": a.sky, "warmup": a.warmup, "reps": a.reps, "bounces": nb,
           "ms": "median, min, max", "spec_diffuse_ms": {}, "spec_mirror_ms": {}, "colour_ms": {}, "grey_ms": {},
           "spec_minus_colour_ms": {}, "spread_ms": {}}
    for k in range(1, nb + 1):
        td, tm, tc, tg = timed(spec(k, False), spec(k, True), colour(k), grey(k))
        res["spec_diffuse_ms"][str(k)], res["spec_mirror_ms"][str(k)] = td, tm
        res["colour_ms"][str(k)], res["grey_ms"][str(k)] = tc, tg
        res["spec_minus_colour_ms"][str(k)] = round(td[0] - tc[0], 3)
        res["spread_ms"][str(k)] = round(max(td[2] - td[1], tc[2] - tc[1]), 3)
    prims = brec.view(torch.int32).reshape(nb, n, 4)[:, :, 3]
    for mirror in (False, True):
        run(spec(nb, mirror))
        key = "mirror" if mirror else "diffuse"
        res["mean_radiance_" + key] = [round(float(x), 5) for x in rad.reshape(P, 3).mean(0)]
        res["live_" + key] = [int((prims[k] != -1).sum()) for k in range(nb)]
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
