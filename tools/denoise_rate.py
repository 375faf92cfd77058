#!/usr/bin/env python3
"""Denoiser rate (bih_denoise_device) at 1920 x 1080 on the 1M soup and on
cornell, tools/path_rgb_rate.py's setup: the reference camera, 4 spp, five
materials (the last one emissive, triangle i taking material i % 5) on the soup
and the scene's own on cornell, the sky (0.25, 0.3, 0.4), scenes.panels(scene
box) on the soup.  The inputs are one frame's radiance (render_path_spec_device,
--bounces levels) and its depth and normal (render_gbuffer_device).

Calls: HIP events on one stream after warm-up, one process; median, min and max
of --reps runs, the launches alternated run by run: bih_denoise_device (default
sigmas, 5 normal squarings, both outputs) at 1, 3 and 5 passes, and the 1-bounce
colour render (render_path_spec_device, radiance and rgba) as the yardstick:
"share_of_render" is the denoise median over the render's.

Kernels (--kernel-times, the default; --no-kernel-times leaves it out): before
this process touches the GPU, a child of its own runs the 5-pass call --warmup +
--reps times per scene under `rocprofv3 --kernel-trace`, and the durations of
k_denoise_setup and of each k_denoise_pass dispatch (steps 1, 2, 4, 8, 16) are
read from its trace, warm-ups dropped: median, min, max in ms.  Per pass the
model bytes -- 48 read and 16 written per valid pixel, each record once -- over
the median time as a share of the HBM peak (8 TB/s): a lower bound of the
traffic the kernel causes, since its 25 gathers per record plane re-read
through the caches; the bound that holds for the model is the memory one (the
filter's arithmetic is about 25 x 40 f32 operations per pixel).

Prints one JSON line; --out also writes it to a file.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bih-gpu-raytracer_amd"))

ALBEDO5 = [(.73, .71, .68), (.63, .065, .05), (.14, .45, .091), (.3, .5, .9), (.78, .78, .78)]
EMISSION5 = [(0, 0, 0)] * 4 + [(1.7, 1.3, .6)]
SKY3 = (.25, .3, .4)
HBM_PEAK = 8.0e12           # bytes per second
MODEL_BYTES = 48 + 16       # per valid pixel and pass
TRACE_PASSES = 5
SCENES = ("soup", "cornell")


def stats(ms):
    return [round(float(np.median(ms)), 4), round(float(min(ms)), 4), round(float(max(ms)), 4)]


class Frame:
    """One scene's tree, renderer and device planes; the inputs rendered once."""

    def __init__(self, a, name, stream):
        import torch
        import bihrt
        self.torch, self.bihrt, self.s = torch, bihrt, stream
        w, h = a.width, a.height
        P = w * h
        if name == "soup":
            tris = bihrt.scenes.soup(a.tris, seed=1)
            materials = (bihrt.pack_materials([al + em for al, em in zip(ALBEDO5, EMISSION5)]),
                         (np.arange(tris.shape[0]) % 5).astype(np.uint32))
        else:
            tris = bihrt.scenes.cornell()
            materials = bihrt.scenes.cornell_materials()
        self.soup = torch.from_numpy(np.ascontiguousarray(tris)).cuda()
        torch.cuda.synchronize()
        self.g = bihrt.GPUArrayManager.from_device(self.soup.data_ptr(), tris.shape[0], stream=stream.cuda_stream)
        self.g.set_materials(*materials)
        self.r = bihrt.Renderer(self.g, w, h, spp=4, camera=bihrt.camera_reference(w, h))
        info = self.g.info()
        self.panels = bihrt.scenes.panels(info.scene_lo[:], info.scene_hi[:]) if name == "soup" else None
        self.tris = int(tris.shape[0])
        self.rad = torch.zeros(3 * P, dtype=torch.float32, device="cuda")
        self.depth = torch.zeros(P, dtype=torch.float32, device="cuda")
        self.nrm = torch.zeros(3 * P, dtype=torch.float32, device="cuda")
        self.out = torch.zeros(3 * P, dtype=torch.float32, device="cuda")
        self.rgba = torch.zeros(P, dtype=torch.int32, device="cuda")
        self.scratch_rad = torch.zeros(3 * P, dtype=torch.float32, device="cuda")
        self.render(a.bounces, self.rad)
        self.r.render_gbuffer_device({"depth": self.depth.data_ptr(), "normal": self.nrm.data_ptr()}, 1,
                                     stream=stream.cuda_stream)
        stream.synchronize()
        self.valid = int((self.depth < float(np.finfo(np.float32).max)).sum())

    def render(self, bounces, rad):
        self.r.render_path_spec_device({"radiance": rad.data_ptr(), "rgba": self.rgba.data_ptr()}, None, None,
                                       self.panels, SKY3, bounces, 1, stream=self.s.cuda_stream)

    def denoise(self, passes):
        self.r.denoise_device({"radiance": self.out.data_ptr(), "rgba": self.rgba.data_ptr()}, self.rad.data_ptr(),
                              self.depth.data_ptr(), self.nrm.data_ptr(), (passes,), stream=self.s.cuda_stream)

    def close(self):
        self.s.synchronize()
        self.g.close()


def child(a):
    """The traced run: per scene --warmup + --reps calls at TRACE_PASSES passes, nothing else of the denoiser's."""
    import torch
    s = torch.cuda.Stream()
    for name in SCENES:
        f = Frame(a, name, s)
        for _ in range(a.warmup + a.reps):
            f.denoise(TRACE_PASSES)
            s.synchronize()
        f.close()


def parse_trace(path, a):
    """{scene: {"setup_ms": .., "pass_ms": [..]}} from the child's kernel trace (CSV)."""
    rows = [r for r in csv.DictReader(open(path)) if "k_denoise_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per_call, calls = 1 + TRACE_PASSES, a.warmup + a.reps
    assert len(rows) == len(SCENES) * calls * per_call, len(rows)
    out = {}
    for k, name in enumerate(SCENES):
        ms = np.zeros((calls, per_call))
        for c in range(calls):
            for j in range(per_call):
                r = rows[(k * calls + c) * per_call + j]
                assert ("k_denoise_setup" if j == 0 else "k_denoise_pass") in r["Kernel_Name"], r["Kernel_Name"]
                ms[c, j] = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
        ms = ms[a.warmup:]
        out[name] = {"setup_ms": stats(ms[:, 0]), "pass_ms": [stats(ms[:, j]) for j in range(1, per_call)]}
    return out


def kernel_times(a):
    """parse_trace of a child process run under rocprofv3 --kernel-trace."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "-d", d, "-o", "k", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--tris", str(a.tris), "--width", str(a.width),
               "--height", str(a.height), "--warmup", str(a.warmup), "--reps", str(a.reps), "--bounces", str(a.bounces)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=900)
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        assert len(files) == 1, files
        return parse_trace(files[0], a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--bounces", type=int, default=3, help="levels of the frame whose radiance is filtered")
    ap.add_argument("--kernel-times", action=argparse.BooleanOptionalAction, default=True)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    kernels = kernel_times(a) if a.kernel_times else None      # (first: this process has not opened the GPU yet)
    import torch
    import bihrt
    assert bihrt.device_count() > 0, "no HIP device"
    s = torch.cuda.Stream()

    def run(launch):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        launch()
        e1.record(s)
        s.synchronize()
        return e0.elapsed_time(e1)

    def timed(launches):
        """[median, min, max] device ms of each launch on stream s, the launches alternated run by run."""
        for _ in range(a.warmup):
            for launch in launches:
                run(launch)
        ms = [[] for _ in launches]
        for _ in range(a.reps):
            for k, launch in enumerate(launches):
                ms[k].append(run(launch))
        return [stats(m) for m in ms]

    d = bihrt.denoise_params()
    res = {"tool": "denoise_rate", "image": [a.width, a.height, 4], "frame": 1, "input_bounces": a.bounces,
           "sky": list(SKY3), "params": {"normal_squarings": d.normal_squarings, "sigma_colour": d.sigma_colour,
                                          "sigma_plane": round(d.sigma_plane, 6)},
           "warmup": a.warmup, "reps": a.reps, "ms": "median, min, max", "model_bytes_per_valid_pixel_and_pass": MODEL_BYTES,
           "hbm_peak_bytes_per_s": HBM_PEAK, "bound": "memory (model bytes: a lower bound of the traffic)", "scenes": {}}
    for name in SCENES:
        f = Frame(a, name, s)
        t1, t3, t5, tr = timed([lambda: f.denoise(1), lambda: f.denoise(3), lambda: f.denoise(5),
                                lambda: f.render(1, f.scratch_rad)])
        sc = {"tris": f.tris, "pixels": a.width * a.height, "valid_pixels": f.valid,
              "denoise_ms": {"1": t1, "3": t3, "5": t5}, "render_1_bounce_ms": tr,
              "share_of_render": {k: round(t[0] / tr[0], 5) for k, t in (("1", t1), ("3", t3), ("5", t5))}}
        f.denoise(5)
        s.synchronize()
        sc["mean_radiance_in"] = [round(float(x), 5) for x in f.rad.reshape(-1, 3).mean(0)]
        sc["mean_radiance_out"] = [round(float(x), 5) for x in f.out.reshape(-1, 3).mean(0)]
        if kernels is not None:
            sc["kernels_at_5_passes"] = kernels[name]
            sc["pass_share_of_hbm_peak"] = [round(MODEL_BYTES * f.valid / (t[0] * 1e-3) / HBM_PEAK, 4)
                                            for t in kernels[name]["pass_ms"]]
        res["scenes"][name] = sc
        f.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        dd = os.path.dirname(a.out)
        if dd:
            os.makedirs(dd, exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
