"""Presentation-free frame loop.

Mirrors the reference application shell without windowing or GL interop:

  main()            src/Main.cpp:42-66   mesh name -> "resources/<name>/<name>.obj"
  App::LoadModels   src/App.cpp:65-164   -> App.load_models (bih_scene_load_obj +
                                            bih_build, host prep on the device)
  App::Run          src/App.cpp:170-187  -> App.run: per frame Renderer::Render
                                            = rebuild the BIH (Renderer.cpp:422-503)
                                            + cudaRender; prints FPS like
                                            Window::ShowFPS
  presentation      Renderer.cpp:644-670 -> PPM per frame (row 0 at the bottom,
                                            as the GL quad shows it)

usage:  python -m bihrt --mesh sponza --resources path/to/resources --frames 10 \
            --out frames/f%04d.ppm [--width 640 --height 480 --no-rebuild]
            [--gbuffer frames/g%04d.npz]   (depth, prim, bary, normal, coverage per written frame)
            [--direct frames/d%04d.ppm [--sun X,Y,Z] [--sky K]]   (sky- and sun-lit grey preview per written frame)
                     [--lamp X,Y,Z[,W]]...            (point lights next to them; --sky 0: lamps only)
                     [--panel CX,CY,CZ,UX,UY,UZ,VX,VY,VZ[,W]]...   (area lights: soft shadows)
                     [--bounce ALBEDO[,SKY]]          (one bounce of indirect light and a sky term; alone: sky only)
                     [--bounces N]                    (with --bounce: paths of N = 1..8 bounces)
                     [--colour]                       (with --bounces, --scene cornell: its materials, RGB)
                     [--mirror]                       (with --colour: the back wall and the tall block are mirrors)
                     [--denoise [PASSES[,SC[,SP]]]]   (with --colour: the PPM is the a-trous filtered frame)
        python -m bihrt --obj file.obj ...     (explicit path)
        python -m bihrt --scene cornell|torus|soup[:N] ...   (built-in scenes)
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

from . import (DENOISE_DEFAULTS, DENOISE_MAX_PASSES, MAX_BOUNCES, RAYS_PER_PIXEL, SCREEN_HEIGHT, SCREEN_WIDTH, SEED, GPUArrayManager, Renderer,
               load_obj, scenes, write_ppm)


def mesh_path(resources: str, name: str) -> str:
    """Main.cpp:55: resources/<name>/<name>.obj"""
    return os.path.join(resources, name, name + ".obj")


def builtin_scene(spec: str) -> np.ndarray:
    name, _, n = spec.partition(":")
    if name == "cornell":
        return scenes.cornell()
    if name == "torus":
        return scenes.torus()
    if name == "soup":
        return scenes.soup(int(n) if n else 1_000_000, seed=1)
    raise ValueError(f"unknown scene {spec!r} (cornell | torus | soup[:N])")


class App:
    """App (src/App.h): owns the scene arrays and the renderer of one device."""

    def __init__(self, width: int = SCREEN_WIDTH, height: int = SCREEN_HEIGHT,
                 spp: int = RAYS_PER_PIXEL, seed: int = SEED, device: int = 0):
        self.width, self.height, self.spp, self.seed, self.device = width, height, spp, seed, device
        self.arrays = None
        self.renderer = None

    def load_models(self, tris_or_path) -> int:
        """App::LoadModels: flatten the model's triangles (file order), then
        build the BIH on the device.  Returns the triangle count."""
        tris = load_obj(tris_or_path) if isinstance(tris_or_path, str) else tris_or_path
        if tris.shape[0] == 0:
            raise ValueError("scene holds no triangles")
        self.arrays = GPUArrayManager(tris, device=self.device)
        self.renderer = Renderer(self.arrays, self.width, self.height, spp=self.spp, seed=self.seed)
        info = self.arrays.info()
        print(f"Loaded {tris.shape[0]} triangles...", flush=True)
        print("scene bbox lo: [%g, %g, %g]" % tuple(info.scene_lo), flush=True)
        print("scene bbox hi: [%g, %g, %g]" % tuple(info.scene_hi), flush=True)
        return tris.shape[0]

    def run(self, frames: int, out_pattern: str | None = None, rebuild: bool = True,
            every: int = 1, gbuffer_pattern: str | None = None, direct_pattern: str | None = None,
            lights=None, lamps=None, panels=None, bounce=None, bounces=None, materials=None, mirror=False,
            denoise=None):
        """App::Run for a fixed number of frames: Renderer::Render each frame
        (BIH rebuild + render), optional PPM output; returns the frames.
        gbuffer_pattern: one .npz of the frame's G-buffer planes
        (Renderer.render_gbuffer) per written frame.  direct_pattern: one PPM
        of the frame's direct lighting under `lights` (Renderer.render_direct's
        rgba plane) per written frame; lights = None: scenes.sky_dome(8).
        lamps: point lights {pos, weight} next to them (Renderer.render_lights).
        panels: area lights, (k, 10) rows {corner, edge_u, edge_v, weight}, next
        to both (Renderer.render_area_lights).  bounce: (albedo, sky) adds one
        bounce of indirect light and the sky term (Renderer.render_indirect);
        lights = None is then no directional light.  bounces: with bounce,
        paths of that many bounces (Renderer.render_path).  materials: with
        bounces, a (palette, tri_material) pair: colour paths under a sky
        (s, s, s), s = bounce's sky (Renderer.render_path_rgb); bounce's albedo
        is not used.  mirror: with materials, their kinds are honoured
        (Renderer.render_path_spec).  denoise: with materials, the params of
        Renderer.denoise: the PPM is the rgba of the frame's radiance filtered
        under render_gbuffer's depth and normal."""
        assert self.renderer is not None, "load_models first"
        if materials is not None:
            self.arrays.set_materials(*materials)
        if direct_pattern and lights is None and bounce is None:
            lights = scenes.sky_dome(8)
        imgs = []
        last = time.perf_counter()
        for f in range(frames):
            if rebuild and f > 0:
                self.arrays.rebuild()
            img = self.renderer.render(f)
            now = time.perf_counter()
            fps = 1.0 / max(now - last, 1e-9)
            last = now
            print(f"frame {f}: {fps:.1f} FPS (incl. host copy)", flush=True)
            if out_pattern and f % every == 0:
                path = out_pattern % f if "%" in out_pattern else out_pattern
                d = os.path.dirname(path)
                if d:
                    os.makedirs(d, exist_ok=True)
                write_ppm(path, img)
            if gbuffer_pattern and f % every == 0:
                path = gbuffer_pattern % f if "%" in gbuffer_pattern else gbuffer_pattern
                d = os.path.dirname(path)
                if d:
                    os.makedirs(d, exist_ok=True)
                np.savez(path, **self.renderer.render_gbuffer(f))
            if direct_pattern and f % every == 0:
                path = direct_pattern % f if "%" in direct_pattern else direct_pattern
                d = os.path.dirname(path)
                if d:
                    os.makedirs(d, exist_ok=True)
                if bounce is not None and bounces is not None and materials is not None:
                    call = self.renderer.render_path_spec if mirror else self.renderer.render_path_rgb
                    if denoise is not None:
                        rad = call(lights, lamps, panels, (bounce[1],) * 3, bounces, f, planes=("radiance",))["radiance"]
                        gb = self.renderer.render_gbuffer(f, planes=("depth", "normal"))
                        shade = self.renderer.denoise(rad, gb["depth"], gb["normal"], denoise, planes=("rgba",))["rgba"]
                    else:
                        shade = call(lights, lamps, panels, (bounce[1],) * 3, bounces, f, planes=("rgba",))["rgba"]
                elif bounce is not None and bounces is not None:
                    shade = self.renderer.render_path(lights, lamps, panels, bounce, bounces, f,
                                                      planes=("rgba",))["rgba"]
                elif bounce is not None:
                    shade = self.renderer.render_indirect(lights, lamps, panels, bounce, f, planes=("rgba",))["rgba"]
                elif panels is not None and len(panels):
                    shade = self.renderer.render_area_lights(lights, lamps, panels, f, planes=("rgba",))["rgba"]
                elif lamps is not None and len(lamps):
                    shade = self.renderer.render_lights(lights, lamps, f, planes=("rgba",))["rgba"]
                else:
                    shade = self.renderer.render_direct(lights, f, planes=("rgba",))["rgba"]
                write_ppm(path, shade)
            imgs.append(img)
        return imgs


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m bihrt", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--mesh", help="mesh name: <resources>/<name>/<name>.obj (Main.cpp:55)")
    src.add_argument("--obj", help="explicit OBJ path")
    src.add_argument("--scene", help="built-in scene: cornell | torus | soup[:N]")
    ap.add_argument("--resources", default="resources")
    ap.add_argument("--width", type=int, default=SCREEN_WIDTH)
    ap.add_argument("--height", type=int, default=SCREEN_HEIGHT)
    ap.add_argument("--spp", type=int, default=RAYS_PER_PIXEL)
    ap.add_argument("--frames", type=int, default=1)
    ap.add_argument("--out", default=None, help="PPM path; '%%d' formats the frame number")
    ap.add_argument("--gbuffer", default=None, metavar="PATTERN",
                    help=".npz path of the G-buffer planes of each written frame; '%%d' formats the frame number")
    ap.add_argument("--direct", default=None, metavar="PATTERN",
                    help="PPM path of the direct-lighting preview of each written frame; '%%d' formats the frame number")
    ap.add_argument("--sun", default=None, metavar="X,Y,Z", help="--direct: direction towards the sun")
    ap.add_argument("--sky", type=int, default=None, metavar="K", help="--direct: sky directions (default 8; 0: none)")
    ap.add_argument("--lamp", action="append", default=None, metavar="X,Y,Z[,W]",
                    help="--direct: a point light at X,Y,Z of weight W (default 1); repeatable")
    ap.add_argument("--panel", action="append", default=None, metavar="CX,CY,CZ,UX,UY,UZ,VX,VY,VZ[,W]",
                    help="--direct: an area light corner + a*U + b*V of radiance W (default 1) that emits to the "
                         "side cross(U, V) points to; repeatable, up to 16")
    ap.add_argument("--bounce", default=None, metavar="ALBEDO[,SKY]",
                    help="--direct: add one bounce of indirect light of reflectance ALBEDO and a sky of irradiance "
                         "SKY (default 1) for bounce rays that escape; --sky then defaults to 0, and without any "
                         "light the image is the sky term alone (ambient occlusion)")
    ap.add_argument("--bounces", type=int, default=None, metavar="N",
                    help="--direct --bounce: follow each path for N = 1..8 bounces (without it: the one-bounce "
                         "render)")
    ap.add_argument("--colour", action="store_true",
                    help="--direct --bounce --bounces, --scene cornell: a colour path render with the scene's "
                         "built-in materials (red and green walls, the lamp quad emissive) under a sky (SKY, SKY, "
                         "SKY); ALBEDO is not used, and there is no light but the lamp's emission unless --sky K, "
                         "--sun, --lamp or --panel add one")
    ap.add_argument("--mirror", action="store_true",
                    help="--colour: the back wall and the tall block are mirrors (albedo 0.9), which reflect a path "
                         "and gather no light themselves")
    ap.add_argument("--denoise", nargs="?", const="", default=None, metavar="PASSES[,SC[,SP]]",
                    help="--colour: the --direct PPM is the frame's radiance after the edge-avoiding a-trous filter "
                         "(PASSES 1..%d passes, default %d; colour support SC, default %g; tangent-plane support SP "
                         "in scene units, default %g), guided by the frame's G-buffer depth and normal"
                         % ((DENOISE_MAX_PASSES,) + DENOISE_DEFAULTS[:1] + DENOISE_DEFAULTS[2:]))
    ap.add_argument("--every", type=int, default=1, help="write every k-th frame")
    ap.add_argument("--no-rebuild", action="store_true",
                    help="build once (the reference rebuilds every frame)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.colour and a.bounces is None:
        ap.error("--colour belongs to --bounces")
    if a.mirror and not a.colour:
        ap.error("--mirror belongs to --colour")
    denoise = None
    if a.denoise is not None:
        if not a.colour:
            ap.error("--denoise belongs to --colour")
        try:
            v = [float(x) for x in a.denoise.split(",")] if a.denoise else []
        except ValueError:
            v = None
        if v is None or len(v) > 3 or (v and not (v[0] == int(v[0]) and 1 <= v[0] <= DENOISE_MAX_PASSES)):
            ap.error("--denoise takes [PASSES[,SC[,SP]]], PASSES = 1..%d" % DENOISE_MAX_PASSES)
        denoise = (int(v[0]) if v else DENOISE_DEFAULTS[0], DENOISE_DEFAULTS[1],
                   v[1] if len(v) > 1 else DENOISE_DEFAULTS[2], v[2] if len(v) > 2 else DENOISE_DEFAULTS[3])
    if a.colour and a.scene != "cornell":
        ap.error("--colour needs a scene with built-in materials (--scene cornell)")
    if a.mesh:
        path = mesh_path(a.resources, a.mesh)
        if not os.path.exists(path):
            print(f"File doesn't exist: {path}", file=sys.stderr)
            return 2
        scene = path
    elif a.obj:
        scene = a.obj
    else:
        scene = builtin_scene(a.scene)
    lights = None
    lamps = None
    panels = None
    if not a.direct and a.panel:
        ap.error("--panel belongs to --direct")
    if not a.direct and (a.sun is not None or a.sky is not None):
        ap.error("--sun and --sky belong to --direct")
    if not a.direct and a.lamp:
        ap.error("--lamp belongs to --direct")
    if not a.direct and a.bounce is not None:
        ap.error("--bounce belongs to --direct")
    if a.bounces is not None and a.bounce is None:
        ap.error("--bounces belongs to --bounce")
    if a.bounces is not None and not 1 <= a.bounces <= MAX_BOUNCES:
        ap.error("--bounces takes 1..%d" % MAX_BOUNCES)
    bounce = None
    if a.direct:
        if a.bounce is not None:
            try:
                v = [float(x) for x in a.bounce.split(",")]
            except ValueError:
                v = []
            if len(v) not in (1, 2):
                ap.error("--bounce takes ALBEDO[,SKY]")
            bounce = (v[0], v[1] if len(v) == 2 else 1.0)
        a.sky = (8 if bounce is None else 0) if a.sky is None else a.sky
        sun = [float(x) for x in a.sun.split(",")] if a.sun else None
        if sun is not None and len(sun) != 3:
            ap.error("--sun takes X,Y,Z")
        if a.lamp:
            rows = []
            for spec in a.lamp:
                try:
                    v = [float(x) for x in spec.split(",")]
                except ValueError:
                    v = []
                if len(v) not in (3, 4):
                    ap.error("--lamp takes X,Y,Z[,W]")
                rows.append(v + [1.0] if len(v) == 3 else v)
            lamps = np.array(rows, np.float32)
        if a.panel:
            rows = []
            for spec in a.panel:
                try:
                    v = [float(x) for x in spec.split(",")]
                except ValueError:
                    v = []
                if len(v) not in (9, 10):
                    ap.error("--panel takes CX,CY,CZ,UX,UY,UZ,VX,VY,VZ[,W]")
                rows.append(v + [1.0] if len(v) == 9 else v)
            if len(rows) > 16:
                ap.error("--direct takes up to 16 panels")
            panels = np.array(rows, np.float32)
        n_lamps = 0 if lamps is None else lamps.shape[0]
        n_panels = 0 if panels is None else panels.shape[0]
        n_dir = a.sky + (sun is not None)
        if a.sky < 0 or n_dir + n_lamps + n_panels > 64 or (n_dir + n_lamps + n_panels == 0 and bounce is None):
            ap.error("--direct needs 1..64 lights (--sky K, --sun, --lamp, --panel)" if n_lamps or n_panels else
                     "--direct needs 1..64 lights (--sky K, --sun)")
        if a.sky:
            lights = scenes.sky_dome(a.sky, sun)
        elif sun is not None:
            lights = scenes.sky_dome(1, sun)[:1]
        else:
            lights = np.zeros(0, scenes.LIGHT_DTYPE)   # lamps only
    app = App(a.width, a.height, a.spp, device=a.device)
    app.load_models(scene)
    app.run(a.frames, a.out, rebuild=not a.no_rebuild, every=a.every, gbuffer_pattern=a.gbuffer,
            direct_pattern=a.direct, lights=lights, lamps=lamps, panels=panels, bounce=bounce,
            bounces=a.bounces, materials=(scenes.cornell_mirror_materials() if a.mirror else scenes.cornell_materials()) if a.colour
            else None, mirror=a.mirror, denoise=denoise)
    return 0
