"""k_render_bins' per-frame prologue (bins status and list offsets read once,
the jitter's two-word select, the origin-relative slab bounds) against the
oracle, under cameras whose rays start inside the scene and at the shapes
where the prologue takes another path.  Every call is a multi-frame call whose
frames run as one item per tile (one_item_tree), so a frame's XORWOW state is
the one the frame before it left, the Weyl counter steps from frame to frame,
and the hit-cache retest runs within an item as well as across launches.
Plus the root-path check's recurrence restated in numpy, serial and
wave-parallel (no device code implements the parallel form yet).
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import camera_cases as cc
from camera_cases import H, W
from conftest import ROOT
from test_cameras import SEED, diff, oracle_frame, to_camera

F32 = np.float32
# (camera, scene): the four inside cameras on their catalogue scenes, and --
# because a case must send lanes through the path table at both of its sites,
# and the hit-cache retest only runs for tiles whose list has 16 entries --
# on scene "D", the catalogue's soup five times as dense: there inside_z and
# inside_diag reach the retest's path check too (on scene A they do not), and
# mirrored stands in for cornell_in, whose lists are all shorter than 16
INSIDE = (("inside_z", "A"), ("inside_diag", "A"), ("at_edge", "A"), ("cornell_in", "C"))
COVERED = (("at_edge", "A"), ("inside_z", "D"), ("inside_diag", "D"), ("mirrored", "D"))
CASES = INSIDE + COVERED[1:]
FC_LIB = os.path.join(ROOT, "bih-gpu-raytracer_amd", "lib", "variants", "libbih_amd_fc.so")
SCENE_D = (100000, 3)           # soup(n, seed)


@functools.lru_cache(maxsize=None)
def scene(s):
    if s != "D":
        return cc.scene(s)
    from bihrt import scenes
    t = np.ascontiguousarray(scenes.soup(SCENE_D[0], seed=SCENE_D[1]), F32).reshape(-1, 9)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def oracle_tree_d():
    import oracle
    return oracle.OracleTree(scene("D"))


def reference(s, name, w, h, spp, frame):
    """The oracle's frame (shared with test_cameras for the catalogue's scenes)."""
    if s != "D":
        return oracle_frame(s, name, w, h, spp, frame)
    return oracle_tree_d().render(w, h, spp=spp, frame=frame, seed=SEED, cam=cc.camera(name, w, h))[0]


def case_id(c):
    return "%s-%s" % c


def one_item_tree(bihrt, tris):
    """The scene's GPU tree with every frame of a call in one k_render_bins item
    per tile (PARAM_ITEM_TILES = 1).  The default split gives an image this
    small one frame per item, and then no frame's state comes from the frame
    before it: each item steps rng_in to its own first frame."""
    g = bihrt.GPUArrayManager(tris)
    g.set_param(bihrt.PARAM_ITEM_TILES, 1)
    return g


def frames_call(r, first, n, w, h, rows=None):
    """One render_device_frames call of n frames: (n, nrows, w) u32."""
    import torch
    nrows = rows.nrows if rows is not None else h
    buf = torch.full((n * nrows * w,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r.render_device_frames(buf.data_ptr(), first, n, nrows * w, rows=rows)
    r.sync()
    return buf.cpu().numpy().view(np.uint32).reshape(n, nrows, w)


# --- GPU ------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_inside_cameras_multi_frame(case, gpu, bihrt_mod):
    """One call of 5 frames, then one of 3 on the same renderer, each call one
    item per tile (frames 1-4 and 6-7 start from the state and the cached hits
    of the frame before, frame 5 from the hit cache the first call left): all
    8 frames equal the oracle."""
    name, s = case
    g = one_item_tree(bihrt_mod, scene(s))
    r = bihrt_mod.Renderer(g, W, H, seed=SEED, camera=to_camera(bihrt_mod, cc.camera(name)))
    got = np.concatenate([frames_call(r, 0, 5, W, H), frames_call(r, 5, 3, W, H)])
    assert g.bins_stats().usable
    for f in range(8):
        ref = reference(s, name, W, H, 4, f)
        assert np.array_equal(got[f], ref), (name, s, f, diff(got[f], ref))
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [1, 16, 64])
def test_inside_diag_sample_counts(spp, gpu, bihrt_mod):
    """48x32 at 1, 16 and 64 spp, one call of two frames: the shortest and the
    longest draw loops, and the two-word select at every sample index."""
    w, h = 48, 32
    g = one_item_tree(bihrt_mod, cc.scene("A"))
    r = bihrt_mod.Renderer(g, w, h, spp=spp, seed=SEED, camera=to_camera(bihrt_mod, cc.camera("inside_diag", w, h)))
    got = frames_call(r, 0, 2, w, h)
    for f in range(2):
        ref = oracle_frame("A", "inside_diag", w, h, spp, f)
        assert np.array_equal(got[f], ref), (spp, f, diff(got[f], ref))
    g.close()


@pytest.mark.gpu
def test_inside_diag_odd_image(gpu, bihrt_mod):
    """37x29: tiles with lanes outside the image on both edges, two frames."""
    w, h = 37, 29
    g = one_item_tree(bihrt_mod, cc.scene("A"))
    r = bihrt_mod.Renderer(g, w, h, seed=SEED, camera=to_camera(bihrt_mod, cc.camera("inside_diag", w, h)))
    got = frames_call(r, 0, 2, w, h)
    for f in range(2):
        ref = oracle_frame("A", "inside_diag", w, h, 4, f)
        assert np.array_equal(got[f], ref), (f, diff(got[f], ref))
    g.close()


@pytest.mark.gpu
def test_inside_diag_interleaved_bands(gpu, bihrt_mod):
    """Rank 1 of 3's interleaved 8-row bands (first row 8): the jitter and the
    camera ray take the global row, two frames."""
    from bihrt.tiling import band_rows, rows_of_rank
    g = one_item_tree(bihrt_mod, cc.scene("A"))
    r = bihrt_mod.Renderer(g, W, H, seed=SEED, camera=to_camera(bihrt_mod, cc.camera("inside_diag")))
    rows, ys = band_rows(H, 8, 1, 3), rows_of_rank(H, 8, 1, 3)
    assert rows.row0 == 8
    got = frames_call(r, 0, 2, W, H, rows=rows)
    for f in range(2):
        ref = oracle_frame("A", "inside_diag", W, H, 4, f)[ys]
        assert np.array_equal(got[f], ref), (f, diff(got[f], ref))
    g.close()


COUNTER_SCRIPT = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(sys.argv[1], "bih-gpu-raytracer_amd"))
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import torch, bihrt
import camera_cases as cc
w, h = cc.W, cc.H
n_d, seed_d = int(sys.argv[2]), int(sys.argv[3])
for case in sys.argv[4:]:
    name, s = case.split("-")
    tris = cc.scene(s) if s != "D" else np.ascontiguousarray(bihrt.scenes.soup(n_d, seed=seed_d), np.float32).reshape(-1, 9)
    g = bihrt.GPUArrayManager(tris)
    g.set_param(bihrt.PARAM_ITEM_TILES, 1)          # every frame of a call in one item per tile
    r = bihrt.Renderer(g, w, h, seed=1984, camera=bihrt.Camera.from_list(cc.camera(name).tolist()))
    buf = torch.zeros(5 * w * h, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for first, n in ((0, 5), (5, 3)):
        sys.stderr.write("case %s\n" % case)
        sys.stderr.flush()
        r.render_device_frames(buf.data_ptr(), first, n, w * h)
        r.sync()
    g.close()
'''


@pytest.fixture(scope="module")
def counter_build_lines():
    """stderr of the counter build rendering the covered cases (5 + 3 frames
    each) in one child process: {case: [counter lines per launch]}."""
    if not os.path.exists(FC_LIB):
        pytest.skip("no counter build (lib/variants/libbih_amd_fc.so)")
    p = subprocess.run([sys.executable, "-c", COUNTER_SCRIPT, ROOT, str(SCENE_D[0]), str(SCENE_D[1])] +
                       [case_id(c) for c in COVERED], env=dict(os.environ, BIH_LIB=FC_LIB),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    out, cur = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("case "):
            cur = out.setdefault(line.split()[1], [])
        elif cur is not None and line.startswith(("bin-counters", "bin-pathcheck")):
            cur.append(line)
    return out


def _field(line, key):
    return int(re.search(r"(?<![\w-])" + re.escape(key) + r" (\d+)", line).group(1))


@pytest.mark.gpu
@pytest.mark.parametrize("case", COVERED, ids=case_id)
def test_counter_build_plans_agree(case, gpu, counter_build_lines):
    """The counter build recomputes the root-path check for every found lane:
    no plan disagrees with it, over a non-zero number of planned lanes; and the
    case sends lanes through the path table at both of its sites in each of
    its two calls (the first call's retests are all within an item: the cache
    across launches is still empty)."""
    lines = counter_build_lines[case_id(case)]
    cnt = [l for l in lines if l.startswith("bin-counters")]
    pc = [l for l in lines if l.startswith("bin-pathcheck")]
    assert len(cnt) == 2 and len(pc) == 2, lines
    planned = sum(_field(l, "planned") for l in cnt)
    bad = sum(_field(l, "plan-disagrees") for l in cnt)
    sites = [sum(int(re.search(site + r"-site tile-frames (\d+) lanes (\d+)", l).group(2)) for l in pc)
             for site in ("cache", "walk")]
    print(f"{case_id(case)}: planned {planned} plan-disagrees {bad} path-table lanes cache-site {sites[0]} "
          f"walk-site {sites[1]}")
    per_call = [[int(re.search(site + r"-site tile-frames (\d+) lanes (\d+)", l).group(2)) for l in pc]
                for site in ("cache", "walk")]
    print(f"{case_id(case)}: per call cache-site {per_call[0]} walk-site {per_call[1]}")
    assert bad == 0 and planned > 0, (case, planned, bad)
    assert all(n > 0 for site in per_call for n in site), (case, per_call)


# --- CPU ------------------------------------------------------------------------

def _t_and_flags(val, meta, inv3):
    """Per step: t, use_hi, right, neg, end, never -- path_step_flat's terms."""
    axis = meta & 3
    inv = np.take_along_axis(inv3, np.minimum(axis, 2), axis=1)     # sel3: axis 3 selects z
    with np.errstate(all="ignore"):
        t = (val.view(F32) * inv).astype(F32)
    neg = F32(0) > inv
    right = (meta & 4) != 0
    return t, neg != right, right, neg, (meta & 8) != 0, (meta & 16) != 0


def path_serial(val, meta, inv3, tmin, tmax):
    """path_verify as the kernel runs it: 32 x path_step_flat per lane."""
    t, use_hi, right, neg, end, never = _t_and_flags(val, meta, inv3)
    lo, hi = tmin.copy(), tmax.copy()
    live = np.ones(len(val), bool)
    ok = np.zeros(len(val), bool)
    stop = np.full(len(val), 32)
    for j in range(32):
        with np.errstate(invalid="ignore"):
            gt = t[:, j] > np.where(use_hi[:, j], hi, lo)
        g = np.where(right[:, j], ~gt, gt) != neg[:, j]
        ok |= live & end[:, j] & ~never[:, j]
        nxt = live & ~end[:, j] & g
        stop = np.where(live & ~nxt, j, stop)
        live = nxt
        lo = np.where(live & use_hi[:, j], t[:, j], lo)
        hi = np.where(live & ~use_hi[:, j], t[:, j], hi)
    return ok, stop


def path_parallel(val, meta, inv3, tmin, tmax):
    """The wave-parallel rule: step j compares its t against the t of the most
    recent earlier step whose use_hi differs (tMax / tMin when there is none);
    the lowest step that does not pass decides."""
    t, use_hi, right, neg, end, never = _t_and_flags(val, meta, inv3)
    j = np.arange(32)
    last = {}
    for side in (False, True):       # most recent i < j with use_hi[i] == side, or -1
        idx = np.maximum.accumulate(np.where(use_hi == side, j, -1), axis=1)
        last[side] = np.concatenate([np.full((len(val), 1), -1), idx[:, :-1]], axis=1)
    src = np.where(use_hi, last[False], last[True])
    bound = np.where(src >= 0, np.take_along_axis(t, np.maximum(src, 0), axis=1),
                     np.where(use_hi, tmax[:, None], tmin[:, None]))
    with np.errstate(invalid="ignore"):
        gt = t > bound
    g = np.where(right, ~gt, gt) != neg
    fail = ~(~end & g)
    s = np.where(fail.any(axis=1), fail.argmax(axis=1), 32)
    sc = np.minimum(s, 31)
    ok = (s < 32) & end[np.arange(len(val)), sc] & ~never[np.arange(len(val)), sc]
    return ok, s


def _random_tables(rng, n):
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 2.5, -0.375, 1e-30, -3e30], F32)
    inv3 = np.where(rng.random((n, 3)) < 0.5, rng.choice(special, (n, 3)),
                    rng.standard_normal((n, 3)).astype(F32) * F32(4)).astype(F32)
    val = np.where(rng.random((n, 32)) < 0.1, rng.choice(special, (n, 32)),
                   rng.standard_normal((n, 32)).astype(F32)).astype(F32).view(np.uint32)
    tmin = np.where(rng.random(n) < 0.1, rng.choice(special, n), -np.abs(rng.standard_normal(n))).astype(F32)
    tmax = np.where(rng.random(n) < 0.1, rng.choice(special, n), np.abs(rng.standard_normal(n)) * 3).astype(F32)
    meta = (rng.integers(0, 4, (n, 32)) | (rng.integers(0, 2, (n, 32)) << 2)).astype(np.uint32)
    meta |= np.where(rng.random((n, 32)) < 0.05, 8 | (rng.integers(0, 2, (n, 32)) << 4), 0).astype(np.uint32)
    return val, meta, inv3, tmin, tmax


def _crafted_tables(rng, n):
    """A prefix of P steps that pass whatever their side (P covers 0..32), then
    an end (with or without bit 16) or a step that fails; the rest random.
    Inverse directions are powers of two of both signs, so val * inv is exact:
    use_hi steps get t in (0, 0.4), the others t in (0.6, 1), [tMin, tMax] =
    [-1, 2]; the failing step takes t = 3 (use_hi) or -2."""
    val, meta, _, _, _ = _random_tables(rng, n)
    inv3 = rng.choice(np.array([2.0, -0.5, 1.0, -4.0], F32), (n, 3))
    tmin, tmax = np.full(n, -1, F32), np.full(n, 2, F32)
    P = np.concatenate([np.tile(np.array([0, 23, 24, 31, 32]), 64), rng.integers(0, 33, n - 320)])
    kind = rng.integers(0, 3, n)                       # at step P: 0 end, 1 end | 16, 2 fail
    j = np.arange(32)[None, :]
    axis = rng.integers(0, 3, (n, 32))
    right = rng.integers(0, 2, (n, 32)).astype(bool)
    inv = np.take_along_axis(inv3, axis, axis=1)
    use_hi = (inv < 0) != right
    t = np.where(use_hi, rng.uniform(0.05, 0.4, (n, 32)), rng.uniform(0.6, 0.95, (n, 32))).astype(F32)
    t = np.where((j == P[:, None]) & (kind[:, None] == 2), np.where(use_hi, 3, -2), t).astype(F32)
    crafted = j <= P[:, None]
    m = (axis | (right << 2)).astype(np.uint32)
    m |= np.where((j == P[:, None]) & (kind[:, None] < 2), 8 | (kind[:, None] << 4), 0).astype(np.uint32)
    meta = np.where(crafted, m, meta)
    val = np.where(crafted, (t / inv).astype(F32).view(np.uint32), val)
    return val, meta, inv3.astype(F32), tmin, tmax


def test_path_check_serial_equals_parallel():
    """The root-path check on 1.3 * 10^5 random 32-step tables, as the serial
    path_step_flat chain (what k_render_bins runs per lane) and as the
    wave-parallel rule: equal verdicts and equal deciding steps.  The tables
    hold negative, zero, infinite and NaN inverse directions, paths ending at
    steps 1, 24, 25 and 32 with and without bit 16, and paths that stop at
    every position."""
    rng = np.random.default_rng(11)
    parts = [_random_tables(rng, 65536), _crafted_tables(rng, 65536)]
    val, meta, inv3, tmin, tmax = (np.concatenate(x) for x in zip(*parts))
    assert len(val) >= 100000
    ok_s, stop_s = path_serial(val, meta, inv3, tmin, tmax)
    ok_p, stop_p = path_parallel(val, meta, inv3, tmin, tmax)
    assert np.array_equal(stop_s, stop_p), int((stop_s != stop_p).sum())
    assert np.array_equal(ok_s, ok_p), int((ok_s != ok_p).sum())
    # what the tables cover
    for x in (inv3 < 0, inv3 == 0, np.isinf(inv3), np.isnan(inv3)):
        assert x.any()
    assert set(np.unique(stop_s)) == set(range(33))          # every position, and paths that never stop
    rows = np.arange(len(val))
    for step in (1, 24, 25, 32):
        at = stop_s == step - 1
        m = meta[rows, np.minimum(stop_s, 31)]
        for never in (0, 16):
            hit = at & ((m & 8) != 0) & ((m & 16) == never)
            assert hit.any(), (step, never)
            assert (ok_s[hit] == (never == 0)).all()
    assert ok_s.any() and (~ok_s).any()
