"""k_render_bins' item splits and stamped state at small shapes.

A multi-frame k_render_bins launch decides per item which frames of which tile
it renders and which XORWOW state it starts from: the split by the queue's
live count (an item whose range starts at f0 > 0 steps the launch's start state
2 * spp * f0 draws), the heavy tiles' finer split of a cost-ordered queue (the
third launch over one camera and row set), and -- from the fourth render in a
row on one stream -- the per-tile stamp and the two state buffers, which the
item ending at the launch's last frame flips while earlier-range items of the
tile may still have to read the old base.  A wrong stride, pre-step or buffer
choice renders plausible frames with the wrong jitter, so every comparison
here is on bits against the oracle, at frames where an item's range starts or
ends.

The call plans (PLANS) are shared by the GPU tests (the default library, pixels
against the oracle), by a child process running the counter build
(lib/variants/libbih_amd_fc.so; its "bin-items" lines are compared with the
item arithmetic restated below) and by the children that run one A/B
environment knob each.  The same file is the children's script.
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np

if __name__ == "__main__":      # a child process: the tests' own directory, then as conftest sets the paths
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pytest

import camera_cases as cc
from conftest import ROOT
from test_cameras import SEED, cam_of, diff, to_camera

TILE = {1: (8, 8), 2: (8, 4), 4: (4, 4), 8: (4, 2), 16: (2, 2), 32: (2, 1), 64: (1, 1)}   # TileShape
BASE = {64: (96, 64), 16: (192, 128), 4: (320, 208)}        # spp -> image of the base shapes
FULL = 0x00FFFF
LIVE_ITEMS = 16384              # live_items_target (bih_capi.cpp)
ITEM_TILES = 65536              # bih_tree's item_tiles unless PARAM_ITEM_TILES sets it
FC_LIB = os.path.join(ROOT, "bih-gpu-raytracer_amd", "lib", "variants", "libbih_amd_fc.so")
GAP = 64                        # words between the frames of a call's buffer


def ntiles_of(w, h, spp, nrows=None):
    tw, th = TILE[spp]
    return -(-w // tw) * -(-(h if nrows is None else nrows) // th)


# --- scenes -----------------------------------------------------------------------

def _dust(n, seed, u, v, dist, spread, half, thin):
    """n thin triangles around the point that inside_diag sees at (u, v) of its
    image, `dist` from the eye: long lists over few tiles, most rays miss."""
    rng = np.random.default_rng(seed)
    f, rt, up = cc.basis(cc.DIAG_F)
    hh, hw = 0.5, 0.5 * 96 / 64
    centre = np.asarray(cc.DIAG_O, np.float64) + dist * (f + (2 * u - 1) * hw * rt + (2 * v - 1) * hh * up)
    c = centre + rng.uniform(-spread, spread, (n, 3))
    a = rng.uniform(-half, half, (n, 3))
    b = np.cross(a, rng.uniform(-1, 1, (n, 3)))
    b *= (thin * half / np.maximum(np.linalg.norm(b, axis=1), 1e-12))[:, None]
    tri = np.stack([c - a, c + a, c + b], axis=1)
    return tri.reshape(n, 9).astype(np.float32)


HEAVY_DUST = dict(n=24000, seed=7, u=0.22, v=0.27, dist=0.5, spread=0.07, half=0.006, thin=0.08)
SCENE_D = (100000, 3)           # soup(n, seed): test_render_diet's scene D
SCALE_S = 1.5                   # scene S: scene A scaled about its centre


@functools.lru_cache(maxsize=None)
def scene(s):
    """"A" (the catalogue's), "H" (A plus a clump of dust in a corner of
    inside_diag's view: tiles whose cost is many times the mean), "S" (A scaled to
    fill half the outside cameras' view: the other tiles are background), "D" and "D2"
    (two soups of the same triangle count); float32 (n, 9), read-only."""
    from bihrt import scenes
    if s == "A":
        return cc.scene("A")
    if s == "H":
        t = np.concatenate([cc.scene("A"), _dust(**HEAVY_DUST)])
    elif s == "S":
        v = cc.scene("A").astype(np.float64).reshape(-1, 3)
        t = (SCALE_S * (v - v.mean(0)) + v.mean(0)).reshape(-1, 9)
    elif s == "D":
        t = scenes.soup(SCENE_D[0], seed=SCENE_D[1])
    elif s == "D2":
        t = scenes.soup(SCENE_D[0], seed=SCENE_D[1] + 2)
    else:
        raise KeyError(s)
    t = np.ascontiguousarray(t, np.float32).reshape(-1, 9)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def otree(s):
    import oracle
    return oracle.OracleTree(scene(s))


@functools.lru_cache(maxsize=None)
def oracle_frame(s, name, w, h, spp, frame, sub=None):
    """The oracle's image of scene s under camera `name`, rendered once and
    read-only: the whole frame, or (sub = (row0, step)) its rows row0::step."""
    rows = None if sub is None else (sub[0], len(range(sub[0], h, sub[1])), sub[1])
    img = otree(s).render(w, h, spp=spp, frame=frame, seed=SEED, cam=cam_of(name, w, h), rows=rows)[0]
    img.setflags(write=False)
    return img


def oracle_bands(s, name, w, h, spp, frame, band, rank, world):
    """The rows of rank `rank`'s interleaved bands of the oracle's frame, in the
    rank's local order (only those rows are rendered)."""
    assert h % (band * world) == 0
    sub = [oracle_frame(s, name, w, h, spp, frame, (rank * band + i, band * world)) for i in range(band)]
    return np.stack(sub, axis=1).reshape(-1, w)


# --- the item arithmetic, restated ------------------------------------------------

def cdiv(a, b):
    return -(-a // b)


def host_item_split(nframes, ntiles, item_tiles):
    """item_split (bih_capi.cpp): (fpi, nsplit) from the launch's tile count."""
    ns = (item_tiles + ntiles // 2) // ntiles if ntiles else nframes
    ns = max(1, min(ns, nframes))
    fpi = cdiv(nframes, ns)
    return fpi, cdiv(nframes, fpi)


def launch_split(nframes, ntiles, live, cost_ordered, item_tiles=None, live_items=LIVE_ITEMS, normalise=True):
    """(ns, fpi, hs, fhv) of a k_render_bins launch: the host's item_split and
    hsplit rule, replaced by the kernel's live-count rule unless
    PARAM_ITEM_TILES was set (item_tiles) or the target is 0; then hs
    normalised to the heavy items that have a frame (normalise=False: the rule
    before that step)."""
    if nframes > 1:
        fpi, ns = host_item_split(nframes, ntiles, ITEM_TILES if item_tiles is None else item_tiles)
    else:
        fpi, ns = nframes, 1
    heavy = cost_ordered and nframes >= 4
    hs = max(ns, min(nframes, ns * (4 if nframes >= 8 else 2))) if heavy else ns
    if item_tiles is None and live_items and nframes > 1:
        ns = (live_items + live // 2) // live if live else nframes
        ns = max(1, min(ns, nframes))
        fpi = cdiv(nframes, ns)
        ns = cdiv(nframes, fpi)
        hs = max(ns, min(ns * (4 if nframes >= 8 else 2), nframes) if heavy else ns)
    fhv = cdiv(nframes, hs)
    if normalise:
        hs = cdiv(nframes, fhv)
    return ns, fpi, hs, fhv


def band_items(live, hv, ns, hs):
    """BinQueue::band_items without the background items; extra(): no tile is
    heavy when hs == ns."""
    x = hv if hs != ns else 0
    return x * hs + (live - x) * ns


def decode_items(it, live, hv, nframes, ns, fpi, hs, fhv):
    """k_render_bins' decode of the live item indices `it` of a band with
    `live` live tiles, the first hv of them heavy: (tile position, f0, nf)."""
    it = np.asarray(it, np.int64)
    x = np.asarray(hv if hs != ns else 0, np.int64)
    if ns == 1 and not np.any(x):
        return it, np.zeros_like(it), np.full_like(it, nframes)
    hx = x * hs
    heavy = it < hx
    k = it - hx
    tile = np.where(heavy, it // hs, x + k // ns)
    f0 = np.where(heavy, (it % hs) * fhv, (k % ns) * fpi)
    nf = np.minimum(f0 + np.where(heavy, fhv, fpi), nframes)
    return tile, f0, nf


def range_starts(n, step):
    return list(range(0, n, step))


# --- the call plans ---------------------------------------------------------------

def _consecutive(sizes, cam, first=0):
    out, f = [], first
    for n in sizes:
        out.append((f, n, cam, 0))
        f += n
    return out


def _stamped_calls():
    """Calls of 16 frames from frame 0 to 144 (ring, ring, ring, then stamped;
    k_rng_sync due at frame 112) under two cameras -- tiles at the object's
    rim are background under one for several calls and then turn live --, a
    call 3 frames late, 5 frames, one frame on a second stream, two more calls."""
    cams = ["reference"] * 5 + ["moved2"] * 3 + ["reference"]
    calls = [(16 * k, 16, cams[k], 0) for k in range(9)]
    calls += [(147, 16, "reference", 0), (163, 5, "moved2", 0), (168, 1, "moved2", 1),
              (169, 16, "moved2", 0), (185, 16, "reference", 0)]
    return calls


STAMPED_SPECIAL = (3, 7, 9)     # the first stamped call, the first after the sync, the one after the gap


def _plan(s, spp, wh, calls, item_tiles=None, bands=None, top=None):
    """bands: (band, rank, world) of interleaved bands; top: the image's first `top` rows."""
    return dict(scene=s, spp=spp, w=wh[0], h=wh[1], calls=calls, item_tiles=item_tiles, bands=bands, top=top)


# The bins serve a call whose rows start and whose bands end on tile rows
# (render_device_impl's use_bins); a whole frame is one band of h rows, so at
# 67x45 a 4x4-tile render would take the per-frame path and never reach
# k_render_bins.  The 67x45 plans render the image's first 44 rows instead.
TOP_67x45 = 44


PLANS = {
    **{f"live_{spp}": _plan("A", spp, BASE[spp], _consecutive((16, 7, 1), "inside_diag")) for spp in BASE},
    "heavy_64": _plan("H", 64, BASE[64], _consecutive((16, 16, 16, 5, 8, 4, 13, 3), "inside_diag")),
    "heavy_4": _plan("H", 4, (67, 45), _consecutive((16, 16, 16, 5, 8, 4, 13, 3), "inside_diag"), item_tiles=1,
                     top=TOP_67x45),
    "stamped_64": _plan("S", 64, BASE[64], _stamped_calls()),
    "stamped_4": _plan("S", 4, BASE[4], _stamped_calls()),
    "bands_16": _plan("A", 16, BASE[16], _consecutive((16, 16, 16, 7), "inside_diag"), bands=(8, 1, 2)),
    "knobs_64": _plan("A", 64, BASE[64], _consecutive((16, 16, 16, 16, 7), "inside_diag")),
}
# live tiles of scene S's queues, from the counter build's "bin-items" lines
# (test_counter_build_item_lines asserts the splits they give): the GPU tests
# take the range starts of the stamped plans from them
S_LIVE = {("stamped_64", "reference"): 4087, ("stamped_64", "moved2"): 3703,
          ("stamped_4", "reference"): 2697, ("stamped_4", "moved2"): 2455}


def plan_rows(p):
    """(bih_rows or None, the global rows of its local rows, local row count)."""
    if p["top"] is not None:
        from bihrt import Rows
        return Rows(0, p["top"], p["top"], 1), np.arange(p["top"]), p["top"]
    if p["bands"] is None:
        return None, np.arange(p["h"]), p["h"]
    from bihrt.tiling import band_rows, rows_of_rank
    ys = rows_of_rank(p["h"], *p["bands"])
    return band_rows(p["h"], *p["bands"]), ys, len(ys)


def plan_live(name, cam):
    p = PLANS[name]
    if p["scene"] == "S":
        return S_LIVE[name, cam]
    return ntiles_of(p["w"], p["h"], p["spp"], plan_rows(p)[2])     # a global list: every tile live


def plan_splits(name, live_items=LIVE_ITEMS):
    """Per call of the plan: (ns, fpi, hs, fhv, cost_ordered, measuring) as
    launch_split predicts them: a camera's first launch over these rows orders
    the queue by list length, its second measures, from the third on the
    queue is cost-ordered."""
    p = PLANS[name]
    nt = ntiles_of(p["w"], p["h"], p["spp"], plan_rows(p)[2])
    uses, out = {}, []
    for _, n, cam, _ in p["calls"]:
        u = uses.get(cam, 0)
        uses[cam] = u + 1
        out.append(launch_split(n, nt, plan_live(name, cam), u >= 2, p["item_tiles"], live_items) + (u >= 2, u == 1))
    return out


def compared_frames(name):
    """Per call of the plan {frame of the call: None (all rows) or (row0, step)}:
    what the GPU test of the plan compares with the oracle."""
    p, splits = PLANS[name], plan_splits(name)
    out = []
    for k, ((_, n, _, _), (ns, fpi, hs, fhv, cost, _)) in enumerate(zip(p["calls"], splits)):
        starts = range_starts(n, fpi)
        ends = [f - 1 for f in starts if f > 0]
        cmp = {0: None, n - 1: None}
        if name.startswith(("live", "bands", "knobs")):
            # call 1 (and the bands' cost-ordered call 3): every range start and end; else the starts
            for f in starts + (ends if k in (0, 2) else []):
                cmp[f] = None
        elif name.startswith("heavy"):
            if k >= 2:
                for j, f in enumerate(range_starts(n, fhv)):
                    cmp.setdefault(f, None if p["spp"] == 4 else ((j + k) % 3, 3))
        else:
            if k in STAMPED_SPECIAL or n < 16:
                for f in starts:
                    cmp[f] = None
            else:
                cmp = {0: (k % 3, 3), n - 1: ((k + 1) % 3, 3), starts[len(starts) // 2]: ((k + 2) % 3, 3)}
                if p["calls"][k - 1][3]:
                    cmp[0] = None               # the frame after the one on the second stream
        out.append(cmp)
    return out


# --- CPU ------------------------------------------------------------------------

@pytest.mark.parametrize("spp", list(BASE))
def test_guard(spp, oracle_mod):
    """What keeps the GPU tests from being vacuous, by the oracle alone: each
    frame test_live_count_split compares at a range start (f0 > 0) differs
    from the frames before and after it on at least 5 % of the pixels -- a
    state stepped one frame too few or too many shows -- and its hit share is
    within [0.10, 0.90].  And a row subset is the whole frame's rows."""
    name = f"live_{spp}"
    p, w, h = PLANS[name], *BASE[spp]
    assert plan_live(name, "inside_diag") == {64: 6144, 16: 6144, 4: 4160}[spp]
    splits = plan_splits(name)
    assert [s[:2] for s in splits] == {64: [(3, 6), (3, 3), (1, 1)], 16: [(3, 6), (3, 3), (1, 1)],
                                       4: [(4, 4), (4, 2), (1, 1)]}[spp]
    checked = 0
    for (first, n, cam, _), (ns, fpi, *_rest) in zip(p["calls"], splits):
        for f0 in range_starts(n, fpi)[1:]:
            f = first + f0
            img = oracle_frame("A", cam, w, h, spp, f)
            share = cc.hit_share(img)
            partial = float(((img != cc.BACKGROUND) & (img != FULL)).mean())
            d = [float((img != oracle_frame("A", cam, w, h, spp, g)).mean()) for g in (f - 1, f + 1)]
            print(f"spp {spp} {w}x{h} frame {f}: hit share {share:.3f}, partially covered {partial:.3f}, "
                  f"differs from frame {f - 1} on {d[0]:.3f}, from {f + 1} on {d[1]:.3f}")
            assert 0.10 <= share <= 0.90, (f, share)
            assert min(d) >= 0.05, (f, d)
            checked += 1
    assert checked >= 4
    sub = oracle_frame("A", "inside_diag", w, h, spp, 6, (1, 3))
    assert np.array_equal(sub, oracle_frame("A", "inside_diag", w, h, spp, 6)[1::3])


def test_heavy_and_stamped_scene_guard(oracle_mod):
    """Scene H's dust covers a corner of inside_diag's view and leaves a varied
    image there; scene S leaves background and object under both cameras of the
    stamped plans, and pixels that are background under one camera show the
    object under the other."""
    w, h = BASE[64]
    a, hv = oracle_frame("A", "inside_diag", w, h, 64, 32), oracle_frame("H", "inside_diag", w, h, 64, 32)
    changed = a != hv
    ys, xs = np.nonzero(changed)
    print(f"scene H: dust changes {changed.mean():.3f} of the pixels, rows {ys.min()}..{ys.max()}, "
          f"columns {xs.min()}..{xs.max()}")
    assert 0.01 <= changed.mean() <= 0.25
    assert ys.max() < h // 2 + 8 and xs.max() < w // 2 + 8           # a corner: most tiles keep their cost
    imgs = {c: oracle_frame("S", c, w, h, 64, 0) for c in ("reference", "moved2")}
    for c, img in imgs.items():
        share = cc.hit_share(img)
        print(f"scene S under {c}: hit share {share:.3f}")
        assert 0.15 <= share <= 0.85, (c, share)
    bg = [img == cc.BACKGROUND for img in imgs.values()]
    assert (bg[0] & ~bg[1]).mean() >= 0.02 and (bg[1] & ~bg[0]).mean() >= 0.02


def test_plans_reach_the_bins_and_split(bihrt_mod):
    """Every plan's rows pass the rule that admits a call to k_render_bins
    (rows start and bands end on tile rows), and the splits the GPU tests
    take their compared frames from are the intended ones: intermediate at
    the base shapes and in the stamped plans, heavy items from the third call
    of the heavy plans on (not in the call of 3 frames)."""
    for name, p in PLANS.items():
        rows, ys, nrows = plan_rows(p)
        th = TILE[p["spp"]][1]
        row0, band_h = (rows.row0, rows.band_h) if rows is not None else (0, p["h"])
        assert row0 % th == 0 and band_h % th == 0, name
        assert len(ys) == nrows and ys.max() < p["h"] and len(compared_frames(name)) == len(p["calls"])
    for spp in BASE:
        assert 1 < plan_splits(f"live_{spp}")[0][1] < 16
    for name in ("stamped_64", "stamped_4"):
        assert all(1 < s[1] < 16 for s in plan_splits(name)[:10]), name
    for name in ("heavy_64", "heavy_4"):
        assert [s[2] > s[0] for s in plan_splits(name)] == [False, False, True, True, True, True, True, False]
    assert [s[:4] for s in plan_splits("heavy_64")[2:7]] == [(3, 6, 8, 2), (3, 2, 5, 1), (3, 3, 8, 1), (2, 2, 4, 1),
                                                             (3, 5, 7, 2)]
    assert [s[:4] for s in plan_splits("heavy_4")[2:7]] == [(1, 16, 4, 4), (1, 5, 2, 3), (1, 8, 4, 2), (1, 4, 2, 2),
                                                            (1, 13, 4, 4)]


def test_item_arithmetic():
    """The host's item_split and hsplit rule and the kernel's live-count rule
    with hs normalised, for every nframes in 1..16, the live counts below, with
    and without a cost-ordered queue and PARAM_ITEM_TILES: the decoded items
    (tile, f0, nf) cover every (live tile, frame) exactly once, none is empty,
    and their number is band_items.  Every heavy count 0..live is decoded in
    full for live <= 500; for the larger counts the items on both sides of the
    heavy / light boundary for every heavy count, and the full decode for a
    spread of them (the decode depends on the count only through that
    boundary).  Without the normalisation the same rule leaves empty items."""
    lives = (1, 500, 1100, 1536, 4160, 6144, 11000, 24000)
    rng = np.random.default_rng(3)
    empty_before, done = 0, set()
    for live in lives:
        for nframes in range(1, 17):
            for item_tiles in (None, 1, 2 * live, 5 * live):
                for cost in (False, True):
                    ns, fpi, hs, fhv = launch_split(nframes, live, live, cost, item_tiles)
                    assert 1 <= ns <= hs <= nframes and fpi * (ns - 1) < nframes <= fpi * ns
                    assert fhv * (hs - 1) < nframes <= fhv * hs and fhv <= fpi
                    if not cost or nframes < 4:
                        assert hs == ns
                    raw = launch_split(nframes, live, live, cost, item_tiles, normalise=False)
                    assert raw[:2] == (ns, fpi) and raw[3] == fhv and raw[2] >= hs
                    empty_before += raw[2] - hs
                    if (live, nframes, ns, fpi, hs, fhv) in done:
                        continue
                    done.add((live, nframes, ns, fpi, hs, fhv))
                    if live <= 500:
                        hvs = np.arange(live + 1)
                    else:
                        hvs = np.unique(np.concatenate([[0, 1, live // 2, live - 1, live],
                                                        rng.integers(0, live + 1, 2)]))
                        # both sides of the boundary, and the last item, for every heavy count
                        hv = np.arange(live + 1)
                        x = hv if hs != ns else np.zeros_like(hv)
                        n_items = x * hs + (live - x) * ns
                        for it, ok in ((x * hs - 1, x > 0), (x * hs, x < live), (n_items - 1, hv >= 0)):
                            t, f0, nf = decode_items(np.where(ok, it, 0), live, hv, nframes, ns, fpi, hs, fhv)
                            assert ((f0 < nf) & (nf <= nframes) & (t >= 0) & (t < live))[ok].all()
                        t, f0, nf = decode_items(n_items - 1, live, hv, nframes, ns, fpi, hs, fhv)
                        assert (t == live - 1).all() and (nf == nframes).all()
                    for hv in hvs:
                        n_items = band_items(live, int(hv), ns, hs)
                        t, f0, nf = decode_items(np.arange(n_items), live, int(hv), nframes, ns, fpi, hs, fhv)
                        assert (f0 < nf).all() and (nf <= nframes).all(), (live, nframes, item_tiles, cost, hv)
                        m = live * nframes + 1
                        cover = np.bincount(t * nframes + f0, minlength=m) - np.bincount(t * nframes + nf, minlength=m)
                        assert (np.cumsum(cover)[:-1] == 1).all(), (live, nframes, item_tiles, cost, hv)
                        assert int((nf - f0).sum()) == live * nframes
    # 16 frames over ~6k live tiles, cost-ordered: ns 3, hs 12 -> 8, fhv 2 (four empty items per heavy tile before)
    assert launch_split(16, 6144, 6144, True) == (3, 6, 8, 2)
    assert launch_split(16, 6144, 6144, True, normalise=False) == (3, 6, 12, 2)
    assert launch_split(9, 204, 204, True, 1, normalise=False) == (1, 9, 4, 3)       # host rule: frames 9.. empty
    assert launch_split(9, 204, 204, True, 1) == (1, 9, 3, 3)
    # the headline call shapes keep their items
    assert launch_split(16, 32400, 24000, True) == (1, 16, 4, 4) and launch_split(4, 32400, 24000, True) == (1, 4, 2, 2)
    assert launch_split(16, 32400, 7300, True) == (2, 8, 8, 2)
    assert empty_before > 0


# --- GPU ------------------------------------------------------------------------

def run_plan(bihrt, name, g=None, sync_each=False, note=None):
    """The plan's calls on one renderer (stream 0: the library's own; others:
    streams of their own), every buffer filled with -1 before the first render:
    per call the frames (n, nrows, w) u32.  The words between the frames stay
    untouched."""
    import torch
    p = PLANS[name]
    w, h, spp = p["w"], p["h"], p["spp"]
    rows, _, nrows = plan_rows(p)
    own = g is None
    if own:
        g = bihrt.GPUArrayManager(scene(p["scene"]))
        if p["item_tiles"] is not None:
            g.set_param(bihrt.PARAM_ITEM_TILES, p["item_tiles"])
    P = nrows * w
    stride = P + GAP
    bufs = [torch.full((n * stride,), -1, dtype=torch.int32, device="cuda") for _, n, _, _ in p["calls"]]
    streams = {k: torch.cuda.Stream() for k in sorted({c[3] for c in p["calls"]} - {0})}
    torch.cuda.synchronize()
    r = bihrt.Renderer(g, w, h, spp=spp, seed=SEED)
    for k, ((first, n, cam, sk), buf) in enumerate(zip(p["calls"], bufs)):
        if note:
            note(name, k)
        r.camera = to_camera(bihrt, cam_of(cam, w, h))
        st = streams[sk].cuda_stream if sk else None
        if n == 1:
            r.render_device(buf.data_ptr(), first, rows=rows, stream=st)
        else:
            r.render_device_frames(buf.data_ptr(), first, n, stride, rows=rows, stream=st)
        if sk:
            streams[sk].synchronize()
        if sync_each:
            r.sync()
    r.sync()
    torch.cuda.synchronize()
    assert g.bins_stats().usable
    out = []
    for k, ((_, n, _, _), buf) in enumerate(zip(p["calls"], bufs)):
        b = buf.cpu().numpy().view(np.uint32).reshape(n, stride)
        assert (b[:, P:] == 0xFFFFFFFF).all(), (name, k, "stride gap written")
        out.append(b[:, :P].reshape(n, nrows, w))
    if own:
        g.close()
    return out


def check_plan(name, frames):
    """The plan's compared frames against the oracle, on bits."""
    p = PLANS[name]
    _, ys, _ = plan_rows(p)
    checked = 0
    for k, ((first, n, cam, _), cmp) in enumerate(zip(p["calls"], compared_frames(name))):
        for j, sub in sorted(cmp.items()):
            if sub is None and p["bands"] is not None:
                got, ref = frames[k][j], oracle_bands(p["scene"], cam, p["w"], p["h"], p["spp"], first + j, *p["bands"])
            elif sub is None:
                got, ref = frames[k][j], oracle_frame(p["scene"], cam, p["w"], p["h"], p["spp"], first + j)[ys]
            else:
                assert p["bands"] is None
                got = frames[k][j][sub[0]::sub[1]]
                ref = oracle_frame(p["scene"], cam, p["w"], p["h"], p["spp"], first + j, sub)
            assert np.array_equal(got, ref), (name, "call", k, "frame", first + j, "of the call", j, diff(got, ref))
            checked += 1
    return checked


@pytest.mark.gpu
@pytest.mark.parametrize("spp", list(BASE))
def test_live_count_split(spp, gpu, bihrt_mod):
    """The kernel's split by the live count (ns 3, fpi 6 resp. ns 4, fpi 4): a
    call of 16 frames, every frame that starts or ends an item's range; a call
    of 7 with the sequence continuing, its first and last frame and its range
    starts; then a single frame."""
    name = f"live_{spp}"
    assert 1 < plan_splits(name)[0][1] < 16
    assert check_plan(name, run_plan(bihrt_mod, name)) >= 9


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["heavy_64", "heavy_4"])
def test_heavy_tiles_split(name, gpu, bihrt_mod):
    """Calls of 16, 16, 16, 5, 8, 4, 13 and 3 frames over scene H: from the
    third on the queue is cost-ordered and the dust's tiles take hs items of
    fhv frames (test_counter_build_item_lines asserts that tiles were heavy);
    the first and last frame and every heavy-range start of calls 3 to 8.  At
    64 spp the kernel's rule, at 4 spp (67x45's first 44 rows,
    PARAM_ITEM_TILES = 1) the host's: other tiles one item, heavy tiles min(nframes, 4)."""
    splits = plan_splits(name)
    assert [s[2] > s[0] for s in splits] == [False, False, True, True, True, True, True, False]
    assert check_plan(name, run_plan(bihrt_mod, name)) >= 26


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [64, 4])
def test_stamped_split_sequence(spp, gpu, bihrt_mod):
    """Stamped launches whose tiles have several multi-frame items: nine calls
    of 16 frames (stamped from the fourth; k_rng_sync before the eighth) under
    two cameras, a call 3 frames late, 5 frames, a frame on a second stream
    (back to the ring), two more calls.  In every call the first and last
    frame and a range start; every range start of the first stamped call, the
    call after the sync, the one after the gap and the short calls."""
    name = f"stamped_{spp}"
    assert all(1 < s[1] < 16 for s in plan_splits(name)[:9])
    assert check_plan(name, run_plan(bihrt_mod, name)) >= 40


@pytest.mark.gpu
def test_bands_split(gpu, bihrt_mod):
    """Rank 1 of 2's interleaved 8-row bands at 16 spp (3072 live tiles: items
    of 4 frames), three calls of 16 and one of 7, against the oracle's rows."""
    p = PLANS["bands_16"]
    rows, ys, nrows = plan_rows(p)
    assert rows.row0 == 8 and nrows == 64 and plan_splits("bands_16")[0][:2] == (4, 4)
    assert check_plan("bands_16", run_plan(bihrt_mod, "bands_16")) >= 20


def _note(name, k):
    sys.stderr.write(f"plan {name} call {k}\n")
    sys.stderr.flush()


COUNTER_PLANS = [n for n in PLANS if not n.startswith("knobs")]


@pytest.fixture(scope="module")
def counter_lines():
    """stderr of one child process that runs the plans on the counter build,
    syncing after every call: {(plan, call): {line kind: line}}."""
    if not os.path.exists(FC_LIB):
        pytest.skip("no counter build (lib/variants/libbih_amd_fc.so)")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "counters"] + COUNTER_PLANS,
                       env=dict(os.environ, BIH_LIB=FC_LIB), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    out, cur = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("plan "):
            w = line.split()
            cur = out.setdefault((w[1], int(w[3])), {})
        elif cur is not None and line.startswith(("bin-items", "bin-counters")):
            cur[line.split()[0]] = line
    return out


def _field(line, key):
    return int(re.search(r"(?<![\w-])" + re.escape(key) + r" (\d+)", line).group(1))


@pytest.mark.gpu
def test_counter_build_item_lines(gpu, counter_lines):
    """The counter build's "bin-items" line of every launch of the plans: the
    split equals launch_split's from the printed live count, every live tile
    has each frame once (tile-frames = live x nframes), the item count is the
    predicted one, no item is empty, and items start past frame 0 wherever a
    tile has more than one.  Across the plans each route occurs: an
    intermediate split at each base spp, heavy tiles (some, not all) in ring
    and in stamped launches, stamped and measuring launches with split items,
    background tiles in stamped launches; and no plan disagrees with the
    root-path check."""
    seen = []
    for name in COUNTER_PLANS:
        p = PLANS[name]
        nt = ntiles_of(p["w"], p["h"], p["spp"], plan_rows(p)[2])
        for k, ((_, n, cam, _), pred) in enumerate(zip(p["calls"], plan_splits(name))):
            line = counter_lines[name, k]["bin-items"]
            print(name, k, cam, line)
            f = {key: _field(line, key) for key in
                 ("nframes", "ns", "fpi", "hs", "fhv", "stamped", "measuring", "live", "heavy", "items",
                  "split-items", "heavy-items", "zero-frame-items", "tile-frames", "bg-tile-frames")}
            cost, measuring = pred[4], pred[5]
            assert f["nframes"] == n and 0 < f["live"] <= nt
            if p["scene"] != "S":
                assert f["live"] == nt, (name, k, f["live"], nt)
            split = launch_split(n, nt, f["live"], cost, p["item_tiles"])
            assert (f["ns"], f["fpi"], f["hs"], f["fhv"]) == split, (name, k, line, split)
            assert split == pred[:4], (name, k, "the GPU tests took another split", split, pred[:4], f["live"])
            assert f["measuring"] == int(measuring), (name, k, line)
            assert f["tile-frames"] == f["live"] * n, (name, k, line)
            assert f["heavy"] <= f["live"] and (f["hs"] != f["ns"] or f["heavy"] == 0)
            assert f["items"] == f["heavy"] * f["hs"] + (f["live"] - f["heavy"]) * f["ns"], (name, k, line)
            assert f["heavy-items"] == f["heavy"] * f["hs"], (name, k, line)
            assert f["zero-frame-items"] == 0, (name, k, line)
            assert f["split-items"] == f["items"] - f["live"], (name, k, line)
            if f["ns"] > 1:
                assert f["split-items"] > 0
            assert f["bg-tile-frames"] == (nt - f["live"]) * n, (name, k, line)
            assert _field(counter_lines[name, k]["bin-counters"], "plan-disagrees") == 0, (name, k)
            seen.append(dict(f, plan=name, spp=p["spp"], base=(p["w"], p["h"]) == BASE.get(p["spp"])))
    for spp in BASE:
        assert any(s["base"] and s["spp"] == spp and 1 < s["fpi"] < s["nframes"] for s in seen), spp
    for stamped in (0, 1):
        assert any(0 < s["heavy"] < s["live"] and s["heavy-items"] > 0 and s["stamped"] == stamped for s in seen), stamped
    for plan in ("heavy_64", "heavy_4"):
        assert any(0 < s["heavy"] < s["live"] and s["heavy-items"] > 0 for s in seen if s["plan"] == plan), plan
    assert any(s["stamped"] and s["ns"] > 1 for s in seen)
    assert any(s["measuring"] and s["ns"] > 1 for s in seen)
    assert any(s["stamped"] and s["ns"] > 1 and s["bg-tile-frames"] > 0 for s in seen)


@pytest.mark.gpu
def test_hit_cache_sequence(gpu, bihrt_mod):
    """The hit cache across launches (one item per tile: PARAM_ITEM_TILES = 1,
    calls of 5 frames over the first 44 rows of 67x45, scene D, lists of 16
    entries and more): camera
    X twice, X on aligned bands (another queue key: the cached hits are void),
    camera Y, X again (its set and its cache were kept), a camera Z whose bins
    are unusable under PARAM_BINS_CAP = 1000 and then rebuilt, a rebuild from
    another soup of the same triangle count (the cached ids now name other
    triangles), X again.  The first and last frame of every call equal the
    oracle of the soup current at the call."""
    import torch
    w, h, spp, n = 67, 45, 4, 5
    X, Y, Z = "inside_diag", "inside_z", "mirrored"
    soup = torch.from_numpy(scene("D").copy()).cuda()
    torch.cuda.synchronize()
    g = bihrt_mod.GPUArrayManager.from_device(soup.data_ptr(), len(scene("D")))
    g.set_param(bihrt_mod.PARAM_ITEM_TILES, 1)
    top, bands = bihrt_mod.Rows(0, TOP_67x45, TOP_67x45, 1), bihrt_mod.Rows(4, 8, 4, 2)
    from test_tile_shapes import rows_ys
    r = bihrt_mod.Renderer(g, w, h, spp=spp, seed=SEED)
    steps = [(X, top, None, "D"), (X, top, None, "D"), (X, bands, None, "D"), (Y, top, None, "D"),
             (X, top, None, "D"), (Z, top, 1000, "D"), (Z, top, 0, "D"), (X, top, None, "D2"),
             (X, top, None, "D2")]
    bufs = [torch.full((n * (h * w + GAP),), -1, dtype=torch.int32, device="cuda") for _ in steps]
    torch.cuda.synchronize()
    usable = []
    for k, ((cam, rows, cap, s), buf) in enumerate(zip(steps, bufs)):
        if cap is not None:
            g.set_param(bihrt_mod.PARAM_BINS_CAP, cap)
        if s == "D2" and steps[k - 1][3] == "D":
            g.sync()                      # (the caller's duty: the soup is not rewritten under a build or render)
            soup.copy_(torch.from_numpy(scene("D2").copy()))
            torch.cuda.synchronize()
            g.rebuild()
        nrows = rows.nrows
        r.camera = to_camera(bihrt_mod, cam_of(cam, w, h))
        r.render_device_frames(buf.data_ptr(), n * k, n, nrows * w + GAP, rows=rows)
        r.sync()
        usable.append(bool(g.bins_stats().usable))
        ys = rows_ys(rows)
        b = buf.cpu().numpy().view(np.uint32)[:n * (nrows * w + GAP)].reshape(n, nrows * w + GAP)
        assert (b[:, nrows * w:] == 0xFFFFFFFF).all(), (k, "stride gap written")
        for j in (0, n - 1):
            got, ref = b[j, :nrows * w].reshape(nrows, w), oracle_frame(s, cam, w, h, spp, n * k + j)[ys]
            assert np.array_equal(got, ref), (k, cam, s, n * k + j, diff(got, ref))
    assert usable == [True, True, True, True, True, False, True, True, True], usable
    # the two soups' images differ where a stale id would be believed
    assert diff(oracle_frame("D", X, w, h, spp, 35), oracle_frame("D2", X, w, h, spp, 35)) > w * h // 10
    g.close()


KNOBS = ["BIH_HIT_CACHE_XL=0", "BIH_COST_QUEUE=0", "BIH_STAMPED=0", "BIH_LIVE_ITEMS=0", "BIH_LIVE_ITEMS=8000",
         "BIH_STATIC_ROUNDS=0", "BIH_STATIC_ROUNDS=3", "BIH_QUEUE_LPT=0", "BIH_CAM_SETS=1"]


@pytest.mark.gpu
@pytest.mark.parametrize("knob", KNOBS)
def test_knobs_change_no_pixel(knob, gpu, tmp_path):
    """Each A/B environment knob in a fresh child process, calls of 16, 16,
    16, 16 and 7 frames at 64 spp on one stream: the first and last frame of
    every call and the range starts of the default split and of the knob's
    equal the oracle's frames."""
    key, val = knob.split("=")
    out = tmp_path / "frames.npy"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "knob", str(out)],
                       env=dict(os.environ, **{key: val}), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = np.load(out)
    plan = PLANS["knobs_64"]
    w, h, spp = plan["w"], plan["h"], plan["spp"]
    assert got.shape == (sum(c[1] for c in plan["calls"]), h, w)
    live_items = int(val) if key == "BIH_LIVE_ITEMS" else LIVE_ITEMS
    for (first, n, cam, _), a, b in zip(plan["calls"], plan_splits("knobs_64"), plan_splits("knobs_64", live_items)):
        for j in sorted({0, n - 1} | set(range_starts(n, a[1])) | set(range_starts(n, b[1])[:3])):
            ref = oracle_frame("A", cam, w, h, spp, first + j)
            assert np.array_equal(got[first + j], ref), (knob, first + j, diff(got[first + j], ref))


# --- the children -----------------------------------------------------------------

def _child(argv):
    import bihrt
    if argv[0] == "counters":
        for name in argv[1:]:
            run_plan(bihrt, name, sync_each=True, note=_note)
    elif argv[0] == "knob":
        np.save(argv[1], np.concatenate(run_plan(bihrt, "knobs_64")))
    else:
        raise SystemExit("usage: test_item_splits.py counters PLAN... | knob OUT.npy")


if __name__ == "__main__":
    _child(sys.argv[1:])
