"""Every render path under cameras inside, across and far from the scene.

The catalogue (tests/camera_cases.py) holds one camera per camera-dependent
branch of the frustum bins: triangles behind the eye plane (k_bin_fp's
side = -1), triangles across it (side = 0: the global list), a global list past
kBinGlobalMax, a mirrored image (bin_camera's flip of n), a sheared off-axis
frustum, cameras bin_camera refuses, and origins far from the scene.  The CPU
tests show from the oracle and f64 numpy alone that each camera populates its
branch and sees a varied image; the GPU tests compare every kernel family
with the oracle under those cameras.  Every comparison is on bits.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import camera_cases as cc
import test_gbuffer as tg
from camera_cases import H, W
from conftest import ROOT

F32 = np.float32
SEED = 1984
NOT_VARIED = ("away", "cornell_in")       # all background / no background: asserted as such

tg.EXTRA_SCENES.update({"cam_A": lambda: cc.scene("A"), "cam_C": lambda: cc.scene("C")})
tg.EXTRA_CAMERAS.update({name: functools.partial(cc.camera, name) for name in cc.CATALOGUE})


@functools.lru_cache(maxsize=None)
def oracle_tree(s):
    import oracle
    return oracle.OracleTree(cc.scene(s))


@functools.lru_cache(maxsize=None)
def oracle_frame(s, name, w, h, spp, frame):
    """The oracle's image of scene s under catalogue camera `name` (or "reference"); read-only."""
    img = oracle_tree(s).render(w, h, spp=spp, frame=frame, seed=SEED, cam=cam_of(name, w, h))[0]
    img.setflags(write=False)
    return img


def cam_of(name, w, h):
    if name == "reference":
        import oracle
        return oracle.camera_reference(w, h)
    if name.startswith("moved"):
        return moved_reference(w, h, *{"moved1": (0.05, -0.03, 0.2), "moved2": (-0.3, 0.1, -0.1)}[name])
    return cc.camera(name, w, h)


def moved_reference(w, h, dx, dy, dz):
    """The reference camera shifted, not rotated (outside every scene)."""
    import oracle
    c = oracle.camera_reference(w, h).copy()
    c[0:3] += F32([dx, dy, dz])
    c[3:6] += F32([dx, dy, dz])
    return c


# --- CPU ------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(cc.CATALOGUE))
def test_catalogue_guard(name, oracle_mod):
    """Each camera reaches the branch it is listed for, and its image is neither
    empty nor saturated, by the oracle and f64 numpy alone -- so a triangle a
    wrong branch drops or lists twice changes pixels."""
    s = cc.scene_of(name)
    cam = cc.camera(name)
    alive, straddle, behind = cc.classify(cc.scene(s), cam)
    A, n, an = cc.plane_terms(cam)
    nl, al = np.linalg.norm(n), np.linalg.norm(A)
    shares = [cc.hit_share(oracle_frame(s, name, W, H, 4, 0)), cc.hit_share(oracle_frame(s, name, 37, 29, 3, 0))]
    print(f"{name}: hit share {shares[0]:.3f} (96x64x4) {shares[1]:.3f} (37x29x3); alive {alive}, "
          f"straddling {straddle}, behind {behind}; A.n {an:.3g}, |A||n| {nl * al:.3g}")
    if name == "away":
        assert shares == [0.0, 0.0] and behind == alive == 9892 and straddle == 0
    elif name == "cornell_in":
        assert shares == [1.0, 1.0]
    else:
        for sh in shares:
            assert 0.10 <= sh <= 0.90, sh
    if name in cc.STRADDLING:
        assert straddle >= 64 and behind > cc.GLOBAL_MAX, (straddle, behind)
    if name in ("at_edge", "cornell_back"):
        assert straddle > 0 and behind > 0, (straddle, behind)
    if name == "mirrored":
        assert an < 0                                          # bin_camera flips n
    elif name not in ("plane_through_origin", "zero_horizontal"):
        assert an > 0
    # bin_camera's conditions, restated in f64
    if name == "zero_horizontal":
        assert nl == 0.0
    elif name == "plane_through_origin":
        assert al > 0 and nl > 0 and not abs(an) > 1e-3 * nl * al and abs(an) < 1e-6 * nl * al
    elif name == "wide_nobins":
        assert al > 0 and nl > 0 and 0 < an <= 1e-3 * nl * al
    else:
        assert abs(an) > 1e-3 * nl * al                        # wide174: 0.028
    if name == "wide174":
        assert abs(an) < 0.05 * nl * al
    if name.startswith("tele"):
        assert straddle == 0 and behind == 0 and alive > 5000
        assert np.abs(cam[0:3]).max() >= 2000


def test_scene_b_overflows_the_global_list(oracle_mod):
    """Scene B's band puts more than twice kBinGlobalMax alive triangles across
    the eye plane of inside_diag (and of mirrored, the same plane) and leaves
    both images as scene A's."""
    for name in ("inside_diag", "mirrored"):
        alive, straddle, behind = cc.classify(cc.scene("B"), cc.camera(name))
        print(f"scene B under {name}: alive {alive}, straddling {straddle}, behind {behind}")
        assert straddle >= 2 * cc.GLOBAL_MAX, straddle
        assert np.array_equal(oracle_frame("B", name, W, H, 4, 0), oracle_frame("A", name, W, H, 4, 0))
    # under the outside cameras that warm the camera sets no triangle straddles
    for name in ("reference", "moved1", "moved2"):
        assert cc.classify(cc.scene("B"), cam_of(name, W, H))[1:] == (0, 0), name


def test_look_pins_camera_reference(oracle_mod):
    """look() from the reference pose with the reference's extents (vertical 2:
    hh = 1, plane 1) gives camera_reference's origin, horizontal, vertical and
    lower_left y, z to the bit.  The reference's lower_left x is origin.x - 2
    whatever the aspect (its frustum is off-axis unless w = 2 h) while look()
    centres the image, origin.x - w / h: at w = 2 h all twelve floats agree to
    the bit, elsewhere x differs by exactly that shift."""
    for w, h in [(96, 64), (640, 480), (1920, 1080), (256, 256), (37, 29), (128, 64), (96, 48), (1920, 960)]:
        got, ref = cc.look((2, 0, -2), (0, 0, 1), w, h, hh=1.0), oracle_mod.camera_reference(w, h)
        same = got.view(np.uint32) == ref.view(np.uint32)
        assert same[[0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11]].all(), (w, h, got, ref)
        assert ref[3] == 0.0 and got[3] == F32(2.0 - w / h)
        if w == 2 * h:
            assert same.all()


@pytest.mark.parametrize("name", list(cc.CATALOGUE))
def test_camera_ray_bound_covers_catalogue(name, bihrt_mod):
    """bih_camera_ray_bound (it sizes the miss-proof boxes) bounds |D| per
    component over the f32 directions of every sample of frame 0."""
    cam = cc.camera(name)
    dmax = bihrt_mod.camera_ray_bound(bihrt_mod.Camera.from_list(cam.tolist()))
    d = np.abs(tg.frame_rays(cam, W, H, 4, 0)).reshape(-1, 3)
    assert np.isfinite(dmax).all() and (d <= dmax[None, :]).all(), (name, dmax, d.max(0))


# --- GPU ------------------------------------------------------------------------

def to_camera(bihrt, cam):
    return bihrt.Camera.from_list(np.asarray(cam, F32).tolist())


def device_render(bihrt, g, cam, w, h, spp, frame, traverse, rows=None, stats=False):
    """One frame of a fresh Renderer into device memory: (nrows, w) u32[, (rays, 3) u32 counters]."""
    import torch
    nrows = rows.nrows if rows is not None else h
    out = torch.full((nrows * w,), -1, dtype=torch.int32, device="cuda")
    st = torch.zeros(3 * nrows * w * spp, dtype=torch.int32, device="cuda") if stats else None
    torch.cuda.synchronize()
    r = bihrt.Renderer(g, w, h, spp=spp, seed=SEED, camera=to_camera(bihrt, cam))
    r.render_device(out.data_ptr(), frame, rows=rows, traverse=traverse, stats_ptr=st.data_ptr() if stats else None)
    r.sync()
    img = out.cpu().numpy().view(np.uint32).reshape(nrows, w)
    return (img, st.cpu().numpy().view(np.uint32).reshape(-1, 3)) if stats else img


def diff(a, b):
    return int((np.asarray(a) != np.asarray(b)).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("name", cc.SCENE_A + ["cornell_back"])
def test_catalogue_matches_oracle(name, gpu, bihrt_mod):
    """Frames 0, 1 and 5 of one Renderer on a fresh tree: the any-hit render
    (through the bins where the camera has them) and the reference walk equal
    the oracle on every pixel; the bins' counts say which branch ran."""
    s = cc.scene_of(name)
    g = bihrt_mod.GPUArrayManager(cc.scene(s))
    cam = cc.camera(name)
    for trav in (bihrt_mod.TRAVERSE_ANYHIT, bihrt_mod.TRAVERSE_REFERENCE):
        for frame in (0, 1, 5):
            img = device_render(bihrt_mod, g, cam, W, H, 4, frame, trav)
            ref = oracle_frame(s, name, W, H, 4, frame)
            assert np.array_equal(img, ref), (name, trav, frame, diff(img, ref))
        if trav == bihrt_mod.TRAVERSE_ANYHIT:
            st = g.bins_stats()
            print(f"bins {name}: usable {st.usable} list_entries {st.list_entries} global_entries {st.global_entries}")
            if name in cc.DEGENERATE:
                assert not st.usable
            else:
                assert st.usable
                assert st.global_entries <= cc.GLOBAL_MAX
            if name in cc.STRADDLING + ("at_edge", "cornell_back"):
                # (with more than 4096 alive triangles behind, also: those were
                # dropped, not listed globally)
                assert st.global_entries > 0
    g.close()


@pytest.mark.gpu
def test_per_ray_counters_from_inside(gpu, bihrt_mod, oracle_mod):
    """Rays that start inside the scene box (the root interval has tmin < 0):
    the reference walk's node, leaf and triangle counts per ray equal the
    oracle's, the any-hit walk's stay below them; at 37x29x3 (k_render_pixel)
    both walks' counters equal the oracle's."""
    g = bihrt_mod.GPUArrayManager(cc.scene("A"))
    ot = oracle_tree("A")
    cam = cc.camera("inside_diag")
    img, s = device_render(bihrt_mod, g, cam, W, H, 4, 0, bihrt_mod.TRAVERSE_REFERENCE, stats=True)
    ref, _, rs = ot.render(W, H, spp=4, seed=SEED, cam=cam, mode=oracle_mod.MODE_GPU_REF, ray_stats=True)
    assert np.array_equal(img, ref)
    for k, what in enumerate(("node", "leaf", "triangle")):
        assert np.array_equal(s[:, k], rs[:, k]), f"{what} counts differ on {diff(s[:, k], rs[:, k])} rays"
    assert rs[:, 2].max() > 0 and (rs[:, 0] > 1).mean() > 0.5
    img2, s2 = device_render(bihrt_mod, g, cam, W, H, 4, 0, bihrt_mod.TRAVERSE_ANYHIT, stats=True)
    assert np.array_equal(img2, ref)
    assert (s2 <= s).all()
    cam3 = cc.camera("inside_diag", 37, 29)
    for trav, mode in ((bihrt_mod.TRAVERSE_REFERENCE, oracle_mod.MODE_GPU_REF),
                       (bihrt_mod.TRAVERSE_ANYHIT, oracle_mod.MODE_GPU_ANYHIT)):
        img3, s3 = device_render(bihrt_mod, g, cam3, 37, 29, 3, 1, trav, stats=True)
        ref3, _, rs3 = ot.render(37, 29, spp=3, frame=1, seed=SEED, cam=cam3, mode=mode, ray_stats=True)
        assert np.array_equal(img3, ref3), trav
        assert np.array_equal(s3, rs3), ("spp 3 counters differ from the oracle's", trav)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["inside_diag", "mirrored"])
def test_every_packet_through_the_fallback(name, gpu, bihrt_mod):
    """PARAM_FORCE_FALLBACK: k_render_fallback walks every live packet from inside the box."""
    g = bihrt_mod.GPUArrayManager(cc.scene("A"))
    g.set_param(bihrt_mod.PARAM_FORCE_FALLBACK, 1)
    for frame in (0, 3):
        img = device_render(bihrt_mod, g, cc.camera(name), W, H, 4, frame, bihrt_mod.TRAVERSE_ANYHIT)
        ref = oracle_frame("A", name, W, H, 4, frame)
        assert np.array_equal(img, ref), (name, frame, diff(img, ref))
    assert g.bins_stats().usable
    g.close()


@pytest.mark.gpu
def test_global_list_past_limit_sized_path(gpu, bihrt_mod):
    """Scene B under inside_diag as a fresh tree's first camera: the bins
    build reads the counts back, finds the global list past kBinGlobalMax and
    builds no lists; the shortcut passes render from inside the box."""
    g = bihrt_mod.GPUArrayManager(cc.scene("B"))
    cam = cc.camera("inside_diag")
    for trav in (bihrt_mod.TRAVERSE_ANYHIT, bihrt_mod.TRAVERSE_REFERENCE):
        for frame in (0, 2):
            img = device_render(bihrt_mod, g, cam, W, H, 4, frame, trav)
            ref = oracle_frame("B", "inside_diag", W, H, 4, frame)
            assert np.array_equal(img, ref), (trav, frame, diff(img, ref))
        if trav == bihrt_mod.TRAVERSE_ANYHIT:
            st = g.bins_stats()
            print(f"bins B/inside_diag sized: usable {st.usable} list_entries {st.list_entries} "
                  f"global_entries {st.global_entries}")
            assert not st.usable and st.global_entries > cc.GLOBAL_MAX, (st.usable, st.global_entries)
    g.close()


@pytest.mark.gpu
def test_global_list_past_limit_without_round_trip(gpu, bihrt_mod):
    """Three outside cameras warm the three camera sets (each set's first build
    sizes its list with a round trip); inside_diag then builds into an earlier
    camera's list buffer without one, k_bin_status finds the global list past
    kBinGlobalMax, and the device status word alone sends every live packet of
    the frame at the switch -- and of the two issued behind it before the host
    has looked -- to the exact walk.  After a sync the host has turned the bins
    off for this camera; the reference camera has its bins again."""
    import torch
    g = bihrt_mod.GPUArrayManager(cc.scene("B"))
    r = bihrt_mod.Renderer(g, W, H, seed=SEED)
    outs = [torch.full((H * W,), -1, dtype=torch.int32, device="cuda") for _ in range(7)]
    torch.cuda.synchronize()

    def image(k):
        return outs[k].cpu().numpy().view(np.uint32).reshape(H, W)

    for f, name in enumerate(("reference", "moved1", "moved2")):
        r.camera = to_camera(bihrt_mod, cam_of(name, W, H))
        r.render_device(outs[f].data_ptr(), f)
        r.sync()
        assert g.bins_stats().usable, name
        assert np.array_equal(image(f), oracle_frame("B", name, W, H, 4, f)), name
    r.camera = to_camera(bihrt_mod, cc.camera("inside_diag"))
    for f in (3, 4, 5):
        r.render_device(outs[f].data_ptr(), f)
    r.sync()
    for f in (3, 4, 5):
        ref = oracle_frame("B", "inside_diag", W, H, 4, f)
        assert np.array_equal(image(f), ref), (f, diff(image(f), ref))
    st = g.bins_stats()
    print(f"bins B/inside_diag no round trip: usable {st.usable} list_entries {st.list_entries} "
          f"global_entries {st.global_entries}")
    assert not st.usable and st.global_entries > cc.GLOBAL_MAX, (st.usable, st.global_entries)
    r.camera = to_camera(bihrt_mod, cam_of("reference", W, H))
    r.render_device(outs[6].data_ptr(), 6)
    r.sync()
    assert g.bins_stats().usable
    assert np.array_equal(image(6), oracle_frame("B", "reference", W, H, 4, 6))
    g.close()


@pytest.mark.gpu
def test_multi_frame_call_and_streams(gpu, bihrt_mod):
    """One call of 5 frames under inside_diag, then 12 one-frame renders on 3
    streams with the camera cycling inside_diag -> reference -> wide_nobins
    (bins with a global list, bins, no bins; one camera set each)."""
    import torch
    g = bihrt_mod.GPUArrayManager(cc.scene("A"))
    r = bihrt_mod.Renderer(g, W, H, seed=SEED, camera=to_camera(bihrt_mod, cc.camera("inside_diag")))
    P = W * H
    buf = torch.full((5 * P,), -1, dtype=torch.int32, device="cuda")
    outs = [torch.full((P,), -1, dtype=torch.int32, device="cuda") for _ in range(12)]
    torch.cuda.synchronize()
    r.render_device_frames(buf.data_ptr(), 0, 5, P)
    r.sync()
    fr = buf.cpu().numpy().view(np.uint32).reshape(5, H, W)
    for f in (0, 4):
        ref = oracle_frame("A", "inside_diag", W, H, 4, f)
        assert np.array_equal(fr[f], ref), (f, diff(fr[f], ref))
    assert g.bins_stats().usable
    streams = [torch.cuda.Stream() for _ in range(3)]
    cycle = ("inside_diag", "reference", "wide_nobins")
    for k in range(12):
        r.camera = to_camera(bihrt_mod, cam_of(cycle[k % 3], W, H))
        r.render_device(outs[k].data_ptr(), 5 + k, stream=streams[k % 3].cuda_stream)
    torch.cuda.synchronize()
    for k in range(12):
        img = outs[k].cpu().numpy().view(np.uint32).reshape(H, W)
        ref = oracle_frame("A", cycle[k % 3], W, H, 4, 5 + k)
        assert np.array_equal(img, ref), (k, cycle[k % 3], diff(img, ref))
    g.close()


VARIANT_SCRIPT = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(sys.argv[1], "bih-gpu-raytracer_amd"))
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import torch, bihrt
import camera_cases as cc
w, h, spp = 64, 48, 4
g = bihrt.GPUArrayManager(cc.scene("A"))
cam = bihrt.Camera.from_list(cc.camera("inside_diag", w, h).tolist())
out = {}
for tname, trav in (("any", bihrt.TRAVERSE_ANYHIT), ("ref", bihrt.TRAVERSE_REFERENCE)):
    for counters in (False, True):
        img = torch.zeros(w * h, dtype=torch.int32, device="cuda")
        st = torch.zeros(3 * w * h * spp, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r = bihrt.Renderer(g, w, h, spp=spp, camera=cam)
        r.render_device(img.data_ptr(), 0, traverse=trav, stats_ptr=st.data_ptr() if counters else None)
        r.sync()
        out[f"{tname}_{int(counters)}_img"] = img.cpu().numpy()
        out[f"{tname}_{int(counters)}_st"] = st.cpu().numpy()
np.savez(sys.argv[2], **out)
'''


def run_variant(variant, path):
    env = dict(os.environ)
    env.pop("BIH_RENDER_KERNEL", None)
    if variant != "default":
        env["BIH_RENDER_KERNEL"] = variant
    subprocess.run([sys.executable, "-c", VARIANT_SCRIPT, ROOT, str(path)], env=env, check=True, timeout=300)
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def default_kernel_result(tmp_path_factory):
    return run_variant("default", tmp_path_factory.mktemp("variants") / "default.npz")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["packet2", "packet1"])
def test_kernel_variants_from_inside(variant, gpu, tmp_path, default_kernel_result):
    """BIH_RENDER_KERNEL=packet2 / packet1, each in a fresh child process,
    under inside_diag at 64x48: both traversals' images (through the bins and
    with counters) and the reference walk's counters equal the default kernel's,
    and the default kernel's image is the oracle's."""
    a, b = default_kernel_result, run_variant(variant, tmp_path / f"{variant}.npz")
    ref = oracle_frame("A", "inside_diag", 64, 48, 4, 0)
    assert sorted(a) == sorted(b) and len(a) == 8
    for k in a:
        if k.endswith("_img"):
            assert np.array_equal(a[k].view(np.uint32).reshape(48, 64), ref), ("default", k)
        if k.endswith("_img") or k == "ref_1_st":
            assert np.array_equal(a[k], b[k]), (variant, k, diff(a[k], b[k]))
    assert a["ref_1_st"].any()


_trees = {}


def tree(s):
    """The scene's GPU tree, shared by the G-buffer tests of this module."""
    import bihrt
    if s not in _trees:
        _trees[s] = bihrt.GPUArrayManager(cc.scene(s))
    return _trees[s]


@pytest.fixture(scope="module", autouse=True)
def _free_trees():
    yield
    while _trees:
        _trees.popitem()[1].close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["inside_diag", "mirrored", "away", "cornell_in", "cornell_back"])
def test_gbuffer_cameras(name, gpu, bihrt_mod):
    """Every plane and `hits` at 48x32x4, frame 1, with the bins' hit mask and
    with every sample walked."""
    s = cc.scene_of(name)
    exp = tg.expected("cam_" + s, name, 48, 32, 4, 1)
    hit = exp["hits"]["prim"] != bihrt_mod.NO_HIT
    if name == "away":
        assert not hit.any() and (exp["hits"]["t"] == tg.FLT_MAX).all()      # every record is the miss record
        assert not exp["coverage"].any() and not tg.bits(exp["bary"]).any() and not tg.bits(exp["normal"]).any()
    elif name == "cornell_in":
        assert hit.all() and np.unique(exp["prim"]).size >= 6 and np.unique(tg.bits(exp["depth"])).size > 1000
    else:
        tg.balanced("cam_" + s, exp)
    g = tree(s)
    r = tg.renderer(g, "cam_" + s, name, 48, 32, 4)
    tg.both_masks(g, lambda: tg.dev_gbuffer(r, 1), exp, name)
    assert g.bins_stats().usable


@pytest.mark.gpu
def test_gbuffer_without_bins(gpu, bihrt_mod):
    """zero_horizontal: no bins, so no hit mask to take from them.  The planes
    with PARAM_GBUFFER_MASK = 1 equal those with 0 and the oracle's."""
    exp = tg.expected("cam_A", "zero_horizontal", 48, 32, 4, 1)
    tg.balanced("cam_A", exp)
    g = tree("A")
    # (bih_bins_get_stats speaks of the latest render issued; a G-buffer call
    # that finds no bins issues none, so a plain render shows their absence)
    img = device_render(bihrt_mod, g, cc.camera("zero_horizontal", 48, 32), 48, 32, 4, 1, bihrt_mod.TRAVERSE_ANYHIT)
    assert np.array_equal(img, oracle_frame("A", "zero_horizontal", 48, 32, 4, 1))
    assert not g.bins_stats().usable
    r = tg.renderer(g, "cam_A", "zero_horizontal", 48, 32, 4)
    got = {}
    try:
        for m in (1, 0):
            g.set_param(bihrt_mod.PARAM_GBUFFER_MASK, m)
            got[m] = tg.dev_gbuffer(r, 1)
    finally:
        g.set_param(bihrt_mod.PARAM_GBUFFER_MASK, 1)
    tg.assert_planes(got[1], got[0], "mask 1 vs mask 0")
    tg.assert_planes(got[1], exp, "mask 1")
    tg.assert_planes(got[0], exp, "mask 0")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_in", "cornell_back", "inside_diag"])
def test_whitted_from_inside(name, gpu, bihrt_mod):
    """8-bounce mirror rays whose primary rays start inside the box, 64x48,
    frames 0 and 2: the image and every sample's hit count equal the oracle's."""
    import torch
    s = cc.scene_of(name)
    w, h, spp = 64, 48, 4
    g = bihrt_mod.GPUArrayManager(cc.scene(s))
    cam = cc.camera(name, w, h)
    r = bihrt_mod.Renderer(g, w, h, spp=spp, seed=SEED, camera=to_camera(bihrt_mod, cam))
    out = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    hits = torch.zeros(h * w * spp, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for frame in (0, 2):
        r.render_whitted_device(out.data_ptr(), frame, hits_ptr=hits.data_ptr())
        r.sync()
        ref, _, dep = oracle_tree(s).render_whitted(w, h, spp=spp, frame=frame, seed=SEED, cam=cam, depths=True)
        hs = hits.cpu().numpy().astype(np.uint8)
        assert np.array_equal(hs, dep), (name, frame, diff(hs, dep))
        assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(h, w), ref), (name, frame)
        assert (dep >= 2).any()                                 # secondary rays hit too
        if name == "cornell_in":
            assert (dep > 0).all() and np.unique(dep).size > 2
    g.close()


@pytest.mark.gpu
def test_band_rows_from_inside(gpu, bihrt_mod):
    """Rank 1 of 3's interleaved 8-row bands under inside_diag equal those rows of the full frame."""
    from bihrt.tiling import band_rows, rows_of_rank
    g = bihrt_mod.GPUArrayManager(cc.scene("A"))
    cam = cc.camera("inside_diag")
    full = device_render(bihrt_mod, g, cam, W, H, 4, 0, bihrt_mod.TRAVERSE_ANYHIT)
    assert np.array_equal(full, oracle_frame("A", "inside_diag", W, H, 4, 0))
    ys = rows_of_rank(H, 8, 1, 3)
    part = device_render(bihrt_mod, g, cam, W, H, 4, 0, bihrt_mod.TRAVERSE_ANYHIT, rows=band_rows(H, 8, 1, 3))
    assert np.array_equal(part, full[ys]), diff(part, full[ys])
    assert 0.10 <= cc.hit_share(full[ys]) <= 0.90
    g.close()
