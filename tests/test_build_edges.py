"""The BIH builder (csrc/bih_build.hip) at every kernel's tile and level
boundary ("Builder sizes under test"): scenes of tests/lattice_scenes.py,
whose N, U and runs of equal codes are exact by construction.

CPU tests show that the inputs are what they claim: the oracle's front half
(codes, stable sort, runs) equals a numpy restatement from the requested code
list that shares no code with it, each case sits on its boundary, and every
compared frame and ray set is neither empty nor saturated.  GPU tests compare
the builder's exported arrays, two rebuilds, closest-hit queries (the packed
`nodes` and `tris_s` records) and one frame through the frustum bins and through
the reference walk (the per-triangle leaf index k_runs writes) with the
oracle.  Every comparison is on bits.
"""
import functools

import numpy as np
import pytest

import lattice_scenes as ls
from camera_cases import hit_share
from test_cameras import SEED, device_render
from test_gpu_parity import TREE_KEYS, _tree_equal
from test_trace import F32, assert_hits, expected_of, gen

W, H, SPP = 48, 32, 4
SCAN_TILE, RS_TILE = 2048, 4096          # kScanTile, kRsTile (bih_build.hip)
RAYS, RAYS_BIG = 2048, 256               # the oracle answers them one at a time from Python


def show(capsys, text):
    """A line of the run's report, printed past pytest's capture."""
    with capsys.disabled():
        print("\n  " + text, end="")


def restated(codes):
    """Sorted codes, stable order, runs: numpy from the requested code list
    alone (pins first, as lattice() emits them)."""
    full = np.concatenate([np.array(ls.PIN_CODES, np.uint32), np.asarray(codes, np.uint32)])
    tri_idx = np.argsort(full, kind="stable").astype(np.uint32)
    morton = full[tri_idx]
    unique_mc, first_idx, dup_cnt = np.unique(morton, return_index=True, return_counts=True)
    return morton, tri_idx, unique_mc, dup_cnt.astype(np.uint32), first_idx.astype(np.int32)


@functools.lru_cache(maxsize=None)
def oracle_image(name):
    img = ls.oracle_tree(name).render(W, H, spp=SPP, frame=0, seed=SEED, cam=ls.camera(name, W, H))[0]
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def ray_set(name):
    """(rays as RAY_DTYPE, the oracle's HIT_DTYPE records), once per process:
    test_trace.gen over the scene, t_lo = 0.  low_digit_only's triangles all
    lie on the box's near face and face out of it, so there every fourth ray
    (an aimed one) starts in front of that face."""
    import bihrt
    tris, ot = ls.tris_of(name), ls.oracle_tree(name)
    n = RAYS_BIG if name in ls.BIG else RAYS
    o, d = gen(tris, ot, n, 11)
    if name == "low_digit_only":
        tgt = o[1::4] + d[1::4]
        o[1::4, 2] = -np.abs(o[1::4, 2]) - F32(0.25)
        d[1::4] = tgt - o[1::4]
    exp = expected_of(tris, ot, o, d, 0.0)
    rays = bihrt.pack_rays(o, d, 0.0)
    rays.setflags(write=False)
    exp.setflags(write=False)
    return rays, exp


def trace_share(exp):
    import bihrt
    return float((exp["prim"] != bihrt.NO_HIT).mean())


def spans_tiles(ot):
    """Runs whose members' input indices span more than a radix tile."""
    return sum(int(ot.tri_idx[f:f + c].max()) - int(ot.tri_idx[f:f + c].min()) > RS_TILE
               for f, c in zip(ot.first_idx, ot.dup_cnt) if c > 1)


# --- CPU ------------------------------------------------------------------------

def test_case_sizes():
    """N of every case, from the generator alone (the boundaries of DESIGN.md's table)."""
    n = {c: ls.tris_of(c).shape[0] for c in ls.CASES}
    assert [n[f"distinct_{k}"] for k in (256, 257, 258, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 8193)] == \
        [256, 257, 258, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 8193]
    assert (n["pow20"], n["pow20_plus1"], n["pow20_plus1_u1027"]) == (1 << 20, (1 << 20) + 1, (1 << 20) + 1)
    assert (n["u1_n5000"], n["u2_n9000"], n["u3_n12289"]) == (5000, 9000, 12289)
    assert n["runs7"] == 6 + 7 * 856 + 2 and n["runs8"] == 7 + 8 * 749 + 2
    assert n["top_digit_only"] == n["low_digit_only"] == 2 * RS_TILE + 2
    assert all(n[c] <= 12289 for c in ls.RENDERED) and len(ls.RENDERED) == len(ls.CASES) - 3


@pytest.mark.parametrize("name", list(ls.LATTICE))
def test_lattice_is_what_it_claims(name, capsys):
    """The oracle's codes, stable order and runs equal the numpy restatement
    from the requested code list; the scene box is the lattice's on bits; and
    the case sits on the boundary it is listed for."""
    codes, _ = ls.codes_of(name)
    ot = ls.oracle_tree(name)
    morton, tri_idx, unique_mc, dup_cnt, first_idx = restated(codes)
    assert ot.n == codes.size + 2 and ot.U == unique_mc.size
    for k, want in (("morton", morton), ("tri_idx", tri_idx), ("unique_mc", unique_mc), ("dup_cnt", dup_cnt),
                    ("first_idx", first_idx)):
        got = getattr(ot, k)
        assert got.dtype == want.dtype and np.array_equal(got, want), k
    assert np.array_equal(ot.scene_lo.view(np.uint32), ls.BOX_LO.view(np.uint32))
    assert np.array_equal(ot.scene_hi.view(np.uint32), ls.BOX_HI.view(np.uint32))
    # each pin is a run of one at the first and the last sorted position
    assert ot.tri_idx[0] == 0 and ot.tri_idx[-1] == 1 and ot.dup_cnt[0] == ot.dup_cnt[-1] == 1
    f, c = ot.first_idx.astype(np.int64), ot.dup_cnt.astype(np.int64)
    facts = ""
    if name.startswith("distinct") or name in ("pow20", "pow20_plus1"):
        assert ot.U == ot.n and not np.array_equal(ot.tri_idx, np.arange(ot.n))
        facts = "all codes distinct, input shuffled"
    elif name == "pow20_plus1_u1027":
        assert ot.U == 1027 and (c[1:-1] == 1023).all()
        # level 10 of the segment tree has 1025 entries for 2 valid ones
        assert (ot.n + 1023) // 1024 == 1025 and (ot.U + 1023) // 1024 == 2
        facts = "1025 runs of 1023; 2 of 1025 level-10 entries valid"
    elif name == "runs7":
        assert c[1] == 6 and (c[2:-1] == 7).all()
        for edge in (SCAN_TILE, 2 * SCAN_TILE):
            assert ((f < edge) & (edge < f + c)).any(), edge
        assert set((f[1:-1] % 8).tolist()) == set(range(8))
        assert spans_tiles(ot) >= 1
        facts = f"runs straddle 2048 and 4096, start at every phase mod 8; {spans_tiles(ot)} runs span > 4096 inputs"
    elif name == "runs8":
        assert c[1] == 7 and (c[2:-1] == 8).all()
        assert SCAN_TILE in f and 2 * SCAN_TILE in f and (f[2:-1] % 8 == 0).all()
        assert spans_tiles(ot) >= 1
        facts = f"runs start at 2048 and 4096, all on multiples of 8; {spans_tiles(ot)} runs span > 4096 inputs"
    elif name == "top_digit_only":
        assert np.unique(codes).size == 1024 and (codes & 0xFFFFF == codes[0] & 0xFFFFF).all()
        assert np.unique(codes >> 20).size == 1024 and (c[1:-1] == 8).all()
        facts = "1024 codes x 8, bits 0..19 shared"
    elif name == "low_digit_only":
        assert np.unique(codes).size == 1024 and (codes >> 10 == codes[0] >> 10).all()
        assert np.unique(codes & 0x3FF).size == 1024 and (c[1:-1] == 8).all()
        facts = "1024 codes x 8, bits 10..29 shared"
    show(capsys, f"{name}: N {ot.n} U {ot.U}; {facts}")


@pytest.mark.parametrize("name", list(ls.FEW))
def test_few_codes_are_what_they_claim(name, capsys):
    """U and the multiset of run lengths of the scenes without pins; every
    leaf holds more than 3 triangles (the node record's count code is the
    escape value 0) and every run fills a radix tile or more."""
    ot = ls.oracle_tree(name)
    counts = ls.few_counts(name)
    assert ot.n == sum(counts) and ot.U == len(counts)
    assert sorted(ot.dup_cnt.tolist()) == sorted(counts)
    assert (ot.dup_cnt > 3).all() and (ot.dup_cnt >= RS_TILE).all()
    assert not np.array_equal(ot.tri_idx, np.arange(ot.n)) or ot.U == 1
    show(capsys, f"{name}: N {ot.n} U {ot.U}; runs {ot.dup_cnt.tolist()}")


@pytest.mark.parametrize("name", ls.RENDERED)
def test_rendered_frames_have_something_to_see(name, capsys):
    share = hit_share(oracle_image(name))
    show(capsys, f"{name}: hit pixels {share:.3f}, {np.unique(oracle_image(name)).size} shades")
    assert 0.10 <= share <= 0.90, share


@pytest.mark.parametrize("name", ls.CASES)
def test_ray_sets_are_balanced(name, capsys):
    rays, exp = ray_set(name)
    assert rays.shape[0] == (RAYS_BIG if name in ls.BIG else RAYS)
    share = trace_share(exp)
    show(capsys, f"{name}: {rays.shape[0]} rays, hit share {share:.3f}")
    assert 0.10 <= share <= 0.90, share


# --- GPU ------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ls.CASES)
def test_arrays_and_rebuilds(name, gpu, bihrt_mod):
    """All 15 exported arrays equal the oracle's (floats on bits) and n_unique
    is U; after each of two rebuilds (graph replay, the epoch tags, the second
    and third tree buffer) the arrays are the first build's byte for byte."""
    g = bihrt_mod.GPUArrayManager(ls.tris_of(name))
    ot = ls.oracle_tree(name)
    assert g.info().n_unique == ot.U
    a = g.arrays()
    _tree_equal(a, ot)
    for k in range(2):
        g.rebuild()
        assert g.info().n_unique == ot.U
        b = g.arrays()
        for key in TREE_KEYS:
            assert a[key].shape == b[key].shape and np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), \
                (key, k)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ls.CASES)
def test_closest_hits(name, gpu, bihrt_mod):
    """t, u, v and prim of every ray equal the oracle's: the check on the packed
    node and sorted-triangle records, which are not exported."""
    from test_trace import dev_trace
    rays, exp = ray_set(name)
    assert 0.10 <= trace_share(exp) <= 0.90
    g = bihrt_mod.GPUArrayManager(ls.tris_of(name))
    got = dev_trace(g, rays, bihrt_mod.QUERY_CLOSEST)
    g.close()
    assert_hits(got, exp, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ls.RENDERED)
def test_frame(name, gpu, bihrt_mod, oracle_mod):
    """Frame 0 at 48x32, 4 spp: the default path (for the lattice cases the
    frustum bins, and so the per-triangle leaf index of k_runs) and the
    reference walk equal the oracle."""
    ref = oracle_image(name)
    cam = ls.camera(name, W, H)
    if cam is None:
        cam = oracle_mod.camera_reference(W, H)
    g = bihrt_mod.GPUArrayManager(ls.tris_of(name))
    for trav in (bihrt_mod.TRAVERSE_ANYHIT, bihrt_mod.TRAVERSE_REFERENCE):
        img = device_render(bihrt_mod, g, cam, W, H, SPP, 0, trav)
        assert np.array_equal(img, ref), (name, trav, int((img != ref).sum()))
        if trav == bihrt_mod.TRAVERSE_ANYHIT:
            st = g.bins_stats()
            print(f"bins {name}: usable {st.usable} list_entries {st.list_entries} "
                  f"global_entries {st.global_entries}")
            # Every lattice frame goes through the bins.  The scenes of copies
            # do not: a one-leaf tree has no node to bin under, and the
            # thousands of screen-sized copies of the other two are more than
            # the bins take (kBinGlobalMax), so the walk renders them.
            assert bool(st.usable) == (name in ls.LATTICE)
    g.close()
