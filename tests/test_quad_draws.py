"""k_render_bins' draws at 4 spp (frame_draws_quad, bih_render.hip): the four
lanes of a pixel hold the same XORWOW state and share the B terms of a frame's
8 steps -- lane s computes B_{s+1} and B_{s+5}, step n reads its term from
lane (n - 1) & 3 of the quad -- while every lane runs the A chain.

CPU: the shared form restated in numpy, lane by lane, equals 8 sequential
xorwow_raw steps.  GPU: every 4-spp instance of the kernel (plain, measuring,
stamped, mask) against the oracle on bits, on the 8,000-triangle soup at
37 x 29, where tiles are cut at the right and at the top edge, under a shifted
reference camera that leaves the soup across both of those edges: the cut
tiles are live (under the reference camera they are background, and no lane of
them draws).  The calls pass one band of 32 rows, of which the image has 29:
band and start lie on tile rows, so the bins serve them (a plain 29-row frame
would take the per-frame kernels and never reach k_render_bins).
"""
import functools

import numpy as np
import pytest

from test_cameras import SEED, diff, moved_reference, to_camera
from test_solid_tiles import otree, soup

U32 = np.uint32
W, H, SPP = 37, 29, 4
BAND = 32                         # the calls' one band: H rows of it exist
SHIFT = (-0.7, -0.5, 1.0)         # the camera: the reference, moved
# pixel_from_hits(k, 4): Color's blend of k hit and 4 - k missed samples, rgbToInt
PIXEL_OF_HITS = {((10 * (4 - k)) << 16) | (((255 * k + 20 * (4 - k)) // 4) * 0x101): k for k in range(5)}


def camera():
    return moved_reference(W, H, *SHIFT)


@functools.lru_cache(maxsize=None)
def oracle_frame(frame):
    img = otree(1).render(W, H, spp=SPP, frame=frame, seed=SEED, cam=camera())[0]
    img.setflags(write=False)
    return img


# --- the two forms, restated --------------------------------------------------------

def xorwow_raw(v):
    """dev::xorwow_raw on (n, 5) u32 states, in place: the step's raw word."""
    t = v[:, 0] ^ (v[:, 0] >> U32(2))
    v[:, 0:4] = v[:, 1:5]
    v[:, 4] = (v[:, 4] ^ (v[:, 4] << U32(4))) ^ (t ^ (t << U32(1)))
    return v[:, 4].copy()


def _a(v):
    return v ^ (v << U32(4))


def _b(x):
    t = x ^ (x >> U32(2))
    return t ^ (t << U32(1))


def quad_draws(rs):
    """frame_draws_quad on (n, 5) states: per lane s = 0..3 of each state's
    quad the end state (n, 4, 5), the 8 outputs (n, 4, 8) and the two words
    the lane keeps (n, 4, 2).  A [:, k] column is quad lane k; quad_lane<K>(x)
    is x[:, K] seen by all four lanes."""
    n = len(rs)
    s = np.arange(4)
    state = np.repeat(rs[:, None, :], 4, axis=1)                 # every lane holds the pixel's state
    own = state[np.arange(n)[:, None], s[None, :], s[None, :]]   # rs[s] of lane s
    lo = _b(own)                                                 # B_{s+1}
    o = [state[:, :, 4]]                                         # o_0
    for k in range(4):
        o.append(_a(o[-1]) ^ lo[:, k:k + 1])
    hin = np.stack([o[0][:, 0], o[1][:, 1], o[2][:, 2], o[3][:, 3]], axis=1)     # o_s of lane s
    hi = _b(hin)                                                 # B_{s+5}
    for k in range(4):
        o.append(_a(o[-1]) ^ hi[:, k:k + 1])
    outs = np.stack(o[1:], axis=2)
    end = np.stack(o[4:9], axis=2)
    rows = np.arange(n)[:, None]
    kept = np.stack([outs[rows, s[None, :], 2 * s[None, :]], outs[rows, s[None, :], 2 * s[None, :] + 1]], axis=2)
    return end, outs, kept


def test_quad_form_equals_sequential_steps():
    """10^5 seeded states plus states with zero words (each single word zero,
    each single word the only non-zero one, all zero): the shared form's end
    state and all 8 outputs on each of the four lanes, and the two words lane
    s keeps (draws 2s and 2s+1), equal 8 sequential xorwow_raw steps."""
    rng = np.random.default_rng(9)
    rs = rng.integers(0, 2 ** 32, (100000, 5), dtype=np.uint64).astype(U32)
    special = [np.zeros(5, U32)]
    for i in range(5):
        z = rng.integers(1, 2 ** 32, 5, dtype=np.uint64).astype(U32)
        z[i] = 0
        special.append(z)
        e = np.zeros(5, U32)
        e[i] = U32(rng.integers(1, 2 ** 32))
        special.append(e)
        special.append(np.where(np.arange(5) == i, U32(0xFFFFFFFF), U32(0)).astype(U32))
    rs = np.concatenate([rs, np.stack(special)])
    v = rs.copy()
    seq = np.stack([xorwow_raw(v) for _ in range(8)], axis=1)            # (n, 8)
    end, outs, kept = quad_draws(rs)
    for lane in range(4):
        assert np.array_equal(outs[:, lane], seq), lane
        assert np.array_equal(end[:, lane], v), lane
        assert np.array_equal(kept[:, lane], seq[:, 2 * lane:2 * lane + 2]), lane
    assert len(np.unique(seq)) > 700000                                  # the outputs are not degenerate


def test_guard(oracle_mod):
    """What keeps the GPU tests from being vacuous, by the oracle alone: at
    37 x 29 the soup's frames are neither empty nor saturated, hold partially
    covered pixels (whose value depends on each sample's jitter), and differ
    from frame to frame -- a state carried wrongly from one frame to the next
    changes pixels.  And the rows rule that admits the calls to k_render_bins."""
    from camera_cases import BACKGROUND
    assert W % 4 and H % 4 and BAND % 4 == 0 and H <= BAND           # tiles cut at both edges, through the bins
    imgs = [oracle_frame(f) for f in range(4)]
    for f, img in enumerate(imgs):
        share = float((img != BACKGROUND).mean())
        partial = float(((img != BACKGROUND) & (img != 0x00FFFF)).mean())
        print(f"frame {f}: hit share {share:.3f}, partially covered {partial:.3f}")
        assert 0.10 <= share <= 0.90 and partial >= 0.05, (f, share, partial)
    for f in range(3):
        assert (imgs[f] != imgs[f + 1]).mean() >= 0.05, f
    # the cut tiles are live: the last pixel column and the last row hold hit and partially covered pixels,
    # and so do the rows of the band share (rank 1 of 3, 4-row bands)
    for f, img in enumerate(imgs):
        part = (img != BACKGROUND) & (img != 0x00FFFF)
        assert part[:, W - 1].any() and part[H - 1].any() and part[[4, 5, 6, 7, 16, 17, 18, 19, 28]].mean() >= 0.05, f
    # pixel_from_hits(k, 4), the values test_gbuffer_call_in_between inverts
    assert set(np.unique(np.concatenate(imgs))) <= set(PIXEL_OF_HITS)


# --- GPU ------------------------------------------------------------------------

def whole_rows(bihrt):
    return bihrt.Rows(0, H, BAND, 1)


def new_renderer(bihrt, item_tiles=None):
    g = bihrt.GPUArrayManager(soup())
    if item_tiles is not None:
        g.set_param(bihrt.PARAM_ITEM_TILES, item_tiles)
    return g, bihrt.Renderer(g, W, H, spp=SPP, seed=SEED, camera=to_camera(bihrt, camera()))


def issue(r, first, n, rows, stream=None):
    """One call of n frames from `first` into a fresh buffer (not synchronised)."""
    import torch
    buf = torch.full((n * rows.nrows * W,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if n == 1:
        r.render_device(buf.data_ptr(), first, rows=rows, stream=stream)
    else:
        r.render_device_frames(buf.data_ptr(), first, n, rows.nrows * W, rows=rows, stream=stream)
    return buf


def check(buf, first, n, rows, ys=None):
    got = buf.cpu().numpy().view(U32).reshape(n, rows.nrows, W)
    for j in range(n):
        ref = oracle_frame(first + j)
        ref = ref if ys is None else ref[ys]
        assert np.array_equal(got[j], ref), ("frame", first + j, diff(got[j], ref))


@pytest.mark.gpu
@pytest.mark.parametrize("item_tiles", [1, None], ids=["one_item", "default_split"])
def test_calls_of_16_and_8_frames(item_tiles, gpu, bihrt_mod):
    """One call of 16 frames and one of 8 (the second launch measures the
    tiles' cost: the cost instance), every frame.  PARAM_ITEM_TILES = 1: one
    item carries a tile's state through every frame of the call; the default
    split gives this image one frame per item, each stepping the launch's
    start state to its own frame."""
    import torch
    g, r = new_renderer(bihrt_mod, item_tiles)
    rows = whole_rows(bihrt_mod)
    a = issue(r, 0, 16, rows)
    b = issue(r, 16, 8, rows)
    r.sync()
    torch.cuda.synchronize()
    assert g.bins_stats().usable
    check(a, 0, 16, rows)
    check(b, 16, 8, rows)
    g.close()


@pytest.mark.gpu
def test_stamped_calls(gpu, bihrt_mod):
    """Five calls of 6 frames in a row on one stream, one item per tile: from
    the fourth on the launches are stamped (the state per tile, read from and
    left in the tile's two buffers).  Every frame."""
    import torch
    g, r = new_renderer(bihrt_mod, 1)
    rows = whole_rows(bihrt_mod)
    bufs = [issue(r, 6 * k, 6, rows) for k in range(5)]
    r.sync()
    torch.cuda.synchronize()
    for k, buf in enumerate(bufs):
        check(buf, 6 * k, 6, rows)
    g.close()


@pytest.mark.gpu
def test_calls_alternating_two_streams(gpu, bihrt_mod):
    """Calls of 8, 1, 8, 1, 8 and 8 frames alternating two streams (never
    stamped: the XORWOW ring), one item per tile.  Every frame."""
    import torch
    g, r = new_renderer(bihrt_mod, 1)
    rows = whole_rows(bihrt_mod)
    streams = [torch.cuda.Stream() for _ in range(2)]
    calls, first = [], 0
    for k, n in enumerate((8, 1, 8, 1, 8, 8)):
        calls.append((first, n, issue(r, first, n, rows, stream=streams[k % 2].cuda_stream)))
        first += n
    torch.cuda.synchronize()
    r.sync()
    for f0, n, buf in calls:
        check(buf, f0, n, rows)
    g.close()


@pytest.mark.gpu
def test_second_of_three_band_share(gpu, bihrt_mod):
    """Rank 1 of 3's interleaved 4-row bands: rows 4-7, 16-19 and 28, so the
    rank's last band is cut after one row (its tiles' other lanes lie outside
    the rows).  Calls of 16 and 8 frames, one item per tile, every frame."""
    import torch
    from bihrt.tiling import band_rows, rows_of_rank
    rows, ys = band_rows(H, 4, 1, 3), rows_of_rank(H, 4, 1, 3)
    assert rows.row0 == 4 and rows.nrows == 9 and list(ys[-2:]) == [19, 28]
    g, r = new_renderer(bihrt_mod, 1)
    a = issue(r, 0, 16, rows)
    b = issue(r, 16, 8, rows)
    r.sync()
    torch.cuda.synchronize()
    check(a, 0, 16, rows, ys)
    check(b, 16, 8, rows, ys)
    g.close()


@pytest.mark.gpu
def test_gbuffer_call_in_between(gpu, bihrt_mod):
    """A call of 8 frames, a G-buffer render of frame 8 (its any-hit pass
    through the bins is the kernel's mask instance), a call of 8 frames from
    frame 8: every frame equals the oracle, and the G-buffer's coverage is the
    oracle pixel's hit count."""
    import torch
    g, r = new_renderer(bihrt_mod, 1)
    rows = whole_rows(bihrt_mod)
    a = issue(r, 0, 8, rows)
    r.sync()
    cov = r.render_gbuffer(8, rows=rows, planes=("coverage",))["coverage"]
    b = issue(r, 8, 8, rows)
    r.sync()
    torch.cuda.synchronize()
    check(a, 0, 8, rows)
    check(b, 8, 8, rows)
    want = np.vectorize(PIXEL_OF_HITS.get)(oracle_frame(8)).astype(U32)
    assert np.array_equal(np.asarray(cov).reshape(H, W), want), diff(cov, want)
    g.close()
