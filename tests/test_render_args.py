"""Argument checks of the primary, multi-frame and Whitted render entries and
of bih_reserve (include/bih.h): each entry's checks come, in its own order and
with its own codes, before the tree or a device is touched, so a stand-in tree
pointer is never dereferenced and the test needs no GPU.

The three render entries share the row rule (band_h and band_step non-zero,
the last local row inside the frame) and differ in what they answer first:
the primary and Whitted entries return BIH_OK for nrows == 0 before the band
check and differ in their TOO_LARGE limits (h*w against h*w*spp + 2^20); the
multi-frame entry checks its stride before anything about the rows; and
bih_reserve answers an over-large frame with BIH_ERR_INVALID.
"""
import ctypes as C

import pytest

SEED = 1984
OK, INVALID, TOO_LARGE = 0, -1, -6
BIG = 1 << 16


@pytest.fixture(scope="module")
def env(bihrt_mod):
    L = bihrt_mod._lib.load()
    raw = (C.c_char * 96)()
    base = (C.addressof(raw) + 15) & ~15
    return L, C.c_void_p(base), C.c_void_p(base), bihrt_mod.Camera(), bihrt_mod.Rows, raw


def _ref(x):
    return C.byref(x) if x is not None else None


def _entries(L):
    """name -> call(tree, cam, w, h, spp, rows, out), frame 0."""
    def device(t, c, w, h, spp, rows, out, traverse=0):
        return L.bih_render_device(t, _ref(c), w, h, spp, 0, SEED, _ref(rows), traverse, out, None, None)

    def frames(t, c, w, h, spp, rows, out, nframes=2, stride=64):
        return L.bih_render_device_frames(t, _ref(c), w, h, spp, 0, nframes, SEED, _ref(rows), out, stride, None)

    def whitted(t, c, w, h, spp, rows, out):
        return L.bih_render_whitted_device(t, _ref(c), w, h, spp, 0, SEED, _ref(rows), out, None, None)

    return {"device": device, "frames": frames, "whitted": whitted}


@pytest.mark.parametrize("name", ["device", "frames", "whitted"])
def test_render_entry_checks(env, name):
    L, fake, out, cam, R, _ = env
    call = _entries(L)[name]
    assert call(None, cam, 8, 8, 4, None, out) == INVALID              # NULL tree, camera, out
    assert call(fake, None, 8, 8, 4, None, out) == INVALID
    assert call(fake, cam, 8, 8, 4, None, None) == INVALID
    for whs in ((0, 8, 4), (8, 0, 4), (8, 8, 0)):
        assert call(fake, cam, *whs, None, out) == INVALID
    assert call(fake, cam, 8, 8, 4, R(0, 4, 0, 1), out) == INVALID     # the row rule
    assert call(fake, cam, 8, 8, 4, R(0, 4, 2, 0), out) == INVALID
    assert call(fake, cam, 8, 8, 4, R(6, 4, 4, 1), out) == INVALID
    assert call(fake, cam, 8, 8, 4, R(0, 8, 4, 2), out) == INVALID
    assert call(fake, cam, BIG, BIG, 1, R(BIG, 1, 1, 1), out) == INVALID   # (before TOO_LARGE)
    # an over-large frame: the multi-frame entry's stride check comes first
    assert call(fake, cam, BIG, BIG, 1, None, out) == (INVALID if name == "frames" else TOO_LARGE)
    assert call(fake, cam, 8, 8, 4, R(0, 0, 1, 1), out) == OK          # nothing to do
    assert call(fake, cam, 8, 8, 64, R(3, 0, 0, 0), out) == OK         # (before the band check)


def test_entry_specific_checks(env):
    L, fake, out, cam, R, _ = env
    e = _entries(L)
    assert e["device"](fake, cam, 8, 8, 4, None, out, traverse=2) == INVALID
    # the limits differ: h*w*spp + 2^20 for Whitted, h*w for the primary entry
    assert e["whitted"](fake, cam, 1 << 15, 1 << 15, 4, None, out) == TOO_LARGE
    assert e["device"](fake, cam, 1 << 15, 1 << 15, 4, R(0, 0, 1, 1), out) == OK
    assert e["frames"](fake, cam, 8, 8, 4, None, out, nframes=0) == INVALID
    assert e["frames"](fake, cam, 8, 8, 4, None, out, nframes=65) == INVALID
    assert e["frames"](fake, cam, 8, 8, 4, None, out, stride=63) == INVALID


def test_reserve_checks(env):
    L, fake, _, _, R, _ = env

    def reserve(w, h, spp, rows, max_frames):
        return L.bih_reserve(fake, w, h, spp, _ref(rows), max_frames)

    assert reserve(8, 8, 4, R(0, 4, 0, 1), 1) == INVALID
    assert reserve(BIG, BIG, 1, None, 1) == INVALID      # (not TOO_LARGE)
    assert reserve(8, 8, 4, None, 65) == INVALID
    assert reserve(8, 8, 4, R(0, 0, 0, 0), 1) == OK
