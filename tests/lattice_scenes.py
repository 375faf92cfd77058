"""The builder's size and run-layout cases of tests/test_build_edges.py: scenes
whose triangle count N, distinct-code count U and runs of equal Morton codes
are exact by construction, one per tile and level boundary of the build chain
(csrc/bih_build.hip; DESIGN.md, "Builder sizes under test").

A plain helper module: no test lives here.

The lattice.  The Morton code per axis is floor(clamp((c - lo) / (hi - lo) *
1024, 0, 1023)) with c = (tri_lo + tri_hi) / 2.  The scene box here is the
cube [0,4] x [-2,2] x [0,4] (side 4, cell 2^-8), and every triangle's
bounding-box centre is a cell centre, so every f32 step is exact and the code
of each triangle is the interleave of its cell.  Two tiny "pin" triangles,
emitted first, touch the low and the high corner of the box: the box is the
same whatever the codes, pin 0 has code 0 and pin 1 code 2^30 - 1, and each is
a run of one at the first and the last sorted position.  N and U below count
the pins.
"""
import functools

import numpy as np

F32 = np.float32
BOX_LO = np.array([0.0, -2.0, 0.0], F32)
BOX_HI = np.array([4.0, 2.0, 4.0], F32)
CELL = 2.0 ** -8                  # (hi - lo) / 1024
PIN = CELL / 4                    # edge of a pin's bounding box
PIN_CODES = (0, (1 << 30) - 1)
TOP = 1 << 20


def _spread(v):
    """Bit k of v (10 bits) to bit 3k."""
    v = np.asarray(v, np.uint64)
    out = np.zeros_like(v)
    for k in range(10):
        out |= ((v >> np.uint64(k)) & np.uint64(1)) << np.uint64(3 * k)
    return out


def cells_to_codes(ix, iy, iz):
    """30-bit codes of cells (x is the most significant bit of each triple)."""
    return (_spread(ix) << np.uint64(2) | _spread(iy) << np.uint64(1) | _spread(iz)).astype(np.uint32)


def codes_to_cells(codes):
    c = np.asarray(codes, np.uint64)
    out = []
    for sh in (2, 1, 0):
        v = np.zeros_like(c)
        for k in range(10):
            v |= ((c >> np.uint64(3 * k + sh)) & np.uint64(1)) << np.uint64(k)
        out.append(v.astype(np.int64))
    return out


def lattice(codes, e):
    """Float32 (len(codes) + 2, 9): the two pins, then one triangle per entry of
    `codes` (30-bit codes, repeats allowed, in this order) centred on its
    cell's centre with vertices (-e,-e,0), (0,e,0), (e,-e,0) from it -- wound
    to face -z, the side the reference camera is on.  e (a scalar or one per
    entry) is a dyadic number, so that c - e, c + e and their mean are exact;
    every triangle stays inside the box."""
    codes = np.asarray(codes, np.uint32)
    ix, iy, iz = codes_to_cells(codes)
    c = BOX_LO.astype(np.float64) + (np.stack([ix, iy, iz], 1) + 0.5) * CELL
    e = np.broadcast_to(np.asarray(e, np.float64), codes.shape)[:, None]
    off = np.array([[-1, -1, 0], [0, 1, 0], [1, -1, 0]], np.float64)
    v = c[:, None, :] + e[:, None, :] * off[None, :, :]
    assert (v >= BOX_LO).all() and (v <= BOX_HI).all(), "a lattice triangle leaves the box"
    lo, hi = BOX_LO.astype(np.float64), BOX_HI.astype(np.float64)
    pins = np.array([[lo, lo + [PIN, 0, 0], lo + [0, PIN, PIN]],
                     [hi, hi - [PIN, 0, 0], hi - [0, PIN, PIN]]])
    out = np.concatenate([pins.reshape(2, 9), v.reshape(-1, 9)])
    tris = out.astype(F32)
    assert np.array_equal(tris.astype(np.float64), out), "a lattice coordinate is not an f32"
    return tris


def _interior_codes(rng, count, margin):
    """`count` distinct random codes of cells at least `margin` from the border."""
    m = 1024 - 2 * margin
    flat = rng.choice(m ** 3, size=count, replace=False)
    ix, r = np.divmod(flat, m * m)
    iy, iz = np.divmod(r, m)
    return cells_to_codes(ix + margin, iy + margin, iz + margin)


def _margin(e):
    return int(np.ceil(e / CELL)) + 8


def _distinct(n, e, seed):
    """n triangles (pins included), all codes distinct, random input order."""
    rng = np.random.default_rng(seed)
    return _interior_codes(rng, n - 2, _margin(e)), e


def _repeated(counts, e, seed):
    """len(counts) distinct random codes, the k-th smallest counts[k] times, the
    entries in a fixed random order."""
    rng = np.random.default_rng(seed)
    codes = np.sort(_interior_codes(rng, len(counts), _margin(e)))
    full = np.repeat(codes, counts)
    return full[rng.permutation(full.size)], e


def _top_digit_only(e):
    """1024 codes that differ in bits 20..29 only (x bits 6..9, y and z bits
    7..9), 8 copies each: N = 8194."""
    a, b, c = np.meshgrid(np.arange(16), np.arange(8), np.arange(8), indexing="ij")
    codes = cells_to_codes(a.ravel() * 64 + 32, b.ravel() * 128 + 64, c.ravel() * 128 + 64)
    full = np.repeat(codes, 8)
    return full[np.random.default_rng(51).permutation(full.size)], e


def _low_digit_only(e_big):
    """1024 codes that differ in bits 0..9 only (z bits 0..3, x and y bits
    0..2), 8 copies each: an 8 x 8 x 16 block of cells in the middle of the
    box's near face.  N = 8194.  The block is 1/32 wide, so the copies of
    every 16th code are large (e_big) to give the frame something to see, and
    the rest small (more than kBinGlobalMax = 4096 large ones leave the camera
    without frustum bins)."""
    a, b, c = np.meshgrid(np.arange(8), np.arange(8), np.arange(16), indexing="ij")
    codes = cells_to_codes(512 + a.ravel(), 512 + b.ravel(), c.ravel())
    full = np.repeat(codes, 8)
    full = full[np.random.default_rng(52).permutation(full.size)]
    return full, np.where(full % 16 == 0, e_big, 2.0 ** -5)


# name -> () -> (codes in input order, e).  The e of a rendered case is chosen
# so that the reference camera's 48x32 frame has 10-90 % hit pixels.
LATTICE = {}
for _n, _e in ((256, 2.0 ** -2), (257, 2.0 ** -2), (258, 2.0 ** -2), (1024, 2.0 ** -3), (1025, 2.0 ** -3),
               (2047, 2.0 ** -4), (2048, 2.0 ** -4), (2049, 2.0 ** -4), (4095, 2.0 ** -4), (4096, 2.0 ** -4),
               (8193, 2.0 ** -5)):
    LATTICE[f"distinct_{_n}"] = functools.partial(_distinct, _n, _e, 100 + _n % 97)
LATTICE["pow20"] = functools.partial(_distinct, TOP, 2.0 ** -6, 20)
LATTICE["pow20_plus1"] = functools.partial(_distinct, TOP + 1, 2.0 ** -6, 21)
# 1025 codes x 1023 copies + 2 pins = 2^20 + 1 triangles, U = 1027
LATTICE["pow20_plus1_u1027"] = functools.partial(_repeated, [1023] * 1025, 2.0 ** -4, 22)
# Behind the pin at sorted position 0: a first run of 6, then runs of 7, start
# at 7k -- every phase modulo 8, and runs straddle positions 2048 and 4096.
# (With the first run 7 long as well, a run would start exactly at 4096 =
# 1 + 7 * 585 and none would straddle it.)
LATTICE["runs7"] = functools.partial(_repeated, [6] + [7] * 856, 2.0 ** -4, 41)
# a first run of 7, then runs of 8: every later run starts on a multiple of 8,
# one exactly at 2048 and one at 4096
LATTICE["runs8"] = functools.partial(_repeated, [7] + [8] * 749, 2.0 ** -4, 42)
LATTICE["top_digit_only"] = functools.partial(_top_digit_only, 2.0 ** -4)
LATTICE["low_digit_only"] = functools.partial(_low_digit_only, 1.75)

# Few codes, many triangles, no pins: copies of one, two or three fixed
# triangles (conftest's dup_all at size).  name -> (triangles, copies of each);
# the input order is a fixed shuffle.
_T = np.array([-1, -1, 0, 0, 1, 0, 1, -1, 0], np.float64)
FEW = {
    "u1_n5000": ([(2.0, 0.0, 2.0, 1.0)], [5000]),
    "u2_n9000": ([(1.0, 0.0, 2.0, 0.75), (3.0, 0.0, 2.5, 0.75)], [4500, 4500]),
    "u3_n12289": ([(1.0, -0.5, 2.0, 0.75), (3.0, -0.5, 2.5, 0.75), (2.0, 0.75, 3.0, 0.75)], [4096, 4097, 4096]),
}
FEW_CAMERA = ((2.0, 0.0, -0.5), (0.0, 0.0, 1.0))   # camera_cases.look(o, f) of the FEW renders

CASES = list(LATTICE) + list(FEW)
BIG = ("pow20", "pow20_plus1", "pow20_plus1_u1027")        # traced with 256 rays, not rendered
RENDERED = [c for c in CASES if c not in BIG]               # N <= 12289


@functools.lru_cache(maxsize=None)
def codes_of(name):
    """(requested codes in input order (uint32), e) of a lattice case, read-only."""
    codes, e = LATTICE[name]()
    codes = np.ascontiguousarray(codes, np.uint32)
    codes.setflags(write=False)
    return codes, e


def few_counts(name):
    return list(FEW[name][1])


@functools.lru_cache(maxsize=None)
def tris_of(name):
    """Float32 (N, 9), read-only."""
    if name in LATTICE:
        t = lattice(*codes_of(name))
    else:
        shapes, counts = FEW[name]
        base = np.array([np.tile(s[:3], 3) + s[3] * _T for s in shapes]).astype(F32)
        t = np.repeat(base, counts, axis=0)
        t = t[np.random.default_rng(30 + len(counts)).permutation(t.shape[0])]
    t = np.ascontiguousarray(t, F32)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def oracle_tree(name):
    """The case's OracleTree, built once per process and never changed."""
    import oracle
    return oracle.OracleTree(tris_of(name))


def camera(name, w, h):
    """The camera a case is rendered under: float32[12], or None for the
    reference camera (every lattice case)."""
    if name in LATTICE:
        return None
    from camera_cases import look
    return look(FEW_CAMERA[0], FEW_CAMERA[1], w, h)
