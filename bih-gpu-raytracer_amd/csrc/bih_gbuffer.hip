// bih_gbuffer.hip -- G-buffer render (bih_render_gbuffer_device / bih_render_gbuffer,
// include/bih.h): the closest hit of every primary sample of a frame and the
// per-pixel planes resolved from them, in one pass on gfx950.
//
// Semantics: bih_trace's CLOSEST query (section
// 4.5.1, the oracle's traverse_closest) applied to the rays bih_render casts:
// sample (x, y, s) of frame f draws r0, r1 from the pixel's XORWOW state
// (cudaRender's draws 2s, 2s+1 of the frame), u = (x + r0) / w, v = (y + r1) / h,
// d = ((lower_left + u*horizontal) + v*vertical) - origin (camera_dir), o =
// origin, t_lo = 0.  Every f32 expression is the oracle's, in its order
// (-ffp-contract=off).
//
// One wave handles one tile of 64 samples, taken from a global cursor by
// persistent one-wave blocks.  For a power-of-two spp the tile is TileShape's
// TW x TH pixels x spp, lane = pixel_in_tile * spp + s: the layout of the
// frustum bins' per-tile hit mask, whose zero bits are samples proven to miss
// (they get the miss record without a walk).  Any other spp <= 64 packs
// floor(64 / spp) consecutive local pixels into a wave.  The ray is made in
// registers (no ray is written to or read from memory), walked with
// bih_closest.h's walk -- its origin the camera's, straight from the kernel
// arguments (wave-uniform: SGPRs), its t_lo the literal 0 -- and the pixel
// planes come from an in-wave min-reduction of (t bits, s) over the pixel's
// spp adjacent lanes: t > 0, so the f32 bits order as integers.
#include <hip/hip_runtime.h>
#include <float.h>

#include "bih_closest.h"
#include "bih_internal.h"
#include "bih_primary.h"

namespace bih {
namespace {

using dev::kNoHit;

constexpr uint32_t kGT = dev::kLanes;    // threads per block: one wave
// stack slots per lane in LDS: 6 KB per wave, so that the VGPRs (24 waves per
// CU), not LDS, bound the occupancy (10 slots: 25.2 against 24.6 ms)
constexpr int kGLds = 8;

struct GArgs {
    float cam[12];              // origin, lower_left, horizontal, vertical
    uint32_t w, h, spp;
    uint32_t row0, nrows, band_h, band_step;
    uint32_t d_base;            // XORWOW Weyl counter at the start of the frame
    uint32_t tiles_x, ntiles;   // POW2: TW x TH pixel tiles; else waves of ppw pixels
    uint32_t log2spp;           // POW2 only
    uint32_t ppw;               // pixels per wave (not POW2): 64 / spp
    const TreeHeader *hdr;
    const uint4 *nodes;
    const float *tris;          // sorted {v0, e1, e2}
    const uint32_t *dup;
    const uint32_t *tri_idx;    // sorted position -> file order; null: prim is the sorted position
    const uint32_t *rng_in;     // 5 planes of nrows*w: XORWOW v at the start of the frame
    const unsigned long long *hit_mask;   // per tile (POW2), or null: every sample is walked
    uint4 *hits;                // bih_hit[P*spp] or null
    float *depth;               // each plane may be null
    uint32_t *prim;
    float *bary;
    float *normal;
    uint32_t *coverage;
    uint32_t *cursor;           // tiles taken so far (zero at launch)
    uint32_t *spill;
};

// LDS: stack slots per lane kept in LDS.  POW2: spp is a power of two (tiles
// of TW x TH pixels, the hit mask's layout).
template <int LDS, bool POW2>
__global__ void __launch_bounds__(kGT) k_gbuffer(const GArgs a) {
    __shared__ uint32_t s_node[LDS * kGT];
    __shared__ float s_min[LDS * kGT];
    __shared__ float s_max[LDS * kGT];
    const uint32_t lane = threadIdx.x;
    // (the stack's layout is the ray queries', whose spill area this kernel borrows)
    const dev::LaneStack<LDS> stk(s_node, s_min, s_max, a.spill);
    const dev::ClosestScene sc = dev::load_closest_scene(a.hdr, a.nodes, a.tris, a.dup);
    const uint64_t P = (uint64_t)a.nrows * a.w;
    const uint32_t spp = a.spp;
    const bool planes = a.depth || a.prim || a.bary || a.normal || a.coverage;
    // this lane's place in every tile
    uint32_t pix, s;
    if (POW2) {
        pix = lane >> a.log2spp;
        s = lane & (spp - 1u);
    } else {
        pix = lane / spp;
        s = lane - pix * spp;
    }
    const uint32_t base = lane - s;                    // the pixel's first lane
    const unsigned long long gmask = spp >= 64u ? ~0ull : (1ull << spp) - 1ull;
    for (;;) {
        uint32_t tile = 0;
        if (lane == 0) tile = atomicAdd(a.cursor, 1u);
        tile = __builtin_amdgcn_readfirstlane(tile);
        // (ntiles <= 2^32 - 2^20 and each wave overshoots it once: no wrap)
        if (tile >= a.ntiles) break;
        uint32_t x, lr;
        bool valid;
        if (POW2) {
            // TileShape: TW x TH pixels, TW * TH = 64 >> log2(spp)
            const uint32_t lpx = 6u - a.log2spp, ltw = (lpx + 1u) / 2u;
            const uint32_t ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
            x = (tx << ltw) + (pix & ((1u << ltw) - 1u));
            lr = (ty << (lpx / 2u)) + (pix >> ltw);
            valid = x < a.w && lr < a.nrows;
        } else {
            const uint64_t lp0 = (uint64_t)tile * a.ppw + pix;
            valid = pix < a.ppw && lp0 < P;
            lr = (uint32_t)(lp0 / a.w);
            x = (uint32_t)(lp0 - (uint64_t)lr * a.w);
        }
        const uint64_t lp = (uint64_t)lr * a.w + x;
        bool walk = valid;
        if (POW2 && a.hit_mask) walk = valid && ((a.hit_mask[tile] >> lane) & 1ull);
        dev::ClosestRay r;
        r.bt = FLT_MAX;
        r.bi = kNoHit;
        if (walk) {
            // the sample's ray (bih_primary.h): draws 2s, 2s+1 of this pixel's frame
            const uint32_t y = dev::global_row(lr, a.row0, a.band_h, a.band_step);
            dev::primary_dir(a.cam, a.rng_in, P, lp, a.d_base, s, x, y, a.w, a.h, r.d);
            if (dev::closest_start<false>(sc, r, a.cam, 0.0f)) {
                while (!dev::closest_step<false>(sc, r, a.cam, 0.0f, stk)) {}
            }
        }
        // the sample's record: the accepted triangle's test once more (the
        // same inputs and expressions, the same bits), then tri_idx
        const bool hit = walk && r.bi != kNoHit;
        float t = FLT_MAX, u = 0.0f, vv = 0.0f;
        uint32_t prim = kNoHit;
        if (hit) {
            (void)dev::mt_tuv(sc.tris + 9ull * r.bi, a.cam, r.d, t, u, vv);
            prim = a.tri_idx ? a.tri_idx[r.bi] : r.bi;
        }
        if (a.hits && valid)
            a.hits[lp * spp + s] = make_uint4(__float_as_uint(t), __float_as_uint(u), __float_as_uint(vv), prim);
        if (!planes) continue;
        // the pixel's representative sample: min (t bits, s) over its hit samples
        unsigned long long key = hit ? ((unsigned long long)__float_as_uint(t) << 32) | s : ~0ull;
        if (POW2) {
            for (uint32_t off = 1; off < spp; off <<= 1) {
                const unsigned long long o = __shfl_xor(key, (int)off, 64);
                key = o < key ? o : key;
            }
        } else {
            // the pixel's first lane gathers its samples' keys, then hands the minimum back
            unsigned long long m = key;
            for (uint32_t k = 1; k < spp; ++k) {
                const unsigned long long o = __shfl(key, (int)((lane + k) & 63u), 64);
                if (s == 0 && o < m) m = o;
            }
            key = __shfl(m, (int)base, 64);
        }
        const unsigned long long hb = __ballot(hit);
        const uint32_t cov = (uint32_t)__popcll((hb >> base) & gmask);
        if (!valid) continue;
        if (key == ~0ull) {
            if (s != 0) continue;
            if (a.depth) a.depth[lp] = FLT_MAX;
            if (a.prim) a.prim[lp] = kNoHit;
            if (a.bary) { a.bary[2 * lp] = 0.0f; a.bary[2 * lp + 1] = 0.0f; }
            if (a.normal) { a.normal[3 * lp] = 0.0f; a.normal[3 * lp + 1] = 0.0f; a.normal[3 * lp + 2] = 0.0f; }
            if (a.coverage) a.coverage[lp] = 0u;
        } else if (hit && s == (uint32_t)key) {
            if (a.depth) a.depth[lp] = t;
            if (a.prim) a.prim[lp] = prim;
            if (a.bary) { a.bary[2 * lp] = u; a.bary[2 * lp + 1] = vv; }
            if (a.normal) {
                float n[3];
                dev::tri_normal(sc.tris + 9ull * r.bi, n);
                a.normal[3 * lp] = n[0];
                a.normal[3 * lp + 1] = n[1];
                a.normal[3 * lp + 2] = n[2];
            }
            if (a.coverage) a.coverage[lp] = cov;
        }
    }
}

}  // namespace

// Tiles of a launch: for a power-of-two spp TileShape's TW x TH pixel tiles
// over the local rows (*tiles_x across), else waves of 64 / spp local pixels.
uint64_t gbuffer_tiles(uint32_t w, uint32_t nrows, uint32_t spp, uint32_t *tiles_x) {
    if ((spp & (spp - 1)) == 0) {
        const Tiles t = tiles_of(w, nrows, spp);
        *tiles_x = t.x;
        return t.count();
    }
    const uint64_t ppw = 64 / spp;
    *tiles_x = 0;
    return ((uint64_t)nrows * w + ppw - 1) / ppw;
}

int launch_gbuffer(const DeviceTree &t, const RenderArgs &ra, const GBufferPlanes &p,
                   const unsigned long long *hit_mask, const WorkArea &wa, void *stream, bool sorted_prim) {
    const hipStream_t st = (hipStream_t)stream;
    if (ra.nrows == 0 || ra.w == 0 || ra.spp == 0 || ra.spp > 64) return 0;
    const bool pow2 = (ra.spp & (ra.spp - 1)) == 0;
    GArgs a;
    for (int k = 0; k < 12; ++k) a.cam[k] = ra.cam[k];
    a.w = ra.w;
    a.h = ra.h;
    a.spp = ra.spp;
    a.row0 = ra.row0;
    a.nrows = ra.nrows;
    a.band_h = ra.band_h;
    a.band_step = ra.band_step;
    a.d_base = ra.d_base;
    const uint64_t ntiles = gbuffer_tiles(ra.w, ra.nrows, ra.spp, &a.tiles_x);
    if (ntiles > 0xFFFFFFFFull - (1ull << 20)) return (int)hipErrorInvalidValue;
    a.ntiles = (uint32_t)ntiles;
    a.log2spp = pow2 ? (uint32_t)__builtin_ctz(ra.spp) : 0u;
    a.ppw = 64u / ra.spp;
    a.hdr = t.hdr;
    a.nodes = t.nodes;
    a.tris = t.tris_s;
    a.dup = t.dup_cnt;
    a.tri_idx = sorted_prim ? nullptr : t.vals;
    a.rng_in = ra.rng_in;
    a.hit_mask = pow2 ? hit_mask : nullptr;
    a.hits = reinterpret_cast<uint4 *>(p.hits);
    a.depth = p.depth;
    a.prim = p.prim;
    a.bary = p.bary;
    a.normal = p.normal;
    a.coverage = p.coverage;
    a.cursor = wa.word(kCurTaken);
    a.spill = wa.spill;
    hipError_t e = hipMemsetAsync(a.cursor, 0, sizeof(uint32_t), st);
    if (e != hipSuccess) return (int)e;
    const dim3 grid(a.ntiles < wa.max_blocks ? a.ntiles : wa.max_blocks), block(kGT);
    const bool small = wa.lds_slots == (uint32_t)kTraceLdsTest;
    if (small && pow2) hipLaunchKernelGGL((k_gbuffer<kTraceLdsTest, true>), grid, block, 0, st, a);
    else if (small) hipLaunchKernelGGL((k_gbuffer<kTraceLdsTest, false>), grid, block, 0, st, a);
    else if (pow2) hipLaunchKernelGGL((k_gbuffer<kGLds, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_gbuffer<kGLds, false>), grid, block, 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace bih
