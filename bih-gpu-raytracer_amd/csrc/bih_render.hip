// bih_render.hip -- the any-hit primary-ray render through the frustum bins
// for gfx950 (MI355X), and launch_render.
//
// Kernels
//   k_render_bins      the frustum-bin list walk,
//   k_render_fallback  finishes the packets it left undecided with the exact
//                      per-lane walk (Walker, bih_ray.h).
// Every other render takes the BIH walk kernels (launch_walk, bih_walk.hip).
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdlib.h>

#include <mutex>
#include <stdio.h>
#include <vector>

#include "bih_pixdiv.h"
#include "bih_ray.h"

namespace bih {
namespace {

// Frustum-bin walk (bih_bins.hip): the packet tests the triangles of its
// tile's list and then of the global list with the exact intersector until
// every lane of `live` has a hit.  Each 48-byte entry starts with the
// triangle's edge pre-test (three affine functions of the lane's f32 (u, v),
// each >= 0 whenever MT can accept): a lane failing one skips the triangle,
// and a triangle no remaining lane passes costs no MT.  A lane with a hit
// keeps the entry's leaf in `cand`; returns the lanes with a candidate.  A
// lane of `live` without one has tested every triangle the exact intersector
// could accept for its ray: a proven miss.
// The list is streamed in chunks of 64 entries: lane j loads entry e + j
// (48 bytes, coalesced vector loads), the next chunk is requested before the
// current one is consumed, and the chunk's entries sit in the wave's LDS
// slots (lent) -- one memory round trip per 64 entries instead of one per
// entry.  The tile list's first chunk stays there across an item's frames.
constexpr uint32_t kNoCache = 0xFFFFFFFFu;
constexpr uint32_t kCacheMinLen = 16;   // list entries from which a tile's items use the hit cache
__device__ __forceinline__ void bin_chunk_load(const float4 *ents, uint32_t e, uint32_t end,
                                               uint32_t lane, float4 &c0, float4 &c1, float4 &c2) {
    const uint32_t k = e + lane;
    if (k < end) {
        const float4 *p = ents + (uint64_t)kBinEntryF4 * k;
        c0 = p[0];
        c1 = p[1];
        c2 = p[2];
    }
}
// 16-bit mask of the pixels (4 lanes each, spp 4) that still have a lane in m
__device__ __forceinline__ uint32_t pixels_of(unsigned long long m) {
    m = (m | (m >> 1) | (m >> 2) | (m >> 3)) & 0x1111111111111111ull;
    m = (m | (m >> 3)) & 0x0303030303030303ull;
    m = (m | (m >> 6)) & 0x000F000F000F000Full;
    m = (m | (m >> 12)) & 0x000000FF000000FFull;
    return (uint32_t)((m | (m >> 24)) & 0xFFFFull);
}
// COUNT: count the entries pre-tested and the intersector calls into fc_ent /
// fc_mt (the work a launch that measures tile costs records)
template <bool PMASK, bool COUNT = false>
__device__ __forceinline__ unsigned long long bin_walk(const RenderArgs &a, const cprim_t *prims,
                                                      uint32_t bin, uint32_t e0, uint32_t e1, uint32_t glen,
                                                      float uf, float vf, float dx,
                                                      float dy, float dz, unsigned long long live,
                                                      uint32_t lane, uint32_t &cand, uint32_t &cmeta,
                                                      uint32_t &cent, uint32_t &fc_ent,
                                                      uint32_t &fc_mt, float4 *lent, uint32_t *ltag) {
    // [e0, e1): the tile's list (bin_off[bin], bin_off[bin + 1]) and glen, the
    // global list's length (*bin_gstat; the bins are usable here): the same
    // for every frame of an item, which reads them once
    const float4 *ents = reinterpret_cast<const float4 *>(a.bin_list);
    uint32_t e = e0, end = e1;
    // (opaque per walk: with e0 known before the frame loop the first chunk's
    // entry addresses are hoisted out of it -- two more VGPRs live over the
    // whole item, on top of the root-path check's register peak)
    asm volatile("" : "+s"(e));
    const uint32_t e_first = e;
    unsigned long long rem = live;
    const unsigned long long me = lane_bit(lane);
    // spp 4: an entry whose pixel mask (word 11 >> 16, bih_bins.hip
    // pixel_mask) misses every pixel that still has a lane is skipped
    // before its pre-test
    uint32_t rpix = PMASK ? pixels_of(rem) : 0xFFFFu;
    for (int part = 0; part < 2; ++part) {
        // the tile list's first chunk is still in the wave's LDS slots from
        // the previous frame of this tile (*ltag: the bin it belongs to)
        bool kept = part == 0 && *ltag == bin;
        float4 c0 = make_float4(0.f, 0.f, 0.f, 0.f), c1 = c0, c2 = c0;
        if (e < end && !kept) bin_chunk_load(ents, e, end, lane, c0, c1, c2);
        while (e < end && rem) {
            // d: this chunk; c takes the next one below, before this one is consumed
            const float4 d0 = c0, d1 = c1, d2 = c2;
            const uint32_t n = end - e < 64u ? end - e : 64u;
            // the chunk's entries whose pixel mask meets a pixel that still
            // has a lane, as one ballot (lane j: entry j), walked in order by
            // find-first-set; a hit shrinks rpix and re-filters the rest
            const uint32_t pm =
                (kept ? reinterpret_cast<const uint32_t *>(lent + 3 * lane + 2)[3] : __float_as_uint(d2.w)) >> 16;
            unsigned long long todo = __ballot(lane < n && (!PMASK || (pm & rpix)));
            // the chunk's entries in the wave's LDS slots (lane j: entry j):
            // each pre-test then reads its entry's 9 plane words as one
            // broadcast instead of 9 v_readlane (12 fewer VALU per entry)
            if (!kept) {
                lent[3 * lane] = d0;
                lent[3 * lane + 1] = d1;
                lent[3 * lane + 2] = d2;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                *ltag = (part == 0 && e == e_first) ? bin : ~0u;
            }
            if (e + 64u < end) bin_chunk_load(ents, e + 64u, end, lane, c0, c1, c2);
            // (the loop tests `todo` alone -- `rem` only after a hit, where it
            // can change -- and clears bit j with one s_bitset0: 6 scalar
            // instructions per rejected entry instead of 14)
            while (todo) {
                const uint32_t j = (uint32_t)__builtin_ctzll(todo);
                asm volatile("s_bitset0_b64 %0, %1" : "+s"(todo) : "s"(j));
                const float4 q0 = lent[3 * j], q1 = lent[3 * j + 1];
                const float q2x = reinterpret_cast<const float *>(lent + 3 * j + 2)[0];
                const float f0 = __builtin_fmaf(q0.z, vf, __builtin_fmaf(q0.y, uf, q0.x));
                const float f1 = __builtin_fmaf(q1.y, vf, __builtin_fmaf(q1.x, uf, q0.w));
                const float f2 = __builtin_fmaf(q2x, vf, __builtin_fmaf(q1.w, uf, q1.z));
                const unsigned long long in =
                    rem & __ballot(!(f0 < 0.0f) && !(f1 < 0.0f) && !(f2 < 0.0f));
                BIH_FC(++fc_ent);
                if (COUNT && !BIH_FAST_COUNTERS) ++fc_ent;
                if (!in) continue;
                BIH_FC(++fc_mt);
                if (COUNT && !BIH_FAST_COUNTERS) ++fc_mt;
                // the entry's words 9-11 (triangle, leaf, plan | pixel mask), broadcast
                const float4 q2 = lent[3 * j + 2];
                const uint32_t ti = (a.dbg & 1024u) ? 0u : __builtin_amdgcn_readfirstlane(__float_as_uint(q2.y));
                const unsigned long long h = prim_hits_pre(prim_rec(prims, ti), dx, dy, dz, in);
                if (h & me) {
                    cand = __float_as_uint(q2.z);
                    cmeta = __float_as_uint(q2.w);
                    cent = ti;
                }
                rem &= ~h;
                if (PMASK && h) {
                    rpix = pixels_of(rem);
                    todo &= __ballot((pm & rpix) != 0u);
                }
                // (no lane left: the loop ends on todo -- with PMASK rpix is then
                // 0 and the ballot above already cleared it; one exit keeps the
                // loop free of the structurizer's break flags)
                if (!PMASK && !rem) todo = 0ull;
            }
            e += 64u;
            kept = false;
        }
        if (!rem) break;
        ents = reinterpret_cast<const float4 *>(a.bin_glist);
        e = 0;
        end = glen;
    }
    return live & ~rem;
}

// fast_verify over the leaf's root path from the per-camera path table
// (bih_bins.hip: 32 steps {clip - O[axis] of the side taken, axis | side << 2}
// root-first, end 8, 16 = never verified): the same decisions and intervals,
// with every load's address known up front (no dependent chain).
// The first 24 steps are requested at once (one round trip for most
// leaves), the last 8 only by lanes whose path is longer.
constexpr int kPathBatch = 8;
// One step, without control flow: fast_verify's decisions and intervals for
// a lane still walking (live); the compare bound and the updated end coincide
// (left: neg ? hi : lo, right: neg ? lo : hi -- the bound compared is the
// one the child keeps, the other becomes t)
__device__ __forceinline__ void path_step_flat(uint32_t val, uint32_t meta, float ix, float iy, float iz,
                                               float &lo, float &hi, bool &live, bool &ok) {
    const bool end = (meta & 8u) != 0u;
    const float inv = sel3(meta & 3u, ix, iy, iz);
    const bool neg = 0.0f > inv;
    const float t = __uint_as_float(val) * inv;
    const bool right = (meta & 4u) != 0u;
    const bool use_hi = neg != right;
    const bool gt = t > (use_hi ? hi : lo);
    const bool g = (right ? !gt : gt) != neg;
    ok = ok || (live && end && (meta & 16u) == 0u);
    live = live && !end && g;
    lo = (live && use_hi) ? t : lo;
    hi = (live && !use_hi) ? t : hi;
}
__device__ __forceinline__ bool path_verify(const uint2 *__restrict__ path, uint32_t k, float ix,
                                            float iy, float iz, float lo, float hi) {
    const uint4 *p = reinterpret_cast<const uint4 *>(path + 32ull * k);
    bool live = true, ok = false;
#pragma unroll
    for (int g = 0; g < 24 / kPathBatch; ++g) {
        // kPathBatch steps per round trip (8: 3 rounds, 16 VGPRs of
        // steps live instead of 48 -- that was k_render_bins' register peak:
        // 98 VGPRs and 4 waves per SIMD, now 79 and 6)
        uint4 q[kPathBatch / 2];
#pragma unroll
        for (int j = 0; j < kPathBatch / 2; ++j) q[j] = p[g * (kPathBatch / 2) + j];
#pragma unroll
        for (int j = 0; j < kPathBatch; ++j) {
            const uint4 w = q[j >> 1];
            path_step_flat((j & 1) ? w.z : w.x, (j & 1) ? w.w : w.y, ix, iy, iz, lo, hi, live, ok);
        }
    }
    if (__ballot(live)) {
        uint4 q[4];
        if (live) {
#pragma unroll
            for (int j = 0; j < 4; ++j) q[j] = p[12 + j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint4 w = q[j >> 1];
            path_step_flat((j & 1) ? w.z : w.x, (j & 1) ? w.w : w.y, ix, iy, iz, lo, hi, live, ok);
        }
    }
    return ok;
}

// Ray::Ray (Ray.cu:3-10) + the scene-AABB slab test (CUDAKernels.cu:237-262):
// the ray's inverse direction and [tMin, tMax]; true when the ray meets the
// box.  The reference forms ((neg ? hi : lo) - O) * inv per axis and ray.
// Here the six differences lo - O, hi - O come in already (SlabU: the same
// f32 subtractions of the same operands, formed once per wave), both of an
// axis are multiplied by the inverse and its sign selects between the
// products: (neg ? hi : lo) * i is neg ? hi * i : lo * i, the same multiply
// of the same operands, and a product takes its uniform factor straight from
// a scalar register where the select of two uniform bounds needs both moved
// into vector registers first.
struct SlabU {
    float lo0, lo1, lo2, hi0, hi1, hi2;
};
__device__ __forceinline__ float wave_uniform(float v) {
    return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v)));
}
__device__ __forceinline__ SlabU slab_bounds(const SceneU &sc) {
    SlabU b;
    b.lo0 = wave_uniform(sc.slo0 - sc.ox); b.hi0 = wave_uniform(sc.shi0 - sc.ox);
    b.lo1 = wave_uniform(sc.slo1 - sc.oy); b.hi1 = wave_uniform(sc.shi1 - sc.oy);
    b.lo2 = wave_uniform(sc.slo2 - sc.oz); b.hi2 = wave_uniform(sc.shi2 - sc.oz);
    return b;
}
__device__ __forceinline__ bool scene_slab(const SlabU &b, float dx, float dy, float dz, float &ix,
                                               float &iy, float &iz, float &tMin, float &tMax) {
    ix = 1.0f / dx;
    iy = 1.0f / dy;
    iz = 1.0f / dz;
    const bool nx = ix < 0.0f, ny = iy < 0.0f, nz = iz < 0.0f;
    const float xl = b.lo0 * ix, xh = b.hi0 * ix;
    tMin = nx ? xh : xl;
    tMax = nx ? xl : xh;
    const float yl = b.lo1 * iy, yh = b.hi1 * iy;
    const float tymin = ny ? yh : yl, tymax = ny ? yl : yh;
    bool in_box = !((tMin > tymax) || (tymin > tMax));
    if (tymin > tMin) tMin = tymin;
    if (tymax < tMax) tMax = tymax;
    const float zl = b.lo2 * iz, zh = b.hi2 * iz;
    const float tzmin = nz ? zh : zl, tzmax = nz ? zl : zh;
    in_box = in_box && !((tMin > tzmax) || (tzmin > tMax));
    if (tzmin > tMin) tMin = tzmin;
    if (tzmax < tMax) tMax = tzmax;
    return in_box;
}

// The frame's 2*SPP draws of one pixel state (rs ends at the next frame's
// state), keeping the raw words (xorwow_raw) of draws 2s and 2s+1, the two
// sample s takes.  Samples go in groups of four: the group's pair is selected
// on the two low bits of s (three selects per word), and the group s >> 2
// names keeps it -- no compare per draw.  The caller adds the Weyl counter
// to the two words it keeps instead of to all 2*SPP.
template <uint32_t SPP>
__device__ __forceinline__ void frame_draws(uint32_t rs[5], uint32_t s, uint32_t &xu, uint32_t &xv) {
    constexpr uint32_t G = SPP < 4u ? SPP : 4u;
    const bool b0 = (s & 1u) != 0u, b1 = (s & 2u) != 0u;
#pragma unroll 1
    for (uint32_t g = 0; g < SPP / G; ++g) {
        uint32_t u[G], v[G];
#pragma unroll
        for (uint32_t j = 0; j < G; ++j) {
            u[j] = dev::xorwow_raw(rs);
            v[j] = dev::xorwow_raw(rs);
        }
        uint32_t gu = u[0], gv = v[0];
        if (G == 2u) {
            gu = b0 ? u[G - 1] : u[0];
            gv = b0 ? v[G - 1] : v[0];
        } else if (G == 4u) {
            const uint32_t ul = b0 ? u[1] : u[0], uh = b0 ? u[G - 1] : u[G / 2];
            const uint32_t vl = b0 ? v[1] : v[0], vh = b0 ? v[G - 1] : v[G / 2];
            gu = b1 ? uh : ul;
            gv = b1 ? vh : vl;
        }
        if (SPP <= 4u || (s >> 2) == g) {
            xu = gu;
            xv = gv;
        }
    }
}

// The same at 4 spp, where a quad of lanes (lane = pix * 4 + s) is one pixel:
// its four lanes hold the same state and share the work of the 8 steps.
// With o_1..o_8 the frame's outputs and rs = (o_-4..o_0), a step is
//   o_n = A(o_{n-1}) ^ B(o_{n-5}),  A(v) = v ^ (v << 4),
//   B(x) = t ^ (t << 1) with t = x ^ (x >> 2)            (dev::xorwow_raw).
// The A chain is sequential and every lane computes it: each needs o_4..o_8
// as the next state and its own two draws.  The eight B terms do not depend
// on the chain, except that B_6..B_8 take o_1..o_3, which every lane has by
// then: lane s computes B_{s+1} = B(rs[s]) and B_{s+5} = B(o_s), and step n
// takes its term from lane (n - 1) & 3 of its quad (a quad-permute DPP
// operand).  XOR is associative: the words are the same bits.
// `own` is rs[s], which the caller reads from the lane's LDS column.
// Every lane of a quad must be active: a DPP operand from an inactive lane
// reads 0.  The caller's `valid` is a property of the pixel (x < w and
// lr < nrows, in cut tiles and row bands alike), so a quad's four lanes enter
// together or not at all.
template <uint32_t K>
__device__ __forceinline__ uint32_t quad_lane(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, (int)(K * 0x55u), 0xf, 0xf, true);
}
__device__ __forceinline__ uint32_t xorwow_b(uint32_t x) {
    const uint32_t t = x ^ (x >> 2);
    return t ^ (t << 1);
}
__device__ __forceinline__ uint32_t xorwow_a(uint32_t v) { return v ^ (v << 4); }
__device__ __forceinline__ void frame_draws_quad(uint32_t rs[5], uint32_t own, uint32_t s, uint32_t &xu,
                                                 uint32_t &xv) {
    const bool b0 = (s & 1u) != 0u, b1 = (s & 2u) != 0u;
    const uint32_t lo = xorwow_b(own);                       // B_{s+1}
    const uint32_t o1 = xorwow_a(rs[4]) ^ quad_lane<0>(lo);
    const uint32_t o2 = xorwow_a(o1) ^ quad_lane<1>(lo);
    const uint32_t o3 = xorwow_a(o2) ^ quad_lane<2>(lo);
    const uint32_t o4 = xorwow_a(o3) ^ quad_lane<3>(lo);
    const uint32_t hl = b0 ? o1 : rs[4], hh = b0 ? o3 : o2;
    const uint32_t hi = xorwow_b(b1 ? hh : hl);              // B_{s+5}
    const uint32_t o5 = xorwow_a(o4) ^ quad_lane<0>(hi);
    const uint32_t o6 = xorwow_a(o5) ^ quad_lane<1>(hi);
    const uint32_t o7 = xorwow_a(o6) ^ quad_lane<2>(hi);
    const uint32_t o8 = xorwow_a(o7) ^ quad_lane<3>(hi);
    rs[0] = o4; rs[1] = o5; rs[2] = o6; rs[3] = o7; rs[4] = o8;
    const uint32_t ul = b0 ? o3 : o1, uh = b0 ? o7 : o5;
    const uint32_t vl = b0 ? o4 : o2, vh = b0 ? o8 : o6;
    xu = b1 ? uh : ul;
    xv = b1 ? vh : vl;
}

// A plan's 1-2 critical comparisons (meta & 3 of them) on its values v
__device__ __forceinline__ bool plan_values_check(uint32_t meta, const float4 v, float ix, float iy, float iz,
                                                  float tMin, float tMax) {
    const uint32_t n = meta & 3u;
    bool ok = true;
#pragma unroll
    for (uint32_t c = 0; c < 2; ++c) {
        if (c >= n) break;
        const uint32_t m = meta >> (2 + 6 * c);
        const float vk = c ? v.z : v.x, vp = c ? v.w : v.y;
        const float tk = vk * sel3(m & 3u, ix, iy, iz);
        const bool is_exit = (m & 4u) != 0u;
        const float tp = (m & 32u) ? (is_exit ? tMin : tMax) : vp * sel3((m >> 3) & 3u, ix, iy, iz);
        ok = ok && (is_exit ? (tk > tp) : !(tk > tp));
    }
    return ok;
}

// The candidate's verification plan (triangle_plan, bih_bins.hip): the
// entry's leaf carries bit 31 when every decision on its root path is
// proven; otherwise meta & 3 = 1-2 critical comparisons, each t_k against
// t_p (another plane on the path, or the slab test's tMin / tMax), whose
// operands sit in the entry's last 16 bytes; 3 = the full root-path check.
__device__ __forceinline__ bool plan_verify(const RenderArgs &a, uint32_t cand, uint32_t meta,
                                            uint32_t cent, float ix, float iy, float iz, float tMin,
                                            float tMax) {
    if (cand >> 31) return true;
    meta &= 0xFFFFu;                   // (bits 16-31: the entry's pixel mask)
    const uint32_t n = meta & 3u;
    if (n == 3u) return path_verify(a.bin_path, cand, ix, iy, iz, tMin, tMax);
    // the triangle's plan values (its k_bin_fp record; the same in every list)
    return plan_values_check(meta, reinterpret_cast<const float4 *>(a.bin_rec)[4ull * cent + 3], ix, iy, iz,
                             tMin, tMax);
}

// ---------------------------------------------------------------------------
// k_render_bins: the any-hit render through the frustum bins alone (no BIH
// walk in this kernel).  Persistent waves draw items from the launch's tile
// queue (launch_bin_queue, bih_bins.hip): a wave starts in its XCD's band of
// tile rows and moves on to the others when that band is drained.  An item is
// a live tile -- one 64-ray packet: jitter, camera ray, scene slab test,
// bin_walk over the tile's list, plan_verify of each lane's candidate -- or
// 64 background tiles (one per lane), which no triangle's footprint touches.
// A packet whose lanes all end as a verified hit or a proven miss writes its
// pixels; a packet with a lane left undecided (a candidate the plan or the
// root-path check rejects, or a single-leaf scene) appends {tile, undecided,
// hits} to the slot's fallback list, and k_render_fallback finishes it with
// the exact walk.  Registers stay those of the list walk (no BIH walk state).
// Queue state (a "head set", kBinSetWords, zero at launch; the launch zeroes
// the slot's other set for its next launch): 8 band heads and the fallback
// count, then per-CU slots like TileQueue's -- a wave claims a position of
// its CU's current batch of kBinBatch consecutive items with one atomicAdd
// on the CU's own 128-byte line, and the wave that drains a batch refills
// the slot from a band head.  One device-wide atomic per batch instead of
// one per item: a single head word saturates near 90 dequeues per us.
// ---------------------------------------------------------------------------
#if BIH_BINS_TIMELINE
// {wave | xcc << 24 | kind << 28, start, duration, list length} per queue
// item (s_memrealtime, 100 MHz); kind 0 live item, 1 background or advance
// item (length 1), 2 wave start, 3 wave exit.  Each wave appends to its own
// run of kTlPerWave records (no shared counter: a single atomic word would
// serialise the items, ~90 per us); g_tl_n[wave] counts them.
constexpr uint32_t kTlWaves = 1u << 14, kTlPerWave = 62;
__device__ uint32_t g_tl_n[kTlWaves];
__device__ uint4 g_tl_rec[kTlWaves * kTlPerWave];
__device__ __forceinline__ void tl_rec(uint32_t lane, uint32_t kind, uint64_t t0, uint64_t t1, uint32_t len) {
    const uint32_t wv = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (lane == 0 && wv < kTlWaves) {
        const uint32_t k = g_tl_n[wv]++;
        if (k < kTlPerWave)
            g_tl_rec[wv * kTlPerWave + k] = make_uint4(wv | (xcc_id() << 24) | (kind << 28), (uint32_t)t0,
                                                       (uint32_t)(t1 - t0), len);
    }
}
#endif
#if BIH_PHASES
// The root-path check's load at its two sites (0: the hit-cache retest, 1:
// after the walk), work[76 + 4 * site ..]: {tile-frames with a lane that needs
// it, those lanes, the most lanes of one tile-frame, tile-frames with more
// than 16 of them}; bih_sync prints them ("bin-pathcheck")
__device__ __forceinline__ void path_site_count(const RenderArgs &a, uint32_t site, unsigned long long need,
                                                uint32_t lane) {
    const uint32_t n = (uint32_t)__popcll(need);
    if (n && lane == 0) {
        atomicAdd(a.work + 76 + 4 * site, 1u);
        atomicAdd(a.work + 77 + 4 * site, n);
        atomicMax(a.work + 78 + 4 * site, n);
        if (n > 16u) atomicAdd(a.work + 79 + 4 * site, 1u);
    }
}
#endif
constexpr uint32_t kFbWords = 8;   // fallback record: tile, undecided lo/hi, hits lo/hi, pad
constexpr uint32_t kBinBatch = 8;   // A/B (16 frames per call): 8 0.0464 ms per frame, 16 0.0471, 32 0.0482
constexpr uint32_t kBinSlot0 = 16 * 32;   // words: heads at b * 32, fallback count at 8 * 32
struct BinQueue {
    const uint4 *hdr;                  // per band {start, live, bg, items}
    uint32_t *set;
    unsigned long long *slot;
    uint32_t band, left;
    uint4 hb;                          // header of the band of the item next() returned
    // items per live tile: ns (RenderArgs::nsplit, frame ranges of a.fpi
    // frames); the band's first heavy[b] tiles take hs each instead
    // (RenderArgs::hsplit); a background item covers 64 tiles in every
    // frame.  hv = the heavy count of the band of the item next() returned
    // (the heavy counts follow the 8 band headers: launch_bin_queue's kQHeavy)
    uint32_t ns, hs, hv;
    __device__ __forceinline__ uint32_t extra(uint32_t b) const {
        return hs != ns ? reinterpret_cast<const uint32_t *>(hdr + 8)[b] : 0u;
    }
    __device__ __forceinline__ uint32_t band_items(const uint4 &h, uint32_t x) const {
        return x * hs + (h.y - x) * ns + (h.w - h.y);
    }
    // Start-up without atomics: each wave's first `rounds` items are static
    // -- in round r, block k's waves take items r * W(b) + (k >> 3) * 4 + w
    // of band b = k & 7, W(b) the band's waves (blocks are dealt round-robin
    // over the XCDs, so that is mostly the XCD's own band; only the speed
    // depends on it) -- and the band heads hand out the items after those:
    // stat(b) per band.  (Every wave starting in the per-CU slot made the 24
    // waves of a CU wait for three serial refills: 5.6 us median to a wave's
    // first item in a one-frame launch, 12 us at q90.)  rounds = 0 with a
    // shared grid, whose heads then hand out every item.
    uint32_t rounds, round;
    __device__ __forceinline__ uint32_t band_waves(uint32_t b) const {
        return gridDim.x > b ? ((gridDim.x - b + 7u) >> 3) * (kThreads / 64) : 0u;
    }
    __device__ __forceinline__ uint32_t stat(uint32_t b) const { return rounds * band_waves(b); }

    // next item: band (this->hb / band) and index within the band
    __device__ bool next(uint32_t lane, uint32_t &item) {
        if (round < rounds) {
            const uint32_t b = blockIdx.x & 7u;
            const uint32_t idx = round * band_waves(b) + (blockIdx.x >> 3) * (kThreads / 64) +
                                 __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
            ++round;
            const uint4 h = hdr[b];
            const uint32_t x = extra(b);
            if (idx < band_items(h, x)) {
                hb = h;
                hv = x;
                item = idx;
                return true;
            }
            round = rounds;   // (the band's items end before this wave's next round)
        }
        for (;;) {
            unsigned long long v = 0;
            if (lane == 0) v = atomicAdd(slot, 1ull);
            const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
            const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
            if (hi == 0xFFFFFFFFu) return false;
            if (hi != 0 && lo < kBinBatch) {
                const uint32_t b = (hi - 1u) >> 24, start = ((hi - 1u) & 0xFFFFFFu) * kBinBatch + stat(b);
                hb = hdr[b];
                hv = extra(b);
                if (start + lo < band_items(hb, hv)) {
                    item = start + lo;
                    band = b;
                    return true;
                }
                continue;                                // past the band's end
            }
            if ((hi == 0 && lo == 0) || (hi != 0 && lo == kBinBatch)) {
                while (left) {
                    const uint4 h = hdr[band];
                    const uint32_t x = extra(band);
                    uint32_t c = 0;
                    if (lane == 0) c = atomicAdd(set + band * 32, kBinBatch);
                    c = __builtin_amdgcn_readfirstlane(c);
                    if (c + stat(band) < band_items(h, x)) {
                        if (lane == 0)
                            atomicExch(slot, ((unsigned long long)(((band << 24) | (c / kBinBatch)) + 1u) << 32) | 1ull);
                        hb = h;
                        hv = x;
                        item = c + stat(band);
                        return true;
                    }
                    band = (band + 1u) & 7u;
                    --left;
                }
                if (lane == 0) atomicExch(slot, kSlotDone);
                return false;
            }
            __builtin_amdgcn_s_sleep(2);                 // another wave is refilling
        }
    }
};
// MODE 1: also write the per-tile hit masks (RenderArgs::hit_mask; the C4
// primary pass); MODE 2: also record each live tile's cycles per frame
// (RenderArgs::bin_cost; the launch after which the queue is ordered by
// measured cost); | kBinsStamped: the XORWOW state per tile
// (RenderArgs::stamps) -- separate instantiations, so the headline kernel
// keeps its registers
constexpr int kBinsStamped = 4;
template <int LOG2SPP, int MODE = 0>
__global__ void __launch_bounds__(kThreads, 1) k_render_bins(const RenderArgs a) {
    constexpr bool MASK = (MODE & 3) == 1, COST = (MODE & 3) == 2, STAMP = (MODE & kBinsStamped) != 0;
    constexpr uint32_t SPP = 1u << LOG2SPP;
    constexpr uint32_t TW = TileShape<LOG2SPP>::TW, TH = TileShape<LOG2SPP>::TH;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    __shared__ uint32_t s_rs[5][kThreads];   // each lane's XORWOW state between the frames of an item
    __shared__ uint32_t s_hc[3][kThreads];   // each lane's hit of the item's previous frame: {record, leaf, plan}
    __shared__ float4 s_ent[kThreads / 64][64 * 3];   // per wave: the list chunk bin_walk pre-tests
    float4 *const lent = s_ent[tid >> 6];
    uint32_t ltag = ~0u;   // the bin whose list's first chunk is in lent
    // the slot's next launch starts from a zeroed set: every one of the 1024
    // per-CU slot lines (cu_key() spans 0..1023 sparsely, whatever the grid)
    if (tid == 0)
        for (uint32_t k = blockIdx.x; k < 1024u; k += gridDim.x)
            *reinterpret_cast<unsigned long long *>(a.bin_heads_next + kBinSlot0 + k * 32) = 0ull;
    if (tid == 0)
        for (uint32_t k = blockIdx.x; k < 9u; k += gridDim.x) a.bin_heads_next[k * 32] = 0u;
    const SceneU sc = load_scene(a);
    const SlabU slab = slab_bounds(sc);
    const cprim_t *prims = (const cprim_t *)(const void *)a.tri_prim;
    const uint32_t tiles_x = (a.w + TW - 1) / TW;
    const float fw = (float)a.w, fh = (float)a.h;
    // the image's reciprocals, correctly rounded, once per wave (pixel_divide)
    const float yw = 1.0f / fw, yh = 1.0f / fh;
    const bool recip = a.w <= kPixelDivideMax && a.h <= kPixelDivideMax;
    const uint32_t pix = lane >> LOG2SPP;
    const uint32_t misspix = pixel_from_hits(0u, SPP), solidpix = pixel_from_hits(SPP, SPP);
    // the bins' status word (k_bin_status wrote it before this launch, nothing
    // writes it during one): read once per wave, as a scalar.  bins_ok: the
    // lists were built; else the exact walk decides
    const uint32_t gstat = ((const cu32_t *)(const void *)a.bin_gstat)[0];
    const bool bins_ok = gstat != kBinsUnusable;
    BinQueue q;
    q.hdr = reinterpret_cast<const uint4 *>(a.bin_qhdr);
    q.set = a.bin_heads;
    q.slot = reinterpret_cast<unsigned long long *>(a.bin_heads + kBinSlot0 + cu_key() * 32);
    q.band = xcc_id();
    q.left = 8;
    // (not while another render holds CU slots: this launch's blocks then
    // start as that one's waves exit, and a late block's static item -- the
    // band's costliest first -- would start late)
    q.rounds = a.shared_grid ? 0u : a.static_rounds;
    q.round = 0;
    q.ns = a.nsplit;   // an item covers a tile in a.fpi consecutive frames of the launch
    q.hs = a.hsplit;
    q.hv = 0;
    uint32_t fpi = a.fpi;
    if (a.live_items && a.nframes > 1u) {
        // items per live tile from the queue's live count (the same in every
        // wave): a launch over few live tiles -- a small mesh, a rank's bands
        // -- splits its tiles' frames so that the items still outnumber the
        // waves; one over many keeps every frame of a tile in one item
        uint32_t live = 0;
        for (uint32_t b = 0; b < 8u; ++b) live += q.hdr[b].y;
        const uint32_t target = a.live_items & 0x7FFFFFFFu;
        uint32_t ns = live ? (target + live / 2u) / live : a.nframes;
        ns = ns < 1u ? 1u : (ns > a.nframes ? a.nframes : ns);
        fpi = (a.nframes + ns - 1u) / ns;
        ns = (a.nframes + fpi - 1u) / fpi;
        const uint32_t hx = ns * (a.nframes >= 8u ? 4u : 2u);
        q.ns = ns;
        q.hs = (a.live_items >> 31) ? (hx < a.nframes ? hx : a.nframes) : ns;
        if (q.hs < ns) q.hs = ns;
    }
    const uint32_t fhv = (a.nframes + q.hs - 1u) / q.hs;   // frames per item of a heavy tile
    // (as ns above: only the items that have a frame -- 16 frames in 12 items
    // of 2 left four of them empty; hs == ns then means no heavy tiles, extra())
    q.hs = (a.nframes + fhv - 1u) / fhv;
    uint32_t it = 0;
#if BIH_FAST_COUNTERS
    // item counters (bih_sync prints them, "bin-items"), work[kItemWord ..]:
    // the split this launch uses and the queue's live and heavy counts, then
    // what lane 0 of every item counts
    if (blockIdx.x == 0 && tid == 0) {
        uint32_t live = 0, heavy = 0;
        for (uint32_t b = 0; b < 8u; ++b) {
            live += q.hdr[b].y;
            heavy += q.extra(b);
        }
        const uint32_t v[9] = {a.nframes, q.ns, fpi, q.hs, fhv, STAMP ? 1u : 0u, COST ? 1u : 0u, live, heavy};
        for (uint32_t k = 0; k < 9u; ++k) a.work[kItemWord + k] = v[k];
        a.work[kItemWord + 15] = a.bin_qhdr[kBinQSolidWord];   // the queue's solid tiles
    }
#endif
#if BIH_PHASES
    // per-phase wave cycles (s_memtime), summed over waves into work[64..75]
    unsigned long long ph[6] = {0, 0, 0, 0, 0, 0};   // queue, background, setup, walk, verify, write
    uint64_t tq = __builtin_amdgcn_s_memtime();
#define BIH_PH(k) do { const uint64_t t_ = __builtin_amdgcn_s_memtime(); ph[k] += t_ - tq; tq = t_; } while (0)
#else
#define BIH_PH(k) do { } while (0)
#endif
#if BIH_BINS_TIMELINE
    const uint64_t tl_w0 = __builtin_amdgcn_s_memrealtime();
    tl_rec(lane, 2u, tl_w0, tl_w0, 0u);
#endif
    while (q.next(lane, it)) {
        BIH_PH(0);
#if BIH_BINS_TIMELINE
        const uint64_t tl_t0 = __builtin_amdgcn_s_memrealtime();
#endif
        const uint4 hb = q.hb;
        // an item covers its tile in frames [f0, nf) of the launch: the
        // band's first hv tiles (measured cost >= kHeavyFactor x the mean)
        // hs items each, frames [sp * fhv, (sp + 1) * fhv), so that no tile's
        // frames run for most of the launch on one wave; the other live tiles
        // ns items of a.fpi frames each -- tile-major, so the queue's LPT
        // order holds for the items; then the background items (`it` past
        // hb.y: 64 tiles each, every frame)
        uint32_t f0 = 0, nf = a.nframes;
#if BIH_FAST_COUNTERS
        const bool ic_heavy = it < q.hv * q.hs;
#endif
        if (q.ns > 1u || q.hv) {   // (one item per tile: `it` is the tile's position already)
            const uint32_t hx = q.hv * q.hs;
            if (it < hx) {
                const uint32_t j = it / q.hs, sp = it - j * q.hs;
                it = j;
                f0 = sp * fhv;
                nf = f0 + fhv < a.nframes ? f0 + fhv : a.nframes;
            } else {
                const uint32_t k = it - hx, nx = (hb.y - q.hv) * q.ns;
                if (k < nx) {
                    const uint32_t j = k / q.ns, sp = k - j * q.ns;
                    it = q.hv + j;
                    f0 = sp * fpi;
                    nf = f0 + fpi < a.nframes ? f0 + fpi : a.nframes;
                } else {
                    it = hb.y + (k - nx);
                }
            }
        }
#if BIH_FAST_COUNTERS
        if (lane == 0) {
            if (it < hb.y) {
                atomicAdd(a.work + kItemWord + 9, 1u);
                if (f0 > 0u) atomicAdd(a.work + kItemWord + 10, 1u);
                if (ic_heavy) atomicAdd(a.work + kItemWord + 11, 1u);
                if (f0 >= nf) atomicAdd(a.work + kItemWord + 12, 1u);
                else atomicAdd(a.work + kItemWord + 13, nf - f0);
            } else {
                const uint32_t k0 = (it - hb.y) * 64u;
                const uint32_t n = k0 < hb.z ? (hb.z - k0 < 64u ? hb.z - k0 : 64u) : 0u;
                atomicAdd(a.work + kItemWord + 14, n * (nf - f0));
            }
        }
#endif
        if (it >= hb.y) {
            // background: every sample misses (Color's background), whatever its jitter;
            // a solid tile (kQueueSolid: launch_bin_queue): every sample of every
            // pixel hits, whatever its jitter -- the constant of SPP hits, and the
            // hit mask the live path would write (its valid lanes)
            const uint32_t k = (it - hb.y) * 64u + lane;
            if (k < hb.z && !(a.dbg & 1u)) {
                const uint32_t tq = a.bin_queue[hb.x + hb.y + k];
                const uint32_t t = tq & ~kQueueSolid;
                const bool solid = (tq & kQueueSolid) != 0u;
                const uint32_t ty = t / tiles_x, tx = t - ty * tiles_x;
                const uint32_t x0 = tx * TW;
                if (MASK) {                          // (one-frame launches)
                    unsigned long long hm = 0ull;
                    if (solid) {
                        const unsigned long long m = (SPP == 64) ? ~0ull : ((1ull << SPP) - 1ull);
                        for (uint32_t p = 0; p < 64u / SPP; ++p)
                            if (x0 + p % TW < a.w && ty * TH + p / TW < a.nrows) hm |= m << (p * SPP);
                    }
                    a.hit_mask[t] = hm;
                }
                const uint32_t bgpix = solid ? solidpix : misspix;
                for (uint32_t fj = f0; fj < nf; ++fj) {
                    uint32_t *const fout = a.out + (uint64_t)fj * a.out_stride;
                    for (uint32_t r = 0; r < TH; ++r) {
                        const uint32_t lr = ty * TH + r;
                        if (lr >= a.nrows) break;
                        uint32_t *o = fout + (uint64_t)lr * a.w + x0;
                        if (TW == 4 && x0 + 4 <= a.w && ((uintptr_t)o & 15u) == 0) {
                            *reinterpret_cast<uint4 *>(o) = make_uint4(bgpix, bgpix, bgpix, bgpix);
                        } else {
                            for (uint32_t c = 0; c < TW && x0 + c < a.w; ++c) o[c] = bgpix;
                        }
                    }
                }
            }
            BIH_PH(1);
#if BIH_BINS_TIMELINE
            tl_rec(lane, 1u, tl_t0, __builtin_amdgcn_s_memrealtime(), 0u);
#endif
            continue;
        }
        if (a.dbg & 2u) continue;
        const uint32_t tile = a.bin_queue[hb.x + it];
        uint32_t x, lr, s;
        ray_coords<LOG2SPP>((uint64_t)tile * 64 + lane, tiles_x, x, lr, s);
        const bool valid = x < a.w && lr < a.nrows;
        const uint64_t lp = (uint64_t)lr * a.w + x;
        const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const uint32_t bin = (global_row(ty * TH, a.row0, a.band_h, a.band_step) / TH) * a.bins_x + tx;
        const uint32_t y = global_row(lr, a.row0, a.band_h, a.band_step);
        // the pixel's XORWOW state at the start of the launch's first frame;
        // each frame takes 2*SPP draws (cudaRender), sample s the draws
        // 2s+1 and 2s+2 of its frame
        // (kept in LDS between frames: registers stay those of the list walk)
        uint32_t dfr = a.d_base + f0 * (2u * SPP * kWeyl);   // Weyl counter at the start of frame fj
        if (valid) {
            // frame f0's state: the launch's first frame's stepped 2*SPP*f0
            // draws on (a later item split or a heavy tile's later frame
            // range: at most ~100 steps, against the frames the item renders)
            const uint64_t P = (uint64_t)a.nrows * a.w;
            const uint32_t *src = a.rng_in;
            uint32_t pre = 2u * SPP * f0;
            if (STAMP) {
                // the tile's stamped state, stepped to frame st_f0 + f0
                const StampBase sb = stamp_base(a.stamps[tile], a.st_seq);
                src = sb.b ? a.st_buf1 : a.st_buf0;
                pre = 2u * SPP * (a.st_f0 + f0 - sb.F);
            }
            uint32_t v[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) v[i] = src[(uint64_t)i * P + lp];
            xorwow_steps(v, pre);
#pragma unroll
            for (int i = 0; i < 5; ++i) s_rs[i][tid] = v[i];
        }
        s_hc[0][tid] = kNoCache;
        // (tiles with short lists: the walk finds a lane's triangle about as
        // fast as the cache test would -- a record gather and a full
        // intersector call per lane -- so they walk every frame)
        // the tile's list [le0, le1) of bin_list: read once per item (bin_walk
        // read both offsets again at the start of every frame's walk)
        const uint32_t le0 = ((const cu32_t *)(const void *)a.bin_off)[bin],
                       le1 = ((const cu32_t *)(const void *)a.bin_off)[bin + 1];
        const bool use_cache = le1 - le0 >= kCacheMinLen;
        // the Weyl counter's offset at this lane's first draw of a frame
        // (frame_draws): draw 2s returns its raw word + dfr + wo, draw 2s+1
        // that + kWeyl
        const uint32_t wo = (2u * s + 1u) * kWeyl;
        // the lane's hit of the tile's last item (an earlier launch of this
        // camera set's current queue, RenderArgs::hcache): valid while the
        // tile's stamp is the queue's sequence number; the triangle's leaf
        // word and plan come from its record (the words every list entry of
        // the triangle carries)
        // A stale id is sound: the cache only chooses which triangle a lane
        // tries first.  Every cached id is re-tested on the new ray by the
        // exact intersector on the current soup's record and then by that
        // record's own plan (the frame loop below), so an id left by another
        // queue, camera or soup -- or read next to a stamp another item of
        // the tile just wrote, there is no ordering between the two -- either
        // proves a hit Color() would find or leaves the lane to the list
        // walk; only ti < n_tris is needed to read it.
        // (tests/test_item_splits.py::test_hit_cache_sequence)
        if (use_cache && a.hcache && valid && a.hstamp[tile] == a.hseq) {
            const uint32_t ti = a.hcache[(uint64_t)tile * 64 + lane];
            if (ti < a.hdr_n_tris) {
                const float4 m = reinterpret_cast<const float4 *>(a.bin_rec)[4ull * ti + 2];
                s_hc[0][tid] = ti;
                s_hc[1][tid] = __float_as_uint(m.z);
                s_hc[2][tid] = __float_as_uint(m.w);
            }
        }
        // (measuring launches) the item's work: entries pre-tested + 4 x
        // intersector calls -- each call a dependent scalar load of the
        // record, which is what makes a tile slow; wall time on a SIMD shared
        // with five other waves orders the tiles worse
        uint32_t work = 0;
#if BIH_BINS_TIMELINE
        uint32_t tl_ent = 0, tl_mt = 0, tl_pv = 0, tl_pl = 0;   // per item: entries, intersector calls, lanes
                                                               // through the path table / a plan
#endif
        for (uint32_t fj = f0; fj < nf; ++fj, dfr += 2u * SPP * kWeyl) {
            uint32_t *const fout = a.out + (uint64_t)fj * a.out_stride;
            float dx = 0.f, dy = 0.f, dz = 1.f, uf = 0.f, vf = 0.f;
            if (valid) {
                // the frame's 2*SPP draws on every lane (uniform control
                // flow); rs ends at the next frame's state
                // (the two words this sample takes are converted to floats,
                // not all 2*SPP: curand_uniform of the same words)
                // (and only those two get the Weyl counter added -- the add
                // is modulo 2^32 and commutes with the select)
                uint32_t xu = 0u, xv = 0u;
                uint32_t rs[5];
#pragma unroll
                for (int i = 0; i < 5; ++i) rs[i] = s_rs[i][tid];
                if constexpr (SPP == 4u) {
                    // (a quad is one pixel: ray_coords' lane = pix * SPP + s)
                    static_assert(LOG2SPP == 2 && kThreads % 64 == 0, "a quad of lanes is one pixel");
                    frame_draws_quad(rs, s_rs[s][tid], s, xu, xv);
                } else {
                    frame_draws<SPP>(rs, s, xu, xv);
                }
                xu += dfr + wo;
                xv += dfr + wo + kWeyl;
                const float ru = dev::xorwow_to_uniform(xu), rv = dev::xorwow_to_uniform(xv);
                if (fj + 1u < nf) {
#pragma unroll
                    for (int i = 0; i < 5; ++i) s_rs[i][tid] = rs[i];
                } else if (STAMP && nf == a.nframes && s == 0u) {
                    // stamped: the state after the launch's last frame
                    // (cudaRender's write-back, CUDAKernels.cu:419) into the
                    // tile's other buffer; other items of the tile read the
                    // base buffer, which nobody writes in this launch
                    const StampBase sb = stamp_base(a.stamps[tile], a.st_seq);
                    uint32_t *dst = sb.b ? a.st_buf0 : a.st_buf1;
                    const uint64_t P = (uint64_t)a.nrows * a.w;
#pragma unroll
                    for (int i = 0; i < 5; ++i) dst[(uint64_t)i * P + lp] = rs[i];
                }
                // CUDAKernels.cu:414-415; the same quotients through the
                // image's reciprocals (bih_pixdiv.h) at the sizes its proof covers
                if (recip) {
                    uf = pixel_divide((float)x + ru, fw, yw);
                    vf = pixel_divide((float)y + rv, fh, yh);
                } else {
                    uf = ((float)x + ru) / fw;
                    vf = ((float)y + rv) / fh;
                }
                camera_dir(a, uf, vf, dx, dy, dz);
            }
            // Ray::Ray (Ray.cu:3-10) + scene-AABB slab test (CUDAKernels.cu:237-262)
            float ix, iy, iz, tMin, tMax;
            const bool in_box = valid && scene_slab(slab, dx, dy, dz, ix, iy, iz, tMin, tMax);
            const unsigned long long live = sc.U > 0 ? __ballot(in_box) : 0ull;
            unsigned long long hits = 0ull, undecided = 0ull;
            BIH_PH(2);
            if (live && sc.U > 1 && bins_ok && !(a.dbg & 8u)) {
                uint32_t cand = 0, cmeta = 0, cent = 0, fc_ent = 0, fc_mt = 0;
                // Hit cache (frames after an item's first): a lane first tests
                // the triangle it hit in the item's previous frame -- the exact
                // intersector on the new ray, then that candidate's verification
                // plan.  Any verified candidate proves the hit Color() needs
                // (a lane of the reference walk that reaches an accepting
                // triangle), whatever the order the candidates are tried in; a
                // lane it does not prove walks the list as before, and only a
                // full walk proves a miss.  The jitter moves a sample within its
                // pixel, so most lanes hit the same small triangle again.
                unsigned long long chit = 0ull;
                if (use_cache && !(a.dbg & 20u)) {
                    const uint32_t cti = s_hc[0][tid];
                    bool okc = false, needc = false;
                    if (in_box && cti != kNoCache) {
                        const float4 *rp = reinterpret_cast<const float4 *>(a.tri_prim) + 4ull * cti;
                        const float4 r0 = rp[0], r1 = rp[1], r2 = rp[2];
                        const float tn = reinterpret_cast<const float *>(rp)[12];
                        const bool hc = prim_hit_lane(r0, r1, r2, tn, dx, dy, dz);
                        needc = hc && !(s_hc[1][tid] >> 31) && (s_hc[2][tid] & 3u) == 3u;
                        okc = hc && plan_verify(a, s_hc[1][tid], s_hc[2][tid], cti, ix, iy, iz, tMin, tMax);
                    }
#if BIH_PHASES
                    path_site_count(a, 0u, __ballot(needc), lane);
#else
                    (void)needc;
#endif
                    chit = __ballot(okc);
                }
                const unsigned long long wlive = live & ~chit;
                const unsigned long long found = wlive ? bin_walk<LOG2SPP == 2, COST || BIH_BINS_TIMELINE>(
                    a, prims, bin, le0, le1, gstat, uf, vf, dx, dy, dz, wlive, lane, cand, cmeta, cent, fc_ent, fc_mt, lent,
                    &ltag) : 0ull;
                if (COST) work += fc_ent + 4u * fc_mt;
#if BIH_BINS_TIMELINE
                tl_ent += fc_ent;
                tl_mt += fc_mt;
                tl_pv += (uint32_t)__popcll(__ballot(((found >> lane) & 1ull) && !(cand >> 31) && (cmeta & 3u) == 3u));
                tl_pl += (uint32_t)__popcll(__ballot(((found >> lane) & 1ull) && !(cand >> 31) && (cmeta & 3u) != 3u));
#endif
                BIH_PH(3);
#if BIH_PHASES
                path_site_count(a, 1u, __ballot(((found >> lane) & 1ull) && !(a.dbg & 16u) && !(cand >> 31) &&
                                                (cmeta & 3u) == 3u), lane);
#endif
                const bool ok = ((found >> lane) & 1ull) &&
                                ((a.dbg & 16u) || plan_verify(a, cand, cmeta, cent, ix, iy, iz, tMin, tMax));
                hits = __ballot(ok) | chit;
                undecided = wlive & found & ~hits;
                // the next frame of the item tries this one first (also a hit
                // among the list's first entries: every lane the cache settles
                // leaves the walk, whose pixel masks then skip more entries --
                // caching only hits past the 4th / 12th entry was slower, r06l)
                if (use_cache && ok) {
                    s_hc[0][tid] = cent;
                    s_hc[1][tid] = cand;
                    s_hc[2][tid] = cmeta;
                }
                BIH_PH(4);
#if BIH_FAST_COUNTERS
                {   // bin counters (bih_sync prints them): candidates decided by a
                    // plan, and plans that disagree with the root-path check (0)
                    const bool fnd = ((found >> lane) & 1ull) != 0ull;
                    const bool planned = fnd && ((cand >> 31) || (cmeta & 3u) != 3u);
                    const bool pv = fnd && path_verify(a.bin_path, cand & 0x7fffffffu, ix, iy, iz, tMin, tMax);
                    const unsigned long long rb = __ballot(planned), bad = __ballot(planned && (pv != ok));
                    if (lane == 0) {
                        atomicAdd(a.work + 38, (uint32_t)__popcll(bad));
                        atomicAdd(a.work + 39, (uint32_t)__popcll(rb));
                        atomicAdd(a.work + 40, 1u);
                        atomicAdd(a.work + 41, (uint32_t)__popcll(live));
                        atomicAdd(a.work + 42, fc_ent);
                        atomicAdd(a.work + 43, fc_mt);
                        atomicAdd(a.work + 44, (uint32_t)__popcll(found));
                        atomicAdd(a.work + 45, (uint32_t)__popcll(hits));
                        atomicAdd(a.work + 46, (uint32_t)__popcll(undecided));
                        atomicAdd(a.work + 47, found != wlive ? 1u : 0u);
                        atomicAdd(a.work + 52, (uint32_t)__popcll(chit));
                    }
                }
#endif
                if (a.dbg & 4u) {              // tests: every live lane to the fallback
                    hits = 0ull;
                    undecided = live;
                }
            } else if (live) {
                undecided = live;              // one leaf (U == 1) or no lists: the exact walk decides
            }
            if (undecided) {
                uint32_t r = 0;
                if (lane == 0) r = atomicAdd(a.bin_heads + 8 * 32, 1u);
                r = __builtin_amdgcn_readfirstlane(r);
                if (lane < 6) {
                    const uint32_t v[6] = {tile, (uint32_t)undecided, (uint32_t)(undecided >> 32), (uint32_t)hits,
                                           (uint32_t)(hits >> 32), fj};
                    a.bin_fb[(uint64_t)r * kFbWords + lane] = v[lane];
                }
                continue;
            }
            if (valid && s == SPP - 1) {
                const unsigned long long m = (SPP == 64) ? ~0ull : ((1ull << SPP) - 1ull);
                fout[lp] = pixel_from_hits(__popcll((hits >> (pix * SPP)) & m), SPP);
            }
            if (MASK && lane == 0) a.hit_mask[tile] = hits;
            BIH_PH(5);
        }
        if (COST && lane == 0) a.bin_cost[bin] = (work << 8) / (nf - f0);
        if (use_cache && a.hcache) {   // for the tile's next item (a later launch)
            if (valid) a.hcache[(uint64_t)tile * 64 + lane] = s_hc[0][tid];
            if (lane == 0) a.hstamp[tile] = a.hseq;
        }
        if (STAMP && nf == a.nframes && lane == 0) {
            // (the item ending at the launch's last frame) the tile's new stamp
            const StampBase sb = stamp_base(a.stamps[tile], a.st_seq);
            a.stamps[tile] = stamp_pack(a.st_f0 + a.nframes, sb.b ^ 1u, sb, a.st_seq);
        }
#if BIH_BINS_TIMELINE
        tl_rec(lane, 0u, tl_t0, __builtin_amdgcn_s_memrealtime(),
               (le1 - le0) | ((nf - f0) << 24));
        tl_rec(lane, 4u, tl_ent, tl_ent + tl_mt, tl_pv | (tl_pl << 16));   // {ent, mt, pv | pl << 16}
#endif
    }
#if BIH_BINS_TIMELINE
    {
        const uint64_t t = __builtin_amdgcn_s_memrealtime();
        tl_rec(lane, 3u, t, t, 0u);
    }
#endif
#if BIH_PHASES
    if (lane == 0)
        for (int k = 0; k < 6; ++k)
            atomicAdd(reinterpret_cast<unsigned long long *>(a.work + 64) + k, ph[k]);
#endif
#undef BIH_PH
}

// The packets k_render_bins left undecided: the undecided lanes take the
// exact any-hit walk (Walker: TraverseTree as the reference runs it, per
// lane, LDS stack), then the tile's pixels are written.  Launched after every
// k_render_bins on the same stream; with no fallback record it only reads
// the count.
template <int LOG2SPP>
__global__ void __launch_bounds__(kThreads) k_render_fallback(const RenderArgs a) {
    constexpr uint32_t SPP = 1u << LOG2SPP;
    constexpr uint32_t TW = TileShape<LOG2SPP>::TW;
    __shared__ uint32_t s_node[kLdsStack * kThreads];
    __shared__ float s_min[kLdsStack * kThreads];
    __shared__ float s_max[kLdsStack * kThreads];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t n = *(volatile const uint32_t *)(a.bin_heads + 8 * 32);
    const uint64_t gwave = (uint64_t)blockIdx.x * (kThreads / 64) + (tid >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * (kThreads / 64);
    if (gwave >= n) return;
    const Stack st = {s_node, s_min, s_max, tid, a.spill, (uint64_t)gridDim.x * kThreads,
                      (uint64_t)blockIdx.x * kThreads + tid};
    const SceneU sc = load_scene(a);
    const uint32_t tiles_x = (a.w + TW - 1) / TW;
    const float fw = (float)a.w, fh = (float)a.h;
    const uint32_t pix = lane >> LOG2SPP;
    for (uint64_t r = gwave; r < n; r += nwaves) {
        const uint32_t *rec = a.bin_fb + r * kFbWords;
        const uint32_t tile = rec[0];
        const unsigned long long und = ((unsigned long long)rec[2] << 32) | rec[1];
        unsigned long long hits = ((unsigned long long)rec[4] << 32) | rec[3];
        const uint32_t fj = rec[5];                      // frame of a multi-frame launch
        uint32_t *const fout = a.out + (uint64_t)fj * a.out_stride;
        uint32_t x, lr, s;
        ray_coords<LOG2SPP>((uint64_t)tile * 64 + lane, tiles_x, x, lr, s);
        const bool valid = x < a.w && lr < a.nrows;
        const uint64_t lp = (uint64_t)lr * a.w + x;
        const bool mine = valid && ((und >> lane) & 1ull);
        float dx = 0.f, dy = 0.f, dz = 1.f;
        if (mine) {
            float ru = 0.f, rv = 0.f;
            ray_jitter<SPP>(a, lp, s, ru, rv, fj, tile);
            const uint32_t y = global_row(lr, a.row0, a.band_h, a.band_step);
            camera_dir(a, ((float)x + ru) / fw, ((float)y + rv) / fh, dx, dy, dz);
        }
        Walker<true, false> w;
        w.start(sc, mine, dx, dy, dz);
        while (w.alive) w.step(sc, st);
        hits |= __ballot(mine && w.hit);
        if (valid && s == SPP - 1) fout[lp] = pixel_of_mask<SPP>(hits, pix);
        if (a.hit_mask && lane == 0) a.hit_mask[tile] = hits;
    }
}

}  // namespace

bool render_uses_prim(uint32_t spp) {
    return spp <= 64 && (spp & (spp - 1)) == 0;
}

// Resident blocks of k_render_bins on `device` (its own occupancy: the list
// walk needs fewer registers than the BIH walks).  A launch of several
// frames takes fewer than the occupancy allows (kBinsMultiPerCU per CU): the
// calls in flight then overlap -- the next call's advance and first waves
// run in the free slots while this one drains (1080p headline, blocks per CU
// of 16-frame launches: 6 (all) 0.0420 ms per frame, 5 0.0419, 4 0.0399, 3
// 0.0397, 2 0.0400; r04zk/zl).  Only while another render is in flight
// (RenderArgs::shared_grid, from the other slots' events): a lone 16-frame
// launch is slower with fewer waves (4: 0.0494 ms per frame against 0.0454
// with all 6), so it takes every slot.  One-frame launches keep every slot
// (4 per CU: 0.087 -> 0.093 ms alone).
constexpr int kBinsMultiPerCU = 4;
uint32_t bins_grid_blocks(int device, uint32_t nframes, bool stamped) {
    static std::mutex mu;
    static uint32_t cache[64][2][2] = {{{0}}};
    std::lock_guard<std::mutex> lk(mu);
    if (device < 0 || device >= 64) return 0;
    if (!cache[device][stamped][0]) {
        int cus = 0, per = 0;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &per, stamped ? reinterpret_cast<const void *>(k_render_bins<2, kBinsStamped>)
                          : reinterpret_cast<const void *>(k_render_bins<2, 0>), kThreads, 0);
        if (cus <= 0) cus = 256;
        if (per <= 0) per = 1;
        int multi = kBinsMultiPerCU < per ? kBinsMultiPerCU : per;
        if (const char *e = getenv("BIH_BINS_BLOCKS_PER_CU")) {
            const int v = atoi(e);
            if (v > 0 && v <= 32) per = v;
        }
        if (const char *e = getenv("BIH_BINS_MULTI_PER_CU")) {
            const int v = atoi(e);
            if (v > 0 && v <= 32) multi = v;
        }
        cache[device][stamped][0] = (uint32_t)(cus * per);
        cache[device][stamped][1] = (uint32_t)(cus * multi);
    }
    return cache[device][stamped][nframes > 1 ? 1 : 0];
}

template <int L>
static hipError_t launch_bins(const RenderArgs &a, hipStream_t st, uint32_t blocks, uint32_t fb_blocks,
                              hipEvent_t k0, hipEvent_t k1) {
    hipError_t e = k0 ? hipEventRecord(k0, st) : hipSuccess;
    if (e != hipSuccess) return e;
    if (a.hit_mask)
        hipLaunchKernelGGL((k_render_bins<L, 1>), dim3(blocks), dim3(kThreads), 0, st, a);
    else if (a.bin_cost && a.stamps)
        hipLaunchKernelGGL((k_render_bins<L, 2 | kBinsStamped>), dim3(blocks), dim3(kThreads), 0, st, a);
    else if (a.bin_cost)
        hipLaunchKernelGGL((k_render_bins<L, 2>), dim3(blocks), dim3(kThreads), 0, st, a);
    else if (a.stamps)
        hipLaunchKernelGGL((k_render_bins<L, kBinsStamped>), dim3(blocks), dim3(kThreads), 0, st, a);
    else
        hipLaunchKernelGGL((k_render_bins<L, 0>), dim3(blocks), dim3(kThreads), 0, st, a);
    e = k1 ? hipEventRecord(k1, st) : hipSuccess;
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_render_fallback<L>, dim3(fb_blocks), dim3(kThreads), 0, st, a);
    return hipGetLastError();
}

// Diagnostic builds (BIH_BINS_TIMELINE): appends the per-item records of the
// k_render_bins launches since the last dump to `path` (raw uint4s) and
// resets the count.  Returns the number of records, or -1.
long bins_timeline_dump(const char *path) {
#if BIH_BINS_TIMELINE
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    std::vector<uint32_t> cnt(kTlWaves);
    std::vector<uint4> rec((size_t)kTlWaves * kTlPerWave);
    if (hipMemcpyFromSymbol(cnt.data(), HIP_SYMBOL(g_tl_n), kTlWaves * 4) != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(rec.data(), HIP_SYMBOL(g_tl_rec), rec.size() * sizeof(uint4)) != hipSuccess) return -1;
    std::vector<uint32_t> zero(kTlWaves, 0u);
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_tl_n), zero.data(), kTlWaves * 4) != hipSuccess) return -1;
    std::vector<uint4> out;
    uint32_t lost = 0;
    for (uint32_t w = 0; w < kTlWaves; ++w) {
        const uint32_t n = cnt[w] < kTlPerWave ? cnt[w] : kTlPerWave;
        lost += cnt[w] - n;
        for (uint32_t k = 0; k < n; ++k) out.push_back(rec[(size_t)w * kTlPerWave + k]);
    }
    if (FILE *f = fopen(path, "ab")) {
        const uint32_t hdr[4] = {0x544C4942u, (uint32_t)out.size(), lost, 0u};   // "BILT", count, dropped
        fwrite(hdr, sizeof hdr, 1, f);
        if (!out.empty()) fwrite(out.data(), sizeof(uint4), out.size(), f);
        fclose(f);
    }
    return (long)out.size();
#else
    (void)path;
    return -1;
#endif
}

int launch_render(const RenderArgs &a, uint32_t traverse, void *stream, void *ev_k0, void *ev_k1) {
    const uint32_t spp = a.spp;
    if (!(a.bin_queue && spp <= 64 && (spp & (spp - 1)) == 0)) return launch_walk(a, traverse, stream, ev_k0, ev_k1);
    hipStream_t st = (hipStream_t)stream;
    const hipEvent_t k0 = (hipEvent_t)ev_k0, k1 = (hipEvent_t)ev_k1;
    int dev = 0;
    (void)hipGetDevice(&dev);
    // frustum bins: the list-walk kernel, then the exact walk for what it
    // left undecided (the fallback grid stays within the spill area)
    const uint32_t grid = wave_grid_blocks(dev);
    const uint32_t fb = grid < 64u ? grid : 64u;
    const uint32_t gb = bins_grid_blocks(dev, a.shared_grid ? 2u : 1u, a.stamps != nullptr);
    if (BIH_FAST_COUNTERS || BIH_PHASES) {
        const hipError_t e = hipMemsetAsync(a.work, 0, kWorkWords * sizeof(uint32_t), st);
        if (e != hipSuccess) return (int)e;
    }
    return (int)with_log2spp(spp, [&](auto l) { return launch_bins<decltype(l)::value>(a, st, gb, fb, k0, k1); });
}

}  // namespace bih
