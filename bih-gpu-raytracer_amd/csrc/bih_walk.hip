// bih_walk.hip -- the BIH walk kernels of the primary-ray render for gfx950.
//
// Replaces cudaRender (reference src/CUDAKernels.cu:391-423) and its callees
// Camera::GetRay (Camera.cu:18-20), Ray::Ray (Ray.cu:3-10), Color (:370-389),
// TraverseTree (:227-368), FindNearestTriangle (:206-224) and
// RayTriangleIntersection (:17-50).  Numerics: bih_ray.h.
//
// Kernels
//   k_render_packet_asm  the exact packet walk (TRAVERSE_REFERENCE, counters,
//                        renders without bins), hand-scheduled gfx950 asm.
//   k_render_packet2     the same packet walk in HIP: the asm walk's cross-check
//                        (BIH_RENDER_KERNEL=packet2, test_kernel_variants_agree).
//   k_render_packet      the packet walk over the canonical packed nodes: scenes
//                        past the camera-relative records' 2^26 triangles.
//   k_render_pixel       spp not a power of two: one lane per pixel, samples in
//                        sequence (cudaRender's own loop order), on Walker.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>

#include "bih_packet_asm.h"
#include "bih_ray.h"

namespace bih {
namespace {

// ---------------------------------------------------------------------------
// k_render_pixel: any spp; one lane per pixel, spp samples in sequence
// (cudaRender's own loop order).  One wave = one 8x8 pixel tile.
// ---------------------------------------------------------------------------
template <bool ANYHIT, bool STATS>
__global__ void __launch_bounds__(kThreads) k_render_pixel(const RenderArgs a) {
    __shared__ uint32_t s_node[kLdsStack * kThreads];
    __shared__ float s_min[kLdsStack * kThreads];
    __shared__ float s_max[kLdsStack * kThreads];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t tiles_x = (a.w + 7) >> 3;
    const uint32_t ntiles = tiles_x * ((a.nrows + 7) >> 3);
    const Stack st = {s_node, s_min, s_max, tid, a.spill, (uint64_t)gridDim.x * kThreads,
                      (uint64_t)blockIdx.x * kThreads + tid};
    const SceneU sc = load_scene(a);
    const uint64_t P = (uint64_t)a.nrows * a.w;
    // grid-stride over 8x8 tiles (the grid is capped at the spill area's size)
    for (uint32_t wv = blockIdx.x * (kThreads / 64) + (tid >> 6); wv < ntiles;
         wv += gridDim.x * (kThreads / 64)) {
        const uint32_t x = (wv % tiles_x) * 8 + (lane & 7);
        const uint32_t lr = (wv / tiles_x) * 8 + (lane >> 3);
        if (x >= a.w || lr >= a.nrows) continue;
        const uint32_t y = global_row(lr, a.row0, a.band_h, a.band_step);
        const uint64_t lp = (uint64_t)lr * a.w + x;
        uint32_t v[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) v[i] = a.rng_in[(uint64_t)i * P + lp];
        uint32_t d = a.d_base;
        uint32_t k = 0;
        for (uint32_t s = 0; s < a.spp; ++s) {
            const float ru = xorwow_uniform(v, d);
            const float rv = xorwow_uniform(v, d);
            float dx, dy, dz;
            camera_dir(a, ((float)x + ru) / (float)a.w, ((float)y + rv) / (float)a.h, dx, dy, dz);
            Walker<ANYHIT, STATS> w;
            w.start(sc, true, dx, dy, dz);
            while (w.alive) w.step(sc, st);
            if (STATS) write_ray_stats(a, lp * a.spp + s, w.cnt.nodes, w.cnt.leaves, w.cnt.tris);
            k += w.hit ? 1u : 0u;
        }
        a.out[lp] = pixel_from_hits(k, a.spp);
    }
}

// ---------------------------------------------------------------------------
// k_render_packet: the wave walks the BIH as one packet of 64 rays.
//
// Every lane keeps its own interval [tMin, tMax] and makes the reference's
// own decision at each node: it visits the near child iff tMin < t[near]
// (interval [tMin, t[near]]) and the far child iff !(tMax < t[far])
// (interval [t[far], tMax]) -- the four cases of TraverseTree
// (CUDAKernels.cu:295-365) reduce to exactly that.  A lane's visited set and
// its intervals depend only on the path from the root, not on the order in
// which subtrees are walked, so the wave may walk the UNION of its lanes'
// sets in one order, with a 64-bit mask of the lanes that visit each node:
// every lane still tests exactly the leaves TraverseTree tests (reference
// walk), or a prefix of them in another order (any-hit walk, whose RGBA only
// needs "some tested triangle hit").
// Node index, masks and the triangle records are wave-uniform (scalar loads
// through the scalar cache); the per-lane intervals of the stack live in
// VGPRs indexed by the uniform stack pointer (s_set_gpr_idx), entries past
// kPacketRegs in a per-wave HBM area.
// ---------------------------------------------------------------------------
template <bool ANYHIT, bool STATS, int LOG2SPP>
__global__ void __launch_bounds__(kThreads) k_render_packet(const RenderArgs a) {
    constexpr uint32_t SPP = 1u << LOG2SPP;
    constexpr uint32_t TW = TileShape<LOG2SPP>::TW, TH = TileShape<LOG2SPP>::TH;
    constexpr int D = kPacketRegs;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned long long me = lane_bit(lane);
    const uint64_t gwave = (uint64_t)blockIdx.x * (kThreads / 64) + wv;
    uint32_t *wspill = a.spill + gwave * (uint64_t)(kStackDepth - D) * 3 * 64;
    const SceneU sc = load_scene(a);
    const cnode_t *nodes = (const cnode_t *)(const void *)a.nodes;
    const cprim_t *prims = (const cprim_t *)(const void *)a.tri_prim;
    const cu32_t *dupc = (const cu32_t *)(const void *)a.dup_cnt;
    const uint32_t tiles_x = (a.w + TW - 1) / TW;
    const uint32_t ntiles = tiles_x * ((a.nrows + TH - 1) / TH);
    const uint32_t pix = lane >> LOG2SPP;

    for (;;) {
        uint32_t tile = 0;
        if (lane == 0) tile = atomicAdd(a.work, 1u);
        tile = __builtin_amdgcn_readfirstlane(tile);
        if (tile >= ntiles) break;
        const PacketRay r = packet_ray<LOG2SPP>(a, sc, tile, lane, tiles_x);
        const bool valid = r.valid, in_box = r.in_box;
        const uint32_t s = r.s, sg = r.sg;
        const uint64_t lp = r.lp;
        const float dx = r.dx, dy = r.dy, dz = r.dz, ix = r.ix, iy = r.iy, iz = r.iz;
        float tMin = r.tMin, tMax = r.tMax;
        bool hit = false;
        uint32_t c_nodes = 0, c_leaves = 0, c_tris = 0;
        // lanes whose ray is still searching
        unsigned long long live = sc.U > 0 ? __ballot(in_box) : 0ull;

        // test the triangles [b, b+n) for the lanes in m (every lane computes,
        // only the lanes of m record: no per-lane branch)
        auto test_leaf = [&](uint32_t b, uint32_t n, unsigned long long m) {
            if (STATS && (m & me)) ++c_leaves;
            for (uint32_t i = 0; i < n; ++i) {
                if (ANYHIT) {
                    m &= live;
                    if (!m) break;
                }
                const sf32x16 rec = prims[b + i];
                const bool in = (m & me) != 0ull;
                if (STATS) c_tris += in ? 1u : 0u;
                hit |= in && prim_hit(rec, dx, dy, dz);
                if (ANYHIT) live &= ~__ballot(hit);
            }
        };

        if (live && sc.U == 1) {                          // single leaf (reference: UB)
            test_leaf(0, sc.N, live);
        } else if (live) {
            float st[3 * D];   // per-lane entries {lo, hi, word} indexed by the uniform sp
            uint32_t cur = 0, sp = 0;
            unsigned long long act = live;
            for (;;) {
                if (STATS && (act & me)) ++c_nodes;
                const su32x4 nd = nodes[cur];
                const uint32_t ax = (nd.z >> 27) & 3u;
                const float org = ax == 0 ? sc.ox : (ax == 1 ? sc.oy : sc.oz);   // uniform
                const float inv = sel3(ax, ix, iy, iz);
                const bool nr = (sg >> ax) & 1u;
                const float t0 = (__uint_as_float(nd.x) - org) * inv;
                const float t1 = (__uint_as_float(nd.y) - org) * inv;
                const float tn = nr ? t1 : t0, tf = nr ? t0 : t1;
                const bool A = tMin < tn;                 // near child visited
                const bool nB = !(tMax < tf);             // far child visited
                // child intervals: near [tMin, tn], far [tf, tMax]
                const float lo_L = nr ? tf : tMin, hi_L = nr ? tMax : tn;
                const float lo_R = nr ? tMin : tf, hi_R = nr ? tn : tMax;
                const unsigned long long mN = __ballot(A) & act, mF = __ballot(nB) & act;
                const unsigned long long mnr = __ballot(nr);
                unsigned long long mL = (mN & ~mnr) | (mF & mnr);
                unsigned long long mR = (mN & mnr) | (mF & ~mnr);
                const uint32_t split = nd.z & kIdxMask, mid = nd.w & kIdxMask;
                const bool leafL = (nd.z >> 29) & 1u, leafR = (nd.z >> 30) & 1u;
                // near first for the majority of the packet
                const bool nearL = __popcll(act & mnr) * 2 <= (uint32_t)__popcll(act);
                if ((leafL && mL) || (leafR && mR)) {
                    uint32_t cL = (nd.w >> 27) & 3u, cR = (nd.w >> 29) & 3u;
                    if (leafL && cL == 0) cL = dupc[split];
                    if (leafR && cR == 0) cR = dupc[split + 1];
                    if (nearL) {
                        if (leafL && mL) test_leaf(mid - cL, cL, mL);
                        if (leafR && mR) test_leaf(mid, cR, mR);
                    } else {
                        if (leafR && mR) test_leaf(mid, cR, mR);
                        if (leafL && mL) test_leaf(mid - cL, cL, mL);
                    }
                }
                if (ANYHIT) {
                    mL &= live;
                    mR &= live;
                }
                const unsigned long long gL = leafL ? 0ull : mL, gR = leafR ? 0ull : mR;
                if (gL && gR) {
                    // descend near, stack far (node, mask, per-lane interval)
                    const uint32_t fnode = nearL ? split + 1 : split;
                    const unsigned long long fmask = nearL ? gR : gL;
                    const float flo = nearL ? lo_R : lo_L, fhi = nearL ? hi_R : hi_L;
                    // entry word: node index | this lane's mask bit << 31
                    const uint32_t word = fnode | (((fmask & me) != 0ull) ? 0x80000000u : 0u);
                    if (sp < (uint32_t)D) {
                        st[3 * sp] = flo;
                        st[3 * sp + 1] = fhi;
                        st[3 * sp + 2] = __uint_as_float(word);
                    } else {
                        uint32_t *q = wspill + ((sp - D) * 3) * 64 + lane;
                        q[0] = __float_as_uint(flo);
                        q[64] = __float_as_uint(fhi);
                        q[128] = word;
                    }
                    sp = __builtin_amdgcn_readfirstlane(sp + 1);
                    cur = nearL ? split : split + 1;
                    act = nearL ? gL : gR;
                    tMin = nearL ? lo_L : lo_R;
                    tMax = nearL ? hi_L : hi_R;
                } else if (gL) {
                    cur = split; act = gL; tMin = lo_L; tMax = hi_L;
                } else if (gR) {
                    cur = split + 1; act = gR; tMin = lo_R; tMax = hi_R;
                } else {
                    // pop until an entry still has a live lane
                    bool found = false;
                    while (sp > 0) {
                        sp = __builtin_amdgcn_readfirstlane(sp - 1);
                        uint32_t word;
                        float lo, hi;
                        if (sp < (uint32_t)D) {
                            lo = st[3 * sp];
                            hi = st[3 * sp + 1];
                            word = __float_as_uint(st[3 * sp + 2]);
                        } else {
                            const uint32_t *q = wspill + ((sp - D) * 3) * 64 + lane;
                            lo = __uint_as_float(q[0]);
                            hi = __uint_as_float(q[64]);
                            word = q[128];
                        }
                        unsigned long long m = __ballot(word >> 31);
                        if (ANYHIT) m &= live;
                        if (!m) continue;
                        cur = __builtin_amdgcn_readfirstlane(word & 0x7fffffffu);
                        act = m;
                        tMin = lo;
                        tMax = hi;
                        found = true;
                        break;
                    }
                    if (!found) break;
                }
            }
        }

        if (STATS && valid) write_ray_stats(a, lp * SPP + s, c_nodes, c_leaves, c_tris);
        const unsigned long long hb = __ballot(hit);
        if (valid && s == SPP - 1) a.out[lp] = pixel_of_mask<SPP>(hb, pix);
    }
}

// ---------------------------------------------------------------------------
// k_render_packet2: the packet walk of k_render_packet, restructured so that
// the per-node work is mostly VALU and the wave-uniform control stays short:
//   * node records relative to the camera origin (k_node_prim): t = d * inv
//     with d = clip - O[axis] computed once per origin (same f32 subtraction
//     as the reference's (clip - origin[axis]), CUDAKernels.cu:300-301);
//   * no near/far swap: with s = sign of this lane's direction on the axis,
//       left  visited iff (t0 > (s ? tMax : tMin)) xor s,
//       right visited iff (t1 > (s ? tMin : tMax)) xnor s,
//     which is exactly tMin < t[near] (near) and !(tMax < t[far]) (far),
//     NaNs included (a NaN compare is false on both sides);
//   * hits kept as one wave-uniform mask; triangle early-outs on the lanes
//     that actually test the leaf;
//   * child order chosen once per packet and axis (majority direction).
// ---------------------------------------------------------------------------
// The descend decision of one packet node step, wave-uniform: pickL = take
// the left child (nearL ? gL != 0 : gR == 0); the taken child gets mask gT,
// node cT and its lanes' intervals, the other (gO, cO, olo/ohi) is stacked
// when gO != 0.  Written as one SALU/VALU sequence (hipcc's own lowering of
// the same selects spends about twice the scalar instructions).
__device__ __forceinline__ void descend_pick(unsigned long long gL, unsigned long long gR,
                                             uint32_t nearL, uint32_t split, float loL, float hiL,
                                             float loR, float hiR, unsigned long long &gT,
                                             unsigned long long &gO, uint32_t &cT, uint32_t &cO,
                                             float &tlo, float &thi, float &olo, float &ohi) {
    uint32_t p, q;
    unsigned long long mk;
    asm volatile(
        "s_cmp_lg_u64 %[gL], 0\n\t"
        "s_cselect_b32 %[p], 1, 0\n\t"
        "s_cmp_eq_u64 %[gR], 0\n\t"
        "s_cselect_b32 %[q], 1, 0\n\t"
        "s_cmp_lg_u32 %[nearL], 0\n\t"
        "s_cselect_b32 %[p], %[p], %[q]\n\t"
        "s_cmp_lg_u32 %[p], 0\n\t"
        "s_cselect_b64 %[gT], %[gL], %[gR]\n\t"
        "s_cselect_b64 %[gO], %[gR], %[gL]\n\t"
        "s_cselect_b64 %[mk], -1, 0\n\t"
        "s_add_u32 %[cO], %[split], %[p]\n\t"
        "s_xor_b32 %[q], %[p], 1\n\t"
        "s_add_u32 %[cT], %[split], %[q]\n\t"
        "v_cndmask_b32_e64 %[tlo], %[loR], %[loL], %[mk]\n\t"
        "v_cndmask_b32_e64 %[thi], %[hiR], %[hiL], %[mk]\n\t"
        "v_cndmask_b32_e64 %[olo], %[loL], %[loR], %[mk]\n\t"
        "v_cndmask_b32_e64 %[ohi], %[hiL], %[hiR], %[mk]"
        : [p] "=&s"(p), [q] "=&s"(q), [mk] "=&s"(mk), [gT] "=&s"(gT), [gO] "=&s"(gO),
          [cT] "=&s"(cT), [cO] "=&s"(cO), [tlo] "=&v"(tlo), [thi] "=&v"(thi), [olo] "=&v"(olo),
          [ohi] "=&v"(ohi)
        : [gL] "s"(gL), [gR] "s"(gR), [nearL] "s"(nearL), [split] "s"(split), [loL] "v"(loL),
          [hiL] "v"(hiL), [loR] "v"(loR), [hiR] "v"(hiR)
        : "scc");
}

template <bool ANYHIT, bool STATS, int LOG2SPP>
__global__ void __launch_bounds__(kThreads) k_render_packet2(const RenderArgs a) {
    constexpr uint32_t SPP = 1u << LOG2SPP;
    constexpr uint32_t TW = TileShape<LOG2SPP>::TW, TH = TileShape<LOG2SPP>::TH;
    constexpr int D = kPacketRegs;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned long long me = lane_bit(lane);
    const uint64_t gwave = (uint64_t)blockIdx.x * (kThreads / 64) + wv;
    uint32_t *wspill = a.spill + gwave * (uint64_t)(kStackDepth - D) * 3 * 64;
    const SceneU sc = load_scene(a);
    const cnode_t *nodes = (const cnode_t *)(const void *)(STATS ? a.node_prim : a.node_cull);
    const cprim_t *prims = (const cprim_t *)(const void *)a.tri_prim;
    const cu32_t *dupc = (const cu32_t *)(const void *)a.dup_cnt;
    const uint32_t tiles_x = (a.w + TW - 1) / TW;
    const uint32_t ntiles = tiles_x * ((a.nrows + TH - 1) / TH);
    const uint32_t pix = lane >> LOG2SPP;

    for (;;) {
        uint32_t tile = 0;
        if (lane == 0) tile = atomicAdd(a.work, 1u);
        tile = __builtin_amdgcn_readfirstlane(tile);
        if (tile >= ntiles) break;
        const PacketRay r = packet_ray<LOG2SPP>(a, sc, tile, lane, tiles_x);
        const bool valid = r.valid, in_box = r.in_box;
        const uint32_t s = r.s, sg = r.sg;
        const uint64_t lp = r.lp;
        const float dx = r.dx, dy = r.dy, dz = r.dz, ix = r.ix, iy = r.iy, iz = r.iz;
        float tMin = r.tMin, tMax = r.tMax;
        uint32_t c_nodes = 0, c_leaves = 0, c_tris = 0;
#if BIH_PACKET_COUNTERS
        uint32_t pk[8] = {1, 0, 0, 0, 0, 0, 0, 0};   // packet-level walk counters (debug builds)
#endif
        const unsigned long long live = sc.U > 0 ? __ballot(in_box) : 0ull;
        unsigned long long hits = 0ull;   // lanes whose ray hit some tested triangle
        // left child first on an axis when most of the packet runs +axis there
        uint32_t nearbits = 0;
#pragma unroll
        for (uint32_t k = 0; k < 3; ++k) {
            const unsigned long long neg = __ballot((sg >> k) & 1u) & live;
            if (__popcll(neg) * 2 <= __popcll(live)) nearbits |= 1u << k;
        }

        // test triangles [b, b+n) for the lanes of m
        auto test_leaf = [&](uint32_t b, uint32_t n, unsigned long long m) {
            if (STATS && (m & me)) ++c_leaves;
#if BIH_PACKET_COUNTERS
            ++pk[2];
#endif
            for (const uint32_t e = b + n; b < e; ++b) {
                if (ANYHIT) {
                    m &= ~hits;
                    if (!m) break;
                }
#if BIH_PACKET_COUNTERS
                ++pk[3];
                if (lane == 0) atomicAdd(a.work + kHistWord + 8 + (31 - __builtin_clz(__popcll(m))), 1u);
#endif
                if (STATS && (m & me)) ++c_tris;
#if BIH_PACKET_COUNTERS
                hits |= prim_hits(prims[b], dx, dy, dz, m, a.work + 56);
#else
                hits |= prim_hits(prims[b], dx, dy, dz, m);
#endif
            }
        };

        if (live && sc.U == 1) {                          // single leaf (reference: UB)
            test_leaf(0, sc.N, live);
        } else if (live) {
            // per-lane entries {lo, hi, node | this lane's mask bit << 31}, one
            // interleaved array (private memory: one dwordx3 access per push/pop)
            float st[3 * D];
            uint32_t cur = 0, sp = 0;
            unsigned long long act = live;
            for (;;) {
                if (STATS && (act & me)) ++c_nodes;
#if BIH_PACKET_COUNTERS
                ++pk[1];
                if (lane == 0) atomicAdd(a.work + kHistWord + (31 - __builtin_clz(__popcll(act))), 1u);
#endif
                const su32x4 nd = nodes[cur];
                const uint32_t ax = nd.z & 3u;          // prim record layout (k_node_prim)
                const float inv = ax == 2u ? iz : (ax == 1u ? iy : ix);
                const bool neg = (sg >> ax) & 1u;
                const float t0 = __uint_as_float(nd.x) * inv;
                const float t1 = __uint_as_float(nd.y) * inv;
                const unsigned long long mneg = __ballot(neg);
                unsigned long long gL = (__ballot(t0 > (neg ? tMax : tMin)) ^ mneg) & act;
                unsigned long long gR = ~(__ballot(t1 > (neg ? tMin : tMax)) ^ mneg) & act;
                const float lo_L = neg ? t0 : tMin, hi_L = neg ? tMax : t0;
                const float lo_R = neg ? tMin : t1, hi_R = neg ? t1 : tMax;
                const uint32_t split = nd.z >> 8, mid = nd.w & 0x3ffffffu;
                // bit 0: left is a leaf, bit 1: right (w' bits 26, 31)
                const uint32_t leaf = ((nd.w >> 26) & 1u) | ((nd.w >> 30) & 2u);
                const uint32_t nearL = (nearbits >> ax) & 1u;
                if (leaf) {
                    const unsigned long long tL = (leaf & 1u) ? gL : 0ull;
                    const unsigned long long tR = (leaf & 2u) ? gR : 0ull;
                    if (tL | tR) {
                        uint32_t cL = (nd.w >> 27) & 3u, cR = (nd.w >> 29) & 3u;
                        if (tL && cL == 0) cL = dupc[split];
                        if (tR && cR == 0) cR = dupc[split + 1];
                        if (nearL) {
                            if (tL) test_leaf(mid - cL, cL, tL);
                            if (tR) test_leaf(mid, cR, tR);
                        } else {
                            if (tR) test_leaf(mid, cR, tR);
                            if (tL) test_leaf(mid - cL, cL, tL);
                        }
                    }
                    if (leaf & 1u) gL = 0ull;
                    if (leaf & 2u) gR = 0ull;
                    if (ANYHIT) {
                        gL &= ~hits;
                        gR &= ~hits;
                    }
                }
                if (gL | gR) {
                    // take the near child (majority order) when both are
                    // visited, else the only one; stack the other if visited
                    unsigned long long gT, gO;
                    uint32_t cT, cO;
                    float tlo, thi, olo, ohi;
                    descend_pick(gL, gR, nearL, split, lo_L, hi_L, lo_R, hi_R, gT, gO, cT, cO, tlo,
                                 thi, olo, ohi);
                    if (gO) {
                        const uint32_t word = cO | ((uint32_t)((gO >> lane) & 1ull) << 31);
                        if (__builtin_expect(sp < (uint32_t)D, 1)) {
                            st[3 * sp] = olo;
                            st[3 * sp + 1] = ohi;
                            st[3 * sp + 2] = __uint_as_float(word);
                        } else {
                            uint32_t *q = wspill + ((sp - D) * 3) * 64 + lane;
                            q[0] = __float_as_uint(olo);
                            q[64] = __float_as_uint(ohi);
                            q[128] = word;
                        }
#if BIH_PACKET_COUNTERS
                        ++pk[4];
                        if (lane == 0) atomicAdd(a.work + 24 + (sp < 32 ? sp : 31), 1u);
                        pk[6] = sp + 1 > pk[6] ? sp + 1 : pk[6];
#endif
                        ++sp;
                    }
                    cur = cT;
                    act = gT;
                    tMin = tlo;
                    tMax = thi;
                    continue;
                }
                // pop until an entry still has a searching lane
                bool found = false;
                while (sp > 0) {
                    --sp;
#if BIH_PACKET_COUNTERS
                    ++pk[5];
#endif
                    uint32_t word;
                    float lo, hi;
                    if (sp < (uint32_t)D) {
                        lo = st[3 * sp];
                        hi = st[3 * sp + 1];
                        word = __float_as_uint(st[3 * sp + 2]);
                    } else {
                        const uint32_t *q = wspill + ((sp - D) * 3) * 64 + lane;
                        lo = __uint_as_float(q[0]);
                        hi = __uint_as_float(q[64]);
                        word = q[128];
                    }
                    unsigned long long m = __ballot(word >> 31);
                    if (ANYHIT) m &= ~hits;
                    if (!m) continue;
                    cur = __builtin_amdgcn_readfirstlane(word & 0x7fffffffu);
                    act = m;
                    tMin = lo;
                    tMax = hi;
                    found = true;
                    break;
                }
                if (!found) break;
            }
        }

#if BIH_PACKET_COUNTERS
        if (lane == 0) {
            for (int k = 0; k < 6; ++k) atomicAdd(a.work + 16 + k, pk[k]);
            atomicMax(a.work + 22, pk[6]);
            // packets by log2(node steps): count, node steps, triangle tests
            const uint32_t bin = pk[1] ? 31 - __builtin_clz(pk[1]) : 0;
            atomicAdd(a.work + kHistWord + 16 + bin, 1u);
            atomicAdd(a.work + kHistWord + 32 + bin, pk[1]);
            atomicAdd(a.work + kHistWord + 48 + bin, pk[3]);
        }
#endif
        if (STATS && valid) write_ray_stats(a, lp * SPP + s, c_nodes, c_leaves, c_tris);
        if (valid && s == SPP - 1) a.out[lp] = pixel_of_mask<SPP>(hits, pix);
    }
}

// Tile scheduling of the persistent packet kernel, two levels:
//  * the image is cut into chunks of kChunkW x kChunkH tiles (a compact
//    block of pixels) and the chunks into kRegions bands of chunk rows, one
//    per XCD: an XCD drains its own band first (its L2 keeps that part of
//    the tree), then helps the others;
//  * all waves on one CU share one current chunk (per-CU slot, keyed by the
//    hardware CU id), so the ~28 packets in flight on a CU trace neighbouring
//    pixels and share the scalar cache's node and triangle lines.
// A slot is one 64-bit word {chunk + 1, next position}: a wave claims
// position p of the slot's chunk with one atomicAdd; the wave that draws
// p == chunk size (or the first one on an empty slot) refills it from the
// band counters; waves that overdraw wait (s_sleep) for the refill.
// 8 x 4 tiles (32 x 16 pixels).  With the any-hit shortcut (short packets):
// 8x4 0.632, 16x2 0.632, 8x2 0.649, 8x8 0.662, 4x4 0.668, 16x4 0.678, 4x2
// 0.86 ms per frame (3 in flight); with the exact walk 4x4 and 8x4 tied.
// Chunks of fewer tiles than half a CU's waves refill too often.
constexpr uint32_t kChunkW = 8, kChunkH = 4, kChunk = kChunkW * kChunkH;
constexpr uint32_t kSlotWord = 64;                     // work[64..): CU slots, kSlotStrideWords apart

struct TileQueue {
    uint32_t *work;
    unsigned long long *slot;
    const uint32_t *order;             // chunk permutation (k_chunk_order) or null
    uint32_t tiles_x, tiles_y, chunks_x, nchunks;
    uint32_t band, left;
    uint32_t chunk;                    // chunk of the tile next() returned

    __device__ uint32_t band_begin(uint32_t b) const {
        const uint32_t rows = (nchunks / chunks_x);
        return (uint32_t)(((uint64_t)rows * b) / kRegions) * chunks_x;
    }

    // Next tile (global tile index t = ty * tiles_x + tx) for this wave.
    __device__ bool next(uint32_t lane, uint32_t &tile) {
        for (;;) {
            unsigned long long v = 0;
            if (lane == 0) v = atomicAdd(slot, 1ull);
            const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
            const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
            if (hi == 0xFFFFFFFFu) return false;
            if (hi != 0 && lo < kChunk) {
                const uint32_t g = hi - 1;
                const uint32_t tx = (g % chunks_x) * kChunkW + lo % kChunkW;
                const uint32_t ty = (g / chunks_x) * kChunkH + lo / kChunkW;
                if (tx < tiles_x && ty < tiles_y) {
                    tile = ty * tiles_x + tx;
                    chunk = g;
                    return true;
                }
                continue;                                // edge chunk: position off the image
            }
            if ((hi == 0 && lo == 0) || (hi != 0 && lo == kChunk)) {
                // this wave refills the slot with the next chunk of its band
                while (left) {
                    uint32_t c = 0;
                    if (lane == 0) c = atomicAdd(work + band, 1u);
                    c = __builtin_amdgcn_readfirstlane(c);
                    const uint32_t b0 = band_begin(band), b1 = band_begin(band + 1);
                    if (c < b1 - b0) {
                        const uint32_t g = order ? order[b0 + c] : b0 + c;
                        if (lane == 0) atomicExch(slot, ((unsigned long long)(g + 1) << 32) | 1ull);
                        tile = (g / chunks_x) * kChunkH * tiles_x + (g % chunks_x) * kChunkW;
                        chunk = g;
                        return true;                     // position 0: always on the image
                    }
                    band = (band + 1) & (kRegions - 1);
                    --left;
                }
                if (lane == 0) atomicExch(slot, kSlotDone);
                return false;
            }
            __builtin_amdgcn_s_sleep(4);                 // another wave is refilling
        }
    }
};

__device__ __forceinline__ TileQueue make_queue(const RenderArgs &a, uint32_t tiles_x,
                                                uint32_t tiles_y) {
    TileQueue q;
    q.work = a.work;
    q.slot = reinterpret_cast<unsigned long long *>(a.work + kSlotWord + kSlotStrideWords * cu_key());
    q.tiles_x = tiles_x;
    q.tiles_y = tiles_y;
    q.chunks_x = (tiles_x + kChunkW - 1) / kChunkW;
    q.nchunks = q.chunks_x * ((tiles_y + kChunkH - 1) / kChunkH);
    q.order = a.chunk_order;
    q.band = xcc_id();
    q.left = kRegions;
    q.chunk = 0;
    return q;
}

// ---------------------------------------------------------------------------
// Any-hit shortcut walk over one shortcut box set (k_fast_fit): the packet
// walks the boxes near-first and tests leaves with the exact intersector
// (prim_hits).  A lane stops at its first hit and keeps that leaf in `cand`.
// Returns the lanes with a candidate.  Nothing is decided here: a candidate
// stands only if fast_verify passes.
//   pass 1 (tight boxes, cons = false): finds the hits of most lanes fast;
//   pass 2 (miss-proof boxes, miss_box; cons = true): the whole line is
//     tested against every box, so a lane of `live` that ends with no
//     candidate has no triangle the exact intersector accepts: a reference
//     miss.  (The walk drops nothing: its stack cannot overflow, below.)
// Entry/exit parameters of the line O + t D against a camera-relative box,
// entry clamped below at cl.  Plain v_min/v_max (no NaN canonicalisation):
// no operand is NaN -- boxes are finite or +-inf, |1/D| >= 1/|D|max > 0 --
// and pass 2 only runs lanes with finite 1/D.
__device__ __forceinline__ void slab_t(float lx, float ly, float lz, float hx, float hy, float hz,
                                       float ix, float iy, float iz, float cl, float &tn,
                                       float &tf) {
    const float a0 = lx * ix, a1 = hx * ix, b0 = ly * iy, b1 = hy * iy;
    const float c0 = lz * iz, c1 = hz * iz;
    float n0, n1, n2, f0, f1, f2;
    asm("v_min_f32 %[n0], %[a0], %[a1]\n\t"
        "v_max_f32 %[f0], %[a0], %[a1]\n\t"
        "v_min_f32 %[n1], %[b0], %[b1]\n\t"
        "v_max_f32 %[f1], %[b0], %[b1]\n\t"
        "v_min_f32 %[n2], %[c0], %[c1]\n\t"
        "v_max_f32 %[f2], %[c0], %[c1]\n\t"
        "v_max3_f32 %[n0], %[n0], %[n1], %[n2]\n\t"
        "v_min3_f32 %[f0], %[f0], %[f1], %[f2]\n\t"
        "v_max_f32 %[n0], %[cl], %[n0]"
        : [n0] "=&v"(n0), [n1] "=&v"(n1), [n2] "=&v"(n2), [f0] "=&v"(f0), [f1] "=&v"(f1),
          [f2] "=&v"(f2)
        : [a0] "v"(a0), [a1] "v"(a1), [b0] "v"(b0), [b1] "v"(b1), [c0] "v"(c0), [c1] "v"(c1),
          [cl] "s"(cl));
    tn = n0;
    tf = f0;
}
__device__ __forceinline__ sf32x16 fast_rec(const float *boxes, uint32_t node) {
    // one s_load with a 32-bit byte offset (no 64-bit address arithmetic);
    // loaded and waited for inside the statement
    sf32x16 r;
    asm volatile("s_load_dwordx16 %0, %1, %2\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=s"(r)
                 : "s"(boxes), "s"(node << 6)
                 : "memory");
    return r;
}
// BIH_FAST_COUNTERS builds: per-frame work of the shortcut passes in
// work[16..32) and their cycles in work[32..38) (printed by bih_sync)
__device__ __forceinline__ unsigned long long fast_walk(const float *boxes, bool cons,
                                                        const cprim_t *prims,
                                                        const cu32_t *dupc, float dx, float dy,
                                                        float dz, float ix, float iy, float iz,
                                                        unsigned long long live, uint32_t lane,
                                                        uint32_t &cand,
                                                        uint32_t &fc_steps, uint32_t &fc_tests) {
    const unsigned long long me = lane_bit(lane);
    unsigned long long found = 0ull;
    uint32_t node = 0;
    unsigned long long mask = live;
    int sp = 0;
    uint32_t st_node = 0, st_lo = 0, st_hi = 0;
    sf32x16 r = fast_rec(boxes, 0);
    while (true) {
        BIH_FC(++fc_steps);
        const uint32_t ref0 = __float_as_uint(r[12]), ref1 = __float_as_uint(r[13]);
        // slab test of both child boxes (camera-relative: t = box * inv); pass
        // 1 clamps the entry at t = 0 (the ray), pass 2 tests the whole line.
        // A dead child's box is NaN: never entered.
        const float cl = cons ? -INFINITY : 0.0f;
        float tn0, tf0, tn1, tf1;
        slab_t(r[0], r[1], r[2], r[3], r[4], r[5], ix, iy, iz, cl, tn0, tf0);
        slab_t(r[6], r[7], r[8], r[9], r[10], r[11], ix, iy, iz, cl, tn1, tf1);
        // child masks and the near child (as the lowest lane entering both
        // sees it), one SALU/VALU sequence (EXEC is the full wave here)
        unsigned long long m0, m1, lt, both;
        uint32_t first1, cnt_both;   // (cnt_both: an SGPR the sequence no longer writes; dropping
                                     // the operand changes the kernel's register allocation)
        asm volatile("v_cmp_le_f32_e64 %[m0], %[tn0], %[tf0]\n\t"
                     "v_cmp_le_f32_e64 %[m1], %[tn1], %[tf1]\n\t"
                     "v_cmp_lt_f32_e64 %[lt], %[tn1], %[tn0]\n\t"
                     "s_and_b64 %[m0], %[m0], %[mask]\n\t"
                     "s_and_b64 %[m1], %[m1], %[mask]\n\t"
                     "s_and_b64 %[both], %[m0], %[m1]\n\t"
                     "s_ff1_i32_b64 %[f1], %[both]\n\t"
                     "s_bitcmp1_b64 %[lt], %[f1]\n\t"
                     "s_cselect_b32 %[f1], 1, 0"
                     : [m0] "=&s"(m0), [m1] "=&s"(m1), [lt] "=&s"(lt), [both] "=&s"(both),
                       [f1] "=&s"(first1), [c] "=&s"(cnt_both)
                     : [tn0] "v"(tn0), [tf0] "v"(tf0), [tn1] "v"(tn1), [tf1] "v"(tf1),
                       [mask] "s"(mask)
                     : "scc");
        if ((ref0 | ref1) & kFastLeaf) {
            // leaf children: test now (near one first)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int s = q ^ (first1 ? 1 : 0);
                const uint32_t ref = s ? ref1 : ref0;
                unsigned long long ms = (s ? m1 : m0) & ~found;
                if (!(ref & kFastLeaf) || !ms) continue;
                const uint32_t k = ref & ~kFastLeaf;
                const uint32_t fc = __float_as_uint(s ? r[15] : r[14]);
                const uint32_t b = fc & 0x3ffffffu;
                const uint32_t c = (fc >> 26) == 63u ? dupc[k] : (fc >> 26);
                for (uint32_t i = b; i < b + c && ms; ++i) {
                    const unsigned long long h = prim_hits(prim_rec(prims, i), dx, dy, dz, ms);
                    if (h & me) cand = k;
                    found |= h;
                    BIH_FC(++fc_tests);
                    ms &= ~h;
                }
            }
            if (ref0 & kFastLeaf) m0 = 0ull;
            if (ref1 & kFastLeaf) m1 = 0ull;
            m0 &= ~found;
            m1 &= ~found;
        }
        // descend: both children -> stack the far one (entry sp in lane sp of
        // st_node/st_lo/st_hi; sp < 31 always: at most one push per level and
        // the Karras tree of distinct 30-bit codes is at most 30 levels deep),
        // one child -> it, none -> pop
        uint32_t pop = 0;
        if (m0 && m1) {
            const uint32_t nf = first1 ? ref0 : ref1;
            const unsigned long long mf = first1 ? m0 : m1;
            uint32_t keep;   // M0 (the lane select) saved and restored
            asm volatile("s_mov_b32 %3, m0\n\t"
                         "s_mov_b32 m0, %7\n\t"
                         "s_nop 0\n\t"
                         "v_writelane_b32 %0, %4, m0\n\t"
                         "v_writelane_b32 %1, %5, m0\n\t"
                         "v_writelane_b32 %2, %6, m0\n\t"
                         "s_mov_b32 m0, %3"
                         : "+v"(st_node), "+v"(st_lo), "+v"(st_hi), "=&s"(keep)
                         : "s"(nf), "s"((uint32_t)mf), "s"((uint32_t)(mf >> 32)), "s"(sp));
            ++sp;
            node = first1 ? ref1 : ref0;
            mask = first1 ? m1 : m0;
        } else if (m0 | m1) {
            node = m0 ? ref0 : ref1;
            mask = m0 | m1;
        } else {
            pop = 1;
        }
        if (pop) {
            mask = 0ull;
            while (sp > 0) {
                --sp;
                mask = (((unsigned long long)__builtin_amdgcn_readlane(st_hi, sp) << 32) |
                        (uint32_t)__builtin_amdgcn_readlane(st_lo, sp)) & ~found;
                if (mask) {
                    node = __builtin_amdgcn_readlane(st_node, sp);
                    break;
                }
            }
            if (!mask) break;
        }
        r = fast_rec(boxes, node);
    }
    return found;
}

// Any-hit shortcut, pass 2: does the reference's own walk reach leaf `k`?
// Per lane, the exact BIH decisions of TraverseTree (CUDAKernels.cu:264-366)
// along the root path of leaf k (left iff k <= split: the Karras ranges),
// on the exact camera-relative records (k_node_prim): visit the near child
// iff tMin < t[near], the far child iff !(tMax < t[far]), intervals [tMin,
// t[near]] / [t[far], tMax] -- the same expressions as the packet walk's
// (BIH_NODE_DEC, BIH_DESCEND).  Every leaf the reference reaches is fully
// tested there, so a lane whose candidate triangle (an exact MT hit with
// 0 < t < FLT_MAX) lies in a reached leaf is a hit of the reference.
__device__ __forceinline__ bool fast_verify(const uint4 *__restrict__ rec, uint32_t k, float ix,
                                            float iy, float iz, float lo, float hi) {
    uint32_t n = 0;
    for (int d = 0; d < 64; ++d) {
        const uint4 r = rec[n];
        const uint32_t ax = r.z & 0xffu, split = r.z >> 8;
        const float inv = sel3(ax, ix, iy, iz);
        const bool neg = 0.0f > inv;
        const bool left = k <= split;
        bool g;
        float nlo, nhi;
        if (left) {
            const float t0 = __uint_as_float(r.x) * inv;
            const float sL = neg ? hi : lo;
            g = (t0 > sL) != neg;
            nlo = neg ? t0 : lo;
            nhi = neg ? hi : t0;
        } else {
            const float t1 = __uint_as_float(r.y) * inv;
            const float sR = neg ? lo : hi;
            g = (!(t1 > sR)) != neg;
            nlo = neg ? lo : t1;
            nhi = neg ? t1 : hi;
        }
        if (!g) return false;
        lo = nlo;
        hi = nhi;
        const uint32_t c = split + (left ? 0u : 1u);
        const bool leaf = left ? ((r.w >> 26) & 1u) : (r.w >> 31);
        if (leaf) return c == k;
        n = c;
    }
    return false;
}

// k_render_packet_asm: k_render_packet2 with the walk as one hand-scheduled
// loop (bih_packet_asm.h); ray setup and writeback stay in HIP.  Triangle
// offsets are 32-bit in the loop: used for scenes of < 2^26 triangles.
// ---------------------------------------------------------------------------
constexpr int kAsmWavesPerEu = 7;
template <bool ANYHIT, bool STATS, int LOG2SPP>
__global__ void __launch_bounds__(kThreads)
__attribute__((amdgpu_waves_per_eu(kAsmWavesPerEu, kAsmWavesPerEu)))
k_render_packet_asm(const RenderArgs a) {
    constexpr uint32_t SPP = 1u << LOG2SPP;
    constexpr uint32_t TW = TileShape<LOG2SPP>::TW, TH = TileShape<LOG2SPP>::TH;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint64_t gwave = (uint64_t)blockIdx.x * (kThreads / 64) + wv;
    const uint32_t *wspill = a.spill + gwave * (uint64_t)(kStackDepth - kPacketRegs) * 3 * 64;
    const SceneU sc = load_scene(a);
    const cprim_t *prims = (const cprim_t *)(const void *)a.tri_prim;
    const void *nodes = (const void *)(STATS ? a.node_prim : a.node_cull);
    const void *dupc = (const void *)a.dup_cnt;
    const uint32_t tiles_x = (a.w + TW - 1) / TW;
    const uint32_t ntiles = tiles_x * ((a.nrows + TH - 1) / TH);
    const uint32_t pix = lane >> LOG2SPP;
    const uint32_t lane4 = lane * 4u;
    const uint32_t snan = 0x7f800001u;
    const uint32_t eps = __float_as_uint(kDetEps), fmax = __float_as_uint(FLT_MAX);

    TileQueue queue = make_queue(a, tiles_x, (a.nrows + TH - 1) / TH);
    uint32_t tile = 0;
    (void)ntiles;
#if BIH_WAVE_TIMELINE
    const uint64_t tl_begin = __builtin_amdgcn_s_memrealtime();
    uint64_t tl_last = tl_begin;
    uint32_t tl_packets = 0, tl_live = 0, tl_max = 0;
    uint64_t tl_max_at = tl_begin, tl_pk = tl_begin;
#endif
    while (queue.next(lane, tile)) {
        const uint64_t t_start = __builtin_amdgcn_s_memtime();
        const PacketRay r = packet_ray<LOG2SPP>(a, sc, tile, lane, tiles_x);
        const bool valid = r.valid, in_box = r.in_box;
        const uint32_t s = r.s, sg = r.sg;
        const uint64_t lp = r.lp;
        const float dx = r.dx, dy = r.dy, dz = r.dz, ix = r.ix, iy = r.iy, iz = r.iz;
        float tMin = r.tMin, tMax = r.tMax;
        uint32_t c_nodes = 0, c_leaves = 0, c_tris = 0;
        unsigned long long live = sc.U > 0 ? __ballot(in_box) : 0ull;
        unsigned long long hits = 0ull, shortcut = 0ull;
#if BIH_FAST_COUNTERS
        uint64_t fc_walk0 = __builtin_amdgcn_s_memtime();
#endif
        if (ANYHIT && !STATS && a.fast && live && sc.U > 1) {
            // any-hit shortcut: lanes whose shortcut hit the reference's walk
            // provably reaches are done; the others take the exact walk below
            uint32_t cand = 0, s1 = 0, n1 = 0, s2 = 0, n2 = 0;
            (void)s1, (void)n1, (void)s2, (void)n2;
            BIH_FC(const uint64_t fc_t0 = __builtin_amdgcn_s_memtime());
            const unsigned long long fin =
                __ballot(__builtin_isfinite(ix) && __builtin_isfinite(iy) && __builtin_isfinite(iz));
            const unsigned long long found =
                fast_walk(a.fast, false, prims, (const cu32_t *)dupc, dx, dy, dz, ix, iy, iz, live,
                          lane, cand, s1, n1);
            BIH_FC(const uint64_t fc_tw = __builtin_amdgcn_s_memtime());
            const bool ok = ((found >> lane) & 1ull) &&
                            fast_verify(a.node_prim, cand, ix, iy, iz, tMin, tMax);
            shortcut = __ballot(ok);
            BIH_FC(const unsigned long long fc_live0 = live);
            BIH_FC(const uint32_t fc_v1 = (uint32_t)__popcll(shortcut));
            live &= ~shortcut;
            BIH_FC(const uint64_t fc_t1 = __builtin_amdgcn_s_memtime());
            // miss proof for the rest (lanes with an infinite 1/D component
            // keep the exact walk: 0 * inf in a slab test)
            const unsigned long long m2 = a.fast2 ? live & fin : 0ull;
            if (m2) {
                const unsigned long long found2 =
                    fast_walk(a.fast2, true, prims, (const cu32_t *)dupc, dx, dy, dz, ix, iy, iz,
                              m2, lane, cand, s2, n2);
                const bool ok2 = ((found2 >> lane) & 1ull) &&
                                 fast_verify(a.node_prim, cand, ix, iy, iz, tMin, tMax);
                const unsigned long long hit2 = __ballot(ok2);
                shortcut |= hit2;
                live &= ~(hit2 | (m2 & ~found2));   // proven misses are done too
                BIH_FC(if (lane == 0) {
                    atomicAdd(a.work + 22, 1u);
                    atomicAdd(a.work + 23, s2);
                    atomicAdd(a.work + 24, n2);
                    atomicAdd(a.work + 25, (uint32_t)__popcll(hit2));
                    atomicAdd(a.work + 26, (uint32_t)__popcll(m2 & ~found2));
                })
            }
#if BIH_FAST_COUNTERS
            const uint64_t fc_t2 = __builtin_amdgcn_s_memtime();
            if (lane == 0) {
                unsigned long long *cy = reinterpret_cast<unsigned long long *>(a.work + 32);
                atomicAdd(a.work + 16, 1u);
                atomicAdd(a.work + 17, (uint32_t)__popcll(fc_live0));
                atomicAdd(a.work + 18, s1);
                atomicAdd(a.work + 19, n1);
                atomicAdd(a.work + 20, (uint32_t)__popcll(found));
                atomicAdd(a.work + 21, fc_v1);
                atomicAdd(a.work + 28, live ? 1u : 0u);
                atomicAdd(a.work + 29, (uint32_t)__popcll(live));
                atomicAdd(cy, (unsigned long long)(fc_t1 - fc_t0));
                atomicAdd(cy + 1, (unsigned long long)(fc_t2 - fc_t1));
                atomicAdd(cy + 3, (unsigned long long)(fc_tw - fc_t0));
            }
            fc_walk0 = __builtin_amdgcn_s_memtime();
#endif
        }
        uint32_t nearbits = 0;
#pragma unroll
        for (uint32_t k = 0; k < 3; ++k) {
            const unsigned long long neg = __ballot((sg >> k) & 1u) & live;
            if (__popcll(neg) * 2 <= __popcll(live)) nearbits |= 1u << k;
        }
        nearbits = __builtin_amdgcn_readfirstlane(nearbits);
        if (live && sc.U == 1) {                          // single leaf (reference: UB)
            unsigned long long m = live;
            if (STATS && (m & lane_bit(lane))) ++c_leaves;
            for (uint32_t b = 0; b < sc.N; ++b) {
                if (ANYHIT) {
                    m &= ~hits;
                    if (!m) break;
                }
                if (STATS && (m & lane_bit(lane))) ++c_tris;
                hits |= prim_hits(prims[b], dx, dy, dz, m);
            }
        } else if (live) {
            if constexpr (ANYHIT && !STATS) {
                asm volatile(BIH_PACKET_WALK(BIH_ANY_ON, BIH_CLR_ON, BIH_POP_ANY, "", "", "", "", "")
                             : BIH_PACKET_OUT : BIH_PACKET_IN : BIH_PACKET_CLOBBERS);
            } else if constexpr (ANYHIT && STATS) {
                asm volatile(BIH_PACKET_WALK(BIH_ANY_ON, BIH_CLR_ON, BIH_POP_ANY, BIH_CNT_NODE, BIH_CNT_LEAF_L,
                                             BIH_CNT_LEAF_R, BIH_CNT_TRI_L, BIH_CNT_TRI_R)
                             : BIH_PACKET_OUT_CNT : BIH_PACKET_IN : BIH_PACKET_CLOBBERS);
            } else if constexpr (!ANYHIT && !STATS) {
                asm volatile(BIH_PACKET_WALK(BIH_ANY_OFF, BIH_CLR_OFF, "", "", "", "", "", "")
                             : BIH_PACKET_OUT : BIH_PACKET_IN : BIH_PACKET_CLOBBERS);
            } else {
                asm volatile(BIH_PACKET_WALK(BIH_ANY_OFF, BIH_CLR_OFF, "", BIH_CNT_NODE, BIH_CNT_LEAF_L,
                                             BIH_CNT_LEAF_R, BIH_CNT_TRI_L, BIH_CNT_TRI_R)
                             : BIH_PACKET_OUT_CNT : BIH_PACKET_IN : BIH_PACKET_CLOBBERS);
            }
        }
        hits |= shortcut;
#if BIH_FAST_COUNTERS
        if (lane == 0 && live)
            atomicAdd(reinterpret_cast<unsigned long long *>(a.work + 32) + 2,
                      (unsigned long long)(__builtin_amdgcn_s_memtime() - fc_walk0));
#endif

        if (STATS && valid) write_ray_stats(a, lp * SPP + s, c_nodes, c_leaves, c_tris);
        if (valid && s == SPP - 1) a.out[lp] = pixel_of_mask<SPP>(hits, pix);
        // the longest packet of a chunk (cycles) orders the chunk in the next
        // frames (k_chunk_order): a chunk's packets run side by side on one
        // CU, so its longest packet is what has to start early
        if (a.chunk_cost && lane == 0)
            atomicMax(a.chunk_cost + queue.chunk,
                      (uint32_t)(__builtin_amdgcn_s_memtime() - t_start));
#if BIH_WAVE_TIMELINE
        {
            // 100 MHz real-time clock (one time base for every XCD)
            const uint64_t now = __builtin_amdgcn_s_memrealtime();
            const uint32_t dt = (uint32_t)(now - tl_pk);
            const uint64_t t_start = tl_pk;
            tl_pk = now;
            tl_last = t_start;
            ++tl_packets;
            tl_live += live ? 1u : 0u;
            if (dt > tl_max) {
                tl_max = dt;
                tl_max_at = t_start;
            }
        }
#endif
    }
#if BIH_WAVE_TIMELINE
    // debug builds: {begin, end, last packet start} u64, packets, live packets,
    // longest packet (cycles) at the wave's spill base (bih_sync prints them)
    if (lane == 0) {
        uint32_t *r = const_cast<uint32_t *>(wspill);
        const uint64_t tl_end = __builtin_amdgcn_s_memrealtime();
        const uint64_t v[3] = {tl_begin, tl_end, tl_last};
        for (int k = 0; k < 3; ++k) {
            r[2 * k] = (uint32_t)v[k];
            r[2 * k + 1] = (uint32_t)(v[k] >> 32);
        }
        r[6] = tl_packets;
        r[7] = tl_live;
        r[8] = tl_max;
        r[9] = xcc_id();
        r[10] = (uint32_t)tl_max_at;
        r[11] = (uint32_t)(tl_max_at >> 32);
    }
#endif
}

// Chunk order of the persistent packet kernel: within each of the kRegions
// bands (TileQueue::band_begin), chunks by descending cost (the cycles their
// longest packet took in an earlier frame of the same geometry), ties by index, so
// that the slow chunks start first and the frame does not end on one long
// packet (longest-processing-time-first).  One block per band sorts the
// band's keys (~cost << 32 | index: descending cost, ascending index; padded
// to a power of two with all-ones keys) bitonically in LDS.  Bands of more
// than kOrderMax chunks keep the identity order.  Only the order of the work
// changes, never a pixel.
constexpr uint32_t kOrderMax = 4096;
__global__ void __launch_bounds__(kThreads) k_chunk_order(const uint32_t *__restrict__ cost,
                                                          uint32_t chunks_x, uint32_t nchunks,
                                                          uint32_t *__restrict__ order) {
    __shared__ unsigned long long key[kOrderMax];
    const uint32_t rows = nchunks / chunks_x, b = blockIdx.x;
    const uint32_t b0 = (uint32_t)(((uint64_t)rows * b) / kRegions) * chunks_x;
    const uint32_t b1 = (uint32_t)(((uint64_t)rows * (b + 1)) / kRegions) * chunks_x;
    const uint32_t n = b1 - b0;
    if (n > kOrderMax) {
        for (uint32_t i = threadIdx.x; i < n; i += kThreads) order[b0 + i] = b0 + i;
        return;
    }
    uint32_t np = 1;
    while (np < n) np <<= 1;
    for (uint32_t i = threadIdx.x; i < np; i += kThreads)
        key[i] = i < n ? ((unsigned long long)(~cost[b0 + i]) << 32) | i : ~0ull;
    __syncthreads();
    for (uint32_t k = 2; k <= np; k <<= 1)
        for (uint32_t jj = k >> 1; jj > 0; jj >>= 1) {
            for (uint32_t i = threadIdx.x; i < np; i += kThreads) {
                const uint32_t l = i ^ jj;
                if (l > i) {
                    const unsigned long long x = key[i], y = key[l];
                    const bool up = (i & k) == 0;
                    if ((x > y) == up) {
                        key[i] = y;
                        key[l] = x;
                    }
                }
            }
            __syncthreads();
        }
    for (uint32_t i = threadIdx.x; i < n; i += kThreads) order[b0 + i] = b0 + (uint32_t)key[i];
}

enum class Variant { Packet1, Packet2, PacketAsm };

Variant variant_from_env() {
    const char *e = getenv("BIH_RENDER_KERNEL");
    if (e && strcmp(e, "packet1") == 0) return Variant::Packet1;
    if (e && strcmp(e, "packet2") == 0) return Variant::Packet2;
    return Variant::PacketAsm;
}

// The camera-relative records (k_node_prim) hold split << 8 and mid < 2^26,
// and the asm walk forms 32-bit triangle byte offsets (64 B records).
bool packet_records_fit(const RenderArgs &a) {
    return a.hdr_n_tris < (1u << 26) && a.n_nodes < (1u << 24);
}

// The kernel of (variant, any-hit, stats) at tile shape L; Packet1 (the packed
// canonical nodes: any scene size) where the camera-relative records do not fit.
using RenderKernel = void (*)(RenderArgs);
#define BIH_AS(k, ...) {{k<false, false, ##__VA_ARGS__>, k<false, true, ##__VA_ARGS__>}, \
                        {k<true, false, ##__VA_ARGS__>, k<true, true, ##__VA_ARGS__>}}
template <int L>
RenderKernel packet_kernel(Variant var, const RenderArgs &a, uint32_t traverse) {
    static const RenderKernel ks[3][2][2] = {BIH_AS(k_render_packet, L), BIH_AS(k_render_packet2, L),
                                             BIH_AS(k_render_packet_asm, L)};
    return ks[packet_records_fit(a) ? (int)var : (int)Variant::Packet1][traverse == 0][a.ray_stats != nullptr];
}

}  // namespace

// Resident blocks of the persistent kernels on `device` (grid size).
uint32_t wave_grid_blocks(int device) {
    static std::mutex mu;
    static uint32_t cache[64] = {0};
    std::lock_guard<std::mutex> lk(mu);
    if (device < 0 || device >= 64) return 0;
    if (!cache[device]) {
        // resident blocks per CU: the largest over the persistent kernels
        // (the LDS-stack kernels fit fewer than the register-stack packet ones)
        const void *kernels[] = {
            reinterpret_cast<const void *>(k_render_packet<true, false, 2>),
            reinterpret_cast<const void *>(k_render_packet2<true, false, 2>),
            reinterpret_cast<const void *>(k_render_packet_asm<true, false, 2>),
        };
        int cus = 0, per = 0;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
        for (const void *k : kernels) {
            int p = 0;
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&p, k, kThreads, 0);
            if (p > per) per = p;
        }
        if (cus <= 0) cus = 256;
        if (per <= 0) per = 1;
        // tuning knob: resident blocks per CU (the occupancy API's answer otherwise)
        if (const char *e = getenv("BIH_BLOCKS_PER_CU")) {
            const int v = atoi(e);
            if (v > 0 && v <= 32) per = v;
        }
        cache[device] = (uint32_t)(cus * per);
    }
    return cache[device];
}

size_t spill_words(uint32_t blocks) {
    // per block: per-lane kernels [(32-kLdsStack)*3][256 lanes]; packet kernel
    // 4 waves x [(32-kPacketRegs)*3][64 lanes] -- size for the larger
    const size_t lane_k = (size_t)kThreads * (kStackDepth - kLdsStack) * 3;
    const size_t packet_k = (size_t)(kThreads / 64) * (kStackDepth - kPacketRegs) * 3 * 64;
    return (size_t)blocks * (lane_k > packet_k ? lane_k : packet_k);
}

uint32_t chunk_count(uint32_t w, uint32_t nrows, uint32_t spp, uint32_t *chunks_x) {
    if (spp == 0 || spp > 64 || (spp & (spp - 1)) != 0) return 0;
    const Tiles t = tiles_of(w, nrows, spp);
    const uint32_t cx = (t.x + kChunkW - 1) / kChunkW;
    if (chunks_x) *chunks_x = cx;
    return cx * ((t.y + kChunkH - 1) / kChunkH);
}

int launch_chunk_order(const uint32_t *cost, uint32_t chunks_x, uint32_t nchunks, uint32_t *order,
                       void *stream) {
    if (nchunks == 0) return 0;
    hipLaunchKernelGGL(k_chunk_order, dim3(kRegions), dim3(kThreads), 0, (hipStream_t)stream, cost,
                       chunks_x, nchunks, order);
    return (int)hipGetLastError();
}

// Renders without frustum bins: the packet walk (spp a power of two <= 64) or
// the pixel kernel.
int launch_walk(const RenderArgs &a, uint32_t traverse, void *stream, void *ev_k0, void *ev_k1) {
    hipStream_t st = (hipStream_t)stream;
    const hipEvent_t k0 = (hipEvent_t)ev_k0, k1 = (hipEvent_t)ev_k1;
    const uint32_t spp = a.spp;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const uint32_t grid = wave_grid_blocks(dev);
    if (spp <= 64 && (spp & (spp - 1)) == 0) {
        static const Variant var = variant_from_env();
        const uint64_t tiles = tiles_of(a.w, a.nrows, spp).count();
        if (tiles == 0) return 0;
        uint32_t blocks = (uint32_t)((tiles + 3) / 4);
        if (blocks > grid) blocks = grid;
        // the tile queue of the per-CU slots starts from zero; the bins' item
        // queue resets itself (counter builds also count into a.work)
        hipError_t e = hipMemsetAsync(a.work, 0, kWorkWords * sizeof(uint32_t), st);
        if (e == hipSuccess && k0) e = hipEventRecord(k0, st);
        if (e != hipSuccess) return (int)e;
        const RenderKernel k =
            with_log2spp(spp, [&](auto l) { return packet_kernel<decltype(l)::value>(var, a, traverse); });
        hipLaunchKernelGGL(k, dim3(blocks), dim3(kThreads), 0, st, a);
        e = hipGetLastError();
        if (e == hipSuccess && k1) e = hipEventRecord(k1, st);
        return (int)e;
    }
    // any other spp: one lane per pixel, grid-stride, grid capped at the spill area
    const uint32_t tiles = ((a.w + 7) >> 3) * ((a.nrows + 7) >> 3);
    if (tiles == 0) return 0;
    uint32_t blocks = (tiles + 3) / 4;
    if (blocks > grid) blocks = grid;
    static const RenderKernel px[2][2] = BIH_AS(k_render_pixel);
    if (k0) (void)hipEventRecord(k0, st);
    hipLaunchKernelGGL(px[traverse == 0][a.ray_stats != nullptr], dim3(blocks), dim3(kThreads), 0, st, a);
    if (k1) (void)hipEventRecord(k1, st);
    return (int)hipGetLastError();
}

}  // namespace bih
