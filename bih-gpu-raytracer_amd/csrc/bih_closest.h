// bih_closest.h -- the per-lane closest-hit BIH walk (the oracle's
// traverse_closest), shared by the ray queries (bih_trace.hip), the G-buffer
// (bih_gbuffer.hip) and config C4's bounces (bih_whitted.hip).
//
// Semantics: min (t, sorted position) over the
// triangles the reference walk tests (TraverseTree's decisions and order,
// CUDAKernels.cu:227-368; RayTriangleIntersection :17-50), t_lo < t < FLT_MAX;
// once a hit is known a node entered beyond it is popped and tMax is clamped
// to it; with t_lo > 0 the walk interval starts at max(box entry, t_lo).
// Every f32 expression is the oracle's, in its order (-ffp-contract=off).
// ANY ends the same walk at the first accepted triangle: until then it has
// the closest walk's visit order, interval clamp and accept test, so "some
// triangle was accepted" is exactly (closest bi != kNoHit).
// WITHIN (segment queries, a ray with a far end t_hi) is the closest walk too
// -- the same accepts, the same bt / bi updates and interval clamp, also for
// hits at or beyond t_hi -- ended at the first accepted triangle with
// t < t_hi.  bt only decreases, so the closest walk's final t is below t_hi
// exactly when some accepted t was: (bi != kNoHit && bt < t_hi) after this
// walk is that of the whole closest walk, and the walk is a prefix of it.
// t_hi bounds no interval and seeds no best hit (the walk culls with f32
// plane distances: that would be another visit set).
//
// The ray's origin and t_lo are arguments, not walk state: a caller whose
// origin is wave-uniform (the G-buffer: kernel arguments) keeps it in SGPRs,
// and a literal t_lo = 0 folds its tests away.
#pragma once
#include <float.h>

#include "bih_device.h"

namespace bih {
namespace dev {

constexpr uint32_t kNoHit = 0xFFFFFFFFu;
constexpr uint32_t kLanes = 64;          // the walk's kernels run one-wave blocks

// Where the walk ends (compile time; false / true of the two first read as before).
constexpr int kWalkClosest = 0;          // when no node is left
constexpr int kWalkAny = 1;              // at the first accepted triangle
constexpr int kWalkWithin = 2;           // at the first accepted triangle with t < ClosestRay::t_hi

__device__ __forceinline__ float pick3(uint32_t ax, float a, float b, float c) {
    return ax == 0 ? a : (ax == 1 ? b : c);
}

struct ClosestScene {
    const uint4 *nodes;
    const float *tris;          // sorted {v0, e1, e2}
    const uint32_t *dup;
    float slo[3], shi[3];
    uint32_t U, N;
};

__device__ __forceinline__ ClosestScene load_closest_scene(const TreeHeader *hdr, const uint4 *nodes,
                                                           const float *tris, const uint32_t *dup) {
    ClosestScene s;
    s.nodes = nodes;
    s.tris = tris;
    s.dup = dup;
    for (int k = 0; k < 3; ++k) {
        s.slo[k] = hdr->scene_lo[k];
        s.shi[k] = hdr->scene_hi[k];
    }
    s.U = hdr->n_unique;
    s.N = hdr->n_tris;
    return s;
}

// RayTriangleIntersection (CUDAKernels.cu:17-50) on a {v0, e1, e2} record:
// true when the ray passes the determinant and barycentric tests; t, u, v as
// the reference computes them (dot = (x + y) + z, inv = 1.0f / det).
__device__ __forceinline__ bool mt_tuv(const float *__restrict__ tp, const float *o, const float *d, float &t,
                                       float &u, float &v) {
    const float v0x = tp[0], v0y = tp[1], v0z = tp[2];
    const float e1x = tp[3], e1y = tp[4], e1z = tp[5];
    const float e2x = tp[6], e2y = tp[7], e2z = tp[8];
    const float dx = d[0], dy = d[1], dz = d[2];
    const float px = dy * e2z - e2y * dz;                  // pvec = cross(D, e2)
    const float py = dz * e2x - e2z * dx;
    const float pz = dx * e2y - e2x * dy;
    const float det = (e1x * px + e1y * py) + e1z * pz;
    if (det <= kDetEps) return false;                      // det < 0.000001 (double); NaN passes
    const float inv = 1.0f / det;
    const float sx = o[0] - v0x, sy = o[1] - v0y, sz = o[2] - v0z;
    u = ((sx * px + sy * py) + sz * pz) * inv;
    if (u < 0.0f || u > 1.0f) return false;
    const float qx = sy * e1z - e1y * sz;                  // qvec = cross(tvec, e1)
    const float qy = sz * e1x - e1z * sx;
    const float qz = sx * e1y - e1x * sy;
    v = ((dx * qx + dy * qy) + dz * qz) * inv;
    if (v < 0.0f || u + v > 1.0f) return false;
    t = ((e2x * qx + e2y * qy) + e2z * qz) * inv;
    return true;
}

// Per-lane stack: slots [0, LDS) in LDS at [slot * kLanes] from this lane's
// base, deeper slots in this thread's memory area (slot-major,
// grid-interleaved: (kStackDepth - LDS) * 3 words per thread of the grid).
template <int LDS>
struct LaneStack {
    uint32_t *sn;
    float *smin, *smax;
    uint32_t *spill;           // + gtid; slot k >= LDS at ((k - LDS) * 3) * gthreads
    uint64_t gthreads;
    // s_node, s_min, s_max: the block's LDS * kLanes words each
    __device__ __forceinline__ LaneStack(uint32_t *s_node, float *s_min, float *s_max, uint32_t *spill_area)
        : sn(s_node + threadIdx.x), smin(s_min + threadIdx.x), smax(s_max + threadIdx.x),
          spill(spill_area + (uint64_t)blockIdx.x * kLanes + threadIdx.x), gthreads((uint64_t)gridDim.x * kLanes) {}
    __device__ __forceinline__ void push(uint32_t sp, uint32_t n, float lo, float hi) const {
        if (sp < (uint32_t)LDS) {
            sn[sp * kLanes] = n; smin[sp * kLanes] = lo; smax[sp * kLanes] = hi;
        } else {
            uint32_t *q = spill + (uint64_t)(sp - LDS) * 3 * gthreads;
            q[0] = n; q[gthreads] = __float_as_uint(lo); q[2 * gthreads] = __float_as_uint(hi);
        }
    }
    __device__ __forceinline__ void pop(uint32_t sp, uint32_t &n, float &lo, float &hi) const {
        if (sp < (uint32_t)LDS) {
            n = sn[sp * kLanes]; lo = smin[sp * kLanes]; hi = smax[sp * kLanes];
        } else {
            const uint32_t *q = spill + (uint64_t)(sp - LDS) * 3 * gthreads;
            n = q[0]; lo = __uint_as_float(q[gthreads]); hi = __uint_as_float(q[2 * gthreads]);
        }
    }
};

// One ray's walk state (its origin and t_lo stay with the caller).  The caller
// sets d; closest_start the rest.  nd: the record of node cur, requested by
// the previous step (one memory round trip per step).
struct ClosestRay {
    float d[3], ix, iy, iz, tMin, tMax, bt;
    uint32_t sg, cur, sp, bi;
    uint4 nd;
    float t_hi;                 // kWalkWithin only (set by the caller; the other modes never touch it)
};

// kWalkWithin's answer once its walk has ended (one strict f32 compare: a NaN
// t_hi gives false).
__device__ __forceinline__ bool within_hit(const ClosestRay &r) { return r.bi != kNoHit && r.bt < r.t_hi; }

// Leaf triangles [b, e): the (t, i) rule with t_lo < t < FLT_MAX.  kWalkAny:
// ends at the first accepted triangle (true); kWalkWithin: at the first
// accepted one below t_hi.
template <int MODE>
__device__ __forceinline__ bool closest_leaf(const ClosestScene &s, ClosestRay &r, const float *o, float t_lo,
                                             uint32_t b, uint32_t e) {
    for (uint32_t i = b; i < e; ++i) {
        float t, u, v;
        if (mt_tuv(s.tris + 9ull * i, o, r.d, t, u, v) && t > t_lo && t < FLT_MAX &&
            (t < r.bt || (t == r.bt && i < r.bi))) {
            r.bt = t;
            r.bi = i;
            if (MODE == kWalkAny) return true;
            if (MODE == kWalkWithin && t < r.t_hi) return true;
        }
    }
    return false;
}

// The walk's prologue (traverse_closest up to its loop); true when the ray
// has nodes to walk, false when its result is final (it misses the scene box,
// or the tree has no internal node: U <= 1 is one leaf of all N triangles and
// has no node record to read).
template <int MODE>
__device__ __forceinline__ bool closest_start(const ClosestScene &s, ClosestRay &r, const float *o, float t_lo) {
    r.bt = FLT_MAX;
    r.bi = kNoHit;
    r.cur = 0;
    r.sp = 0;
    r.ix = 1.0f / r.d[0];
    r.iy = 1.0f / r.d[1];
    r.iz = 1.0f / r.d[2];
    r.sg = (r.ix < 0.0f ? 1u : 0u) | (r.iy < 0.0f ? 2u : 0u) | (r.iz < 0.0f ? 4u : 0u);
    // scene-AABB slab test, CUDAKernels.cu:237-262 (tMin may be negative)
    float tMin = (((r.sg & 1) ? s.shi[0] : s.slo[0]) - o[0]) * r.ix;
    float tMax = (((r.sg & 1) ? s.slo[0] : s.shi[0]) - o[0]) * r.ix;
    const float tymin = (((r.sg & 2) ? s.shi[1] : s.slo[1]) - o[1]) * r.iy;
    const float tymax = (((r.sg & 2) ? s.slo[1] : s.shi[1]) - o[1]) * r.iy;
    if ((tMin > tymax) || (tymin > tMax)) return false;
    if (tymin > tMin) tMin = tymin;
    if (tymax < tMax) tMax = tymax;
    const float tzmin = (((r.sg & 4) ? s.shi[2] : s.slo[2]) - o[2]) * r.iz;
    const float tzmax = (((r.sg & 4) ? s.slo[2] : s.shi[2]) - o[2]) * r.iz;
    if ((tMin > tzmax) || (tzmin > tMax)) return false;
    if (tzmin > tMin) tMin = tzmin;
    if (tzmax < tMax) tMax = tzmax;
    if (t_lo > 0.0f && tMin < t_lo) tMin = t_lo;   // the walk starts at t_lo (oracle)
    if (s.U < 2) {   // single leaf (reference: UB; defined as the oracle's)
        (void)closest_leaf<MODE>(s, r, o, t_lo, 0, s.U ? s.N : 0u);
        return false;
    }
    r.tMin = tMin;
    r.tMax = tMax;
    r.nd = s.nodes[0];
    return true;
}

// One iteration of traverse_closest's loop; true when the walk has ended.
// The next node's record is requested before the leaves this step visits are
// tested, so the node load and the leaves' triangle loads are in flight
// together (they are still tested before the next node's decisions read the
// best hit: the same decisions, the same hit).  COUNT: nodes entered (cn) and
// triangles tested (ct), for the work counters.
template <int MODE, bool COUNT, int LDS>
__device__ __forceinline__ bool closest_step(const ClosestScene &s, ClosestRay &r, const float *o, float t_lo,
                                             const LaneStack<LDS> &stk, uint32_t &cn, uint32_t &ct) {
    const float best = r.bi != kNoHit ? r.bt : __builtin_inff();
    if (r.tMin > best) {                          // entered beyond the best hit: skip
        if (r.sp == 0) return true;
        --r.sp;
        stk.pop(r.sp, r.cur, r.tMin, r.tMax);
        r.nd = s.nodes[r.cur];
        return false;
    }
    if (best < r.tMax) r.tMax = best;
    if (COUNT) ++cn;
    const uint4 nd = r.nd;
    const uint32_t ax = (nd.z >> 27) & 3u;
    const float org = pick3(ax, o[0], o[1], o[2]), inv = pick3(ax, r.ix, r.iy, r.iz);
    const uint32_t nr = (r.sg >> ax) & 1u;
    const float t0 = (__uint_as_float(nd.x) - org) * inv;
    const float t1 = (__uint_as_float(nd.y) - org) * inv;
    const float tn = nr ? t1 : t0, tf = nr ? t0 : t1;
    const bool A = r.tMin < tn, B = r.tMax < tf;
    const uint32_t split = nd.z & kIdxMask, mid = nd.w & kIdxMask;
    const bool leafL = (nd.z >> 29) & 1u, leafR = (nd.z >> 30) & 1u;
    const bool leafN = nr ? leafR : leafL, leafF = nr ? leafL : leafR;
    uint32_t cL = (nd.w >> 27) & 3u, cR = (nd.w >> 29) & 3u;
    if (leafL && cL == 0) cL = s.dup[split];
    if (leafR && cR == 0) cR = s.dup[split + 1];
    const uint32_t nb = nr ? mid : mid - cL, ne = nr ? mid + cR : mid;
    const uint32_t fb = nr ? mid - cL : mid, fe = nr ? mid : mid + cR;
    const uint32_t nearc = split + nr, farc = split + 1u - nr;
    // the leaves this step visits, in the walk's order: [l0b, l0e) then [l1b, l1e)
    uint32_t l0b = 0, l0e = 0, l1b = 0, l1e = 0;
    bool pop = false;
    if (!A && B) {
        pop = true;
    } else if (A && B) {
        if (leafN) { l0b = nb; l0e = ne; pop = true; }
        else { r.cur = nearc; r.tMax = tn; }
    } else if (!A && !B) {
        if (leafF) { l0b = fb; l0e = fe; pop = true; }
        else { r.cur = farc; r.tMin = tf; }
    } else {
        if (leafN && leafF) {
            l0b = nb; l0e = ne;
            l1b = fb; l1e = fe;
            pop = true;
        } else if (!leafN && leafF) {
            l0b = fb; l0e = fe;
            r.cur = nearc; r.tMax = tn;
        } else if (leafN && !leafF) {
            l0b = nb; l0e = ne;
            r.cur = farc; r.tMin = tf;
        } else {
            stk.push(r.sp, farc, tf, r.tMax);
            ++r.sp;
            r.cur = nearc; r.tMax = tn;
        }
    }
    bool fin = false;
    if (pop) {
        if (r.sp == 0) {
            fin = true;
        } else {
            --r.sp;
            stk.pop(r.sp, r.cur, r.tMin, r.tMax);
        }
    }
    if (!fin) r.nd = s.nodes[r.cur];
    if (COUNT) ct += (l0e - l0b) + (l1e - l1b);
    if (closest_leaf<MODE>(s, r, o, t_lo, l0b, l0e)) return true;   // (kWalkAny, kWalkWithin) an accepted triangle ends the walk
    if (closest_leaf<MODE>(s, r, o, t_lo, l1b, l1e)) return true;
    return fin;
}

template <int MODE, int LDS>
__device__ __forceinline__ bool closest_step(const ClosestScene &s, ClosestRay &r, const float *o, float t_lo,
                                             const LaneStack<LDS> &stk) {
    uint32_t cn = 0, ct = 0;
    return closest_step<MODE, false>(s, r, o, t_lo, stk, cn, ct);
}

}  // namespace dev
}  // namespace bih
