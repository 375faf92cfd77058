// bih_trace.hip -- ray queries (bih_trace_device / bih_trace, include/bih.h):
// closest hit and occlusion for caller-supplied rays on gfx950.
//
// Semantics are config C4's closest hit, the oracle's
// traverse_closest: min (t, sorted position) over the triangles the reference
// walk tests (TraverseTree's decisions and order, CUDAKernels.cu:227-368;
// RayTriangleIntersection :17-50), t_lo < t < FLT_MAX; once a hit is known a
// node entered beyond it is popped and tMax is clamped to it; with t_lo > 0
// the walk interval starts at max(box entry, t_lo).  Every f32 expression is
// the oracle's, in its order (-ffp-contract=off).  The occlusion query is the
// same walk ended at the first accepted triangle: until then it has the
// closest walk's visit order, interval clamp and accept test, so its flag is
// exactly (closest prim != BIH_NO_HIT).
//
// Caller rays are incoherent and their walks very unequal, so the kernel has
// k_wh_trace_dyn's shape (bih_whitted.hip): persistent one-wave blocks; a lane
// whose walk has ended takes the next ray index from a global cursor while its
// wave-mates keep walking (idle lanes are refilled with one atomic per wave);
// each result goes to its ray's own slot, in caller order.  The walk is
// written anew here (it also ends early for occlusion and keeps t_lo per
// ray); bih_whitted.hip's is left as it is.
#include <hip/hip_runtime.h>
#include <float.h>

#include "bih_device.h"
#include "bih_internal.h"

namespace bih {
namespace {

using dev::kDetEps;

constexpr uint32_t kTT = 64;             // threads per block: one wave
constexpr uint32_t kTBlocksPerCU = 32;   // persistent grid (as k_wh_trace)
constexpr uint32_t kNoHit = 0xFFFFFFFFu;
constexpr int kTRefill = 16;             // idle lanes of a wave that trigger a refill (as k_wh_trace_dyn)
constexpr int kTSteps = 256;             // walk steps per lane between refill checks (as k_wh_trace_dyn)

struct TScene {
    const uint4 *nodes;
    const float *tris;          // sorted {v0, e1, e2}
    const uint32_t *dup;
    float slo[3], shi[3];
    uint32_t U, N;
};

struct TraceArgs {
    const TreeHeader *hdr;
    const uint4 *nodes;
    const float *tris;
    const uint32_t *dup;
    const uint32_t *tri_idx;    // sorted position -> file order (BIH_ARR_TRI_INDEX)
    const float4 *rays;         // bih_ray: {o, t_lo}, {d, reserved}
    void *out;                  // bih_hit[n] or u8[n]
    uint32_t n;
    uint32_t *cursor;           // rays taken so far (zero at launch)
    uint32_t *spill;
};

__device__ __forceinline__ float pick3(uint32_t ax, float a, float b, float c) {
    return ax == 0 ? a : (ax == 1 ? b : c);
}

// One ray's walk state.  nd: the record of node cur, requested by the
// previous step (one memory round trip per step, as k_wh_trace_dyn).
struct TRay {
    float o[3], d[3], ix, iy, iz, tMin, tMax, bt, t_lo;
    uint32_t sg, cur, sp, bi, id;
    uint4 nd;
};

// RayTriangleIntersection (CUDAKernels.cu:17-50) on a {v0, e1, e2} record:
// true when the ray passes the determinant and barycentric tests; t, u, v as
// the reference computes them (dot = (x + y) + z, inv = 1.0f / det).
__device__ __forceinline__ bool mt_tuv(const float *__restrict__ tp, const TRay &r, float &t, float &u, float &v) {
    const float v0x = tp[0], v0y = tp[1], v0z = tp[2];
    const float e1x = tp[3], e1y = tp[4], e1z = tp[5];
    const float e2x = tp[6], e2y = tp[7], e2z = tp[8];
    const float dx = r.d[0], dy = r.d[1], dz = r.d[2];
    const float px = dy * e2z - e2y * dz;                  // pvec = cross(D, e2)
    const float py = dz * e2x - e2z * dx;
    const float pz = dx * e2y - e2x * dy;
    const float det = (e1x * px + e1y * py) + e1z * pz;
    if (det <= kDetEps) return false;                      // det < 0.000001 (double); NaN passes
    const float inv = 1.0f / det;
    const float sx = r.o[0] - v0x, sy = r.o[1] - v0y, sz = r.o[2] - v0z;
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

// Leaf triangles [b, e): the (t, i) rule with t_lo < t < FLT_MAX.  ANY: ends
// at the first accepted triangle (true).
template <bool ANY>
__device__ __forceinline__ bool tleaf(const TScene &s, TRay &r, uint32_t b, uint32_t e) {
    for (uint32_t i = b; i < e; ++i) {
        float t, u, v;
        if (mt_tuv(s.tris + 9ull * i, r, t, u, v) && t > r.t_lo && t < FLT_MAX &&
            (t < r.bt || (t == r.bt && i < r.bi))) {
            r.bt = t;
            r.bi = i;
            if (ANY) return true;
        }
    }
    return false;
}

// Per-lane stack: slots [0, LDS) in LDS at [slot * kTT] from this lane's
// base, deeper slots in this thread's HBM area (slot-major, grid-interleaved;
// as WStack, bih_whitted.hip).
template <int LDS>
struct TStack {
    uint32_t *sn;
    float *smin, *smax;
    uint32_t *spill;           // + gtid; slot k >= LDS at ((k - LDS) * 3) * gthreads
    uint64_t gthreads;
    __device__ __forceinline__ void push(uint32_t sp, uint32_t n, float lo, float hi) const {
        if (sp < (uint32_t)LDS) {
            sn[sp * kTT] = n; smin[sp * kTT] = lo; smax[sp * kTT] = hi;
        } else {
            uint32_t *q = spill + (uint64_t)(sp - LDS) * 3 * gthreads;
            q[0] = n; q[gthreads] = __float_as_uint(lo); q[2 * gthreads] = __float_as_uint(hi);
        }
    }
    __device__ __forceinline__ void pop(uint32_t sp, uint32_t &n, float &lo, float &hi) const {
        if (sp < (uint32_t)LDS) {
            n = sn[sp * kTT]; lo = smin[sp * kTT]; hi = smax[sp * kTT];
        } else {
            const uint32_t *q = spill + (uint64_t)(sp - LDS) * 3 * gthreads;
            n = q[0]; lo = __uint_as_float(q[gthreads]); hi = __uint_as_float(q[2 * gthreads]);
        }
    }
};

// The walk's prologue (traverse_closest up to its loop); true when the ray
// has nodes to walk, false when its result is final (it misses the scene box,
// or the tree has no internal node: U <= 1 is one leaf of all N triangles).
template <bool ANY>
__device__ __forceinline__ bool tray_start(const TScene &s, TRay &r) {
    r.bt = FLT_MAX;
    r.bi = kNoHit;
    r.cur = 0;
    r.sp = 0;
    r.ix = 1.0f / r.d[0];
    r.iy = 1.0f / r.d[1];
    r.iz = 1.0f / r.d[2];
    r.sg = (r.ix < 0.0f ? 1u : 0u) | (r.iy < 0.0f ? 2u : 0u) | (r.iz < 0.0f ? 4u : 0u);
    // scene-AABB slab test, CUDAKernels.cu:237-262 (tMin may be negative)
    float tMin = (((r.sg & 1) ? s.shi[0] : s.slo[0]) - r.o[0]) * r.ix;
    float tMax = (((r.sg & 1) ? s.slo[0] : s.shi[0]) - r.o[0]) * r.ix;
    const float tymin = (((r.sg & 2) ? s.shi[1] : s.slo[1]) - r.o[1]) * r.iy;
    const float tymax = (((r.sg & 2) ? s.slo[1] : s.shi[1]) - r.o[1]) * r.iy;
    if ((tMin > tymax) || (tymin > tMax)) return false;
    if (tymin > tMin) tMin = tymin;
    if (tymax < tMax) tMax = tymax;
    const float tzmin = (((r.sg & 4) ? s.shi[2] : s.slo[2]) - r.o[2]) * r.iz;
    const float tzmax = (((r.sg & 4) ? s.slo[2] : s.shi[2]) - r.o[2]) * r.iz;
    if ((tMin > tzmax) || (tzmin > tMax)) return false;
    if (tzmin > tMin) tMin = tzmin;
    if (tzmax < tMax) tMax = tzmax;
    if (r.t_lo > 0.0f && tMin < r.t_lo) tMin = r.t_lo;   // the walk starts at t_lo (oracle)
    if (s.U < 2) {   // single leaf (reference: UB; defined as the oracle's)
        (void)tleaf<ANY>(s, r, 0, s.U ? s.N : 0u);
        return false;
    }
    r.tMin = tMin;
    r.tMax = tMax;
    r.nd = s.nodes[0];
    return true;
}

// One iteration of traverse_closest's loop; true when the walk has ended.
// The next node's record is requested before the leaves this step visits are
// tested (they are still tested before the next node's decisions read the
// best hit: the same decisions, the same hit).
template <bool ANY, class Stack>
__device__ __forceinline__ bool tray_step(const TScene &s, TRay &r, const Stack &stk) {
    const float best = r.bi != kNoHit ? r.bt : __builtin_inff();
    if (r.tMin > best) {                          // entered beyond the best hit: skip
        if (r.sp == 0) return true;
        --r.sp;
        stk.pop(r.sp, r.cur, r.tMin, r.tMax);
        r.nd = s.nodes[r.cur];
        return false;
    }
    if (best < r.tMax) r.tMax = best;
    const uint4 nd = r.nd;
    const uint32_t ax = (nd.z >> 27) & 3u;
    const float org = pick3(ax, r.o[0], r.o[1], r.o[2]), inv = pick3(ax, r.ix, r.iy, r.iz);
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
    if (tleaf<ANY>(s, r, l0b, l0e)) return true;   // (ANY only) the first accepted triangle ends the walk
    if (tleaf<ANY>(s, r, l1b, l1e)) return true;
    return fin;
}

// The ray's result into its own slot: bih_hit {t, u, v, prim} as one 16-byte
// store (u, v: the accepted triangle's test once more -- the same inputs and
// expressions, the same bits), or the occlusion byte.
template <bool ANY>
__device__ __forceinline__ void tray_write(const TraceArgs &a, const TScene &s, const TRay &r) {
    if (ANY) {
        reinterpret_cast<uint8_t *>(a.out)[r.id] = r.bi != kNoHit ? 1 : 0;
        return;
    }
    float t = FLT_MAX, u = 0.0f, v = 0.0f;
    uint32_t prim = kNoHit;
    if (r.bi != kNoHit) {
        (void)mt_tuv(s.tris + 9ull * r.bi, r, t, u, v);
        prim = a.tri_idx[r.bi];
    }
    reinterpret_cast<uint4 *>(a.out)[r.id] = make_uint4(__float_as_uint(t), __float_as_uint(u), __float_as_uint(v), prim);
}

// LDS: stack slots per lane kept in LDS (the rest in this thread's HBM area).
template <int LDS, bool ANY>
__global__ void __launch_bounds__(kTT) k_trace(const TraceArgs a) {
    __shared__ uint32_t s_node[LDS * kTT];
    __shared__ float s_min[LDS * kTT];
    __shared__ float s_max[LDS * kTT];
    const uint32_t lane = threadIdx.x;
    TStack<LDS> stk;
    stk.sn = s_node + lane;
    stk.smin = s_min + lane;
    stk.smax = s_max + lane;
    stk.gthreads = (uint64_t)gridDim.x * kTT;
    stk.spill = a.spill + (uint64_t)blockIdx.x * kTT + lane;
    TScene sc;
    sc.nodes = a.nodes;
    sc.tris = a.tris;
    sc.dup = a.dup;
    for (int k = 0; k < 3; ++k) {
        sc.slo[k] = a.hdr->scene_lo[k];
        sc.shi[k] = a.hdr->scene_hi[k];
    }
    sc.U = a.hdr->n_unique;
    sc.N = a.hdr->n_tris;
    const uint32_t n = a.n;
    TRay r;
    bool has = false;          // this lane walks a ray
    bool more = true;          // (wave-uniform) the cursor may still be short of n
    for (;;) {
        const unsigned long long idle = __ballot(!has);
        if (more && (__popcll(idle) >= kTRefill || idle == ~0ull)) {
            const uint32_t k = (uint32_t)__popcll(idle);
            uint32_t first = 0;
            if (lane == 0) first = atomicAdd(a.cursor, k);
            first = __builtin_amdgcn_readfirstlane(first);
            // (n <= 2^30 and each wave overshoots it by one fetch at most: no wrap)
            if ((uint64_t)first + k >= n) more = false;
            if (!has) {
                const uint32_t rk = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32),
                                                             __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                const uint64_t i = (uint64_t)first + rk;
                if (i < n) {
                    const float4 q0 = a.rays[2 * i], q1 = a.rays[2 * i + 1];   // two 16-byte loads
                    r.o[0] = q0.x; r.o[1] = q0.y; r.o[2] = q0.z; r.t_lo = q0.w;
                    r.d[0] = q1.x; r.d[1] = q1.y; r.d[2] = q1.z;               // (q1.w: reserved, not read)
                    r.id = (uint32_t)i;
                    has = tray_start<ANY>(sc, r);
                    if (!has) tray_write<ANY>(a, sc, r);   // missed the box / one-leaf tree: final
                }
            }
        }
        if (!__ballot(has)) {
            if (!more) break;
            continue;
        }
        if (has) {
            bool fin = false;
            for (int k = 0; k < kTSteps && !fin; ++k) fin = tray_step<ANY>(sc, r, stk);
            if (fin) {
                tray_write<ANY>(a, sc, r);
                has = false;
            }
        }
    }
}

}  // namespace

uint32_t trace_grid_blocks(int device) {
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    return (uint32_t)(cus > 0 ? cus : 256) * kTBlocksPerCU;
}

// every lane of the full grid, every slot but the kTraceLdsTest kept on chip
size_t trace_spill_words(uint32_t blocks) {
    return (size_t)blocks * kTT * (kStackDepth - kTraceLdsTest) * 3;
}

int launch_trace(const DeviceTree &t, const void *d_rays, uint32_t n, bool occluded, void *d_out,
                 uint32_t lds_slots, uint32_t *cursor, uint32_t *spill, uint32_t max_blocks, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    if (n == 0) return 0;
    TraceArgs a;
    a.hdr = t.hdr;
    a.nodes = t.nodes;
    a.tris = t.tris_s;
    a.dup = t.dup_cnt;
    a.tri_idx = t.vals;
    a.rays = reinterpret_cast<const float4 *>(d_rays);
    a.out = d_out;
    a.n = n;
    a.cursor = cursor;
    a.spill = spill;
    hipError_t e = hipMemsetAsync(cursor, 0, sizeof(uint32_t), st);
    if (e != hipSuccess) return (int)e;
    const uint32_t need = (n + kTT - 1) / kTT;
    const dim3 grid(need < max_blocks ? need : max_blocks), block(kTT);
    const bool small = lds_slots == (uint32_t)kTraceLdsTest;
    if (small && occluded) hipLaunchKernelGGL((k_trace<kTraceLdsTest, true>), grid, block, 0, st, a);
    else if (small) hipLaunchKernelGGL((k_trace<kTraceLdsTest, false>), grid, block, 0, st, a);
    else if (occluded) hipLaunchKernelGGL((k_trace<kTraceLds, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_trace<kTraceLds, false>), grid, block, 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace bih
