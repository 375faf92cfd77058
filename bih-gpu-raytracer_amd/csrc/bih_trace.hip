// bih_trace.hip -- ray queries (bih_trace_device / bih_trace, include/bih.h):
// closest hit and occlusion for caller-supplied rays on gfx950.
//
// Semantics are config C4's closest hit, the oracle's
// traverse_closest: the walk of bih_closest.h, with each ray's own origin and
// t_lo.  The occlusion query is the same walk ended at the first accepted
// triangle (ANY), so its flag is exactly (closest prim != BIH_NO_HIT).
// The segment queries (BIH_QUERY_T_HI: the ray ends at its t_hi) are defined on
// the closest query's result: OCCLUDED_WITHIN is the same walk ended at the
// first accepted triangle below t_hi (kWalkWithin, a prefix of the closest
// walk), CLOSEST_WITHIN the closest kernel with the t < t_hi filter at its
// write.  The two older queries do not read that float.
//
// Caller rays are incoherent and their walks very unequal, so the kernel has
// k_wh_trace's shape (bih_whitted.hip): persistent one-wave blocks; a lane
// whose walk has ended takes the next ray index from a global cursor while its
// wave-mates keep walking (idle lanes are refilled with one atomic per wave);
// each result goes to its ray's own slot, in caller order.
#include <hip/hip_runtime.h>
#include <float.h>

#include "bih_closest.h"
#include "bih_internal.h"

namespace bih {
namespace {

using dev::ClosestRay;
using dev::ClosestScene;
using dev::kNoHit;

constexpr uint32_t kTT = dev::kLanes;    // threads per block: one wave
constexpr uint32_t kTBlocksPerCU = 32;   // persistent grid (as k_wh_trace)
constexpr int kTRefill = 16;             // idle lanes of a wave that trigger a refill (as k_wh_trace)
constexpr int kTSteps = 256;             // walk steps per lane between refill checks (as k_wh_trace)

struct TraceArgs {
    const TreeHeader *hdr;
    const uint4 *nodes;
    const float *tris;
    const uint32_t *dup;
    const uint32_t *tri_idx;    // sorted position -> file order (BIH_ARR_TRI_INDEX)
    const float4 *rays;         // bih_ray: {o, t_lo}, {d, t_hi}
    void *out;                  // bih_hit[n] or u8[n]
    uint32_t n;
    uint32_t *cursor;           // rays taken so far (zero at launch)
    uint32_t *spill;
};

// A caller's ray: what bih_ray gives and where its result goes, and its walk.
struct TRay {
    float o[3], t_lo;
    uint32_t id;
    ClosestRay w;
};

// The ray's result into its own slot: bih_hit {t, u, v, prim} as one 16-byte
// store (u, v: the accepted triangle's test once more -- the same inputs and
// expressions, the same bits), or the occlusion byte.
// T_HI: a segment query; the answer is the closest one's when its t < t_hi.
template <bool ANY, bool T_HI>
__device__ __forceinline__ void tray_write(const TraceArgs &a, const ClosestScene &s, const TRay &r) {
    const bool hit = T_HI ? dev::within_hit(r.w) : r.w.bi != kNoHit;
    if (ANY) {
        reinterpret_cast<uint8_t *>(a.out)[r.id] = hit ? 1 : 0;
        return;
    }
    float t = FLT_MAX, u = 0.0f, v = 0.0f;
    uint32_t prim = kNoHit;
    if (hit) {
        (void)dev::mt_tuv(s.tris + 9ull * r.w.bi, r.o, r.w.d, t, u, v);
        prim = a.tri_idx[r.w.bi];
    }
    reinterpret_cast<uint4 *>(a.out)[r.id] = make_uint4(__float_as_uint(t), __float_as_uint(u), __float_as_uint(v), prim);
}

// The kernels' body.  LDS: stack slots per lane kept in LDS (the rest in this
// thread's HBM area; s_node, s_min, s_max: LDS * kTT words each).  T_HI: the
// rays' last float is read.
template <int LDS, bool ANY, bool T_HI>
__device__ __forceinline__ void trace_body(const TraceArgs &a, uint32_t *s_node, float *s_min, float *s_max) {
    // (CLOSEST_WITHIN walks the whole closest walk: its record needs the closest hit)
    constexpr int MODE = !ANY ? dev::kWalkClosest : (T_HI ? dev::kWalkWithin : dev::kWalkAny);
    const uint32_t lane = threadIdx.x;
    const dev::LaneStack<LDS> stk(s_node, s_min, s_max, a.spill);
    const ClosestScene sc = dev::load_closest_scene(a.hdr, a.nodes, a.tris, a.dup);
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
                    r.w.d[0] = q1.x; r.w.d[1] = q1.y; r.w.d[2] = q1.z;
                    if (T_HI) r.w.t_hi = q1.w;                                 // (else q1.w: reserved, not read)
                    r.id = (uint32_t)i;
                    has = dev::closest_start<MODE>(sc, r.w, r.o, r.t_lo);
                    if (!has) tray_write<ANY, T_HI>(a, sc, r);   // missed the box / one-leaf tree: final
                }
            }
        }
        if (!__ballot(has)) {
            if (!more) break;
            continue;
        }
        if (has) {
            bool fin = false;
            for (int k = 0; k < kTSteps && !fin; ++k) fin = dev::closest_step<MODE>(sc, r.w, r.o, r.t_lo, stk);
            if (fin) {
                tray_write<ANY, T_HI>(a, sc, r);
                has = false;
            }
        }
    }
}

template <int LDS, bool ANY>
__global__ void __launch_bounds__(kTT) k_trace(const TraceArgs a) {
    __shared__ uint32_t s_node[LDS * kTT];
    __shared__ float s_min[LDS * kTT];
    __shared__ float s_max[LDS * kTT];
    trace_body<LDS, ANY, false>(a, s_node, s_min, s_max);
}

// The segment queries (BIH_QUERY_T_HI).
template <int LDS, bool ANY>
__global__ void __launch_bounds__(kTT) k_trace_within(const TraceArgs a) {
    __shared__ uint32_t s_node[LDS * kTT];
    __shared__ float s_min[LDS * kTT];
    __shared__ float s_max[LDS * kTT];
    trace_body<LDS, ANY, true>(a, s_node, s_min, s_max);
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

int launch_trace(const DeviceTree &t, const void *d_rays, uint32_t n, uint32_t query, void *d_out,
                 const WorkArea &wa, void *stream) {
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
    a.cursor = wa.word(kCurTaken);
    a.spill = wa.spill;
    hipError_t e = hipMemsetAsync(a.cursor, 0, sizeof(uint32_t), st);
    if (e != hipSuccess) return (int)e;
    const uint32_t need = (n + kTT - 1) / kTT;
    const dim3 grid(need < wa.max_blocks ? need : wa.max_blocks), block(kTT);
    const bool small = wa.lds_slots == (uint32_t)kTraceLdsTest;
    const bool occluded = (query & ~kQueryTHi) == 1u;   // BIH_QUERY_OCCLUDED
    if (query & kQueryTHi) {
        if (small && occluded) hipLaunchKernelGGL((k_trace_within<kTraceLdsTest, true>), grid, block, 0, st, a);
        else if (small) hipLaunchKernelGGL((k_trace_within<kTraceLdsTest, false>), grid, block, 0, st, a);
        else if (occluded) hipLaunchKernelGGL((k_trace_within<kTraceLds, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_trace_within<kTraceLds, false>), grid, block, 0, st, a);
    } else if (small && occluded) hipLaunchKernelGGL((k_trace<kTraceLdsTest, true>), grid, block, 0, st, a);
    else if (small) hipLaunchKernelGGL((k_trace<kTraceLdsTest, false>), grid, block, 0, st, a);
    else if (occluded) hipLaunchKernelGGL((k_trace<kTraceLds, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_trace<kTraceLds, false>), grid, block, 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace bih
