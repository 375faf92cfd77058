// bih_direct.hip -- direct-lighting render (bih_render_direct_device /
// bih_render_direct, include/bih.h): per primary sample the set of directional
// lights that reach its hit point, and the pixel's irradiance and grey shade
// summed from them, on gfx950.
//
// Semantics, no new rule: the G-buffer's closest hit
// of the sample (section 4.5.2), then for every light that faces the hit
// triangle bih_trace's OCCLUDED query (section 4.5.1) of the ray {o = P, t_lo
// = BIH_SHADOW_T_LO, d = light direction}, then sums in a stated order.  Every
// f32 expression is separately rounded (-ffp-contract=off).
//
// Three kernels behind the G-buffer launch, which leaves every sample's hit
// record -- prim = the triangle's sorted position -- in the call's scratch:
//   k_direct_setup    per sample: the primary direction once more (bih_primary.h),
//                     P = o + t*d, the triangle's normal, the 64-bit mask of
//                     facing lights; hit samples with a facing light are
//                     appended to a list (wave ballot, prefix count, one atomic
//                     per wave), their record's {t, u, v} becomes P; lit = 0.
//   k_shadow          the hot path, k_trace's shape (bih_trace.hip): persistent
//                     one-wave blocks; work item = (listed sample, light k),
//                     taken from a global cursor; a lane whose walk has ended
//                     takes the next item while its wave-mates keep walking.
//                     No ray is written to or read from memory: the origin
//                     comes from the sample's record, the direction from the
//                     kernel arguments.  The walk is
//                     bih_closest.h's ANY walk; an unoccluded item sets its bit
//                     of the sample's lit word with one 64-bit atomic OR (the
//                     order of the ORs does not matter: deterministic).
//   k_direct_resolve  per pixel: the sums, in the header's order.
// The lights travel in the kernel arguments (the call's copy of the caller's
// host array): no device buffer of them exists.
//
// Point lights (bih_render_lights*, n_dir < n_lights) share the 64 light slots
// and take instantiations of their own of the three kernels (k_lights_setup,
// k_shadow_lights, k_lights_resolve); calls without one launch the kernels
// above, unchanged.  A lamp's L = Q - P is one expression (lamp_dir) on the
// same bits of P in all three; its shadow ray is a segment query (t_hi = 1:
// a triangle at or beyond the lamp does not shadow), the walk bih_closest.h's
// kWalkWithin, a directional item riding along with t_hi = +inf.
//
// Area lights (bih_render_area_lights*, n_area > 0) take the last slots and a
// third instantiation (k_area_setup, k_shadow_area, k_area_resolve) with an
// argument block of their own (AArgs: DArgs plus the panels); calls without
// one launch the kernels above with DArgs, unchanged.  An area light is a lamp
// whose position Q differs per sample: Q is bih_area.h's hash of (seed, global
// pixel, frame*spp + s, light), recomputed from the item's sample index in all
// three kernels (area_dir), so a lane's walk state stays SRay's {o, d, i, k}.
//
// Multi-bounce paths (bih_render_path*) run the stages once per level,
// list-driven past the primary level, with the walk k_path_bounce between the
// levels: see PArgs below.  One-bounce indirect lighting (bih_render_indirect*)
// is that pipeline with one level past the primary one.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stddef.h>
#include <type_traits>

#include "bih_area.h"
#include "bih_bounce.h"
#include "bih_closest.h"
#include "bih_internal.h"
#include "bih_primary.h"

namespace bih {
namespace {

using dev::ClosestRay;
using dev::ClosestScene;
using dev::kNoHit;

constexpr uint32_t kDT = dev::kLanes;    // k_shadow: threads per block, one wave
constexpr uint32_t kDSetupT = 256;       // k_direct_setup, k_direct_resolve: threads per block
constexpr int kDRefill = 16;             // idle lanes of a wave that trigger a refill (as k_trace)
constexpr int kDSteps = 256;             // walk steps per lane between refill checks (as k_trace)
constexpr float kShadowTLo = 1e-4f;      // BIH_SHADOW_T_LO
constexpr uint32_t kMissShade = 0x00281414u;   // (20, 20, 40): Whitted's miss shade

struct DLight { float x, y, z, w; };     // bih_light {dir, weight} or bih_point_light {pos, weight}

// A point light's L at the hit point P: one expression for the facing mask
// (setup), the shadow ray's direction (k_shadow) and the contribution
// (resolve), each from the same bits of P (a listed sample's record).
__device__ __forceinline__ void lamp_dir(const DLight &q, const float *p, float *l) {
    l[0] = q.x - p[0];
    l[1] = q.y - p[1];
    l[2] = q.z - p[2];
}

struct DArgs {
    float cam[12];              // origin, lower_left, horizontal, vertical
    uint32_t w, h, spp;
    uint32_t row0, nrows, band_h, band_step;
    uint32_t d_base;            // XORWOW Weyl counter at the start of the frame
    uint32_t n_lights;
    uint32_t n_dir;             // lights [0, n_dir) are directional, [n_dir, n_lights) point lights
    const TreeHeader *hdr;
    const uint4 *nodes;
    const float *tris;          // sorted {v0, e1, e2}
    const uint32_t *dup;
    const uint32_t *rng_in;     // 5 planes of nrows*w: XORWOW v at the start of the frame
    uint4 *rec;                 // [P*spp]: the G-buffer's {t, u, v, sorted position}; listed samples: {P, sorted position}
    uint32_t *list;             // [P*spp]: listed samples
    unsigned long long *face;   // [P*spp]: a listed sample's facing lights
    unsigned long long *lit;    // [P*spp]
    float *irradiance;          // [P] or null
    uint32_t *rgba;             // [P] or null
    uint32_t *count;            // listed samples (zero at launch)
    unsigned long long *cursor; // items taken so far (zero at launch)
    uint32_t *spill;
    DLight lights[kMaxLights];
};

// The kernels' instantiations: what kinds of light the call has.
constexpr int kDir = 0;     // directional only (bih_render_direct's kernels)
constexpr int kPoint = 1;   // point lights too (a.n_dir < a.n_lights)
constexpr int kArea = 2;    // area lights too (ax.n_area > 0)

struct APanel { float u[3], v[3], nl[3]; };   // edges; nl = cross(u, v) in the header's order (host, f32)

// The area kernels' argument block.  Slots [d.n_lights - n_area, d.n_lights)
// of d.lights are area lights {corner, weight}, the point lights end before.
struct AArgs {
    DArgs d;
    uint32_t n_area;
    uint32_t hseed;             // area_seed_hash(seed)
    uint32_t fs0;               // frame * spp (wrapping)
    APanel panel[kMaxAreaLights];
};

// Sample i of the call's rows: its global pixel y*w + x (y the global row) and s.
__device__ __forceinline__ uint32_t sample_pixel(const DArgs &a, uint32_t i, uint32_t *s) {
    const uint32_t lp = i / a.spp;
    *s = i - lp * a.spp;
    const uint32_t lr = lp / a.w, x = lp - lr * a.w;
    return dev::global_row(lr, a.row0, a.band_h, a.band_step) * a.w + x;
}

// Area light j's L = Q - P for sample s of global pixel gp: as lamp_dir, one
// expression for all three kernels (q: the light's slot, {corner, weight}).
__device__ __forceinline__ void area_dir(const AArgs &ax, uint32_t j, const DLight &q, uint32_t gp, uint32_t s,
                                         const float *p, float *l) {
    const float c[3] = {q.x, q.y, q.z};
    float pt[3];
    area_point(ax.hseed, gp, ax.fs0 + s, j, c, ax.panel[j].u, ax.panel[j].v, pt);
    l[0] = pt[0] - p[0];
    l[1] = pt[1] - p[1];
    l[2] = pt[2] - p[2];
}

// The 64-bit mask of the lights that face a point pt with normal nrm, the
// point of sample s of global pixel gp (the area lights' Q).  KIND (compile
// time): kDir, kPoint or kArea; ax: the area lights (kArea only).
template <int KIND>
__device__ __forceinline__ unsigned long long facing_mask(const DArgs &a, const AArgs *ax, const float *nrm,
                                                          const float *pt, uint32_t gp, uint32_t s) {
    unsigned long long face = 0ull;
    const uint32_t n_dir = KIND != kDir ? a.n_dir : a.n_lights;
    for (uint32_t k = 0; k < n_dir; ++k) {   // (k is uniform: the lights come as scalars)
        const float c = (nrm[0] * a.lights[k].x + nrm[1] * a.lights[k].y) + nrm[2] * a.lights[k].z;
        if (c > 0.0f) face |= 1ull << k;
    }
    if (KIND != kDir) {
        const uint32_t n_lamp = KIND == kArea ? a.n_lights - ax->n_area : a.n_lights;
        for (uint32_t k = n_dir; k < n_lamp; ++k) {
            float l[3];
            lamp_dir(a.lights[k], pt, l);
            const float c = (nrm[0] * l[0] + nrm[1] * l[1]) + nrm[2] * l[2];
            if (c > 0.0f) face |= 1ull << k;
        }
    }
    if (KIND == kArea) {
        const uint32_t k0 = a.n_lights - ax->n_area;
        for (uint32_t j = 0; j < ax->n_area; ++j) {
            float l[3];
            area_dir(*ax, j, a.lights[k0 + j], gp, s, pt, l);
            const float *nl = ax->panel[j].nl;
            const float c = (nrm[0] * l[0] + nrm[1] * l[1]) + nrm[2] * l[2];
            const float g = -((nl[0] * l[0] + nl[1] * l[1]) + nl[2] * l[2]);
            if (c > 0.0f && g > 0.0f) face |= 1ull << (k0 + j);   // it faces the panel's emitting side
        }
    }
    return face;
}

// KIND (compile time): kDir, kPoint or kArea; ax: the area lights (kArea only).
template <int KIND>
__device__ __forceinline__ void direct_setup_body(const DArgs &a, const AArgs *ax) {
    const uint64_t P = (uint64_t)a.nrows * a.w;
    const uint64_t n = P * a.spp;
    const uint64_t i = (uint64_t)blockIdx.x * kDSetupT + threadIdx.x;
    unsigned long long face = 0ull;
    float pt[3] = {0.0f, 0.0f, 0.0f};
    uint32_t bi = kNoHit;
    if (i < n) {
        const uint4 h = a.rec[i];
        bi = h.w;
        if (bi != kNoHit) {
            const uint64_t lp = i / a.spp;
            const uint32_t s = (uint32_t)(i - lp * a.spp);
            const uint32_t lr = (uint32_t)(lp / a.w), x = (uint32_t)(lp - (uint64_t)lr * a.w);
            const uint32_t y = dev::global_row(lr, a.row0, a.band_h, a.band_step);
            float d[3], nrm[3];
            dev::primary_dir(a.cam, a.rng_in, P, lp, a.d_base, s, x, y, a.w, a.h, d);
            const float t = __uint_as_float(h.x);
            for (int k = 0; k < 3; ++k) pt[k] = a.cam[k] + t * d[k];
            dev::tri_normal(a.tris + 9ull * bi, nrm);
            face = facing_mask<KIND>(a, ax, nrm, pt, y * a.w + x, s);
        }
        a.lit[i] = 0ull;
    }
    // the wave's listed samples take consecutive list slots: one atomic per wave
    const bool listed = face != 0ull;
    const unsigned long long m = __ballot(listed);
    if (!m) return;
    const uint32_t rk = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    uint32_t first = 0;
    if ((threadIdx.x & (dev::kLanes - 1u)) == 0) first = atomicAdd(a.count, (uint32_t)__popcll(m));
    first = __builtin_amdgcn_readfirstlane(first);
    if (listed) {
        const uint32_t j = first + rk;
        a.rec[i] = make_uint4(__float_as_uint(pt[0]), __float_as_uint(pt[1]), __float_as_uint(pt[2]), bi);
        a.list[j] = (uint32_t)i;
        a.face[j] = face;
    }
}

__global__ void __launch_bounds__(kDSetupT) k_direct_setup(const DArgs a) { direct_setup_body<kDir>(a, nullptr); }
__global__ void __launch_bounds__(kDSetupT) k_lights_setup(const DArgs a) { direct_setup_body<kPoint>(a, nullptr); }
__global__ void __launch_bounds__(kDSetupT) k_area_setup(const AArgs a) { direct_setup_body<kArea>(a.d, &a); }

// A work item: where its ray starts, whose bit it decides, and its walk.
struct SRay {
    float o[3];
    uint32_t i, k;              // sample, light
    ClosestRay w;
};

// SEG: the item's ray is a segment (within_hit: hit below its t_hi).
template <bool SEG>
__device__ __forceinline__ void sray_write(const DArgs &a, const SRay &r) {
    const bool occluded = SEG ? dev::within_hit(r.w) : r.w.bi != kNoHit;
    if (!occluded) atomicOr(a.lit + r.i, 1ull << r.k);
}

// The shadow kernels' body.  LDS: stack slots per lane kept in LDS (the rest
// in this thread's HBM area; s_node, s_min, s_max: LDS * kDT words each).
// KIND (compile time) kPoint or kArea: the call has point or area lights.  An
// item then carries its own t_hi -- 1.0f for a lamp or an area light's point
// (it sits at t = 1 of d = Q - P), +inf for a directional light -- and the
// walk is kWalkWithin, which with t_hi = +inf is exactly the ANY walk (every
// accepted t is below FLT_MAX).  An area item's Q is recomputed here from its
// sample index: past the fetch it is a lamp item.
template <int LDS, int KIND>
__device__ __forceinline__ void shadow_body(const DArgs &a, const AArgs *ax, uint32_t *s_node, float *s_min,
                                            float *s_max) {
    constexpr bool POINT = KIND != kDir;
    constexpr int MODE = POINT ? dev::kWalkWithin : dev::kWalkAny;
    const uint32_t lane = threadIdx.x;
    const dev::LaneStack<LDS> stk(s_node, s_min, s_max, a.spill);
    const ClosestScene sc = dev::load_closest_scene(a.hdr, a.nodes, a.tris, a.dup);
    const uint32_t K = a.n_lights;
    const uint64_t n = (uint64_t)*a.count * K;    // items: (listed sample, light)
    SRay r;
    bool has = false;          // this lane walks a ray
    bool more = true;          // (wave-uniform) the cursor may still be short of n
    for (;;) {
        // (fetched again while enough lanes stay idle: a non-facing item leaves its lane idle)
        unsigned long long idle = __ballot(!has);
        while (more && (__popcll(idle) >= kDRefill || idle == ~0ull)) {
            const uint32_t cnt = (uint32_t)__popcll(idle);
            unsigned long long first = 0;
            if (lane == 0) first = atomicAdd(a.cursor, (unsigned long long)cnt);
            first = ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(first >> 32)) << 32) |
                    __builtin_amdgcn_readfirstlane((uint32_t)first);
            // (a 64-bit cursor: n < 2^38, and the grid's overshoot is far below 2^63)
            if (first + cnt >= n) more = false;
            if (!has && first < n) {
                const uint32_t rk = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32),
                                                             __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                // item = first + rk = (j0 * K + k0) + rk: one wide division per fetch (uniform)
                const uint64_t j0 = first / K;
                const uint32_t kk = (uint32_t)(first - j0 * K) + rk;
                const uint64_t j = j0 + kk / K;
                const uint32_t k = kk % K;
                if (first + rk < n && ((a.face[j] >> k) & 1ull)) {   // a non-facing item ends at once
                    r.i = a.list[j];
                    r.k = k;
                    const uint4 q = a.rec[r.i];
                    r.o[0] = __uint_as_float(q.x); r.o[1] = __uint_as_float(q.y); r.o[2] = __uint_as_float(q.z);
                    // (from the kernel arguments, one 16-byte load per item: a copy in LDS
                    // costs the walk three waves per CU, 175 against 164 ms)
                    const DLight l = a.lights[k];
                    r.w.d[0] = l.x; r.w.d[1] = l.y; r.w.d[2] = l.z;
                    if (POINT) {
                        r.w.t_hi = __builtin_inff();
                        if (k >= a.n_dir) {
                            if (KIND == kArea && k >= a.n_lights - ax->n_area) {
                                uint32_t s;
                                const uint32_t gp = sample_pixel(a, r.i, &s);
                                area_dir(*ax, k - (a.n_lights - ax->n_area), l, gp, s, r.o, r.w.d);
                            } else {
                                lamp_dir(l, r.o, r.w.d);
                            }
                            r.w.t_hi = 1.0f;
                        }
                    }
                    has = dev::closest_start<MODE>(sc, r.w, r.o, kShadowTLo);
                    if (!has) sray_write<POINT>(a, r);   // missed the box / one-leaf tree: final
                }
            }
            idle = __ballot(!has);
        }
        if (!__ballot(has)) {
            if (!more) break;
            continue;
        }
        if (has) {
            bool fin = false;
            for (int k = 0; k < kDSteps && !fin; ++k) fin = dev::closest_step<MODE>(sc, r.w, r.o, kShadowTLo, stk);
            if (fin) {
                sray_write<POINT>(a, r);
                has = false;
            }
        }
    }
}

template <int LDS>
__global__ void __launch_bounds__(kDT) k_shadow(const DArgs a) {
    __shared__ uint32_t s_node[LDS * kDT];
    __shared__ float s_min[LDS * kDT];
    __shared__ float s_max[LDS * kDT];
    shadow_body<LDS, kDir>(a, nullptr, s_node, s_min, s_max);
}

// bih_render_lights* with point lights: the same LDS per block.
template <int LDS>
__global__ void __launch_bounds__(kDT) k_shadow_lights(const DArgs a) {
    __shared__ uint32_t s_node[LDS * kDT];
    __shared__ float s_min[LDS * kDT];
    __shared__ float s_max[LDS * kDT];
    shadow_body<LDS, kPoint>(a, nullptr, s_node, s_min, s_max);
}

// bih_render_area_lights* with area lights: the same LDS per block.
template <int LDS>
__global__ void __launch_bounds__(kDT) k_shadow_area(const AArgs a) {
    __shared__ uint32_t s_node[LDS * kDT];
    __shared__ float s_min[LDS * kDT];
    __shared__ float s_max[LDS * kDT];
    shadow_body<LDS, kArea>(a.d, &a, s_node, s_min, s_max);
}

// A sample's sum over its lit lights l, k ascending, in the header's order:
// bi its triangle, *recp its record ({P, bi} when l != 0), (gp, s) its global
// pixel and sample (the area lights' Q).
template <int KIND>
__device__ __forceinline__ float sample_sum(const DArgs &a, const AArgs *ax, const DLight *s_light, const uint4 *recp,
                                            uint32_t bi, unsigned long long l, uint32_t gp, uint32_t s) {
    constexpr bool POINT = KIND != kDir;
    float e = 0.0f;
    if (l) {
        float nrm[3];
        dev::tri_normal(a.tris + 9ull * bi, nrm);
        while (l) {   // k ascending over the lit bits
            const uint32_t k = (uint32_t)__builtin_ctzll(l);
            const DLight q = s_light[k];
            l &= l - 1ull;
            if (POINT && k >= a.n_dir) {
                const uint4 rec = *recp;   // (a lit sample is a listed one: rec.xyz = P)
                const float pt[3] = {__uint_as_float(rec.x), __uint_as_float(rec.y), __uint_as_float(rec.z)};
                float L[3];
                const bool area = KIND == kArea && k >= a.n_lights - ax->n_area;
                if (area) area_dir(*ax, k - (a.n_lights - ax->n_area), q, gp, s, pt, L);
                else lamp_dir(q, pt, L);
                const float c = (nrm[0] * L[0] + nrm[1] * L[1]) + nrm[2] * L[2];
                const float r2 = (L[0] * L[0] + L[1] * L[1]) + L[2] * L[2];
                const float len = sqrtf(r2);
                if (area) {   // the emitter's own cosine times its area: g = -(nl . L)
                    const float *nl = ax->panel[k - (a.n_lights - ax->n_area)].nl;
                    const float g = -((nl[0] * L[0] + nl[1] * L[1]) + nl[2] * L[2]);
                    e = e + ((q.w * (c / len)) * (g / len)) / r2;
                } else {
                    e = e + (q.w * (c / len)) / r2;
                }
            } else {
                const float c = (nrm[0] * q.x + nrm[1] * q.y) + nrm[2] * q.z;
                e = e + q.w * c;
            }
        }
    }
    return e;
}

template <int KIND>
__device__ __forceinline__ void direct_resolve_body(const DArgs &a, const AArgs *ax, DLight *s_light) {
    if (threadIdx.x < a.n_lights) s_light[threadIdx.x] = a.lights[threadIdx.x];
    __syncthreads();
    const uint64_t P = (uint64_t)a.nrows * a.w;
    const uint64_t lp = (uint64_t)blockIdx.x * kDSetupT + threadIdx.x;
    if (lp >= P) return;
    float E = 0.0f;
    bool any = false;
    uint32_t gp = 0;   // (kArea) the global pixel
    if (KIND == kArea) {
        const uint32_t lr = (uint32_t)(lp / a.w), px = (uint32_t)(lp - (uint64_t)lr * a.w);
        gp = dev::global_row(lr, a.row0, a.band_h, a.band_step) * a.w + px;
    }
    for (uint32_t s = 0; s < a.spp; ++s) {
        const uint64_t i = lp * a.spp + s;
        const uint32_t bi = a.rec[i].w;
        any = any || bi != kNoHit;
        const float e = sample_sum<KIND>(a, ax, s_light, a.rec + i, bi, a.lit[i], gp, s);
        E = s == 0 ? e : E + e;
    }
    E = E / (float)a.spp;
    if (a.irradiance) a.irradiance[lp] = E;
    if (a.rgba) {
        const uint32_t g = (uint32_t)(int)fmaxf(0.0f, fminf(255.0f, 255.0f * E));
        a.rgba[lp] = any ? (g | (g << 8) | (g << 16)) : kMissShade;
    }
}

__global__ void __launch_bounds__(kDSetupT) k_direct_resolve(const DArgs a) {
    __shared__ DLight s_light[kMaxLights];
    direct_resolve_body<kDir>(a, nullptr, s_light);
}

__global__ void __launch_bounds__(kDSetupT) k_lights_resolve(const DArgs a) {
    __shared__ DLight s_light[kMaxLights];
    direct_resolve_body<kPoint>(a, nullptr, s_light);
}

__global__ void __launch_bounds__(kDSetupT) k_area_resolve(const AArgs a) {
    __shared__ DLight s_light[kMaxLights];
    direct_resolve_body<kArea>(a.d, &a, s_light);
}

// ---- Multi-bounce paths (bih_render_path*; with one level,
// bih_render_indirect*, 4.5.6) ----
// The stages above once per level, list-driven past the primary one.  Level 0
// is bih_render_area_lights' primary level for every light set (n_area, the
// lamps or all lights may be 0; k_path_setup0: every hit sample's record
// becomes {P, sorted position}, the hit samples are level 0's live list).
// Level k = 1..n_bounces: k_path_bounce walks one hashed, cosine-distributed
// ray (bih_bounce.h, slot kBounceSlot + k - 1) per sample of level k-1's live
// list to its closest hit, reads its record from one of two record buffers and
// leaves {P_k, sorted position} in the other, appends the samples it stopped to
// level k's live list and adds an escaped sample's thr_{k-1} * sky;
// k_path_setup lists the live samples a light faces for the shadow pass, which
// is the kernels above on the level's records and lit plane (a record keeps its
// sample's index, so sample_pixel still gives the primary's (gp, s) for an area
// light's Q); k_path_accum adds thr_k * e_k.  The sums go forward
// into one f32 per sample (acc), so k_path_resolve needs no level's data.
// thr_k is the same for every sample alive at level k: it travels as a scalar.
struct PArgs {
    AArgs a;                    // a.d.rec, a.d.lit: the level's records and lit plane (k_path_bounce: a.d.rec the level
                                // before's); a.d.list, face, count, cursor: the shadow list, as everywhere
    uint4 *rec_out;             // k_path_bounce: the level's records, the other buffer
    uint4 *bounce;              // [P*spp] the level's plane of the caller's bih_hit, prim in file order, or null
    const uint32_t *live;       // the live samples: of the level before (k_path_bounce), else of the level
    const uint32_t *n_live;
    uint32_t *live_out;         // k_path_bounce, k_path_setup0: the level's live samples
    uint32_t *n_live_out;       // (zero at launch)
    float *acc;                 // [P*spp] the sample's sum so far
    uint8_t *hit0;              // [P*spp] 1: the primary sample hit (the pixel's miss shade)
    const uint32_t *tri_idx;    // sorted position -> file order
    uint32_t slot;              // k_path_bounce: the hash slot of the level's direction
    float thr;                  // k_path_bounce: thr_{k-1}; k_path_accum: thr_k
    float sky;
};

constexpr uint32_t kPListBlocks = 2048;   // the list-driven kernels' grid cap (they stride)
constexpr uint32_t kMatMirror = 1u;       // BIH_MAT_MIRROR (bih_render_path_spec*, section 4.5.9)

// The wave's lanes with `on` take consecutive slots from *count: one atomic
// per wave (all lanes of the wave call it).
__device__ __forceinline__ uint32_t wave_append(bool on, uint32_t *count) {
    const unsigned long long m = __ballot(on);
    const uint32_t rk = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    uint32_t first = 0;
    if (m && (threadIdx.x & (dev::kLanes - 1u)) == 0) first = atomicAdd(count, (uint32_t)__popcll(m));
    return __builtin_amdgcn_readfirstlane(first) + rk;
}

// Level 0's setup over every sample of the call: the area setup's point, normal
// and facing mask for every light set; EVERY hit sample's record becomes {P,
// sorted position} and joins level 0's live list, the ones a light faces also
// the shadow list; lit = 0, the sample's sum starts and whether it hit is noted.
// Shared with the mirror paths (k_path_spec_setup0, section 4.5.9), which pass
// their argument block as `sa`: a mirror hit faces no light, and the sample's
// record of incoming direction and kind starts here.
template <class S>
__device__ __forceinline__ void path_setup0_body(const PArgs &pa, const S *sa) {
    const DArgs &a = pa.a.d;
    const uint64_t P = (uint64_t)a.nrows * a.w;
    const uint64_t n = P * a.spp;
    const uint64_t i = (uint64_t)blockIdx.x * kDSetupT + threadIdx.x;
    unsigned long long face = 0ull;
    uint32_t bi = kNoHit;
    if (i < n) {
        const uint4 h = a.rec[i];
        bi = h.w;
        if (bi != kNoHit) {
            const uint64_t lp = i / a.spp;
            const uint32_t s = (uint32_t)(i - lp * a.spp);
            const uint32_t lr = (uint32_t)(lp / a.w), x = (uint32_t)(lp - (uint64_t)lr * a.w);
            const uint32_t y = dev::global_row(lr, a.row0, a.band_h, a.band_step);
            float d[3], nrm[3], pt[3];
            dev::primary_dir(a.cam, a.rng_in, P, lp, a.d_base, s, x, y, a.w, a.h, d);
            const float t = __uint_as_float(h.x);
            for (int k = 0; k < 3; ++k) pt[k] = a.cam[k] + t * d[k];
            dev::tri_normal(a.tris + 9ull * bi, nrm);
            if constexpr (std::is_same<S, void>::value) {
                face = facing_mask<kArea>(a, &pa.a, nrm, pt, y * a.w + x, s);
            } else {
                const uint32_t kind = spec_kind(*sa, pa.tri_idx[bi]);
                if (kind != kMatMirror) face = facing_mask<kArea>(a, &pa.a, nrm, pt, y * a.w + x, s);
                sa->dk[i] = make_uint4(__float_as_uint(d[0]), __float_as_uint(d[1]), __float_as_uint(d[2]), kind);
            }
            a.rec[i] = make_uint4(__float_as_uint(pt[0]), __float_as_uint(pt[1]), __float_as_uint(pt[2]), bi);
        }
        a.lit[i] = 0ull;
        pa.acc[i] = 0.0f;
        pa.hit0[i] = bi != kNoHit ? 1 : 0;
    }
    const uint32_t jb = wave_append(bi != kNoHit, pa.n_live_out);
    if (bi != kNoHit) pa.live_out[jb] = (uint32_t)i;
    const uint32_t j = wave_append(face != 0ull, a.count);
    if (face != 0ull) {
        a.list[j] = (uint32_t)i;
        a.face[j] = face;
    }
}

__global__ void __launch_bounds__(kDSetupT) k_path_setup0(const PArgs pa) {
    path_setup0_body<void>(pa, nullptr);
}

// A bounce ray: where it starts, whose it is, and its walk.
struct BRay {
    float o[3];
    uint32_t i;                 // sample
    ClosestRay w;
};

// The end of a level's walk for the lane's sample: a stopped ray leaves {P_k,
// sorted position} in the level's record buffer and stays alive (returns true);
// an escaped one collects thr_{k-1} * sky and ends.  The caller's bih_hit is
// bih_trace's: u, v from the accepted triangle's test once more, prim in file
// order; the miss record for an escape.
__device__ __forceinline__ bool pray_write(const PArgs &pa, const ClosestScene &s, const BRay &r) {
    const bool stopped = r.w.bi != kNoHit;
    float t = FLT_MAX, u = 0.0f, v = 0.0f;
    uint32_t prim = kNoHit;
    if (stopped) {
        (void)dev::mt_tuv(s.tris + 9ull * r.w.bi, r.o, r.w.d, t, u, v);
        prim = pa.tri_idx[r.w.bi];
        pa.rec_out[r.i] = make_uint4(__float_as_uint(r.o[0] + t * r.w.d[0]), __float_as_uint(r.o[1] + t * r.w.d[1]),
                                     __float_as_uint(r.o[2] + t * r.w.d[2]), r.w.bi);
    } else {
        pa.acc[r.i] = pa.acc[r.i] + pa.thr * pa.sky;
    }
    if (pa.bounce) pa.bounce[r.i] = make_uint4(__float_as_uint(t), __float_as_uint(u), __float_as_uint(v), prim);
    return stopped;
}

// ---- Colour paths (bih_render_path_rgb*) ----
// The paths above with a material per triangle: the sample's sum and its
// throughput are RGB and per sample, one 16-byte record each ({R, G, B, -}: a
// lane moves its sample's three channels with one load or store), touched by
// list-driven kernels and the walk's writer only.  Levels, rays, lists, lit
// words and e_k are the grey call's: every kernel that steers a path runs
// unchanged.  A hit's material comes from its file-order triangle, which the
// generation's tri_idx gives from the sorted position: ids follow a rebuild.
struct CArgs {
    PArgs p;                    // (p.acc, p.thr, p.sky: unused)
    float4 *acc3;               // [P*spp] the sample's RGB sum so far
    float4 *thr3;               // [P*spp] the sample's RGB throughput
    const float4 *pal;          // two per material: {albedo, -}, {emission, -} (bih_material)
    const uint32_t *ids;        // file-order triangle -> material, or null: material 0
    float *radiance;            // [3P] or null
    float sky[3];
};

__device__ __forceinline__ const PArgs &path_args(const PArgs &pa) { return pa; }
__device__ __forceinline__ const PArgs &path_args(const CArgs &ca) { return ca.p; }

// pray_write for a colour path: a stopped ray collects thr_{k-1} * emission(m_k)
// and its throughput takes albedo(m_k); an escaped one collects thr_{k-1} * sky.
// dk (mirror paths, section 4.5.9; else null and SPEC false): the sample's
// record of the ray that found this hit and of the hit's kind, the material's
// fourth word, which came with its albedo.
template <bool SPEC>
__device__ __forceinline__ bool pray_write_rgb(const CArgs &ca, uint4 *dk, const ClosestScene &s, const BRay &r) {
    const PArgs &pa = ca.p;
    const bool stopped = r.w.bi != kNoHit;
    float t = FLT_MAX, u = 0.0f, v = 0.0f;
    uint32_t prim = kNoHit;
    float4 acc = ca.acc3[r.i];
    const float4 thr = ca.thr3[r.i];
    if (stopped) {
        (void)dev::mt_tuv(s.tris + 9ull * r.w.bi, r.o, r.w.d, t, u, v);
        prim = pa.tri_idx[r.w.bi];
        pa.rec_out[r.i] = make_uint4(__float_as_uint(r.o[0] + t * r.w.d[0]), __float_as_uint(r.o[1] + t * r.w.d[1]),
                                     __float_as_uint(r.o[2] + t * r.w.d[2]), r.w.bi);
        const uint32_t m = ca.ids ? ca.ids[prim] : 0u;
        const float4 al = ca.pal[2 * m], em = ca.pal[2 * m + 1];
        acc = make_float4(acc.x + thr.x * em.x, acc.y + thr.y * em.y, acc.z + thr.z * em.z, 0.0f);
        ca.thr3[r.i] = make_float4(thr.x * al.x, thr.y * al.y, thr.z * al.z, 0.0f);
        if constexpr (SPEC)
            dk[r.i] = make_uint4(__float_as_uint(r.w.d[0]), __float_as_uint(r.w.d[1]), __float_as_uint(r.w.d[2]),
                                 __float_as_uint(al.w));
    } else {
        acc = make_float4(acc.x + thr.x * ca.sky[0], acc.y + thr.y * ca.sky[1], acc.z + thr.z * ca.sky[2], 0.0f);
    }
    ca.acc3[r.i] = acc;
    if (pa.bounce) pa.bounce[r.i] = make_uint4(__float_as_uint(t), __float_as_uint(u), __float_as_uint(v), prim);
    return stopped;
}

__device__ __forceinline__ bool pray_write(const CArgs &ca, const ClosestScene &s, const BRay &r) {
    return pray_write_rgb<false>(ca, nullptr, s, r);
}

// ---- Mirror paths (bih_render_path_spec*) ----
// The colour paths with a material kind that steers: a sample whose latest hit
// is a mirror goes on along the reflection of the ray that found it, not along
// the hashed lobe, and no light is gathered there (the setups give it no list
// entry: its lit word stays 0 and k_path_rgb_accum adds thr * +0).  One 16-byte
// record per sample, {D, kind} of its latest hit, carries what that takes from
// the writer of one level (level 0: the setup) to the next level's ray
// generation and to the level's setup.  The sums are the colour kernels'.
struct SArgs {
    CArgs c;
    uint4 *dk;                  // [P*spp] {D_k.x, D_k.y, D_k.z, kind_k} of the sample's latest hit
};

__device__ __forceinline__ const PArgs &path_args(const SArgs &sa) { return sa.c.p; }

// kind(m) of the file-order triangle prim.
__device__ __forceinline__ uint32_t spec_kind(const SArgs &sa, uint32_t prim) {
    const uint32_t m = sa.c.ids ? sa.c.ids[prim] : 0u;
    return __float_as_uint(sa.c.pal[2 * m].w);
}

__device__ __forceinline__ bool pray_write(const SArgs &sa, const ClosestScene &s, const BRay &r) {
    return pray_write_rgb<true>(sa.c, sa.dk, s, r);
}

// The direction of the level's ray from the lane's sample i, whose latest hit
// has the normal nrm: the level's hashed lobe; behind a mirror hit (SArgs
// only) the reflection of the ray that found it.
template <class X>
__device__ __forceinline__ void path_ray_dir(const X &x, const PArgs &pa, uint32_t i, const float *nrm, float *d) {
    const DArgs &a = pa.a.d;
    if constexpr (std::is_same<X, SArgs>::value) {
        const uint4 q = x.dk[i];
        if (q.w == kMatMirror) {
            const float D[3] = {__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z)};
            const float dn = (D[0] * nrm[0] + D[1] * nrm[1]) + D[2] * nrm[2];
            const float k2 = 2.0f * dn;
            for (int c = 0; c < 3; ++c) d[c] = D[c] - k2 * nrm[c];
            return;
        }
    }
    uint32_t s;
    const uint32_t gp = sample_pixel(a, i, &s);
    bounce_dir(pa.a.hseed, gp, pa.a.fs0 + s, pa.slot, nrm, d);
}

// A level's bounce walk, k_trace's shape: persistent one-wave blocks; work
// item = a sample of the level before's live list, taken from the global
// cursor; a lane whose walk has ended takes the next item while its wave-mates
// keep walking.  No ray goes through memory: the origin is the sample's P, the
// direction path_ray_dir's.  The walk is bih_closest.h's closest walk.
// The lanes whose walks ended in one round write together, so
// that the stopped ones take consecutive slots of the level's live list with
// one atomic (wave_append needs the whole wave).
// The walk is shared with the colour paths (k_path_rgb_bounce, section 4.5.8)
// and the mirror paths (k_path_spec_bounce, section 4.5.9): X is PArgs, CArgs or
// SArgs, which differ in what the end of a walk writes, SArgs also in the
// direction a new ray takes (outside the walk loop).
template <int LDS, class X>
__device__ __forceinline__ void path_bounce_body(const X &x) {
    const PArgs &pa = path_args(x);
    __shared__ uint32_t s_node[LDS * kDT];
    __shared__ float s_min[LDS * kDT];
    __shared__ float s_max[LDS * kDT];
    const DArgs &a = pa.a.d;
    const uint32_t lane = threadIdx.x;
    const dev::LaneStack<LDS> stk(s_node, s_min, s_max, a.spill);
    const ClosestScene sc = dev::load_closest_scene(a.hdr, a.nodes, a.tris, a.dup);
    const uint64_t n = *pa.n_live;
    BRay r;
    bool has = false;          // this lane walks a ray
    bool more = true;          // (wave-uniform) the cursor may still be short of n
    for (;;) {
        bool fin = false;      // this lane's walk ended in this round
        const unsigned long long idle = __ballot(!has);
        if (more && (__popcll(idle) >= kDRefill || idle == ~0ull)) {
            const uint32_t cnt = (uint32_t)__popcll(idle);
            unsigned long long first = 0;
            if (lane == 0) first = atomicAdd(a.cursor, (unsigned long long)cnt);
            first = ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(first >> 32)) << 32) |
                    __builtin_amdgcn_readfirstlane((uint32_t)first);
            if (first + cnt >= n) more = false;
            if (!has) {
                const uint32_t rk = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32),
                                                             __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                if (first + rk < n) {
                    r.i = pa.live[first + rk];
                    const uint4 q = a.rec[r.i];   // {P, sorted position} of the level before
                    r.o[0] = __uint_as_float(q.x); r.o[1] = __uint_as_float(q.y); r.o[2] = __uint_as_float(q.z);
                    float nrm[3];
                    dev::tri_normal(a.tris + 9ull * q.w, nrm);
                    path_ray_dir(x, pa, r.i, nrm, r.w.d);
                    has = dev::closest_start<dev::kWalkClosest>(sc, r.w, r.o, kShadowTLo);
                    fin = !has;   // missed the box / one-leaf tree: final
                }
            }
        }
        if (has) {
            for (int k = 0; k < kDSteps && !fin; ++k)
                fin = dev::closest_step<dev::kWalkClosest>(sc, r.w, r.o, kShadowTLo, stk);
            if (fin) has = false;
        }
        if (__ballot(fin)) {
            const bool stopped = fin && pray_write(x, sc, r);
            const uint32_t j = wave_append(stopped, pa.n_live_out);
            if (stopped) pa.live_out[j] = r.i;
        }
        if (!__ballot(has) && !more) break;
    }
}

template <int LDS>
__global__ void __launch_bounds__(kDT) k_path_bounce(const PArgs pa) {
    path_bounce_body<LDS>(pa);
}

template <int LDS>
__global__ void __launch_bounds__(kDT) k_path_rgb_bounce(const CArgs ca) {
    path_bounce_body<LDS>(ca);
}

template <int LDS>
__global__ void __launch_bounds__(kDT) k_path_spec_bounce(const SArgs sa) {
    path_bounce_body<LDS>(sa);
}

// Level 0's setup of a mirror path: k_path_setup0's, see there.
__global__ void __launch_bounds__(kDSetupT) k_path_spec_setup0(const SArgs sa) {
    path_setup0_body(sa.c.p, &sa);
}

// A level's setup over its live samples: the facing mask at {P_k, n_k}; the
// samples a light faces go to the shadow list; the level's lit word starts at 0.
// dk (mirror paths, k_path_spec_setup; else null and SPEC false): a mirror hit
// faces no light.
template <bool SPEC>
__device__ __forceinline__ void path_setup_body(const PArgs &pa, const uint4 *dk) {
    const DArgs &a = pa.a.d;
    const uint32_t n = *pa.n_live;
    // (the trip count is the block's: wave_append needs the whole wave)
    for (uint32_t base = blockIdx.x * kDSetupT; base < n; base += gridDim.x * kDSetupT) {
        const uint32_t j0 = base + threadIdx.x;
        unsigned long long face = 0ull;
        uint32_t i = 0;
        if (j0 < n) {
            i = pa.live[j0];
            bool lights = a.n_lights != 0;
            if constexpr (SPEC) lights = lights && dk[i].w != kMatMirror;
            if (lights) {
                const uint4 h = a.rec[i];
                const float pt[3] = {__uint_as_float(h.x), __uint_as_float(h.y), __uint_as_float(h.z)};
                float nrm[3];
                dev::tri_normal(a.tris + 9ull * h.w, nrm);
                uint32_t s;
                const uint32_t gp = sample_pixel(a, i, &s);
                face = facing_mask<kArea>(a, &pa.a, nrm, pt, gp, s);
            }
            a.lit[i] = 0ull;
        }
        const uint32_t j = wave_append(face != 0ull, a.count);
        if (face != 0ull) {
            a.list[j] = i;
            a.face[j] = face;
        }
    }
}

__global__ void __launch_bounds__(kDSetupT) k_path_setup(const PArgs pa) {
    path_setup_body<false>(pa, nullptr);
}

__global__ void __launch_bounds__(kDSetupT) k_path_spec_setup(const SArgs sa) {
    path_setup_body<true>(sa.c.p, sa.dk);
}

// A level's sum over its live samples, behind its shadow pass: acc += thr_k * e_k.
__global__ void __launch_bounds__(kDSetupT) k_path_accum(const PArgs pa) {
    __shared__ DLight s_light[kMaxLights];
    const DArgs &a = pa.a.d;
    if (threadIdx.x < a.n_lights) s_light[threadIdx.x] = a.lights[threadIdx.x];
    __syncthreads();
    const uint32_t n = *pa.n_live;
    for (uint32_t j = blockIdx.x * kDSetupT + threadIdx.x; j < n; j += gridDim.x * kDSetupT) {
        const uint32_t i = pa.live[j];
        uint32_t s;
        const uint32_t gp = sample_pixel(a, i, &s);
        const float e = sample_sum<kArea>(a, &pa.a, s_light, a.rec + i, a.rec[i].w, a.lit[i], gp, s);
        pa.acc[i] = pa.acc[i] + pa.thr * e;
    }
}

// Per pixel: E over the samples' sums in the header's order, and the shade.
__global__ void __launch_bounds__(kDSetupT) k_path_resolve(const PArgs pa) {
    const DArgs &a = pa.a.d;
    const uint64_t P = (uint64_t)a.nrows * a.w;
    const uint64_t lp = (uint64_t)blockIdx.x * kDSetupT + threadIdx.x;
    if (lp >= P) return;
    float E = 0.0f;
    bool any = false;
    for (uint32_t s = 0; s < a.spp; ++s) {
        const uint64_t i = lp * a.spp + s;
        any = any || pa.hit0[i] != 0;
        const float e = pa.acc[i];
        E = s == 0 ? e : E + e;
    }
    E = E / (float)a.spp;
    if (a.irradiance) a.irradiance[lp] = E;
    if (a.rgba) {
        const uint32_t g = (uint32_t)(int)fmaxf(0.0f, fminf(255.0f, 255.0f * E));
        a.rgba[lp] = any ? (g | (g << 8) | (g << 16)) : kMissShade;
    }
}

// The caller's level planes before any level writes them: the miss record and
// lit word 0, which an ended path's elements keep.
__global__ void __launch_bounds__(kDSetupT) k_path_fill(uint4 *bounces, unsigned long long *lits, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kDSetupT + threadIdx.x;
    if (i >= n) return;
    if (bounces) bounces[i] = make_uint4(__float_as_uint(FLT_MAX), 0u, 0u, kNoHit);
    if (lits) lits[i] = 0ull;
}

// Level 0 of a colour path over its live samples, behind k_path_setup0 (whose
// records hold the sorted position): acc = emission(m_0), thr_0 = albedo(m_0).
// A missed primary sample has no record here: k_path_rgb_resolve takes it as 0.
__global__ void __launch_bounds__(kDSetupT) k_path_rgb_setup0(const CArgs ca) {
    const PArgs &pa = ca.p;
    const uint32_t n = *pa.n_live;
    for (uint32_t j = blockIdx.x * kDSetupT + threadIdx.x; j < n; j += gridDim.x * kDSetupT) {
        const uint32_t i = pa.live[j];
        const uint32_t m = ca.ids ? ca.ids[pa.tri_idx[pa.a.d.rec[i].w]] : 0u;
        ca.thr3[i] = ca.pal[2 * m];
        ca.acc3[i] = ca.pal[2 * m + 1];
    }
}

// k_path_accum per channel: acc[c] += thr_k[c] * e_k.
__global__ void __launch_bounds__(kDSetupT) k_path_rgb_accum(const CArgs ca) {
    __shared__ DLight s_light[kMaxLights];
    const PArgs &pa = ca.p;
    const DArgs &a = pa.a.d;
    if (threadIdx.x < a.n_lights) s_light[threadIdx.x] = a.lights[threadIdx.x];
    __syncthreads();
    const uint32_t n = *pa.n_live;
    for (uint32_t j = blockIdx.x * kDSetupT + threadIdx.x; j < n; j += gridDim.x * kDSetupT) {
        const uint32_t i = pa.live[j];
        uint32_t s;
        const uint32_t gp = sample_pixel(a, i, &s);
        const float e = sample_sum<kArea>(a, &pa.a, s_light, a.rec + i, a.rec[i].w, a.lit[i], gp, s);
        const float4 acc = ca.acc3[i], thr = ca.thr3[i];
        ca.acc3[i] = make_float4(acc.x + thr.x * e, acc.y + thr.y * e, acc.z + thr.z * e, 0.0f);
    }
}

// Per pixel: E[c] over the samples' sums in the header's order, and the shade.
__global__ void __launch_bounds__(kDSetupT) k_path_rgb_resolve(const CArgs ca) {
    const PArgs &pa = ca.p;
    const DArgs &a = pa.a.d;
    const uint64_t P = (uint64_t)a.nrows * a.w;
    const uint64_t lp = (uint64_t)blockIdx.x * kDSetupT + threadIdx.x;
    if (lp >= P) return;
    float E[3] = {0.0f, 0.0f, 0.0f};
    bool any = false;
    for (uint32_t s = 0; s < a.spp; ++s) {
        const uint64_t i = lp * a.spp + s;
        const bool hit = pa.hit0[i] != 0;
        any = any || hit;
        const float4 q = hit ? ca.acc3[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const float e[3] = {q.x, q.y, q.z};
        for (int c = 0; c < 3; ++c) E[c] = s == 0 ? e[c] : E[c] + e[c];
    }
    uint32_t px = 0;
    for (int c = 0; c < 3; ++c) {
        E[c] = E[c] / (float)a.spp;
        if (ca.radiance) ca.radiance[3 * lp + c] = E[c];
        px |= (uint32_t)(int)fmaxf(0.0f, fminf(255.0f, 255.0f * E[c])) << (8 * c);
    }
    if (a.rgba) a.rgba[lp] = any ? px : kMissShade;
}

// The argument block of a call: the frame, the tree, the lights in slot order
// with the area lights' panels, the primary level's planes and scratch, and the
// work area's words.  (Without an area light the direct kernels take aa.d alone.)
static void fill_args(AArgs &aa, const DeviceTree &t, const RenderArgs &ra, const Lights &l, const DirectPlanes &p,
                      const Scratch &s, const WorkArea &wa) {
    DArgs &a = aa.d;
    for (int k = 0; k < 12; ++k) a.cam[k] = ra.cam[k];
    a.w = ra.w;
    a.h = ra.h;
    a.spp = ra.spp;
    a.row0 = ra.row0;
    a.nrows = ra.nrows;
    a.band_h = ra.band_h;
    a.band_step = ra.band_step;
    a.d_base = ra.d_base;
    a.n_lights = l.n_lights;
    a.n_dir = l.n_dir;
    a.hdr = t.hdr;
    a.nodes = t.nodes;
    a.tris = t.tris_s;
    a.dup = t.dup_cnt;
    a.rng_in = ra.rng_in;
    a.rec = reinterpret_cast<uint4 *>(s.rec);
    a.list = s.list;
    a.face = s.face;
    a.lit = p.lit;
    a.irradiance = p.irradiance;
    a.rgba = p.rgba;
    a.count = wa.word(kCurListed);
    a.cursor = wa.items();
    a.spill = wa.spill;
    for (uint32_t k = 0; k < kMaxLights; ++k) {
        const bool on = k < l.n_lights;
        a.lights[k] = DLight{on ? l.slots[4 * k] : 0.0f, on ? l.slots[4 * k + 1] : 0.0f, on ? l.slots[4 * k + 2] : 0.0f,
                             on ? l.slots[4 * k + 3] : 0.0f};
    }
    const uint32_t n_area = l.area.n;
    aa.n_area = n_area;
    aa.hseed = l.area.hseed;
    aa.fs0 = l.area.fs0;
    if (n_area) {
        for (uint32_t j = 0; j < kMaxAreaLights; ++j)
            for (int c = 0; c < 3; ++c) {
                aa.panel[j].u[c] = j < n_area ? l.area.uvn[j][c] : 0.0f;
                aa.panel[j].v[c] = j < n_area ? l.area.uvn[j][3 + c] : 0.0f;
                aa.panel[j].nl[c] = j < n_area ? l.area.uvn[j][6 + c] : 0.0f;
            }
    }
}

// The launch's listed-sample count and item cursor start from zero.
static hipError_t reset_counts(const DArgs &a, hipStream_t st) {
    const hipError_t e = hipMemsetAsync(a.count, 0, sizeof(uint32_t), st);
    return e == hipSuccess ? hipMemsetAsync(a.cursor, 0, sizeof(unsigned long long), st) : e;
}

// The shadow pass over the samples listed in aa.d: the kernel of the call's
// kinds of light (n_area, then point: n_dir < n_lights, else bih_render_direct's).
static hipError_t launch_shadow(const AArgs &aa, uint32_t n_area, uint64_t n, uint32_t lds_slots, uint32_t max_blocks,
                                hipStream_t st) {
    const DArgs &a = aa.d;
    const bool point = a.n_dir < a.n_lights;
    // (the listed samples are counted on the device: the grid covers all of them)
    const uint64_t need = (n * a.n_lights + kDT - 1) / kDT;
    const dim3 grid((uint32_t)(need < max_blocks ? need : max_blocks)), block(kDT);
    const bool small = lds_slots == (uint32_t)kTraceLdsTest;
    if (n_area && small) hipLaunchKernelGGL((k_shadow_area<kTraceLdsTest>), grid, block, 0, st, aa);
    else if (n_area) hipLaunchKernelGGL((k_shadow_area<kTraceLds>), grid, block, 0, st, aa);
    else if (point && small) hipLaunchKernelGGL((k_shadow_lights<kTraceLdsTest>), grid, block, 0, st, a);
    else if (point) hipLaunchKernelGGL((k_shadow_lights<kTraceLds>), grid, block, 0, st, a);
    else if (small) hipLaunchKernelGGL((k_shadow<kTraceLdsTest>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_shadow<kTraceLds>), grid, block, 0, st, a);
    return hipGetLastError();
}

}  // namespace

int launch_direct(const DeviceTree &t, const RenderArgs &ra, const DirectPlanes &p, const Lights &l, const Scratch &s,
                  const WorkArea &wa, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    const uint32_t n_area = l.area.n;
    if (ra.nrows == 0 || ra.w == 0 || ra.spp == 0 || l.n_lights == 0) return 0;
    if (l.n_lights > kMaxLights || l.n_dir > l.n_lights) return (int)hipErrorInvalidValue;
    if (n_area > kMaxAreaLights || n_area > l.n_lights - l.n_dir) return (int)hipErrorInvalidValue;
    static_assert(offsetof(DArgs, n_dir) + 4 == offsetof(DArgs, hdr) && offsetof(DArgs, n_dir) % 8 == 4,
                  "n_dir sits in what was padding before the pointers: the argument block has not grown");
    const bool point = l.n_dir < l.n_lights;   // else: bih_render_direct's kernels
    AArgs aa;
    const DArgs &a = aa.d;
    fill_args(aa, t, ra, l, p, s, wa);
    hipError_t e = reset_counts(a, st);
    if (e != hipSuccess) return (int)e;
    const uint64_t P = (uint64_t)ra.nrows * ra.w, n = P * ra.spp;
    const dim3 sgrid((uint32_t)((n + kDSetupT - 1) / kDSetupT));
    if (n_area) hipLaunchKernelGGL(k_area_setup, sgrid, dim3(kDSetupT), 0, st, aa);
    else if (point) hipLaunchKernelGGL(k_lights_setup, sgrid, dim3(kDSetupT), 0, st, a);
    else hipLaunchKernelGGL(k_direct_setup, sgrid, dim3(kDSetupT), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    e = launch_shadow(aa, n_area, n, wa.lds_slots, wa.max_blocks, st);
    if (e != hipSuccess) return (int)e;
    if (p.irradiance || p.rgba) {
        const dim3 rgrid((uint32_t)((P + kDSetupT - 1) / kDSetupT));
        if (n_area) hipLaunchKernelGGL(k_area_resolve, rgrid, dim3(kDSetupT), 0, st, aa);
        else if (point) hipLaunchKernelGGL(k_lights_resolve, rgrid, dim3(kDSetupT), 0, st, a);
        else hipLaunchKernelGGL(k_direct_resolve, rgrid, dim3(kDSetupT), 0, st, a);
        e = hipGetLastError();
    }
    return (int)e;
}

// The call's passes, each behind the one before on the stream: the fill of the
// caller's level planes, level 0's setup, shadow pass and sum, then per level
// the bounce walk, the setup, the shadow pass and the sum, and the resolve.
// Nothing comes back to the host between them: every grid is sized for the
// call's samples and the kernels read the lists' counts on the device.
//
// Two record buffers and two live lists suffice.  Level k's records go to
// buffer k & 1 and its live list to list k & 1; its bounce walk reads level
// k-1's (the other ones).  Level k's bounce, setup, shadow pass and sum have all
// ended, in stream order, before level k+1's bounce overwrites level k-1's
// records and list, which nothing reads after level k's bounce.  The shadow
// list (list, face, count, cursor) is free again after each level's shadow pass.
//
// c (a colour call, else null): the walk's and the sum's colour kernels take the
// places of the grey ones, k_path_rgb_setup0 follows level 0's setup, and the
// resolve is the colour one; every other launch is the grey call's.
// c->dk (a mirror call, else null): the mirror paths' setups and walk take the
// places of the grey setups and the colour walk; every other launch is the
// colour call's.
int launch_path(const DeviceTree &t, const RenderArgs &ra, const PathPlanes &p, const Lights &l, float albedo, float sky,
                uint32_t n_bounces, const Scratch &s, const WorkArea &wa, void *stream, const PathRgb *c) {
    const hipStream_t st = (hipStream_t)stream;
    if (c && (!c->palette || !c->acc3 || !c->thr3)) return (int)hipErrorInvalidValue;
    if (ra.nrows == 0 || ra.w == 0 || ra.spp == 0) return 0;
    if (l.n_lights > kMaxLights || l.n_dir > l.n_lights) return (int)hipErrorInvalidValue;
    if (l.area.n > kMaxAreaLights || l.area.n > l.n_lights - l.n_dir) return (int)hipErrorInvalidValue;
    if (n_bounces == 0 || n_bounces > kMaxBounces) return (int)hipErrorInvalidValue;
    static_assert(sizeof(SArgs) <= 4096, "kernel arguments");
    SArgs sa;
    CArgs &ca = sa.c;
    PArgs &pa = ca.p;
    sa.dk = c ? reinterpret_cast<uint4 *>(c->dk) : nullptr;
    const bool spec = sa.dk != nullptr;
    fill_args(pa.a, t, ra, l, p, s, wa);
    ca.acc3 = c ? reinterpret_cast<float4 *>(c->acc3) : nullptr;
    ca.thr3 = c ? reinterpret_cast<float4 *>(c->thr3) : nullptr;
    ca.pal = c ? reinterpret_cast<const float4 *>(c->palette) : nullptr;
    ca.ids = c ? c->ids : nullptr;
    ca.radiance = c ? c->radiance : nullptr;
    for (int k = 0; k < 3; ++k) ca.sky[k] = c ? c->sky[k] : 0.0f;
    uint4 *const recs[2] = {reinterpret_cast<uint4 *>(s.rec), reinterpret_cast<uint4 *>(s.rec2)};
    uint32_t *const lists[2] = {s.blist, s.blist2};
    uint32_t *const counts[2] = {wa.word(kCurBounce), wa.word(kCurBounce2)};
    pa.rec_out = nullptr;
    pa.bounce = nullptr;
    pa.live = nullptr;
    pa.n_live = nullptr;
    pa.live_out = lists[0];
    pa.n_live_out = counts[0];
    pa.acc = s.acc;
    pa.hit0 = s.hit0;
    pa.tri_idx = t.vals;
    pa.slot = kBounceSlot;
    pa.thr = 1.0f;
    pa.sky = sky;
    const uint64_t P = (uint64_t)ra.nrows * ra.w, n = P * ra.spp;
    const dim3 sgrid((uint32_t)((n + kDSetupT - 1) / kDSetupT));
    const dim3 lgrid(sgrid.x < kPListBlocks ? sgrid.x : kPListBlocks);
    hipError_t e = hipSuccess;
    if (p.bounces || p.lits) {
        const uint64_t m = n * n_bounces;
        hipLaunchKernelGGL(k_path_fill, dim3((uint32_t)((m + kDSetupT - 1) / kDSetupT)), dim3(kDSetupT), 0, st,
                           reinterpret_cast<uint4 *>(p.bounces), p.lits, m);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = reset_counts(pa.a.d, st);
    if (e == hipSuccess) e = hipMemsetAsync(counts[0], 0, sizeof(uint32_t), st);
    if (e != hipSuccess) return (int)e;
    if (spec) hipLaunchKernelGGL(k_path_spec_setup0, sgrid, dim3(kDSetupT), 0, st, sa);
    else hipLaunchKernelGGL(k_path_setup0, sgrid, dim3(kDSetupT), 0, st, pa);
    e = hipGetLastError();
    if (c && e == hipSuccess) {
        pa.live = lists[0];
        pa.n_live = counts[0];
        hipLaunchKernelGGL(k_path_rgb_setup0, lgrid, dim3(kDSetupT), 0, st, ca);
        e = hipGetLastError();
    }
    float thr = 1.0f;   // thr_k (the grey call's)
    for (uint32_t k = 0;; ++k) {
        // level k's shadow pass and sum over its live samples (pa.a.d.rec, lit: the level's)
        pa.live = lists[k & 1];
        pa.n_live = counts[k & 1];
        pa.thr = thr;
        if (e == hipSuccess && l.n_lights) e = launch_shadow(pa.a, l.area.n, n, wa.lds_slots, wa.max_blocks, st);
        if (e != hipSuccess) return (int)e;
        if (c) hipLaunchKernelGGL(k_path_rgb_accum, lgrid, dim3(kDSetupT), 0, st, ca);
        else hipLaunchKernelGGL(k_path_accum, lgrid, dim3(kDSetupT), 0, st, pa);
        e = hipGetLastError();
        if (k == n_bounces) break;
        // level k+1: the walk from level k's records into the other buffer, then its setup
        pa.rec_out = recs[(k + 1) & 1];
        pa.live_out = lists[(k + 1) & 1];
        pa.n_live_out = counts[(k + 1) & 1];
        pa.bounce = p.bounces ? reinterpret_cast<uint4 *>(p.bounces) + (uint64_t)k * n : nullptr;
        pa.slot = kBounceSlot + k;
        if (e == hipSuccess) e = reset_counts(pa.a.d, st);
        if (e == hipSuccess) e = hipMemsetAsync(pa.n_live_out, 0, sizeof(uint32_t), st);
        if (e != hipSuccess) return (int)e;
        {
            const uint64_t need = (n + kDT - 1) / kDT;
            const dim3 grid((uint32_t)(need < wa.max_blocks ? need : wa.max_blocks)), block(kDT);
            const bool small = wa.lds_slots == (uint32_t)kTraceLdsTest;
            if (spec && small) hipLaunchKernelGGL((k_path_spec_bounce<kTraceLdsTest>), grid, block, 0, st, sa);
            else if (spec) hipLaunchKernelGGL((k_path_spec_bounce<kTraceLds>), grid, block, 0, st, sa);
            else if (c && small) hipLaunchKernelGGL((k_path_rgb_bounce<kTraceLdsTest>), grid, block, 0, st, ca);
            else if (c) hipLaunchKernelGGL((k_path_rgb_bounce<kTraceLds>), grid, block, 0, st, ca);
            else if (small) hipLaunchKernelGGL((k_path_bounce<kTraceLdsTest>), grid, block, 0, st, pa);
            else hipLaunchKernelGGL((k_path_bounce<kTraceLds>), grid, block, 0, st, pa);
            e = hipGetLastError();
        }
        thr = thr * albedo;
        pa.a.d.rec = pa.rec_out;
        pa.a.d.lit = p.lits ? p.lits + (uint64_t)k * n : p.lit_scratch;
        pa.live = pa.live_out;
        pa.n_live = pa.n_live_out;
        if (e == hipSuccess) e = hipMemsetAsync(pa.a.d.cursor, 0, sizeof(unsigned long long), st);
        if (e != hipSuccess) return (int)e;
        if (spec) hipLaunchKernelGGL(k_path_spec_setup, lgrid, dim3(kDSetupT), 0, st, sa);
        else hipLaunchKernelGGL(k_path_setup, lgrid, dim3(kDSetupT), 0, st, pa);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return (int)e;
    if (c ? (c->radiance || p.rgba) : (p.irradiance || p.rgba)) {
        const dim3 rgrid((uint32_t)((P + kDSetupT - 1) / kDSetupT));
        if (c) hipLaunchKernelGGL(k_path_rgb_resolve, rgrid, dim3(kDSetupT), 0, st, ca);
        else hipLaunchKernelGGL(k_path_resolve, rgrid, dim3(kDSetupT), 0, st, pa);
        e = hipGetLastError();
    }
    return (int)e;
}

}  // namespace bih
