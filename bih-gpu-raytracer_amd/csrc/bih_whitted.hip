// bih_whitted.hip -- config C4 (BASELINE.json configs[3]): 8-bounce Whitted
// mirror rays at 3840x2160 on gfx950, as a wavefront of compacted ray queues.
//
// The reference has primary rays only (cudaRender, CUDAKernels.cu:391-423;
// Color :370-389 is binary).  C4's semantics are the build's own, defined in
// the test oracle (ob_render_whitted) and DESIGN.md section 4.5:
//   closest hit = bih_closest.h's walk (the oracle's traverse_closest) with
//   t_lo = 0 for primary rays, 1e-4 after;
//   P = O + t*D, n = cross(e1, e2), k = (2*dot(D, n)) / dot(n, n), R = D - k*n;
//   shade(d) = miss ? (20,20,40) : d == 8 ? (255,255,0) : 0.5*Y + 0.5*shade(d+1).
// The (t, i) rule is order-independent, so any walk order over the same visit
// set gives the oracle's hit; every f32 expression is the oracle's, in its
// order (-ffp-contract=off): bit-exact RGBA.
//
// Kernels (one frame, all on the caller's stream, no host round trip):
//   k_wh_gen    one thread per sample: the XORWOW jitter (cudaRender's draws)
//               and camera direction into ray queue 0; zeroes the counters.
//   k_wh_trace  bounce d (9 launches): persistent waves drain queue d%2
//               (length counts[d]); each lane walks its ray's BIH visit set
//               for the closest hit and takes the next ray when its walk
//               ends (every tree, a one-leaf one included); hits reflect and
//               are appended to queue (d+1)%2 with one ballot + mbcnt per wave
//               and one atomic per wave (wavefront compaction: the next
//               bounce's waves are full).
//   k_wh_shade  one thread per pixel: the samples' shades -> rgbToInt.
#include <hip/hip_runtime.h>
#include <float.h>

#include "bih_closest.h"
#include "bih_internal.h"

namespace bih {
namespace {

using dev::camera_dir;
using dev::ClosestRay;
using dev::ClosestScene;
using dev::global_row;
using dev::kNoHit;
using dev::rgb_to_int;
using dev::xorwow_uniform;

constexpr uint32_t kWT = dev::kLanes;   // threads per block: one wave
constexpr int kWStack = kStackDepth;    // Karras path length <= 30 (bih_internal.h)
// stack slots per lane in LDS; deeper ones in HBM
// (A/B r04r/s, ms per C4 frame: 6 958, 8 725, 10 683, 12 752, 16 877)
constexpr int kWLds = 10;
constexpr uint32_t kWBlocksPerCU = 32;  // persistent grid of k_wh_trace
constexpr float kBounceTLo = 1e-4f;     // t_lo of secondary rays (oracle: 1e-4f)
constexpr uint32_t kWCounts = 32;       // counter words: [0..9] rays per queue, [16..25] rays taken (k_wh_trace)
constexpr uint32_t kWFetch = 16;
// the bounce queues' sort key (wh_sort_key): origin cells per axis 2^bits (3:
// LDS-aggregated counts; more: global atomics; A/B r04zo per 4K frame: 3
// 0.636 s, 4 0.644, 5 0.620, 6 0.623) x 8 direction octants (3 bits: 4096)
constexpr uint32_t kWSortBits = 5;
constexpr uint32_t kWSortBuckets = 8u << (3 * kWSortBits);
constexpr uint32_t kWWorkWords = 18;    // work counters: {nodes, triangles} per bounce, u64 (k_wh_trace<true>)

__device__ __forceinline__ ClosestScene load_wscene(const RenderArgs &a) {
    return dev::load_closest_scene(a.hdr, a.nodes, a.tris, a.dup_cnt);
}

// Ray queue: 7 planes of `cap` words {ox, oy, oz, dx, dy, dz, sample}.
struct WQueue {
    float *p;
    uint64_t cap;
    __device__ __forceinline__ void put(uint64_t i, const float o[3], const float d[3], uint32_t sid) const {
        for (int k = 0; k < 3; ++k) {
            p[k * cap + i] = o[k];
            p[(3 + k) * cap + i] = d[k];
        }
        reinterpret_cast<uint32_t *>(p)[6 * cap + i] = sid;
    }
};

// counts[0..9]: rays in queue d (d = bounce depth).  With hit_mask (the
// primary samples' any-hit result from the frustum bins, one u64 per tile of
// TW x TH pixels, lane = pixel * spp + sample): only the samples that hit are
// queued for bounce 0, compacted per wave (ballot + mbcnt, one atomic on
// counts[0], zeroed before the launch); a sample the bins prove to miss has no
// closest hit either (the same visit set and test), so its depth stays 0.
__global__ void __launch_bounds__(kWT) k_wh_gen(const RenderArgs a, WQueue q, uint32_t *counts,
                                                uint8_t *hits, uint32_t *sort_hist,
                                                const unsigned long long *hit_mask, uint32_t tiles_x,
                                                uint32_t log2spp) {
    const uint64_t P = (uint64_t)a.nrows * a.w;
    const uint64_t rays = P * a.spp;
    const uint64_t gid = (uint64_t)blockIdx.x * kWT + threadIdx.x;
    // k_wh_sort_*'s histogram (zeroed again by each scan), whatever the grid
    for (uint64_t k = gid; k < kWSortBuckets; k += (uint64_t)gridDim.x * kWT) sort_hist[k] = 0u;
    if (gid == 0 && !hit_mask) {
        counts[0] = (uint32_t)rays;
        for (uint32_t k = 1; k < kWCounts; ++k) counts[k] = 0u;
    }
    const bool in = gid < rays;
    const uint64_t lp = in ? gid / a.spp : 0;
    const uint32_t s = (uint32_t)(gid % a.spp);
    const uint32_t lr = (uint32_t)(lp / a.w), x = (uint32_t)(lp % a.w);
    bool hit = in;
    if (hit_mask && in) {
        // TileShape: TW x TH pixels, TW * TH = 64 >> log2(spp)
        const uint32_t lpx = 6 - log2spp, tw = 1u << ((lpx + 1) / 2), th = 1u << (lpx / 2);
        const uint32_t tile = (lr / th) * tiles_x + x / tw;
        const uint32_t bit = (((lr % th) * tw + (x % tw)) << log2spp) + s;
        hit = (hit_mask[tile] >> bit) & 1ull;
    }
    uint64_t slot = gid;
    if (hit_mask) {
        const unsigned long long b = __ballot(hit);
        uint32_t base = 0;
        if (threadIdx.x == 0 && b) base = atomicAdd(counts, (uint32_t)__popcll(b));
        base = __builtin_amdgcn_readfirstlane(base);
        slot = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    }
    if (in) hits[gid] = 0;
    if (!hit) return;
    // draws 2s, 2s+1 of this pixel's frame (cudaRender :413-415)
    uint32_t v[5];
    for (int i = 0; i < 5; ++i) v[i] = a.rng_in[(uint64_t)i * P + lp];
    uint32_t d = a.d_base;
    float ru = 0.f, rv = 0.f;
    for (uint32_t k = 0; k <= s; ++k) {
        ru = xorwow_uniform(v, d);
        rv = xorwow_uniform(v, d);
    }
    const uint32_t y = global_row(lr, a.row0, a.band_h, a.band_step);
    float dir[3];
    camera_dir(a, ((float)x + ru) / (float)a.w, ((float)y + rv) / (float)a.h, dir[0], dir[1], dir[2]);
    q.put(slot, a.cam, dir, (uint32_t)gid);
}

// k_wh_trace: per-lane ray fetching.  A lane whose walk has ended takes the
// next ray of the queue while the other lanes of its wave keep walking, so a
// wave does not wait for its slowest ray before taking 64 new ones (secondary
// rays trapped in the soup walk very unequal visit sets).  Each lane's walk is
// bih_closest.h's, one step per inner iteration.  Idle lanes are refilled with
// one atomic per wave when a quarter of the wave is idle (or all of it).
constexpr int kWRefill = 16;   // idle lanes of a wave that trigger a refill
// walk steps per lane between refill checks (A/B r03: 1 1.792 s, 2 1.777, 4 1.755 per 4K frame;
// r04y-zg after the one-round-trip step: 2 0.698, 4 0.680, 8 0.669, 16 0.660, 32 0.653,
// 64 0.645, 128 0.639, 256 0.635, 512 0.636, 1024 0.647: a refill stalls the whole wave
// on the new rays' loads, so fewer, larger refills pay until idle lanes wait too long)
constexpr int kWSteps = 256;
// A queued ray: its origin and sample, and its walk (t_lo is the launch's).
struct WRay {
    float o[3];
    uint32_t sid;
    ClosestRay w;
};
// COUNT: nodes entered and triangles tested, summed into the work counters.
template <bool COUNT>
__global__ void __launch_bounds__(kWT) k_wh_trace(const RenderArgs a, uint32_t depth, WQueue qin, WQueue qout,
                                                  uint32_t *counts, uint8_t *hits, uint32_t *spill,
                                                  unsigned long long *work) {
    uint32_t cn = 0, ct = 0;   // COUNT: nodes entered, triangles tested by this lane
#if BIH_WH_MAXDIAG
    uint32_t cn_ray0 = 0, cmax = 0;   // (diagnostic build: the longest walk, in nodes, reported as 'tris')
#endif
    __shared__ uint32_t s_node[kWLds * kWT];
    __shared__ float s_min[kWLds * kWT];
    __shared__ float s_max[kWLds * kWT];
    const uint32_t lane = threadIdx.x;
    const dev::LaneStack<kWLds> stk(s_node, s_min, s_max, spill);
    const ClosestScene sc = load_wscene(a);
    const uint32_t n = counts[depth];
    uint32_t *fetch = counts + kWFetch + depth;   // rays of queue `depth` taken so far
    const float t_lo = depth ? kBounceTLo : 0.0f;
    const uint32_t *sid_in = reinterpret_cast<const uint32_t *>(qin.p) + 6 * qin.cap;
    WRay r;
    bool has = false;          // this lane walks a ray
    bool more = true;          // (wave-uniform) the queue may still hold rays
    for (;;) {
        bool fin = false;      // this lane's ray ended in this iteration
        const unsigned long long idle = __ballot(!has);
        if (more && (__popcll(idle) >= kWRefill || idle == ~0ull)) {
            const uint32_t k = (uint32_t)__popcll(idle);
            uint32_t first = 0;
            if (lane == 0) first = atomicAdd(fetch, k);
            first = __builtin_amdgcn_readfirstlane(first);
            if ((uint64_t)first + k >= n) more = false;   // u64: no wrap of first + k
            if (!has) {
                const uint32_t rk = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32),
                                                             __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                const uint64_t i = (uint64_t)first + rk;
                if (i < n) {
                    for (int c = 0; c < 3; ++c) {
                        r.o[c] = qin.p[c * qin.cap + i];
                        r.w.d[c] = qin.p[(3 + c) * qin.cap + i];
                    }
                    r.sid = sid_in[i];
                    // a ray that misses the scene box, or any ray of a one-leaf tree (which
                    // may hit: its leaf is not counted as work), ends here
                    has = dev::closest_start<false>(sc, r.w, r.o, t_lo);
                    fin = !has;
#if BIH_WH_MAXDIAG
                    cn_ray0 = cn;
#endif
                }
            }
        }
        if (!__ballot(has || fin)) {
            if (!more) break;
            continue;
        }
        if (has)
            for (int k = 0; k < kWSteps && !fin; ++k)
                fin = dev::closest_step<false, COUNT>(sc, r.w, r.o, t_lo, stk, cn, ct);
#if BIH_WH_MAXDIAG
        if (fin && cn - cn_ray0 > cmax) cmax = cn - cn_ray0;
#endif
        const bool hit = fin && r.w.bi != kNoHit;
        if (hit) hits[r.sid] = (uint8_t)(depth + 1);
        // the mirror ray (oracle whitted_path), then compaction into qout
        const bool next = hit && depth < 8u;
        float po[3], rd[3];
        if (next) {
            const float *v = sc.tris + 9ull * r.w.bi;
            const float e1x = v[3], e1y = v[4], e1z = v[5], e2x = v[6], e2y = v[7], e2z = v[8];
            const float nx = e1y * e2z - e2y * e1z;        // n = cross(e1, e2), glm order
            const float ny = e1z * e2x - e2z * e1x;
            const float nz = e1x * e2y - e2x * e1y;
            const float *d = r.w.d;
            const float dn = (d[0] * nx + d[1] * ny) + d[2] * nz;
            const float nn = (nx * nx + ny * ny) + nz * nz;
            const float kk = (2.0f * dn) / nn;
            const float nv[3] = {nx, ny, nz};
            for (int k = 0; k < 3; ++k) {
                const float td = r.w.bt * d[k];
                po[k] = r.o[k] + td;
                const float kn = kk * nv[k];
                rd[k] = d[k] - kn;
            }
        }
        const unsigned long long m = __ballot(next);
        if (m) {
            uint32_t first = 0;
            if (lane == 0) first = atomicAdd(counts + depth + 1, (uint32_t)__popcll(m));
            first = __builtin_amdgcn_readfirstlane(first);
            if (next) {
                const uint32_t rk = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                             __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                qout.put((uint64_t)first + rk, po, rd, r.sid);
            }
        }
        if (fin) has = false;
    }
    if (COUNT) {   // work[2 depth] += nodes, work[2 depth + 1] += triangles (per wave, u64)
        unsigned long long n64 = cn, t64 = ct;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            n64 += __shfl_xor(n64, off, 64);
            t64 += __shfl_xor(t64, off, 64);
        }
#if BIH_WH_MAXDIAG
        unsigned long long m64 = cmax;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(m64, off, 64);
            m64 = o > m64 ? o : m64;
        }
        if (lane == 0) {
            atomicAdd(work + 2 * depth, n64);
            atomicMax(work + 2 * depth + 1, m64);
        }
#else
        if (lane == 0) {
            atomicAdd(work + 2 * depth, n64);
            atomicAdd(work + 2 * depth + 1, t64);
        }
#endif
    }
}

// Ray order of a bounce queue (round 4).  The rays of queue d+1 arrive in the
// order their waves finished, so neighbouring lanes start unrelated walks.
// Before bounce d+1 the queue is reordered by a key of origin cell (3 bits of
// the scene box per axis, Morton-interleaved) x direction octant: lanes and
// waves of one XCD then walk neighbouring subtrees, and the node / triangle
// lines they share stay in that XCD's L2.  A counting sort (k_wh_sort_count,
// k_wh_sort_scan, k_wh_sort_scatter); the order within a bucket is arbitrary.
// No result depends on the queue order (each ray carries its sample id and
// its walk is its own), so the pixels and hit counts are unchanged.
constexpr bool kWSortLds = kWSortBuckets == 4096;               // counts aggregated in LDS per block
constexpr uint32_t kWSortChunk = 4096;                          // rays per sort block (16 per thread)
__device__ __forceinline__ uint32_t wh_cell(float o, float lo, float hi) {
    const float q = (o - lo) / (hi - lo) * (float)(1u << kWSortBits);
    // NaN and out-of-box origins clamp (any key is correct, only the order changes)
    return q >= 1.0f ? (q < (float)((1u << kWSortBits) - 1u) ? (uint32_t)q : (1u << kWSortBits) - 1u) : 0u;
}
__device__ __forceinline__ uint32_t wh_sort_key(const ClosestScene &s, const WQueue &q, uint64_t i) {
    uint32_t cell = 0;
    for (int c = 0; c < 3; ++c) {
        const uint32_t v = wh_cell(q.p[c * q.cap + i], s.slo[c], s.shi[c]);
        for (uint32_t b = 0; b < kWSortBits; ++b) cell |= ((v >> b) & 1u) << (3 * b + (2 - c));
    }
    const float dx = q.p[3 * q.cap + i], dy = q.p[4 * q.cap + i], dz = q.p[5 * q.cap + i];
    const uint32_t oct = (dx < 0.0f ? 1u : 0u) | (dy < 0.0f ? 2u : 0u) | (dz < 0.0f ? 4u : 0u);
    return (cell << 3) | oct;
}
// Per-block bucket counts of queue q's rays [blockIdx.x * chunk, +chunk) into
// LDS; SCATTER = false adds them to the global histogram, true reserves each
// non-zero bucket's range at its cursor and copies the rays to qout.
template <bool SCATTER>
__global__ void __launch_bounds__(256) k_wh_sort_pass(const RenderArgs a, uint32_t depth, WQueue qin, WQueue qout,
                                                      const uint32_t *counts, uint32_t *hist) {
    __shared__ uint32_t s_cnt[kWSortLds ? kWSortBuckets : 1];
    __shared__ uint32_t s_base[(SCATTER && kWSortLds) ? kWSortBuckets : 1];
    const uint32_t n = counts[depth];
    const uint64_t c0 = (uint64_t)blockIdx.x * kWSortChunk;
    if (c0 >= n) return;
    if (!kWSortLds) {
        // finer keys: one global atomic per ray (count, then the ray's slot)
        const ClosestScene sc = load_wscene(a);
        const uint32_t *sid_in = reinterpret_cast<const uint32_t *>(qin.p) + 6 * qin.cap;
        uint32_t *cur = hist + kWSortBuckets;
        for (uint32_t r = 0; r < kWSortChunk / 256; ++r) {
            const uint64_t i = c0 + r * 256 + threadIdx.x;
            if (i >= n) continue;
            const uint32_t key = wh_sort_key(sc, qin, i);
            if (!SCATTER) {
                atomicAdd(hist + key, 1u);
            } else {
                const uint64_t j = atomicAdd(cur + key, 1u);
                float o[3], d[3];
                for (int c = 0; c < 3; ++c) {
                    o[c] = qin.p[c * qin.cap + i];
                    d[c] = qin.p[(3 + c) * qin.cap + i];
                }
                qout.put(j, o, d, sid_in[i]);
            }
        }
        return;
    }
    for (uint32_t k = threadIdx.x; k < kWSortBuckets; k += 256) s_cnt[k] = 0u;
    __syncthreads();
    const ClosestScene sc = load_wscene(a);
    uint32_t key[kWSortChunk / 256], rank[kWSortChunk / 256];
#pragma unroll
    for (uint32_t r = 0; r < kWSortChunk / 256; ++r) {
        const uint64_t i = c0 + r * 256 + threadIdx.x;
        key[r] = i < n ? wh_sort_key(sc, qin, i) : 0u;
        rank[r] = i < n ? atomicAdd(&s_cnt[key[r]], 1u) : 0u;
    }
    __syncthreads();
    uint32_t *cur = hist + kWSortBuckets;   // [kWSortBuckets, 2 kWSortBuckets): scatter cursors
    for (uint32_t k = threadIdx.x; k < kWSortBuckets; k += 256) {
        const uint32_t c = s_cnt[k];
        if (SCATTER) s_base[k] = c ? atomicAdd(cur + k, c) : 0u;
        else if (c) atomicAdd(hist + k, c);
    }
    if (!SCATTER) return;
    __syncthreads();
    const uint32_t *sid_in = reinterpret_cast<const uint32_t *>(qin.p) + 6 * qin.cap;
#pragma unroll
    for (uint32_t r = 0; r < kWSortChunk / 256; ++r) {
        const uint64_t i = c0 + r * 256 + threadIdx.x;
        if (i >= n) continue;
        const uint64_t j = s_base[key[r]] + rank[r];
        float o[3], d[3];
        for (int c = 0; c < 3; ++c) {
            o[c] = qin.p[c * qin.cap + i];
            d[c] = qin.p[(3 + c) * qin.cap + i];
        }
        qout.put(j, o, d, sid_in[i]);
    }
}
// Bucket starts: cursors = exclusive scan of the histogram; the histogram is
// zeroed for the next bounce's count (one block of 1024 threads, kPer buckets each).
constexpr uint32_t kWSortPer = kWSortBuckets / 1024;
__global__ void __launch_bounds__(1024) k_wh_sort_scan(uint32_t *hist) {
    __shared__ uint32_t s_w[16];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    uint32_t v[kWSortPer], sum = 0;
    for (uint32_t k = 0; k < kWSortPer; ++k) {
        v[k] = hist[kWSortPer * t + k];
        sum += v[k];
    }
    uint32_t inc = sum;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t y = __shfl_up(inc, d, 64);
        if (lane >= d) inc += y;
    }
    if (lane == 63u) s_w[w] = inc;
    __syncthreads();
    uint32_t run = inc - sum;
    for (uint32_t k = 0; k < w; ++k) run += s_w[k];
    for (uint32_t k = 0; k < kWSortPer; ++k) {
        hist[kWSortBuckets + kWSortPer * t + k] = run;
        hist[kWSortPer * t + k] = 0u;
        run += v[k];
    }
}
static_assert(kWSortBuckets % 1024 == 0, "k_wh_sort_scan: 1024 threads x kWSortPer buckets");

// shade of a sample with h hits (oracle whitted_shade), f32
__device__ __forceinline__ void wh_shade(uint32_t h, float &r, float &g, float &b) {
    if (h > 8u) { r = 255.0f; g = 255.0f; b = 0.0f; h = 8u; }
    else { r = 20.0f; g = 20.0f; b = 40.0f; }
    for (uint32_t k = 0; k < h; ++k) {
        r = 0.5f * 255.0f + 0.5f * r;
        g = 0.5f * 255.0f + 0.5f * g;
        b = 0.5f * 0.0f + 0.5f * b;
    }
}

__global__ void __launch_bounds__(256) k_wh_shade(const RenderArgs a, const uint8_t *hits, uint32_t *d_hits) {
    const uint64_t P = (uint64_t)a.nrows * a.w;
    const uint64_t lp = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (lp >= P) return;
    float cr = 0.f, cg = 0.f, cb = 0.f;
    for (uint32_t s = 0; s < a.spp; ++s) {
        const uint32_t h = hits[lp * a.spp + s];
        if (d_hits) d_hits[lp * a.spp + s] = h;
        float r, g, b;
        wh_shade(h, r, g, b);
        cr += r; cg += g; cb += b;                     // col += Color(...), sample order
    }
    const float fs = (float)a.spp;
    a.out[lp] = rgb_to_int(cr / fs, cg / fs, cb / fs);
}

}  // namespace

static uint32_t whitted_grid(uint64_t rays) {
    int dev = 0, cus = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const uint64_t need = (rays + kWT - 1) / kWT, cap = (uint64_t)(cus > 0 ? cus : 256) * kWBlocksPerCU;
    return (uint32_t)(need < cap ? need : cap);
}

// two queues of 7 planes, 16 counters, per-sample hits (u8), the stack
// spill, the ray-order histogram and cursors
static uint64_t whitted_spill_words(uint64_t rays) {
    return (uint64_t)whitted_grid(rays) * kWT * (kWStack - kWLds) * 3;
}
size_t whitted_bytes(uint64_t rays) {
    const uint64_t q = 2 * 7 * rays * 4, hits = (rays + 255) & ~255ull;
    return q + kWCounts * 4 + hits + whitted_spill_words(rays) * 4 + 2 * kWSortBuckets * 4 + kWWorkWords * 8;
}
// the work counters of the last launch_whitted with counters on (u64[2 x 9]:
// nodes, triangles per bounce) and its rays per bounce (u32[9])
int whitted_work(const void *mem, uint64_t rays, uint32_t ray_counts[9], unsigned long long work[18],
                 void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    const char *base = reinterpret_cast<const char *>(mem);
    const uint32_t *counts = reinterpret_cast<const uint32_t *>(base + 14 * rays * 4);
    const uint8_t *hits = reinterpret_cast<const uint8_t *>(counts + kWCounts);
    const uint32_t *spill = reinterpret_cast<const uint32_t *>(hits + ((rays + 255) & ~255ull));
    const unsigned long long *w =
        reinterpret_cast<const unsigned long long *>(spill + whitted_spill_words(rays) + 2 * kWSortBuckets);
    hipError_t e = hipMemcpyAsync(ray_counts, counts, 9 * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(work, w, 18 * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return (int)e;
}

int launch_whitted(const RenderArgs &a, void *mem, uint64_t rays, uint32_t *d_hits, void *stream, void *ev_k0,
                   void *ev_k1, bool count, const unsigned long long *hit_mask, uint32_t tiles_x) {
    const hipStream_t st = (hipStream_t)stream;
    if (rays == 0) return 0;
    float *base = reinterpret_cast<float *>(mem);
    WQueue q0{base, rays}, q1{base + 7 * rays, rays};
    uint32_t *counts = reinterpret_cast<uint32_t *>(base + 14 * rays);
    uint8_t *hits = reinterpret_cast<uint8_t *>(counts + kWCounts);
    uint32_t *spill = reinterpret_cast<uint32_t *>(hits + ((rays + 255) & ~255ull));
    uint32_t *hist = spill + whitted_spill_words(rays);
    unsigned long long *work = reinterpret_cast<unsigned long long *>(hist + 2 * kWSortBuckets);
    if (count) {
        const hipError_t ez = hipMemsetAsync(work, 0, kWWorkWords * 8, st);
        if (ez != hipSuccess) return (int)ez;
    }
    if (hit_mask) {
        // k_wh_gen appends the primary samples that hit to queue 0
        const hipError_t ez = hipMemsetAsync(counts, 0, kWCounts * 4, st);
        if (ez != hipSuccess) return (int)ez;
    }
    hipLaunchKernelGGL(k_wh_gen, dim3((uint32_t)((rays + kWT - 1) / kWT)), dim3(kWT), 0, st, a, q0, counts, hits,
                       hist, hit_mask, tiles_x, (uint32_t)__builtin_ctz(a.spp));
    hipError_t e = ev_k0 ? hipEventRecord((hipEvent_t)ev_k0, st) : hipSuccess;
    if (e != hipSuccess) return (int)e;
    const uint32_t grid = whitted_grid(rays);
    // ray order (k_wh_sort_*; BIH_WH_SORT=0 for A/B): queue d+1 is written to
    // q1 and sorted back into q0, so every bounce reads q0
    static const bool sort_on = [] {
        const char *e = getenv("BIH_WH_SORT");
        return !(e && e[0] == '0');
    }();
    const bool srt = sort_on && a.n_nodes > 0;
    const uint32_t sort_blocks = (uint32_t)((rays + kWSortChunk - 1) / kWSortChunk);
    for (uint32_t d = 0; d <= 8; ++d) {
        const WQueue &qi = (srt || !(d & 1)) ? q0 : q1, &qo = (srt || !(d & 1)) ? q1 : q0;
        if (count)
            hipLaunchKernelGGL(k_wh_trace<true>, dim3(grid), dim3(kWT), 0, st, a, d, qi, qo, counts, hits, spill,
                               work);
        else
            hipLaunchKernelGGL(k_wh_trace<false>, dim3(grid), dim3(kWT), 0, st, a, d, qi, qo, counts, hits, spill,
                               work);
        if (srt && d < 8) {
            hipLaunchKernelGGL(k_wh_sort_pass<false>, dim3(sort_blocks), dim3(256), 0, st, a, d + 1, q1, q0,
                               counts, hist);
            hipLaunchKernelGGL(k_wh_sort_scan, dim3(1), dim3(1024), 0, st, hist);
            hipLaunchKernelGGL(k_wh_sort_pass<true>, dim3(sort_blocks), dim3(256), 0, st, a, d + 1, q1, q0,
                               counts, hist);
        }
    }
    e = ev_k1 ? hipEventRecord((hipEvent_t)ev_k1, st) : hipSuccess;
    if (e != hipSuccess) return (int)e;
    const uint64_t P = (uint64_t)a.nrows * a.w;
    hipLaunchKernelGGL(k_wh_shade, dim3((uint32_t)((P + 255) / 256)), dim3(256), 0, st, a, hits, d_hits);
    return (int)hipGetLastError();
}

}  // namespace bih
