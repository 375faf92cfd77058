// bih_prim.hip -- the camera-relative records of a primary-ray origin: triangle
// and node records (exact and culled) and the any-hit walk's shortcut boxes.
#include <hip/hip_runtime.h>

#include "bih_bound.h"
#include "bih_ray.h"

namespace bih {
namespace {

// A primary ray from O can hit triangle k only if its tnum = dot(e2, q) (the
// ray-independent numerator of t, k_tri_prim) is a positive finite f32:
// t = tnum * (1/det) with 1/det > 0 finite for every lane that passes the
// det test (CUDAKernels.cu:33-47), so tnum <= 0, +inf or NaN gives t <= 0,
// inf or NaN, and the t > 0 && t < FLT_MAX test fails for every ray.
__device__ __forceinline__ bool tri_alive(const float *prim, uint32_t k) {
    return dev::tnum_alive(prim[16ull * k + 12]);
}

// Leaf k can produce a hit only if one of its triangles [first[k],
// first[k] + cnt[k]) is alive; long duplicate runs count as alive unscanned.
__global__ void __launch_bounds__(kThreads) k_leaf_alive(const float *__restrict__ prim,
                                                         const int32_t *__restrict__ first,
                                                         const uint32_t *__restrict__ cnt,
                                                         uint32_t U, uint8_t *__restrict__ alive) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= U) return;
    const uint32_t b = (uint32_t)first[k], c = cnt[k];
    bool a = c > 64u;
    for (uint32_t i = 0; !a && i < c; ++i) a = tri_alive(prim, b + i);
    alive[k] = a ? 1 : 0;
}

// Internal node p is alive if a child is (leaf: leaf_alive; internal: this
// array).  Starts all-alive and only ever clears entries whose children are
// both dead, so any number of passes (run in place, in any order) leaves a
// conservative answer; dead subtrees of height h need h passes.
__global__ void __launch_bounds__(kThreads) k_node_alive(const uint4 *__restrict__ nodes, uint32_t m,
                                                         const uint8_t *__restrict__ leaf_alive,
                                                         uint8_t *__restrict__ node_alive) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= m || !node_alive[p]) return;
    const uint4 nd = nodes[p];
    const uint32_t split = nd.z & 0x7ffffffu;
    const bool aL = ((nd.z >> 29) & 1u) ? leaf_alive[split] : node_alive[split];
    const bool aR = ((nd.z >> 30) & 1u) ? leaf_alive[split + 1] : node_alive[split + 1];
    if (!aL && !aR) node_alive[p] = 0;
}

// Camera-relative node records {clip0 - O[axis], clip1 - O[axis], z', w'} with
// z' = split << 8 | axis (z' >> 4: the byte offset of the children's record
// pair; the low byte is the axis alone, an s_set_gpr_idx_on index) and w' =
// the packed w (mid | cntL << 27 | cntR << 29) | leafL << 26 | leafR << 31 --
// for split < 2^24 and mid < 2^26, the scenes the packet kernels take
// (packet_records_fit) -- and the
// same records with every child subtree that no primary ray from O can
// hit (all its triangles dead, tri_alive) cut off: clip0 - O = -inf (left) /
// clip1 - O = +inf (right) make t0 = -inf*inv / t1 = +inf*inv fail the
// child's visit test (tMin < t[near], !(tMax < t[far])) for either ray
// direction, so the walk never enters it.  Only which dead subtrees are
// visited changes, so the hit set -- and the image -- is the same; the
// per-ray counters are not, and STATS launches use the exact records.
__global__ void __launch_bounds__(kThreads) k_node_prim(const uint4 *__restrict__ nodes, uint32_t m,
                                                        float ox, float oy, float oz,
                                                        const uint8_t *__restrict__ leaf_alive,
                                                        const uint8_t *__restrict__ node_alive,
                                                        uint4 *__restrict__ out,
                                                        uint4 *__restrict__ out_cull) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= m) return;
    const uint4 nd = nodes[i];
    const uint32_t ax = (nd.z >> 27) & 3u;
    const float org = sel3(ax, ox, oy, oz);
    const uint32_t split = nd.z & 0x7ffffffu;
    const uint32_t z = (split << 8) | ax;
    const uint32_t w = nd.w | (((nd.z >> 29) & 1u) << 26) | (((nd.z >> 30) & 1u) << 31);
    uint4 r = make_uint4(__float_as_uint(__uint_as_float(nd.x) - org),
                         __float_as_uint(__uint_as_float(nd.y) - org), z, w);
    out[i] = r;
    if (!out_cull) return;   // records only (launch_prim); the culled set follows in launch_prim_cull
    const bool aL = ((nd.z >> 29) & 1u) ? leaf_alive[split] : node_alive[split];
    const bool aR = ((nd.z >> 30) & 1u) ? leaf_alive[split + 1] : node_alive[split + 1];
    if (!aL) r.x = 0xff800000u;   // -inf
    if (!aR) r.y = 0x7f800000u;   // +inf
    out_cull[i] = r;
}

// Primary-ray triangle records for the camera origin O (every primary ray of
// a frame starts at O, Camera.cu:18-20): dev::tri_prim_record per
// Morton-ordered triangle.  (Renders through the frustum bins get the same
// records from k_cam_tris, bih_bins.hip.)
__global__ void __launch_bounds__(kThreads) k_tri_prim(const float *__restrict__ tris, uint32_t n,
                                                       float ox, float oy, float oz,
                                                       float *__restrict__ prim) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    (void)dev::tri_prim_record(tris + 9ull * i, ox, oy, oz, prim + 16ull * i);
}

// ---------------------------------------------------------------------------
// Shortcut boxes (the any-hit walk's shortcut passes, k_render_packet_asm):
// per internal node p a 64-byte record {box of child 0 (lo xyz, hi xyz), box
// of child 1, ref 0, ref 1, leaf 0, leaf 1}, camera-relative (box - O), each
// box an AABB of the child subtree's ALIVE triangles (tri_alive: the only
// ones that can produce a hit from O) -- set 1 tight, set 2 the miss-proof
// boxes (miss_box).  ref = internal node index, or kFastLeaf | leaf index,
// or kFastDead (no alive triangle below); leaf s = first | min(count, 63) << 26
// for a leaf child (63: read dup_cnt).  The topology is the BIH's own
// (children {split, split+1}); only the culling geometry differs.  Nothing
// here decides a pixel by itself: a hit found through these boxes is kept
// only after the exact BIH decisions are replayed along the leaf's root path
// (fast_verify); a miss only when the miss-proof walk finds no triangle the
// exact intersector accepts; every other lane runs the exact walk.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void fbox_put(float *slot, const float lo[3], const float hi[3]) {
    int32_t acc = 0;
    int32_t *s = reinterpret_cast<int32_t *>(slot);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        acc ^= atomicExch(s + c, __float_as_int(lo[c]));
        acc ^= atomicExch(s + 3 + c, __float_as_int(hi[c]));
    }
    asm volatile("" ::"v"(acc) : "memory");
}
__device__ __forceinline__ void fbox_get(float *slot, float lo[3], float hi[3]) {
    int32_t *s = reinterpret_cast<int32_t *>(slot);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        lo[c] = __int_as_float(atomicOr(s + c, 0));
        hi[c] = __int_as_float(atomicOr(s + 3 + c, 0));
    }
}

// Miss-proof box of one alive triangle (camera-relative), from its primary-ray
// record r and dmax[] (miss_bary, bih_bound.h): the AABB of the inflated
// triangle of barycentric corners (-a, -b), (1+b+c, -b), (-a, 1+a+c), padded
// by 1e-5 + 1e-6|x| (far more than the slab test's own rounding).  If the
// exact intersector returns a hit for direction D, the line O + t D passes
// through this box.  No bound gives the unbounded box.
__device__ __forceinline__ void miss_box(const float *r, const float *dmax, float lo[3],
                                         float hi[3]) {
    const float e1[3] = {r[0], r[1], r[2]}, e2[3] = {r[3], r[4], r[5]};
    const float sv[3] = {r[6], r[7], r[8]};
    float a, bb, c;
    bool ok = miss_bary(r, dmax, a, bb, c);
    const float cu[3] = {-a, 1.0f + bb + c, -a}, cv[3] = {-bb, -bb, 1.0f + a + c};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        float l = INFINITY, h = -INFINITY;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float x = (cu[j] * e1[ax] + cv[j] * e2[ax]) - sv[ax];
            l = fminf(l, x);
            h = fmaxf(h, x);
        }
        lo[ax] = l - (1e-5f + 1e-6f * fabsf(l));
        hi[ax] = h + (1e-5f + 1e-6f * fabsf(h));
        ok = ok && lo[ax] > -1e30f && hi[ax] < 1e30f;
    }
    if (!ok) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) { lo[ax] = -INFINITY; hi[ax] = INFINITY; }
    }
}

// One thread per leaf: the leaf's box of alive triangles (empty: lo = +inf,
// hi = -inf), then up the parent chain; the second arriver at a node unions
// both slots and climbs on (the same hand-off as the builder's k_fit).
__global__ void __launch_bounds__(kThreads) k_fast_fit(const float *__restrict__ tris,
                                                       const float *__restrict__ prim,
                                                       const int32_t *__restrict__ first,
                                                       const uint32_t *__restrict__ cnt,
                                                       const int32_t *__restrict__ leaf_parent,
                                                       const int32_t *__restrict__ parent,
                                                       const uint4 *__restrict__ nodes, uint32_t U,
                                                       float ox, float oy, float oz,
                                                       bool cons, float dmx, float dmy, float dmz,
                                                       uint32_t *__restrict__ arrive,
                                                       float *fast) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (U < 2 || k >= U) return;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const uint32_t b = (uint32_t)first[k], c = cnt[k];
    const float o[3] = {ox, oy, oz};
    for (uint32_t i = b; i < b + c; ++i) {
        if (!tri_alive(prim, i)) continue;
        float tlo[3], thi[3];
        if (cons) {
            const float dmax[3] = {dmx, dmy, dmz};
            miss_box(prim + 16ull * i, dmax, tlo, thi);
        } else {
            const float *t = tris + 9ull * i;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float v0 = t[a] - o[a], v1 = v0 + t[3 + a], v2 = v0 + t[6 + a];
                tlo[a] = fminf(v0, fminf(v1, v2));
                thi[a] = fmaxf(v0, fmaxf(v1, v2));
            }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], tlo[a]);
            hi[a] = fmaxf(hi[a], thi[a]);
        }
    }
    int32_t prev = (int32_t)k;
    bool prev_leaf = true;
    int32_t p = leaf_parent[k];
    while (p >= 0) {
        const uint32_t z = nodes[p].z;
        const uint32_t split = z & kIdxMask;
        const bool leafL = (z >> 29) & 1u;
        // child 0 is `split` (a leaf iff leafL), child 1 is split + 1
        const int side = ((uint32_t)prev == split && prev_leaf == leafL) ? 0 : 1;
        const int32_t pp = parent[p];
        fbox_put(fast + 16ull * p + 6 * side, lo, hi);
        if (atomicAdd(arrive + p, 1u) == 0u) return;
        float slo[3], shi[3];
        fbox_get(fast + 16ull * p + 6 * (1 - side), slo, shi);
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], slo[a]); hi[a] = fmaxf(hi[a], shi[a]); }
        prev = p;
        prev_leaf = false;
        p = pp;
    }
}

// Child refs of every record, once both boxes are in.
__global__ void __launch_bounds__(kThreads) k_fast_refs(const uint4 *__restrict__ nodes, uint32_t m,
                                                        const int32_t *__restrict__ first,
                                                        const uint32_t *__restrict__ cnt,
                                                        float *__restrict__ fast) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= m) return;
    const uint32_t z = nodes[p].z;
    const uint32_t split = z & kIdxMask;
    float *r = fast + 16ull * p;
    uint32_t ref[2], fst[2] = {0u, 0u};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const bool leaf = (z >> (29 + s)) & 1u;
        const bool dead = !(r[6 * s] <= r[6 * s + 3]);   // empty box (or never reached)
        ref[s] = dead ? kFastDead : leaf ? (kFastLeaf | (split + s)) : (split + s);
        if (dead)   // NaN box: every slab test of it fails
            for (int c = 0; c < 6; ++c) r[6 * s + c] = __uint_as_float(0x7fc00000u);
        if (leaf) {
            // first | count << 26 (count 63: read dup_cnt; first < 2^26 for
            // the scenes the packet kernel takes, packet_records_fit)
            const uint32_t c = cnt[split + s];
            fst[s] = (uint32_t)first[split + s] | ((c < 63u ? c : 63u) << 26);
        }
    }
    r[12] = __uint_as_float(ref[0]);
    r[13] = __uint_as_float(ref[1]);
    r[14] = __uint_as_float(fst[0]);
    r[15] = __uint_as_float(fst[1]);
}

}  // namespace

// triangle records, then the exact and the culled node records, each with
// one record of padding (the packet walk prefetches the record pair {split,
// split+1}, and split+1 may be one past the last internal node), then the
// leaf and node alive bytes
size_t alive_bytes(uint32_t m) { return ((size_t)(m + 1) + m + 15) & ~(size_t)15; }
size_t prim_bytes(uint32_t n, uint32_t m) {
    return (size_t)n * 64 + 2 * (size_t)(m + 1) * 16 + alive_bytes(m) +
           2 * (size_t)(m + 1) * 64 + (size_t)m * 4;
}
size_t fast_offset(uint32_t n, uint32_t m) {
    return (size_t)n * 64 + 2 * (size_t)(m + 1) * 16 + alive_bytes(m);
}

// (n triangles, m = U-1 internal nodes of the tree the records are for)
static uint32_t internal_nodes(const DeviceTree &t) { return t.u > 0 ? t.u - 1 : 0; }

int launch_prim(const DeviceTree &t, const float origin[3], float *prim, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    const uint32_t n = t.n, m = internal_nodes(t);
    if (n > 0)
        hipLaunchKernelGGL(k_tri_prim, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, st,
                           t.tris_s, n, origin[0], origin[1], origin[2], prim);
    if (m > 0) {
        uint4 *rec = reinterpret_cast<uint4 *>(prim + 16ull * n);
        const dim3 gn((m + kThreads - 1) / kThreads);
        hipLaunchKernelGGL(k_node_prim, gn, dim3(kThreads), 0, st, t.nodes, m, origin[0], origin[1],
                           origin[2], nullptr, nullptr, rec, nullptr);
    }
    return (int)hipGetLastError();
}

// The culled node records (node_cull) for the records launch_prim wrote:
// only the BIH walk kernels read them, so renders through the frustum bins
// never pay for them (bih_capi.cpp builds them on first use per camera).
int launch_prim_cull(const DeviceTree &t, const float origin[3], float *prim, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    const uint32_t m = internal_nodes(t);
    if (m > 0) {
        uint4 *rec = reinterpret_cast<uint4 *>(prim + 16ull * t.n);
        uint8_t *leaf_alive = reinterpret_cast<uint8_t *>(rec + 2 * (size_t)(m + 1));
        uint8_t *node_alive = leaf_alive + (m + 1);
        const dim3 gl((m + 1 + kThreads - 1) / kThreads), gn((m + kThreads - 1) / kThreads);
        hipLaunchKernelGGL(k_leaf_alive, gl, dim3(kThreads), 0, st, prim, t.first_idx, t.dup_cnt, m + 1,
                           leaf_alive);
        hipError_t e = hipMemsetAsync(node_alive, 1, m, st);
        if (e != hipSuccess) return (int)e;
        // dead subtrees of a random soup are a few levels high (1M triangles:
        // 12 % of the nodes, every one found within 7 passes)
        for (int pass = 0; pass < 8; ++pass)
            hipLaunchKernelGGL(k_node_alive, gn, dim3(kThreads), 0, st, t.nodes, m, leaf_alive,
                               node_alive);
        hipLaunchKernelGGL(k_node_prim, gn, dim3(kThreads), 0, st, t.nodes, m, origin[0], origin[1],
                           origin[2], leaf_alive, node_alive, rec, rec + (m + 1));
    }
    return (int)hipGetLastError();
}

// The any-hit BIH walk's shortcut boxes for the records launch_prim wrote
// (only renders without frustum bins read them).
int launch_fast_boxes(const DeviceTree &t, const float origin[3], const float dmax[3], float *prim, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    const uint32_t m = internal_nodes(t);
    if (m > 0) {
        const dim3 gl((m + 1 + kThreads - 1) / kThreads), gn((m + kThreads - 1) / kThreads);
        hipError_t e = hipSuccess;
        // shortcut boxes of the any-hit walk: tight (pass 1), miss-proof (pass 2)
        float *fast = reinterpret_cast<float *>(reinterpret_cast<char *>(prim) + fast_offset(t.n, m));
        uint32_t *arrive = reinterpret_cast<uint32_t *>(fast + 2 * 16ull * (m + 1));
        for (int pass = 0; pass < 2; ++pass) {
            float *boxes = fast + pass * 16ull * (m + 1);
            e = hipMemsetAsync(arrive, 0, sizeof(uint32_t) * m, st);
            if (e != hipSuccess) return (int)e;
            hipLaunchKernelGGL(k_fast_fit, gl, dim3(kThreads), 0, st, t.tris_s, prim, t.first_idx,
                               t.dup_cnt, t.leaf_parent, t.parent, t.nodes, m + 1, origin[0], origin[1],
                               origin[2], pass == 1, dmax[0], dmax[1], dmax[2], arrive, boxes);
            hipLaunchKernelGGL(k_fast_refs, gn, dim3(kThreads), 0, st, t.nodes, m, t.first_idx, t.dup_cnt,
                               boxes);
        }
    }
    return (int)hipGetLastError();
}

}  // namespace bih
