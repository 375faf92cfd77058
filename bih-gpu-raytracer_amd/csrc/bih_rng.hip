// bih_rng.hip -- the per-pixel cuRAND XORWOW state: InitRandGPU (reference
// src/CUDAKernels.cu:450-459), the state a render leaves behind (:419) and the
// per-tile stamped state (RenderArgs::stamps), for gfx950 (MI355X).
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <mutex>

#include "bih_ray.h"

namespace bih {
namespace {

// ---------------------------------------------------------------------------
// RNG: v = M^skip * J^pixel * seed_state (J = M^(2^67)), cuRAND XORWOW.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void gf2_apply(const uint32_t *__restrict__ m, uint32_t x[5]) {
    uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0;
    for (int w = 0; w < 5; ++w) {
        uint32_t bits = x[w];
        while (bits) {
            int b = __ffs(bits) - 1;
            bits &= bits - 1;
            const uint32_t *c = m + (w * 32 + b) * 5;
            r0 ^= c[0]; r1 ^= c[1]; r2 ^= c[2]; r3 ^= c[3]; r4 ^= c[4];
        }
    }
    x[0] = r0; x[1] = r1; x[2] = r2; x[3] = r3; x[4] = r4;
}

// Per-pixel curand_init(seed, pixel, 0) + skip (InitRandGPU,
// CUDAKernels.cu:450-459).  The host applied M^skip to the seed state
// (powers of M commute).  A wave seeds a segment of 64 x kRngRun consecutive
// pixels of one row: lane l's first pixel jumps to its subsequence with at
// most 4 byte-table applies (J^(b << 8k)), its next ones (64 pixels further
// each) are one J^64 step through the nibble table in LDS, and the 64 lanes
// store 64 consecutive words per plane (coalesced: a lane-per-run layout
// spread each store over 64 lines and was store-bound at 0.18 ms / 1080p).
constexpr uint32_t kRngRun = 32;
__device__ __forceinline__ void jump_lds(const uint32_t *__restrict__ nib, uint32_t x[5]) {
    uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0;
#pragma unroll
    for (int g = 0; g < 40; ++g) {
        const uint32_t n = (x[g >> 3] >> ((g & 7) * 4)) & 15u;
        const uint32_t *c = nib + (g * 16 + n) * 5;
        r0 ^= c[0]; r1 ^= c[1]; r2 ^= c[2]; r3 ^= c[3]; r4 ^= c[4];
    }
    x[0] = r0; x[1] = r1; x[2] = r2; x[3] = r3; x[4] = r4;
}

__global__ void __launch_bounds__(kThreads) k_rng_init(uint32_t *__restrict__ rng, uint32_t w,
                                                       uint32_t row0, uint32_t nrows, uint32_t band_h,
                                                       uint32_t band_step, uint32_t s0, uint32_t s1,
                                                       uint32_t s2, uint32_t s3, uint32_t s4,
                                                       const uint32_t *__restrict__ tables) {
    __shared__ uint32_t s_nib[40 * 16 * 5];
    const uint32_t *nib64 = tables + 4 * 256 * 800 + 40 * 16 * 5;   // J^64
    for (uint32_t k = threadIdx.x; k < 40 * 16 * 5; k += kThreads) s_nib[k] = nib64[k];
    __syncthreads();
    constexpr uint32_t kSeg = 64 * kRngRun;
    const uint32_t segs = (w + kSeg - 1) / kSeg;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) >> 6;
    if (wave >= (uint64_t)nrows * segs) return;
    const uint32_t lr = (uint32_t)(wave / segs), x0 = (uint32_t)(wave % segs) * kSeg + lane;
    if (x0 >= w) return;
    const uint64_t pix = (uint64_t)global_row(lr, row0, band_h, band_step) * w + x0;
    uint32_t v[5] = {s0, s1, s2, s3, s4};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t b = (uint32_t)(pix >> (8 * k)) & 255u;
        if (b) gf2_apply(tables + ((uint32_t)k * 256 + b) * 800, v);
    }
    const uint64_t P = (uint64_t)nrows * w, lp0 = (uint64_t)lr * w + x0;
    for (uint32_t i = 0; i < kRngRun && x0 + 64 * i < w; ++i) {
        if (i) jump_lds(s_nib, v);
#pragma unroll
        for (int j = 0; j < 5; ++j) rng[(uint64_t)j * P + lp0 + 64 * i] = v[j];
    }
}

// dst = every pixel's XORWOW xorshift state `steps` draws after src's (dst
// may be src).  2*spp*nframes steps: the state the launch after a render of
// nframes frames starts from (cudaRender's write-back, CUDAKernels.cu:419);
// more: a gap in the frame sequence.  The Weyl counter d is derived from the
// frame index, not stored.  Up to two of the powers 2^7 .. 2^13 of `steps`
// jump through their nibble tables in LDS (40 lookups each, against 128 ..
// 8192 steps; the frame-jump tables of k_rng_sync), the rest is stepped.
// The tables are re-laid in LDS as words 0-3 (one ds_read_b128) + word 4 of
// each entry; each thread loads its PPT pixels' states before it jumps any
// (their loads in flight together), PPT pixels a grid's width apart.
__device__ __forceinline__ void jump_lds4(const uint4 *__restrict__ a, const uint32_t *__restrict__ b, uint32_t x[5]) {
    uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0;
#pragma unroll
    for (int g = 0; g < 40; ++g) {
        const uint32_t e = g * 16 + ((x[g >> 3] >> ((g & 7) * 4)) & 15u);
        const uint4 c = a[e];
        r0 ^= c.x; r1 ^= c.y; r2 ^= c.z; r3 ^= c.w; r4 ^= b[e];
    }
    x[0] = r0; x[1] = r1; x[2] = r2; x[3] = r3; x[4] = r4;
}
template <int PPT>
__global__ void __launch_bounds__(kThreads) k_rng_advance(const uint32_t *src, uint32_t *dst, uint64_t P,
                                                          uint32_t steps, const uint32_t *__restrict__ jumps,
                                                          uint32_t k0, uint32_t k1) {
    __shared__ uint4 s_a[2][40 * 16];
    __shared__ uint32_t s_b[2][40 * 16];
    const uint32_t nj = (k0 < 7u) + (k1 < 7u);
    for (uint32_t t = 0; t < nj; ++t) {
        const uint32_t *tab = jumps + (t ? k1 : k0) * kRngNibWords;
        for (uint32_t e = threadIdx.x; e < 40 * 16; e += kThreads) {
            s_a[t][e] = make_uint4(tab[5 * e], tab[5 * e + 1], tab[5 * e + 2], tab[5 * e + 3]);
            s_b[t][e] = tab[5 * e + 4];
        }
    }
    if (nj) __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t lp0 = (uint64_t)blockIdx.x * kThreads + threadIdx.x; lp0 < P; lp0 += stride * PPT) {
        uint32_t v[PPT][5];
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const uint64_t lp = lp0 + j * stride;
            if (lp < P) {
#pragma unroll
                for (int i = 0; i < 5; ++i) v[j][i] = src[(uint64_t)i * P + lp];
            }
        }
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            for (uint32_t t = 0; t < nj; ++t) jump_lds4(s_a[t], s_b[t], v[j]);
#pragma unroll 8
            for (uint32_t k = 0; k < steps; ++k) {
                const uint32_t t = v[j][0] ^ (v[j][0] >> 2);
                v[j][0] = v[j][1]; v[j][1] = v[j][2]; v[j][2] = v[j][3]; v[j][3] = v[j][4];
                v[j][4] = (v[j][4] ^ (v[j][4] << 4)) ^ (t ^ (t << 1));
            }
        }
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const uint64_t lp = lp0 + j * stride;
            if (lp < P) {
#pragma unroll
                for (int i = 0; i < 5; ++i) dst[(uint64_t)i * P + lp] = v[j][i];
            }
        }
    }
}

// Stamped state (RenderArgs::stamps): every tile at frame F in buffer 0.
__global__ void __launch_bounds__(kThreads) k_stamp_init(unsigned long long *__restrict__ stamps, uint32_t ntiles,
                                                         uint32_t frame) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t < ntiles)
        stamps[t] = (unsigned long long)frame | ((unsigned long long)frame << 27);   // cur = prev = (F, 0), seq 0
}
// Every pixel's stamped state brought to frame `target` (2*spp draws per
// frame): into its tile's other buffer with the tile's new stamp (launch
// `seq`; the tile's first pixel writes it), or -- full != null -- into `full`
// for every pixel, leaving the stamps as they are (back to the ring).  Whole
// kStampJumpFrames runs jump through the nibble table of their matrix (40
// lookups against 64 * 2 * spp steps: background tiles lag by exactly that
// much between syncs), the rest is stepped.  Grid-stride, so that few blocks
// load the table into LDS.
__global__ void __launch_bounds__(kThreads) k_rng_sync(unsigned long long *__restrict__ stamps, uint32_t *buf0,
                                                       uint32_t *buf1, uint32_t *__restrict__ full, uint32_t w,
                                                       uint32_t nrows, uint32_t log2spp, uint32_t target,
                                                       uint32_t seq, const uint32_t *__restrict__ jump) {
    __shared__ uint32_t s_nib[kRngNibWords];
    for (uint32_t k = threadIdx.x; k < kRngNibWords; k += kThreads) s_nib[k] = jump[k];
    __syncthreads();
    const uint64_t P = (uint64_t)nrows * w;
    const Tiles tl = tiles_of(w, nrows, 1u << log2spp);
    const uint32_t tw = tl.tw, th = tl.th, tiles_x = tl.x;
    for (uint64_t lp = (uint64_t)blockIdx.x * kThreads + threadIdx.x; lp < P; lp += (uint64_t)gridDim.x * kThreads) {
        const uint32_t lr = (uint32_t)(lp / w), x = (uint32_t)(lp - (uint64_t)lr * w);
        const uint32_t t = (lr / th) * tiles_x + x / tw;
        const StampBase sb = stamp_base(stamps[t], seq);
        if (!full && sb.F >= target) continue;   // already at the frame
        const uint32_t *src = sb.b ? buf1 : buf0;
        uint32_t v[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) v[i] = src[(uint64_t)i * P + lp];
        const uint32_t lag = target - sb.F;
        for (uint32_t q = 0; q < lag / kStampJumpFrames; ++q) jump_lds(s_nib, v);
        xorwow_steps(v, (lag % kStampJumpFrames) << (log2spp + 1));
        uint32_t *dst = full ? full : (sb.b ? buf0 : buf1);
#pragma unroll
        for (int i = 0; i < 5; ++i) dst[(uint64_t)i * P + lp] = v[i];
        if (!full && lr % th == 0 && x % tw == 0) stamps[t] = stamp_pack(target, sb.b ^ 1u, sb, seq);
    }
}

std::mutex g_tab_mu;
uint32_t *g_tab_dev[64] = {nullptr};

}  // namespace

int upload_rng_tables(int device) {
    if (device < 0 || device >= 64) return (int)hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lk(g_tab_mu);
    if (g_tab_dev[device]) return 0;
    const size_t bytes = kRngInitWords * sizeof(uint32_t);
    uint32_t *p = nullptr;
    hipError_t e = hipMalloc((void **)&p, bytes);
    if (e != hipSuccess) return (int)e;
    e = hipMemcpy(p, xorwow_init_tables_host(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(p); return (int)e; }
    g_tab_dev[device] = p;
    return 0;
}

const uint32_t *rng_tables_device(int device) {
    std::lock_guard<std::mutex> lk(g_tab_mu);
    return (device >= 0 && device < 64) ? g_tab_dev[device] : nullptr;
}

int launch_rng_init(uint32_t *rng, uint32_t w, uint32_t row0, uint32_t nrows, uint32_t band_h,
                    uint32_t band_step, uint64_t seed, uint64_t skip, int device, void *stream) {
    const uint32_t *tab = rng_tables_device(device);
    if (!tab) return (int)hipErrorNotInitialized;
    uint32_t v[5], d;
    xorwow_seed(seed, v, &d);
    xorwow_skip(v, skip);   // M^skip commutes with the subsequence jumps
    const uint64_t threads = (uint64_t)nrows * ((w + 64 * kRngRun - 1) / (64 * kRngRun)) * 64;
    if (threads == 0) return 0;
    const uint32_t blocks = (uint32_t)((threads + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_rng_init, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, rng, w, row0,
                       nrows, band_h, band_step, v[0], v[1], v[2], v[3], v[4], tab);
    return (int)hipGetLastError();
}

int launch_stamp_init(unsigned long long *stamps, uint32_t ntiles, uint32_t frame, void *stream) {
    if (ntiles == 0) return 0;
    hipLaunchKernelGGL(k_stamp_init, dim3((ntiles + kThreads - 1) / kThreads), dim3(kThreads), 0,
                       (hipStream_t)stream, stamps, ntiles, frame);
    return (int)hipGetLastError();
}

int launch_rng_sync(unsigned long long *stamps, uint32_t *buf0, uint32_t *buf1, uint32_t *full, uint32_t w,
                    uint32_t nrows, uint32_t spp, uint32_t target, uint32_t seq, int device, void *stream) {
    const uint64_t P = (uint64_t)nrows * w;
    if (P == 0) return 0;
    const uint32_t *tab = rng_tables_device(device);
    if (!tab || spp == 0 || spp > 64 || (spp & (spp - 1))) return (int)hipErrorInvalidValue;
    const uint32_t L = (uint32_t)__builtin_ctz(spp);
    // 8 pixels per thread: 1/8 of the blocks load the 12.8 KB table
    const uint64_t blocks = (P + 8 * kThreads - 1) / (8 * kThreads);
    hipLaunchKernelGGL(k_rng_sync, dim3((uint32_t)blocks), dim3(kThreads), 0, (hipStream_t)stream, stamps, buf0, buf1,
                       full, w, nrows, L, target, seq, tab + kRngJumpOffset + L * kRngNibWords);
    return (int)hipGetLastError();
}

int launch_rng_advance(const uint32_t *src, uint32_t *dst, uint64_t pixels, uint32_t steps, int device,
                       void *stream) {
    if (pixels == 0 || (steps == 0 && src == dst)) return 0;
    const uint32_t *tab = rng_tables_device(device);
    if (!tab) return (int)hipErrorNotInitialized;
    // the two highest powers 2^7 .. 2^13 of `steps` through tables (index
    // k - 7; 7 = none), unless BIH_ADVANCE_JUMP=0 (A/B)
    static const bool jump = [] {
        const char *e = getenv("BIH_ADVANCE_JUMP");
        return !(e && e[0] == '0');
    }();
    uint32_t k0 = 7, k1 = 7, rest = steps;
    for (int k = 13; k >= 7 && jump && k1 == 7u; --k)
        if (rest >> k & 1u) {
            rest &= ~(1u << k);
            if (k0 == 7u) k0 = (uint32_t)k - 7;
            else k1 = (uint32_t)k - 7;
        }
    // with tables: up to 8 pixels per thread (fewer blocks load them), at
    // least ~2048 blocks (a rank's share of the rows is 1/8 of the frame)
    uint32_t ppt = 1;
    if (k0 < 7u)
        while (ppt < 8u && pixels > 2ull * ppt * 2048ull * kThreads) ppt *= 2;
    const uint64_t per = (uint64_t)ppt * kThreads;
    const uint32_t blocks = (uint32_t)((pixels + per - 1) / per);
    const uint32_t *jt = tab + kRngJumpOffset;
    const hipStream_t st = (hipStream_t)stream;
    if (ppt == 8)
        hipLaunchKernelGGL(k_rng_advance<8>, dim3(blocks), dim3(kThreads), 0, st, src, dst, (uint64_t)pixels, rest, jt, k0, k1);
    else if (ppt == 4)
        hipLaunchKernelGGL(k_rng_advance<4>, dim3(blocks), dim3(kThreads), 0, st, src, dst, (uint64_t)pixels, rest, jt, k0, k1);
    else if (ppt == 2)
        hipLaunchKernelGGL(k_rng_advance<2>, dim3(blocks), dim3(kThreads), 0, st, src, dst, (uint64_t)pixels, rest, jt, k0, k1);
    else
        hipLaunchKernelGGL(k_rng_advance<1>, dim3(blocks), dim3(kThreads), 0, st, src, dst, (uint64_t)pixels, rest, jt, k0, k1);
    return (int)hipGetLastError();
}

}  // namespace bih
