// bih_denoise.hip -- the edge-avoiding a-trous denoiser (bih_denoise_device /
// bih_denoise, include/bih.h) on gfx950.
//
// Semantics: the header's, operation for operation (-ffp-contract=off): a
// valid pixel (depth < FLT_MAX) is the weighted mean of the valid taps of a
// 5 x 5 B3-spline stencil with holes (step 1 << pass), each tap weighted by
// the agreement of its normal, its position on the centre's tangent plane and
// its colour with the centre's; the taps are summed with dy the outer and dx
// the inner loop, ascending, and a tap contributes exactly when its weight is
// > 0.
//
// k_denoise_setup packs what every pass gathers into 16-byte records, one
// plane each: {Pos, valid}, {n, 0} and the colour {R, G, B, 0} (pass 0's
// input: the caller's radiance is never read again, so it may be the output).
// k_denoise_pass runs once per pass, one pixel per lane, in blocks of kTW x kTH
// pixels (a wave: two rows of 32 pixels, 512 contiguous bytes per record plane
// and tap): 25 gathers of the three records through the caches, the step a
// kernel argument.  A tap outside the image reads the centre's records instead
// (every index stays inside the planes) and is masked out.  The last pass
// writes radiance_out and rgba_out and no record.  Staging a block's tile and
// halo in LDS for the steps 1 and 2 was measured and lost:
// the gathers of a wave are contiguous rows, which the caches serve as well.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>

#include "bih_internal.h"

namespace bih {
namespace {

constexpr uint32_t kDT = 256;                  // threads per block
constexpr uint32_t kTW = 32, kTH = 8;          // a block's pixels
static_assert(kTW * kTH == kDT, "one pixel per lane");
constexpr uint32_t kMaxBlocks = 1u << 20;      // blocks of a launch (each strides over the tiles)
constexpr uint32_t kMissShade = 0x00281414u;   // bih_render_direct's miss shade

struct SetupArgs {
    float cam[12];              // origin, lower_left, horizontal, vertical
    uint32_t w, h, pixels;
    const float *radiance, *depth, *normal;
    float4 *pos, *nrm, *col;
};

struct PassArgs {
    uint32_t w, h, tiles_x, ntiles;
    uint32_t step, squarings;
    float sigma_plane;
    float sc2;                  // (sigma_colour * 2^-pass)^2
    const float4 *pos, *nrm, *cin;
    float4 *cout;               // null: the last pass
    float *radiance_out;        // the last pass's outputs, either may be null
    uint32_t *rgba_out;
};

__global__ void __launch_bounds__(kDT) k_denoise_setup(const SetupArgs a) {
    for (uint32_t p = blockIdx.x * kDT + threadIdx.x; p < a.pixels; p += gridDim.x * kDT) {
        const uint32_t x = p % a.w, y = p / a.w;
        const float depth = a.depth[p];
        const float u = ((float)x + 0.5f) / (float)a.w;
        const float v = ((float)y + 0.5f) / (float)a.h;
        float P[3];
        for (int c = 0; c < 3; ++c) {
            const float d = ((a.cam[3 + c] + u * a.cam[6 + c]) + v * a.cam[9 + c]) - a.cam[c];
            P[c] = a.cam[c] + depth * d;
        }
        const size_t p3 = (size_t)3 * p;
        a.pos[p] = make_float4(P[0], P[1], P[2], depth < FLT_MAX ? 1.0f : 0.0f);
        a.nrm[p] = make_float4(a.normal[p3], a.normal[p3 + 1], a.normal[p3 + 2], 0.0f);
        a.col[p] = make_float4(a.radiance[p3], a.radiance[p3 + 1], a.radiance[p3 + 2], 0.0f);
    }
}

// g(x) = t*t, t = fmaxf(0, 1 - x): 1 at 0, 0 from 1 on, 0 for NaN
__device__ __forceinline__ float support(float x) {
    const float t = fmaxf(0.0f, 1.0f - x);
    return t * t;
}

// One tap of a valid centre {pp, np, cp} at q's records: the header's weight,
// added to the sums when the tap is there (inside the image, valid) and w > 0.
__device__ __forceinline__ void tap(const PassArgs &a, float k, const float4 &pp, const float4 &np, const float4 &cp,
                                    const float4 &pq, const float4 &nq, const float4 &cq, bool there, float sum[3],
                                    float &wsum) {
    const float dn = (np.x * nq.x + np.y * nq.y) + np.z * nq.z;
    float m = fmaxf(0.0f, dn);
    for (uint32_t j = 0; j < a.squarings; ++j) m = m * m;
    const float e0 = pq.x - pp.x, e1 = pq.y - pp.y, e2 = pq.z - pp.z;
    const float pd = (np.x * e0 + np.y * e1) + np.z * e2;
    const float wp = support(fabsf(pd) / a.sigma_plane);
    const float d0 = cq.x - cp.x, d1 = cq.y - cp.y, d2 = cq.z - cp.z;
    const float dd = (d0 * d0 + d1 * d1) + d2 * d2;
    const float wc = support(dd / a.sc2);
    const float wt = ((k * m) * wp) * wc;
    if (there && pq.w != 0.0f && wt > 0.0f) {
        sum[0] = sum[0] + wt * cq.x;
        sum[1] = sum[1] + wt * cq.y;
        sum[2] = sum[2] + wt * cq.z;
        wsum = wsum + wt;
    }
}

// the B3 spline's tap weight K[|dx|] * K[|dy|]
__device__ __forceinline__ float spline(int dx, int dy) {
    const float kern[3] = {0.375f, 0.25f, 0.0625f};
    return kern[dx < 0 ? -dx : dx] * kern[dy < 0 ? -dy : dy];
}

// Pixel p's result of the pass: the next colour record, or (the last pass) the caller's planes.
__device__ __forceinline__ void write_pixel(const PassArgs &a, uint32_t p, const float out[3], bool valid) {
    if (a.cout) {
        a.cout[p] = make_float4(out[0], out[1], out[2], 0.0f);
        return;
    }
    if (a.radiance_out) {
        const size_t p3 = (size_t)3 * p;
        for (int c = 0; c < 3; ++c) a.radiance_out[p3 + c] = out[c];
    }
    if (a.rgba_out) {
        uint32_t px = 0u;
        for (int c = 0; c < 3; ++c) px |= (uint32_t)(int)fmaxf(0.0f, fminf(255.0f, 255.0f * out[c])) << (8 * c);
        a.rgba_out[p] = valid ? px : kMissShade;
    }
}

__global__ void __launch_bounds__(kDT) k_denoise_pass(const PassArgs a) {
    const uint32_t lx = threadIdx.x % kTW, ly = threadIdx.x / kTW;
    const int step = (int)a.step;
    for (uint32_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const uint32_t x = (t % a.tiles_x) * kTW + lx, y = (t / a.tiles_x) * kTH + ly;
        if (x >= a.w || y >= a.h) continue;
        const uint32_t p = y * a.w + x;
        const float4 pp = a.pos[p], np = a.nrm[p], cp = a.cin[p];
        float out[3] = {cp.x, cp.y, cp.z};
        const bool valid = pp.w != 0.0f;
        if (valid) {
            float sum[3] = {0.0f, 0.0f, 0.0f}, wsum = 0.0f;
#pragma unroll
            for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
                for (int dx = -2; dx <= 2; ++dx) {
                    const float k = spline(dx, dy);
                    if (dx == 0 && dy == 0) {
                        for (int c = 0; c < 3; ++c) sum[c] = sum[c] + k * out[c];
                        wsum = wsum + k;
                        continue;
                    }
                    // |dx * step| <= 256 and x < 2^28: no overflow; a negative coordinate wraps past w
                    const uint32_t qx = (uint32_t)((int)x + dx * step), qy = (uint32_t)((int)y + dy * step);
                    const bool inside = qx < a.w && qy < a.h;
                    const uint32_t q = inside ? qy * a.w + qx : p;
                    tap(a, k, pp, np, cp, a.pos[q], a.nrm[q], a.cin[q], inside, sum, wsum);
                }
            }
            for (int c = 0; c < 3; ++c) out[c] = sum[c] / wsum;
        }
        write_pixel(a, p, out, valid);
    }
}

}  // namespace

int launch_denoise(const DenoiseArgs &d, void *scratch, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    const uint32_t P = d.w * d.h;   // <= BIH_DENOISE_MAX_PIXELS (the caller's check)
    float4 *pos = static_cast<float4 *>(scratch), *nrm = pos + P, *col[2] = {nrm + P, nrm + 2 * (size_t)P};
    SetupArgs s;
    for (int k = 0; k < 12; ++k) s.cam[k] = d.cam[k];
    s.w = d.w;
    s.h = d.h;
    s.pixels = P;
    s.radiance = d.radiance;
    s.depth = d.depth;
    s.normal = d.normal;
    s.pos = pos;
    s.nrm = nrm;
    s.col = col[0];
    const uint32_t sblocks = (P + kDT - 1) / kDT;
    hipLaunchKernelGGL(k_denoise_setup, dim3(sblocks < kMaxBlocks ? sblocks : kMaxBlocks), dim3(kDT), 0, st, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    PassArgs a;
    a.w = d.w;
    a.h = d.h;
    a.tiles_x = (d.w + kTW - 1) / kTW;
    // (tiles_x * tiles_y <= P / 256 + w / 32 + h / 8 + 1 < 2^31)
    a.ntiles = a.tiles_x * ((d.h + kTH - 1) / kTH);
    a.squarings = d.squarings;
    a.sigma_plane = d.sigma_plane;
    a.pos = pos;
    a.nrm = nrm;
    for (uint32_t i = 0; i < d.passes; ++i) {
        const bool last = i + 1 == d.passes;
        const float sc = ldexpf(d.sigma_colour, -(int)i);
        a.step = 1u << i;
        a.sc2 = sc * sc;
        a.cin = col[i & 1];
        a.cout = last ? nullptr : col[(i + 1) & 1];
        a.radiance_out = last ? d.radiance_out : nullptr;
        a.rgba_out = last ? d.rgba_out : nullptr;
        hipLaunchKernelGGL(k_denoise_pass, dim3(a.ntiles < kMaxBlocks ? a.ntiles : kMaxBlocks), dim3(kDT), 0, st, a);
        e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

}  // namespace bih
