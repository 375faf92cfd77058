// bih_area.h -- the sample point of an area light (bih_render_area_lights*,
// include/bih.h): ONE expression for the setup, shadow
// and resolve kernels of bih_direct.hip and for bih_area_light_sample on the
// host, as lamp_dir is for a lamp's L.  The point comes from a counter-based
// integer hash of (seed, global pixel, frame*spp + s, light), not from the
// pixel's XORWOW subsequence: no draw of any frame moves.  u32 arithmetic
// wraps and the two floats are exact, so host and device agree on every bit
// (every f32 operation separately rounded: -ffp-contract=off on both sides).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BIH_AREA_FN __host__ __device__ __forceinline__
#else
#define BIH_AREA_FN inline
#endif

namespace bih {

BIH_AREA_FN uint32_t area_mix(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// The hash's uniform prefix, the two steps over the seed (done once per call, on the host).
BIH_AREA_FN uint32_t area_seed_hash(uint64_t seed) {
    const uint32_t h = area_mix((uint32_t)seed);
    return area_mix(h ^ (uint32_t)(seed >> 32));
}

// Q of area light j {corner c, edges u, v} for sample `fs` = frame*spp + s
// (wrapping) of global pixel gp = y*w + x; hseed = area_seed_hash(seed).
BIH_AREA_FN void area_point(uint32_t hseed, uint32_t gp, uint32_t fs, uint32_t j, const float *c, const float *u,
                            const float *v, float *q) {
    uint32_t h = area_mix(hseed ^ gp);
    h = area_mix(h ^ fs);
    h = area_mix(h ^ j);
    const uint32_t ha = area_mix(h + 0x9E3779B9u);
    const uint32_t hb = area_mix(h + 0x3C6EF372u);
    const float a = (float)(ha >> 8) * 0x1p-24f;   // 24 bits: exact, in [0, 1)
    const float b = (float)(hb >> 8) * 0x1p-24f;
    for (int k = 0; k < 3; ++k) q[k] = (c[k] + a * u[k]) + b * v[k];
}

}  // namespace bih
