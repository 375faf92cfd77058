// bih_primary.h -- what the kernels that restate a frame's primary samples
// share: the sample's ray direction (bih_gbuffer.hip casts it, bih_direct.hip
// needs it again for the hit point) and the hit triangle's normal (the
// G-buffer's `normal` plane, the direct-lighting facing test).
//
// Every f32 expression is the oracle's, in its order (-ffp-contract=off).
#pragma once
#include "bih_device.h"

namespace bih {
namespace dev {

// Direction of sample s of local pixel lp = (x, local row of global row y):
// draws 2s, 2s+1 of the pixel's frame (cudaRender :413-415) from its XORWOW
// state at the start of the frame (rng_in: 5 planes of P words, Weyl counter
// d_base), then Camera::GetRay's direction (Camera.cu:18-20).
__device__ __forceinline__ void primary_dir(const float *cam, const uint32_t *__restrict__ rng_in, uint64_t P,
                                            uint64_t lp, uint32_t d_base, uint32_t s, uint32_t x, uint32_t y,
                                            uint32_t w, uint32_t h, float *dir) {
    uint32_t v[5];
    for (int i = 0; i < 5; ++i) v[i] = rng_in[(uint64_t)i * P + lp];
    uint32_t d = d_base;
    float ru = 0.f, rv = 0.f;
    for (uint32_t k = 0; k <= s; ++k) {
        ru = xorwow_uniform(v, d);
        rv = xorwow_uniform(v, d);
    }
    const float fu = ((float)x + ru) / (float)w, fv = ((float)y + rv) / (float)h;
    for (int k = 0; k < 3; ++k) dir[k] = ((cam[3 + k] + fu * cam[6 + k]) + fv * cam[9 + k]) - cam[k];
}

// n = cross(e1, e2) (glm order) of a {v0, e1, e2} record, normalised: each op
// one rounded f32 op.
__device__ __forceinline__ void tri_normal(const float *__restrict__ tp, float *n) {
    const float e1x = tp[3], e1y = tp[4], e1z = tp[5];
    const float e2x = tp[6], e2y = tp[7], e2z = tp[8];
    const float nx = e1y * e2z - e2y * e1z;
    const float ny = e1z * e2x - e2z * e1x;
    const float nz = e1x * e2y - e2x * e1y;
    const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
    n[0] = nx / len;
    n[1] = ny / len;
    n[2] = nz / len;
}

}  // namespace dev
}  // namespace bih
