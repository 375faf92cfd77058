// bih_pixdiv.h -- a pixel coordinate's division by the image size without a
// division sequence: uf = (x + ru) / w, vf = (y + rv) / h of the primary ray
// (CUDAKernels.cu:414-415), for k_render_bins (bih_render.hip) and the host
// entry the tests call (bih_pixel_divide, bih_capi.cpp).
//
// With y = fl(1 / d), the correctly rounded reciprocal formed once per wave:
//   q = fl(n * y);  r = fma(-q, d, n);  result = fma(r, y, q)
// equals fl(n / d), the IEEE quotient, for every integer d in
// [1, kPixelDivideMax] and every positive normal n whose quotient is far from
// underflow (n = fl(x + ru) >= 2^-33).  DESIGN.md section 4.14 has the proof:
// r is exact, the fma's unrounded value is n/d + (n/d - q) e1 with
// |e1| <= 2^-24 the reciprocal's relative error, less than 2^-22 ulp from
// n/d, and n/d with integer d is at least ulp / (2 d) from every rounding
// midpoint.  tests/test_pixel_divide.py checks it against numpy's division.
// Both fma are explicit: the sources are compiled -ffp-contract=off.
#pragma once
#include <cstdint>

namespace bih {

// the largest image side that takes the reciprocal form; a larger one keeps
// the division (the proof holds to 2^21; this is the range the test covers)
constexpr uint32_t kPixelDivideMax = 65536u;

__host__ __device__ __forceinline__ float pixel_divide(float n, float d, float y) {
    const float q = n * y;
    const float r = __builtin_fmaf(-q, d, n);
    return __builtin_fmaf(r, y, q);
}

}  // namespace bih
