// bih_bounce.h -- the bounce direction of a primary-hit sample
// (bih_render_indirect*, include/bih.h): ONE
// expression for the bounce walk of bih_direct.hip (k_path_bounce) and for
// bih_bounce_sample on the host, as bih_area.h is for the panels.  The
// direction comes from the area lights' counter-based hash with the slot
// kBounceSlot, which no light index takes: no XORWOW draw of any frame moves.
// Level k of a path (bih_render_path*, section 4.5.7; k_path_bounce,
// bih_path_sample) takes the slot kBounceSlot + (k - 1), wrapping.
// B = n + w, w a point of the unit sphere: cosine-distributed about a unit n.
// No library trigonometry (host and device sinf differ): the circle's point is
// a quadrant and a degree-9 Taylor sine of (pi/2)x, every f32 operation
// separately rounded (-ffp-contract=off on both sides), so host and device
// agree on every bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "bih_area.h"

namespace bih {

constexpr uint32_t kBounceSlot = 0x80000000u;   // BIH_BOUNCE_SLOT

// sin((pi/2) x) on [0, 1]: the Taylor terms' f32 constants (+-(pi/2)^k / k!), Horner in x*x.
BIH_AREA_FN float bounce_sin(float x) {
    const float x2 = x * x;
    return ((((0x1.507834p-13f * x2 + -0x1.32d2ccp-8f) * x2 + 0x1.466bc6p-4f) * x2 + -0x1.4abbcep-1f) * x2 +
            0x1.921fb6p+0f) * x;
}

// B of sample `fs` = frame*spp + s (wrapping) of global pixel gp = y*w + x for
// the normal n; hseed = area_seed_hash(seed); slot: the hash's last mix.
BIH_AREA_FN void bounce_dir(uint32_t hseed, uint32_t gp, uint32_t fs, uint32_t slot, const float *n, float *d) {
    uint32_t h = area_mix(hseed ^ gp);
    h = area_mix(h ^ fs);
    h = area_mix(h ^ slot);
    const uint32_t ha = area_mix(h + 0x9E3779B9u);
    const uint32_t hb = area_mix(h + 0x3C6EF372u);
    const float a = (float)(ha >> 8) * 0x1p-24f;   // 24 bits: exact, in [0, 1)
    const float b = (float)(hb >> 8) * 0x1p-24f;
    const float z = 1.0f - 2.0f * a;
    const float r = sqrtf(fmaxf(0.0f, 1.0f - z * z));
    const float b4 = 4.0f * b;
    const int q = (int)b4;                         // the quadrant, 0..3
    const float f = b4 - (float)q;                 // exact
    const float sn = bounce_sin(f), cs = bounce_sin(1.0f - f);
    const float cx = q == 0 ? cs : (q == 1 ? -sn : (q == 2 ? -cs : sn));
    const float sx = q == 0 ? sn : (q == 1 ? cs : (q == 2 ? -sn : -cs));
    d[0] = n[0] + r * cx;
    d[1] = n[1] + r * sx;
    d[2] = n[2] + z;
}

}  // namespace bih
