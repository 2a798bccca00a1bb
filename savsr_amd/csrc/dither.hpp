// Ordered dither of the quantisers behind the network (video.hip, yuv.hip, luma.hip; the `_d` entries of ABI 47): the threshold and the
// per-sample rule of the specification (savsr_amd/dither.py), once.  Where a quantiser computes rintf(t) its dithered instantiation
// computes floorf(t + theta(y, x)), t the float32 value in output code units and (y, x) the sample's coordinates in its own plane.
// Plain C++ apart from the function qualifiers: tools/check_dither_host.py compiles it into a host program and compares it with
// dither.py at every position and over a sweep of t.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIP__)
#define SAVSR_DITHER_FN __host__ __device__ __forceinline__
#else
#define SAVSR_DITHER_FN inline
#endif

namespace savsr {

// The 16 x 16 Bayer index matrix in closed form, B[y & 15][x & 15] = sum over b = 0 .. 3 of 4^(3 - b) (2 (((x ^ y) >> b) & 1) + ((y >> b) & 1)):
// every value 0 .. 255 once.  Integer operations on the coordinates, so no table is indexed per lane (a by-value table would go to
// private memory).
SAVSR_DITHER_FN uint32_t dither_bayer16(uint32_t y, uint32_t x) {
    const uint32_t a = x ^ y;
    uint32_t r = 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b) r |= (2u * ((a >> b) & 1u) + ((y >> b) & 1u)) << (2 * (3 - b));
    return r;
}

// theta(y, x) = (B + 0.5) / 256 as (2 B + 1) / 512: the integer is at most 511 and the power of two exact in float32, whatever the
// contraction; inside (0, 1).
SAVSR_DITHER_FN float dither_theta_of(uint32_t b) { return (float)(2u * b + 1u) * 0.001953125f; }
SAVSR_DITHER_FN float dither_theta(uint32_t y, uint32_t x) { return dither_theta_of(dither_bayer16(y, x)); }

// The thresholds of 4 consecutive samples (y, x0 .. x0 + 3), x0 a multiple of 4: what the vector forms own.  x0 + e differs from x0 in
// its two low bits alone, which reach B through the digits b = 0 and b = 1 of x ^ y: bits 7 and 5.  So B(y, x0 + e) is B(y, x0) with
// those two bits flipped where e has a bit set: one matrix entry and an exclusive-or per sample.
SAVSR_DITHER_FN void dither_theta4(uint32_t y, uint32_t x0, float (&th)[4]) {
    const uint32_t b0 = dither_bayer16(y, x0);
#pragma unroll
    for (uint32_t e = 0; e < 4; ++e) th[e] = dither_theta_of(b0 ^ (((e & 1u) << 7) | ((e & 2u) << 4)));
}

// floor(t + theta): ONE float32 addition, round to nearest even, never contracted with the multiply that made t -- the pragma holds for
// this block wherever it is inlined (the addition carries no contraction flag, so no fused multiply-add is formed from it).
SAVSR_DITHER_FN float dither_add_floor(float t, float theta) {
#pragma clang fp contract(off)
    const float s = t + theta;
    return floorf(s);
}

// The rule at a sample: what stands in rintf(t)'s place.
SAVSR_DITHER_FN float dither_floor(float t, uint32_t y, uint32_t x) { return dither_add_floor(t, dither_theta(y, x)); }

// (y, x) = (p / W, p % W) of linear sample index p in a plane W wide, for the kernels that index samples linearly: once per thread, and
// without a divide wherever p fits 32 bits (every real frame) -- the host makes the multiplier of the division by the invariant W once
// per launch (Granlund and Montgomery's round-up form: with l = ceil(log2 W), mul = floor(2^32 (2^l - W) / W) + 1 and t = mulhi(mul, p),
// p / W = (t + ((p - t) >> min(l, 1))) >> max(l - 1, 0) for every 32-bit p); the 64-bit division otherwise.
struct DitherDiv { uint32_t w, mul, sh1, sh2; };
inline DitherDiv dither_div(int W) {
    uint32_t l = 0;
    while ((1ull << l) < (unsigned long long)W) ++l;
    const unsigned long long m = ((1ull << 32) * ((1ull << l) - (unsigned long long)W)) / (unsigned long long)W + 1ull;
    return DitherDiv{(uint32_t)W, (uint32_t)m, l < 1u ? l : 1u, l > 0u ? l - 1u : 0u};
}
SAVSR_DITHER_FN void dither_row_col(long long p, const DitherDiv& d, uint32_t& y, uint32_t& x) {
    if (p <= 0xffffffffLL) {
        const uint32_t n = (uint32_t)p;
        const uint32_t t = (uint32_t)(((unsigned long long)d.mul * n) >> 32);
        y = (t + ((n - t) >> d.sh1)) >> d.sh2;
        x = n - y * d.w;
    } else {
        y = (uint32_t)(p / d.w);
        x = (uint32_t)(p % d.w);
    }
}

// The packed-RGB and luma quantisers' dithered value of a float: clamp to [0, 1] (fmaxf(NaN, 0) = 0), x mul (255 for packed RGB,
// 255 * 2^(d - 8) for luma) as a product of its own, then the rule with the pixel's threshold.
SAVSR_DITHER_FN uint32_t dither_quant_unit(float v, float mul, float theta) {
#pragma clang fp contract(off)
    const float t = fminf(fmaxf(v, 0.f), 1.f) * mul;
    return (uint32_t)dither_add_floor(t, theta);
}

}  // namespace savsr
