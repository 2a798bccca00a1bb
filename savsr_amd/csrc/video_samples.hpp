// The sample rules the kernels in front of the network share (scene.hip, active.hip, pulldown.hip, deinterlace.hip, video.hip): each
// rule of the specifications (savsr_amd/scenes.py, active.py, pulldown.py) once, as a device helper.  Included after common.hpp (its
// f32x4), or after the host checks' stand-in for it (tools/host_check/hip_stub.h), where the plain-C++ branches are taken.
#pragma once
#include <cmath>
#include <cstdint>

namespace savsr {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));          // a 16-byte load

// |a.b0 - b.b0| + ... + |a.b3 - b.b3| + acc over the four bytes of a dword: one v_sad_u8
__device__ __forceinline__ uint32_t sad4(uint32_t a, uint32_t b, uint32_t acc) {
#if __has_builtin(__builtin_amdgcn_sad_u8)
    return __builtin_amdgcn_sad_u8(a, b, acc);
#else
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int d = (int)((a >> (8 * e)) & 255u) - (int)((b >> (8 * e)) & 255u);
        acc += (uint32_t)(d < 0 ? -d : d);
    }
    return acc;
#endif
}

// b0 + b1 + b2 + b3 + acc over the four bytes of a dword: v_sad_u8 against zero
__device__ __forceinline__ uint32_t sum4(uint32_t a, uint32_t acc) { return sad4(a, 0u, acc); }

__device__ __forceinline__ uint32_t absdiff(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }

// |a.lo - b.lo| + |a.hi - b.hi| + acc over the two 16-bit halves of a dword: one v_sad_u16
__device__ __forceinline__ uint32_t sad2(uint32_t a, uint32_t b, uint32_t acc) {
#if __has_builtin(__builtin_amdgcn_sad_u16)
    return __builtin_amdgcn_sad_u16(a, b, acc);
#else
    return acc + absdiff(a & 0xffffu, b & 0xffffu) + absdiff(a >> 16, b >> 16);
#endif
}

// The 8 most significant bits of a 16-bit sample of depth d (top = 2^d - 1, shift = d - 8): min(s, top) >> shift.  A sample above the
// depth's range counts as the largest one, so the detectors' scores keep the 8-bit scale at every depth.
__device__ __forceinline__ uint32_t msb8(uint32_t s, uint32_t top, int shift) { return min(s, top) >> shift; }

// msb8 of the two 16-bit samples of a dword, each in its half
__device__ __forceinline__ uint32_t msb8x2(uint32_t x, uint32_t top, int shift) {
    return msb8(x & 0xffffu, top, shift) | (msb8(x >> 16, top, shift) << 16);
}

// The uint8 output's value of a float (savsr_video_quantize_u8, tensor2img): clamp_(0, 1); (img * 255.0).round(): half to even;
// fmaxf(NaN, 0) = 0
__device__ __forceinline__ uint32_t quant_u8(float x) { return (uint32_t)rintf(fminf(fmaxf(x, 0.f), 1.f) * 255.0f); }

// quant_u8 of four floats, as the four bytes of a dword
__device__ __forceinline__ uint32_t quant4(const f32x4 v) {
    return quant_u8(v[0]) | (quant_u8(v[1]) << 8) | (quant_u8(v[2]) << 16) | (quant_u8(v[3]) << 24);
}

}  // namespace savsr
