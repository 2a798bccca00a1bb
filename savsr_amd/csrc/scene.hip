// The scene-cut detector's scores (ABI 36): per pair of consecutive frames the sum of absolute differences of their 8-bit samples,
// an exact integer (savsr_amd/scenes.py `pair_sad` is the specification; the cut rule itself runs on the host in exact arithmetic,
// `cuts_from_sad`).  Elementwise and HBM-bound like video.hip's conversions: a pair reads both of its frames once.  Integer sums do
// not depend on their order, so the grid shape and the atomics change nothing in the result.
//
//   uint8 HWC frames   every byte                                   S = c * h * w
//   I420 frames        the Y plane only                             S = h * w
//   fp32 CHW frames    every value after savsr_video_quantize_u8's  S = c * h * w
//                      rule (clamp(0, 1) * 255.0f, rintf; NaN -> 0)
//   10- / 12-bit I420  the Y plane only, every 16-bit sample as its     S = h * w
//   (ABI 38)           8 most significant bits: min(s, 2^d - 1) >> (d - 8)
//   4:2:2 / 4:4:4      the Y plane only, as for I420 at the same depth: the Y   S = h * w
//   (ABI 39)           plane is the first h * w samples of a frame in every layout, so savsr_video_pair_sad_yuvp is host work only
//                      (another frame stride for the same kernels)
#include "common.hpp"
#include "video_samples.hpp"

#include <cstdint>

namespace savsr {
namespace {

constexpr int SAD_THREADS = 256;
constexpr int SAD_VEC_ITERS = 4;       // 16-byte chunks (or float4) per thread and frame in the vector forms
constexpr int SAD_ONE_ITERS = 16;      // samples per thread in the one-sample forms
constexpr int SAD_MAX_PAIRS_Y = 65535; // grid.y

// A workgroup's partial sum (a thread adds at most 64 samples of <= 255 each: far below 2^32) -> one 64-bit vector atomic on the pair's cell.
__device__ __forceinline__ void block_add(uint32_t acc, unsigned long long* cell) {
    __shared__ uint32_t part[SAD_THREADS / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
#pragma unroll
        for (int i = 0; i < SAD_THREADS / 64; ++i) s += part[i];
        if (s) atomicAdd(cell, s);
    }
}

// Frames `stride` bytes apart, the first `len` bytes of each compared; pair blockIdx.y = frames (k, k + 1).  VEC: frames and stride
// 16-byte aligned: 16-byte loads from both frames over len / 16 chunks, the len % 16 bytes left over by workgroup 0's first lanes.
// Otherwise a byte per lane and iteration (any base pointer, any size).
template <bool VEC>
__global__ __launch_bounds__(SAD_THREADS) void pair_sad_u8_kernel(const uint8_t* __restrict__ frames, long long stride, long long len,
                                                                  unsigned long long* __restrict__ sad) {
    const uint8_t* a = frames + (long long)blockIdx.y * stride;
    const uint8_t* b = a + stride;
    uint32_t acc = 0;
    if (VEC) {
        const long long nchunk = len >> 4;
        const long long c0 = (long long)blockIdx.x * (SAD_THREADS * SAD_VEC_ITERS) + threadIdx.x;
        u32x4 x[SAD_VEC_ITERS], y[SAD_VEC_ITERS];
#pragma unroll
        for (int it = 0; it < SAD_VEC_ITERS; ++it) {
            const long long ch = c0 + it * SAD_THREADS;
            x[it] = y[it] = u32x4{0u, 0u, 0u, 0u};
            if (ch < nchunk) {
                x[it] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a) + ch);
                y[it] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(b) + ch);
            }
        }
#pragma unroll
        for (int it = 0; it < SAD_VEC_ITERS; ++it) {
            acc = sad4(x[it].x, y[it].x, acc);
            acc = sad4(x[it].y, y[it].y, acc);
            acc = sad4(x[it].z, y[it].z, acc);
            acc = sad4(x[it].w, y[it].w, acc);
        }
        const long long t = (nchunk << 4) + threadIdx.x;
        if (blockIdx.x == 0 && threadIdx.x < 16 && t < len) acc += absdiff(a[t], b[t]);
    } else {
        const long long i0 = (long long)blockIdx.x * (SAD_THREADS * SAD_ONE_ITERS) + threadIdx.x;
#pragma unroll 4
        for (int it = 0; it < SAD_ONE_ITERS; ++it) {
            const long long i = i0 + it * SAD_THREADS;
            if (i < len) acc += absdiff(a[i], b[i]);
        }
    }
    block_add(acc, sad + blockIdx.y);
}

// fp32 frames of nfl values each, quantised value by value.  VEC: nfl % 4 == 0 and 16-byte aligned frames: a float4 from both frames
// per lane and iteration, four quantised bytes per v_sad_u8.
template <bool VEC>
__global__ __launch_bounds__(SAD_THREADS) void pair_sad_f32_kernel(const float* __restrict__ frames, long long nfl,
                                                                   unsigned long long* __restrict__ sad) {
    const float* a = frames + (long long)blockIdx.y * nfl;
    const float* b = a + nfl;
    uint32_t acc = 0;
    if (VEC) {
        const long long nchunk = nfl >> 2;
        const long long c0 = (long long)blockIdx.x * (SAD_THREADS * SAD_VEC_ITERS) + threadIdx.x;
        f32x4 x[SAD_VEC_ITERS], y[SAD_VEC_ITERS];
#pragma unroll
        for (int it = 0; it < SAD_VEC_ITERS; ++it) {
            const long long ch = c0 + it * SAD_THREADS;
            x[it] = y[it] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (ch < nchunk) {
                x[it] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a) + ch);
                y[it] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(b) + ch);
            }
        }
#pragma unroll
        for (int it = 0; it < SAD_VEC_ITERS; ++it) acc = sad4(quant4(x[it]), quant4(y[it]), acc);
    } else {
        const long long i0 = (long long)blockIdx.x * (SAD_THREADS * SAD_ONE_ITERS) + threadIdx.x;
#pragma unroll 4
        for (int it = 0; it < SAD_ONE_ITERS; ++it) {
            const long long i = i0 + it * SAD_THREADS;
            if (i < nfl) acc += absdiff(quant_u8(a[i]), quant_u8(b[i]));
        }
    }
    block_add(acc, sad + blockIdx.y);
}

// High-depth frames `stride` bytes apart, the first `len` 16-bit samples of each compared (the Y plane); pair blockIdx.y = frames (k, k + 1).
// VEC: frames and stride 16-byte aligned: 16-byte loads (8 samples) from both frames over len / 8 chunks, the len % 8 samples left over by
// workgroup 0's first lanes.  Otherwise a sample per lane and iteration (any 2-byte aligned base, any size).
template <bool VEC>
__global__ __launch_bounds__(SAD_THREADS) void pair_sad_u16_kernel(const uint8_t* __restrict__ frames, long long stride, long long len, uint32_t top,
                                                                   int shift, unsigned long long* __restrict__ sad) {
    const uint8_t* fa = frames + (long long)blockIdx.y * stride;
    const uint16_t* a = reinterpret_cast<const uint16_t*>(fa);
    const uint16_t* b = reinterpret_cast<const uint16_t*>(fa + stride);
    uint32_t acc = 0;
    if (VEC) {
        const long long nchunk = len >> 3;
        const long long c0 = (long long)blockIdx.x * (SAD_THREADS * SAD_VEC_ITERS) + threadIdx.x;
        u32x4 x[SAD_VEC_ITERS], y[SAD_VEC_ITERS];
#pragma unroll
        for (int it = 0; it < SAD_VEC_ITERS; ++it) {
            const long long ch = c0 + it * SAD_THREADS;
            x[it] = y[it] = u32x4{0u, 0u, 0u, 0u};
            if (ch < nchunk) {
                x[it] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a) + ch);
                y[it] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(b) + ch);
            }
        }
#pragma unroll
        for (int it = 0; it < SAD_VEC_ITERS; ++it) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = sad2(msb8x2(x[it][e], top, shift), msb8x2(y[it][e], top, shift), acc);
        }
        const long long t = (nchunk << 3) + threadIdx.x;
        if (blockIdx.x == 0 && threadIdx.x < 8 && t < len) acc += absdiff(msb8(a[t], top, shift), msb8(b[t], top, shift));
    } else {
        const long long i0 = (long long)blockIdx.x * (SAD_THREADS * SAD_ONE_ITERS) + threadIdx.x;
#pragma unroll 4
        for (int it = 0; it < SAD_ONE_ITERS; ++it) {
            const long long i = i0 + it * SAD_THREADS;
            if (i < len) acc += absdiff(msb8(a[i], top, shift), msb8(b[i], top, shift));
        }
    }
    block_add(acc, sad + blockIdx.y);
}

inline unsigned sad_blocks(long long units, int per_thread) {
    const long long per_block = (long long)SAD_THREADS * per_thread;
    const long long nb = (units + per_block - 1) / per_block;
    return (unsigned)(nb < 1 ? 1 : nb);
}

int zero_scores(int64_t* sad_out, int n_pairs, hipStream_t st, const char* what) {
    hipError_t e = hipMemsetAsync(sad_out, 0, sizeof(int64_t) * (size_t)n_pairs, st);
    if (e != hipSuccess) { set_error("%s: hipMemsetAsync failed: %s", what, hipGetErrorString(e)); return (int)e; }
    return 0;
}

// frames `stride` bytes apart, `len` bytes of each compared (the uint8 and the I420 entry)
int launch_bytes(const uint8_t* frames, int n_frames, long long stride, long long len, int64_t* sad_out, hipStream_t st, const char* what) {
    const int n_pairs = n_frames - 1;
    if (n_pairs == 0) return 0;
    if (int rc = zero_scores(sad_out, n_pairs, st, what)) return rc;
    const bool vec = stride % 16 == 0 && (reinterpret_cast<uintptr_t>(frames) & 15) == 0 && len >= 16;
    const unsigned gx = vec ? sad_blocks(len >> 4, SAD_VEC_ITERS) : sad_blocks(len, SAD_ONE_ITERS);
    for (int p0 = 0; p0 < n_pairs; p0 += SAD_MAX_PAIRS_Y) {
        const int np = n_pairs - p0 < SAD_MAX_PAIRS_Y ? n_pairs - p0 : SAD_MAX_PAIRS_Y;
        const uint8_t* f = frames + (long long)p0 * stride;
        unsigned long long* s = reinterpret_cast<unsigned long long*>(sad_out) + p0;
        if (vec) hipLaunchKernelGGL((pair_sad_u8_kernel<true>), dim3(gx, np), dim3(SAD_THREADS), 0, st, f, stride, len, s);
        else hipLaunchKernelGGL((pair_sad_u8_kernel<false>), dim3(gx, np), dim3(SAD_THREADS), 0, st, f, stride, len, s);
        if (int rc = check_launch("pair_sad_u8_kernel")) return rc;
    }
    return 0;
}

// high-depth frames `stride` bytes apart, the first `len` 16-bit samples of each compared (the 10- / 12-bit entries)
int launch_words(const uint8_t* frames, int n_frames, long long stride, long long len, int depth, int64_t* sad_out, hipStream_t st, const char* what) {
    const int n_pairs = n_frames - 1;
    if (n_pairs == 0) return 0;
    if (int rc = zero_scores(sad_out, n_pairs, st, what)) return rc;
    const bool vec = stride % 16 == 0 && (reinterpret_cast<uintptr_t>(frames) & 15) == 0 && len >= 8;
    const unsigned gx = vec ? sad_blocks(len >> 3, SAD_VEC_ITERS) : sad_blocks(len, SAD_ONE_ITERS);
    const uint32_t top = (1u << depth) - 1u;
    for (int p0 = 0; p0 < n_pairs; p0 += SAD_MAX_PAIRS_Y) {
        const int np = n_pairs - p0 < SAD_MAX_PAIRS_Y ? n_pairs - p0 : SAD_MAX_PAIRS_Y;
        const uint8_t* f = frames + (long long)p0 * stride;
        unsigned long long* s = reinterpret_cast<unsigned long long*>(sad_out) + p0;
        if (vec) hipLaunchKernelGGL((pair_sad_u16_kernel<true>), dim3(gx, np), dim3(SAD_THREADS), 0, st, f, stride, len, top, depth - 8, s);
        else hipLaunchKernelGGL((pair_sad_u16_kernel<false>), dim3(gx, np), dim3(SAD_THREADS), 0, st, f, stride, len, top, depth - 8, s);
        if (int rc = check_launch("pair_sad_u16_kernel")) return rc;
    }
    return 0;
}

// Planar frames of any chroma layout (SAVSR_CHROMA_*) and depth (8, 10, 12): the Y plane is the first h * w samples of a frame of
// h * w + 2 * ch * cw samples, so the three planar entries are this one choice of stride and length for the launches above.
int launch_planar(const uint8_t* frames, int n_frames, int h, int w, int depth, int chroma, int64_t* sad_out, void* stream, const char* what) {
    const long long ch = chroma == SAVSR_CHROMA_420 ? (h + 1) / 2 : h, cw = chroma == SAVSR_CHROMA_444 ? w : (w + 1) / 2;
    const long long len = (long long)h * w, samples = len + 2 * ch * cw;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (depth == 8) return launch_bytes(frames, n_frames, samples, len, sad_out, st, what);
    return launch_words(frames, n_frames, 2 * samples, len, depth, sad_out, st, what);
}

}  // namespace
}  // namespace savsr

using namespace savsr;

extern "C" int savsr_video_pair_sad_u8(const uint8_t* frames, int n_frames, int c, int h, int w, int64_t* sad_out, void* stream) {
    if (!frames || (!sad_out && n_frames > 1)) return fail_arg("video_pair_sad_u8: null pointer");
    if (c < 1 || c > 3 || h < 1 || w < 1 || n_frames < 1) return fail_arg("video_pair_sad_u8: c in 1 .. 3, h, w, n_frames >= 1");
    if (reinterpret_cast<uintptr_t>(sad_out) & 7) return fail_arg("video_pair_sad_u8: sad_out must be 8-byte aligned");
    const long long len = (long long)c * h * w;
    return launch_bytes(frames, n_frames, len, len, sad_out, static_cast<hipStream_t>(stream), "video_pair_sad_u8");
}

extern "C" int savsr_video_pair_sad_i420(const uint8_t* frames, int n_frames, int h, int w, int64_t* sad_out, void* stream) {
    if (!frames || (!sad_out && n_frames > 1)) return fail_arg("video_pair_sad_i420: null pointer");
    if (h < 1 || w < 1 || n_frames < 1) return fail_arg("video_pair_sad_i420: h, w, n_frames >= 1");
    if (reinterpret_cast<uintptr_t>(sad_out) & 7) return fail_arg("video_pair_sad_i420: sad_out must be 8-byte aligned");
    return launch_planar(frames, n_frames, h, w, 8, SAVSR_CHROMA_420, sad_out, stream, "video_pair_sad_i420");
}

extern "C" int savsr_video_pair_sad_f32(const float* frames, int n_frames, int c, int h, int w, int64_t* sad_out, void* stream) {
    if (!frames || (!sad_out && n_frames > 1)) return fail_arg("video_pair_sad_f32: null pointer");
    if (c < 1 || c > 3 || h < 1 || w < 1 || n_frames < 1) return fail_arg("video_pair_sad_f32: c in 1 .. 3, h, w, n_frames >= 1");
    if (reinterpret_cast<uintptr_t>(frames) & 3) return fail_arg("video_pair_sad_f32: frames must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(sad_out) & 7) return fail_arg("video_pair_sad_f32: sad_out must be 8-byte aligned");
    const int n_pairs = n_frames - 1;
    if (n_pairs == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = zero_scores(sad_out, n_pairs, st, "video_pair_sad_f32")) return rc;
    const long long nfl = (long long)c * h * w;
    const bool vec = nfl % 4 == 0 && (reinterpret_cast<uintptr_t>(frames) & 15) == 0;
    const unsigned gx = vec ? sad_blocks(nfl >> 2, SAD_VEC_ITERS) : sad_blocks(nfl, SAD_ONE_ITERS);
    for (int p0 = 0; p0 < n_pairs; p0 += SAD_MAX_PAIRS_Y) {
        const int np = n_pairs - p0 < SAD_MAX_PAIRS_Y ? n_pairs - p0 : SAD_MAX_PAIRS_Y;
        const float* f = frames + (long long)p0 * nfl;
        unsigned long long* s = reinterpret_cast<unsigned long long*>(sad_out) + p0;
        if (vec) hipLaunchKernelGGL((pair_sad_f32_kernel<true>), dim3(gx, np), dim3(SAD_THREADS), 0, st, f, nfl, s);
        else hipLaunchKernelGGL((pair_sad_f32_kernel<false>), dim3(gx, np), dim3(SAD_THREADS), 0, st, f, nfl, s);
        if (int rc = check_launch("pair_sad_f32_kernel")) return rc;
    }
    return 0;
}

// ABI 38: 10- / 12-bit I420 frames (little-endian 16-bit samples): the Y plane's samples as their 8 most significant bits, so the scores
// have savsr_video_pair_sad_i420's scale.
extern "C" int savsr_video_pair_sad_i420_16(const uint8_t* frames, int n_frames, int h, int w, int depth, int64_t* sad_out, void* stream) {
    if (!frames || (!sad_out && n_frames > 1)) return fail_arg("video_pair_sad_i420_16: null pointer");
    if (h < 1 || w < 1 || n_frames < 1) return fail_arg("video_pair_sad_i420_16: h, w, n_frames >= 1");
    if (depth != 10 && depth != 12) return fail_arg("video_pair_sad_i420_16: depth 10 or 12 (8 bits: savsr_video_pair_sad_i420)");
    if (reinterpret_cast<uintptr_t>(frames) & 1) return fail_arg("video_pair_sad_i420_16: frames must be 2-byte aligned (16-bit samples)");
    if (reinterpret_cast<uintptr_t>(sad_out) & 7) return fail_arg("video_pair_sad_i420_16: sad_out must be 8-byte aligned");
    return launch_planar(frames, n_frames, h, w, depth, SAVSR_CHROMA_420, sad_out, stream, "video_pair_sad_i420_16");
}

// ABI 39: frames of any chroma layout (SAVSR_CHROMA_*) and depth (8, 10, 12): the Y plane, h * w samples at the start of a frame of
// h * w + 2 * ch * cw samples.  Host work only: the kernels above with the layout's frame stride (`launch_planar`, which the two I420
// entries above reach as well after their own checks).
extern "C" int savsr_video_pair_sad_yuvp(const uint8_t* frames, int n_frames, int h, int w, int depth, int chroma, int64_t* sad_out, void* stream) {
    if (chroma < SAVSR_CHROMA_420 || chroma > SAVSR_CHROMA_444) return fail_arg("video_pair_sad_yuvp: chroma 0 (4:2:0), 1 (4:2:2) or 2 (4:4:4)");
    if (depth != 8 && depth != 10 && depth != 12) return fail_arg("video_pair_sad_yuvp: depth 8, 10 or 12");
    if (!frames || (!sad_out && n_frames > 1)) return fail_arg("video_pair_sad_yuvp: null pointer");
    if (h < 1 || w < 1 || n_frames < 1) return fail_arg("video_pair_sad_yuvp: h, w, n_frames >= 1");
    if (depth != 8 && (reinterpret_cast<uintptr_t>(frames) & 1)) return fail_arg("video_pair_sad_yuvp: frames must be 2-byte aligned (16-bit samples)");
    if (reinterpret_cast<uintptr_t>(sad_out) & 7) return fail_arg("video_pair_sad_yuvp: sad_out must be 8-byte aligned");
    return launch_planar(frames, n_frames, h, w, depth, chroma, sad_out, stream, "video_pair_sad_yuvp");
}
