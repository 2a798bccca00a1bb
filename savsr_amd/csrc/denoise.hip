// Temporal noise reduction in front of the network (ABI 50): N frames -> N frames, ffmpeg atadenoise's serial rule in 32-bit integers
// (savsr_amd/denoise.py `denoise_matrix` is the specification, sample by sample; the kernels equal it bit for bit).  Output sample x of
// frame t is the rounded mean of x and the taps taken by two independent walks over the same sample of frames t - 1, t - 2, ... and
// t + 1, t + 2, ...: a walk takes the tap at distance d while |x - tap| <= A and the walk's sum of differences stays <= B, and ends at
// the first tap that fails, after `radius` taps or where the resident frames end.
//
//   _u8    matrices of rows x row_bytes bytes (a plane, or the h x (w * c) bytes of packed frames: no neighbour in space is read)
//   _u16   matrices of rows x cols little-endian 16-bit samples, every sample read as min(s, 2^depth - 1)
//
// One launch per call, grid = (tile of the matrix, output frame).  The rule knows no rows: a matrix is a run of rows * row_bytes bytes.
// Vector form (the plane pointers and frame strides of both sides and the plane's bytes multiples of 16): a lane owns 16 bytes, 16 or 8
// samples, and keeps per sample the two walks' accumulators and one word with the sum (bits 0 .. 19, below 2^18 at 12 bits) and the
// tap count (bits 20 ..).  A walk that has ended has its accumulator at DN_DEAD, so "alive" is not a bit of its own: every later
// comparison against B fails.  The trip count is uniform: distance d loads both neighbour frames' chunks together, the pair of distance
// d + 1 is issued before the pair of distance d is used, and a side is left once no sample of the wave is alive on it (a wave vote), the
// loop once both are.  One-sample form (any pointer, stride and size): a lane owns one sample and walks until its own taps fail.
// The division by k = 1 .. 33 is a multiply by ceil(2^32 / k) and the high word: exact while sum * (k - 1) < 2^32, and the sums stay
// below 33 * 4095 + 16.
//
// Cache policy: every line is read by up to 2 * radius + 1 output frames, and the frames around an output frame (nine SD frames at
// radius 4: 5.6 MB) fit the L2s and the memory-side cache many times over, so the loads are plain (they may hit L1 and keep their lines
// in L2 for the next frames' workgroups; `nt` / `sc1` loads would bypass L1 and gain nothing) and so are the stores (a plain store keeps
// its line in L2, which costs the reads nothing at these sizes; write-through stores are for hand-offs inside a launch).
#include "common.hpp"
#include "video_samples.hpp"
#include "field_matrix.hpp"

#include <cstdint>

namespace savsr {
namespace {

constexpr int DN_THREADS = 256;
constexpr int DN_MAX_RADIUS = 16;
constexpr uint32_t DN_DEAD = 1u << 30;          // the accumulator of a walk that has ended: above every B, and + a difference still fits
constexpr int DN_COUNT_SHIFT = 20;              // sum | count << 20 in one word

struct DnJob {
    const uint8_t* src;          // the matrix of resident frame 0
    uint8_t* dst;                // the matrix of output frame 0
    long long stride, dst_stride;
    long long units;             // 16-byte chunks (vector form) or samples (one-sample form) of a matrix
    int n_frames, from, radius;
    uint32_t top, A, B;          // 2^depth - 1; the thresholds in sample units
};

struct DnRecip {
    uint32_t m[2 * DN_MAX_RADIUS + 2];
    constexpr DnRecip() : m() {
        for (int k = 2; k < 2 * DN_MAX_RADIUS + 2; ++k) m[k] = (uint32_t)(((1ull << 32) + k - 1) / k);
    }
};

// (sum + (k >> 1)) / k of the word sum | k << 20
__device__ __forceinline__ uint32_t mean_of(uint32_t sk) {
    constexpr DnRecip recip{};
    const uint32_t k = sk >> DN_COUNT_SHIFT, n = (sk & ((1u << DN_COUNT_SHIFT) - 1u)) + (k >> 1);
    return k == 1 ? n : (uint32_t)(((unsigned long long)n * recip.m[k]) >> 32);
}

// One step of a walk: tap v against x.  true while the walk goes on.
__device__ __forceinline__ bool walk(uint32_t x, uint32_t v, uint32_t& acc, uint32_t& sk, uint32_t A, uint32_t B) {
    const uint32_t diff = absdiff(x, v), sum = acc + diff;
    const bool take = diff <= A && sum <= B;          // (acc == DN_DEAD after the end: sum > B)
    acc = take ? sum : DN_DEAD;
    sk += take ? (v | (1u << DN_COUNT_SHIFT)) : 0u;
    return take;
}

__device__ __forceinline__ bool wave_any(bool p) {
#ifdef SAVSR_HOST_CHECK          // the host check runs one thread at a time
    return p;
#else
    return __any(p);
#endif
}

// Sample i of a chunk: a constant bit field once the loops are unrolled.
template <int BYTES>
__device__ __forceinline__ uint32_t sample_of(const u32x4& w, int i, uint32_t top) {
    if constexpr (BYTES == 1) return (w[i >> 2] >> (8 * (i & 3))) & 255u;
    else return min((w[i >> 1] >> (16 * (i & 1))) & 0xffffu, top);
}

__device__ __forceinline__ u32x4 chunk_at(const uint8_t* mat, long long chunk) { return *(reinterpret_cast<const u32x4*>(mat) + chunk); }

// Vector form: lane = one 16-byte chunk of output frame blockIdx.y.
template <int BYTES>
__global__ __launch_bounds__(DN_THREADS) void denoise_vec_kernel(DnJob jb) {
    constexpr int SPL = 16 / BYTES;          // samples of a chunk
    const long long chunk = (long long)blockIdx.x * DN_THREADS + threadIdx.x;
    if (chunk >= jb.units) return;          // (a lane that left takes no part in the votes)
    const int t = jb.from + (int)blockIdx.y;
    const uint8_t* cur = jb.src + (long long)t * jb.stride;
    const u32x4 xv = chunk_at(cur, chunk);
    bool back = t >= 1, fwd = t + 1 < jb.n_frames;          // the walks some sample of the wave is still on
    u32x4 vb = xv, vf = xv;
    if (back) vb = chunk_at(cur - jb.stride, chunk);
    if (fwd) vf = chunk_at(cur + jb.stride, chunk);
    uint32_t x[SPL], ab[SPL], af[SPL], sk[SPL];
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
        x[i] = sample_of<BYTES>(xv, i, jb.top);
        ab[i] = af[i] = 0u;
        sk[i] = x[i] | (1u << DN_COUNT_SHIFT);
    }
    for (int d = 1; back || fwd; ++d) {
        // the pair of the next distance, where the frames exist (asked for before this distance's votes: at most one pair too many)
        const bool more = d < jb.radius, nb = back && more && t - d >= 1, nf = fwd && more && t + d + 1 < jb.n_frames;
        u32x4 pb = vb, pf = vf;
        if (nb) pb = chunk_at(cur - (long long)(d + 1) * jb.stride, chunk);
        if (nf) pf = chunk_at(cur + (long long)(d + 1) * jb.stride, chunk);
        if (back) {
            bool alive = false;
#pragma unroll
            for (int i = 0; i < SPL; ++i) alive |= walk(x[i], sample_of<BYTES>(vb, i, jb.top), ab[i], sk[i], jb.A, jb.B);
            back = nb && wave_any(alive);
        }
        if (fwd) {
            bool alive = false;
#pragma unroll
            for (int i = 0; i < SPL; ++i) alive |= walk(x[i], sample_of<BYTES>(vf, i, jb.top), af[i], sk[i], jb.A, jb.B);
            fwd = nf && wave_any(alive);
        }
        vb = pb;
        vf = pf;
    }
    uint32_t res[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
        const uint32_t v = mean_of(sk[i]);
        if constexpr (BYTES == 1) res[i >> 2] |= v << (8 * (i & 3));
        else res[i >> 1] |= v << (16 * (i & 1));
    }
    *(reinterpret_cast<u32x4*>(jb.dst + (long long)blockIdx.y * jb.dst_stride) + chunk) = u32x4{res[0], res[1], res[2], res[3]};
}

template <int BYTES>
__device__ __forceinline__ uint32_t one_at(const uint8_t* mat, long long s, uint32_t top) {
    if constexpr (BYTES == 1) return mat[s];
    else return min((uint32_t)reinterpret_cast<const uint16_t*>(mat)[s], top);
}

// One-sample form: lane = one sample of output frame blockIdx.y.
template <int BYTES>
__global__ __launch_bounds__(DN_THREADS) void denoise_one_kernel(DnJob jb) {
    const long long s = (long long)blockIdx.x * DN_THREADS + threadIdx.x;
    if (s >= jb.units) return;
    const int t = jb.from + (int)blockIdx.y;
    const uint8_t* cur = jb.src + (long long)t * jb.stride;
    const uint32_t x = one_at<BYTES>(cur, s, jb.top);
    uint32_t sk = x | (1u << DN_COUNT_SHIFT), acc = 0u;
    for (int d = 1; d <= jb.radius && t - d >= 0; ++d)
        if (!walk(x, one_at<BYTES>(cur - (long long)d * jb.stride, s, jb.top), acc, sk, jb.A, jb.B)) break;
    acc = 0u;
    for (int d = 1; d <= jb.radius && t + d < jb.n_frames; ++d)
        if (!walk(x, one_at<BYTES>(cur + (long long)d * jb.stride, s, jb.top), acc, sk, jb.A, jb.B)) break;
    uint8_t* out = jb.dst + (long long)blockIdx.y * jb.dst_stride;
    if constexpr (BYTES == 1) out[s] = (uint8_t)mean_of(sk);
    else reinterpret_cast<uint16_t*>(out)[s] = (uint16_t)mean_of(sk);
}

// The body of the two entries.  width: row_bytes (_u8) or cols (_u16); thr_a, thr_b: 8-bit code units, shifted to the depth here.
template <int BYTES>
int denoise(const char* who, const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int width, int depth, int radius,
            int thr_a, int thr_b, int from, int to, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset, void* stream) {
    constexpr MatrixRule rule{1, 0, nullptr, "the range needs 0 <= from < to <= n_frames", false};
    const int64_t row_bytes = (int64_t)BYTES * width;
    const char* why = check_matrix(rule, frames && out ? frames : nullptr, n_frames, frame_bytes, plane_offset, rows, row_bytes, 0, from, to, out_plane_offset);
    if (!why) why = check_out_plane(out_frame_bytes, out_plane_offset, rows, row_bytes);
    if (why) return refuse(who, why);
    if (BYTES == 2)
        if (int rc = check_samples16(who, depth, frames, frame_bytes, plane_offset, true, out, out_frame_bytes, out_plane_offset)) return rc;
    if (radius < 1 || radius > DN_MAX_RADIUS) return refuse(who, "radius 1 .. 16");
    if (thr_a < 0 || thr_a > thr_b || thr_b > 255) return refuse(who, "thresholds 0 <= thr_a <= thr_b <= 255 (8-bit code units)");
    if (out < frames + (int64_t)n_frames * frame_bytes && frames < out + (int64_t)(to - from) * out_frame_bytes)
        return refuse(who, "the source frames and the output overlap");
    const long long bytes = (long long)rows * row_bytes;
    const uint8_t* src = frames + plane_offset;
    uint8_t* dst = out + out_plane_offset;
    const bool vec = aligned16(src, frame_bytes, bytes) && aligned16(dst, out_frame_bytes, 0);
    const DnJob jb{src, dst, frame_bytes, out_frame_bytes, vec ? bytes / 16 : bytes / BYTES, n_frames, from, radius,
                   (1u << depth) - 1u, (uint32_t)thr_a << (depth - 8), (uint32_t)thr_b << (depth - 8)};
    const unsigned gx = blocks(jb.units, DN_THREADS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return for_frame_chunks(to - from, FM_MAX_FRAMES, [&](int f0, int nf) {
        const dim3 grid(gx, (unsigned)nf), block(DN_THREADS);
        DnJob part = jb;
        part.from = jb.from + f0;
        part.dst = jb.dst + (long long)f0 * jb.dst_stride;
        if (vec) hipLaunchKernelGGL((denoise_vec_kernel<BYTES>), grid, block, 0, st, part);
        else hipLaunchKernelGGL((denoise_one_kernel<BYTES>), grid, block, 0, st, part);
        return check_launch(vec ? "denoise_vec_kernel" : "denoise_one_kernel");
    });
}

}  // namespace
}  // namespace savsr

using namespace savsr;

extern "C" int savsr_video_denoise_u8(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int row_bytes, int radius,
                                      int thr_a, int thr_b, int from, int to, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset,
                                      void* stream) {
    return denoise<1>("video_denoise_u8", frames, n_frames, frame_bytes, plane_offset, rows, row_bytes, 8, radius, thr_a, thr_b, from, to, out, out_frame_bytes,
                      out_plane_offset, stream);
}

extern "C" int savsr_video_denoise_u16(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int depth,
                                       int radius, int thr_a, int thr_b, int from, int to, uint8_t* out, int64_t out_frame_bytes,
                                       int64_t out_plane_offset, void* stream) {
    return denoise<2>("video_denoise_u16", frames, n_frames, frame_bytes, plane_offset, rows, cols, depth, radius, thr_a, thr_b, from, to, out, out_frame_bytes,
                      out_plane_offset, stream);
}
