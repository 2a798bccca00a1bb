// Scan detection (ABI 46): the field statistics that tell progressive, interlaced and telecined video apart (savsr_amd/scan.py
// `field_stats` is the specification; the kernels equal it bit for bit, the decision is made on the host in exact arithmetic).
//
// Frame n of the range gets eight sums, out[8 n + 2 k + q], q the parity of the rows summed over:
//   k = 0, 1, 2   comb against row y of frame max(n - 1, 0), of frame min(n + 1, n_frames - 1), of frame n itself: the sum over the rows y
//                 of parity q, 1 <= y <= rows - 2, and all x of |a - b| + |c - b| - |a - c|, a = F[n][y - 1], c = F[n][y + 1], b the sample
//                 at (y, x) of that frame: pulldown.hip's measure
//   k = 3         the sum over ALL rows y of parity q and all x of |F[n][y] - F[max(n - 1, 0)][y]|
// Never negative, and exact integers in any order, so the grid shape and the atomics change nothing in the result.
//
//   _u8    matrices of rows x row_bytes bytes (a plane, or the h x (w * c) bytes of packed frames: only vertical neighbours meet)
//   _u16   matrices of rows x cols little-endian 16-bit samples, every sample read as min(s, 2^depth - 1) >> (depth - 8)
//
// One launch per call after one hipMemsetAsync of the sums; grid = (lane tiles over one parity's rows x row pieces, frame, parity), so
// every lane of a workgroup adds to the same four cells.  Vector form (plane base pointer, frame stride and row bytes multiples of 16):
// a lane owns 16 bytes of one row y and issues its five 16-byte nontemporal loads (rows y - 1, y, y + 1 of the frame, row y of the
// previous and of the next frame) before the first use; v_sad_u8 per dword, |a - c| computed once for the three combs.  Rows 0 and
// rows - 1 have no two neighbours: their a / c loads are aimed at row y itself (in bounds, in cache) and their comb sums dropped, so
// they add to k = 3 only.  One-sample form (any pointer, stride and row length): a lane owns SC_ONE_ITERS samples.  Lane sums are
// 32-bit, reduced over the wave by __shfl_xor, over the workgroup through 16 LDS words, then four 64-bit vector atomics per workgroup.
#include "common.hpp"
#include "video_samples.hpp"

#include <cstdint>

namespace savsr {
namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_ONE_ITERS = 8;                     // samples per lane in the one-sample form
constexpr int SC_SUMS = 4;                          // per parity: comb prev / next / self, rep
constexpr int SC_CELLS = 8;                         // per frame
constexpr int SC_MAX_Y = 65535;                     // grid.y: frames per launch
constexpr long long SC_MAX_PLANE = 0x7fff0000ll;    // bytes of a plane: the lane tiles of a frame fit grid.x and 32-bit counts

// What a launch works on.  Rows are `pitch` bytes apart.
struct StatJob {
    const uint8_t* src;          // the matrix of resident frame 0
    long long stride, pitch;     // bytes between frames / rows
    int n_frames, from, cols;    // cols: samples of a row
    int rows;
    uint32_t top;                // 2^depth - 1
    int shift;                   // depth - 8
};

// The four lane sums of a workgroup -> one 64-bit vector atomic each on cell[0], cell[2], cell[4], cell[6].  A lane sum is at most
// SC_ONE_ITERS (or 16, the bytes of a vector lane's row piece) x 2 x 255 <= 8160, a workgroup's at most 256 x 8160 < 2^21: the 32-bit
// partials cannot overflow whatever the frame size, because a lane never holds more than one row piece.
__device__ __forceinline__ void sc_block_add(const uint32_t (&acc)[SC_SUMS], unsigned long long* cell) {
#ifdef SAVSR_HOST_CHECK          // the host check runs one thread at a time: every thread adds its own sums
    for (int k = 0; k < SC_SUMS; ++k)
        if (acc[k]) atomicAdd(cell + 2 * k, (unsigned long long)acc[k]);
#else
    __shared__ uint32_t part[SC_SUMS][SC_THREADS / 64];
    uint32_t v[SC_SUMS];
#pragma unroll
    for (int k = 0; k < SC_SUMS; ++k) v[k] = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < SC_SUMS; ++k) v[k] += __shfl_xor(v[k], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < SC_SUMS; ++k) part[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < SC_SUMS) {
        unsigned long long s = 0;
#pragma unroll
        for (int i = 0; i < SC_THREADS / 64; ++i) s += part[threadIdx.x][i];
        if (s) atomicAdd(cell + 2 * threadIdx.x, s);
    }
#endif
}

// The rows of parity q: y = q + 2 s, s = 0 .. (rows - q + 1) / 2 - 1.
__device__ __forceinline__ uint32_t sc_parity_rows(int rows, uint32_t q) { return (uint32_t)(rows - (int)q + 1) >> 1; }

// Vector form: lane = (row s of the parity, 16-byte chunk) = (idx / chunks, idx % chunks), idx = blockIdx.x * SC_THREADS + threadIdx.x;
// frame blockIdx.y of the launch, parity blockIdx.z.  BYTES: of a sample.
template <int BYTES>
__global__ __launch_bounds__(SC_THREADS) void field_stats_vec_kernel(StatJob jb, unsigned long long* __restrict__ out) {
    const uint32_t q = blockIdx.z;
    const uint32_t chunks = (uint32_t)(jb.pitch >> 4);
    const uint32_t idx = blockIdx.x * SC_THREADS + threadIdx.x;
    const uint32_t s = idx / chunks, chunk = idx - s * chunks;
    uint32_t acc[SC_SUMS] = {0u, 0u, 0u, 0u};
    if (s < sc_parity_rows(jb.rows, q)) {
        const int n = jb.from + (int)blockIdx.y;
        const int np = n > 0 ? n - 1 : 0;
        const int nn = n < jb.n_frames - 1 ? n + 1 : n;
        const long long y = (long long)q + 2ll * s;
        const bool inner = y >= 1 && y <= (long long)jb.rows - 2;
        const long long up = inner ? jb.pitch : 0;          // rows 0 and rows - 1: a and c are row y itself and their combs are dropped
        const uint8_t* cur = jb.src + (long long)n * jb.stride + y * jb.pitch;
        const uint8_t* prev = jb.src + (long long)np * jb.stride + y * jb.pitch;
        const uint8_t* next = jb.src + (long long)nn * jb.stride + y * jb.pitch;
        const u32x4 a = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(cur - up) + chunk);
        const u32x4 c = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(cur + up) + chunk);
        const u32x4 b = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(cur) + chunk);
        const u32x4 bp = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(prev) + chunk);
        const u32x4 bn = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(next) + chunk);
        uint32_t ac = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if constexpr (BYTES == 1) {
                ac = sad4(a[e], c[e], ac);
                acc[0] = sad4(c[e], bp[e], sad4(a[e], bp[e], acc[0]));
                acc[1] = sad4(c[e], bn[e], sad4(a[e], bn[e], acc[1]));
                acc[2] = sad4(c[e], b[e], sad4(a[e], b[e], acc[2]));
                acc[3] = sad4(b[e], bp[e], acc[3]);
            } else {
                const uint32_t ae = msb8x2(a[e], jb.top, jb.shift), ce = msb8x2(c[e], jb.top, jb.shift), be = msb8x2(b[e], jb.top, jb.shift);
                const uint32_t pe = msb8x2(bp[e], jb.top, jb.shift), ne = msb8x2(bn[e], jb.top, jb.shift);
                ac = sad2(ae, ce, ac);
                acc[0] = sad2(ce, pe, sad2(ae, pe, acc[0]));
                acc[1] = sad2(ce, ne, sad2(ae, ne, acc[1]));
                acc[2] = sad2(ce, be, sad2(ae, be, acc[2]));
                acc[3] = sad2(be, pe, acc[3]);
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] = inner ? acc[k] - ac : 0u;          // per sample |a - b| + |c - b| >= |a - c|: the sums stay >= 0
    }
    sc_block_add(acc, out + SC_CELLS * blockIdx.y + q);
}

template <int BYTES>
__device__ __forceinline__ uint32_t sc_sample(const uint8_t* row, uint32_t x, uint32_t top, int shift) {
    if constexpr (BYTES == 1) return row[x];
    else return msb8(reinterpret_cast<const uint16_t*>(row)[x], top, shift);
}

// One-sample form: sample i = (row s of the parity, x) = (i / cols, i % cols), i = blockIdx.x * (SC_THREADS * SC_ONE_ITERS) + it * SC_THREADS + tid.
template <int BYTES>
__global__ __launch_bounds__(SC_THREADS) void field_stats_one_kernel(StatJob jb, unsigned long long* __restrict__ out) {
    const uint32_t q = blockIdx.z;
    const int n = jb.from + (int)blockIdx.y;
    const int np = n > 0 ? n - 1 : 0;
    const int nn = n < jb.n_frames - 1 ? n + 1 : n;
    const uint8_t* cur = jb.src + (long long)n * jb.stride;
    const uint8_t* prev = jb.src + (long long)np * jb.stride;
    const uint8_t* next = jb.src + (long long)nn * jb.stride;
    const uint32_t total = sc_parity_rows(jb.rows, q) * (uint32_t)jb.cols;
    const uint32_t i0 = blockIdx.x * (SC_THREADS * SC_ONE_ITERS) + threadIdx.x;
    uint32_t acc[SC_SUMS] = {0u, 0u, 0u, 0u};
#pragma unroll 2
    for (int it = 0; it < SC_ONE_ITERS; ++it) {
        const uint32_t i = i0 + it * SC_THREADS;
        if (i < total) {
            const uint32_t s = i / (uint32_t)jb.cols, x = i - s * (uint32_t)jb.cols;
            const long long y = (long long)q + 2ll * s;
            const long long off = y * jb.pitch;
            const uint32_t b = sc_sample<BYTES>(cur + off, x, jb.top, jb.shift), bp = sc_sample<BYTES>(prev + off, x, jb.top, jb.shift);
            acc[3] += absdiff(b, bp);
            if (y >= 1 && y <= (long long)jb.rows - 2) {
                const uint32_t a = sc_sample<BYTES>(cur + off - jb.pitch, x, jb.top, jb.shift), c = sc_sample<BYTES>(cur + off + jb.pitch, x, jb.top, jb.shift);
                const uint32_t bn = sc_sample<BYTES>(next + off, x, jb.top, jb.shift);
                const uint32_t ac = absdiff(a, c);
                acc[0] += absdiff(a, bp) + absdiff(c, bp) - ac;
                acc[1] += absdiff(a, bn) + absdiff(c, bn) - ac;
                acc[2] += absdiff(a, b) + absdiff(c, b) - ac;
            }
        }
    }
    sc_block_add(acc, out + SC_CELLS * blockIdx.y + q);
}

inline unsigned sc_blocks(long long units, int per_block) { return (unsigned)((units + per_block - 1) / per_block); }

template <int BYTES>
int launch_stats(StatJob jb, int n_out, int64_t* out, hipStream_t st, const char* what) {
    hipError_t e = hipMemsetAsync(out, 0, sizeof(int64_t) * SC_CELLS * (size_t)n_out, st);
    if (e != hipSuccess) { set_error("%s: hipMemsetAsync failed: %s", what, hipGetErrorString(e)); return (int)e; }
    const bool vec = (reinterpret_cast<uintptr_t>(jb.src) & 15) == 0 && jb.stride % 16 == 0 && jb.pitch % 16 == 0;
    const long long even_rows = (jb.rows + 1) / 2;          // parity 0 has the most rows: the grid is sized for it
    const unsigned gx = vec ? sc_blocks(even_rows * (jb.pitch >> 4), SC_THREADS) : sc_blocks(even_rows * jb.cols, SC_THREADS * SC_ONE_ITERS);
    const unsigned gz = jb.rows > 1 ? 2u : 1u;
    for (int f0 = 0; f0 < n_out; f0 += SC_MAX_Y) {          // (one launch for up to 65535 frames)
        const int nf = n_out - f0 < SC_MAX_Y ? n_out - f0 : SC_MAX_Y;
        StatJob part = jb;
        part.from = jb.from + f0;
        unsigned long long* cells = reinterpret_cast<unsigned long long*>(out) + (long long)SC_CELLS * f0;
        if (vec) hipLaunchKernelGGL((field_stats_vec_kernel<BYTES>), dim3(gx, (unsigned)nf, gz), dim3(SC_THREADS), 0, st, part, cells);
        else hipLaunchKernelGGL((field_stats_one_kernel<BYTES>), dim3(gx, (unsigned)nf, gz), dim3(SC_THREADS), 0, st, part, cells);
        if (int rc = check_launch(vec ? "field_stats_vec_kernel" : "field_stats_one_kernel")) return rc;
    }
    return 0;
}

// The checks of a matrix inside resident frames; nullptr or the reason.
const char* sc_check_matrix(const void* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int64_t row_bytes, int lo, int hi) {
    if (!frames) return "null pointer";
    if (n_frames < 1) return "n_frames >= 1";
    if (rows < 1) return "rows >= 1";
    if (row_bytes < 1) return "a row holds at least one sample";
    if ((long long)rows * row_bytes > SC_MAX_PLANE) return "a plane of at most 2147418112 bytes";
    if (lo < 0 || hi > n_frames || lo > hi) return "the range needs 0 <= lo <= hi <= n_frames";
    if (plane_offset < 0) return "plane offsets >= 0";
    if (frame_bytes < plane_offset + (int64_t)rows * row_bytes) return "frame_bytes smaller than plane_offset plus the rows x row_bytes plane";
    return nullptr;
}

int sc_refuse(const char* who, const char* why) {
    char msg[192];
    snprintf(msg, sizeof msg, "%s: %s", who, why);
    return fail_arg(msg);
}

}  // namespace
}  // namespace savsr

using namespace savsr;

extern "C" int savsr_video_field_stats_u8(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int row_bytes,
                                          int lo, int hi, int64_t* out, void* stream) {
    const char* who = "video_field_stats_u8";
    if (const char* why = sc_check_matrix(frames, n_frames, frame_bytes, plane_offset, rows, row_bytes, lo, hi)) return sc_refuse(who, why);
    if (!out && hi > lo) return sc_refuse(who, "null pointer");
    if (reinterpret_cast<uintptr_t>(out) & 7) return sc_refuse(who, "out must be 8-byte aligned");
    if (hi == lo) return 0;
    return launch_stats<1>(StatJob{frames + plane_offset, frame_bytes, row_bytes, n_frames, lo, row_bytes, rows, 255u, 0}, hi - lo, out,
                           static_cast<hipStream_t>(stream), who);
}

extern "C" int savsr_video_field_stats_u16(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols,
                                           int depth, int lo, int hi, int64_t* out, void* stream) {
    const char* who = "video_field_stats_u16";
    if (const char* why = sc_check_matrix(frames, n_frames, frame_bytes, plane_offset, rows, 2 * (int64_t)cols, lo, hi)) return sc_refuse(who, why);
    if (depth != 10 && depth != 12) return sc_refuse(who, "depth 10 or 12 (8 bits: savsr_video_field_stats_u8)");
    if ((reinterpret_cast<uintptr_t>(frames) & 1) || ((frame_bytes | plane_offset) & 1))
        return sc_refuse(who, "frames, the frame stride and the plane offset must be 2-byte aligned (16-bit samples)");
    if (!out && hi > lo) return sc_refuse(who, "null pointer");
    if (reinterpret_cast<uintptr_t>(out) & 7) return sc_refuse(who, "out must be 8-byte aligned");
    if (hi == lo) return 0;
    return launch_stats<2>(StatJob{frames + plane_offset, frame_bytes, 2 * (int64_t)cols, n_frames, lo, cols, rows, (1u << depth) - 1u, depth - 8},
                           hi - lo, out, static_cast<hipStream_t>(stream), who);
}
