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
// 32-bit (at most SC_ONE_ITERS, or 16, the bytes of a vector lane's row piece, x 2 x 255 <= 8160) and leave the workgroup through
// field_matrix.hpp's block_reduce: four 64-bit vector atomics per workgroup.  The matrix, its checks and the launch chunking are that header's.
#include "common.hpp"
#include "video_samples.hpp"
#include "field_matrix.hpp"

#include <cstdint>

namespace savsr {
namespace {

constexpr int SC_THREADS = FM_THREADS;
constexpr int SC_ONE_ITERS = 8;                     // samples per lane in the one-sample form
constexpr int SC_SUMS = 4;                          // per parity: comb prev / next / self, rep
constexpr int SC_CELLS = 8;                         // per frame
constexpr MatrixRule SC_RULE{1, 0, nullptr, "the range needs 0 <= lo <= hi <= n_frames", true};

// The rows of parity q: y = q + 2 s, s = 0 .. (rows - q + 1) / 2 - 1.
__device__ __forceinline__ uint32_t sc_parity_rows(int rows, uint32_t q) { return (uint32_t)(rows - (int)q + 1) >> 1; }

// Vector form: lane = (row s of the parity, 16-byte chunk) = (idx / chunks, idx % chunks), idx = blockIdx.x * SC_THREADS + threadIdx.x;
// frame blockIdx.y of the launch, parity blockIdx.z.  BYTES: of a sample.
template <int BYTES>
__global__ __launch_bounds__(SC_THREADS) void field_stats_vec_kernel(FieldMatrix jb, unsigned long long* __restrict__ out) {
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
    block_reduce<SC_SUMS, 2>(acc, out + SC_CELLS * blockIdx.y + q);
}

// One-sample form: sample i = (row s of the parity, x) = (i / cols, i % cols), i = blockIdx.x * (SC_THREADS * SC_ONE_ITERS) + it * SC_THREADS + tid.
template <int BYTES>
__global__ __launch_bounds__(SC_THREADS) void field_stats_one_kernel(FieldMatrix jb, unsigned long long* __restrict__ out) {
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
            const uint32_t b = sample8<BYTES>(cur + off, x, jb.top, jb.shift), bp = sample8<BYTES>(prev + off, x, jb.top, jb.shift);
            acc[3] += absdiff(b, bp);
            if (y >= 1 && y <= (long long)jb.rows - 2) {
                const uint32_t a = sample8<BYTES>(cur + off - jb.pitch, x, jb.top, jb.shift), c = sample8<BYTES>(cur + off + jb.pitch, x, jb.top, jb.shift);
                const uint32_t bn = sample8<BYTES>(next + off, x, jb.top, jb.shift);
                const uint32_t ac = absdiff(a, c);
                acc[0] += absdiff(a, bp) + absdiff(c, bp) - ac;
                acc[1] += absdiff(a, bn) + absdiff(c, bn) - ac;
                acc[2] += absdiff(a, b) + absdiff(c, b) - ac;
            }
        }
    }
    block_reduce<SC_SUMS, 2>(acc, out + SC_CELLS * blockIdx.y + q);
}

template <int BYTES>
int launch_stats(FieldMatrix jb, int n_out, int64_t* out, hipStream_t st, const char* what) {
    if (int rc = clear_cells(out, SC_CELLS, n_out, st, what)) return rc;
    const bool vec = aligned16(jb.src, jb.stride, jb.pitch);
    const long long even_rows = (jb.rows + 1) / 2;          // parity 0 has the most rows: the grid is sized for it
    const unsigned gx = vec ? blocks(even_rows * (jb.pitch >> 4), SC_THREADS) : blocks(even_rows * jb.cols, SC_THREADS * SC_ONE_ITERS);
    const unsigned gz = jb.rows > 1 ? 2u : 1u;
    return for_frame_chunks(n_out, FM_MAX_FRAMES, [&](int f0, int nf) {
        FieldMatrix part = jb;
        part.from = jb.from + f0;
        unsigned long long* cells = reinterpret_cast<unsigned long long*>(out) + (long long)SC_CELLS * f0;
        if (vec) hipLaunchKernelGGL((field_stats_vec_kernel<BYTES>), dim3(gx, (unsigned)nf, gz), dim3(SC_THREADS), 0, st, part, cells);
        else hipLaunchKernelGGL((field_stats_one_kernel<BYTES>), dim3(gx, (unsigned)nf, gz), dim3(SC_THREADS), 0, st, part, cells);
        return check_launch(vec ? "field_stats_vec_kernel" : "field_stats_one_kernel");
    });
}

// The body of the two entries.  width: row_bytes (_u8) or cols (_u16).
template <int BYTES>
int field_stats(const char* who, const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int width, int depth, int lo,
                int hi, int64_t* out, void* stream) {
    if (const char* why = check_matrix(SC_RULE, frames, n_frames, frame_bytes, plane_offset, rows, (int64_t)BYTES * width, 0, lo, hi)) return refuse(who, why);
    if (BYTES == 2)
        if (int rc = check_samples16(who, depth, frames, frame_bytes, plane_offset)) return rc;
    if (const char* why = check_cells(out, hi > lo)) return refuse(who, why);
    if (hi == lo) return 0;
    return launch_stats<BYTES>(field_matrix<BYTES>(frames, n_frames, frame_bytes, plane_offset, rows, width, depth, lo), hi - lo, out,
                               static_cast<hipStream_t>(stream), who);
}

}  // namespace
}  // namespace savsr

using namespace savsr;

extern "C" int savsr_video_field_stats_u8(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int row_bytes,
                                          int lo, int hi, int64_t* out, void* stream) {
    return field_stats<1>("video_field_stats_u8", frames, n_frames, frame_bytes, plane_offset, rows, row_bytes, 8, lo, hi, out, stream);
}

extern "C" int savsr_video_field_stats_u16(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols,
                                           int depth, int lo, int hi, int64_t* out, void* stream) {
    return field_stats<2>("video_field_stats_u16", frames, n_frames, frame_bytes, plane_offset, rows, cols, depth, lo, hi, out, stream);
}
