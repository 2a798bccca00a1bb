// Noise statistics (ABI 55): how large is the second difference of a plane, cell by cell (savsr_amd/noise.py `noise_stats_matrix` is the
// specification; the kernels equal it bit for bit, the decision is made on the host in exact arithmetic).
//
// A plane of rows x cols pixels of `step` samples each (sample x of a row meets samples x +- j * step only: step = the channels of packed
// frames), every sample v = min(s, 2^depth - 1) at its own depth.  With h[y][x] = v[y][x - 1] - 2 v[y][x] + v[y][x + 1] and
// L[y][x] = |h[y - 1][x] - 2 h[y][x] + h[y + 1][x]| (1 <= y <= rows - 2, 1 <= x <= cols - 2), cell (i, j), i < (rows - 2) / 8,
// j < (cols - 2) / 8, holds the 64 values L[8i + 1 .. 8i + 8][8j + 1 .. 8j + 8]: its support is rows 8i .. 8i + 9, columns 8j .. 8j + 9.
// A cell one of whose 8 row sums or 8 column sums of L is 0 is flat: out[512 n + 2 * 255] += 1.  Any other cell has S = (sum of L) >>
// (depth - 8) and b = min(S >> 4, 254): out[512 n + 2 b] += 1, out[512 n + 2 b + 1] += S.  sum of L <= 64 * 16 * 4095 < 2^32.
// Field-wise, each field is a plane of its own (rows of one parity, twice the pitch) and both add into the frame's table: grid.z is the
// field.  Counts and sums are exact integers in any order, so the grid shape and the atomics change nothing in the result.  The table is
// ADDED to: the caller zeroes it once (Cb and Cr land in one class that way).
//
//   _u8    planes of rows x (cols * step) bytes
//   _u16   the same in little-endian 16-bit samples
//
// One launch per call, no memset, grid = (cells of a field over workgroups, frame, field).  A lane owns one cell and walks down its 10
// rows: of each it loads the 10 samples of the support -- in the vector form (step 1; the plane's base pointer, the frame stride and
// the row bytes multiples of 8 for bytes, of 16 for 16-bit samples) the 8 own samples in one load and the dword behind them, which a
// row that has this cell always holds (cols is a multiple of 8 there, and cols >= 8j + 10); in the one-sample form (any pointer, stride,
// row length and step) sample by sample.  It keeps the horizontal second differences of the two previous rows in registers, so a row
// costs one separable update, and the 8 column sums and the row sum for the flat test.  (A lane of two cells, 16 bytes of a row of
// bytes, halves the lanes: a 576 x 720 plane has 71 x 89 cells, 16 frames are 395 workgroups of one-cell lanes on 256 CUs, and would
// be 200 of two-cell lanes -- fewer than the chip has CUs, as grid.hip's band of 16 rows was.)  A cell goes into a per-wave LDS table
// of 256 x (count, sum) 32-bit words (64 lanes x 2^22 stay below 2^32) and leaves the workgroup as 64-bit vector atomics on the rows
// that are not zero.
#include "common.hpp"
#include "video_samples.hpp"
#include "field_matrix.hpp"

#include <cstdint>

namespace savsr {
namespace {

constexpr int NS_THREADS = FM_THREADS;
constexpr int NS_ROWS = 256;                        // of a frame's table: 255 bins and the flat cells
constexpr int NS_FLAT = 255;
constexpr int NS_CELL = 8;                          // a cell is 8 x 8 values of L, its support 10 x 10 samples
constexpr int NS_SUP = NS_CELL + 2;
constexpr int NS_MAX_STEP = 4;

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));          // an 8-byte load

struct NoiseJob {
    const uint8_t* src;          // the plane of frame 0
    long long stride, pitch;     // bytes between frames and between the plane's rows
    int rows, cols, step;        // cols: pixels of a row
    int fields;                  // 1, or 2: every field a plane of its own
    uint32_t top;                // 2^depth - 1
    int shift;                   // depth - 8
};

// The 10 samples of a cell's support in `row`: elements e0, e0 + step, ...  VEC: step is 1 and e0 a multiple of 8.
template <int BYTES, bool VEC>
__device__ __forceinline__ void ns_load(const NoiseJob& jb, const uint8_t* row, long long e0, int step, int (&v)[NS_SUP]) {
    if constexpr (VEC && BYTES == 1) {
        const uint32_t* words = reinterpret_cast<const uint32_t*>(row + e0);
        const u32x2 own = *reinterpret_cast<const u32x2*>(words);
        const uint32_t w[3] = {own[0], own[1], words[2]};
#pragma unroll
        for (int i = 0; i < NS_SUP; ++i) v[i] = (int)((w[i / 4] >> (8 * (i % 4))) & 255u);
    } else if constexpr (VEC) {
        const uint32_t* words = reinterpret_cast<const uint32_t*>(row + 2 * e0);
        const u32x4 own = *reinterpret_cast<const u32x4*>(words);
        const uint32_t w[5] = {own[0], own[1], own[2], own[3], words[4]};
#pragma unroll
        for (int i = 0; i < NS_SUP; ++i) v[i] = (int)min((w[i / 2] >> (16 * (i % 2))) & 0xffffu, jb.top);
    } else {
#pragma unroll
        for (int i = 0; i < NS_SUP; ++i) {
            if constexpr (BYTES == 1) v[i] = (int)row[e0 + (long long)i * step];
            else v[i] = (int)min((uint32_t) reinterpret_cast<const uint16_t*>(row)[e0 + (long long)i * step], jb.top);
        }
    }
}

// One cell of one lane.  Lane idx = (cell row, cell column, sample of the pixel).  add(b, S): one more cell in row b of the frame's table.
template <int BYTES, bool VEC, class Add>
__device__ __forceinline__ void ns_cell(const NoiseJob& jb, uint32_t idx, uint32_t field, Add add) {
    const int rows = (jb.rows - (int)field + jb.fields - 1) / jb.fields;          // of this field
    const uint32_t ny = (uint32_t)(max(rows, 2) - 2) / NS_CELL, nx = (uint32_t)(max(jb.cols, 2) - 2) / NS_CELL;
    const uint32_t step = VEC ? 1u : (uint32_t)jb.step, per = nx * step;          // lanes of a cell row
    if (per == 0) return;
    const uint32_t i = idx / per, rest = idx - i * per;
    if (i >= ny) return;
    const uint32_t j = rest / step, ch = rest - j * step;
    const long long pitch = jb.pitch * jb.fields;
    const uint8_t* row = jb.src + (long long)field * jb.pitch + (long long)(NS_CELL * i) * pitch;
    const long long e0 = (long long)(NS_CELL * j) * step + ch;
    int h1[NS_CELL], h2[NS_CELL];          // the horizontal second differences of rows r - 1 and r - 2
    uint32_t col[NS_CELL], total = 0;
    bool flat = false;
#pragma unroll
    for (int x = 0; x < NS_CELL; ++x) h1[x] = h2[x] = 0, col[x] = 0u;
#pragma unroll
    for (int r = 0; r < NS_SUP; ++r) {
        int v[NS_SUP], h[NS_CELL];
        ns_load<BYTES, VEC>(jb, row + (long long)r * pitch, e0, (int)step, v);
#pragma unroll
        for (int x = 0; x < NS_CELL; ++x) h[x] = v[x] - 2 * v[x + 1] + v[x + 2];
        if (r >= 2) {
            uint32_t sum = 0;
#pragma unroll
            for (int x = 0; x < NS_CELL; ++x) {
                const int l = h2[x] - 2 * h1[x] + h[x];
                const uint32_t a = (uint32_t)(l < 0 ? -l : l);
                col[x] += a;
                sum += a;
            }
            flat = flat || sum == 0u;
            total += sum;
        }
#pragma unroll
        for (int x = 0; x < NS_CELL; ++x) h2[x] = h1[x], h1[x] = h[x];
    }
#pragma unroll
    for (int x = 0; x < NS_CELL; ++x) flat = flat || col[x] == 0u;
    if (flat) {
        add((uint32_t)NS_FLAT, 0u);
    } else {
        const uint32_t S = total >> jb.shift;
        add(min(S >> 4, (uint32_t)(NS_FLAT - 1)), S);
    }
}

template <int BYTES, bool VEC>
__global__ __launch_bounds__(NS_THREADS) void noise_stats_kernel(NoiseJob jb, unsigned long long* __restrict__ out) {
    NoiseJob fr = jb;
    fr.src = jb.src + (long long)blockIdx.y * jb.stride;
    unsigned long long* table = out + (long long)(2 * NS_ROWS) * blockIdx.y;
#ifdef SAVSR_HOST_CHECK          // the host check runs one thread at a time: every thread adds its own cell
    ns_cell<BYTES, VEC>(fr, blockIdx.x * NS_THREADS + threadIdx.x, blockIdx.z, [&](uint32_t b, uint32_t S) {
        atomicAdd(table + 2 * b, 1ull);
        if (S) atomicAdd(table + 2 * b + 1, (unsigned long long)S);
    });
#else
    __shared__ uint32_t part[NS_THREADS / 64][NS_ROWS][2];
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = tid; k < (NS_THREADS / 64) * NS_ROWS * 2; k += NS_THREADS) (&part[0][0][0])[k] = 0u;
    __syncthreads();
    uint32_t(*wave_part)[2] = part[tid >> 6];
    ns_cell<BYTES, VEC>(fr, blockIdx.x * NS_THREADS + tid, blockIdx.z, [&](uint32_t b, uint32_t S) {
        atomicAdd(&wave_part[b][0], 1u);
        if (S) atomicAdd(&wave_part[b][1], S);
    });
    __syncthreads();
    for (uint32_t b = tid; b < NS_ROWS; b += NS_THREADS) {
        unsigned long long cnt = 0, sum = 0;
#pragma unroll
        for (int w = 0; w < NS_THREADS / 64; ++w) cnt += part[w][b][0], sum += part[w][b][1];
        if (cnt) atomicAdd(table + 2 * b, cnt);
        if (sum) atomicAdd(table + 2 * b + 1, sum);
    }
#endif
}

template <int BYTES, bool VEC>
int ns_launch(const NoiseJob& jb, int nf, unsigned long long* out, hipStream_t st) {
    const long long ny = (max((jb.rows + jb.fields - 1) / jb.fields, 2) - 2) / NS_CELL;          // of field 0, which has the most rows
    const long long nx = (max(jb.cols, 2) - 2) / NS_CELL;
    const long long lanes = ny * nx * (VEC ? 1 : jb.step);
    if (lanes == 0) return 0;          // no plane of the call holds a cell: nothing to add
    hipLaunchKernelGGL((noise_stats_kernel<BYTES, VEC>), dim3(blocks(lanes, NS_THREADS), (unsigned)nf, (unsigned)jb.fields), dim3(NS_THREADS), 0, st, jb,
                       out);
    return check_launch("noise_stats_kernel");
}

// The body of the two entries.  cols: pixels of a row; step: samples of a pixel.
template <int BYTES>
int noise_stats(const char* who, const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step, int depth,
                int interlaced, int64_t* out, void* stream) {
    constexpr MatrixRule rule{1, 0, nullptr, "", false};
    if (step < 1 || step > NS_MAX_STEP) return refuse(who, "step 1 .. 4 (the samples of a pixel)");
    if (cols < 1) return refuse(who, "a row holds at least one sample");
    const int64_t row_bytes = (int64_t)BYTES * cols * step;
    if (const char* why = check_matrix(rule, frames, n_frames, frame_bytes, plane_offset, rows, row_bytes, 0, 0, n_frames)) return refuse(who, why);
    if (BYTES == 2)
        if (int rc = check_samples16(who, depth, frames, frame_bytes, plane_offset)) return rc;
    if (const char* why = check_cells(out, true)) return refuse(who, why);
    if (interlaced != 0 && interlaced != 1) return refuse(who, "interlaced 0 or 1");
    const NoiseJob jb{frames + plane_offset, frame_bytes, row_bytes, rows, cols, step, interlaced && rows > 1 ? 2 : 1, (1u << depth) - 1u, depth - 8};
    constexpr uintptr_t A = 8 * BYTES;          // the vector form's own load
    const bool vec = step == 1 && (reinterpret_cast<uintptr_t>(jb.src) % A) == 0 && jb.stride % (long long)A == 0 && jb.pitch % (long long)A == 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return for_frame_chunks(n_frames, FM_MAX_FRAMES, [&](int f0, int nf) {
        NoiseJob part = jb;
        part.src = jb.src + (long long)f0 * jb.stride;
        unsigned long long* table = reinterpret_cast<unsigned long long*>(out) + (long long)(2 * NS_ROWS) * f0;
        return vec ? ns_launch<BYTES, true>(part, nf, table, st) : ns_launch<BYTES, false>(part, nf, table, st);
    });
}

}  // namespace
}  // namespace savsr

using namespace savsr;

extern "C" int savsr_video_noise_stats_u8(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step,
                                          int interlaced, int64_t* out, void* stream) {
    return noise_stats<1>("video_noise_stats_u8", frames, n_frames, frame_bytes, plane_offset, rows, cols, step, 8, interlaced, out, stream);
}

extern "C" int savsr_video_noise_stats_u16(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step,
                                           int depth, int interlaced, int64_t* out, void* stream) {
    return noise_stats<2>("video_noise_stats_u16", frames, n_frames, frame_bytes, plane_offset, rows, cols, step, depth, interlaced, out, stream);
}
