// The active-picture detector's line sums (ABI 42): per matrix of a batch the sum of the 8-bit samples of every row and of every
// column, exact integers (savsr_amd/active.py `line_sums` is the specification; cropdetect's rule itself runs on the host in exact
// arithmetic, `active_rect`).  Elementwise and HBM-bound like scene.hip's scores: one read of the samples gives both sets of sums.
// Integer sums do not depend on their order, so the grid shape and the atomics change nothing in the result.
//
//   _u8    matrices of rows x row_bytes bytes, frame_bytes apart: packed uint8 frames (h x (w * c), the host folds the c byte columns of
//          a pixel) and the Y plane of 8-bit planar frames (h x w at the start of a frame)
//   _u16   matrices of rows x cols 16-bit samples, frame_bytes apart: the Y plane of 10- / 12-bit planar frames, every sample as its 8
//          most significant bits, min(s, 2^d - 1) >> (d - 8)
//   _f32   n_mats contiguous matrices of rows x cols floats: the planes of [N][c][h][w] frames, every value after
//          savsr_video_quantize_u8's rule (clamp(0, 1) * 255.0f, rintf; NaN -> 0); the host sums the channels
//
// A workgroup owns a tile of LS_TILE_ROWS rows.  Vector form (base pointer, frame stride and row pitch multiples of 16 bytes): 16 lanes x
// 16 bytes cover LS_TILE_BYTES bytes of a row, so a wave reads 4 rows and the workgroup 16 rows per step, LS_LOADS steps, all loads issued
// before the first use.  A row's partial is v_sad_u8 against zero, reduced over its 16 lanes by __shfl_xor, one 32-bit vector atomic per
// row and tile.  Column sums stay in the lane over all rows of the tile, two 16-bit fields per register (a wave adds at most
// 16 rows x 255 per field), meet in LDS and leave by one 32-bit vector atomic per column and tile.  One-sample form (any base pointer,
// stride and size): a lane owns 4 columns 64 apart (LS_ONE_COLS per tile), a wave reads one row per step.
#include "common.hpp"
#include "video_samples.hpp"

#include <cstdint>

namespace savsr {
namespace {

constexpr int LS_THREADS = 256;
constexpr int LS_TILE_ROWS = 64;                    // rows of a workgroup's tile, both forms
constexpr int LS_TILE_BYTES = 256;                  // bytes of a tile's row in the vector forms: 16 lanes x 16 bytes
constexpr int LS_ONE_COLS = 256;                    // samples of a tile's row in the one-sample forms: 4 per lane
constexpr int LS_LOADS = LS_TILE_ROWS / 16;         // 16-byte loads per lane: 4 waves x 4 rows each per step
constexpr int LS_MAX_Z = 65535;                     // grid.z
constexpr int LS_MAX_LINES = 65535 * LS_TILE_ROWS;  // grid.y; a line's sum stays below 2^32 far beyond it
static_assert(LS_ONE_COLS == LS_THREADS && LS_TILE_ROWS % 16 == 0 && LS_TILE_ROWS / 4 * 255 < 65536, "a wave's column partial must fit a 16-bit field");

enum { LS_U8 = 0, LS_U16 = 1, LS_F32 = 2 };

template <int KIND>
struct Kind {
    static constexpr int BYTES = KIND == LS_U8 ? 1 : (KIND == LS_U16 ? 2 : 4);          // of a sample
    static constexpr int SPL = 16 / BYTES;                                             // samples per 16-byte load
    static constexpr int NACC = KIND == LS_U8 ? 8 : (KIND == LS_U16 ? 4 : 2);           // column registers per lane, two 16-bit fields each
    static constexpr int COLS = LS_TILE_BYTES / BYTES;                                 // sample columns of a tile in the vector form
};

// Vector form.  base + blockIdx.z * stride: a matrix of rows x cols samples, rows `pitch` bytes apart; cols % SPL == 0.
// Lane = (row group rg = lane >> 4, chunk sub = lane & 15); step `it` reads rows tile + 16 * it + 4 * wave + rg.
template <int KIND>
__global__ __launch_bounds__(LS_THREADS) void line_sums_vec_kernel(const uint8_t* __restrict__ base, long long stride, int rows, int cols, long long pitch,
                                                                   uint32_t top, int shift, uint32_t* __restrict__ row_sums,
                                                                   uint32_t* __restrict__ col_sums) {
    typedef Kind<KIND> K;
    __shared__ uint32_t part[LS_THREADS / 64][K::COLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane & 15, rg = lane >> 4;
    const long long chunk = (long long)blockIdx.x * 16 + sub;
    const bool cok = chunk < cols / K::SPL;
    const long long row0 = (long long)blockIdx.y * LS_TILE_ROWS + 4 * wave + rg;
    const uint8_t* f = base + (long long)blockIdx.z * stride;
    u32x4 x[LS_LOADS];
#pragma unroll
    for (int it = 0; it < LS_LOADS; ++it) {
        const long long r = row0 + 16 * it;
        x[it] = u32x4{0u, 0u, 0u, 0u};          // (zero bits are the sample 0 in every kind)
        if (cok && r < rows) x[it] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(f + r * pitch) + chunk);
    }
    uint32_t acc[K::NACC];
#pragma unroll
    for (int a = 0; a < K::NACC; ++a) acc[a] = 0u;
#pragma unroll
    for (int it = 0; it < LS_LOADS; ++it) {
        uint32_t rs = 0u;
        if constexpr (KIND == LS_U8) {
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const uint32_t v = x[it][d];
                rs = sum4(v, rs);
                acc[2 * d] += v & 0x00ff00ffu;
                acc[2 * d + 1] += (v >> 8) & 0x00ff00ffu;
            }
        } else if constexpr (KIND == LS_U16) {
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const uint32_t v = msb8x2(x[it][d], top, shift);
                rs = sum4(v, rs);
                acc[d] += v;
            }
        } else {
            const uint32_t v = quant_u8(__uint_as_float(x[it][0])) | (quant_u8(__uint_as_float(x[it][1])) << 8) |
                               (quant_u8(__uint_as_float(x[it][2])) << 16) | (quant_u8(__uint_as_float(x[it][3])) << 24);
            rs = sum4(v, rs);
            acc[0] += v & 0x00ff00ffu;
            acc[1] += (v >> 8) & 0x00ff00ffu;
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) rs += __shfl_xor(rs, o, 64);
        const long long r = row0 + 16 * it;
        if (sub == 0 && rs && r < rows) atomicAdd(row_sums + (long long)blockIdx.z * rows + r, rs);
    }
    // the wave's four row groups, then the four waves through LDS
#pragma unroll
    for (int a = 0; a < K::NACC; ++a) {
        acc[a] += __shfl_xor(acc[a], 16, 64);
        acc[a] += __shfl_xor(acc[a], 32, 64);
    }
    if (rg == 0) {
        uint32_t* p = part[wave] + sub * K::SPL;
        if constexpr (KIND == LS_U16) {
#pragma unroll
            for (int d = 0; d < K::NACC; ++d) {
                p[2 * d] = acc[d] & 0xffffu;
                p[2 * d + 1] = acc[d] >> 16;
            }
        } else {          // a dword's bytes 0, 2 in the even register's fields, 1, 3 in the odd one's
#pragma unroll
            for (int d = 0; d < K::NACC / 2; ++d) {
                p[4 * d] = acc[2 * d] & 0xffffu;
                p[4 * d + 1] = acc[2 * d + 1] & 0xffffu;
                p[4 * d + 2] = acc[2 * d] >> 16;
                p[4 * d + 3] = acc[2 * d + 1] >> 16;
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < K::COLS) {
        uint32_t s = 0u;
#pragma unroll
        for (int wv = 0; wv < LS_THREADS / 64; ++wv) s += part[wv][threadIdx.x];
        const long long col = (long long)blockIdx.x * K::COLS + threadIdx.x;
        if (s && col < cols) atomicAdd(col_sums + (long long)blockIdx.z * cols + col, s);
    }
}

template <int KIND>
__device__ __forceinline__ uint32_t sample_of(const uint8_t* row, long long c, uint32_t top, int shift) {
    if constexpr (KIND == LS_U8) return row[c];
    else if constexpr (KIND == LS_U16) return msb8(reinterpret_cast<const uint16_t*>(row)[c], top, shift);
    else return quant_u8(reinterpret_cast<const float*>(row)[c]);
}

// One-sample form: a lane owns columns tile + lane + 64 j, j = 0 .. 3; step `it` reads row tile + 4 * it + wave.
template <int KIND>
__global__ __launch_bounds__(LS_THREADS) void line_sums_one_kernel(const uint8_t* __restrict__ base, long long stride, int rows, int cols, long long pitch,
                                                                   uint32_t top, int shift, uint32_t* __restrict__ row_sums,
                                                                   uint32_t* __restrict__ col_sums) {
    __shared__ uint32_t part[LS_THREADS / 64][LS_ONE_COLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long col0 = (long long)blockIdx.x * LS_ONE_COLS + lane;
    const uint8_t* f = base + (long long)blockIdx.z * stride;
    uint32_t acc[LS_ONE_COLS / 64];
#pragma unroll
    for (int j = 0; j < LS_ONE_COLS / 64; ++j) acc[j] = 0u;
#pragma unroll 4
    for (int it = 0; it < LS_TILE_ROWS / 4; ++it) {
        const long long r = (long long)blockIdx.y * LS_TILE_ROWS + 4 * it + wave;
        uint32_t rs = 0u;
        if (r < rows) {
#pragma unroll
            for (int j = 0; j < LS_ONE_COLS / 64; ++j) {
                const long long c = col0 + 64 * j;
                if (c < cols) {
                    const uint32_t v = sample_of<KIND>(f + r * pitch, c, top, shift);
                    acc[j] += v;
                    rs += v;
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) rs += __shfl_xor(rs, o, 64);
        if (lane == 0 && rs && r < rows) atomicAdd(row_sums + (long long)blockIdx.z * rows + r, rs);
    }
#pragma unroll
    for (int j = 0; j < LS_ONE_COLS / 64; ++j) part[wave][lane + 64 * j] = acc[j];
    __syncthreads();
    uint32_t s = 0u;
#pragma unroll
    for (int wv = 0; wv < LS_THREADS / 64; ++wv) s += part[wv][threadIdx.x];
    const long long col = (long long)blockIdx.x * LS_ONE_COLS + threadIdx.x;
    if (s && col < cols) atomicAdd(col_sums + (long long)blockIdx.z * cols + col, s);
}

// n matrices of rows x cols samples `stride` bytes apart, rows `pitch` bytes apart: zero both outputs, then the tiles
template <int KIND>
int launch_line_sums(const uint8_t* base, int n, long long stride, int rows, int cols, long long pitch, int depth, uint32_t* row_sums, uint32_t* col_sums,
                     hipStream_t st, const char* what) {
    // (one memset when the column cells follow the row cells directly, as savsr_amd.line_sums allocates them: a call is enqueue-bound)
    const size_t nr = (size_t)n * (size_t)rows, nc = (size_t)n * (size_t)cols;
    const bool joined = col_sums == row_sums + nr;
    hipError_t e = hipMemsetAsync(row_sums, 0, sizeof(uint32_t) * (joined ? nr + nc : nr), st);
    if (e == hipSuccess && !joined) e = hipMemsetAsync(col_sums, 0, sizeof(uint32_t) * nc, st);
    if (e != hipSuccess) { set_error("%s: hipMemsetAsync failed: %s", what, hipGetErrorString(e)); return (int)e; }
    typedef Kind<KIND> K;
    const bool vec = (reinterpret_cast<uintptr_t>(base) & 15) == 0 && stride % 16 == 0 && pitch % 16 == 0;
    const unsigned gx = (unsigned)((cols + (vec ? K::COLS : LS_ONE_COLS) - 1) / (vec ? K::COLS : LS_ONE_COLS));
    const unsigned gy = (unsigned)((rows + LS_TILE_ROWS - 1) / LS_TILE_ROWS);
    const uint32_t top = depth > 8 ? (1u << depth) - 1u : 255u;
    const int shift = depth > 8 ? depth - 8 : 0;
    for (int m0 = 0; m0 < n; m0 += LS_MAX_Z) {
        const int nm = n - m0 < LS_MAX_Z ? n - m0 : LS_MAX_Z;
        const uint8_t* f = base + (long long)m0 * stride;
        uint32_t* rs = row_sums + (long long)m0 * rows;
        uint32_t* cs = col_sums + (long long)m0 * cols;
        if (vec) hipLaunchKernelGGL((line_sums_vec_kernel<KIND>), dim3(gx, gy, nm), dim3(LS_THREADS), 0, st, f, stride, rows, cols, pitch, top, shift, rs, cs);
        else hipLaunchKernelGGL((line_sums_one_kernel<KIND>), dim3(gx, gy, nm), dim3(LS_THREADS), 0, st, f, stride, rows, cols, pitch, top, shift, rs, cs);
        if (int rc = check_launch(vec ? "line_sums_vec_kernel" : "line_sums_one_kernel")) return rc;
    }
    return 0;
}

}  // namespace
}  // namespace savsr

using namespace savsr;

extern "C" int savsr_video_line_sums_u8(const uint8_t* frames, int n, int64_t frame_bytes, int rows, int row_bytes, uint32_t* row_sums,
                                        uint32_t* col_sums, void* stream) {
    if (!frames || !row_sums || !col_sums) return fail_arg("video_line_sums_u8: null pointer");
    if (n < 1 || rows < 1 || row_bytes < 1) return fail_arg("video_line_sums_u8: n, rows, row_bytes >= 1");
    if (rows > LS_MAX_LINES || row_bytes > LS_MAX_LINES) return fail_arg("video_line_sums_u8: rows, row_bytes <= 4194240 (a line's sum is a 32-bit cell)");
    if (frame_bytes < (int64_t)rows * row_bytes) return fail_arg("video_line_sums_u8: frame_bytes smaller than the rows x row_bytes matrix");
    if ((reinterpret_cast<uintptr_t>(row_sums) | reinterpret_cast<uintptr_t>(col_sums)) & 3) return fail_arg("video_line_sums_u8: the sums must be 4-byte aligned");
    return launch_line_sums<LS_U8>(frames, n, frame_bytes, rows, row_bytes, row_bytes, 8, row_sums, col_sums, static_cast<hipStream_t>(stream),
                                   "video_line_sums_u8");
}

extern "C" int savsr_video_line_sums_u16(const uint8_t* frames, int n, int64_t frame_bytes, int rows, int cols, int depth, uint32_t* row_sums,
                                         uint32_t* col_sums, void* stream) {
    if (!frames || !row_sums || !col_sums) return fail_arg("video_line_sums_u16: null pointer");
    if (n < 1 || rows < 1 || cols < 1) return fail_arg("video_line_sums_u16: n, rows, cols >= 1");
    if (depth != 10 && depth != 12) return fail_arg("video_line_sums_u16: depth 10 or 12 (8 bits: savsr_video_line_sums_u8)");
    if (rows > LS_MAX_LINES || cols > LS_MAX_LINES) return fail_arg("video_line_sums_u16: rows, cols <= 4194240 (a line's sum is a 32-bit cell)");
    if (frame_bytes < 2 * (int64_t)rows * cols) return fail_arg("video_line_sums_u16: frame_bytes smaller than the rows x cols matrix of 16-bit samples");
    if ((reinterpret_cast<uintptr_t>(frames) & 1) || (frame_bytes & 1)) {
        set_error("video_line_sums_u16: frames and frame_bytes must be 2-byte aligned (16-bit samples)");
        return SAVSR_E_ALIGN;
    }
    if ((reinterpret_cast<uintptr_t>(row_sums) | reinterpret_cast<uintptr_t>(col_sums)) & 3) return fail_arg("video_line_sums_u16: the sums must be 4-byte aligned");
    return launch_line_sums<LS_U16>(frames, n, frame_bytes, rows, cols, 2ll * cols, depth, row_sums, col_sums, static_cast<hipStream_t>(stream),
                                    "video_line_sums_u16");
}

extern "C" int savsr_video_line_sums_f32(const float* mats, int n_mats, int rows, int cols, uint32_t* row_sums, uint32_t* col_sums, void* stream) {
    if (!mats || !row_sums || !col_sums) return fail_arg("video_line_sums_f32: null pointer");
    if (n_mats < 1 || rows < 1 || cols < 1) return fail_arg("video_line_sums_f32: n_mats, rows, cols >= 1");
    if (rows > LS_MAX_LINES || cols > LS_MAX_LINES) return fail_arg("video_line_sums_f32: rows, cols <= 4194240 (a line's sum is a 32-bit cell)");
    if (reinterpret_cast<uintptr_t>(mats) & 3) {
        set_error("video_line_sums_f32: mats must be 4-byte aligned");
        return SAVSR_E_ALIGN;
    }
    if ((reinterpret_cast<uintptr_t>(row_sums) | reinterpret_cast<uintptr_t>(col_sums)) & 3) return fail_arg("video_line_sums_f32: the sums must be 4-byte aligned");
    return launch_line_sums<LS_F32>(reinterpret_cast<const uint8_t*>(mats), n_mats, 4ll * rows * cols, rows, cols, 4ll * cols, 8, row_sums, col_sums,
                                    static_cast<hipStream_t>(stream), "video_line_sums_f32");
}
