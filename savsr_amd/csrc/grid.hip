// Block-grid statistics (ABI 53): where do small isolated steps lie, modulo 16, along the rows and along the columns of a plane
// (savsr_amd/grid.py `grid_stats_matrix` is the specification; the kernels equal it bit for bit, the decision is made on the host in
// exact arithmetic).
//
// A plane of rows x cols pixels of `step` samples each (sample x of a row meets samples x +- j * step only: step = the channels of packed
// frames), every sample on the detectors' 8-bit scale.  Along a line v, at every boundary x with 2 <= x <= L - 2:
//   s = |v[x] - v[x - 1]|, l = |v[x - 1] - v[x - 2]|, r = |v[x + 1] - v[x]|;   a hit iff s > l + r and s <= cap.
// out[32 n + x mod 16] += the hits along the rows of frame n, out[32 n + 16 + y mod 16] += those along its columns.  Field-wise, each
// field is a plane of its own (rows of one parity, twice the pitch) and y is the field row; the rows of both fields are all the rows,
// so one kernel serves both: grid.z is the field.  Counts are exact integers in any order, so the grid shape and the atomics change
// nothing in the result.  The cells are ADDED to: the caller zeroes them once (Cb and Cr land in one class that way).
//
//   _u8    planes of rows x (cols * step) bytes
//   _u16   the same in little-endian 16-bit samples, every sample read as min(s, 2^depth - 1) >> (depth - 8)
//
// One launch per call, no memset, grid = (lane tiles over bands x row pieces, frame, field).  A lane owns one piece of a row -- 16 bytes
// in the vector form (plane base pointer, frame stride and row bytes multiples of 16), one sample in the one-sample form (any pointer,
// stride and row length) -- and walks down a band of 4 (field) rows.  It keeps the four rows a column boundary reads (y - 2 .. y + 1) in
// registers as it goes: 7 row pieces are loaded for 4 rows of boundaries, the three shared with the neighbouring bands come from cache.
// (A band of 16 rows loads 19 for 16, but a 576 x 720 plane then has 1620 lanes a frame, 16 frames fill 102 workgroups of a 256-CU
// chip, and the kernel took 24 us at 576 x 720 and at 720 x 1280 alike: the lanes' serial walk, not the traffic, set its time.)  The row hits of a piece need 2 * step samples to its left and step to its right: dwords of the neighbouring pieces,
// loaded beside its own (the neighbouring lanes have just asked for the same lines).  Hits are kept per lane in packed byte counters
// (16 row positions, 4 band rows; none exceeds 16), mapped to cells once per band, added into the workgroup's 32 LDS cells (a copy per
// wave, so that at most 64 lanes meet on an address) and leave the workgroup as at most 32 64-bit vector atomics.
#include "common.hpp"
#include "video_samples.hpp"
#include "field_matrix.hpp"

#include <cstdint>

namespace savsr {
namespace {

constexpr int GS_THREADS = FM_THREADS;
constexpr int GS_BAND = 4;                          // (field) rows of boundaries a lane walks (a divisor of 16, the cells' modulus)
constexpr int GS_CELLS = 32;                        // per frame: 16 along the rows, 16 along the columns
constexpr int GS_MAX_STEP = 4;

struct GridJob {
    const uint8_t* src;          // the plane of frame 0
    long long stride, pitch;     // bytes between frames and between the plane's rows
    int rows, cols, step;        // cols: pixels of a row
    int fields;                  // 1, or 2: every field a plane of its own
    uint32_t top;                // 2^depth - 1
    int shift;                   // depth - 8
    uint32_t cap;
};

// The samples a lane reads of one row: E of its own and 2 S to the left, S to the right.  ext[2 S + e] is sample g0 + e of the row.
template <int BYTES, int STEP, bool VEC>
struct GsPiece {
    static constexpr int E = VEC ? 16 / BYTES : 1, S = STEP, N = E + 3 * S;
};

// Sample g of a row on the 8-bit scale; anything (0) outside the row: no boundary that is counted reads it.
template <int BYTES>
__device__ __forceinline__ uint32_t gs_sample(const GridJob& jb, const uint8_t* row, long long g, long long row_elems) {
    if (g < 0 || g >= row_elems) return 0u;
    return sample8<BYTES>(row, (uint32_t)g, jb.top, jb.shift);
}

// The N samples around a lane's piece of `row`, own samples g0 .. g0 + E - 1.  WIDE = false: the own samples alone (the rows above and
// below a band, which only the columns read); the others are left at 0.
template <int BYTES, int STEP, bool VEC, bool WIDE>
__device__ __forceinline__ void gs_load(const GridJob& jb, const uint8_t* row, long long g0, long long row_elems, uint32_t* ext) {
    using P = GsPiece<BYTES, STEP, VEC>;
    if constexpr (VEC) {
        constexpr int PER = 4 / BYTES;                                  // samples of a dword
        constexpr int LD = (2 * STEP + PER - 1) / PER, RD = (STEP + PER - 1) / PER;          // dwords to the left and to the right
        const uint32_t* words = reinterpret_cast<const uint32_t*>(row) + g0 / PER;          // (g0 is a multiple of 16 / BYTES)
        const u32x4 own = *reinterpret_cast<const u32x4*>(words);
        uint32_t w[LD + 4 + RD];
#pragma unroll
        for (int i = 0; i < LD; ++i) w[i] = WIDE && g0 > 0 ? words[i - LD] : 0u;          // (a piece is at least LD dwords: the left one holds them all)
#pragma unroll
        for (int i = 0; i < 4; ++i) w[LD + i] = own[i];
#pragma unroll
        for (int i = 0; i < RD; ++i) w[LD + 4 + i] = WIDE && g0 + P::E < row_elems ? words[4 + i] : 0u;
#pragma unroll
        for (int i = 0; i < P::N; ++i) {
            if (!WIDE && (i < 2 * STEP || i >= 2 * STEP + P::E)) {
                ext[i] = 0u;
                continue;
            }
            const int at = LD * PER - 2 * STEP + i;          // sample index among the dwords' samples
            if constexpr (BYTES == 1) ext[i] = (w[at / 4] >> (8 * (at % 4))) & 255u;
            else ext[i] = msb8((w[at / 2] >> (16 * (at % 2))) & 0xffffu, jb.top, jb.shift);
        }
    } else {
#pragma unroll
        for (int i = 0; i < P::N; ++i) ext[i] = WIDE || i == 2 * STEP ? gs_sample<BYTES>(jb, row, g0 - 2 * STEP + i, row_elems) : 0u;
    }
}

// |a - b| of two samples on the 8-bit scale: one v_sad_u8 (the upper bytes of both are zero).
__device__ __forceinline__ uint32_t gs_diff(uint32_t a, uint32_t b) { return sad4(a, b, 0u); }

// One band of one lane.  Lane idx = (band, piece) = (idx / pieces, idx % pieces).  add(cell, n): n more hits in a cell of the frame.
template <int BYTES, int STEP, bool VEC, class Add>
__device__ __forceinline__ void gs_band(const GridJob& jb, uint32_t idx, uint32_t field, Add add) {
    using P = GsPiece<BYTES, STEP, VEC>;
    constexpr int E = P::E, S = P::S;
    const long long row_elems = (long long)jb.cols * STEP;
    const uint32_t pieces = (uint32_t)((row_elems + E - 1) / E);
    const int rows = (jb.rows - (int)field + jb.fields - 1) / jb.fields;          // of this field
    const uint32_t band = idx / pieces, piece = idx - band * pieces;
    const int y0 = (int)band * GS_BAND;
    if (y0 >= rows) return;
    const long long g0 = (long long)piece * E;
    const uint8_t* plane = jb.src + (long long)field * jb.pitch;
    const long long pitch = jb.pitch * jb.fields;
    uint32_t a[E], b[E], c[E], d[E];          // the own samples of rows y - 2, y - 1, y, y + 1
    uint32_t row_cnt[(E + 3) / 4] = {}, col_cnt[GS_BAND / 4] = {};          // packed bytes: hits by own sample, hits by band row
#pragma unroll
    for (int e = 0; e < E; ++e) a[e] = b[e] = c[e] = d[e] = 0u;
#pragma unroll
    for (int j = -2; j <= GS_BAND; ++j) {
        const int rho = y0 + j;          // the row loaded now; row hits are its own, the column boundary is y = rho - 1
        uint32_t ext[P::N];
        const uint8_t* row = plane + (long long)min(max(rho, 0), rows - 1) * pitch;
        if (j >= 0 && j < GS_BAND) gs_load<BYTES, STEP, VEC, true>(jb, row, g0, row_elems, ext);
        else gs_load<BYTES, STEP, VEC, false>(jb, row, g0, row_elems, ext);
#pragma unroll
        for (int e = 0; e < E; ++e) a[e] = b[e], b[e] = c[e], c[e] = d[e], d[e] = ext[2 * S + e];
        if (j >= 0 && j < GS_BAND && rho < rows) {
            uint32_t h[E + 2 * S];          // h[i] = |ext[i + S] - ext[i]|
#pragma unroll
            for (int i = 0; i < E + 2 * S; ++i) h[i] = gs_diff(ext[i + S], ext[i]);
#pragma unroll
            for (int e = 0; e < E; ++e) {          // sample g = g0 + e of pixel x = g / S: 2 <= x <= cols - 2 iff 2 S <= g < row_elems - S
                const int g = (int)g0 + e;          // (a plane holds fewer than 2^31 samples)
                const bool hit = h[e + S] > h[e] + h[e + 2 * S] && h[e + S] <= jb.cap && g >= 2 * S && g < (int)row_elems - S;
                row_cnt[e / 4] += (uint32_t)hit << (8 * (e % 4));
            }
        }
        if (j >= 1) {
            const int y = rho - 1;
            if (y >= 2 && y <= rows - 2) {
                uint32_t hits = 0;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const uint32_t s = gs_diff(c[e], b[e]), l = gs_diff(b[e], a[e]), r = gs_diff(d[e], c[e]);
                    hits += (uint32_t)(s > l + r && s <= jb.cap && (VEC || g0 + e < row_elems));
                }
                col_cnt[(j - 1) / 4] += hits << (8 * ((j - 1) % 4));
            }
        }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const uint32_t n = (row_cnt[e / 4] >> (8 * (e % 4))) & 255u;
        if (n) add((int)((uint32_t)((g0 + e) / S) & 15u), n);
    }
#pragma unroll
    for (int k = 0; k < GS_BAND; ++k) {
        const uint32_t n = (col_cnt[k / 4] >> (8 * (k % 4))) & 255u;
        if (n) add(16 + ((y0 + k) & 15), n);
    }
}

template <int BYTES, int STEP, bool VEC>
__global__ __launch_bounds__(GS_THREADS) void grid_stats_kernel(GridJob jb, unsigned long long* __restrict__ out) {
    GridJob fr = jb;
    fr.src = jb.src + (long long)blockIdx.y * jb.stride;
    unsigned long long* cell = out + (long long)GS_CELLS * blockIdx.y;
#ifdef SAVSR_HOST_CHECK          // the host check runs one thread at a time: every thread adds its own counts
    gs_band<BYTES, STEP, VEC>(fr, blockIdx.x * GS_THREADS + threadIdx.x, blockIdx.z, [&](int k, uint32_t n) { atomicAdd(cell + k, (unsigned long long)n); });
#else
    __shared__ uint32_t part[GS_THREADS / 64][GS_CELLS];
    const uint32_t tid = threadIdx.x;
    if (tid < (GS_THREADS / 64) * GS_CELLS) (&part[0][0])[tid] = 0u;
    __syncthreads();
    uint32_t* wave_part = part[tid >> 6];
    gs_band<BYTES, STEP, VEC>(fr, blockIdx.x * GS_THREADS + tid, blockIdx.z, [&](int k, uint32_t n) { atomicAdd(wave_part + k, n); });
    __syncthreads();
    if (tid < GS_CELLS) {
        unsigned long long s = 0;
#pragma unroll
        for (int i = 0; i < GS_THREADS / 64; ++i) s += part[i][tid];
        if (s) atomicAdd(cell + tid, s);
    }
#endif
}

template <int BYTES, int STEP, bool VEC>
int gs_launch(const GridJob& jb, int nf, unsigned long long* out, hipStream_t st) {
    constexpr int E = GsPiece<BYTES, STEP, VEC>::E;
    const long long pieces = ((long long)jb.cols * STEP + E - 1) / E;
    const long long bands = ((jb.rows + jb.fields - 1) / jb.fields + GS_BAND - 1) / GS_BAND;          // of field 0, which has the most rows
    hipLaunchKernelGGL((grid_stats_kernel<BYTES, STEP, VEC>), dim3(blocks(bands * pieces, GS_THREADS), (unsigned)nf, (unsigned)jb.fields),
                       dim3(GS_THREADS), 0, st, jb, out);
    return check_launch("grid_stats_kernel");
}

template <int BYTES, bool VEC>
int gs_launch_step(const GridJob& jb, int nf, unsigned long long* out, hipStream_t st) {
    switch (jb.step) {
        case 1: return gs_launch<BYTES, 1, VEC>(jb, nf, out, st);
        case 2: return gs_launch<BYTES, 2, VEC>(jb, nf, out, st);
        case 3: return gs_launch<BYTES, 3, VEC>(jb, nf, out, st);
        default: return gs_launch<BYTES, 4, VEC>(jb, nf, out, st);
    }
}

// The body of the two entries.  cols: pixels of a row; step: samples of a pixel.
template <int BYTES>
int grid_stats(const char* who, const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step, int depth,
               int interlaced, int cap, int64_t* out, void* stream) {
    constexpr MatrixRule rule{1, 0, nullptr, "", false};
    if (step < 1 || step > GS_MAX_STEP) return refuse(who, "step 1 .. 4 (the samples of a pixel)");
    if (cols < 1) return refuse(who, "a row holds at least one sample");
    const int64_t row_bytes = (int64_t)BYTES * cols * step;
    if (const char* why = check_matrix(rule, frames, n_frames, frame_bytes, plane_offset, rows, row_bytes, 0, 0, n_frames)) return refuse(who, why);
    if (BYTES == 2)
        if (int rc = check_samples16(who, depth, frames, frame_bytes, plane_offset)) return rc;
    if (const char* why = check_cells(out, true)) return refuse(who, why);
    if (interlaced != 0 && interlaced != 1) return refuse(who, "interlaced 0 or 1");
    if (cap < 0 || cap > 255) return refuse(who, "cap 0 .. 255 (the largest step that counts, in 8-bit codes)");
    const GridJob jb{frames + plane_offset, frame_bytes, row_bytes, rows, cols, step, interlaced && rows > 1 ? 2 : 1, (1u << depth) - 1u, depth - 8, (uint32_t)cap};
    const bool vec = aligned16(jb.src, jb.stride, jb.pitch);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return for_frame_chunks(n_frames, FM_MAX_FRAMES, [&](int f0, int nf) {
        GridJob part = jb;
        part.src = jb.src + (long long)f0 * jb.stride;
        unsigned long long* cells = reinterpret_cast<unsigned long long*>(out) + (long long)GS_CELLS * f0;
        return vec ? gs_launch_step<BYTES, true>(part, nf, cells, st) : gs_launch_step<BYTES, false>(part, nf, cells, st);
    });
}

}  // namespace
}  // namespace savsr

using namespace savsr;

extern "C" int savsr_video_grid_stats_u8(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step,
                                         int interlaced, int cap, int64_t* out, void* stream) {
    return grid_stats<1>("video_grid_stats_u8", frames, n_frames, frame_bytes, plane_offset, rows, cols, step, 8, interlaced, cap, out, stream);
}

extern "C" int savsr_video_grid_stats_u16(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step,
                                          int depth, int interlaced, int cap, int64_t* out, void* stream) {
    return grid_stats<2>("video_grid_stats_u16", frames, n_frames, frame_bytes, plane_offset, rows, cols, step, depth, interlaced, cap, out, stream);
}
