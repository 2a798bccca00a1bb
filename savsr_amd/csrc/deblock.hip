// Deblocking in front of the network (ABI 52): a weak / strong filter across the edges of a fixed block grid, pass X then pass Y, in
// integers (savsr_amd/deblock.py `deblock_matrix` / `deblock_fields` is the specification; the kernels equal it bit for bit).
//
//   _u8    planes of rows x (cols * step) bytes; sample x of a row meets samples x +- j * step only (step = the channels of packed frames)
//   _u16   the same in little-endian 16-bit samples, every sample read as min(s, 2^depth - 1)
//
// One launch per call, both passes in it, grid = (tile column, tile row, frame), 256 lanes; global memory is read once (plus the halo)
// and written once, and pass X's result never leaves LDS.  A workgroup owns a tile of 32 frame rows x T samples whose origin lies on the
// block grid (T = 256 / step, 64 at step 3: a multiple of 16, and 32 is one, so every block's edges and both fields' edges fall on the
// same places in every tile).  A grid origin (oy, ox) (ABI 53, the `_o` entries) keeps that: the kernel works in coordinates shifted by
// (block - o) % block, so the tile grid starts up to block - 1 samples before the plane -- tile origins tx0, ty0 may be negative, the
// staging clamp reads the plane's first row and column there, nothing of it is stored -- and every edge test and LDS index is what it
// was.  Four phases with a barrier between them:
//   stage   the tile plus its halo into LDS as 16-bit values, coordinates clamped to the plane (to the field, row-wise, in field mode),
//           so the border rule costs nothing afterwards.  A lane loads a dword (4 bytes / 2 words) where the dword lies inside the row
//           and is aligned, and single samples elsewhere (the clamped halo, rows of a plane whose pitch or base is not a multiple of 4).
//   pass X  in place in LDS on every staged row: one lane per (row, vertical edge, channel), lanes along the rows -- the pitch is 145
//           dwords, odd, so the 32 lanes of a bank group hit 32 banks.
//   pass Y  in place on the tile's own columns: one lane per (column, horizontal edge, field), lanes along the row: consecutive 16-bit
//           words, two lanes a bank word, no conflict.
//   store   the tile's own samples, a dword per lane where aligned.
// In place is sound because the samples of two edges of one pass never overlap (deblock.py has the argument), the clamped copies beyond
// the plane included: they belong to the last edge alone and are never stored.
//
// The halo.  Pass Y's output at field row e - 3 (strong's P2) reads pass X's result at rows e - 3 .. e + 2: up to 5 rows away, on the far
// side of edge e.  A tile's own rows begin at an edge e0 and end at the next tile's e1: its rows e0 .. e0 + 2 (the Q side of e0) need
// e0 - 3 .. e0 - 1, and its rows e1 - 3 .. e1 - 1 (the P side of e1) need e1 .. e1 + 2 -- 3 field rows above and below, which are 6 frame
// rows in field mode, every one with pass X applied, which is why pass X runs on the halo rows too.  The same holds along a row with 3
// samples left and right.  44 rows x 290 words: 25 520 bytes of LDS.
#include "common.hpp"
#include "video_samples.hpp"
#include "field_matrix.hpp"

#include <cstdint>

namespace savsr {
namespace {

typedef uint32_t __attribute__((may_alias)) dbk_dword;          // a dword of samples, in memory or in the staged tile

constexpr int DBK_THREADS = 256;
constexpr int DBK_TILE_ROWS = 32;
constexpr int DBK_HALO = 3;                     // samples / field rows a filter reaches on either side of an edge
constexpr int DBK_MAX_STEP = 4;
constexpr int DBK_LEFT = DBK_HALO * DBK_MAX_STEP;                      // words in front of a staged row's first own sample (a multiple of 4)
constexpr int DBK_PITCH = 290;                  // words of a staged row (>= 12 + 256 + 12), 145 dwords
constexpr int DBK_LDS_ROWS = DBK_TILE_ROWS + 4 * DBK_HALO;            // the tile and 6 halo frame rows either way (field mode)
constexpr int DBK_LDS_WORDS = DBK_LDS_ROWS * DBK_PITCH;
constexpr int DBK_BIAS = 32;                    // samples added before a division by step so that it rounds down (> 15 + 3 + 3)

struct DeblockJob {
    const uint8_t* src;          // the plane of frame 0
    uint8_t* dst;                // the plane of output frame 0
    long long stride, dst_stride, pitch;          // bytes between frames (either side) and between rows
    int rows, cols, step;
    int block, lb, strong;       // lb: log2 block
    int a, b;                    // A and Bt, in the depth's codes
    int top;                     // 2^depth - 1
    int shift_x, shift_y;        // (block - origin) % block: the tile grid starts this many samples / frame rows before the plane
};

// Samples of a tile's row at `step` samples a pixel: 256 / step, 64 at step 3.
constexpr int dbk_tile_cols(int step) { return step == 3 ? 64 : 256 / step; }

// One edge of one line: s = P2 P1 P0 Q0 Q1 Q2 -> the filtered six, true where the conditions hold (s is left alone where not).
__device__ __forceinline__ bool dbk_edge(int (&s)[6], bool strong, int A, int Bt, int top) {
    const int d = s[3] - s[2], ad = d < 0 ? -d : d;
    if (ad >= A || abs(s[2] - s[1]) >= Bt || abs(s[3] - s[4]) >= Bt) return false;
    if (strong && (abs(s[1] - s[0]) >= Bt || abs(s[4] - s[5]) >= Bt)) return false;
    const int t2 = d < 0 ? -(ad >> 1) : ad >> 1, t4 = d < 0 ? -(ad >> 2) : ad >> 2, t8 = d < 0 ? -(ad >> 3) : ad >> 3;
    if (strong) {
        s[0] += t8, s[1] += t4, s[5] -= t8, s[4] -= t4;
    } else {
        s[1] += t8, s[4] -= t8;
    }
    s[2] += t2, s[3] -= t2;
#pragma unroll
    for (int j = 0; j < 6; ++j) s[j] = min(max(s[j], 0), top);
    return true;
}

// The six samples at words p - 3 q .. p + 2 q of the staged tile, filtered in place.
__device__ __forceinline__ void dbk_edge_lds(uint16_t* p, int q, bool strong, const DeblockJob& jb) {
    int s[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) s[j] = p[(j - DBK_HALO) * q];
    if (!dbk_edge(s, strong, jb.a, jb.b, jb.top)) return;
#pragma unroll
    for (int j = 0; j < 6; ++j)
        if (strong || (j != 0 && j != 5)) p[(j - DBK_HALO) * q] = (uint16_t)s[j];
}

// The plane row behind staged row r of the tile at frame row ty0: frame row ty0 - 3 G + r, clamped inside its own field.
template <int G>
__device__ __forceinline__ int dbk_plane_row(const DeblockJob& jb, int ty0, int r) {
    const int p = r & (G - 1);
    const int f = ty0 / G - DBK_HALO + r / G, nf = (jb.rows - p + G - 1) / G;          // the field row; the field's rows
    return min(max(min(f, nf - 1), 0) * G + p, jb.rows - 1);
}

// Phase 1: row element E0 - 3 step + ... of every staged row into LDS (word LEFT + s of a staged row is row element E0 + s).
// (The pixel's samples STEP and the field count G are template parameters so that every division below is by a constant.)
template <int BYTES, int STEP, int G>
__device__ __forceinline__ void dbk_stage(const DeblockJob& jb, const uint8_t* plane, uint16_t* tile, int tid, int tx0, int ty0) {
    constexpr int GE = 4 / BYTES;          // samples of a dword
    constexpr int step = STEP, nrows = DBK_TILE_ROWS + 2 * DBK_HALO * G;
    constexpr int c_lo = (DBK_LEFT - DBK_HALO * step) / GE * GE, c_hi = DBK_LEFT + dbk_tile_cols(STEP) * step + DBK_HALO * step;
    constexpr int ngroups = (c_hi - c_lo + GE - 1) / GE;
    const int E0 = tx0 * step, row_elems = jb.cols * step;
    for (int i = tid; i < nrows * ngroups; i += DBK_THREADS) {
        const int r = i / ngroups, c0 = c_lo + (i - r * ngroups) * GE;
        const uint8_t* row = plane + (long long)dbk_plane_row<G>(jb, ty0, r) * jb.pitch;
        const int g0 = E0 + c0 - DBK_LEFT;
        uint32_t v[GE];
        if (g0 >= 0 && g0 + GE <= row_elems && ((reinterpret_cast<uintptr_t>(row) + (uintptr_t)g0 * BYTES) & 3) == 0) {
            const uint32_t w = *reinterpret_cast<const dbk_dword*>(row + (long long)g0 * BYTES);
            if constexpr (BYTES == 1) {
                v[0] = w & 255u, v[1] = (w >> 8) & 255u, v[2] = (w >> 16) & 255u, v[3] = w >> 24;
            } else {
                v[0] = min(w & 0xffffu, (uint32_t)jb.top), v[1] = min(w >> 16, (uint32_t)jb.top);
            }
        } else {
#pragma unroll
            for (int k = 0; k < GE; ++k) {          // element g is channel g mod step of sample g div step, the sample clamped to the row
                const int gs = g0 + k + DBK_BIAS * step, x = min(max(gs / step - DBK_BIAS, 0), jb.cols - 1), ch = gs % step;
                const long long e = (long long)x * step + ch;
                if constexpr (BYTES == 1) v[k] = row[e];
                else v[k] = min((uint32_t)reinterpret_cast<const uint16_t*>(row)[e], (uint32_t)jb.top);
            }
        }
        dbk_dword* out = reinterpret_cast<dbk_dword*>(tile + r * DBK_PITCH + c0);          // (c0 and the pitch are even)
        if constexpr (BYTES == 1) {
            out[0] = v[0] | (v[1] << 16), out[1] = v[2] | (v[3] << 16);
        } else {
            out[0] = v[0] | (v[1] << 16);
        }
    }
}

// Phase 2: the vertical edges tx0 + k block, k = 0 .. tcols / block, of every staged row and channel.
template <int STEP, int G>
__device__ __forceinline__ void dbk_pass_x(const DeblockJob& jb, uint16_t* tile, int tid, int tx0) {
    constexpr int step = STEP, nrows = DBK_TILE_ROWS + 2 * DBK_HALO * G;
    const int nedges = (dbk_tile_cols(STEP) >> jb.lb) + 1;
    const bool strong = jb.strong && jb.block >= 8;
    for (int i = tid; i < nrows * nedges * step; i += DBK_THREADS) {
        const int r = i % nrows, rest = i / nrows, ch = rest % step, k = rest / step;
        const int e = tx0 + (k << jb.lb);
        if (e < 1 || e > jb.cols - 1) continue;
        dbk_edge_lds(tile + r * DBK_PITCH + DBK_LEFT + (k << jb.lb) * step + ch, step, strong, jb);
    }
}

// Phase 3: the horizontal edges of either field on the tile's own columns.  Field row ty0 / G - 3 + j of parity p is staged row G j + p.
template <int STEP, int G>
__device__ __forceinline__ void dbk_pass_y(const DeblockJob& jb, uint16_t* tile, int tid, int tx0, int ty0) {
    const int by = jb.block / G, lby = jb.lb - (G - 1);
    if (by < 4) return;          // (the fields of block 4: a 2-row block has no interior)
    const bool strong = jb.strong && by >= 8;
    constexpr int te = dbk_tile_cols(STEP) * STEP;
    const int own = min(te, jb.cols * STEP - tx0 * STEP), nedges = ((DBK_TILE_ROWS / G) >> lby) + 1;
    for (int i = tid; i < te * nedges * G; i += DBK_THREADS) {
        const int c = i % te, rest = i / te, p = rest % G, k = rest / G;
        const int e = ty0 / G + k * by, nf = (jb.rows - p + G - 1) / G;
        if (c >= own || e < 1 || e > nf - 1) continue;
        dbk_edge_lds(tile + (G * (DBK_HALO + k * by) + p) * DBK_PITCH + DBK_LEFT + c, G * DBK_PITCH, strong, jb);
    }
}

// Phase 4: the tile's own samples.  SHIFTED: the tile grid starts before the plane (a grid origin), so a tile's first rows and samples may
// lie in front of it; without it the code is what it was.
template <int BYTES, int STEP, int G, bool SHIFTED>
__device__ __forceinline__ void dbk_store(const DeblockJob& jb, uint8_t* plane, const uint16_t* tile, int tid, int tx0, int ty0) {
    constexpr int GE = 4 / BYTES, te = dbk_tile_cols(STEP) * STEP, ngroups = te / GE;
    const int E0 = tx0 * STEP, row_elems = jb.cols * STEP;
    for (int i = tid; i < DBK_TILE_ROWS * ngroups; i += DBK_THREADS) {
        const int r = i / ngroups, c0 = (i - r * ngroups) * GE, y = ty0 + r, g0 = E0 + c0;
        if (y >= jb.rows || g0 >= row_elems || (SHIFTED && (y < 0 || g0 + GE <= 0))) continue;
        const uint16_t* in = tile + (DBK_HALO * G + r) * DBK_PITCH + DBK_LEFT + c0;
        uint8_t* row = plane + (long long)y * jb.pitch;
        if ((!SHIFTED || g0 >= 0) && g0 + GE <= row_elems && ((reinterpret_cast<uintptr_t>(row) + (uintptr_t)g0 * BYTES) & 3) == 0) {
            const dbk_dword* pair = reinterpret_cast<const dbk_dword*>(in);          // (LEFT, c0 and the pitch are even: two words a read)
            uint32_t w = pair[0];
            if constexpr (BYTES == 1) {
                const uint32_t hi = pair[1];
                w = (w & 255u) | ((w >> 8) & 0xff00u) | ((hi & 255u) << 16) | ((hi >> 16) << 24);
            }
            *reinterpret_cast<dbk_dword*>(row + (long long)g0 * BYTES) = w;
        } else {
#pragma unroll
            for (int k = 0; k < GE; ++k) {
                if (g0 + k >= row_elems) break;
                if (SHIFTED && g0 + k < 0) continue;
                if constexpr (BYTES == 1) row[g0 + k] = (uint8_t)in[k];
                else reinterpret_cast<uint16_t*>(row)[g0 + k] = in[k];
            }
        }
    }
}

#ifdef SAVSR_HOST_CHECK
// The host check's form: the four phases as they are, lane after lane where the GPU has a barrier, on a heap tile of the exact size
// (the launch has one thread per workgroup).
template <int BYTES, int STEP, int G, bool SHIFTED>
__global__ void deblock_kernel(DeblockJob jb) {
    uint16_t* tile = new uint16_t[DBK_LDS_WORDS];
    for (int i = 0; i < DBK_LDS_WORDS; ++i) tile[i] = 0xDEAD;
    const int tx0 = (int)blockIdx.x * dbk_tile_cols(STEP) - (SHIFTED ? jb.shift_x : 0), ty0 = (int)blockIdx.y * DBK_TILE_ROWS - (SHIFTED ? jb.shift_y : 0);
    const uint8_t* plane = jb.src + (long long)blockIdx.z * jb.stride;
    for (int tid = 0; tid < DBK_THREADS; ++tid) dbk_stage<BYTES, STEP, G>(jb, plane, tile, tid, tx0, ty0);
    for (int tid = 0; tid < DBK_THREADS; ++tid) dbk_pass_x<STEP, G>(jb, tile, tid, tx0);
    for (int tid = 0; tid < DBK_THREADS; ++tid) dbk_pass_y<STEP, G>(jb, tile, tid, tx0, ty0);
    for (int tid = 0; tid < DBK_THREADS; ++tid) dbk_store<BYTES, STEP, G, SHIFTED>(jb, jb.dst + (long long)blockIdx.z * jb.dst_stride, tile, tid, tx0, ty0);
    delete[] tile;
}
constexpr int DBK_LAUNCH_THREADS = 1;
#else
template <int BYTES, int STEP, int G, bool SHIFTED>
__global__ __launch_bounds__(DBK_THREADS) void deblock_kernel(DeblockJob jb) {
    __shared__ __attribute__((aligned(16))) uint16_t tile[DBK_LDS_WORDS];
    const int tid = (int)threadIdx.x, tx0 = (int)blockIdx.x * dbk_tile_cols(STEP) - (SHIFTED ? jb.shift_x : 0);
    const int ty0 = (int)blockIdx.y * DBK_TILE_ROWS - (SHIFTED ? jb.shift_y : 0);
    dbk_stage<BYTES, STEP, G>(jb, jb.src + (long long)blockIdx.z * jb.stride, tile, tid, tx0, ty0);
    __syncthreads();
    dbk_pass_x<STEP, G>(jb, tile, tid, tx0);
    __syncthreads();
    dbk_pass_y<STEP, G>(jb, tile, tid, tx0, ty0);
    __syncthreads();
    dbk_store<BYTES, STEP, G, SHIFTED>(jb, jb.dst + (long long)blockIdx.z * jb.dst_stride, tile, tid, tx0, ty0);
}
constexpr int DBK_LAUNCH_THREADS = DBK_THREADS;
#endif

template <int BYTES, int STEP, int G>
int dbk_launch(const DeblockJob& jb, int nf, hipStream_t st) {
    const dim3 grid(blocks(jb.cols + jb.shift_x, dbk_tile_cols(STEP)), blocks(jb.rows + jb.shift_y, DBK_TILE_ROWS), (unsigned)nf);
    if (jb.shift_x || jb.shift_y) hipLaunchKernelGGL((deblock_kernel<BYTES, STEP, G, true>), grid, dim3(DBK_LAUNCH_THREADS), 0, st, jb);
    else hipLaunchKernelGGL((deblock_kernel<BYTES, STEP, G, false>), grid, dim3(DBK_LAUNCH_THREADS), 0, st, jb);          // the kernel as it was
    return check_launch("deblock_kernel");
}

template <int BYTES, int G>
int dbk_launch_step(const DeblockJob& jb, int nf, hipStream_t st) {
    switch (jb.step) {
        case 1: return dbk_launch<BYTES, 1, G>(jb, nf, st);
        case 2: return dbk_launch<BYTES, 2, G>(jb, nf, st);
        case 3: return dbk_launch<BYTES, 3, G>(jb, nf, st);
        default: return dbk_launch<BYTES, 4, G>(jb, nf, st);
    }
}

// The body of the four entries.  cols: pixels of a row; step: samples of a pixel; (origin_y, origin_x): the grid's origin, (0, 0) from the
// entries that have none.
template <int BYTES>
int deblock(const char* who, const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step, int depth,
            int block, int strong, int interlaced, int thr_a, int thr_b, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset, void* stream,
            int origin_y = 0, int origin_x = 0) {
    constexpr MatrixRule rule{1, 0, nullptr, "", false};
    if (step < 1 || step > DBK_MAX_STEP) return refuse(who, "step 1 .. 4 (the samples of a pixel)");
    if (cols < 1) return refuse(who, "a row holds at least one sample");
    const int64_t row_bytes = (int64_t)BYTES * cols * step;
    const char* why = check_matrix(rule, frames && out ? frames : nullptr, n_frames, frame_bytes, plane_offset, rows, row_bytes, 0, 0, n_frames, out_plane_offset);
    if (!why) why = check_out_plane(out_frame_bytes, out_plane_offset, rows, row_bytes);
    if (why) return refuse(who, why);
    if (BYTES == 2)
        if (int rc = check_samples16(who, depth, frames, frame_bytes, plane_offset, true, out, out_frame_bytes, out_plane_offset)) return rc;
    if (block != 4 && block != 8 && block != 16) return refuse(who, "block 4, 8 or 16");
    if ((strong != 0 && strong != 1) || (interlaced != 0 && interlaced != 1)) return refuse(who, "strong and interlaced 0 or 1");
    const int max_thr = 255 << (depth - 8);
    if (thr_a < 0 || thr_a > max_thr || thr_b < 0 || thr_b > max_thr) return refuse(who, "thresholds 0 .. 255 << (depth - 8)");
    if (origin_y < 0 || origin_y >= block || origin_x < 0 || origin_x >= block) return refuse(who, "origin_y and origin_x 0 .. block - 1");
    if (interlaced && (origin_y & 1)) return refuse(who, "origin_y even with interlaced (an odd origin swaps the fields' parity)");
    if (out < frames + (int64_t)n_frames * frame_bytes && frames < out + (int64_t)n_frames * out_frame_bytes)
        return refuse(who, "the source frames and the output overlap");
    const DeblockJob jb{frames + plane_offset, out + out_plane_offset, frame_bytes, out_frame_bytes, row_bytes, rows, cols, step,
                        block, block == 4 ? 2 : block == 8 ? 3 : 4, strong, thr_a, thr_b, (1 << depth) - 1,
                        (block - origin_x) % block, (block - origin_y) % block};
    hipStream_t st = static_cast<hipStream_t>(stream);
    return for_frame_chunks(n_frames, FM_MAX_FRAMES, [&](int f0, int nf) {
        DeblockJob part = jb;
        part.src = jb.src + (long long)f0 * jb.stride;
        part.dst = jb.dst + (long long)f0 * jb.dst_stride;
        return interlaced ? dbk_launch_step<BYTES, 2>(part, nf, st) : dbk_launch_step<BYTES, 1>(part, nf, st);
    });
}

}  // namespace
}  // namespace savsr

using namespace savsr;

extern "C" int savsr_video_deblock_u8(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step,
                                      int block, int strong, int interlaced, int thr_a, int thr_b, uint8_t* out, int64_t out_frame_bytes,
                                      int64_t out_plane_offset, void* stream) {
    return deblock<1>("video_deblock_u8", frames, n_frames, frame_bytes, plane_offset, rows, cols, step, 8, block, strong, interlaced, thr_a, thr_b, out,
                      out_frame_bytes, out_plane_offset, stream);
}

extern "C" int savsr_video_deblock_u16(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step,
                                       int depth, int block, int strong, int interlaced, int thr_a, int thr_b, uint8_t* out, int64_t out_frame_bytes,
                                       int64_t out_plane_offset, void* stream) {
    return deblock<2>("video_deblock_u16", frames, n_frames, frame_bytes, plane_offset, rows, cols, step, depth, block, strong, interlaced, thr_a, thr_b,
                      out, out_frame_bytes, out_plane_offset, stream);
}

extern "C" int savsr_video_deblock_u8_o(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step,
                                        int block, int strong, int interlaced, int thr_a, int thr_b, uint8_t* out, int64_t out_frame_bytes,
                                        int64_t out_plane_offset, int origin_y, int origin_x, void* stream) {
    return deblock<1>("video_deblock_u8_o", frames, n_frames, frame_bytes, plane_offset, rows, cols, step, 8, block, strong, interlaced, thr_a, thr_b, out,
                      out_frame_bytes, out_plane_offset, stream, origin_y, origin_x);
}

extern "C" int savsr_video_deblock_u16_o(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step,
                                         int depth, int block, int strong, int interlaced, int thr_a, int thr_b, uint8_t* out, int64_t out_frame_bytes,
                                         int64_t out_plane_offset, int origin_y, int origin_x, void* stream) {
    return deblock<2>("video_deblock_u16_o", frames, n_frames, frame_bytes, plane_offset, rows, cols, step, depth, block, strong, interlaced, thr_a, thr_b,
                      out, out_frame_bytes, out_plane_offset, stream, origin_y, origin_x);
}
