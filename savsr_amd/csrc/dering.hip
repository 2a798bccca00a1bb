// Deringing in front of the network (ABI 54): a direction search per 8 x 8 block and a constrained filter along and across the direction,
// in integers (savsr_amd/dering.py `dering_matrix` / `dering_fields` is the specification; the kernels equal it bit for bit).
//
//   _u8    planes of rows x (cols * step) bytes; sample x of a row meets samples x +- j * step only (step = the channels of packed frames)
//   _u16   the same in little-endian 16-bit samples, every sample read as min(s, 2^depth - 1)
//
// One launch per call, grid = (tile column, tile row, frame), 256 lanes; global memory is read once (plus the halo) and written once.  A
// workgroup owns a tile of 32 frame rows x T pixels (T = 256 / step, 64 at step 3: multiples of 8, and 32 rows are 4 blocks, or 2 blocks of
// either field), so a tile's origin lies on the 8-grid of the plane, and of both fields in field mode.  Three phases, a barrier between:
//   stage      the tile plus a halo of 2 samples and 2 field rows into LDS as 16-bit values, coordinates clamped to the plane (to the
//              field, row-wise, in field mode): the clamp of the rule's at() and the clamped copies of a partial block cost nothing
//              afterwards.  A lane loads a dword (4 bytes / 2 words) where the dword lies inside the row and is aligned, single samples
//              elsewhere.
//   direction  one lane per block (a block: 8 x 8 samples of one channel and one field; at most 128 a tile): its 64 samples from LDS,
//              the eight sets of line sums, the costs, dir and var, and from var the primary strength -- once per block, not per sample --
//              as one LDS word (dir | P8 << 3).  Lanes run along the blocks of a row of blocks: 8 * step words apart, which is 2-way on
//              the 64 banks at step 1 and 2 (lanes l and l + 16 of a 32-lane group share a bank) and 4-way at step 4; the phase has 64
//              reads a lane against the filter's 13 a sample x 8 samples a lane and is not the larger one.
//   filter     one lane per dword of output (4 bytes / 2 words): x and its up to 12 taps from LDS, lanes along the row (consecutive
//              16-bit words: no conflict), the result straight to global memory, a dword per lane where aligned.  Nothing filtered is
//              written back to LDS: no output is ever read.
// Divergence: a wave's 64 lanes cover 8 blocks (4 at 16 bits) of one row; with S > 0 every block takes the secondary taps and only the
// primary ones depend on the block (P8 = 0 on flat blocks), so the lanes of a flat block wait for their neighbours' four primary taps;
// with S = 0 a flat block's lanes copy and wait for all of it.  The taps' offsets come from a select chain on dir, not from a table in
// memory.  40 rows x 274 words + 128 words: 22 176 bytes of LDS.
#include "common.hpp"
#include "video_samples.hpp"
#include "field_matrix.hpp"

#include <cstdint>

namespace savsr {
namespace {

typedef uint32_t __attribute__((may_alias)) drg_dword;          // a dword of samples, in memory or in the staged tile

constexpr int DRG_THREADS = 256;
constexpr int DRG_TILE_ROWS = 32;
constexpr int DRG_HALO = 2;                     // samples / field rows a tap reaches
constexpr int DRG_MAX_STEP = 4;
constexpr int DRG_LEFT = DRG_HALO * DRG_MAX_STEP;                      // words in front of a staged row's first own sample (a multiple of 4)
constexpr int DRG_PITCH = 274;                  // words of a staged row (>= 8 + 256 + 8), 137 dwords
constexpr int DRG_LDS_ROWS = DRG_TILE_ROWS + 4 * DRG_HALO;            // the tile and 4 halo frame rows either way (field mode)
constexpr int DRG_LDS_WORDS = DRG_LDS_ROWS * DRG_PITCH;
constexpr int DRG_MAX_BLOCKS = 128;             // blocks of a tile: 4 rows of blocks x (T / 8) x step
constexpr int DRG_BIAS = 32;                    // samples added before a division by step so that it rounds down
constexpr int DRG_MAX_PRI = 15, DRG_MAX_SEC = 4;

struct DeringJob {
    const uint8_t* src;          // the plane of frame 0
    uint8_t* dst;                // the plane of output frame 0
    long long stride, dst_stride, pitch;          // bytes between frames (either side) and between rows
    int rows, cols, step;
    int pri8, sec;               // p in 8-bit codes; S in the depth's codes
    int shift, damping;          // depth - 8; Dd = D + shift
    int top;                     // 2^depth - 1
};

// Pixels of a tile's row at `step` samples a pixel: 256 / step, 64 at step 3.
constexpr int drg_tile_cols(int step) { return step == 3 ? 64 : 256 / step; }

__device__ __forceinline__ int drg_msb(int n) { return 31 - __builtin_clz((unsigned)n); }          // n >= 1

// The line of direction k that sample (i, j) of a block belongs to.
__device__ __forceinline__ constexpr int drg_line(int k, int i, int j) {
    return k == 0 ? i + j : k == 1 ? i + j / 2 : k == 2 ? i : k == 3 ? 3 + i - j / 2 : k == 4 ? 7 + i - j : k == 5 ? 3 - i / 2 + j : k == 6 ? j : i / 2 + j;
}

// Step 1 of the rule: b = the block's 64 samples on the 8-bit scale minus 128 -> dir, var.  (Every index is a constant once unrolled.)
__device__ __forceinline__ void drg_direction(const int (&b)[8][8], int& dir, int& var) {
    constexpr int W[9] = {0, 840, 420, 280, 210, 168, 140, 120, 105};
    int cost[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int part[15];
#pragma unroll
        for (int n = 0; n < 15; ++n) part[n] = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int j = 0; j < 8; ++j) part[drg_line(k, i, j)] += b[i][j];
        }
        int c = 0;
        if (k == 2 || k == 6) {
#pragma unroll
            for (int i = 0; i < 8; ++i) c += part[i] * part[i];
            c *= 105;
        } else if (k == 0 || k == 4) {
#pragma unroll
            for (int i = 0; i < 7; ++i) c += (part[i] * part[i] + part[14 - i] * part[14 - i]) * W[i + 1];
            c += 105 * part[7] * part[7];
        } else {
#pragma unroll
            for (int j = 0; j < 5; ++j) c += part[3 + j] * part[3 + j];
            c *= 105;
#pragma unroll
            for (int j = 0; j < 3; ++j) c += (part[j] * part[j] + part[10 - j] * part[10 - j]) * W[2 * j + 2];
        }
        cost[k] = c;
    }
    int best = cost[0], across = cost[4];
    dir = 0;
#pragma unroll
    for (int k = 1; k < 8; ++k)
        if (cost[k] > best) best = cost[k], across = cost[(k + 4) & 7], dir = k;          // (strictly larger: the smallest index of equal maxima)
    var = (best - across) >> 10;
}

// Step 2: P8 of a block.
__device__ __forceinline__ int drg_primary8(int var, int p) {
    if (var == 0) return 0;
    const int i = var < 64 ? 0 : min(drg_msb(var >> 6), 12);
    return (p * (4 + i) + 8) >> 4;
}

// The taps of direction k as word offsets of the staged tile: tap 0 in the low half, tap 1 in the high half, each a signed 16-bit value;
// qy: words between two rows of the plane (of the field), qx: words between two pixels.
__device__ __forceinline__ void drg_taps(int k, int qy, int qx, int& o0, int& o1) {
    // (dy0, dx0, dy1, dx1) + 2, three bits each
    constexpr uint32_t T[8] = {1 | 3 << 3 | 0 << 6 | 4 << 9, 2 | 3 << 3 | 1 << 6 | 4 << 9, 2 | 3 << 3 | 2 << 6 | 4 << 9, 2 | 3 << 3 | 3 << 6 | 4 << 9,
                               3 | 3 << 3 | 4 << 6 | 4 << 9, 3 | 2 << 3 | 4 << 6 | 3 << 9, 3 | 2 << 3 | 4 << 6 | 2 << 9, 3 | 2 << 3 | 4 << 6 | 1 << 9};
    uint32_t t = T[0];
#pragma unroll
    for (int n = 1; n < 8; ++n) t = k == n ? T[n] : t;
    o0 = ((int)(t & 7u) - 2) * qy + ((int)((t >> 3) & 7u) - 2) * qx;
    o1 = ((int)((t >> 6) & 7u) - 2) * qy + ((int)((t >> 9) & 7u) - 2) * qx;
}

__device__ __forceinline__ int drg_con(int delta, int T, int q) {
    const int ad = delta < 0 ? -delta : delta, m = min(ad, max(0, T - (ad >> q)));
    return delta < 0 ? -m : m;
}

// One class of taps around the staged sample at c: +- o0 with weight w0, +- o1 with weight w1.
__device__ __forceinline__ void drg_class(const uint16_t* c, int x, int o0, int o1, int w0, int w1, int T, int q, int& sum, int& lo, int& hi) {
    const int a = c[o0], b = c[-o0], d = c[o1], e = c[-o1];
    sum += w0 * (drg_con(a - x, T, q) + drg_con(b - x, T, q)) + w1 * (drg_con(d - x, T, q) + drg_con(e - x, T, q));
    lo = min(min(lo, min(a, b)), min(d, e));
    hi = max(max(hi, max(a, b)), max(d, e));
}

// Step 3 for the staged sample at c of a block with `info` = dir | P8 << 3.
__device__ __forceinline__ int drg_sample(const DeringJob& jb, const uint16_t* c, int info, int qy, int qx) {
    const int x = c[0], dir = info & 7, P8 = info >> 3, P = P8 << jb.shift, S = jb.sec, Dd = jb.damping + jb.shift;
    if (P == 0 && S == 0) return x;
    int sum = 0, lo = x, hi = x, o0, o1;
    if (P > 0) {
        drg_taps(dir, qy, qx, o0, o1);
        drg_class(c, x, o0, o1, P8 & 1 ? 3 : 4, P8 & 1 ? 3 : 2, P, max(0, Dd - drg_msb(P)), sum, lo, hi);
    }
    if (S > 0) {
        const int q = max(0, Dd - drg_msb(S));
        drg_taps((dir + 2) & 7, qy, qx, o0, o1);
        drg_class(c, x, o0, o1, 2, 1, S, q, sum, lo, hi);
        drg_taps((dir + 6) & 7, qy, qx, o0, o1);
        drg_class(c, x, o0, o1, 2, 1, S, q, sum, lo, hi);
    }
    return min(max(x + ((8 + sum - (sum < 0)) >> 4), lo), hi);
}

// The plane row behind staged row r of the tile at frame row ty0: field row ty0 / G - 2 + r / G of parity r mod G, clamped inside its field.
template <int G>
__device__ __forceinline__ int drg_plane_row(const DeringJob& jb, int ty0, int r) {
    const int p = r & (G - 1);
    const int f = ty0 / G - DRG_HALO + r / G, nf = (jb.rows - p + G - 1) / G;          // the field row; the field's rows
    return min(max(min(f, nf - 1), 0) * G + p, jb.rows - 1);
}

// Phase 1: row element E0 - 2 step + ... of every staged row into LDS (word LEFT + s of a staged row is row element E0 + s).
template <int BYTES, int STEP, int G>
__device__ __forceinline__ void drg_stage(const DeringJob& jb, const uint8_t* plane, uint16_t* tile, int tid, int tx0, int ty0) {
    constexpr int GE = 4 / BYTES;          // samples of a dword
    constexpr int step = STEP, nrows = DRG_TILE_ROWS + 2 * DRG_HALO * G;
    constexpr int c_lo = (DRG_LEFT - DRG_HALO * step) / GE * GE, c_hi = DRG_LEFT + drg_tile_cols(STEP) * step + DRG_HALO * step;
    constexpr int ngroups = (c_hi - c_lo + GE - 1) / GE;
    static_assert(c_lo + ngroups * GE <= DRG_PITCH && (c_lo + ngroups * GE) % 2 == 0, "a staged row fits its pitch");
    const int E0 = tx0 * step, row_elems = jb.cols * step;
    for (int i = tid; i < nrows * ngroups; i += DRG_THREADS) {
        const int r = i / ngroups, c0 = c_lo + (i - r * ngroups) * GE;
        const uint8_t* row = plane + (long long)drg_plane_row<G>(jb, ty0, r) * jb.pitch;
        const int g0 = E0 + c0 - DRG_LEFT;
        uint32_t v[GE];
        if (g0 >= 0 && g0 + GE <= row_elems && ((reinterpret_cast<uintptr_t>(row) + (uintptr_t)g0 * BYTES) & 3) == 0) {
            const uint32_t w = *reinterpret_cast<const drg_dword*>(row + (long long)g0 * BYTES);
            if constexpr (BYTES == 1) {
                v[0] = w & 255u, v[1] = (w >> 8) & 255u, v[2] = (w >> 16) & 255u, v[3] = w >> 24;
            } else {
                v[0] = min(w & 0xffffu, (uint32_t)jb.top), v[1] = min(w >> 16, (uint32_t)jb.top);
            }
        } else {
#pragma unroll
            for (int k = 0; k < GE; ++k) {          // element g is channel g mod step of pixel g div step, the pixel clamped to the row
                const int gs = g0 + k + DRG_BIAS * step, x = min(max(gs / step - DRG_BIAS, 0), jb.cols - 1), ch = gs % step;
                const long long e = (long long)x * step + ch;
                if constexpr (BYTES == 1) v[k] = row[e];
                else v[k] = min((uint32_t)reinterpret_cast<const uint16_t*>(row)[e], (uint32_t)jb.top);
            }
        }
        drg_dword* out = reinterpret_cast<drg_dword*>(tile + r * DRG_PITCH + c0);          // (c0 and the pitch are even)
        if constexpr (BYTES == 1) {
            out[0] = v[0] | (v[1] << 16), out[1] = v[2] | (v[3] << 16);
        } else {
            out[0] = v[0] | (v[1] << 16);
        }
    }
}

// Block n of a tile: row of blocks n / nbr (field mode: rows of blocks 0, 1 of parity 0, then of parity 1 -- see drg_block_of), and in a
// row of blocks the 8-pixel group n % nbr / step of channel n % nbr % step.  nbr = (T / 8) * step.
template <int STEP>
constexpr int drg_blocks_row() { return drg_tile_cols(STEP) / 8 * STEP; }

// The block of the tile's own sample (row r, element c): index into the info words.
template <int STEP, int G>
__device__ __forceinline__ int drg_block_of(int r, int c) {
    const int p = r & (G - 1), fr = r / G;
    return ((fr >> 3) * G + p) * drg_blocks_row<STEP>() + c / (8 * STEP) * STEP + c % STEP;
}

// Phase 2: dir and P8 of every block that has a sample inside the plane.
template <int STEP, int G>
__device__ __forceinline__ void drg_blocks(const DeringJob& jb, const uint16_t* tile, uint16_t* info, int tid, int tx0, int ty0) {
    constexpr int nbr = drg_blocks_row<STEP>(), nblocks = 4 * nbr;
    static_assert(nblocks <= DRG_MAX_BLOCKS, "the info words hold a tile's blocks");
    for (int n = tid; n < nblocks; n += DRG_THREADS) {
        const int rb = n / nbr, cb = n - rb * nbr, p = rb & (G - 1), fb = rb / G;          // row of blocks: parity p, block fb of the field's tile rows
        const int px = cb / STEP, ch = cb - px * STEP;
        const int y0 = ty0 + (fb * 8) * G + p;          // the block's first frame row and pixel
        if (y0 >= jb.rows || tx0 + px * 8 >= jb.cols) continue;
        const uint16_t* at = tile + (DRG_HALO * G + fb * 8 * G + p) * DRG_PITCH + DRG_LEFT + px * 8 * STEP + ch;
        int b[8][8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int j = 0; j < 8; ++j) b[i][j] = ((int)at[i * G * DRG_PITCH + j * STEP] >> jb.shift) - 128;
        }
        int dir, var;
        drg_direction(b, dir, var);
        info[n] = (uint16_t)(dir | drg_primary8(var, jb.pri8) << 3);
    }
}

// Phase 3: the tile's own samples, filtered from LDS and stored, a dword of output per lane and turn.
template <int BYTES, int STEP, int G>
__device__ __forceinline__ void drg_filter(const DeringJob& jb, uint8_t* plane, const uint16_t* tile, const uint16_t* info, int tid, int tx0, int ty0) {
    constexpr int GE = 4 / BYTES, te = drg_tile_cols(STEP) * STEP, ngroups = te / GE;
    const int E0 = tx0 * STEP, row_elems = jb.cols * STEP;
    for (int i = tid; i < DRG_TILE_ROWS * ngroups; i += DRG_THREADS) {
        const int r = i / ngroups, c0 = (i - r * ngroups) * GE, y = ty0 + r, g0 = E0 + c0;
        if (y >= jb.rows || g0 >= row_elems) continue;
        const uint16_t* in = tile + (DRG_HALO * G + r) * DRG_PITCH + DRG_LEFT + c0;
        uint32_t v[GE];
#pragma unroll
        for (int k = 0; k < GE; ++k)          // (an element beyond the row's end belongs to a block outside the plane: not computed, not stored)
            v[k] = g0 + k < row_elems ? (uint32_t)drg_sample(jb, in + k, info[drg_block_of<STEP, G>(r, c0 + k)], G * DRG_PITCH, STEP) : 0u;
        uint8_t* row = plane + (long long)y * jb.pitch;
        if (g0 + GE <= row_elems && ((reinterpret_cast<uintptr_t>(row) + (uintptr_t)g0 * BYTES) & 3) == 0) {
            if constexpr (BYTES == 1) *reinterpret_cast<drg_dword*>(row + g0) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
            else *reinterpret_cast<drg_dword*>(row + (long long)g0 * 2) = v[0] | (v[1] << 16);
        } else {
#pragma unroll
            for (int k = 0; k < GE; ++k) {
                if (g0 + k >= row_elems) break;
                if constexpr (BYTES == 1) row[g0 + k] = (uint8_t)v[k];
                else reinterpret_cast<uint16_t*>(row)[g0 + k] = (uint16_t)v[k];
            }
        }
    }
}

#ifdef SAVSR_HOST_CHECK
// The host check's form: the three phases as they are, lane after lane where the GPU has a barrier, on heap buffers of the exact sizes
// (the launch has one thread per workgroup).
template <int BYTES, int STEP, int G>
__global__ void dering_kernel(DeringJob jb) {
    uint16_t* tile = new uint16_t[DRG_LDS_WORDS];
    uint16_t* info = new uint16_t[DRG_MAX_BLOCKS];
    for (int i = 0; i < DRG_LDS_WORDS; ++i) tile[i] = 0xDEAD;
    for (int i = 0; i < DRG_MAX_BLOCKS; ++i) info[i] = 0xDEAD;
    const int tx0 = (int)blockIdx.x * drg_tile_cols(STEP), ty0 = (int)blockIdx.y * DRG_TILE_ROWS;
    for (int tid = 0; tid < DRG_THREADS; ++tid) drg_stage<BYTES, STEP, G>(jb, jb.src + (long long)blockIdx.z * jb.stride, tile, tid, tx0, ty0);
    for (int tid = 0; tid < DRG_THREADS; ++tid) drg_blocks<STEP, G>(jb, tile, info, tid, tx0, ty0);
    for (int tid = 0; tid < DRG_THREADS; ++tid) drg_filter<BYTES, STEP, G>(jb, jb.dst + (long long)blockIdx.z * jb.dst_stride, tile, info, tid, tx0, ty0);
    delete[] tile;
    delete[] info;
}
constexpr int DRG_LAUNCH_THREADS = 1;
#else
template <int BYTES, int STEP, int G>
__global__ __launch_bounds__(DRG_THREADS) void dering_kernel(DeringJob jb) {
    __shared__ __attribute__((aligned(16))) uint16_t tile[DRG_LDS_WORDS];
    __shared__ uint16_t info[DRG_MAX_BLOCKS];
    const int tid = (int)threadIdx.x, tx0 = (int)blockIdx.x * drg_tile_cols(STEP), ty0 = (int)blockIdx.y * DRG_TILE_ROWS;
    drg_stage<BYTES, STEP, G>(jb, jb.src + (long long)blockIdx.z * jb.stride, tile, tid, tx0, ty0);
    __syncthreads();
    drg_blocks<STEP, G>(jb, tile, info, tid, tx0, ty0);
    __syncthreads();
    drg_filter<BYTES, STEP, G>(jb, jb.dst + (long long)blockIdx.z * jb.dst_stride, tile, info, tid, tx0, ty0);
}
constexpr int DRG_LAUNCH_THREADS = DRG_THREADS;
#endif

template <int BYTES, int STEP, int G>
int drg_launch(const DeringJob& jb, int nf, hipStream_t st) {
    const dim3 grid(blocks(jb.cols, drg_tile_cols(STEP)), blocks(jb.rows, DRG_TILE_ROWS), (unsigned)nf);
    hipLaunchKernelGGL((dering_kernel<BYTES, STEP, G>), grid, dim3(DRG_LAUNCH_THREADS), 0, st, jb);
    return check_launch("dering_kernel");
}

template <int BYTES, int G>
int drg_launch_step(const DeringJob& jb, int nf, hipStream_t st) {
    switch (jb.step) {
        case 1: return drg_launch<BYTES, 1, G>(jb, nf, st);
        case 2: return drg_launch<BYTES, 2, G>(jb, nf, st);
        case 3: return drg_launch<BYTES, 3, G>(jb, nf, st);
        default: return drg_launch<BYTES, 4, G>(jb, nf, st);
    }
}

// The body of the two entries.  cols: pixels of a row; step: samples of a pixel; pri, sec: P's p and S in the depth's codes.
template <int BYTES>
int dering(const char* who, const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step, int depth,
           int interlaced, int pri, int sec, int damping, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset, void* stream) {
    constexpr MatrixRule rule{1, 0, nullptr, "", false};
    if (step < 1 || step > DRG_MAX_STEP) return refuse(who, "step 1 .. 4 (the samples of a pixel)");
    if (cols < 1) return refuse(who, "a row holds at least one sample");
    const int64_t row_bytes = (int64_t)BYTES * cols * step;
    const char* why = check_matrix(rule, frames && out ? frames : nullptr, n_frames, frame_bytes, plane_offset, rows, row_bytes, 0, 0, n_frames, out_plane_offset);
    if (!why) why = check_out_plane(out_frame_bytes, out_plane_offset, rows, row_bytes);
    if (why) return refuse(who, why);
    if (BYTES == 2)
        if (int rc = check_samples16(who, depth, frames, frame_bytes, plane_offset, true, out, out_frame_bytes, out_plane_offset)) return rc;
    if (interlaced != 0 && interlaced != 1) return refuse(who, "interlaced 0 or 1");
    const int sh = depth - 8, unit = (1 << sh) - 1;
    if (pri < 0 || (pri & unit) || (pri >> sh) > DRG_MAX_PRI) return refuse(who, "pri a multiple of 1 << (depth - 8), 0 .. 15 << (depth - 8)");
    if (sec < 0 || (sec & unit) || (sec >> sh) > DRG_MAX_SEC) return refuse(who, "sec a multiple of 1 << (depth - 8), 0 .. 4 << (depth - 8)");
    if (damping < 3 || damping > 6) return refuse(who, "damping 3 .. 6 (8-bit code units; the depth is added inside)");
    if (out < frames + (int64_t)n_frames * frame_bytes && frames < out + (int64_t)n_frames * out_frame_bytes)
        return refuse(who, "the source frames and the output overlap");
    const DeringJob jb{frames + plane_offset, out + out_plane_offset, frame_bytes, out_frame_bytes, row_bytes, rows, cols, step,
                       pri >> sh, sec, sh, damping, (1 << depth) - 1};
    hipStream_t st = static_cast<hipStream_t>(stream);
    return for_frame_chunks(n_frames, FM_MAX_FRAMES, [&](int f0, int nf) {
        DeringJob part = jb;
        part.src = jb.src + (long long)f0 * jb.stride;
        part.dst = jb.dst + (long long)f0 * jb.dst_stride;
        return interlaced ? drg_launch_step<BYTES, 2>(part, nf, st) : drg_launch_step<BYTES, 1>(part, nf, st);
    });
}

}  // namespace
}  // namespace savsr

using namespace savsr;

extern "C" int savsr_video_dering_u8(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step,
                                     int interlaced, int pri, int sec, int damping, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset,
                                     void* stream) {
    return dering<1>("video_dering_u8", frames, n_frames, frame_bytes, plane_offset, rows, cols, step, 8, interlaced, pri, sec, damping, out,
                     out_frame_bytes, out_plane_offset, stream);
}

extern "C" int savsr_video_dering_u16(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step,
                                      int depth, int interlaced, int pri, int sec, int damping, uint8_t* out, int64_t out_frame_bytes,
                                      int64_t out_plane_offset, void* stream) {
    return dering<2>("video_dering_u16", frames, n_frames, frame_bytes, plane_offset, rows, cols, step, depth, interlaced, pri, sec, damping, out,
                     out_frame_bytes, out_plane_offset, stream);
}
