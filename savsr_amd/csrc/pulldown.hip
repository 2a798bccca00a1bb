// Inverse 3:2 pulldown (ABI 44): the field-match scores and the weave of telecined film (savsr_amd/pulldown.py `field_scores` and `weave`
// are the specification; the kernels equal them bit for bit, the match and the decimation are decided on the host in exact arithmetic).
// The first field is the rows of parity p (0 for tff, 1 for bff), the second field the rows of parity 1 - p.
//
// Scores.  Source frame n has two candidates for its second field: j = 0 the second field of frame max(n - 1, 0), j = 1 its own.  A
// candidate's score is the sum over the second field's rows y, 1 <= y <= rows - 2 (y = 1 + p + 2 s, s = 0 .. (rows - 1 - p) / 2 - 1),
// and all x of |a - b| + |c - b| - |a - c|, a = F[n][y - 1], c = F[n][y + 1], b the candidate's sample: never negative, and an exact
// integer in any order, so the grid shape and the atomics change nothing in the result.
//
//   _u8    matrices of rows x row_bytes bytes (a plane, or the h x (w * c) bytes of packed frames: only vertical neighbours meet)
//   _u16   matrices of rows x cols little-endian 16-bit samples, every sample read as min(s, 2^depth - 1) >> (depth - 8)
//
// One launch per call after one hipMemsetAsync of the scores; grid = (lane tiles over scored rows x row pieces, frame).  Vector form
// (plane base pointer, frame stride and row bytes multiples of 16): a lane owns 16 bytes of one second-field row and issues its four
// 16-byte nontemporal loads (a, c, the frame's own b and the previous frame's b) before the first use; v_sad_u8 per dword, |a - c|
// shared by both candidates; no LDS staging of rows: the rows above and below are read by the two neighbouring scored rows as well and
// come from L2.  One-sample form (any pointer, stride and row length): a lane owns PD_ONE_ITERS samples.  Lane sums are 32-bit and leave
// the workgroup through field_matrix.hpp's block_reduce: one 64-bit vector atomic per workgroup and candidate.  The matrix, its checks
// and the launch chunking are that header's.
//
// Weave.  Output frame o of source frame n = from + o: the rows of parity p from frame n, the others from frame clamp(n + delta[o], 0,
// n_frames - 1); delta is a device table the entry cannot see, so the kernel clamps.  A byte copy at every depth: a 16-byte form and a
// byte form, one launch per plane.
//
// (ABI 49) Comb windows: the residual combing of woven frames, behind combed= (`comb_windows` is the specification); see the section below.
#include "common.hpp"
#include "video_samples.hpp"
#include "field_matrix.hpp"

#include <cstdint>

namespace savsr {
namespace {

constexpr int PD_THREADS = FM_THREADS;
constexpr int PD_ONE_ITERS = 8;                     // samples (bytes, for the weave) per lane in the one-sample forms
constexpr MatrixRule PD_RULE{1, 0, nullptr, "the range needs 0 <= from <= to <= n_frames", true};

// What a score launch works on.  A lane sum is at most PD_ONE_ITERS (or 16, the bytes of a vector lane's row piece) x 3 x 255 <= 12240.
// (Not an extension of FieldMatrix: the scored rows stand for its rows, and behind it they moved a kernel's scalar-register count.)
struct ScoreJob {
    const uint8_t* src;          // the matrix of resident frame 0
    long long stride, pitch;     // bytes between frames / rows
    int n_frames, from, cols;    // cols: samples of a row
    int y0, srows;               // the scored rows: y0 + 2 s, s = 0 .. srows - 1
    uint32_t top;                // 2^depth - 1
    int shift;                   // depth - 8
};

// Vector form: lane = (scored row s, 16-byte chunk) = (idx / chunks, idx % chunks), idx = blockIdx.x * PD_THREADS + threadIdx.x; frame
// blockIdx.y of the launch.  BYTES: of a sample.
template <int BYTES>
__global__ __launch_bounds__(PD_THREADS) void field_scores_vec_kernel(ScoreJob jb, unsigned long long* __restrict__ out) {
    const uint32_t chunks = (uint32_t)(jb.pitch >> 4);
    const uint32_t idx = blockIdx.x * PD_THREADS + threadIdx.x;
    const uint32_t s = idx / chunks, chunk = idx - s * chunks;
    uint32_t acc0 = 0, acc1 = 0;
    if (s < (uint32_t)jb.srows) {
        const int n = jb.from + (int)blockIdx.y;
        const int np = n > 0 ? n - 1 : 0;
        const long long y = jb.y0 + 2ll * s;
        const uint8_t* cur = jb.src + (long long)n * jb.stride + y * jb.pitch;
        const uint8_t* prev = jb.src + (long long)np * jb.stride + y * jb.pitch;
        const u32x4 a = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(cur - jb.pitch) + chunk);
        const u32x4 c = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(cur + jb.pitch) + chunk);
        const u32x4 b1 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(cur) + chunk);
        const u32x4 b0 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(prev) + chunk);
        uint32_t ac = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if constexpr (BYTES == 1) {
                ac = sad4(a[e], c[e], ac);
                acc0 = sad4(c[e], b0[e], sad4(a[e], b0[e], acc0));
                acc1 = sad4(c[e], b1[e], sad4(a[e], b1[e], acc1));
            } else {
                const uint32_t ae = msb8x2(a[e], jb.top, jb.shift), ce = msb8x2(c[e], jb.top, jb.shift);
                const uint32_t p0 = msb8x2(b0[e], jb.top, jb.shift), p1 = msb8x2(b1[e], jb.top, jb.shift);
                ac = sad2(ae, ce, ac);
                acc0 = sad2(ce, p0, sad2(ae, p0, acc0));
                acc1 = sad2(ce, p1, sad2(ae, p1, acc1));
            }
        }
        acc0 -= ac;          // per sample |a - b| + |c - b| >= |a - c|: the sums stay >= 0
        acc1 -= ac;
    }
    const uint32_t acc[2] = {acc0, acc1};
    block_reduce<2, 1>(acc, out + 2 * blockIdx.y);
}

// One-sample form: sample i = (scored row, x) = (i / cols, i % cols), i = blockIdx.x * (PD_THREADS * PD_ONE_ITERS) + it * PD_THREADS + tid.
template <int BYTES>
__global__ __launch_bounds__(PD_THREADS) void field_scores_one_kernel(ScoreJob jb, unsigned long long* __restrict__ out) {
    const int n = jb.from + (int)blockIdx.y;
    const int np = n > 0 ? n - 1 : 0;
    const uint8_t* cur = jb.src + (long long)n * jb.stride;
    const uint8_t* prev = jb.src + (long long)np * jb.stride;
    const uint32_t total = (uint32_t)jb.srows * (uint32_t)jb.cols;
    const uint32_t i0 = blockIdx.x * (PD_THREADS * PD_ONE_ITERS) + threadIdx.x;
    uint32_t acc0 = 0, acc1 = 0;
#pragma unroll 2
    for (int it = 0; it < PD_ONE_ITERS; ++it) {
        const uint32_t i = i0 + it * PD_THREADS;
        if (i < total) {
            const uint32_t s = i / (uint32_t)jb.cols, x = i - s * (uint32_t)jb.cols;
            const long long off = (jb.y0 + 2ll * s) * jb.pitch;
            const uint32_t a = sample8<BYTES>(cur + off - jb.pitch, x, jb.top, jb.shift), c = sample8<BYTES>(cur + off + jb.pitch, x, jb.top, jb.shift);
            const uint32_t b0 = sample8<BYTES>(prev + off, x, jb.top, jb.shift), b1 = sample8<BYTES>(cur + off, x, jb.top, jb.shift);
            const uint32_t ac = absdiff(a, c);
            acc0 += absdiff(a, b0) + absdiff(c, b0) - ac;
            acc1 += absdiff(a, b1) + absdiff(c, b1) - ac;
        }
    }
    const uint32_t acc[2] = {acc0, acc1};
    block_reduce<2, 1>(acc, out + 2 * blockIdx.y);
}

template <int BYTES>
int launch_scores(ScoreJob jb, int n_out, int64_t* out, hipStream_t st, const char* what) {
    if (int rc = clear_cells(out, 2, n_out, st, what)) return rc;
    if (jb.srows < 1) return 0;          // fewer than three rows, or no second-field row between two others: zeros
    const bool vec = aligned16(jb.src, jb.stride, jb.pitch);
    const unsigned gx = vec ? blocks((long long)jb.srows * (jb.pitch >> 4), PD_THREADS) : blocks((long long)jb.srows * jb.cols, PD_THREADS * PD_ONE_ITERS);
    return for_frame_chunks(n_out, FM_MAX_FRAMES, [&](int f0, int nf) {
        ScoreJob part = jb;
        part.from = jb.from + f0;
        unsigned long long* cells = reinterpret_cast<unsigned long long*>(out) + 2ll * f0;
        if (vec) hipLaunchKernelGGL((field_scores_vec_kernel<BYTES>), dim3(gx, (unsigned)nf), dim3(PD_THREADS), 0, st, part, cells);
        else hipLaunchKernelGGL((field_scores_one_kernel<BYTES>), dim3(gx, (unsigned)nf), dim3(PD_THREADS), 0, st, part, cells);
        return check_launch(vec ? "field_scores_vec_kernel" : "field_scores_one_kernel");
    });
}

// What a weave launch works on.  Rows are `pitch` bytes apart on both sides.
struct WeaveJob : FieldMatrix {
    uint8_t* dst;                // the plane of output frame 0
    const int32_t* delta;        // device: one of -1, 0 per output frame of the launch
    long long dst_stride;
    int parity;
};

// The source row of output row y of output frame o: frame n where y has the first field's parity, else frame clamp(n + delta[o]).
__device__ __forceinline__ const uint8_t* weave_row(const WeaveJob& jb, int o, uint32_t y) {
    const int n = jb.from + o;
    int m = n;
    if ((int)(y & 1u) != jb.parity) {
        m = n + jb.delta[o];
        m = m < 0 ? 0 : (m > jb.n_frames - 1 ? jb.n_frames - 1 : m);
    }
    return jb.src + (long long)m * jb.stride + (long long)y * jb.pitch;
}

// 16-byte form: lane = (row, chunk) = (idx / chunks, idx % chunks); output frame blockIdx.y of the launch.
__global__ __launch_bounds__(PD_THREADS) void weave_vec_kernel(WeaveJob jb) {
    const uint32_t chunks = (uint32_t)(jb.pitch >> 4);
    const uint32_t idx = blockIdx.x * PD_THREADS + threadIdx.x;
    const uint32_t y = idx / chunks, chunk = idx - y * chunks;
    if (y >= (uint32_t)jb.rows) return;
    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(weave_row(jb, (int)blockIdx.y, y)) + chunk);
    *(reinterpret_cast<u32x4*>(jb.dst + (long long)blockIdx.y * jb.dst_stride + (long long)y * jb.pitch) + chunk) = v;
}

// Byte form: byte i = (row, x) = (i / pitch, i % pitch), PD_ONE_ITERS bytes per lane.
__global__ __launch_bounds__(PD_THREADS) void weave_one_kernel(WeaveJob jb) {
    const uint32_t pitch = (uint32_t)jb.pitch, total = (uint32_t)jb.rows * pitch;
    const uint32_t i0 = blockIdx.x * (PD_THREADS * PD_ONE_ITERS) + threadIdx.x;
    uint8_t* dst = jb.dst + (long long)blockIdx.y * jb.dst_stride;
#pragma unroll 2
    for (int it = 0; it < PD_ONE_ITERS; ++it) {
        const uint32_t i = i0 + it * PD_THREADS;
        if (i < total) {
            const uint32_t y = i / pitch, x = i - y * pitch;
            dst[i] = weave_row(jb, (int)blockIdx.y, y)[x];
        }
    }
}

// ---- residual combing after the match (ABI 49; `comb_windows` is the specification) ---------------------------------------------------------
// A sample on a second-field row is combed iff its match measure exceeds 2 * threshold; cells of 8 rows x 8 pixels count them; a window is
// 2 x 2 cells, one at every cell origin; per frame the largest window count and the total.  A workgroup owns a tile of CW_TR x tc cells
// (the origins of its windows) and reads one more cell row below and one more cell column to the right, so every window's four cells are
// counted by the workgroup that sums it and no cell count crosses workgroups.  Lanes walk the tile's second-field rows (vector form: 16
// bytes of a row and its two vertical neighbours, three loads; a chunk meets at most two cells, so two LDS adds per lane and row piece;
// one-sample form: one sample, one LDS add where it is combed), then the window sums are taken from the LDS cells, reduced over the
// workgroup, and one 64-bit atomicMax and one 64-bit atomicAdd per workgroup go to the frame's two cells.  Counts are exact integers and
// max / + commute, so the grid shape changes nothing.
constexpr int CW_CELL = 8;                 // rows and pixels of a cell
constexpr int CW_TR = 8;                   // cell rows of a tile: 64 rows of the matrix, 72 with the halo
constexpr int CW_TILE_BYTES = 512;         // bytes of a tile's row (without the halo cell)
constexpr int CW_MAX_TC = CW_TILE_BYTES / CW_CELL;          // cell columns of a tile: at most 64 (8-byte cells)
constexpr int CW_LROWS = (CW_TR + 1) * CW_CELL / 2;         // second-field rows of a tile with its halo

// (Not an extension of FieldMatrix, like ScoreJob: the kernels have no use for n_frames, and with it their argument loads changed.)
struct CombJob {
    const uint8_t* src;          // the matrix of resident frame 0
    long long stride, pitch;     // bytes between frames / rows
    int from, rows, cols;        // cols: samples of a row
    int q;                       // the second field's parity
    int cell_w;                  // samples of a cell's row: 8 * step
    int ncr, ncc;                // cell rows / columns of the matrix
    int tc, tiles_x;             // cell columns of a tile; tiles of a cell row
    uint32_t top;                // 2^depth - 1
    int shift;                   // depth - 8
    uint32_t thresh2;            // 2 * threshold
};

__device__ __forceinline__ bool pd_combed(uint32_t a, uint32_t b, uint32_t c, uint32_t thresh2) {
    return absdiff(a, b) + absdiff(c, b) - absdiff(a, c) > thresh2;
}

typedef uint32_t CombCells[CW_TR + 1][CW_MAX_TC + 1];

// Lane `tid`'s share of tile (tx, ty) of frame n: combed counts into the tile's cells (LDS adds).
template <int BYTES, bool VEC>
__device__ __forceinline__ void comb_count(const CombJob& jb, int tx, int ty, int n, uint32_t tid, CombCells& cells) {
    const uint8_t* cur = jb.src + (long long)n * jb.stride;
    const int cc0 = tx * jb.tc;                                   // the tile's first cell column
    const int x0 = cc0 * jb.cell_w;                               // its first sample and the one past its last (halo included)
    const int x1 = min(x0 + (jb.tc + 1) * jb.cell_w, jb.cols);
    const int yt = ty * CW_TR * CW_CELL;                          // its first row (even, so local parities are the matrix's)
    if constexpr (VEC) {
        constexpr int SPL = 16 / BYTES;                           // samples of a chunk
        const int c0 = x0 / SPL, nch = (x1 + SPL - 1) / SPL - c0; // the chunks that meet the tile (the row is whole chunks: pitch % 16 == 0)
        for (uint32_t u = tid; u < (uint32_t)(CW_LROWS * nch); u += PD_THREADS) {
            const int lr = (int)(u / (uint32_t)nch), chunk = c0 + (int)(u - (uint32_t)lr * (uint32_t)nch);
            const int y = yt + 2 * lr + jb.q;
            if (y < 1 || y > jb.rows - 2) continue;
            const uint8_t* row = cur + (long long)y * jb.pitch;
            const u32x4 a = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(row - jb.pitch) + chunk);
            const u32x4 b = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(row) + chunk);
            const u32x4 c = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(row + jb.pitch) + chunk);
            uint32_t mask = 0;                                    // bit i: sample i of the chunk is combed
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if constexpr (BYTES == 1) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        mask |= (uint32_t)pd_combed((a[e] >> (8 * k)) & 255u, (b[e] >> (8 * k)) & 255u, (c[e] >> (8 * k)) & 255u, jb.thresh2) << (4 * e + k);
                } else {
#pragma unroll
                    for (int k = 0; k < 2; ++k)
                        mask |= (uint32_t)pd_combed(msb8((a[e] >> (16 * k)) & 0xffffu, jb.top, jb.shift), msb8((b[e] >> (16 * k)) & 0xffffu, jb.top, jb.shift),
                                                    msb8((c[e] >> (16 * k)) & 0xffffu, jb.top, jb.shift), jb.thresh2) << (2 * e + k);
                }
            }
            const int xs = chunk * SPL;                           // the chunk's samples [xs, xs + SPL) lie in cell columns ca and ca + 1
            const int ca = xs / jb.cell_w;
            const int na = min((ca + 1) * jb.cell_w - xs, SPL);   // how many of them in ca
            const uint32_t in_a = __builtin_popcount(mask & ((1u << na) - 1u)), in_b = __builtin_popcount(mask >> na);
            const int la = ca - cc0;                              // (cells outside the tile with its halo: another tile's)
            if (in_a && la >= 0 && la <= jb.tc) atomicAdd(&cells[lr >> 2][la], in_a);
            if (in_b && la + 1 >= 0 && la + 1 <= jb.tc) atomicAdd(&cells[lr >> 2][la + 1], in_b);
        }
    } else {
        const int ns = x1 - x0;
        for (uint32_t u = tid; u < (uint32_t)(CW_LROWS * ns); u += PD_THREADS) {
            const int lr = (int)(u / (uint32_t)ns), x = x0 + (int)(u - (uint32_t)lr * (uint32_t)ns);
            const int y = yt + 2 * lr + jb.q;
            if (y < 1 || y > jb.rows - 2) continue;
            const uint8_t* row = cur + (long long)y * jb.pitch;
            if (pd_combed(sample8<BYTES>(row - jb.pitch, (uint32_t)x, jb.top, jb.shift), sample8<BYTES>(row, (uint32_t)x, jb.top, jb.shift),
                          sample8<BYTES>(row + jb.pitch, (uint32_t)x, jb.top, jb.shift), jb.thresh2))
                atomicAdd(&cells[lr >> 2][x / jb.cell_w - cc0], 1u);
        }
    }
}

// Lane `tid`'s windows of tile (tx, ty): the largest window sum into mx, the tile's own cells (not the halo's) into total.
__device__ __forceinline__ void comb_sum(const CombJob& jb, int tx, int ty, uint32_t tid, const CombCells& cells, uint32_t& mx, uint32_t& total) {
    for (uint32_t u = tid; u < (uint32_t)(CW_TR * jb.tc); u += PD_THREADS) {
        const int i = (int)(u / (uint32_t)jb.tc), j = (int)(u - (uint32_t)i * (uint32_t)jb.tc);
        if (ty * CW_TR + i >= jb.ncr || tx * jb.tc + j >= jb.ncc) continue;          // (no such cell: no window)
        const uint32_t own = cells[i][j];
        total += own;
        mx = max(mx, own + cells[i + 1][j] + cells[i][j + 1] + cells[i + 1][j + 1]);  // (cells past the matrix hold 0)
    }
}

// Tile blockIdx.x = ty * tiles_x + tx of frame blockIdx.y of the launch.
template <int BYTES, bool VEC>
__global__ __launch_bounds__(PD_THREADS) void comb_windows_kernel(CombJob jb, unsigned long long* __restrict__ out) {
    const int ty = (int)(blockIdx.x / (uint32_t)jb.tiles_x), tx = (int)(blockIdx.x - (uint32_t)ty * (uint32_t)jb.tiles_x);
    const int n = jb.from + (int)blockIdx.y;
    unsigned long long* cell = out + 2 * blockIdx.y;
    uint32_t mx = 0, total = 0;
    // (The reduction stays here, not in block_reduce: a maximum beside a sum, both sent by thread 0; sent by two threads the kernels' code changed.)
#ifdef SAVSR_HOST_CHECK          // the host check runs one thread at a time: the first clears the cells, the last sums every lane's windows
    static CombCells cells;
    if (threadIdx.x == 0) memset(cells, 0, sizeof cells);
    comb_count<BYTES, VEC>(jb, tx, ty, n, threadIdx.x, cells);
    if (threadIdx.x + 1 < PD_THREADS) return;
    for (uint32_t t = 0; t < PD_THREADS; ++t) comb_sum(jb, tx, ty, t, cells, mx, total);
    if (mx) atomicMax(cell, (unsigned long long)mx);
    if (total) atomicAdd(cell + 1, (unsigned long long)total);
#else
    __shared__ CombCells cells;
    __shared__ uint32_t part[2][PD_THREADS / 64];
    for (uint32_t i = threadIdx.x; i < (CW_TR + 1) * (CW_MAX_TC + 1); i += PD_THREADS) (&cells[0][0])[i] = 0u;
    __syncthreads();
    comb_count<BYTES, VEC>(jb, tx, ty, n, threadIdx.x, cells);
    __syncthreads();
    comb_sum(jb, tx, ty, threadIdx.x, cells, mx, total);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mx = max(mx, (uint32_t)__shfl_xor(mx, o, 64));
        total += __shfl_xor(total, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = mx;
        part[1][threadIdx.x >> 6] = total;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = 0, s = 0;
#pragma unroll
        for (int i = 0; i < PD_THREADS / 64; ++i) {
            m = max(m, (unsigned long long)part[0][i]);
            s += part[1][i];
        }
        if (m) atomicMax(cell, m);
        if (s) atomicAdd(cell + 1, s);
    }
#endif
}

template <int BYTES>
int launch_comb(CombJob jb, int n_out, int64_t* out, hipStream_t st, const char* what) {
    if (int rc = clear_cells(out, 2, n_out, st, what)) return rc;
    if (jb.rows < 3) return 0;          // no second-field row between two others: zeros
    const bool vec = aligned16(jb.src, jb.stride, jb.pitch);
    const unsigned gx = (unsigned)jb.tiles_x * (unsigned)((jb.ncr + CW_TR - 1) / CW_TR);
    return for_frame_chunks(n_out, FM_MAX_FRAMES, [&](int f0, int nf) {
        CombJob part = jb;
        part.from = jb.from + f0;
        unsigned long long* cells = reinterpret_cast<unsigned long long*>(out) + 2ll * f0;
        if (vec) hipLaunchKernelGGL((comb_windows_kernel<BYTES, true>), dim3(gx, (unsigned)nf), dim3(PD_THREADS), 0, st, part, cells);
        else hipLaunchKernelGGL((comb_windows_kernel<BYTES, false>), dim3(gx, (unsigned)nf), dim3(PD_THREADS), 0, st, part, cells);
        return check_launch("comb_windows_kernel");
    });
}

// The checks the reducing entries share (`samples16`: the entry is a _u16 one); the cells' own come after the entry's.
int check_reducing(const char* who, bool samples16, const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows,
                   int64_t row_bytes, int depth, int order, int from, int to) {
    if (const char* why = check_matrix(PD_RULE, frames, n_frames, frame_bytes, plane_offset, rows, row_bytes, order, from, to)) return refuse(who, why);
    return samples16 ? check_samples16(who, depth, frames, frame_bytes, plane_offset) : 0;
}

// The body of the two score entries.  width: row_bytes (_u8) or cols (_u16).
template <int BYTES>
int field_scores(const char* who, const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int width, int depth,
                 int order, int from, int to, int64_t* out, void* stream) {
    if (int rc = check_reducing(who, BYTES == 2, frames, n_frames, frame_bytes, plane_offset, rows, (int64_t)BYTES * width, depth, order, from, to)) return rc;
    if (const char* why = check_cells(out, to > from)) return refuse(who, why);
    if (to == from) return 0;
    const int srows = rows - 1 - order > 0 ? (rows - 1 - order) / 2 : 0;
    const ScoreJob jb{frames + plane_offset, frame_bytes, (long long)BYTES * width, n_frames, from, width, 1 + order, srows, (1u << depth) - 1u, depth - 8};
    return launch_scores<BYTES>(jb, to - from, out, static_cast<hipStream_t>(stream), who);
}

// The body of the two comb entries.  step: the samples of a pixel (1 for _u16).
template <int BYTES>
int comb_windows(const char* who, const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int width, int step,
                 int depth, int order, int from, int to, int threshold, int64_t* out, void* stream) {
    if (int rc = check_reducing(who, BYTES == 2, frames, n_frames, frame_bytes, plane_offset, rows, (int64_t)BYTES * width, depth, order, from, to)) return rc;
    if (step < 1 || step > 4) return refuse(who, "step 1 .. 4");
    if (threshold < 0 || threshold > 255) return refuse(who, "threshold 0 .. 255");
    if (const char* why = check_cells(out, to > from)) return refuse(who, why);
    if (to == from) return 0;
    const int cell_w = CW_CELL * step, tc = CW_TILE_BYTES / (cell_w * BYTES);
    const int ncr = (rows + CW_CELL - 1) / CW_CELL, ncc = (width + cell_w - 1) / cell_w;
    const CombJob jb{frames + plane_offset, frame_bytes, (long long)BYTES * width, from, rows, width, 1 - order, cell_w, ncr, ncc, tc, (ncc + tc - 1) / tc,
                     (1u << depth) - 1u, depth - 8, 2u * (uint32_t)threshold};
    return launch_comb<BYTES>(jb, to - from, out, static_cast<hipStream_t>(stream), who);
}

}  // namespace
}  // namespace savsr

using namespace savsr;

extern "C" int savsr_video_field_scores_u8(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int row_bytes,
                                           int order, int from, int to, int64_t* out, void* stream) {
    return field_scores<1>("video_field_scores_u8", frames, n_frames, frame_bytes, plane_offset, rows, row_bytes, 8, order, from, to, out, stream);
}

extern "C" int savsr_video_field_scores_u16(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols,
                                            int depth, int order, int from, int to, int64_t* out, void* stream) {
    return field_scores<2>("video_field_scores_u16", frames, n_frames, frame_bytes, plane_offset, rows, cols, depth, order, from, to, out, stream);
}

extern "C" int savsr_video_comb_windows_u8(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int row_bytes,
                                           int step, int order, int from, int to, int threshold, int64_t* out, void* stream) {
    return comb_windows<1>("video_comb_windows_u8", frames, n_frames, frame_bytes, plane_offset, rows, row_bytes, step, 8, order, from, to, threshold, out,
                           stream);
}

extern "C" int savsr_video_comb_windows_u16(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols,
                                            int depth, int order, int from, int to, int threshold, int64_t* out, void* stream) {
    return comb_windows<2>("video_comb_windows_u16", frames, n_frames, frame_bytes, plane_offset, rows, cols, 1, depth, order, from, to, threshold, out,
                           stream);
}

// A byte copy at every depth, so one entry: the _u8 body of a pair without a _u16 sibling.
extern "C" int savsr_video_weave(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int row_bytes, int order,
                                 int from, int to, const int32_t* delta, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset,
                                 void* stream) {
    const char* who = "video_weave";
    if (const char* why = check_matrix(PD_RULE, frames, n_frames, frame_bytes, plane_offset, rows, row_bytes, order, from, to)) return refuse(who, why);
    if (const char* why = check_table(delta, to > from && (!delta || !out), "delta must be 4-byte aligned")) return refuse(who, why);
    if (const char* why = check_out_plane(out_frame_bytes, out_plane_offset, rows, row_bytes)) return refuse(who, why);
    if (to == from) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const WeaveJob jb{field_matrix<1>(frames, n_frames, frame_bytes, plane_offset, rows, row_bytes, 8, from), out + out_plane_offset, delta, out_frame_bytes,
                      order};
    const bool vec = aligned16(jb.src, jb.stride, jb.pitch) && aligned16(jb.dst, jb.dst_stride, 0);
    const unsigned gx = vec ? blocks((long long)rows * (row_bytes >> 4), PD_THREADS) : blocks((long long)rows * row_bytes, PD_THREADS * PD_ONE_ITERS);
    return for_frame_chunks(to - from, FM_MAX_FRAMES, [&](int f0, int nf) {
        WeaveJob part = jb;
        part.from = from + f0;
        part.delta = delta + f0;
        part.dst = jb.dst + (long long)f0 * out_frame_bytes;
        if (vec) hipLaunchKernelGGL(weave_vec_kernel, dim3(gx, (unsigned)nf), dim3(PD_THREADS), 0, st, part);
        else hipLaunchKernelGGL(weave_one_kernel, dim3(gx, (unsigned)nf), dim3(PD_THREADS), 0, st, part);
        return check_launch(vec ? "weave_vec_kernel" : "weave_one_kernel");
    });
}
