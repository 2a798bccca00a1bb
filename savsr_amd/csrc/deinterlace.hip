// The motion-adaptive deinterlacer (ABI 43): N interlaced frames -> 2N progressive ones, ffmpeg yadif's rule in 32-bit integers
// (savsr_amd/deinterlace.py `deinterlace_matrix` is the specification, sample by sample; the kernels equal it bit for bit).  Output frame
// 2n + f keeps the rows of parity p (f for tff, 1 - f for bff) of source frame n and interpolates the others from cur = n, prev =
// max(n - 1, 0), next = min(n + 1, n_frames - 1).  A stencil over three frames: per interpolated sample 2 rows of cur with +-3 pixel
// steps of halo, 3 rows of the field's two temporal neighbours p2 / n2 and 2 rows each of prev and next.
//
//   _u8    matrices of rows x row_bytes bytes with a pixel step (1 for a plane, c for packed h x (w * c) frames)
//   _u16   matrices of rows x cols little-endian 16-bit samples, every sample read as min(s, 2^depth - 1); step 1
//
// One launch per call, grid = (column tile, row tile, output frame).  A lane owns one interpolated row piece and copies the kept row
// above it (and the last row below it, where that one is kept): the copy costs no load, the kept row is the lane's `c` / `e` row.
// Vector form (plane base pointers, frame strides and row pitches of both sides multiples of 16 bytes): a lane owns 16 bytes; the +-3 step
// neighbours of the directional search come from the two 16-byte chunks beside its own in the `c` and `e` rows (overlapping loads that
// the neighbouring lanes issue as well, so they are L1 / L2 hits; 18 loads and 2 stores of 16 bytes per lane, all loads issued before
// the first use, no LDS).  The pixel step is a template argument, so every sample is a constant bit field of a register.  One-sample
// form (any pointer, stride and size): a lane owns one sample.  Absolute differences are v_sad_u8 / v_sad_u16 on single samples.
//
// (ABI 48) savsr_video_deinterlace_u8_m / _u16_m add a method and a rate.  Method 1 is ffmpeg bwdif's rule (`bwdif_matrix` is its
// specification): yadif's temporal clamp around the w3fdif filters, a 4-tap vertical filter on cur (rows y +- 1, y +- 3) plus a 3-row
// high-frequency term of p2 + n2 (rows y, y +- 2, y +- 4).  No horizontal taps, so no pixel step and no neighbour chunks: the vector form
// issues 18 loads of 16 bytes per lane as yadif's does (cur x 4, p2 / n2 x 10, prev / next x 4), all before the first use, no LDS.  The
// still case, the three interpolations and the clips are selects; the filter products are 24-bit multiplies (sums below 2^14 by constants
// below 2^13).  Rate 1 ("same") launches one output frame per source frame, its first field in time: the second fields are not computed.
#include "common.hpp"
#include "video_samples.hpp"
#include "field_matrix.hpp"

#include <cstdint>

namespace savsr {
namespace {

constexpr int DI_THREADS = 256;
constexpr int DI_TILE_IROWS = 16;                   // interpolated rows of a vector tile: DI_TILE_ROWS = 32 rows of the matrix
constexpr int DI_TILE_BYTES = 256;                  // bytes of a vector tile's row: 16 lanes x 16 bytes
constexpr int DI_ONE_IROWS = 4;                     // interpolated rows of a one-sample tile (one per wave)
constexpr int DI_ONE_COLS = 64;                     // samples of a one-sample tile's row
constexpr int DI_MAX_OUT = FM_MAX_FRAMES - 1;       // output frames of a launch: an even count, so that a launch starts at field 0 of a source frame
constexpr int DI_MAX_ROWS = 65535 * 2 * DI_ONE_IROWS;          // grid.y of the one-sample form

template <int BYTES>
__device__ __forceinline__ int absdiff(int a, int b) {
    if constexpr (BYTES == 1) {
#if __has_builtin(__builtin_amdgcn_sad_u8)
        return (int)__builtin_amdgcn_sad_u8((uint32_t)a, (uint32_t)b, 0u);
#else
        return a > b ? a - b : b - a;
#endif
    } else {
#if __has_builtin(__builtin_amdgcn_sad_u16)
        return (int)__builtin_amdgcn_sad_u16((uint32_t)a, (uint32_t)b, 0u);
#else
        return a > b ? a - b : b - a;
#endif
    }
}

// a * b of values that fit 24 bits: v_mul_i32_i24 on the device.
__device__ __forceinline__ int mul24(int a, int b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(a, b);
#else
    return a * b;
#endif
}

// The samples one interpolated sample reads.  u / l: the rows above and below in cur at x + (k - 3) * step, k = 0 .. 6.
struct Taps {
    int u[7], l[7];
    int p2y, n2y, p2m, n2m, p2p, n2p;          // p2 / n2 at rows y, y - 2, y + 2
    int pu, pl, nu, nl;                       // prev and next at the rows above and below
};

template <int BYTES>
__device__ __forceinline__ int check(const Taps& t, int j, int& score, int& pred, bool allowed) {
    // CHECK(j): u[x + (j - 1) s] with l[x - (j + 1) s], u[x + j s] with l[x - j s], u[x + (j + 1) s] with l[x - (j - 1) s]
    const int sc = absdiff<BYTES>(t.u[3 + j - 1], t.l[3 - j - 1]) + absdiff<BYTES>(t.u[3 + j], t.l[3 - j]) + absdiff<BYTES>(t.u[3 + j + 1], t.l[3 - j + 1]);
    const bool taken = allowed && sc < score;
    score = taken ? sc : score;
    pred = taken ? (t.u[3 + j] + t.l[3 - j]) >> 1 : pred;
    return taken;
}

// deinterlace.py's rule for one sample.  edge: x - 3 s >= 0 and x + 3 s <= C - 1; inner: y - 2 >= 0 and y + 2 <= R - 1.
template <int BYTES>
__device__ __forceinline__ int yadif(const Taps& t, bool edge, bool inner) {
    const int c = t.u[3], e = t.l[3];
    const int d = (t.p2y + t.n2y) >> 1;
    const int t0 = absdiff<BYTES>(t.p2y, t.n2y);
    const int t1 = (absdiff<BYTES>(t.pu, c) + absdiff<BYTES>(t.pl, e)) >> 1;
    const int t2 = (absdiff<BYTES>(t.nu, c) + absdiff<BYTES>(t.nl, e)) >> 1;
    int diff = max(max(t0 >> 1, t1), t2);
    int pred = (c + e) >> 1;
    int score = absdiff<BYTES>(t.u[2], t.l[2]) + absdiff<BYTES>(c, e) + absdiff<BYTES>(t.u[4], t.l[4]) - 1;
    const bool m1 = check<BYTES>(t, -1, score, pred, edge);
    check<BYTES>(t, -2, score, pred, m1);
    const bool p1 = check<BYTES>(t, 1, score, pred, edge);
    check<BYTES>(t, 2, score, pred, p1);
    const int b = (t.p2m + t.n2m) >> 1, f = (t.p2p + t.n2p) >> 1;
    const int mx = max(max(d - e, d - c), min(b - c, f - e));
    const int mn = min(min(d - e, d - c), max(b - c, f - e));
    diff = inner ? max(max(diff, mn), -mx) : diff;
    return min(max(pred, d - diff), d + diff);
}

// The samples one interpolated sample of bwdif reads.
struct BTaps {
    int c, e, c3m, c3p;                       // cur at rows y - 1, y + 1 (mirrored), y - 3, y + 3
    int p2y, n2y, p2m, n2m, p2p, n2p;          // p2 / n2 at rows y, y - 2, y + 2
    int p2mm, n2mm, p2pp, n2pp;               // p2 / n2 at rows y - 4, y + 4
    int pu, pl, nu, nl;                       // prev and next at the rows above and below
};

// deinterlace.py's `bwdif_matrix` for one sample.  inner: y - 2 >= 0 and y + 2 <= R - 1; line: y - 4 >= 0 and y + 4 <= R - 1.  Every >>
// is an arithmetic shift of a signed 32-bit value (the floor, as the specification's); every operand of a product is below 2^14.
template <int BYTES>
__device__ __forceinline__ int bwdif(const BTaps& t, bool inner, bool line, int top) {
    constexpr int LF0 = 4309, LF1 = 213, HF0 = 5570, HF1 = 3801, HF2 = 1016, SP0 = 5077, SP1 = 981;
    const int c = t.c, e = t.e;
    const int s0 = t.p2y + t.n2y, sm = t.p2m + t.n2m, sp = t.p2p + t.n2p;
    const int d = s0 >> 1;
    const int t0 = absdiff<BYTES>(t.p2y, t.n2y);
    const int t1 = (absdiff<BYTES>(t.pu, c) + absdiff<BYTES>(t.pl, e)) >> 1;
    const int t2 = (absdiff<BYTES>(t.nu, c) + absdiff<BYTES>(t.nl, e)) >> 1;
    const int diff = max(max(t0 >> 1, t1), t2);
    const int b = (sm >> 1) - c, g = (sp >> 1) - e;
    const int mx = max(max(d - e, d - c), min(b, g));
    const int mn = min(min(d - e, d - c), max(b, g));
    const int wide = inner ? max(max(diff, mn), -mx) : diff;
    const int ce = c + e, c3 = t.c3m + t.c3p, far = t.p2mm + t.n2mm + t.p2pp + t.n2pp;
    const int hf = ((mul24(HF0, s0) - mul24(HF1, sm + sp) + mul24(HF2, far)) >> 2) + mul24(LF0, ce) - mul24(LF1, c3);
    const int spat = mul24(SP0, ce) - mul24(SP1, c3);
    const int filt = (absdiff<BYTES>(c, e) > t0 ? hf : spat) >> 13;
    const int interp = line ? filt : ce >> 1;
    const int clamped = min(max(interp, d - wide), d + wide);
    return diff == 0 ? d : min(max(clamped, 0), top);
}

// What a launch works on.  Rows are `pitch` bytes apart on both sides.
// (Not an extension of FieldMatrix: the kernels read every field here and have no use for its shift, and with the two sides' fields apart
// every kernel's scalar-register count moved.)
struct Job {
    const uint8_t* src;          // plane of resident frame 0
    uint8_t* dst;                // plane of output frame 0
    long long stride, dst_stride, pitch;
    int n_frames, from, rows, cols, order, top;          // cols: samples of a row; top: 2^depth - 1
    int same;                                            // 1: output frame o is field 0 of source frame from + o (rate "same")
    const int32_t* flags;                                // masked entries (device, one per output frame of the launch): 0: copy the frame
};

// The rows and frames of output frame `o` of the launch and interpolated row index `ri`: false if there is no such row.
struct Where {
    const uint8_t *cur, *prev, *next, *p2, *n2;
    uint8_t* out;
    int y, up, dn, ym, yp;
    int y3m, y3p, y4m, y4p;          // rows y -+ 3 and y -+ 4 (bwdif)
    bool inner, line;
};

__device__ __forceinline__ bool locate(const Job& jb, int o, int ri, Where& w) {
    const int n = jb.from + (jb.same ? o : o >> 1), f = jb.same ? 0 : o & 1;
    const int p = jb.order == 0 ? f : 1 - f;
    const int y = 2 * ri + (1 - p);
    if (y >= jb.rows) return false;
    const int np = n > 0 ? n - 1 : 0, nn = n + 1 < jb.n_frames ? n + 1 : jb.n_frames - 1;
    w.cur = jb.src + (long long)n * jb.stride;
    w.prev = jb.src + (long long)np * jb.stride;
    w.next = jb.src + (long long)nn * jb.stride;
    w.p2 = f == 0 ? w.prev : w.cur;
    w.n2 = f == 0 ? w.cur : w.next;
    w.out = jb.dst + (long long)o * jb.dst_stride;
    w.y = y;
    w.up = y > 0 ? y - 1 : y + 1;
    w.dn = y < jb.rows - 1 ? y + 1 : y - 1;
    w.inner = y - 2 >= 0 && y + 2 <= jb.rows - 1;
    w.ym = w.inner ? y - 2 : y;          // (not used by the result when !inner: any row that exists)
    w.yp = w.inner ? y + 2 : y;
    w.line = y - 4 >= 0 && y + 4 <= jb.rows - 1;
    w.y3m = w.line ? y - 3 : w.up;       // (not used by the result when !line: any row that exists)
    w.y3p = w.line ? y + 3 : w.dn;
    w.y4m = w.line ? y - 4 : y;
    w.y4p = w.line ? y + 4 : y;
    return true;
}

// Sample i of a run of dwords: a constant bit field once the loops are unrolled.
template <int BYTES>
__device__ __forceinline__ int field(const uint32_t* w, int i, int top) {
    if constexpr (BYTES == 1) return (int)((w[i >> 2] >> (8 * (i & 3))) & 255u);
    else return min((int)((w[i >> 1] >> (16 * (i & 1))) & 0xffffu), top);
}

__device__ __forceinline__ u32x4 load16(const uint8_t* row, long long chunk) { return *(reinterpret_cast<const u32x4*>(row) + chunk); }

// An unflagged frame of the masked entries: the lane's rows (its interpolated row, the kept row above, the last row below) as they are.
__device__ __forceinline__ void copy_vec(const Job& jb, const Where& w, int chunk) {
    const long long P = jb.pitch;
    *(reinterpret_cast<u32x4*>(w.out + w.y * P) + chunk) = load16(w.cur + w.y * P, chunk);
    if (w.y > 0) *(reinterpret_cast<u32x4*>(w.out + (w.y - 1) * P) + chunk) = load16(w.cur + (w.y - 1) * P, chunk);
    if (w.y + 1 == jb.rows - 1) *(reinterpret_cast<u32x4*>(w.out + (w.y + 1) * P) + chunk) = load16(w.cur + (w.y + 1) * P, chunk);
}

// Vector form: lane = (interpolated row ri = tile + (tid >> 4), 16-byte chunk = tile + (tid & 15)).
template <int BYTES, int STEP, bool MASKED = false>
__global__ __launch_bounds__(DI_THREADS) void deinterlace_vec_kernel(Job jb) {
    constexpr int SPL = 16 / BYTES;          // samples of a chunk
    const int chunks = (int)(jb.pitch >> 4);
    const int chunk = (int)blockIdx.x * 16 + ((int)threadIdx.x & 15);
    const int ri = (int)blockIdx.y * DI_TILE_IROWS + ((int)threadIdx.x >> 4);
    Where w;
    if (chunk >= chunks || !locate(jb, (int)blockIdx.z, ri, w)) return;
    if constexpr (MASKED) {
        if (!jb.flags[blockIdx.z]) { copy_vec(jb, w, chunk); return; }
    }
    const long long P = jb.pitch;
    const int cl = chunk > 0 ? chunk - 1 : chunk, cr = chunk + 1 < chunks ? chunk + 1 : chunk;          // (clamped: read, never used, at the row's ends)
    uint32_t U[12], L[12];
    {
        const uint8_t *ru = w.cur + w.up * P, *rl = w.cur + w.dn * P;
        const u32x4 a0 = load16(ru, cl), a1 = load16(ru, chunk), a2 = load16(ru, cr);
        const u32x4 b0 = load16(rl, cl), b1 = load16(rl, chunk), b2 = load16(rl, cr);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            U[k] = a0[k]; U[4 + k] = a1[k]; U[8 + k] = a2[k];
            L[k] = b0[k]; L[4 + k] = b1[k]; L[8 + k] = b2[k];
        }
    }
    uint32_t Q[10][4];          // p2 / n2 at rows y, y - 2, y + 2; prev and next at the rows above and below
    {
        const u32x4 v0 = load16(w.p2 + w.y * P, chunk), v1 = load16(w.n2 + w.y * P, chunk);
        const u32x4 v2 = load16(w.p2 + w.ym * P, chunk), v3 = load16(w.n2 + w.ym * P, chunk);
        const u32x4 v4 = load16(w.p2 + w.yp * P, chunk), v5 = load16(w.n2 + w.yp * P, chunk);
        const u32x4 v6 = load16(w.prev + w.up * P, chunk), v7 = load16(w.prev + w.dn * P, chunk);
        const u32x4 v8 = load16(w.next + w.up * P, chunk), v9 = load16(w.next + w.dn * P, chunk);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            Q[0][k] = v0[k]; Q[1][k] = v1[k]; Q[2][k] = v2[k]; Q[3][k] = v3[k]; Q[4][k] = v4[k];
            Q[5][k] = v5[k]; Q[6][k] = v6[k]; Q[7][k] = v7[k]; Q[8][k] = v8[k]; Q[9][k] = v9[k];
        }
    }
    const int x0 = chunk * SPL;
    uint32_t res[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
        Taps t;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            t.u[k] = field<BYTES>(U, SPL + i + (k - 3) * STEP, jb.top);
            t.l[k] = field<BYTES>(L, SPL + i + (k - 3) * STEP, jb.top);
        }
        t.p2y = field<BYTES>(Q[0], i, jb.top); t.n2y = field<BYTES>(Q[1], i, jb.top);
        t.p2m = field<BYTES>(Q[2], i, jb.top); t.n2m = field<BYTES>(Q[3], i, jb.top);
        t.p2p = field<BYTES>(Q[4], i, jb.top); t.n2p = field<BYTES>(Q[5], i, jb.top);
        t.pu = field<BYTES>(Q[6], i, jb.top);  t.pl = field<BYTES>(Q[7], i, jb.top);
        t.nu = field<BYTES>(Q[8], i, jb.top);  t.nl = field<BYTES>(Q[9], i, jb.top);
        const int x = x0 + i;
        const int v = yadif<BYTES>(t, x - 3 * STEP >= 0 && x + 3 * STEP <= jb.cols - 1, w.inner);
        if constexpr (BYTES == 1) res[i >> 2] |= (uint32_t)v << (8 * (i & 3));
        else res[i >> 1] |= (uint32_t)v << (16 * (i & 1));
    }
    *(reinterpret_cast<u32x4*>(w.out + w.y * P) + chunk) = u32x4{res[0], res[1], res[2], res[3]};
    // the kept rows, as they are: the row above, and the matrix's last row where it lies below
    if (w.y > 0) *(reinterpret_cast<u32x4*>(w.out + (w.y - 1) * P) + chunk) = u32x4{U[4], U[5], U[6], U[7]};
    if (w.y + 1 == jb.rows - 1) *(reinterpret_cast<u32x4*>(w.out + (w.y + 1) * P) + chunk) = u32x4{L[4], L[5], L[6], L[7]};
}

template <int BYTES>
__device__ __forceinline__ int raw_at(const uint8_t* row, int x) {
    if constexpr (BYTES == 1) return row[x];
    else return reinterpret_cast<const uint16_t*>(row)[x];
}

template <int BYTES>
__device__ __forceinline__ void put_at(uint8_t* row, int x, int v) {
    if constexpr (BYTES == 1) row[x] = (uint8_t)v;
    else reinterpret_cast<uint16_t*>(row)[x] = (uint16_t)v;
}

template <int BYTES>
__device__ __forceinline__ void copy_one(const Job& jb, const Where& w, int x) {
    const long long P = jb.pitch;
    put_at<BYTES>(w.out + w.y * P, x, raw_at<BYTES>(w.cur + w.y * P, x));
    if (w.y > 0) put_at<BYTES>(w.out + (w.y - 1) * P, x, raw_at<BYTES>(w.cur + (w.y - 1) * P, x));
    if (w.y + 1 == jb.rows - 1) put_at<BYTES>(w.out + (w.y + 1) * P, x, raw_at<BYTES>(w.cur + (w.y + 1) * P, x));
}

// One-sample form: lane = (interpolated row ri = tile + wave, sample x = tile + lane).
template <int BYTES, bool MASKED = false>
__global__ __launch_bounds__(DI_THREADS) void deinterlace_one_kernel(Job jb, int step) {
    const int x = (int)blockIdx.x * DI_ONE_COLS + ((int)threadIdx.x & 63);
    const int ri = (int)blockIdx.y * DI_ONE_IROWS + ((int)threadIdx.x >> 6);
    Where w;
    if (x >= jb.cols || !locate(jb, (int)blockIdx.z, ri, w)) return;
    if constexpr (MASKED) {
        if (!jb.flags[blockIdx.z]) { copy_one<BYTES>(jb, w, x); return; }
    }
    const long long P = jb.pitch;
    const uint8_t *ru = w.cur + w.up * P, *rl = w.cur + w.dn * P;
    const bool edge = x - 3 * step >= 0 && x + 3 * step <= jb.cols - 1;
    Taps t;
    const int cu = raw_at<BYTES>(ru, x), cl = raw_at<BYTES>(rl, x);          // (unclipped: the kept rows' copies)
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const int xk = edge ? x + (k - 3) * step : x;          // (without the search only the middle tap is read)
        t.u[k] = min(raw_at<BYTES>(ru, xk), jb.top);
        t.l[k] = min(raw_at<BYTES>(rl, xk), jb.top);
    }
    t.p2y = min(raw_at<BYTES>(w.p2 + w.y * P, x), jb.top);  t.n2y = min(raw_at<BYTES>(w.n2 + w.y * P, x), jb.top);
    t.p2m = min(raw_at<BYTES>(w.p2 + w.ym * P, x), jb.top); t.n2m = min(raw_at<BYTES>(w.n2 + w.ym * P, x), jb.top);
    t.p2p = min(raw_at<BYTES>(w.p2 + w.yp * P, x), jb.top); t.n2p = min(raw_at<BYTES>(w.n2 + w.yp * P, x), jb.top);
    t.pu = min(raw_at<BYTES>(w.prev + w.up * P, x), jb.top); t.pl = min(raw_at<BYTES>(w.prev + w.dn * P, x), jb.top);
    t.nu = min(raw_at<BYTES>(w.next + w.up * P, x), jb.top); t.nl = min(raw_at<BYTES>(w.next + w.dn * P, x), jb.top);
    put_at<BYTES>(w.out + w.y * P, x, yadif<BYTES>(t, edge, w.inner));
    if (w.y > 0) put_at<BYTES>(w.out + (w.y - 1) * P, x, cu);
    if (w.y + 1 == jb.rows - 1) put_at<BYTES>(w.out + (w.y + 1) * P, x, cl);
}

// bwdif, vector form: the geometry of deinterlace_vec_kernel, 18 loads of the lane's own chunk.
template <int BYTES, bool MASKED = false>
__global__ __launch_bounds__(DI_THREADS) void bwdif_vec_kernel(Job jb) {
    constexpr int SPL = 16 / BYTES;
    const int chunks = (int)(jb.pitch >> 4);
    const int chunk = (int)blockIdx.x * 16 + ((int)threadIdx.x & 15);
    const int ri = (int)blockIdx.y * DI_TILE_IROWS + ((int)threadIdx.x >> 4);
    Where w;
    if (chunk >= chunks || !locate(jb, (int)blockIdx.z, ri, w)) return;
    if constexpr (MASKED) {
        if (!jb.flags[blockIdx.z]) { copy_vec(jb, w, chunk); return; }
    }
    const long long P = jb.pitch;
    uint32_t Q[18][4];
    {
        const u32x4 v0 = load16(w.cur + w.up * P, chunk), v1 = load16(w.cur + w.dn * P, chunk);
        const u32x4 v2 = load16(w.cur + w.y3m * P, chunk), v3 = load16(w.cur + w.y3p * P, chunk);
        const u32x4 v4 = load16(w.p2 + w.y * P, chunk), v5 = load16(w.n2 + w.y * P, chunk);
        const u32x4 v6 = load16(w.p2 + w.ym * P, chunk), v7 = load16(w.n2 + w.ym * P, chunk);
        const u32x4 v8 = load16(w.p2 + w.yp * P, chunk), v9 = load16(w.n2 + w.yp * P, chunk);
        const u32x4 v10 = load16(w.p2 + w.y4m * P, chunk), v11 = load16(w.n2 + w.y4m * P, chunk);
        const u32x4 v12 = load16(w.p2 + w.y4p * P, chunk), v13 = load16(w.n2 + w.y4p * P, chunk);
        const u32x4 v14 = load16(w.prev + w.up * P, chunk), v15 = load16(w.prev + w.dn * P, chunk);
        const u32x4 v16 = load16(w.next + w.up * P, chunk), v17 = load16(w.next + w.dn * P, chunk);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            Q[0][k] = v0[k]; Q[1][k] = v1[k]; Q[2][k] = v2[k]; Q[3][k] = v3[k]; Q[4][k] = v4[k]; Q[5][k] = v5[k];
            Q[6][k] = v6[k]; Q[7][k] = v7[k]; Q[8][k] = v8[k]; Q[9][k] = v9[k]; Q[10][k] = v10[k]; Q[11][k] = v11[k];
            Q[12][k] = v12[k]; Q[13][k] = v13[k]; Q[14][k] = v14[k]; Q[15][k] = v15[k]; Q[16][k] = v16[k]; Q[17][k] = v17[k];
        }
    }
    uint32_t res[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
        BTaps t;
        t.c = field<BYTES>(Q[0], i, jb.top);     t.e = field<BYTES>(Q[1], i, jb.top);
        t.c3m = field<BYTES>(Q[2], i, jb.top);   t.c3p = field<BYTES>(Q[3], i, jb.top);
        t.p2y = field<BYTES>(Q[4], i, jb.top);   t.n2y = field<BYTES>(Q[5], i, jb.top);
        t.p2m = field<BYTES>(Q[6], i, jb.top);   t.n2m = field<BYTES>(Q[7], i, jb.top);
        t.p2p = field<BYTES>(Q[8], i, jb.top);   t.n2p = field<BYTES>(Q[9], i, jb.top);
        t.p2mm = field<BYTES>(Q[10], i, jb.top); t.n2mm = field<BYTES>(Q[11], i, jb.top);
        t.p2pp = field<BYTES>(Q[12], i, jb.top); t.n2pp = field<BYTES>(Q[13], i, jb.top);
        t.pu = field<BYTES>(Q[14], i, jb.top);   t.pl = field<BYTES>(Q[15], i, jb.top);
        t.nu = field<BYTES>(Q[16], i, jb.top);   t.nl = field<BYTES>(Q[17], i, jb.top);
        const int v = bwdif<BYTES>(t, w.inner, w.line, jb.top);
        if constexpr (BYTES == 1) res[i >> 2] |= (uint32_t)v << (8 * (i & 3));
        else res[i >> 1] |= (uint32_t)v << (16 * (i & 1));
    }
    *(reinterpret_cast<u32x4*>(w.out + w.y * P) + chunk) = u32x4{res[0], res[1], res[2], res[3]};
    // the kept rows, as they are: the row above, and the matrix's last row where it lies below
    if (w.y > 0) *(reinterpret_cast<u32x4*>(w.out + (w.y - 1) * P) + chunk) = u32x4{Q[0][0], Q[0][1], Q[0][2], Q[0][3]};
    if (w.y + 1 == jb.rows - 1) *(reinterpret_cast<u32x4*>(w.out + (w.y + 1) * P) + chunk) = u32x4{Q[1][0], Q[1][1], Q[1][2], Q[1][3]};
}

// bwdif, one-sample form: the geometry of deinterlace_one_kernel.
template <int BYTES, bool MASKED = false>
__global__ __launch_bounds__(DI_THREADS) void bwdif_one_kernel(Job jb) {
    const int x = (int)blockIdx.x * DI_ONE_COLS + ((int)threadIdx.x & 63);
    const int ri = (int)blockIdx.y * DI_ONE_IROWS + ((int)threadIdx.x >> 6);
    Where w;
    if (x >= jb.cols || !locate(jb, (int)blockIdx.z, ri, w)) return;
    if constexpr (MASKED) {
        if (!jb.flags[blockIdx.z]) { copy_one<BYTES>(jb, w, x); return; }
    }
    const long long P = jb.pitch;
    const int cu = raw_at<BYTES>(w.cur + w.up * P, x), cl = raw_at<BYTES>(w.cur + w.dn * P, x);          // (unclipped: the kept rows' copies)
    BTaps t;
    t.c = min(cu, jb.top); t.e = min(cl, jb.top);
    t.c3m = min(raw_at<BYTES>(w.cur + w.y3m * P, x), jb.top); t.c3p = min(raw_at<BYTES>(w.cur + w.y3p * P, x), jb.top);
    t.p2y = min(raw_at<BYTES>(w.p2 + w.y * P, x), jb.top);    t.n2y = min(raw_at<BYTES>(w.n2 + w.y * P, x), jb.top);
    t.p2m = min(raw_at<BYTES>(w.p2 + w.ym * P, x), jb.top);   t.n2m = min(raw_at<BYTES>(w.n2 + w.ym * P, x), jb.top);
    t.p2p = min(raw_at<BYTES>(w.p2 + w.yp * P, x), jb.top);   t.n2p = min(raw_at<BYTES>(w.n2 + w.yp * P, x), jb.top);
    t.p2mm = min(raw_at<BYTES>(w.p2 + w.y4m * P, x), jb.top); t.n2mm = min(raw_at<BYTES>(w.n2 + w.y4m * P, x), jb.top);
    t.p2pp = min(raw_at<BYTES>(w.p2 + w.y4p * P, x), jb.top); t.n2pp = min(raw_at<BYTES>(w.n2 + w.y4p * P, x), jb.top);
    t.pu = min(raw_at<BYTES>(w.prev + w.up * P, x), jb.top);  t.pl = min(raw_at<BYTES>(w.prev + w.dn * P, x), jb.top);
    t.nu = min(raw_at<BYTES>(w.next + w.up * P, x), jb.top);  t.nl = min(raw_at<BYTES>(w.next + w.dn * P, x), jb.top);
    put_at<BYTES>(w.out + w.y * P, x, bwdif<BYTES>(t, w.inner, w.line, jb.top));
    if (w.y > 0) put_at<BYTES>(w.out + (w.y - 1) * P, x, cu);
    if (w.y + 1 == jb.rows - 1) put_at<BYTES>(w.out + (w.y + 1) * P, x, cl);
}

// n_out output frames of source frames jb.from ...: two per source frame, or one with jb.same.  method 0: yadif, 1: bwdif.
// MASKED: jb.flags has one entry per output frame (jb.same is 1); the workgroups of a frame whose entry is 0 copy it.
template <int BYTES, bool MASKED>
int launch_deinterlace(Job jb, int step, int n_out, hipStream_t st, int method) {
    const bool vec = aligned16(jb.src, jb.stride, jb.pitch) && aligned16(jb.dst, jb.dst_stride, 0);
    const int irows = (jb.rows + 1) / 2;          // of the field with more interpolated rows; the other one's last tile row may be empty
    const unsigned gx = vec ? blocks(jb.pitch, DI_TILE_BYTES) : blocks(jb.cols, DI_ONE_COLS), gy = blocks(irows, vec ? DI_TILE_IROWS : DI_ONE_IROWS);
    return for_frame_chunks(n_out, DI_MAX_OUT, [&](int o0, int no) {
        const dim3 grid(gx, gy, (unsigned)no), block(DI_THREADS);
        Job part = jb;
        part.from = jb.from + (jb.same ? o0 : o0 / 2);
        part.dst = jb.dst + (long long)o0 * jb.dst_stride;
        if (MASKED) part.flags = jb.flags + o0;
        if (method == 1) {
            if (vec) hipLaunchKernelGGL((bwdif_vec_kernel<BYTES, MASKED>), grid, block, 0, st, part);
            else hipLaunchKernelGGL((bwdif_one_kernel<BYTES, MASKED>), grid, block, 0, st, part);
            return check_launch(vec ? "bwdif_vec_kernel" : "bwdif_one_kernel");
        }
        if (vec && BYTES == 2) hipLaunchKernelGGL((deinterlace_vec_kernel<2, 1, MASKED>), grid, block, 0, st, part);
        else if (vec && step == 1) hipLaunchKernelGGL((deinterlace_vec_kernel<1, 1, MASKED>), grid, block, 0, st, part);
        else if (vec && step == 2) hipLaunchKernelGGL((deinterlace_vec_kernel<1, 2, MASKED>), grid, block, 0, st, part);
        else if (vec && step == 3) hipLaunchKernelGGL((deinterlace_vec_kernel<1, 3, MASKED>), grid, block, 0, st, part);
        else if (vec) hipLaunchKernelGGL((deinterlace_vec_kernel<1, 4, MASKED>), grid, block, 0, st, part);
        else hipLaunchKernelGGL((deinterlace_one_kernel<BYTES, MASKED>), grid, block, 0, st, part, step);
        return check_launch(vec ? "deinterlace_vec_kernel" : "deinterlace_one_kernel");
    });
}


// The body of the six entries.  width: row_bytes (_u8) or cols (_u16); sd: the pixel step (_u8) or the depth (_u16).  The plain entries pass
// method 0, rate 0 and no flags; the masked ones ((ABI 49), behind the pulldown removal's combed=) rate 1 and their flags: rate "same" for
// the frames whose flag is set, a byte copy of the others; the flags are a device table the entry cannot see.
template <int BYTES, bool MASKED>
int deinterlace(const char* who, const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int width, int sd, int order,
                int from, int to, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset, int method, int rate, const int32_t* flags, void* stream) {
    constexpr MatrixRule rule{2, DI_MAX_ROWS, "rows <= 524280", "the range needs 0 <= from < to <= n_frames", false};
    const int64_t row_bytes = (int64_t)BYTES * width;
    const char* why = check_matrix(rule, frames && out ? frames : nullptr, n_frames, frame_bytes, plane_offset, rows, row_bytes, order, from, to, out_plane_offset);
    if (!why) why = check_out_plane(out_frame_bytes, out_plane_offset, rows, row_bytes);
    if (why) return refuse(who, why);
    if (BYTES == 1) {
        if (sd < 1 || sd > 4 || width % sd) return refuse(who, "step 1 .. 4 and a divisor of row_bytes");
    } else if (int rc = check_samples16(who, sd, frames, frame_bytes, plane_offset, true, out, out_frame_bytes, out_plane_offset)) {
        return rc;
    }
    if (MASKED)
        if (const char* bad = check_table(flags, !flags, "flags must be 4-byte aligned")) return refuse(who, bad);
    if (method != 0 && method != 1) return refuse(who, "method 0 (yadif) or 1 (bwdif)");
    if (rate != 0 && rate != 1) return refuse(who, "rate 0 (double) or 1 (same)");
    if (MASKED && out < frames + (int64_t)n_frames * frame_bytes && frames < out + (int64_t)(to - from) * out_frame_bytes)
        return refuse(who, "the source frames and the output overlap");
    const Job jb{frames + plane_offset, out + out_plane_offset, frame_bytes, out_frame_bytes, row_bytes, n_frames, from, rows, width, order,
                 BYTES == 1 ? 255 : (1 << sd) - 1, rate, flags};
    return launch_deinterlace<BYTES, MASKED>(jb, BYTES == 1 ? sd : 1, (rate ? 1 : 2) * (to - from), static_cast<hipStream_t>(stream), method);
}

}  // namespace
}  // namespace savsr

using namespace savsr;

extern "C" int savsr_video_deinterlace_u8(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int row_bytes,
                                          int step, int order, int from, int to, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset,
                                          void* stream) {
    return deinterlace<1, false>("video_deinterlace_u8", frames, n_frames, frame_bytes, plane_offset, rows, row_bytes, step, order, from, to, out, out_frame_bytes,
                                 out_plane_offset, 0, 0, nullptr, stream);
}

extern "C" int savsr_video_deinterlace_u8_m(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int row_bytes,
                                            int step, int order, int from, int to, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset,
                                            int method, int rate, void* stream) {
    return deinterlace<1, false>("video_deinterlace_u8_m", frames, n_frames, frame_bytes, plane_offset, rows, row_bytes, step, order, from, to, out, out_frame_bytes,
                                 out_plane_offset, method, rate, nullptr, stream);
}

extern "C" int savsr_video_deinterlace_u16(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols,
                                           int depth, int order, int from, int to, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset,
                                           void* stream) {
    return deinterlace<2, false>("video_deinterlace_u16", frames, n_frames, frame_bytes, plane_offset, rows, cols, depth, order, from, to, out, out_frame_bytes,
                                 out_plane_offset, 0, 0, nullptr, stream);
}

extern "C" int savsr_video_deinterlace_u16_m(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols,
                                             int depth, int order, int from, int to, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset,
                                             int method, int rate, void* stream) {
    return deinterlace<2, false>("video_deinterlace_u16_m", frames, n_frames, frame_bytes, plane_offset, rows, cols, depth, order, from, to, out, out_frame_bytes,
                                 out_plane_offset, method, rate, nullptr, stream);
}

extern "C" int savsr_video_deinterlace_masked_u8(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int row_bytes,
                                                 int step, int order, int from, int to, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset,
                                                 int method, const int32_t* flags, void* stream) {
    return deinterlace<1, true>("video_deinterlace_masked_u8", frames, n_frames, frame_bytes, plane_offset, rows, row_bytes, step, order, from, to, out, out_frame_bytes,
                                 out_plane_offset, method, 1, flags, stream);
}

extern "C" int savsr_video_deinterlace_masked_u16(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols,
                                                  int depth, int order, int from, int to, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset,
                                                  int method, const int32_t* flags, void* stream) {
    return deinterlace<2, true>("video_deinterlace_masked_u16", frames, n_frames, frame_bytes, plane_offset, rows, cols, depth, order, from, to, out, out_frame_bytes,
                                 out_plane_offset, method, 1, flags, stream);
}
