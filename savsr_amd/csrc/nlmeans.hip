// Spatial noise reduction in front of the network (ABI 51): non-local means in 32-bit integers, every frame on its own
// (savsr_amd/nlmeans.py `nlm_matrix` is the specification; the kernels equal it bit for bit).  Output sample p is the weighted mean of
// the candidates q = p + (dy, dx), |dy|, |dx| <= S, that lie inside the plane, w = W[((SSD >> 2 (depth - 8)) * 64) / D] (0 from k = 577
// on), SSD the sum of squared differences of the (2 P + 1)^2 patches around p and q with coordinates clamped to the plane.
//
//   _u8    planes of rows x (cols * step) bytes; sample x of a row meets samples x +- k * step only (step = the channels of packed frames)
//   _u16   the same in little-endian 16-bit samples, every sample read as min(s, 2^depth - 1)
//
// One launch per call, grid = (tile column, tile row, frame * step + channel), 256 lanes.  A workgroup owns a tile of 64 rows x
// (64 - 2 P) columns of outputs and stages the tile plus a halo of S + P samples into LDS with clamped coordinates, as 16-bit values
// (84 rows x 80 columns at the largest P and S: 13 440 bytes, and the 578 weights as words: 2 312), so the border rule costs nothing
// afterwards and one form serves every size, pointer and step.  A wave owns 16 rows; a lane owns one column of the staged tile, keeps
// that column's 16 + 2 P samples in registers for the whole call and, per offset, walks down it: one LDS read (the candidate's column),
// one squared difference, the running sum over 2 P + 1 rows kept with a register ring of the differences that leave it (the loop is
// unrolled, so the ring's index is a constant), and the sum over 2 P + 1 neighbouring columns taken from the neighbouring lanes with
// DPP wave shifts (P to the left and P to the right: no LDS traffic).  The P lanes at either end of a wave have no full window and
// write nothing: the tile's columns overlap by 2 P.  That is (16 + 2 P) / 16 squared differences per candidate where the naive form has
// (2 P + 1)^2.  k's division by D is a multiply by m = ceil(2^(28 + l) / D), l = ceil(log2 D), and a shift: exact for
// every n < 2^28 because m D - 2^(28 + l) < D <= 2^l (Granlund and Montgomery); the dividend is passed shifted left by 4 so that the
// product's high word is enough.  The weight comes from the table in LDS; accumulators are 32-bit (nlmeans.py has the bounds).
#include "common.hpp"
#include "video_samples.hpp"
#include "field_matrix.hpp"
#include "nlmeans_weights.hpp"

#include <cstdint>

namespace savsr {
namespace {

constexpr int NLM_THREADS = 256;
constexpr int NLM_MAX_PATCH = 3, NLM_MAX_SEARCH = 7;
constexpr int NLM_MAX_DIVISOR = 65536;          // 2^16: the magic multiplier stays below 2^29 + 1 (the callers' largest is 49 * 32^2 = 50176)
constexpr int NLM_MAX_STEP = 4;
constexpr int NLM_STRIP = 16;                   // output rows of a wave
constexpr int NLM_TILE_ROWS = NLM_STRIP * (NLM_THREADS / 64);
constexpr int NLM_PITCH = 64 + 2 * NLM_MAX_SEARCH + 2;                                   // 16-bit samples of a staged row
constexpr int NLM_LDS_ROWS = NLM_TILE_ROWS + 2 * (NLM_MAX_PATCH + NLM_MAX_SEARCH);

struct NlmJob {
    const uint8_t* src;          // the plane of frame 0
    uint8_t* dst;                // the plane of output frame 0
    long long stride, dst_stride, pitch;          // bytes between frames (either side) and between rows
    int rows, cols, step, search;
    uint32_t top;                // 2^depth - 1
    int shift;                   // 2 (depth - 8)
    uint32_t magic;              // ceil(2^(28 + lg) / D)
    int lg;                      // ceil(log2 D)
};

// Sample (y, x) of channel ch of a plane, coordinates clamped to it.
template <int BYTES>
__device__ __forceinline__ uint32_t nlm_sample(const NlmJob& jb, const uint8_t* plane, int ch, int y, int x) {
    y = min(max(y, 0), jb.rows - 1);
    x = min(max(x, 0), jb.cols - 1);
    const uint8_t* row = plane + (long long)y * jb.pitch;
    const long long s = (long long)x * jb.step + ch;
    if constexpr (BYTES == 1) return row[s];
    else return min((uint32_t)reinterpret_cast<const uint16_t*>(row)[s], jb.top);
}

// The table index of a patch distance: min(((ssd >> shift) * 64) / D, 577).
__device__ __forceinline__ uint32_t nlm_bucket(uint32_t ssd, const NlmJob& jb) {
    const uint32_t n = (ssd >> jb.shift) << 10;          // ((ssd >> shift) * 64) << 4, below 2^32
    const uint32_t k = (uint32_t)(((unsigned long long)n * jb.magic) >> 32) >> jb.lg;
    return min(k, (uint32_t)NLM_N_WEIGHTS);
}

__device__ __forceinline__ uint32_t nlm_mean(uint32_t sv, uint32_t sw) { return (sv + (sw >> 1)) / sw; }

template <int BYTES>
__device__ __forceinline__ void nlm_store(const NlmJob& jb, uint8_t* plane, int ch, int y, int x, uint32_t v) {
    uint8_t* row = plane + (long long)y * jb.pitch;
    const long long s = (long long)x * jb.step + ch;
    if constexpr (BYTES == 1) row[s] = (uint8_t)v;
    else reinterpret_cast<uint16_t*>(row)[s] = (uint16_t)v;
}

#ifdef SAVSR_HOST_CHECK
// The host check's form (one thread at a time, no LDS and no wave): a lane owns one output sample and evaluates the rule with the
// device functions above, every patch term from memory.  The tiled kernel below is what the GPU runs.
template <int BYTES, int P>
__global__ void nlm_tile_kernel(NlmJob jb) {
    const int x = (int)(blockIdx.x * NLM_THREADS + threadIdx.x) % jb.cols, y = (int)(blockIdx.x * NLM_THREADS + threadIdx.x) / jb.cols;
    if (y >= jb.rows) return;
    const int f = (int)blockIdx.z / jb.step, ch = (int)blockIdx.z % jb.step;
    const uint8_t* plane = jb.src + (long long)f * jb.stride;
    uint32_t sw = 0, sv = 0;
    for (int dy = -jb.search; dy <= jb.search; ++dy)
        for (int dx = -jb.search; dx <= jb.search; ++dx) {
            if (y + dy < 0 || y + dy >= jb.rows || x + dx < 0 || x + dx >= jb.cols) continue;
            uint32_t ssd = 0;
            for (int i = -P; i <= P; ++i)
                for (int j = -P; j <= P; ++j) {
                    const int d = (int)nlm_sample<BYTES>(jb, plane, ch, y + i, x + j) - (int)nlm_sample<BYTES>(jb, plane, ch, y + dy + i, x + dx + j);
                    ssd += (uint32_t)(d * d);
                }
            const uint32_t w = NLM_WEIGHTS[nlm_bucket(ssd, jb)];
            sw += w;
            sv += w * nlm_sample<BYTES>(jb, plane, ch, y + dy, x + dx);
        }
    nlm_store<BYTES>(jb, jb.dst + (long long)f * jb.dst_stride, ch, y, x, nlm_mean(sv, sw));
}

template <int P>
inline dim3 nlm_grid(const NlmJob& jb, int nf) { return dim3(blocks((long long)jb.rows * jb.cols, NLM_THREADS), 1, (unsigned)(nf * jb.step)); }
#else
// The sum of c over the lanes l - P .. l + P of the wave (lanes outside it count 0; those lanes' outputs are not used).
template <int P>
__device__ __forceinline__ uint32_t nlm_across(uint32_t c) {
    uint32_t s = c, l = c, r = c;
#pragma unroll
    for (int k = 0; k < P; ++k) {
        l = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)l, 0x138, 0xf, 0xf, true);          // wave_shr:1
        r = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)r, 0x130, 0xf, 0xf, true);          // wave_shl:1
        s += l + r;
    }
    return s;
}

template <int BYTES, int P>
__global__ __launch_bounds__(NLM_THREADS) void nlm_tile_kernel(NlmJob jb) {
    constexpr int N = 2 * P + 1, WALK = NLM_STRIP + 2 * P, TW = 64 - 2 * P;
    __shared__ uint16_t tile[NLM_LDS_ROWS * NLM_PITCH];
    __shared__ uint32_t wtab[NLM_N_WEIGHTS + 1];
    const int S = jb.search, tid = (int)threadIdx.x;
    const int tx0 = (int)blockIdx.x * TW, ty0 = (int)blockIdx.y * NLM_TILE_ROWS;
    const int f = (int)blockIdx.z / jb.step, ch = (int)blockIdx.z % jb.step;
    const uint8_t* plane = jb.src + (long long)f * jb.stride;
    {   // the tile and its halo, coordinates clamped: staged row r is plane row ty0 - P - S + r, staged column c is plane column tx0 - P - S + c
        const int w = 64 + 2 * S, n = (NLM_TILE_ROWS + 2 * (P + S)) * w;
        for (int i = tid; i < n; i += NLM_THREADS) {
            const int r = i / w, c = i - r * w;
            tile[r * NLM_PITCH + c] = (uint16_t)nlm_sample<BYTES>(jb, plane, ch, ty0 - P - S + r, tx0 - P - S + c);
        }
        for (int i = tid; i <= NLM_N_WEIGHTS; i += NLM_THREADS) wtab[i] = NLM_WEIGHTS[i];
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    const int y0 = ty0 + wave * NLM_STRIP, x = tx0 - P + lane;          // the strip's first output row; the lane's column
    if (y0 >= jb.rows) return;          // (a whole wave: the lanes of a wave stay together for the shifts)
    // the lane's column: walk row j is plane row y0 - P + j, staged row wave * STRIP + S + j
    const uint16_t* own = tile + (wave * NLM_STRIP + S) * NLM_PITCH + lane + S;
    int col[WALK];
#pragma unroll
    for (int j = 0; j < WALK; ++j) col[j] = own[j * NLM_PITCH];
    uint32_t sw[NLM_STRIP], sv[NLM_STRIP];
#pragma unroll
    for (int j = 0; j < NLM_STRIP; ++j) sw[j] = sv[j] = 0u;
    for (int dy = -S; dy <= S; ++dy) {
        for (int dx = -S; dx <= S; ++dx) {
            const uint16_t* cand = own + dy * NLM_PITCH + dx;
            const bool x_in = (unsigned)(x + dx) < (unsigned)jb.cols;
            uint32_t ring[N], vq[P + 1], c = 0u;
#pragma unroll
            for (int j = 0; j < WALK; ++j) {
                const int q = cand[j * NLM_PITCH], d = col[j] - q;
                const uint32_t dd = (uint32_t)(d * d);
                c += dd;
                if (j >= N) c -= ring[j % N];          // the row that left the window
                ring[j % N] = dd;
                vq[j % (P + 1)] = (uint32_t)q;
                if (j >= 2 * P) {          // the window is rows j - 2 P .. j: output row o = j - 2 P of the strip, its own row is walk row j - P
                    const int o = j - 2 * P;
                    const bool taken = x_in && (unsigned)(y0 + o + dy) < (unsigned)jb.rows;
                    const uint32_t w = wtab[max(nlm_bucket(nlm_across<P>(c), jb), taken ? 0u : (uint32_t)NLM_N_WEIGHTS)];          // (entry 577 is 0)
                    sw[o] += w;
                    sv[o] += __umul24(w, vq[(j - P) % (P + 1)]);          // (w <= 4096 and a sample <= 4095: 24 bits hold both)
                }
            }
        }
    }
    if (lane < P || lane >= 64 - P || x >= jb.cols) return;
    uint8_t* out = jb.dst + (long long)f * jb.dst_stride;
#pragma unroll
    for (int o = 0; o < NLM_STRIP; ++o)
        if (y0 + o < jb.rows) nlm_store<BYTES>(jb, out, ch, y0 + o, x, nlm_mean(sv[o], sw[o]));
}

template <int P>
inline dim3 nlm_grid(const NlmJob& jb, int nf) {
    return dim3(blocks(jb.cols, 64 - 2 * P), blocks(jb.rows, NLM_TILE_ROWS), (unsigned)(nf * jb.step));
}
#endif

template <int BYTES, int P>
int nlm_launch(const NlmJob& jb, int nf, hipStream_t st) {
    hipLaunchKernelGGL((nlm_tile_kernel<BYTES, P>), nlm_grid<P>(jb, nf), dim3(NLM_THREADS), 0, st, jb);
    return check_launch("nlm_tile_kernel");
}

// The body of the two entries.  cols: pixels of a row; step: samples of a pixel.
template <int BYTES>
int nlmeans(const char* who, const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step, int depth,
            int patch, int search, int divisor, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset, void* stream) {
    constexpr MatrixRule rule{1, 0, nullptr, "", false};
    if (step < 1 || step > NLM_MAX_STEP) return refuse(who, "step 1 .. 4 (the samples of a pixel)");
    if (cols < 1) return refuse(who, "a row holds at least one sample");
    const int64_t row_bytes = (int64_t)BYTES * cols * step;
    const char* why = check_matrix(rule, frames && out ? frames : nullptr, n_frames, frame_bytes, plane_offset, rows, row_bytes, 0, 0, n_frames, out_plane_offset);
    if (!why) why = check_out_plane(out_frame_bytes, out_plane_offset, rows, row_bytes);
    if (why) return refuse(who, why);
    if (BYTES == 2)
        if (int rc = check_samples16(who, depth, frames, frame_bytes, plane_offset, true, out, out_frame_bytes, out_plane_offset)) return rc;
    if (patch < 1 || patch > NLM_MAX_PATCH) return refuse(who, "patch 1 .. 3");
    if (search < 1 || search > NLM_MAX_SEARCH) return refuse(who, "search 1 .. 7");
    if (divisor < 1 || divisor > NLM_MAX_DIVISOR) return refuse(who, "divisor 1 .. 65536");
    if (out < frames + (int64_t)n_frames * frame_bytes && frames < out + (int64_t)n_frames * out_frame_bytes)
        return refuse(who, "the source frames and the output overlap");
    int lg = 0;
    while ((1 << lg) < divisor) ++lg;
    const unsigned long long pow = 1ull << (28 + lg);
    const NlmJob jb{frames + plane_offset, out + out_plane_offset, frame_bytes, out_frame_bytes, row_bytes, rows, cols, step, search,
                    (1u << depth) - 1u, 2 * (depth - 8), (uint32_t)((pow + divisor - 1) / divisor), lg};
    hipStream_t st = static_cast<hipStream_t>(stream);
    return for_frame_chunks(n_frames, FM_MAX_FRAMES / NLM_MAX_STEP, [&](int f0, int nf) {
        NlmJob part = jb;
        part.src = jb.src + (long long)f0 * jb.stride;
        part.dst = jb.dst + (long long)f0 * jb.dst_stride;
        return patch == 1 ? nlm_launch<BYTES, 1>(part, nf, st) : patch == 2 ? nlm_launch<BYTES, 2>(part, nf, st) : nlm_launch<BYTES, 3>(part, nf, st);
    });
}

}  // namespace
}  // namespace savsr

using namespace savsr;

extern "C" int savsr_video_nlmeans_u8(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step,
                                      int patch, int search, int divisor, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset,
                                      void* stream) {
    return nlmeans<1>("video_nlmeans_u8", frames, n_frames, frame_bytes, plane_offset, rows, cols, step, 8, patch, search, divisor, out, out_frame_bytes,
                      out_plane_offset, stream);
}

extern "C" int savsr_video_nlmeans_u16(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step,
                                       int depth, int patch, int search, int divisor, uint8_t* out, int64_t out_frame_bytes,
                                       int64_t out_plane_offset, void* stream) {
    return nlmeans<2>("video_nlmeans_u16", frames, n_frames, frame_bytes, plane_offset, rows, cols, step, depth, patch, search, divisor, out,
                      out_frame_bytes, out_plane_offset, stream);
}
