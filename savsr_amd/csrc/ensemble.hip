// Geometric self-ensemble (ABI 33; SAVSR.set_self_ensemble): the input side expands a clip into its 8 flip /
// transpose variants, the output side undoes each variant on its network output and averages the 8 in one pass.  The network runs
// between the two unchanged; satu.hip, tail.hip and common.hpp are not touched (savsr_source_hash_satu() and hr_plans.json stay valid).
//
// Variant k:  fw = k & 1 (flip width), fh = (k >> 1) & 1 (flip height), t = k >> 2 (transpose the last two dims).  Forward: the flips,
// then the transpose (lbasicsr/models/sr_model.py:162-164, `v`, `h`, `t`); inverse: the transpose, then the flips (:178-184).
//
//   savsr_ensemble_gather_u8 / _f32  frames -> fp32 clip slots of variant k ([c][h][w], or [c][w][h] when t is set)
//   savsr_ensemble_merge             the 8 outputs -> ((((o0 + o1) + o2) + ...) + o7) * 0.125f, fp32 [c][H][W] or uint8 [H][W][c]
#include "common.hpp"

#include <cstdint>

namespace savsr {
namespace {

// np.float32(u) / 255.0 for every byte value, the table of video.hip (a constant expression: the compiler rounds each division once),
// so a variant-0 gather equals savsr_video_gather_u8 bit for bit.
struct U8Table { float v[256]; };
constexpr U8Table make_u8_table() {
    U8Table t{};
    for (int i = 0; i < 256; ++i) t.v[i] = static_cast<float>(i) / 255.0f;
    return t;
}
__constant__ U8Table kEnsU8ToF32 = make_u8_table();

struct EnsIdx { int32_t f[SAVSR_VIDEO_MAX_SLOTS]; };     // slot -> frame, by value in the kernel arguments
struct EnsOffs { long long o[8]; };                      // variant -> element offset of its output from the base pointer

constexpr int TILE = 32;        // transposing tiles: 32 x 32 elements, rows padded to 33 floats
constexpr int TPAD = TILE + 1;

template <bool U8>
__device__ __forceinline__ float load_px(const void* frame, const float* lut, int c, int h, int w, int ch, int y, int x) {
    if (U8) return lut[static_cast<const uint8_t*>(frame)[((long long)y * w + x) * c + ch]];      // [h][w][c] interleaved
    return static_cast<const float*>(frame)[((long long)ch * h + y) * w + x];                     // [c][h][w] planar
}

// Plain variants (t = 0): out slot [c][h][w], out[ch][y][x] = frame(fh ? h-1-y : y, fw ? w-1-x : x).  A thread writes 4 consecutive
// pixels of one plane row, one float4 when VEC (w % 4 == 0, 16-byte aligned out); the source reads run backwards along a flipped row.
template <bool U8, bool VEC>
__global__ __launch_bounds__(256) void ens_gather_plain_kernel(const void* __restrict__ src, int c, int h, int w, EnsIdx idx, int fw, int fh,
                                                               float* __restrict__ out) {
    __shared__ float lut[256];
    if (U8) {
        lut[threadIdx.x] = kEnsU8ToF32.v[threadIdx.x];
        __syncthreads();
    }
    const int s = blockIdx.y;
    const long long npx = (long long)h * w;
    const void* frame = U8 ? (const void*)(static_cast<const uint8_t*>(src) + (long long)idx.f[s] * npx * c)
                           : (const void*)(static_cast<const float*>(src) + (long long)idx.f[s] * npx * c);
    float* o = out + (long long)s * c * npx;
    const int wq = (w + 3) / 4;                              // 4-pixel groups per row
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long long)h * wq) return;
    const int y = (int)(g / wq), x0 = (int)(g % wq) * 4;
    const int sy = fh ? h - 1 - y : y;
    for (int ch = 0; ch < c; ++ch) {
        float* orow = o + ((long long)ch * h + y) * w;
        if (VEC) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = load_px<U8>(frame, lut, c, h, w, ch, sy, fw ? w - 1 - (x0 + e) : x0 + e);
            *reinterpret_cast<f32x4*>(orow + x0) = v;
        } else {
            for (int e = 0; e < 4 && x0 + e < w; ++e) orow[x0 + e] = load_px<U8>(frame, lut, c, h, w, ch, sy, fw ? w - 1 - (x0 + e) : x0 + e);
        }
    }
}

// Transposed variants (t = 1): out slot [c][w][h], out[ch][i][j] = frame(fh ? h-1-j : j, fw ? w-1-i : i).  A 32 x 32 tile per workgroup
// (grid.x along j, grid.y along i): the source rows are read with the lanes along x (consecutive addresses, descending when fw) into
// tile[j][i], the slot rows written with the lanes along j from tile[j][i] -- row pitch 33 floats, so both phases put the 32 lanes of a
// half-wave on 32 different banks.
template <bool U8>
__global__ __launch_bounds__(256) void ens_gather_tr_kernel(const void* __restrict__ src, int c, int h, int w, EnsIdx idx, int fw, int fh,
                                                            float* __restrict__ out) {
    __shared__ float lut[256];
    __shared__ float tile[3][TILE][TPAD];
    if (U8) lut[threadIdx.x] = kEnsU8ToF32.v[threadIdx.x];
    __syncthreads();
    const int s = blockIdx.z;
    const long long npx = (long long)h * w;
    const void* frame = U8 ? (const void*)(static_cast<const uint8_t*>(src) + (long long)idx.f[s] * npx * c)
                           : (const void*)(static_cast<const float*>(src) + (long long)idx.f[s] * npx * c);
    float* o = out + (long long)s * c * npx;
    const int j0 = blockIdx.x * TILE, i0 = blockIdx.y * TILE;
    const int lane = threadIdx.x & 31, row = threadIdx.x >> 5;
#pragma unroll
    for (int r = 0; r < TILE / 8; ++r) {                    // read: tile[jl][il] = frame(row of j, column of i)
        const int jl = row + 8 * r, il = lane;
        const int j = j0 + jl, i = i0 + il;
        if (j < h && i < w) {
            const int sy = fh ? h - 1 - j : j, sx = fw ? w - 1 - i : i;
            for (int ch = 0; ch < c; ++ch) tile[ch][jl][il] = load_px<U8>(frame, lut, c, h, w, ch, sy, sx);
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < TILE / 8; ++r) {                    // write: out[ch][i][j], the lanes along j
        const int il = row + 8 * r, jl = lane;
        const int i = i0 + il, j = j0 + jl;
        if (i < w && j < h) {
            for (int ch = 0; ch < c; ++ch) o[((long long)ch * w + i) * h + j] = tile[ch][jl][il];
        }
    }
}

__device__ __forceinline__ uint32_t ens_quant_u8(float x) {
    return (uint32_t)rintf(fminf(fmaxf(x, 0.f), 1.f) * 255.0f);      // savsr_video_quantize_u8's rule: clamp, x 255.0f, half to even
}

// The merge.  A workgroup owns a 32 x 32 tile of the output (Y0.., X0..); a thread owns 4 consecutive pixels of one row (yl = tid / 8,
// X = X0 + 4 (tid % 8)) in every channel.  Per channel: the 4 plain inputs are read straight (a flipped row's 4 pixels are one float4 read
// backwards when VEC), the 4 transposed inputs are staged through tile[v][X][Y] (lanes along Y, their contiguous axis) and read back
// with a half-wave on 8 X quads x 4 rows: banks 33 * 4q + yl = 4q + yl (mod 32), all different.  The sum runs k = 0 .. 7 in that order.
// VEC: H % 4 == 0 is not needed, W % 4 == 0 and 16-byte aligned inputs / fp32 output (4-byte aligned uint8 output).
template <int C, bool OUT_U8, bool VEC>
__global__ __launch_bounds__(256) void ens_merge_kernel(const float* __restrict__ base, EnsOffs offs, int H, int W, void* __restrict__ out) {
    __shared__ float tile[4][TILE][TPAD];
    const int X0 = blockIdx.x * TILE, Y0 = blockIdx.y * TILE;
    const int tid = threadIdx.x;
    const int yl = tid >> 3, xl = (tid & 7) * 4;
    const int Y = Y0 + yl, X = X0 + xl;
    const long long plane = (long long)H * W;
    float acc[C][4];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        // transposed inputs of this channel -> LDS (tile[v][il][jl] = o_{4+v}[ch][fw ? W-1-X : X][fh ? H-1-Y : Y])
        if (ch > 0) __syncthreads();                        // (the previous channel's reads of the tiles are done)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int fw = v & 1, fh = v >> 1;
            const float* src = base + offs.o[4 + v] + ch * plane;          // [W][H]
#pragma unroll
            for (int r = 0; r < TILE / 8; ++r) {
                const int il = (tid >> 5) + 8 * r, jl = tid & 31;
                const int x = X0 + il, y = Y0 + jl;
                if (x < W && y < H) tile[v][il][jl] = src[(long long)(fw ? W - 1 - x : x) * H + (fh ? H - 1 - y : y)];
            }
        }
        // plain inputs straight into registers
        float p[4][4] = {};
        if (Y < H) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int fw = v & 1, fh = v >> 1;
                const float* row = base + offs.o[v] + ch * plane + (long long)(fh ? H - 1 - Y : Y) * W;
                if (VEC) {
                    if (X < W) {
                        const f32x4 q = *reinterpret_cast<const f32x4*>(row + (fw ? W - 4 - X : X));
#pragma unroll
                        for (int e = 0; e < 4; ++e) p[v][e] = fw ? q[3 - e] : q[e];
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) p[v][e] = X + e < W ? row[fw ? W - 1 - (X + e) : X + e] : 0.f;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float s = p[0][e];
            s = s + p[1][e];
            s = s + p[2][e];
            s = s + p[3][e];
#pragma unroll
            for (int v = 0; v < 4; ++v) s = s + tile[v][xl + e][yl];
            acc[ch][e] = s * 0.125f;
        }
    }
    if (Y >= H || X >= W) return;
    const long long px = (long long)Y * W + X;
    if (!OUT_U8) {
        float* o = static_cast<float*>(out);
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            if (VEC) {
                f32x4 q;
#pragma unroll
                for (int e = 0; e < 4; ++e) q[e] = acc[ch][e];
                *reinterpret_cast<f32x4*>(o + ch * plane + px) = q;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (X + e < W) o[ch * plane + px + e] = acc[ch][e];
            }
        }
    } else {
        uint8_t* o = static_cast<uint8_t*>(out) + px * C;          // [H][W][C]
        if (VEC) {                                                  // 4 pixels x C bytes = C dwords, 4-byte aligned (X % 4 == 0, W % 4 == 0)
            uint32_t wv[C];
#pragma unroll
            for (int j = 0; j < C; ++j) wv[j] = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int ch = 0; ch < C; ++ch) {
                    const int b = e * C + ch;
                    wv[b >> 2] |= ens_quant_u8(acc[ch][e]) << (8 * (b & 3));
                }
            uint32_t* d = reinterpret_cast<uint32_t*>(o);
#pragma unroll
            for (int j = 0; j < C; ++j) d[j] = wv[j];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (X + e < W)
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) o[e * C + ch] = (uint8_t)ens_quant_u8(acc[ch][e]);
        }
    }
}

int load_ens_idx(const int32_t* idx, int n, int n_frames, EnsIdx* gi, const char* what) {
    if (!idx) { set_error("%s: null index list", what); return SAVSR_E_ARG; }
    if (n < 1 || n > SAVSR_VIDEO_MAX_SLOTS) { set_error("%s: %d slots (1 .. %d)", what, n, SAVSR_VIDEO_MAX_SLOTS); return SAVSR_E_ARG; }
    for (int i = 0; i < n; ++i) {
        if (idx[i] < 0 || idx[i] >= n_frames) { set_error("%s: slot %d names frame %d of %d", what, i, idx[i], n_frames); return SAVSR_E_ARG; }
        gi->f[i] = idx[i];
    }
    return 0;
}

template <bool U8>
int ens_gather(const void* frames, int n_frames, int c, int h, int w, const int32_t* idx, int n_idx, int k, float* out, void* stream,
               const char* what) {
    if (!frames || !out) { set_error("%s: null pointer", what); return SAVSR_E_ARG; }
    if (c < 1 || c > 3 || h < 1 || w < 1 || n_frames < 1) { set_error("%s: c in 1 .. 3, h, w, n_frames >= 1", what); return SAVSR_E_ARG; }
    if (k < 0 || k > 7) { set_error("%s: variant %d (0 .. 7)", what, k); return SAVSR_E_ARG; }
    EnsIdx gi;
    if (int rc = load_ens_idx(idx, n_idx, n_frames, &gi, what)) return rc;
    const int fw = k & 1, fh = (k >> 1) & 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (k >> 2) {
        const dim3 grid((h + TILE - 1) / TILE, (w + TILE - 1) / TILE, n_idx);
        hipLaunchKernelGGL((ens_gather_tr_kernel<U8>), grid, dim3(256), 0, st, frames, c, h, w, gi, fw, fh, out);
        return check_launch("ens_gather_tr_kernel");
    }
    const bool vec = w % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const long long groups = (long long)h * ((w + 3) / 4);
    const dim3 grid((unsigned)((groups + 255) / 256), n_idx);
    if (vec) hipLaunchKernelGGL((ens_gather_plain_kernel<U8, true>), grid, dim3(256), 0, st, frames, c, h, w, gi, fw, fh, out);
    else hipLaunchKernelGGL((ens_gather_plain_kernel<U8, false>), grid, dim3(256), 0, st, frames, c, h, w, gi, fw, fh, out);
    return check_launch("ens_gather_plain_kernel");
}

}  // namespace
}  // namespace savsr

using namespace savsr;

extern "C" int savsr_ensemble_gather_u8(const uint8_t* frames, int n_frames, int c, int h, int w, const int32_t* idx, int n_idx, int k,
                                        float* out, void* stream) {
    return ens_gather<true>(frames, n_frames, c, h, w, idx, n_idx, k, out, stream, "ensemble_gather_u8");
}

extern "C" int savsr_ensemble_gather_f32(const float* frames, int n_frames, int c, int h, int w, const int32_t* idx, int n_idx, int k,
                                         float* out, void* stream) {
    return ens_gather<false>(frames, n_frames, c, h, w, idx, n_idx, k, out, stream, "ensemble_gather_f32");
}

extern "C" int savsr_ensemble_merge(const float* base, const int64_t* offs, int c, int H, int W, int out_u8, void* out, void* stream) {
    if (!base || !offs || !out) return fail_arg("ensemble_merge: null pointer");
    if (c < 1 || c > 3 || H < 1 || W < 1) return fail_arg("ensemble_merge: c in 1 .. 3, H, W >= 1");
    if (out_u8 != 0 && out_u8 != 1) return fail_arg("ensemble_merge: out_u8 is 0 or 1");
    if ((H + TILE - 1) / TILE > 65535) return fail_arg("ensemble_merge: H too large");
    EnsOffs eo;
    bool aligned = (reinterpret_cast<uintptr_t>(out) & (out_u8 ? 3 : 15)) == 0;
    for (int k = 0; k < 8; ++k) {
        eo.o[k] = offs[k];
        aligned = aligned && ((reinterpret_cast<uintptr_t>(base + offs[k]) & 15) == 0);
    }
    const bool vec = W % 4 == 0 && aligned;
    const dim3 grid((W + TILE - 1) / TILE, (H + TILE - 1) / TILE);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define SAVSR_ENS_MERGE(CC, U)                                                                                 \
    if (vec) hipLaunchKernelGGL((ens_merge_kernel<CC, U, true>), grid, dim3(256), 0, st, base, eo, H, W, out); \
    else hipLaunchKernelGGL((ens_merge_kernel<CC, U, false>), grid, dim3(256), 0, st, base, eo, H, W, out);
#define SAVSR_ENS_MERGE_C(CC)                  \
    if (out_u8) { SAVSR_ENS_MERGE(CC, true) }  \
    else { SAVSR_ENS_MERGE(CC, false) }
    switch (c) {
        case 1: SAVSR_ENS_MERGE_C(1) break;
        case 2: SAVSR_ENS_MERGE_C(2) break;
        default: SAVSR_ENS_MERGE_C(3) break;
    }
#undef SAVSR_ENS_MERGE_C
#undef SAVSR_ENS_MERGE
    return check_launch("ens_merge_kernel");
}
