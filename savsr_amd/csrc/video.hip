// The sequence path's conversions on either side of the network (ABI 31): uint8 frames -> the fp32 clip batch the engine stages,
// and the fp32 result -> uint8 frames for an encoder.  Neither is fused into the SATU / tail kernels (satu.hip, tail.hip and
// common.hpp stay as they are, and with them savsr_source_hash_satu() and savsr_amd/hr_plans.json).
//
//   read_img_seq / img2tensor   lbasicsr/data/data_util.py:29-60   uint8 -> float32 / 255.0, HWC -> CHW
//   generate_frame_indices      lbasicsr/data/data_util.py:63-112  the window's frame list (the caller's index arguments)
//   tensor2img                  lbasicsr/utils/img_util.py:66-90   clamp(0, 1) * 255, round half to even, uint8, CHW -> HWC
#include "common.hpp"
#include "video_samples.hpp"
#include "dither.hpp"

#include <cstdint>

namespace savsr {
namespace {

// np.float32(u) / 255.0 for every byte value: a constant expression, so the compiler evaluates the IEEE division once, correctly
// rounded (round to nearest even), exactly as numpy's float32 division does.  The kernels index this table; no division on the device.
struct U8Table { float v[256]; };
constexpr U8Table make_u8_table() {
    U8Table t{};
    for (int i = 0; i < 256; ++i) t.v[i] = static_cast<float>(i) / 255.0f;
    return t;
}
__constant__ U8Table kU8ToF32 = make_u8_table();

// The frame of every output slot, passed by value in the kernel arguments (no index tensor, no host -> device copy).
struct GatherIdx { int32_t f[SAVSR_VIDEO_MAX_SLOTS]; };

inline unsigned blocks_for(long long units) { return (unsigned)((units + 255) / 256); }

// uint8 HWC frames [N][h][w][C] -> fp32 planar slots [n][C][h][w], slot k = frame idx.f[k].  A thread converts 4 pixels of one slot;
// VEC: 4 C bytes as C dwords in, one float4 per plane out (npx % 4 == 0, 4-byte aligned frames, 16-byte aligned out).
template <int C, bool VEC>
__global__ __launch_bounds__(256) void gather_u8_kernel(const uint8_t* __restrict__ src, long long npx, GatherIdx idx, float* __restrict__ out) {
    __shared__ float lut[256];
    lut[threadIdx.x] = kU8ToF32.v[threadIdx.x];
    __syncthreads();
    const int k = blockIdx.y;
    const uint8_t* f = src + (long long)idx.f[k] * npx * C;
    float* o = out + (long long)k * C * npx;
    const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= npx) return;
    if (VEC) {
        const uint32_t* s = reinterpret_cast<const uint32_t*>(f + p0 * C);
        uint32_t wv[C];
#pragma unroll
        for (int j = 0; j < C; ++j) wv[j] = s[j];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int b = e * C + ch;
                v[e] = lut[(wv[b >> 2] >> (8 * (b & 3))) & 255u];
            }
            *reinterpret_cast<f32x4*>(o + ch * npx + p0) = v;
        }
    } else {
        for (int e = 0; e < 4 && p0 + e < npx; ++e) {
#pragma unroll
            for (int ch = 0; ch < C; ++ch) o[ch * npx + p0 + e] = lut[f[(p0 + e) * C + ch]];
        }
    }
}

// fp32 planar frames [N][C][h][w] -> slots [n][C][h][w]: a whole-frame copy per slot, float4 where npx * C % 4 == 0.
template <bool VEC>
__global__ __launch_bounds__(256) void gather_f32_kernel(const float* __restrict__ src, long long nfl, GatherIdx idx, float* __restrict__ out) {
    const int k = blockIdx.y;
    const float* f = src + (long long)idx.f[k] * nfl;
    float* o = out + (long long)k * nfl;
    const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= nfl) return;
    if (VEC) {
        *reinterpret_cast<f32x4*>(o + i0) = *reinterpret_cast<const f32x4*>(f + i0);
    } else {
        for (int e = 0; e < 4 && i0 + e < nfl; ++e) o[i0 + e] = f[i0 + e];
    }
}

// fp32 planar [n][C][H][W] -> uint8 HWC [n][H][W][C].  VEC: a thread quantises 16 pixels -- four float4 per plane in, C 16-byte stores
// out (npx % 16 == 0, 16-byte aligned pointers); otherwise one pixel per thread.  DITHER (savsr_video_quantize_u8_d): floor(t + theta)
// in rint's place (dither.hpp), theta at the pixel's (y, x) = (p / W, p % W) and shared by its channels; a vector thread's run of 16
// pixels crosses row ends whenever W is no multiple of 16, so it splits p once (dither_row_col) and walks (y, x) from there.  Without
// DITHER, dv is not read.
template <int C, bool VEC, bool DITHER>
__global__ __launch_bounds__(256) void quantize_u8_kernel(const float* __restrict__ in, long long npx, uint8_t* __restrict__ out, DitherDiv dv) {
    const int k = blockIdx.y;
    const float* src = in + (long long)k * C * npx;
    uint8_t* dst = out + (long long)k * C * npx;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        const long long p0 = g * 16;
        if (p0 >= npx) return;
        float th[16];
        if constexpr (DITHER) {
            uint32_t y, x;
            dither_row_col(p0, dv, y, x);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                th[i] = dither_theta(y, x);
                if (++x == dv.w) { x = 0u; ++y; }
            }
        }
        uint32_t wv[4 * C];
#pragma unroll
        for (int j = 0; j < 4 * C; ++j) wv[j] = 0u;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
#pragma unroll
            for (int v4 = 0; v4 < 4; ++v4) {
                const f32x4 x = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + ch * npx + p0) + v4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int b = (4 * v4 + e) * C + ch;
                    if constexpr (DITHER) wv[b >> 2] |= dither_quant_unit(x[e], 255.0f, th[4 * v4 + e]) << (8 * (b & 3));
                    else wv[b >> 2] |= quant_u8(x[e]) << (8 * (b & 3));
                }
            }
        }
        uint4* d = reinterpret_cast<uint4*>(dst + p0 * C);
#pragma unroll
        for (int j = 0; j < C; ++j) d[j] = make_uint4(wv[4 * j], wv[4 * j + 1], wv[4 * j + 2], wv[4 * j + 3]);
    } else {
        if (g >= npx) return;
        if constexpr (DITHER) {
            uint32_t y, x;
            dither_row_col(g, dv, y, x);
            const float th = dither_theta(y, x);
#pragma unroll
            for (int ch = 0; ch < C; ++ch) dst[g * C + ch] = (uint8_t)dither_quant_unit(src[ch * npx + g], 255.0f, th);
        } else {
#pragma unroll
            for (int ch = 0; ch < C; ++ch) dst[g * C + ch] = (uint8_t)quant_u8(src[ch * npx + g]);
        }
    }
}

int load_idx(const int32_t* idx, int n, int n_frames, GatherIdx* gi, const char* what) {
    if (!idx) { set_error("%s: null index list", what); return SAVSR_E_ARG; }
    if (n < 1 || n > SAVSR_VIDEO_MAX_SLOTS) { set_error("%s: %d slots (1 .. %d)", what, n, SAVSR_VIDEO_MAX_SLOTS); return SAVSR_E_ARG; }
    for (int i = 0; i < n; ++i) {
        if (idx[i] < 0 || idx[i] >= n_frames) { set_error("%s: slot %d names frame %d of %d", what, i, idx[i], n_frames); return SAVSR_E_ARG; }
        gi->f[i] = idx[i];
    }
    return 0;
}

}  // namespace
}  // namespace savsr

using namespace savsr;

extern "C" int savsr_video_gather_u8(const uint8_t* frames, int n_frames, int c, int h, int w, const int32_t* idx, int n_idx, float* out,
                                     void* stream) {
    if (!frames || !out) return fail_arg("video_gather_u8: null pointer");
    if (c < 1 || c > 3 || h < 1 || w < 1 || n_frames < 1) return fail_arg("video_gather_u8: c in 1 .. 3, h, w, n_frames >= 1");
    GatherIdx gi;
    if (int rc = load_idx(idx, n_idx, n_frames, &gi, "video_gather_u8")) return rc;
    const long long npx = (long long)h * w;
    const bool vec = npx % 4 == 0 && (reinterpret_cast<uintptr_t>(frames) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const dim3 grid(blocks_for((npx + 3) / 4), n_idx);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define SAVSR_GATHER_U8(CC)                                                                                       \
    if (vec) hipLaunchKernelGGL((gather_u8_kernel<CC, true>), grid, dim3(256), 0, st, frames, npx, gi, out);      \
    else hipLaunchKernelGGL((gather_u8_kernel<CC, false>), grid, dim3(256), 0, st, frames, npx, gi, out);
    switch (c) {
        case 1: SAVSR_GATHER_U8(1) break;
        case 2: SAVSR_GATHER_U8(2) break;
        default: SAVSR_GATHER_U8(3) break;
    }
#undef SAVSR_GATHER_U8
    return check_launch("gather_u8_kernel");
}

extern "C" int savsr_video_gather_f32(const float* frames, int n_frames, int c, int h, int w, const int32_t* idx, int n_idx, float* out,
                                      void* stream) {
    if (!frames || !out) return fail_arg("video_gather_f32: null pointer");
    if (c < 1 || c > 3 || h < 1 || w < 1 || n_frames < 1) return fail_arg("video_gather_f32: c in 1 .. 3, h, w, n_frames >= 1");
    GatherIdx gi;
    if (int rc = load_idx(idx, n_idx, n_frames, &gi, "video_gather_f32")) return rc;
    const long long nfl = (long long)c * h * w;
    const bool vec = nfl % 4 == 0 && (reinterpret_cast<uintptr_t>(frames) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const dim3 grid(blocks_for((nfl + 3) / 4), n_idx);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL((gather_f32_kernel<true>), grid, dim3(256), 0, st, frames, nfl, gi, out);
    else hipLaunchKernelGGL((gather_f32_kernel<false>), grid, dim3(256), 0, st, frames, nfl, gi, out);
    return check_launch("gather_f32_kernel");
}

// The body of savsr_video_quantize_u8 and savsr_video_quantize_u8_d: `what` names the one called in its messages.
static int quantize_u8(const char* what, const float* in, int n, int c, int H, int W, bool dither, uint8_t* out, void* stream) {
    if (!in || !out) { set_error("invalid argument: %s: null pointer", what); return SAVSR_E_ARG; }
    if (n < 1 || n > 65535 || c < 1 || c > 3 || H < 1 || W < 1) {
        set_error("invalid argument: %s: n in 1 .. 65535, c in 1 .. 3, H, W >= 1", what);
        return SAVSR_E_ARG;
    }
    const long long npx = (long long)H * W;
    const bool vec = npx % 16 == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const dim3 grid(blocks_for(vec ? npx / 16 : npx), n);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const DitherDiv dv = dither_div(W);
#define SAVSR_QUANT_D(CC, D)                                                                                       \
    if (vec) hipLaunchKernelGGL((quantize_u8_kernel<CC, true, D>), grid, dim3(256), 0, st, in, npx, out, dv);      \
    else hipLaunchKernelGGL((quantize_u8_kernel<CC, false, D>), grid, dim3(256), 0, st, in, npx, out, dv);
#define SAVSR_QUANT(CC) if (dither) { SAVSR_QUANT_D(CC, true) } else { SAVSR_QUANT_D(CC, false) }
    switch (c) {
        case 1: SAVSR_QUANT(1) break;
        case 2: SAVSR_QUANT(2) break;
        default: SAVSR_QUANT(3) break;
    }
#undef SAVSR_QUANT
#undef SAVSR_QUANT_D
    return check_launch("quantize_u8_kernel");
}

extern "C" int savsr_video_quantize_u8(const float* in, int n, int c, int H, int W, uint8_t* out, void* stream) {
    return quantize_u8("video_quantize_u8", in, n, c, H, W, false, out, stream);
}

// dither 0: the kernels and the bytes of savsr_video_quantize_u8; 1: ordered dither (savsr_amd/dither.py).
extern "C" int savsr_video_quantize_u8_d(const float* in, int n, int c, int H, int W, int dither, uint8_t* out, void* stream) {
    if (dither != SAVSR_DITHER_NONE && dither != SAVSR_DITHER_ORDERED) {
        set_error("invalid argument: video_quantize_u8_d: dither %d (0 = none, 1 = ordered)", dither);
        return SAVSR_E_ARG;
    }
    return quantize_u8("video_quantize_u8_d", in, n, c, H, W, dither == SAVSR_DITHER_ORDERED, out, stream);
}
