// Luma-only checkpoints (num_in_ch = 1) on planar YUV and grey-scale video (ABI 41): the Y plane goes through the network, Cb / Cr go from
// samples to samples through a separable, siting-aware cubic at the network's scale.  The counterparts of savsr_video_gather_yuvs /
// _quantize_yuvs (yuv.hip) for a network that never forms RGB; like them not fused into the SATU / tail kernels (satu.hip, tail.hip and
// common.hpp stay as they are, and with them savsr_source_hash_satu() and savsr_amd/hr_plans.json).  savsr_amd/yuv.py (`luma_to_unit`,
// `unit_to_luma`, `chroma_axis_table`, `resample_chroma`) restates every kernel here bit for bit: float32 with a fixed operation order
// and no fused multiply-add (the whole file is compiled with fp contraction off).
//
//   gather    min(s, 2^d - 1) as float, divided by 255 * 2^(d - 8): one IEEE division (hipcc's float division is correctly rounded), the
//             value of video.hip's byte table at 8 bits.
//   quantise  rintf(clamp(v, 0, 1) * (255 * 2^(d - 8))), half to even, NaN -> 0: video.hip's quant_u8 at 8 bits.
//   resample  one launch per plane serves both axes: a workgroup owns a TILE_H x TILE_W tile of output chroma samples, stages the
//             horizontally filtered input rows its tile needs in LDS as float32 (LDS_ROWS rows of TILE_W at a time) and runs the vertical
//             pass from LDS.  A tile whose rows need more input rows than one buffer holds (downscaling, many vertical taps) loops over
//             buffers: the vertical sum takes its taps in ascending row order, so cutting it at buffer boundaries changes no bit.
#pragma clang fp contract(off)
#include "common.hpp"
#include "dither.hpp"

#include <cstdint>

namespace savsr {
namespace {

struct LumaIdx { int32_t f[SAVSR_VIDEO_MAX_SLOTS]; };

typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));

template <typename S> struct Vec4;
template <> struct Vec4<uint8_t> { typedef uint32_t type; };
template <> struct Vec4<uint16_t> { typedef u16x4 type; };

template <typename S> __device__ __forceinline__ uint32_t sample_of(typename Vec4<S>::type v, int e);
template <> __device__ __forceinline__ uint32_t sample_of<uint8_t>(uint32_t v, int e) { return (v >> (8 * e)) & 255u; }
template <> __device__ __forceinline__ uint32_t sample_of<uint16_t>(u16x4 v, int e) { return v[e]; }

template <typename S> __device__ __forceinline__ typename Vec4<S>::type pack4(const uint32_t (&q)[4]);
template <> __device__ __forceinline__ uint32_t pack4<uint8_t>(const uint32_t (&q)[4]) { return q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24); }
template <> __device__ __forceinline__ u16x4 pack4<uint16_t>(const uint32_t (&q)[4]) {
    return u16x4{(uint16_t)q[0], (uint16_t)q[1], (uint16_t)q[2], (uint16_t)q[3]};
}

inline unsigned blocks_for(long long units) { return (unsigned)((units + 255) / 256); }

// Y planes [h * w] of S samples, `stride` bytes from frame to frame -> fp32 slots [n][h * w], slot k = frame idx.f[k].  A thread converts
// 4 samples.  VEC: 4 samples in one access (a dword or 8 bytes), one float4 out.
template <typename S, bool VEC>
__global__ __launch_bounds__(256) void gather_luma_kernel(const uint8_t* __restrict__ src, long long stride, long long npx, uint32_t top, float den,
                                                          LumaIdx idx, float* __restrict__ out) {
    const int k = blockIdx.y;
    const S* f = reinterpret_cast<const S*>(src + (long long)idx.f[k] * stride);
    float* o = out + (long long)k * npx;
    const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= npx) return;
    if (VEC) {
        const typename Vec4<S>::type v = *reinterpret_cast<const typename Vec4<S>::type*>(f + p0);
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = (float)min(sample_of<S>(v, e), top) / den;
        *reinterpret_cast<f32x4*>(o + p0) = r;
    } else {
        for (int e = 0; e < 4 && p0 + e < npx; ++e) o[p0 + e] = (float)min((uint32_t)f[p0 + e], top) / den;
    }
}

__device__ __forceinline__ uint32_t quant_luma(float x, float mul) {
    return (uint32_t)rintf(fminf(fmaxf(x, 0.f), 1.f) * mul);      // clamp (fmaxf(NaN, 0) = 0), x 255 k, half to even
}

// fp32 [n][H * W] -> the Y plane of every output frame, `stride` bytes from frame to frame.  A thread quantises 4 samples; VEC: one
// nontemporal float4 in, one dword or 8-byte store out.  DITHER (savsr_video_quantize_luma_d): floor(t + theta) in rint's place
// (dither.hpp), theta at the sample's (y, x) = (p / W, p % W) (dither_row_col).  VEC has W % 4 == 0, so its 4 samples lie in one row from
// a multiple of 4 (dither_theta4); the scalar form's 4 may cross row ends and walk (y, x).  Without DITHER, dv is not read.
template <typename S, bool VEC, bool DITHER>
__global__ __launch_bounds__(256) void quantize_luma_kernel(const float* __restrict__ in, long long npx, float mul, uint8_t* __restrict__ out,
                                                            long long stride, DitherDiv dv) {
    const int k = blockIdx.y;
    const float* src = in + (long long)k * npx;
    S* dst = reinterpret_cast<S*>(out + (long long)k * stride);
    const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= npx) return;
    uint32_t y = 0u, x0 = 0u;
    if constexpr (DITHER) dither_row_col(p0, dv, y, x0);
    if (VEC) {
        const f32x4 x = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + p0));
        uint32_t q[4];
        float th[4];
        if constexpr (DITHER) dither_theta4(y, x0, th);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if constexpr (DITHER) q[e] = dither_quant_unit(x[e], mul, th[e]);
            else q[e] = quant_luma(x[e], mul);
        }
        *reinterpret_cast<typename Vec4<S>::type*>(dst + p0) = pack4<S>(q);
    } else {
        for (int e = 0; e < 4 && p0 + e < npx; ++e) {
            if constexpr (DITHER) {
                dst[p0 + e] = (S)dither_quant_unit(__builtin_nontemporal_load(src + p0 + e), mul, dither_theta(y, x0));
                if (++x0 == dv.w) { x0 = 0u; ++y; }
            } else {
                dst[p0 + e] = (S)quant_luma(__builtin_nontemporal_load(src + p0 + e), mul);
            }
        }
    }
}

// The chroma resampler.  256 threads own TILE_H x TILE_W output samples, thread t the 4 consecutive samples (t >> 4, 4 (t & 15) ..) of the
// tile.  LDS: LDS_ROWS x TILE_W floats = 8 KiB, static.  Every index read from the tables is clamped into the plane, so a wrong table
// gives wrong samples and never an access outside the planes.  The two axes treat a window that runs past the plane (xmin + xsize > cw,
// ymin + ysize > ch: no table of chroma_axis_table does) differently: the horizontal pass reads the last column again for such taps, as
// the numpy restatement does on both axes; the vertical pass drops them (the staged rows end at the plane's last row).
constexpr int TILE_H = 16, TILE_W = 64, LDS_ROWS = 32;

struct ResampleParams {
    const uint8_t* src;
    uint8_t* dst;
    long long src_frame_bytes, dst_frame_bytes;      // the plane offsets are already added to src / dst
    int ch, cw, cH, cW;
    const int32_t* ymin;
    const int32_t* ysize;
    const float* wy;
    int taps_y;
    const int32_t* xmin;
    const int32_t* xsize;
    const float* wx;
    int taps_x;
    uint32_t top_in;
    float scale, top_out;                             // 2^(D - d); 2^D - 1
    int vec;                                          // 4 output samples in one store: cW % 4 == 0 and dst / its stride aligned to them
};

template <typename SI, typename SO>
__global__ __launch_bounds__(256) void resample_chroma_kernel(const ResampleParams p) {
    __shared__ __attribute__((aligned(16))) float rows[LDS_ROWS][TILE_W];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * TILE_H;
    const SI* src = reinterpret_cast<const SI*>(p.src + (long long)blockIdx.z * p.src_frame_bytes);
    SO* dst = reinterpret_cast<SO*>(p.dst + (long long)blockIdx.z * p.dst_frame_bytes);
    const int th = min(TILE_H, p.cH - y0);
    // the input rows the tile's output rows read: [lo, hi)
    int lo = p.ch, hi = 0;
    for (int r = 0; r < th; ++r) {
        const int a = min(max(p.ymin[y0 + r], 0), p.ch - 1);
        const int n = min(max(p.ysize[y0 + r], 0), p.taps_y);
        lo = min(lo, a);
        hi = max(hi, min(a + n, p.ch));
    }
    const int ty = tid >> 4, tx = (tid & 15) * 4;
    const int yo = y0 + ty;
    const bool live = ty < th && x0 + tx < p.cW;
    int ya = 0, yn = 0;
    const float* wyr = p.wy;
    if (live) {
        ya = min(max(p.ymin[yo], 0), p.ch - 1);
        yn = min(max(p.ysize[yo], 0), p.taps_y);
        wyr = p.wy + (long long)yo * p.taps_y;
    }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = lo; c0 < hi; c0 += LDS_ROWS) {
        const int cn = min(LDS_ROWS, hi - c0);
        __syncthreads();                                  // (the previous buffer has been read)
        for (int e = tid; e < cn * TILE_W; e += 256) {
            const int r = e / TILE_W, c = e - r * TILE_W;
            const int xo = x0 + c;
            float a = 0.f;
            if (xo < p.cW) {
                const SI* row = src + (long long)(c0 + r) * p.cw;
                const int xa = min(max(p.xmin[xo], 0), p.cw - 1);
                const int n = min(max(p.xsize[xo], 0), p.taps_x);
                const float* wv = p.wx + (long long)xo * p.taps_x;
                for (int j = 0; j < n; ++j) a = a + wv[j] * (float)min((uint32_t)row[min(xa + j, p.cw - 1)], p.top_in);
            }
            rows[r][c] = a;
        }
        __syncthreads();
        if (live) {
            const int j0 = max(c0 - ya, 0), j1 = min(c0 + cn - ya, yn);
            for (int j = j0; j < j1; ++j) {
                const float wv = wyr[j];
                const f32x4 s = *reinterpret_cast<const f32x4*>(&rows[ya + j - c0][tx]);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = acc[e] + wv * s[e];
            }
        }
    }
    if (!live) return;
    uint32_t q[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) q[e] = (uint32_t)fminf(fmaxf(rintf(acc[e] * p.scale), 0.f), p.top_out);
    SO* o = dst + (long long)yo * p.cW + x0 + tx;
    if (p.vec) {
        *reinterpret_cast<typename Vec4<SO>::type*>(o) = pack4<SO>(q);
    } else {
        for (int e = 0; e < 4 && x0 + tx + e < p.cW; ++e) o[e] = (SO)q[e];
    }
}

int fail_align(const char* what) {
    set_error("alignment: %s", what);
    return SAVSR_E_ALIGN;
}

bool depth_ok(int d) { return d == 8 || d == 10 || d == 12; }

}  // namespace
}  // namespace savsr

using namespace savsr;

extern "C" int savsr_video_gather_luma(const uint8_t* frames, int n_frames, int64_t frame_bytes, int h, int w, int depth, const int32_t* idx,
                                       int n_idx, float* out, void* stream) {
    if (!frames || !out) return fail_arg("video_gather_luma: null pointer");
    if (h < 1 || w < 1 || n_frames < 1) return fail_arg("video_gather_luma: h, w, n_frames >= 1");
    if (!depth_ok(depth)) return fail_arg("video_gather_luma: depth is 8, 10 or 12");
    const int s = depth == 8 ? 1 : 2;
    const long long npx = (long long)h * w;
    if (frame_bytes < npx * s) return fail_arg("video_gather_luma: frame_bytes is smaller than the Y plane (h * w samples)");
    if (s == 2 && ((reinterpret_cast<uintptr_t>(frames) & 1) || (frame_bytes & 1)))
        return fail_align("video_gather_luma: 16-bit samples need a 2-byte aligned frame pointer and an even frame_bytes");
    if (!idx) return fail_arg("video_gather_luma: null index list");
    if (n_idx < 1 || n_idx > SAVSR_VIDEO_MAX_SLOTS) { set_error("video_gather_luma: %d slots (1 .. %d)", n_idx, SAVSR_VIDEO_MAX_SLOTS); return SAVSR_E_ARG; }
    LumaIdx gi;
    for (int i = 0; i < n_idx; ++i) {
        if (idx[i] < 0 || idx[i] >= n_frames) { set_error("video_gather_luma: slot %d names frame %d of %d", i, idx[i], n_frames); return SAVSR_E_ARG; }
        gi.f[i] = idx[i];
    }
    const int va = 4 * s;
    const bool vec = w % 4 == 0 && (reinterpret_cast<uintptr_t>(frames) % va) == 0 && frame_bytes % va == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const uint32_t top = (1u << depth) - 1u;
    const float den = (float)(255 << (depth - 8));
    const dim3 grid(blocks_for((npx + 3) / 4), n_idx);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define SAVSR_GATHER_LUMA(S, V) hipLaunchKernelGGL((gather_luma_kernel<S, V>), grid, dim3(256), 0, st, frames, (long long)frame_bytes, npx, top, den, gi, out)
    if (s == 1) { if (vec) SAVSR_GATHER_LUMA(uint8_t, true); else SAVSR_GATHER_LUMA(uint8_t, false); }
    else { if (vec) SAVSR_GATHER_LUMA(uint16_t, true); else SAVSR_GATHER_LUMA(uint16_t, false); }
#undef SAVSR_GATHER_LUMA
    return check_launch("gather_luma_kernel");
}

// The body of savsr_video_quantize_luma and savsr_video_quantize_luma_d: `what` names the one called in its messages.
static int quantize_luma(const char* what, const float* in, int n, int H, int W, int depth, bool dither, uint8_t* out, int64_t out_frame_bytes,
                         void* stream) {
    auto refuse = [&](const char* msg) { set_error("invalid argument: %s: %s", what, msg); return SAVSR_E_ARG; };
    if (!in || !out) return refuse("null pointer");
    if (n < 1 || n > 65535 || H < 1 || W < 1) return refuse("n in 1 .. 65535, H, W >= 1");
    if (!depth_ok(depth)) return refuse("depth is 8, 10 or 12");
    const int s = depth == 8 ? 1 : 2;
    const long long npx = (long long)H * W;
    if (out_frame_bytes < npx * s) return refuse("out_frame_bytes is smaller than the Y plane (H * W samples)");
    if (s == 2 && ((reinterpret_cast<uintptr_t>(out) & 1) || (out_frame_bytes & 1))) {
        set_error("alignment: %s: 16-bit samples need a 2-byte aligned frame pointer and an even out_frame_bytes", what);
        return SAVSR_E_ALIGN;
    }
    const int va = 4 * s;
    const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(out) % va) == 0 && out_frame_bytes % va == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0;
    const float mul = (float)(255 << (depth - 8));
    const dim3 grid(blocks_for((npx + 3) / 4), n);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const DitherDiv dv = dither_div(W);
#define SAVSR_QUANT_LUMA(S, V, D) \
    hipLaunchKernelGGL((quantize_luma_kernel<S, V, D>), grid, dim3(256), 0, st, in, npx, mul, out, (long long)out_frame_bytes, dv)
#define SAVSR_QUANT_LUMA_D(S, V) do { if (dither) SAVSR_QUANT_LUMA(S, V, true); else SAVSR_QUANT_LUMA(S, V, false); } while (0)
    if (s == 1) { if (vec) SAVSR_QUANT_LUMA_D(uint8_t, true); else SAVSR_QUANT_LUMA_D(uint8_t, false); }
    else { if (vec) SAVSR_QUANT_LUMA_D(uint16_t, true); else SAVSR_QUANT_LUMA_D(uint16_t, false); }
#undef SAVSR_QUANT_LUMA_D
#undef SAVSR_QUANT_LUMA
    return check_launch("quantize_luma_kernel");
}

extern "C" int savsr_video_quantize_luma(const float* in, int n, int H, int W, int depth, uint8_t* out, int64_t out_frame_bytes, void* stream) {
    return quantize_luma("video_quantize_luma", in, n, H, W, depth, false, out, out_frame_bytes, stream);
}

// dither 0: the kernels and the bytes of savsr_video_quantize_luma; 1: ordered dither (savsr_amd/dither.py).
extern "C" int savsr_video_quantize_luma_d(const float* in, int n, int H, int W, int depth, int dither, uint8_t* out, int64_t out_frame_bytes,
                                           void* stream) {
    if (dither != SAVSR_DITHER_NONE && dither != SAVSR_DITHER_ORDERED) {
        set_error("invalid argument: video_quantize_luma_d: dither %d (0 = none, 1 = ordered)", dither);
        return SAVSR_E_ARG;
    }
    return quantize_luma("video_quantize_luma_d", in, n, H, W, depth, dither == SAVSR_DITHER_ORDERED, out, out_frame_bytes, stream);
}

extern "C" int savsr_video_resample_chroma(const uint8_t* src, int n, int64_t src_frame_bytes, int64_t src_plane_offset, int ch, int cw, int depth_in,
                                           uint8_t* dst, int64_t dst_frame_bytes, int64_t dst_plane_offset, int cH, int cW, int depth_out,
                                           const int32_t* ymin, const int32_t* ysize, const float* wy, int taps_y, const int32_t* xmin,
                                           const int32_t* xsize, const float* wx, int taps_x, void* stream) {
    if (!src || !dst || !ymin || !ysize || !wy || !xmin || !xsize || !wx) return fail_arg("video_resample_chroma: null pointer");
    if (n < 1 || n > 65535 || ch < 1 || cw < 1 || cH < 1 || cW < 1) return fail_arg("video_resample_chroma: n in 1 .. 65535, ch, cw, cH, cW >= 1");
    if (!depth_ok(depth_in) || !depth_ok(depth_out)) return fail_arg("video_resample_chroma: depth_in and depth_out are 8, 10 or 12");
    if (taps_y < 1 || taps_x < 1 || taps_y > 65536 || taps_x > 65536) return fail_arg("video_resample_chroma: taps_y, taps_x in 1 .. 65536");
    if ((cH + TILE_H - 1) / TILE_H > 65535) return fail_arg("video_resample_chroma: cH beyond 65535 tiles of 16 rows");
    const int si = depth_in == 8 ? 1 : 2, so = depth_out == 8 ? 1 : 2;
    if (src_plane_offset < 0 || src_plane_offset + (long long)ch * cw * si > src_frame_bytes)
        return fail_arg("video_resample_chroma: the source plane (src_plane_offset, ch * cw samples) does not lie inside src_frame_bytes");
    if (dst_plane_offset < 0 || dst_plane_offset + (long long)cH * cW * so > dst_frame_bytes)
        return fail_arg("video_resample_chroma: the destination plane (dst_plane_offset, cH * cW samples) does not lie inside dst_frame_bytes");
    if (si == 2 && ((reinterpret_cast<uintptr_t>(src) & 1) || (src_frame_bytes & 1) || (src_plane_offset & 1)))
        return fail_align("video_resample_chroma: 16-bit source samples need a 2-byte aligned pointer, frame stride and plane offset");
    if (so == 2 && ((reinterpret_cast<uintptr_t>(dst) & 1) || (dst_frame_bytes & 1) || (dst_plane_offset & 1)))
        return fail_align("video_resample_chroma: 16-bit destination samples need a 2-byte aligned pointer, frame stride and plane offset");
    ResampleParams p;
    p.src = src + src_plane_offset; p.dst = dst + dst_plane_offset;
    p.src_frame_bytes = src_frame_bytes; p.dst_frame_bytes = dst_frame_bytes;
    p.ch = ch; p.cw = cw; p.cH = cH; p.cW = cW;
    p.ymin = ymin; p.ysize = ysize; p.wy = wy; p.taps_y = taps_y;
    p.xmin = xmin; p.xsize = xsize; p.wx = wx; p.taps_x = taps_x;
    p.top_in = (1u << depth_in) - 1u;
    p.scale = depth_out >= depth_in ? (float)(1 << (depth_out - depth_in)) : 1.0f / (float)(1 << (depth_in - depth_out));
    p.top_out = (float)((1 << depth_out) - 1);
    const int va = 4 * so;
    p.vec = cW % 4 == 0 && (reinterpret_cast<uintptr_t>(p.dst) % va) == 0 && dst_frame_bytes % va == 0;
    const dim3 grid((cW + TILE_W - 1) / TILE_W, (cH + TILE_H - 1) / TILE_H, n);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (si == 1 && so == 1) hipLaunchKernelGGL((resample_chroma_kernel<uint8_t, uint8_t>), grid, dim3(256), 0, st, p);
    else if (si == 1) hipLaunchKernelGGL((resample_chroma_kernel<uint8_t, uint16_t>), grid, dim3(256), 0, st, p);
    else if (so == 1) hipLaunchKernelGGL((resample_chroma_kernel<uint16_t, uint8_t>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((resample_chroma_kernel<uint16_t, uint16_t>), grid, dim3(256), 0, st, p);
    return check_launch("resample_chroma_kernel");
}
