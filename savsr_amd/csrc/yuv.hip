// Planar YUV 4:2:0 (I420) on either side of the network (ABI 35; the colour space as an argument: ABI 37): I420 frames -> the fp32 planar
// RGB clip batch the engine stages, and the fp32 result -> I420 frames for an encoder or a Y4M pipe.  The I420 counterparts of savsr_video_gather_u8 / _quantize_u8
// (video.hip); like them not fused into the SATU / tail kernels (satu.hip, tail.hip and common.hpp stay as they are, and with them
// savsr_source_hash_satu() and savsr_amd/hr_plans.json).
//
//   rgb2ycbcr / ycbcr2rgb   lbasicsr/utils/color_util.py:5-35, 71-97   ITU-R BT.601, limited range, Matlab's rounded constants
//
// That is colour space 0 (SAVSR_YUV_BT601) and what the entries without a colour argument run.  1 .. 3 are BT.709 limited, BT.601 full
// (JFIF) and BT.709 full, built from (Kr, Kb, range) by make_matrix; the arithmetic is the same for all four, and full range clips the
// rounded samples to 0 .. 255 (pure red / blue give a chroma of 255.5, which rounds to 256).
//
// savsr_amd/yuv.py restates both kernels in numpy and is what they are tested against, bit for bit: float32, a fixed operation order
// and no fused multiply-add (contraction is off for this whole file).
//
// I420 frame of an h x w picture: h * w Y bytes, ch * cw U bytes, ch * cw V bytes, ch = (h + 1) / 2, cw = (w + 1) / 2.
// ABI 38 adds 10 and 12 bits (16-bit samples), ABI 39 the 4:2:2 and 4:4:4 layouts at every depth (further down).
#include "common.hpp"

#include <cstdint>

#pragma clang fp contract(off)

namespace savsr {
namespace {

// A colour space's coefficient table (yuv.py: matrix).  to-RGB entries per 8-bit step with the result in [0, 1], offsets in 8-bit
// steps; to-YCbCr rows in 8-bit steps per unit of RGB.
struct YuvMatrix {
    double y, rv, gu, gv, bu, off_r, off_g, off_b;     // ycbcr2rgb
    float ky[3], kcb[3], kcr[3], oy, oc;               // rgb2ycbcr
    bool full;                                         // full range: the rounded samples are clipped to 0 .. 255
};
constexpr YuvMatrix kBt601 = {0.00456621, 0.00625893, -0.00153632, -0.00318811, 0.00791071, -222.921, 135.576, -276.836,
                              {65.481f, 128.553f, 24.966f}, {-37.797f, -74.203f, 112.0f}, {112.0f, -93.786f, -18.214f}, 16.0f, 128.0f, false};

// The table of luma weights (Kr, Kb) and a range (yuv.py: _build, the same float64 expressions in the same order; a constant expression
// is evaluated in IEEE double without contraction, as Python evaluates them).  Kg = 1 - Kr - Kb, Cb = (B - Y') / (2 (1 - Kb)),
// Cr = (R - Y') / (2 (1 - Kr)); Y = oy + sy Y', C = 128 + sc C' with (sy, oy, sc) = (219, 16, 224) limited, (255, 0, 255) full.
constexpr YuvMatrix make_matrix(double kr, double kb, bool full) {
    const double sy = full ? 255.0 : 219.0, oy = full ? 0.0 : 16.0, sc = full ? 255.0 : 224.0;
    const double kg = (1.0 - kr) - kb;
    const double db = 2.0 * (1.0 - kb), dr = 2.0 * (1.0 - kr);
    YuvMatrix m{};
    m.y = 1.0 / sy;
    m.rv = dr / sc;
    m.gu = -((db * kb) / (kg * sc));
    m.gv = -((dr * kr) / (kg * sc));
    m.bu = db / sc;
    const double base = -(oy * m.y);
    m.off_r = (base - 128.0 * m.rv) * 255.0;
    m.off_g = ((base - 128.0 * m.gu) - 128.0 * m.gv) * 255.0;
    m.off_b = (base - 128.0 * m.bu) * 255.0;
    m.ky[0] = static_cast<float>(sy * kr); m.ky[1] = static_cast<float>(sy * kg); m.ky[2] = static_cast<float>(sy * kb);
    m.kcb[0] = static_cast<float>(-((sc * kr) / db)); m.kcb[1] = static_cast<float>(-((sc * kg) / db)); m.kcb[2] = static_cast<float>(sc * 0.5);
    m.kcr[0] = static_cast<float>(sc * 0.5); m.kcr[1] = static_cast<float>(-((sc * kg) / dr)); m.kcr[2] = static_cast<float>(-((sc * kb) / dr));
    m.oy = static_cast<float>(oy);
    m.oc = 128.0f;
    m.full = full;
    return m;
}
// By colour id (savsr_hip.h: SAVSR_YUV_*; yuv.py: COLOURS).
enum { N_COLOURS = 4 };
struct YuvMatrices { YuvMatrix m[N_COLOURS]; };
constexpr YuvMatrices kYuv = {{kBt601, make_matrix(0.2126, 0.0722, false), make_matrix(0.299, 0.114, true), make_matrix(0.2126, 0.0722, true)}};

// Per-sample terms of ycbcr2rgb (yuv.py: to_rgb_tables): the float64 product, plus the channel's offset / 255 where it is folded in,
// rounded once to float32 -- a constant expression, so the compiler evaluates it in IEEE double exactly as numpy does.
//   R = y + rv      G = (y + gu) + gv      B = y + bu
enum { T_Y = 0, T_RV, T_GU, T_GV, T_BU, T_COUNT };
struct YuvTables { float v[T_COUNT][256]; };
constexpr YuvTables make_tables(const YuvMatrix& m) {
    YuvTables t{};
    for (int i = 0; i < 256; ++i) {
        t.v[T_Y][i] = static_cast<float>(i * m.y);
        t.v[T_RV][i] = static_cast<float>(i * m.rv + m.off_r / 255.0);
        t.v[T_GU][i] = static_cast<float>(i * m.gu + m.off_g / 255.0);
        t.v[T_GV][i] = static_cast<float>(i * m.gv);
        t.v[T_BU][i] = static_cast<float>(i * m.bu + m.off_b / 255.0);
    }
    return t;
}
struct YuvTablesAll { YuvTables c[N_COLOURS]; };
constexpr YuvTablesAll make_all_tables() {
    YuvTablesAll a{};
    for (int c = 0; c < N_COLOURS; ++c) a.c[c] = make_tables(kYuv.m[c]);
    return a;
}
constexpr YuvTablesAll kTablesValue = make_all_tables();
__constant__ YuvTablesAll kYuvToRgb = kTablesValue;              // 4 x 5 KiB

struct YuvIdx { int32_t f[SAVSR_VIDEO_MAX_SLOTS]; };     // slot -> frame, by value in the kernel arguments

inline unsigned blocks_for(long long units) { return (unsigned)((units + 255) / 256); }

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// One pixel of slot `o` (planes npx apart) from its three samples.
__device__ __forceinline__ void put_rgb(const float (*lut)[256], uint32_t y, uint32_t u, uint32_t v, float& r, float& g, float& b) {
    const float ty = lut[T_Y][y];
    r = clamp01(ty + lut[T_RV][v]);
    g = clamp01((ty + lut[T_GU][u]) + lut[T_GV][v]);
    b = clamp01(ty + lut[T_BU][u]);
}

// I420 frames [N][fb] -> fp32 planar RGB slots [n][3][h][w], slot k = frame idx.f[k].  A thread owns a block of 2 rows so that a chroma
// sample is read once.  VEC: 2 rows x 4 pixels -- a Y dword per row and 2 + 2 chroma bytes in, one float4 per plane row out (w % 4 == 0,
// 4-byte aligned frames, 16-byte aligned out: then every Y row is dword aligned and every chroma row 2-byte aligned); otherwise 2 x 2
// pixels with byte loads and scalar stores.  `colour` (0 .. N_COLOURS - 1, checked by the entry) picks the five tables staged in LDS.
template <bool VEC>
__global__ __launch_bounds__(256) void gather_i420_kernel(const uint8_t* __restrict__ src, int h, int w, long long fb, YuvIdx idx, int colour,
                                                          float* __restrict__ out) {
    __shared__ float lut[T_COUNT][256];
#pragma unroll
    for (int t = 0; t < T_COUNT; ++t) lut[t][threadIdx.x] = kYuvToRgb.c[colour].v[t][threadIdx.x];
    __syncthreads();
    const int k = blockIdx.y;
    const long long npx = (long long)h * w;
    const int ch = (h + 1) / 2, cw = (w + 1) / 2;
    const uint8_t* fy = src + (long long)idx.f[k] * fb;
    const uint8_t* fu = fy + npx;
    const uint8_t* fv = fu + (long long)ch * cw;
    float* o = out + (long long)k * 3 * npx;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        const int wq = w / 4;                                   // 4-pixel groups per row
        if (g >= (long long)ch * wq) return;
        const int cy = (int)(g / wq), x0 = (int)(g % wq) * 4;
        const long long coff = (long long)cy * cw + x0 / 2;
        const uint32_t uu = *reinterpret_cast<const uint16_t*>(fu + coff);
        const uint32_t vv = *reinterpret_cast<const uint16_t*>(fv + coff);
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int y = 2 * cy + dy;
            if (y >= h) break;
            const long long p = (long long)y * w + x0;
            const uint32_t yy = *reinterpret_cast<const uint32_t*>(fy + p);
            f32x4 r, gg, b;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pr, pg, pb;
                put_rgb(lut, (yy >> (8 * e)) & 255u, (uu >> (8 * (e >> 1))) & 255u, (vv >> (8 * (e >> 1))) & 255u, pr, pg, pb);
                r[e] = pr; gg[e] = pg; b[e] = pb;
            }
            *reinterpret_cast<f32x4*>(o + p) = r;
            *reinterpret_cast<f32x4*>(o + npx + p) = gg;
            *reinterpret_cast<f32x4*>(o + 2 * npx + p) = b;
        }
    } else {
        if (g >= (long long)ch * cw) return;
        const int cy = (int)(g / cw), cx = (int)(g % cw);
        const uint32_t u = fu[(long long)cy * cw + cx], v = fv[(long long)cy * cw + cx];
        for (int dy = 0; dy < 2 && 2 * cy + dy < h; ++dy) {
            for (int dx = 0; dx < 2 && 2 * cx + dx < w; ++dx) {
                const long long p = (long long)(2 * cy + dy) * w + 2 * cx + dx;
                float pr, pg, pb;
                put_rgb(lut, fy[p], u, v, pr, pg, pb);
                o[p] = pr; o[npx + p] = pg; o[2 * npx + p] = pb;
            }
        }
    }
}

// rgb2ycbcr's rows in 8-bit steps: every product and every sum rounded to float32 (yuv.py: _row).  Plain operators under this file's
// `fp contract(off)`: the header's __fmul_rn / __fadd_rn are compiled with contraction allowed and fuse again once inlined.
// CLIP (full range): the rounded value clipped to 0 .. 255 (yuv.py: rgb_to_i420); limited range stays inside 16 .. 240 by itself.
template <bool CLIP>
__device__ __forceinline__ uint32_t row3_u8(float k0, float k1, float k2, float off, float r, float g, float b) {
    const float v = rintf(((r * k0 + g * k1) + b * k2) + off);
    return (uint32_t)(CLIP ? fminf(fmaxf(v, 0.f), 255.f) : v);
}
// The rows of colour space C: the coefficients are constants of the instantiation (immediates in the code).
template <int C> __device__ __forceinline__ uint32_t luma_u8(float r, float g, float b) {
    constexpr YuvMatrix m = kYuv.m[C];
    return row3_u8<m.full>(m.ky[0], m.ky[1], m.ky[2], m.oy, r, g, b);
}
template <int C> __device__ __forceinline__ uint32_t cb_u8(float r, float g, float b) {
    constexpr YuvMatrix m = kYuv.m[C];
    return row3_u8<m.full>(m.kcb[0], m.kcb[1], m.kcb[2], m.oc, r, g, b);
}
template <int C> __device__ __forceinline__ uint32_t cr_u8(float r, float g, float b) {
    constexpr YuvMatrix m = kYuv.m[C];
    return row3_u8<m.full>(m.kcr[0], m.kcr[1], m.kcr[2], m.oc, r, g, b);
}

// fp32 planar RGB [n][3][H][W] -> I420 frames [n][fb]: clamp(0, 1); Y per pixel; Cb / Cr from the mean RGB of the block's in-image
// pixels -- ((a + b) + (c + d)) * 0.25 with a b the upper row, (a + b) * 0.5 for a pair, the pixel alone (yuv.py: _block_mean); rintf
// (round half to even).  VEC: a thread owns 2 rows x 4 pixels -- one float4 per plane row in (nontemporal: the result is read once), a Y
// dword per row and 2 + 2 chroma bytes out (W % 4 == 0, 16-byte aligned in, 4-byte aligned out); otherwise 2 x 2 pixels, scalar.
// C: the colour space, a template argument so that its rows stay immediates.
template <bool VEC, int C>
__global__ __launch_bounds__(256) void quantize_i420_kernel(const float* __restrict__ in, int H, int W, long long fb, uint8_t* __restrict__ out) {
    const int k = blockIdx.y;
    const long long npx = (long long)H * W;
    const int ch = (H + 1) / 2, cw = (W + 1) / 2;
    const float* src = in + (long long)k * 3 * npx;
    uint8_t* fy = out + (long long)k * fb;
    uint8_t* fu = fy + npx;
    uint8_t* fv = fu + (long long)ch * cw;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        const int wq = W / 4;
        if (g >= (long long)ch * wq) return;
        const int cy = (int)(g / wq), x0 = (int)(g % wq) * 4;
        const bool two = 2 * cy + 1 < H;
        f32x4 px[2][3];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            if (dy == 1 && !two) break;
            const long long p = (long long)(2 * cy + dy) * W + x0;
            uint32_t yy = 0u;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const f32x4 x = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + c * npx + p));
#pragma unroll
                for (int e = 0; e < 4; ++e) px[dy][c][e] = clamp01(x[e]);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) yy |= luma_u8<C>(px[dy][0][e], px[dy][1][e], px[dy][2][e]) << (8 * e);
            *reinterpret_cast<uint32_t*>(fy + p) = yy;
        }
        uint32_t uu = 0u, vv = 0u;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float m[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float top = px[0][c][2 * j] + px[0][c][2 * j + 1];
                m[c] = two ? (top + (px[1][c][2 * j] + px[1][c][2 * j + 1])) * 0.25f : top * 0.5f;
            }
            uu |= cb_u8<C>(m[0], m[1], m[2]) << (8 * j);
            vv |= cr_u8<C>(m[0], m[1], m[2]) << (8 * j);
        }
        const long long coff = (long long)cy * cw + x0 / 2;
        *reinterpret_cast<uint16_t*>(fu + coff) = (uint16_t)uu;
        *reinterpret_cast<uint16_t*>(fv + coff) = (uint16_t)vv;
    } else {
        if (g >= (long long)ch * cw) return;
        const int cy = (int)(g / cw), cx = (int)(g % cw);
        const bool two_y = 2 * cy + 1 < H, two_x = 2 * cx + 1 < W;
        float q[2][2][3];
        for (int dy = 0; dy < 2; ++dy) {
            for (int dx = 0; dx < 2; ++dx) {
                if ((dy && !two_y) || (dx && !two_x)) continue;
                const long long p = (long long)(2 * cy + dy) * W + 2 * cx + dx;
#pragma unroll
                for (int c = 0; c < 3; ++c) q[dy][dx][c] = clamp01(src[c * npx + p]);
                fy[p] = (uint8_t)luma_u8<C>(q[dy][dx][0], q[dy][dx][1], q[dy][dx][2]);
            }
        }
        float m[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (two_x && two_y) m[c] = ((q[0][0][c] + q[0][1][c]) + (q[1][0][c] + q[1][1][c])) * 0.25f;
            else if (two_x) m[c] = (q[0][0][c] + q[0][1][c]) * 0.5f;
            else if (two_y) m[c] = (q[0][0][c] + q[1][0][c]) * 0.5f;
            else m[c] = q[0][0][c];
        }
        fu[(long long)cy * cw + cx] = (uint8_t)cb_u8<C>(m[0], m[1], m[2]);
        fv[(long long)cy * cw + cx] = (uint8_t)cr_u8<C>(m[0], m[1], m[2]);
    }
}

int load_idx(const int32_t* idx, int n, int n_frames, YuvIdx* gi, const char* what) {
    if (!idx) { set_error("%s: null index list", what); return SAVSR_E_ARG; }
    if (n < 1 || n > SAVSR_VIDEO_MAX_SLOTS) { set_error("%s: %d slots (1 .. %d)", what, n, SAVSR_VIDEO_MAX_SLOTS); return SAVSR_E_ARG; }
    for (int i = 0; i < n; ++i) {
        if (idx[i] < 0 || idx[i] >= n_frames) { set_error("%s: slot %d names frame %d of %d", what, i, idx[i], n_frames); return SAVSR_E_ARG; }
        gi->f[i] = idx[i];
    }
    return 0;
}

inline long long i420_bytes(int h, int w) { return (long long)h * w + 2LL * ((h + 1) / 2) * ((w + 1) / 2); }

int check_colour(int colour, const char* what) {
    if (colour < 0 || colour >= N_COLOURS) { set_error("invalid argument: %s: colour %d (0 .. %d)", what, colour, N_COLOURS - 1); return SAVSR_E_ARG; }
    return 0;
}

int fail(const char* what, const char* msg) {
    set_error("invalid argument: %s: %s", what, msg);
    return SAVSR_E_ARG;
}

// The two entries of either kernel: `what` names the one called in its messages.
int gather_yuv420(const char* what, const uint8_t* frames, int n_frames, int h, int w, const int32_t* idx, int n_idx, int colour, float* out,
                  void* stream) {
    if (!frames || !out) return fail(what, "null pointer");
    if (h < 1 || w < 1 || n_frames < 1) return fail(what, "h, w, n_frames >= 1");
    if (int rc = check_colour(colour, what)) return rc;
    YuvIdx gi;
    if (int rc = load_idx(idx, n_idx, n_frames, &gi, what)) return rc;
    const bool vec = w % 4 == 0 && (reinterpret_cast<uintptr_t>(frames) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const long long units = (long long)((h + 1) / 2) * (vec ? w / 4 : (w + 1) / 2);
    const dim3 grid(blocks_for(units), n_idx);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL((gather_i420_kernel<true>), grid, dim3(256), 0, st, frames, h, w, i420_bytes(h, w), gi, colour, out);
    else hipLaunchKernelGGL((gather_i420_kernel<false>), grid, dim3(256), 0, st, frames, h, w, i420_bytes(h, w), gi, colour, out);
    return check_launch("gather_i420_kernel");
}

template <int C>
void launch_quantize(bool vec, dim3 grid, hipStream_t st, const float* in, int H, int W, uint8_t* out) {
    if (vec) hipLaunchKernelGGL((quantize_i420_kernel<true, C>), grid, dim3(256), 0, st, in, H, W, i420_bytes(H, W), out);
    else hipLaunchKernelGGL((quantize_i420_kernel<false, C>), grid, dim3(256), 0, st, in, H, W, i420_bytes(H, W), out);
}

int quantize_yuv420(const char* what, const float* in, int n, int H, int W, int colour, uint8_t* out, void* stream) {
    if (!in || !out) return fail(what, "null pointer");
    if (n < 1 || n > 65535 || H < 1 || W < 1) return fail(what, "n in 1 .. 65535, H, W >= 1");
    if (int rc = check_colour(colour, what)) return rc;
    const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
    const long long units = (long long)((H + 1) / 2) * (vec ? W / 4 : (W + 1) / 2);
    const dim3 grid(blocks_for(units), n);
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (colour) {
        case 0: launch_quantize<0>(vec, grid, st, in, H, W, out); break;
        case 1: launch_quantize<1>(vec, grid, st, in, H, W, out); break;
        case 2: launch_quantize<2>(vec, grid, st, in, H, W, out); break;
        default: launch_quantize<3>(vec, grid, st, in, H, W, out); break;
    }
    return check_launch("quantize_i420_kernel");
}


// ---- 10 and 12 bits (ABI 38) -----------------------------------------------------------------------------------------------------------
// A frame is the 8-bit frame's planes with every sample a little-endian 16-bit word (Y4M's C420p10 / C420p12): fb = 2 * i420_bytes.  Limited
// range only (colour spaces 0 and 1): a sample is the 8-bit one times k = 2^(d - 8), so the constants are the 8-bit ones scaled by a power
// of two.  yuv.py's "High depth" is the specification, bit for bit.  No LDS tables: the input is arithmetic, not a lookup.
enum { N_COLOURS_16 = 2, N_DEPTHS_16 = 2 };      // colour spaces 0, 1; depths 10, 12

// to_rgb_coefficients: c = float32(coef / k), o = float32(offset / 255) -- constant expressions, evaluated in IEEE double as numpy does.
struct ToRgb16 { float y, rv, gu, gv, bu, o_r, o_g, o_b; };
constexpr ToRgb16 make_to_rgb16(const YuvMatrix& m, double k) {
    return ToRgb16{static_cast<float>(m.y / k), static_cast<float>(m.rv / k), static_cast<float>(m.gu / k), static_cast<float>(m.gv / k),
                   static_cast<float>(m.bu / k), static_cast<float>(m.off_r / 255.0), static_cast<float>(m.off_g / 255.0),
                   static_cast<float>(m.off_b / 255.0)};
}
struct ToRgb16All { ToRgb16 c[N_COLOURS_16][N_DEPTHS_16]; };
__constant__ ToRgb16All kToRgb16 = {{{make_to_rgb16(kYuv.m[0], 4.0), make_to_rgb16(kYuv.m[0], 16.0)},
                                     {make_to_rgb16(kYuv.m[1], 4.0), make_to_rgb16(kYuv.m[1], 16.0)}}};

// One pixel from its three samples (already limited to 2^d - 1):  Yt = y c_y,  R = (Yt + v c_rv) + o_R,  G = ((Yt + u c_gu) + v c_gv) + o_G,
// B = (Yt + u c_bu) + o_B, every product and sum rounded to float32 (contraction is off).
__device__ __forceinline__ void put_rgb16(const ToRgb16& c, uint32_t y, uint32_t u, uint32_t v, float& r, float& g, float& b) {
    const float fy = (float)y, fu = (float)u, fv = (float)v;
    const float yt = fy * c.y;
    r = clamp01((yt + fv * c.rv) + c.o_r);
    g = clamp01(((yt + fu * c.gu) + fv * c.gv) + c.o_g);
    b = clamp01((yt + fu * c.bu) + c.o_b);
}

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// High-depth frames [N][fb] -> fp32 planar RGB slots [n][3][h][w], slot k = frame idx.f[k]; a sample above top = 2^d - 1 reads as top.  A
// thread owns 2 rows so that a chroma sample is read once.  VEC: 2 rows x 4 pixels -- 8 bytes of Y per row and 4 + 4 chroma bytes in, one
// float4 per plane row out (w % 4 == 0, 8-byte aligned frames, 16-byte aligned out: then fb, every Y row and the chroma planes' rows keep
// that alignment); otherwise 2 x 2 pixels with 16-bit loads and scalar stores (any 2-byte aligned frames).  ci, di: the row of kToRgb16.
template <bool VEC>
__global__ __launch_bounds__(256) void gather_i420_16_kernel(const uint8_t* __restrict__ src, int h, int w, long long fb, YuvIdx idx, int ci, int di,
                                                             uint32_t top, float* __restrict__ out) {
    const ToRgb16 c = kToRgb16.c[ci][di];
    const int k = blockIdx.y;
    const long long npx = (long long)h * w;
    const int ch = (h + 1) / 2, cw = (w + 1) / 2;
    const uint16_t* fy = reinterpret_cast<const uint16_t*>(src + (long long)idx.f[k] * fb);
    const uint16_t* fu = fy + npx;
    const uint16_t* fv = fu + (long long)ch * cw;
    float* o = out + (long long)k * 3 * npx;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        const int wq = w / 4;
        if (g >= (long long)ch * wq) return;
        const int cy = (int)(g / wq), x0 = (int)(g % wq) * 4;
        const long long coff = (long long)cy * cw + x0 / 2;
        const uint32_t uu = *reinterpret_cast<const uint32_t*>(fu + coff);
        const uint32_t vv = *reinterpret_cast<const uint32_t*>(fv + coff);
        uint32_t us[2], vs[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            us[j] = min((uu >> (16 * j)) & 0xffffu, top);
            vs[j] = min((vv >> (16 * j)) & 0xffffu, top);
        }
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int y = 2 * cy + dy;
            if (y >= h) break;
            const long long p = (long long)y * w + x0;
            const u32x2 yy = *reinterpret_cast<const u32x2*>(fy + p);
            f32x4 r, gg, b;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pr, pg, pb;
                put_rgb16(c, min((yy[e >> 1] >> (16 * (e & 1))) & 0xffffu, top), us[e >> 1], vs[e >> 1], pr, pg, pb);
                r[e] = pr; gg[e] = pg; b[e] = pb;
            }
            *reinterpret_cast<f32x4*>(o + p) = r;
            *reinterpret_cast<f32x4*>(o + npx + p) = gg;
            *reinterpret_cast<f32x4*>(o + 2 * npx + p) = b;
        }
    } else {
        if (g >= (long long)ch * cw) return;
        const int cy = (int)(g / cw), cx = (int)(g % cw);
        const uint32_t u = min((uint32_t)fu[(long long)cy * cw + cx], top), v = min((uint32_t)fv[(long long)cy * cw + cx], top);
        for (int dy = 0; dy < 2 && 2 * cy + dy < h; ++dy) {
            for (int dx = 0; dx < 2 && 2 * cx + dx < w; ++dx) {
                const long long p = (long long)(2 * cy + dy) * w + 2 * cx + dx;
                float pr, pg, pb;
                put_rgb16(c, min((uint32_t)fy[p], top), u, v, pr, pg, pb);
                o[p] = pr; o[npx + p] = pg; o[2 * npx + p] = pb;
            }
        }
    }
}

// rint(row * k): the 8-bit row's float32 value (yuv.py: _row) times k = 2^(d - 8), exact, then half to even.  Limited range stays inside
// 16 k .. 240 k by itself: no clip.
__device__ __forceinline__ uint32_t row3_u16(const float (&kk)[3], float off, float k, float r, float g, float b) {
    return (uint32_t)rintf((((r * kk[0] + g * kk[1]) + b * kk[2]) + off) * k);
}

// fp32 planar RGB [n][3][H][W] -> high-depth frames [n][fb], quantize_i420_kernel's arithmetic with the rows scaled by k before the rounding.
// VEC: a thread owns 2 rows x 4 pixels -- one float4 per plane row in (nontemporal: the result is read once), 8 bytes of Y per row and
// 4 + 4 chroma bytes out (W % 4 == 0, 16-byte aligned in, 8-byte aligned out); otherwise 2 x 2 pixels with 16-bit stores.  C: the colour
// space (0 or 1), a template argument so that its rows stay immediates.
template <bool VEC, int C>
__global__ __launch_bounds__(256) void quantize_i420_16_kernel(const float* __restrict__ in, int H, int W, long long fb, float k,
                                                               uint8_t* __restrict__ out) {
    constexpr YuvMatrix m = kYuv.m[C];
    static_assert(!m.full, "high depth is defined for limited range only");
    const int f = blockIdx.y;
    const long long npx = (long long)H * W;
    const int ch = (H + 1) / 2, cw = (W + 1) / 2;
    const float* src = in + (long long)f * 3 * npx;
    uint16_t* fy = reinterpret_cast<uint16_t*>(out + (long long)f * fb);
    uint16_t* fu = fy + npx;
    uint16_t* fv = fu + (long long)ch * cw;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        const int wq = W / 4;
        if (g >= (long long)ch * wq) return;
        const int cy = (int)(g / wq), x0 = (int)(g % wq) * 4;
        const bool two = 2 * cy + 1 < H;
        f32x4 px[2][3];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            if (dy == 1 && !two) break;
            const long long p = (long long)(2 * cy + dy) * W + x0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const f32x4 x = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + c * npx + p));
#pragma unroll
                for (int e = 0; e < 4; ++e) px[dy][c][e] = clamp01(x[e]);
            }
            u32x2 yy = {0u, 0u};
#pragma unroll
            for (int e = 0; e < 4; ++e) yy[e >> 1] |= row3_u16(m.ky, m.oy, k, px[dy][0][e], px[dy][1][e], px[dy][2][e]) << (16 * (e & 1));
            *reinterpret_cast<u32x2*>(fy + p) = yy;
        }
        uint32_t uu = 0u, vv = 0u;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float mean[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float top = px[0][c][2 * j] + px[0][c][2 * j + 1];
                mean[c] = two ? (top + (px[1][c][2 * j] + px[1][c][2 * j + 1])) * 0.25f : top * 0.5f;
            }
            uu |= row3_u16(m.kcb, m.oc, k, mean[0], mean[1], mean[2]) << (16 * j);
            vv |= row3_u16(m.kcr, m.oc, k, mean[0], mean[1], mean[2]) << (16 * j);
        }
        const long long coff = (long long)cy * cw + x0 / 2;
        *reinterpret_cast<uint32_t*>(fu + coff) = uu;
        *reinterpret_cast<uint32_t*>(fv + coff) = vv;
    } else {
        if (g >= (long long)ch * cw) return;
        const int cy = (int)(g / cw), cx = (int)(g % cw);
        const bool two_y = 2 * cy + 1 < H, two_x = 2 * cx + 1 < W;
        float q[2][2][3];
        for (int dy = 0; dy < 2; ++dy) {
            for (int dx = 0; dx < 2; ++dx) {
                if ((dy && !two_y) || (dx && !two_x)) continue;
                const long long p = (long long)(2 * cy + dy) * W + 2 * cx + dx;
#pragma unroll
                for (int c = 0; c < 3; ++c) q[dy][dx][c] = clamp01(src[c * npx + p]);
                fy[p] = (uint16_t)row3_u16(m.ky, m.oy, k, q[dy][dx][0], q[dy][dx][1], q[dy][dx][2]);
            }
        }
        float mean[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (two_x && two_y) mean[c] = ((q[0][0][c] + q[0][1][c]) + (q[1][0][c] + q[1][1][c])) * 0.25f;
            else if (two_x) mean[c] = (q[0][0][c] + q[0][1][c]) * 0.5f;
            else if (two_y) mean[c] = (q[0][0][c] + q[1][0][c]) * 0.5f;
            else mean[c] = q[0][0][c];
        }
        fu[(long long)cy * cw + cx] = (uint16_t)row3_u16(m.kcb, m.oc, k, mean[0], mean[1], mean[2]);
        fv[(long long)cy * cw + cx] = (uint16_t)row3_u16(m.kcr, m.oc, k, mean[0], mean[1], mean[2]);
    }
}

// depth 10 / 12 and a limited-range colour space, or the refusal that names the rule
int check_depth16(int colour, int depth, const char* what) {
    if (depth != 10 && depth != 12) { set_error("invalid argument: %s: depth %d (10 or 12; 8 bits: the entries without _16)", what, depth); return SAVSR_E_ARG; }
    if (colour < 0 || colour >= N_COLOURS_16) {
        set_error("invalid argument: %s: colour %d (0 .. %d: 10 and 12 bits are defined for limited range only)", what, colour, N_COLOURS_16 - 1);
        return SAVSR_E_ARG;
    }
    return 0;
}


// ---- 4:2:2 and 4:4:4 (ABI 39) -----------------------------------------------------------------------------------------------------------
// The same arithmetic with another block shape (yuv.py: "Chroma layouts"): a frame is h * w Y samples, then ch * cw U, then ch * cw V with
// (ch, cw) = (h, (w + 1) / 2) in 4:2:2 and (h, w) in 4:4:4.  SX is the layout's horizontal subsampling (2: 4:2:2, 1: 4:4:4); neither layout
// shares chroma between rows, so a thread owns pixels of one row only.  VEC: 4 pixels -- a Y dword (8 bits) or 8 bytes (16 bits), the
// 4 / SX chroma samples under them in one access per plane, one float4 per plane row.  Otherwise one chroma sample and its SX pixels
// with sample-sized accesses.  What VEC needs is 4:2:0's: w % 4 == 0, frames 4-byte (8 bits) / 8-byte (16 bits) aligned, the fp32 side
// 16-byte aligned.  With w = 4 q, in bytes from the frame's start (s = bytes per sample):
//   4:4:4   fb = 12 q h s; U at 4 q h s, V at 8 q h s; every row of every plane is 4 q s long       -> every 4-pixel group 4 s-aligned
//   4:2:2   fb = 8 q h s;  U at 4 q h s, V at 6 q h s; a chroma row is 2 q s long, a group's pair
//           of chroma samples lies 2 s (x0 / 4) into it                                              -> every chroma pair 2 s-aligned
// so the Y access (4 s bytes) and the 4:4:4 chroma access (4 s bytes) are naturally aligned, and the 4:2:2 chroma access (2 s bytes) is too.
template <int SX> __device__ __forceinline__ int chroma_w(int w) { return SX == 2 ? (w + 1) / 2 : w; }
inline long long yuvp_bytes(int h, int w, int sx) { return (long long)h * w + 2LL * h * (sx == 2 ? (w + 1) / 2 : w); }

template <int SX, bool VEC>
__global__ __launch_bounds__(256) void gather_yuvp_kernel(const uint8_t* __restrict__ src, int h, int w, long long fb, YuvIdx idx, int colour,
                                                          float* __restrict__ out) {
    __shared__ float lut[T_COUNT][256];
#pragma unroll
    for (int t = 0; t < T_COUNT; ++t) lut[t][threadIdx.x] = kYuvToRgb.c[colour].v[t][threadIdx.x];
    __syncthreads();
    const int k = blockIdx.y;
    const long long npx = (long long)h * w;
    const int cw = chroma_w<SX>(w);
    const uint8_t* fy = src + (long long)idx.f[k] * fb;
    const uint8_t* fu = fy + npx;
    const uint8_t* fv = fu + (long long)h * cw;
    float* o = out + (long long)k * 3 * npx;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        const int wq = w / 4;
        if (g >= (long long)h * wq) return;
        const int y = (int)(g / wq), x0 = (int)(g % wq) * 4;
        const long long p = (long long)y * w + x0;
        const long long coff = (long long)y * cw + x0 / SX;
        uint32_t uu, vv;
        if (SX == 2) {
            uu = *reinterpret_cast<const uint16_t*>(fu + coff);
            vv = *reinterpret_cast<const uint16_t*>(fv + coff);
        } else {
            uu = *reinterpret_cast<const uint32_t*>(fu + coff);
            vv = *reinterpret_cast<const uint32_t*>(fv + coff);
        }
        const uint32_t yy = *reinterpret_cast<const uint32_t*>(fy + p);
        f32x4 r, gg, b;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pr, pg, pb;
            put_rgb(lut, (yy >> (8 * e)) & 255u, (uu >> (8 * (e / SX))) & 255u, (vv >> (8 * (e / SX))) & 255u, pr, pg, pb);
            r[e] = pr; gg[e] = pg; b[e] = pb;
        }
        *reinterpret_cast<f32x4*>(o + p) = r;
        *reinterpret_cast<f32x4*>(o + npx + p) = gg;
        *reinterpret_cast<f32x4*>(o + 2 * npx + p) = b;
    } else {
        if (g >= (long long)h * cw) return;
        const int cy = (int)(g / cw), cx = (int)(g % cw);
        const uint32_t u = fu[(long long)cy * cw + cx], v = fv[(long long)cy * cw + cx];
        for (int dx = 0; dx < SX && SX * cx + dx < w; ++dx) {
            const long long p = (long long)cy * w + SX * cx + dx;
            float pr, pg, pb;
            put_rgb(lut, fy[p], u, v, pr, pg, pb);
            o[p] = pr; o[npx + p] = pg; o[2 * npx + p] = pb;
        }
    }
}

// fp32 planar RGB [n][3][H][W] -> 4:2:2 / 4:4:4 frames [n][fb]: quantize_i420_kernel's arithmetic; Cb / Cr from (a + b) * 0.5 of a 4:2:2
// pair, the pixel alone in the last column of an odd W, the pixel's own clamped RGB in 4:4:4.  C: the colour space, a template argument.
template <int SX, bool VEC, int C>
__global__ __launch_bounds__(256) void quantize_yuvp_kernel(const float* __restrict__ in, int H, int W, long long fb, uint8_t* __restrict__ out) {
    const int k = blockIdx.y;
    const long long npx = (long long)H * W;
    const int cw = chroma_w<SX>(W);
    const float* src = in + (long long)k * 3 * npx;
    uint8_t* fy = out + (long long)k * fb;
    uint8_t* fu = fy + npx;
    uint8_t* fv = fu + (long long)H * cw;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        const int wq = W / 4;
        if (g >= (long long)H * wq) return;
        const int y = (int)(g / wq), x0 = (int)(g % wq) * 4;
        const long long p = (long long)y * W + x0;
        f32x4 px[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const f32x4 x = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + c * npx + p));
#pragma unroll
            for (int e = 0; e < 4; ++e) px[c][e] = clamp01(x[e]);
        }
        uint32_t yy = 0u, uu = 0u, vv = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) yy |= luma_u8<C>(px[0][e], px[1][e], px[2][e]) << (8 * e);
        *reinterpret_cast<uint32_t*>(fy + p) = yy;
#pragma unroll
        for (int j = 0; j < 4 / SX; ++j) {
            float m[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) m[c] = SX == 2 ? (px[c][2 * j] + px[c][2 * j + 1]) * 0.5f : px[c][j];
            uu |= cb_u8<C>(m[0], m[1], m[2]) << (8 * j);
            vv |= cr_u8<C>(m[0], m[1], m[2]) << (8 * j);
        }
        const long long coff = (long long)y * cw + x0 / SX;
        if (SX == 2) {
            *reinterpret_cast<uint16_t*>(fu + coff) = (uint16_t)uu;
            *reinterpret_cast<uint16_t*>(fv + coff) = (uint16_t)vv;
        } else {
            *reinterpret_cast<uint32_t*>(fu + coff) = uu;
            *reinterpret_cast<uint32_t*>(fv + coff) = vv;
        }
    } else {
        if (g >= (long long)H * cw) return;
        const int cy = (int)(g / cw), cx = (int)(g % cw);
        const bool two = SX == 2 && 2 * cx + 1 < W;
        float q[2][3];
        for (int dx = 0; dx < (two ? 2 : 1); ++dx) {
            const long long p = (long long)cy * W + SX * cx + dx;
#pragma unroll
            for (int c = 0; c < 3; ++c) q[dx][c] = clamp01(src[c * npx + p]);
            fy[p] = (uint8_t)luma_u8<C>(q[dx][0], q[dx][1], q[dx][2]);
        }
        float m[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = two ? (q[0][c] + q[1][c]) * 0.5f : q[0][c];
        fu[(long long)cy * cw + cx] = (uint8_t)cb_u8<C>(m[0], m[1], m[2]);
        fv[(long long)cy * cw + cx] = (uint8_t)cr_u8<C>(m[0], m[1], m[2]);
    }
}

// The 10- / 12-bit forms: gather_i420_16_kernel's / quantize_i420_16_kernel's arithmetic on the blocks above.  VEC: 8 bytes of Y and
// 4 (4:2:2) or 8 (4:4:4) bytes per chroma plane.
template <int SX, bool VEC>
__global__ __launch_bounds__(256) void gather_yuvp_16_kernel(const uint8_t* __restrict__ src, int h, int w, long long fb, YuvIdx idx, int ci, int di,
                                                             uint32_t top, float* __restrict__ out) {
    const ToRgb16 c = kToRgb16.c[ci][di];
    const int k = blockIdx.y;
    const long long npx = (long long)h * w;
    const int cw = chroma_w<SX>(w);
    const uint16_t* fy = reinterpret_cast<const uint16_t*>(src + (long long)idx.f[k] * fb);
    const uint16_t* fu = fy + npx;
    const uint16_t* fv = fu + (long long)h * cw;
    float* o = out + (long long)k * 3 * npx;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        const int wq = w / 4;
        if (g >= (long long)h * wq) return;
        const int y = (int)(g / wq), x0 = (int)(g % wq) * 4;
        const long long p = (long long)y * w + x0;
        const long long coff = (long long)y * cw + x0 / SX;
        u32x2 uu = {0u, 0u}, vv = {0u, 0u};
        if (SX == 2) {
            uu[0] = *reinterpret_cast<const uint32_t*>(fu + coff);
            vv[0] = *reinterpret_cast<const uint32_t*>(fv + coff);
        } else {
            uu = *reinterpret_cast<const u32x2*>(fu + coff);
            vv = *reinterpret_cast<const u32x2*>(fv + coff);
        }
        const u32x2 yy = *reinterpret_cast<const u32x2*>(fy + p);
        f32x4 r, gg, b;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = e / SX;                                   // the chroma sample over pixel e
            float pr, pg, pb;
            put_rgb16(c, min((yy[e >> 1] >> (16 * (e & 1))) & 0xffffu, top), min((uu[j >> 1] >> (16 * (j & 1))) & 0xffffu, top),
                      min((vv[j >> 1] >> (16 * (j & 1))) & 0xffffu, top), pr, pg, pb);
            r[e] = pr; gg[e] = pg; b[e] = pb;
        }
        *reinterpret_cast<f32x4*>(o + p) = r;
        *reinterpret_cast<f32x4*>(o + npx + p) = gg;
        *reinterpret_cast<f32x4*>(o + 2 * npx + p) = b;
    } else {
        if (g >= (long long)h * cw) return;
        const int cy = (int)(g / cw), cx = (int)(g % cw);
        const uint32_t u = min((uint32_t)fu[(long long)cy * cw + cx], top), v = min((uint32_t)fv[(long long)cy * cw + cx], top);
        for (int dx = 0; dx < SX && SX * cx + dx < w; ++dx) {
            const long long p = (long long)cy * w + SX * cx + dx;
            float pr, pg, pb;
            put_rgb16(c, min((uint32_t)fy[p], top), u, v, pr, pg, pb);
            o[p] = pr; o[npx + p] = pg; o[2 * npx + p] = pb;
        }
    }
}

template <int SX, bool VEC, int C>
__global__ __launch_bounds__(256) void quantize_yuvp_16_kernel(const float* __restrict__ in, int H, int W, long long fb, float k,
                                                               uint8_t* __restrict__ out) {
    constexpr YuvMatrix m = kYuv.m[C];
    static_assert(!m.full, "high depth is defined for limited range only");
    const int f = blockIdx.y;
    const long long npx = (long long)H * W;
    const int cw = chroma_w<SX>(W);
    const float* src = in + (long long)f * 3 * npx;
    uint16_t* fy = reinterpret_cast<uint16_t*>(out + (long long)f * fb);
    uint16_t* fu = fy + npx;
    uint16_t* fv = fu + (long long)H * cw;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        const int wq = W / 4;
        if (g >= (long long)H * wq) return;
        const int y = (int)(g / wq), x0 = (int)(g % wq) * 4;
        const long long p = (long long)y * W + x0;
        f32x4 px[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const f32x4 x = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + c * npx + p));
#pragma unroll
            for (int e = 0; e < 4; ++e) px[c][e] = clamp01(x[e]);
        }
        u32x2 yy = {0u, 0u}, uu = {0u, 0u}, vv = {0u, 0u};
#pragma unroll
        for (int e = 0; e < 4; ++e) yy[e >> 1] |= row3_u16(m.ky, m.oy, k, px[0][e], px[1][e], px[2][e]) << (16 * (e & 1));
        *reinterpret_cast<u32x2*>(fy + p) = yy;
#pragma unroll
        for (int j = 0; j < 4 / SX; ++j) {
            float mean[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) mean[c] = SX == 2 ? (px[c][2 * j] + px[c][2 * j + 1]) * 0.5f : px[c][j];
            uu[j >> 1] |= row3_u16(m.kcb, m.oc, k, mean[0], mean[1], mean[2]) << (16 * (j & 1));
            vv[j >> 1] |= row3_u16(m.kcr, m.oc, k, mean[0], mean[1], mean[2]) << (16 * (j & 1));
        }
        const long long coff = (long long)y * cw + x0 / SX;
        if (SX == 2) {
            *reinterpret_cast<uint32_t*>(fu + coff) = uu[0];
            *reinterpret_cast<uint32_t*>(fv + coff) = vv[0];
        } else {
            *reinterpret_cast<u32x2*>(fu + coff) = uu;
            *reinterpret_cast<u32x2*>(fv + coff) = vv;
        }
    } else {
        if (g >= (long long)H * cw) return;
        const int cy = (int)(g / cw), cx = (int)(g % cw);
        const bool two = SX == 2 && 2 * cx + 1 < W;
        float q[2][3];
        for (int dx = 0; dx < (two ? 2 : 1); ++dx) {
            const long long p = (long long)cy * W + SX * cx + dx;
#pragma unroll
            for (int c = 0; c < 3; ++c) q[dx][c] = clamp01(src[c * npx + p]);
            fy[p] = (uint16_t)row3_u16(m.ky, m.oy, k, q[dx][0], q[dx][1], q[dx][2]);
        }
        float mean[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) mean[c] = two ? (q[0][c] + q[1][c]) * 0.5f : q[0][c];
        fu[(long long)cy * cw + cx] = (uint16_t)row3_u16(m.kcb, m.oc, k, mean[0], mean[1], mean[2]);
        fv[(long long)cy * cw + cx] = (uint16_t)row3_u16(m.kcr, m.oc, k, mean[0], mean[1], mean[2]);
    }
}

// The high-depth entries' bodies: `what` names the entry called in its messages.
int gather_yuv420_16(const char* what, const uint8_t* frames, int n_frames, int h, int w, const int32_t* idx, int n_idx, int colour, int depth,
                     float* out, void* stream) {
    if (!frames || !out) return fail(what, "null pointer");
    if (h < 1 || w < 1 || n_frames < 1) return fail(what, "h, w, n_frames >= 1");
    if (int rc = check_depth16(colour, depth, what)) return rc;
    if (reinterpret_cast<uintptr_t>(frames) & 1) return fail(what, "frames must be 2-byte aligned (16-bit samples)");
    if (reinterpret_cast<uintptr_t>(out) & 3) return fail(what, "out must be 4-byte aligned");
    YuvIdx gi;
    if (int rc = load_idx(idx, n_idx, n_frames, &gi, what)) return rc;
    const bool vec = w % 4 == 0 && (reinterpret_cast<uintptr_t>(frames) & 7) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const long long units = (long long)((h + 1) / 2) * (vec ? w / 4 : (w + 1) / 2);
    const dim3 grid(blocks_for(units), n_idx);
    const long long fb = 2 * i420_bytes(h, w);
    const int di = depth == 10 ? 0 : 1;
    const uint32_t top = (1u << depth) - 1u;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL((gather_i420_16_kernel<true>), grid, dim3(256), 0, st, frames, h, w, fb, gi, colour, di, top, out);
    else hipLaunchKernelGGL((gather_i420_16_kernel<false>), grid, dim3(256), 0, st, frames, h, w, fb, gi, colour, di, top, out);
    return check_launch("gather_i420_16_kernel");
}

int quantize_yuv420_16(const char* what, const float* in, int n, int H, int W, int colour, int depth, uint8_t* out, void* stream) {
    if (!in || !out) return fail(what, "null pointer");
    if (n < 1 || n > 65535 || H < 1 || W < 1) return fail(what, "n in 1 .. 65535, H, W >= 1");
    if (int rc = check_depth16(colour, depth, what)) return rc;
    if (reinterpret_cast<uintptr_t>(out) & 1) return fail(what, "out must be 2-byte aligned (16-bit samples)");
    if (reinterpret_cast<uintptr_t>(in) & 3) return fail(what, "in must be 4-byte aligned");
    const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0;
    const long long units = (long long)((H + 1) / 2) * (vec ? W / 4 : (W + 1) / 2);
    const dim3 grid(blocks_for(units), n);
    const long long fb = 2 * i420_bytes(H, W);
    const float k = (float)(1 << (depth - 8));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (colour == 0) {
        if (vec) hipLaunchKernelGGL((quantize_i420_16_kernel<true, 0>), grid, dim3(256), 0, st, in, H, W, fb, k, out);
        else hipLaunchKernelGGL((quantize_i420_16_kernel<false, 0>), grid, dim3(256), 0, st, in, H, W, fb, k, out);
    } else {
        if (vec) hipLaunchKernelGGL((quantize_i420_16_kernel<true, 1>), grid, dim3(256), 0, st, in, H, W, fb, k, out);
        else hipLaunchKernelGGL((quantize_i420_16_kernel<false, 1>), grid, dim3(256), 0, st, in, H, W, fb, k, out);
    }
    return check_launch("quantize_i420_16_kernel");
}

// ---- ABI 39: the entries of every chroma layout ---------------------------------------------------------------------------------------
int check_chroma_depth(int chroma, int depth, const char* what) {
    if (chroma < SAVSR_CHROMA_420 || chroma > SAVSR_CHROMA_444) {
        set_error("invalid argument: %s: chroma %d (0 = 4:2:0, 1 = 4:2:2, 2 = 4:4:4)", what, chroma);
        return SAVSR_E_ARG;
    }
    if (depth != 8 && depth != 10 && depth != 12) { set_error("invalid argument: %s: depth %d (8, 10 or 12)", what, depth); return SAVSR_E_ARG; }
    return 0;
}

template <int SX>
void launch_gather_yuvp(bool vec, dim3 grid, hipStream_t st, const uint8_t* frames, int h, int w, long long fb, const YuvIdx& gi, int colour,
                        int depth, float* out) {
    if (depth == 8) {
        if (vec) hipLaunchKernelGGL((gather_yuvp_kernel<SX, true>), grid, dim3(256), 0, st, frames, h, w, fb, gi, colour, out);
        else hipLaunchKernelGGL((gather_yuvp_kernel<SX, false>), grid, dim3(256), 0, st, frames, h, w, fb, gi, colour, out);
    } else {
        const int di = depth == 10 ? 0 : 1;
        const uint32_t top = (1u << depth) - 1u;
        if (vec) hipLaunchKernelGGL((gather_yuvp_16_kernel<SX, true>), grid, dim3(256), 0, st, frames, h, w, fb, gi, colour, di, top, out);
        else hipLaunchKernelGGL((gather_yuvp_16_kernel<SX, false>), grid, dim3(256), 0, st, frames, h, w, fb, gi, colour, di, top, out);
    }
}

template <int SX, int C>
void launch_quantize_yuvp(bool vec, dim3 grid, hipStream_t st, const float* in, int H, int W, long long fb, uint8_t* out) {
    if (vec) hipLaunchKernelGGL((quantize_yuvp_kernel<SX, true, C>), grid, dim3(256), 0, st, in, H, W, fb, out);
    else hipLaunchKernelGGL((quantize_yuvp_kernel<SX, false, C>), grid, dim3(256), 0, st, in, H, W, fb, out);
}
template <int SX, int C>
void launch_quantize_yuvp_16(bool vec, dim3 grid, hipStream_t st, const float* in, int H, int W, long long fb, float k, uint8_t* out) {
    if (vec) hipLaunchKernelGGL((quantize_yuvp_16_kernel<SX, true, C>), grid, dim3(256), 0, st, in, H, W, fb, k, out);
    else hipLaunchKernelGGL((quantize_yuvp_16_kernel<SX, false, C>), grid, dim3(256), 0, st, in, H, W, fb, k, out);
}
template <int SX>
void launch_quantize_yuvp_any(bool vec, dim3 grid, hipStream_t st, const float* in, int H, int W, long long fb, int colour, int depth,
                              uint8_t* out) {
    if (depth == 8) {
        switch (colour) {
            case 0: launch_quantize_yuvp<SX, 0>(vec, grid, st, in, H, W, fb, out); break;
            case 1: launch_quantize_yuvp<SX, 1>(vec, grid, st, in, H, W, fb, out); break;
            case 2: launch_quantize_yuvp<SX, 2>(vec, grid, st, in, H, W, fb, out); break;
            default: launch_quantize_yuvp<SX, 3>(vec, grid, st, in, H, W, fb, out); break;
        }
    } else {
        const float k = (float)(1 << (depth - 8));
        if (colour == 0) launch_quantize_yuvp_16<SX, 0>(vec, grid, st, in, H, W, fb, k, out);
        else launch_quantize_yuvp_16<SX, 1>(vec, grid, st, in, H, W, fb, k, out);
    }
}

}  // namespace
}  // namespace savsr

using namespace savsr;

extern "C" int savsr_video_gather_yuv420(const uint8_t* frames, int n_frames, int h, int w, const int32_t* idx, int n_idx, int colour, float* out,
                                         void* stream) {
    return gather_yuv420("video_gather_yuv420", frames, n_frames, h, w, idx, n_idx, colour, out, stream);
}

extern "C" int savsr_video_quantize_yuv420(const float* in, int n, int H, int W, int colour, uint8_t* out, void* stream) {
    return quantize_yuv420("video_quantize_yuv420", in, n, H, W, colour, out, stream);
}

// The entries of ABI 35: colour space 0.
extern "C" int savsr_video_gather_i420(const uint8_t* frames, int n_frames, int h, int w, const int32_t* idx, int n_idx, float* out, void* stream) {
    return gather_yuv420("video_gather_i420", frames, n_frames, h, w, idx, n_idx, SAVSR_YUV_BT601, out, stream);
}

extern "C" int savsr_video_quantize_i420(const float* in, int n, int H, int W, uint8_t* out, void* stream) {
    return quantize_yuv420("video_quantize_i420", in, n, H, W, SAVSR_YUV_BT601, out, stream);
}

// ABI 38: 10- and 12-bit frames, little-endian 16-bit samples in the I420 plane order.
extern "C" int savsr_video_gather_yuv420_16(const uint8_t* frames, int n_frames, int h, int w, const int32_t* idx, int n_idx, int colour, int depth,
                                            float* out, void* stream) {
    return gather_yuv420_16("video_gather_yuv420_16", frames, n_frames, h, w, idx, n_idx, colour, depth, out, stream);
}

extern "C" int savsr_video_quantize_yuv420_16(const float* in, int n, int H, int W, int colour, int depth, uint8_t* out, void* stream) {
    return quantize_yuv420_16("video_quantize_yuv420_16", in, n, H, W, colour, depth, out, stream);
}

// ABI 39: one entry per side for every (chroma layout, depth).  chroma = SAVSR_CHROMA_420 runs the kernels above.
extern "C" int savsr_video_gather_yuvp(const uint8_t* frames, int n_frames, int h, int w, const int32_t* idx, int n_idx, int colour, int depth,
                                       int chroma, float* out, void* stream) {
    const char* what = "video_gather_yuvp";
    if (int rc = check_chroma_depth(chroma, depth, what)) return rc;
    if (!frames || !out) return fail(what, "null pointer");
    if (h < 1 || w < 1 || n_frames < 1) return fail(what, "h, w, n_frames >= 1");
    if (depth == 8) { if (int rc = check_colour(colour, what)) return rc; }
    else if (int rc = check_depth16(colour, depth, what)) return rc;
    if (depth != 8 && (reinterpret_cast<uintptr_t>(frames) & 1)) return fail(what, "frames must be 2-byte aligned (16-bit samples)");
    if (reinterpret_cast<uintptr_t>(out) & 3) return fail(what, "out must be 4-byte aligned");
    if (chroma == SAVSR_CHROMA_420) {
        return depth == 8 ? gather_yuv420(what, frames, n_frames, h, w, idx, n_idx, colour, out, stream)
                          : gather_yuv420_16(what, frames, n_frames, h, w, idx, n_idx, colour, depth, out, stream);
    }
    YuvIdx gi;
    if (int rc = load_idx(idx, n_idx, n_frames, &gi, what)) return rc;
    const int sx = chroma == SAVSR_CHROMA_422 ? 2 : 1;
    const uintptr_t fmask = depth == 8 ? 3 : 7;
    const bool vec = w % 4 == 0 && (reinterpret_cast<uintptr_t>(frames) & fmask) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const long long units = (long long)h * (vec ? w / 4 : (sx == 2 ? (w + 1) / 2 : w));
    const dim3 grid(blocks_for(units), n_idx);
    const long long fb = yuvp_bytes(h, w, sx) * (depth == 8 ? 1 : 2);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (sx == 2) launch_gather_yuvp<2>(vec, grid, st, frames, h, w, fb, gi, colour, depth, out);
    else launch_gather_yuvp<1>(vec, grid, st, frames, h, w, fb, gi, colour, depth, out);
    return check_launch(depth == 8 ? "gather_yuvp_kernel" : "gather_yuvp_16_kernel");
}

extern "C" int savsr_video_quantize_yuvp(const float* in, int n, int H, int W, int colour, int depth, int chroma, uint8_t* out, void* stream) {
    const char* what = "video_quantize_yuvp";
    if (int rc = check_chroma_depth(chroma, depth, what)) return rc;
    if (!in || !out) return fail(what, "null pointer");
    if (n < 1 || n > 65535 || H < 1 || W < 1) return fail(what, "n in 1 .. 65535, H, W >= 1");
    if (depth == 8) { if (int rc = check_colour(colour, what)) return rc; }
    else if (int rc = check_depth16(colour, depth, what)) return rc;
    if (depth != 8 && (reinterpret_cast<uintptr_t>(out) & 1)) return fail(what, "out must be 2-byte aligned (16-bit samples)");
    if (reinterpret_cast<uintptr_t>(in) & 3) return fail(what, "in must be 4-byte aligned");
    if (chroma == SAVSR_CHROMA_420) {
        return depth == 8 ? quantize_yuv420(what, in, n, H, W, colour, out, stream) : quantize_yuv420_16(what, in, n, H, W, colour, depth, out, stream);
    }
    const int sx = chroma == SAVSR_CHROMA_422 ? 2 : 1;
    const uintptr_t omask = depth == 8 ? 3 : 7;
    const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & omask) == 0;
    const long long units = (long long)H * (vec ? W / 4 : (sx == 2 ? (W + 1) / 2 : W));
    const dim3 grid(blocks_for(units), n);
    const long long fb = yuvp_bytes(H, W, sx) * (depth == 8 ? 1 : 2);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (sx == 2) launch_quantize_yuvp_any<2>(vec, grid, st, in, H, W, fb, colour, depth, out);
    else launch_quantize_yuvp_any<1>(vec, grid, st, in, H, W, fb, colour, depth, out);
    return check_launch(depth == 8 ? "quantize_yuvp_kernel" : "quantize_yuvp_16_kernel");
}
