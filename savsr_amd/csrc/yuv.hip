// Planar YUV on either side of the network: frames -> the fp32 planar RGB clip batch the engine stages, and the fp32 result -> frames for
// an encoder or a Y4M pipe.  The YUV counterparts of savsr_video_gather_u8 / _quantize_u8 (video.hip); like them not fused into the SATU /
// tail kernels (satu.hip, tail.hip and common.hpp stay as they are, and with them savsr_source_hash_satu() and savsr_amd/hr_plans.json).
//
// One gather kernel and one quantise kernel serve every format; a format is three compile-time choices:
//   block shape <SX, SY>   the pixels under one chroma sample: <2, 2> is 4:2:0, <2, 1> 4:2:2, <1, 1> 4:4:4.  A frame of an h x w picture is
//                          h * w Y samples, then ch * cw U, then ch * cw V, ch = ceil(h / SY), cw = ceil(w / SX); odd sizes are first class
//   sample type            uint8_t at 8 bits, a little-endian uint16_t at 10 and 12 (Y4M's C420p10 ...): load_samples / store_samples
//   arithmetic             a policy: Rgb8 (five tables in LDS) or Rgb16 (float arithmetic, min(s, 2^d - 1)) to RGB; Quant8<C> (rounded,
//                          clipped in full range) or Quant16<C> (times k = 2^(d - 8), rounded) from RGB, C the colour space
// and a thread's work is either the vector form (VEC: SY rows x 4 pixels with the widest accesses, conditions below) or the scalar form (one
// chroma sample and its SY x SX in-image pixels, sample-sized accesses).
//
//   rgb2ycbcr / ycbcr2rgb   lbasicsr/utils/color_util.py:5-35, 71-97   ITU-R BT.601, limited range, Matlab's rounded constants
//
// That is colour space 0 (SAVSR_YUV_BT601) and what the entries without a colour argument run.  1 .. 3 are BT.709 limited, BT.601 full
// (JFIF) and BT.709 full, built from (Kr, Kb, range) by make_matrix; the arithmetic is the same for all four, and full range clips the
// rounded samples to 0 .. 255 (pure red / blue give a chroma of 255.5, which rounds to 256).  10 and 12 bits are defined for limited range
// only (colour spaces 0 and 1): a sample is the 8-bit one times k, so the constants are the 8-bit ones scaled by a power of two.
//
// Chroma siting (savsr_video_gather_yuvs / _quantize_yuvs; yuv.py's "Chroma siting" is the specification): the kernels above read chroma by
// nearest replication and write it through a box, which models no siting.  gather_linear_kernel interpolates chroma linearly at the
// positions a siting gives the samples and quantize_cosited_kernel filters cosited axes with [1 2 1] / 4; they serve the <2, 2> and
// <2, 1> blocks and keep the thread ownership and the vector / scalar split of the two kernels above, whose code and instantiations they
// leave alone (siting 0, 4:4:4 and the centre-sited quantiser run those).
//
// savsr_amd/yuv.py restates both kernels in numpy and is what they are tested against, bit for bit: float32, a fixed operation order
// and no fused multiply-add (contraction is off for this whole file).
#include "common.hpp"
#include "dither.hpp"

#include <cstdint>
#include <type_traits>

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

// 10 and 12 bits: the to-RGB constants per (colour space, depth).
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

// The linear gather: to_rgb_coefficients for every colour space at depth 8 (k = 1) beside the limited-range rows at 10 and 12, where the
// two full-range rows are never read (the entry refuses them).  A table of its own, so that kToRgb16 and its readers stay as they are.
enum { N_DEPTHS = 3 };                           // 8, 10, 12
struct ToRgbLinAll { ToRgb16 c[N_COLOURS][N_DEPTHS]; };
constexpr ToRgbLinAll make_to_rgb_lin() {
    ToRgbLinAll a{};
    for (int c = 0; c < N_COLOURS; ++c) {
        a.c[c][0] = make_to_rgb16(kYuv.m[c], 1.0);
        a.c[c][1] = make_to_rgb16(kYuv.m[c], 4.0);
        a.c[c][2] = make_to_rgb16(kYuv.m[c], 16.0);
    }
    return a;
}
__constant__ ToRgbLinAll kToRgbLin = make_to_rgb_lin();

// ---- Samples ---------------------------------------------------------------------------------------------------------------------------
// N consecutive samples of type S in one access of N * sizeof(S) bytes: 2 (a 16-bit access), 4 (a dword) or 8 (a u32x2).  What VEC needs
// for them to be aligned: w % 4 == 0, frames 4 s-byte aligned with s the bytes per sample (so 4 bytes at 8 bits, 8 at 10 and 12), the
// fp32 side 16-byte aligned.  With w = 4 q, in bytes from the frame's start:
//   4:4:4   fb = 12 q h s; U at 4 q h s, V at 8 q h s; every row of every plane is 4 q s long       -> every 4-pixel group 4 s-aligned
//   4:2:2   fb = 8 q h s;  U at 4 q h s, V at 6 q h s; a chroma row is 2 q s long, a group's pair
//           of chroma samples lies 2 s (x0 / 4) into it                                              -> every chroma pair 2 s-aligned
//   4:2:0   fb = 4 q (h + ch) s; U at 4 q h s, V at (4 q h + 2 q ch) s; chroma rows and pairs as in
//           4:2:2, one row of them under two Y rows                                                  -> every chroma pair 2 s-aligned
// so the Y access (4 s bytes) and the 4:4:4 chroma access (4 s bytes) are naturally aligned, and the 4:2:2 / 4:2:0 chroma access (2 s
// bytes) is too.
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
template <int BYTES> struct Word;
template <> struct Word<2> { typedef uint16_t type; };
template <> struct Word<4> { typedef uint32_t type; };
template <> struct Word<8> { typedef u32x2 type; };
__device__ __forceinline__ uint32_t dword_of(uint16_t wd, int) { return wd; }
__device__ __forceinline__ uint32_t dword_of(uint32_t wd, int) { return wd; }
__device__ __forceinline__ uint32_t dword_of(u32x2 wd, int i) { return wd[i]; }
__device__ __forceinline__ void put_word(uint16_t* p, const uint32_t (&d)[2]) { *p = (uint16_t)d[0]; }
__device__ __forceinline__ void put_word(uint32_t* p, const uint32_t (&d)[2]) { *p = d[0]; }
__device__ __forceinline__ void put_word(u32x2* p, const uint32_t (&d)[2]) { *p = u32x2{d[0], d[1]}; }

template <int N, class S>
__device__ __forceinline__ void load_samples(const S* p, uint32_t (&s)[N]) {
    constexpr int BITS = 8 * sizeof(S);
    const typename Word<N * sizeof(S)>::type wd = *reinterpret_cast<const typename Word<N * sizeof(S)>::type*>(p);
#pragma unroll
    for (int e = 0; e < N; ++e) s[e] = (dword_of(wd, (BITS * e) >> 5) >> ((BITS * e) & 31)) & ((1u << BITS) - 1u);
}
// the mirror image; every s[e] fits its sample
template <int N, class S>
__device__ __forceinline__ void store_samples(S* p, const uint32_t (&s)[N]) {
    constexpr int BITS = 8 * sizeof(S);
    uint32_t d[2] = {0u, 0u};
#pragma unroll
    for (int e = 0; e < N; ++e) d[(BITS * e) >> 5] |= s[e] << ((BITS * e) & 31);
    put_word(reinterpret_cast<typename Word<N * sizeof(S)>::type*>(p), d);
}

// ---- To RGB ----------------------------------------------------------------------------------------------------------------------------
// A policy is the kernel argument; begin() gives what a thread converts with: clip(sample) and rgb(y, u, v) -> the pixel's clamped R, G, B.
// 8 bits: `colour` (0 .. N_COLOURS - 1, checked by the entry) picks the five tables, staged in LDS by the 256 threads of the block.
struct Rgb8 {
    typedef uint8_t Sample;
    int colour;
    struct Pixel {
        const float (*lut)[256];
        __device__ __forceinline__ uint32_t clip(uint32_t s) const { return s; }
        __device__ __forceinline__ void rgb(uint32_t y, uint32_t u, uint32_t v, float (&c)[3]) const {
            const float ty = lut[T_Y][y];
            c[0] = clamp01(ty + lut[T_RV][v]);
            c[1] = clamp01((ty + lut[T_GU][u]) + lut[T_GV][v]);
            c[2] = clamp01(ty + lut[T_BU][u]);
        }
    };
    __device__ __forceinline__ Pixel begin() const {
        __shared__ float lut[T_COUNT][256];
#pragma unroll
        for (int t = 0; t < T_COUNT; ++t) lut[t][threadIdx.x] = kYuvToRgb.c[colour].v[t][threadIdx.x];
        __syncthreads();
        return Pixel{lut};
    }
};
// 10 and 12 bits: no tables, the input is arithmetic and not a lookup (yuv.py's "High depth" is the specification).  ci, di: the row of
// kToRgb16; a sample above top = 2^d - 1 reads as top.  Yt = y c_y,  R = (Yt + v c_rv) + o_R,  G = ((Yt + u c_gu) + v c_gv) + o_G,
// B = (Yt + u c_bu) + o_B, every product and sum rounded to float32 (contraction is off).
struct Rgb16 {
    typedef uint16_t Sample;
    int ci, di;
    uint32_t top;
    struct Pixel {
        ToRgb16 k;
        uint32_t top;
        __device__ __forceinline__ uint32_t clip(uint32_t s) const { return min(s, top); }
        __device__ __forceinline__ void rgb(uint32_t y, uint32_t u, uint32_t v, float (&c)[3]) const {
            const float fy = (float)y, fu = (float)u, fv = (float)v;
            const float yt = fy * k.y;
            c[0] = clamp01((yt + fv * k.rv) + k.o_r);
            c[1] = clamp01(((yt + fu * k.gu) + fv * k.gv) + k.o_g);
            c[2] = clamp01((yt + fu * k.bu) + k.o_b);
        }
    };
    __device__ __forceinline__ Pixel begin() const { return Pixel{kToRgb16.c[ci][di], top}; }
};

// Frames [N][fb] -> fp32 planar RGB slots [n][3][h][w], slot k = frame idx.f[k].  A thread owns all SY rows under its chroma samples so
// that each is read once.  VEC: SY rows x 4 pixels -- 4 Y samples per row and the 4 / SX chroma samples under them in one access per
// plane, one float4 per plane row out; otherwise a chroma sample and its SY x SX in-image pixels with sample-sized loads and scalar stores.
template <int SX, int SY, bool VEC, class P>
__global__ __launch_bounds__(256) void gather_kernel(const uint8_t* __restrict__ src, int h, int w, long long fb, YuvIdx idx, P pol,
                                                     float* __restrict__ out) {
    typedef typename P::Sample S;
    const typename P::Pixel px = pol.begin();
    const int k = blockIdx.y;
    const long long npx = (long long)h * w;
    const int ch = (h + SY - 1) / SY, cw = (w + SX - 1) / SX;
    const S* fy = reinterpret_cast<const S*>(src + (long long)idx.f[k] * fb);
    const S* fu = fy + npx;
    const S* fv = fu + (long long)ch * cw;
    float* o = out + (long long)k * 3 * npx;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        constexpr int NC = 4 / SX;
        const int wq = w / 4;                                   // 4-pixel groups per row
        if (g >= (long long)ch * wq) return;
        const int cy = (int)(g / wq), x0 = (int)(g % wq) * 4;
        const long long coff = (long long)cy * cw + x0 / SX;
        uint32_t u[NC], v[NC];
        load_samples(fu + coff, u);
        load_samples(fv + coff, v);
#pragma unroll
        for (int j = 0; j < NC; ++j) { u[j] = px.clip(u[j]); v[j] = px.clip(v[j]); }
#pragma unroll
        for (int dy = 0; dy < SY; ++dy) {
            const int y = SY * cy + dy;
            if (SY > 1 && y >= h) break;
            const long long p = (long long)y * w + x0;
            uint32_t yy[4];
            load_samples(fy + p, yy);
            f32x4 rgb[3];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float c[3];
                px.rgb(px.clip(yy[e]), u[e / SX], v[e / SX], c);
#pragma unroll
                for (int q = 0; q < 3; ++q) rgb[q][e] = c[q];
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) *reinterpret_cast<f32x4*>(o + q * npx + p) = rgb[q];
        }
    } else {
        if (g >= (long long)ch * cw) return;
        const int cy = (int)(g / cw), cx = (int)(g % cw);
        const uint32_t u = px.clip(fu[(long long)cy * cw + cx]), v = px.clip(fv[(long long)cy * cw + cx]);
#pragma unroll
        for (int dy = 0; dy < SY && SY * cy + dy < h; ++dy) {
#pragma unroll
            for (int dx = 0; dx < SX && SX * cx + dx < w; ++dx) {
                const long long p = (long long)(SY * cy + dy) * w + SX * cx + dx;
                float c[3];
                px.rgb(px.clip(fy[p]), u, v, c);
#pragma unroll
                for (int q = 0; q < 3; ++q) o[q * npx + p] = c[q];
            }
        }
    }
}

// ---- To RGB, chroma interpolated linearly (yuv.py: interpolate_chroma, _i420_to_rgb_sited) -------------------------------------------------
// The policy: Rgb16's arithmetic on fractional chroma at every depth, 8 included (S = uint8_t, top = 255, row [colour][0] of kToRgbLin).
template <class S> struct RgbLin {
    typedef S Sample;
    int ci, di;
    uint32_t top;
    struct Pixel {
        ToRgb16 k;
        uint32_t top;
        __device__ __forceinline__ uint32_t clip(uint32_t s) const { return min(s, top); }
        __device__ __forceinline__ void rgb(uint32_t y, float fu, float fv, float (&c)[3]) const {
            const float yt = (float)y * k.y;
            c[0] = clamp01((yt + fv * k.rv) + k.o_r);
            c[1] = clamp01(((yt + fu * k.gu) + fv * k.gv) + k.o_g);
            c[2] = clamp01((yt + fu * k.bu) + k.o_b);
        }
    };
    __device__ __forceinline__ Pixel begin() const { return Pixel{kToRgbLin.c[ci][di], top}; }
};

// One subsampled axis, as an integer numerator over 4.  Pixel 2 c from C[c - 1] and C[c], pixel 2 c + 1 from C[c] and C[c + 1]:
//   centre-sited (the sample lies at 2 c + 0.5)   (3 C[c] + C[c - 1]) / 4      (3 C[c] + C[c + 1]) / 4
//   cosited      (the sample lies at 2 c)         C[c]                         (C[c] + C[c + 1]) / 2
template <bool COS> __device__ __forceinline__ uint32_t lerp_even(uint32_t prev, uint32_t cur) { return COS ? 4u * cur : 3u * cur + prev; }
template <bool COS> __device__ __forceinline__ uint32_t lerp_odd(uint32_t cur, uint32_t next) { return COS ? 2u * cur + 2u * next : 3u * cur + next; }

// The numerators of one chroma plane for a thread's SY rows x NP pixels, the pixels under chroma samples (cy, c0 .. c0 + NP / 2 - 1): over
// 16 in 4:2:0, over 4 in 4:2:2; at most 4095 * 16.  Every neighbour's index is clamped into the plane (edge samples replicated), so every
// access lies inside it; NP = 4 reads the thread's pair in one access (the alignment table above holds for every chroma row).
template <int SY, bool CX, bool CY, int NP, class S, class Px>
__device__ __forceinline__ void chroma_numerators(const S* __restrict__ pl, int ch, int cw, int cy, int c0, const Px& px, uint32_t (&num)[SY][NP]) {
    constexpr int NC = NP / 2;
    auto row = [&](int r, uint32_t (&hn)[NP]) {
        const S* p = pl + (long long)r * cw;
        uint32_t c[NC + 2];                                     // C[c0 - 1], C[c0 .. c0 + NC - 1], C[c0 + NC]
        if constexpr (NC == 2) {
            uint32_t t[2];
            load_samples(p + c0, t);
            c[1] = t[0];
            c[2] = t[1];
        } else {
            c[1] = p[c0];
        }
        c[0] = CX ? 0u : (uint32_t)p[max(c0 - 1, 0)];           // (a cosited axis has no use for the sample before)
        c[NC + 1] = p[min(c0 + NC, cw - 1)];
#pragma unroll
        for (int j = 0; j < NC + 2; ++j) c[j] = px.clip(c[j]);
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            hn[2 * j] = lerp_even<CX>(c[j], c[j + 1]);
            hn[2 * j + 1] = lerp_odd<CX>(c[j + 1], c[j + 2]);
        }
    };
    uint32_t mid[NP];
    row(cy, mid);
    if constexpr (SY == 1) {
#pragma unroll
        for (int e = 0; e < NP; ++e) num[0][e] = mid[e];
    } else {
        uint32_t up[NP] = {}, dn[NP];
        if constexpr (!CY) row(max(cy - 1, 0), up);
        row(min(cy + 1, ch - 1), dn);
#pragma unroll
        for (int e = 0; e < NP; ++e) {
            num[0][e] = lerp_even<CY>(up[e], mid[e]);
            num[1][e] = lerp_odd<CY>(mid[e], dn[e]);
        }
    }
}

// gather_kernel with chroma at every pixel interpolated between the two nearest samples per subsampled axis; CX / CY: that axis is cosited.
// Same units and ownership: a thread converts the SY rows x 4 (VEC) or x 2 pixels under its chroma samples and reads, beside them, the
// sample before (a centre-sited axis) and after them in the row, and the chroma row above (centre-sited) and below.
template <int SY, bool VEC, bool CX, bool CY, class P>
__global__ __launch_bounds__(256) void gather_linear_kernel(const uint8_t* __restrict__ src, int h, int w, long long fb, YuvIdx idx, P pol,
                                                            float* __restrict__ out) {
    typedef typename P::Sample S;
    constexpr int SX = 2;
    constexpr float SCALE = SY == 2 ? 0.0625f : 0.25f;
    const typename P::Pixel px = pol.begin();
    const int k = blockIdx.y;
    const long long npx = (long long)h * w;
    const int ch = (h + SY - 1) / SY, cw = (w + SX - 1) / SX;
    const S* fy = reinterpret_cast<const S*>(src + (long long)idx.f[k] * fb);
    const S* fu = fy + npx;
    const S* fv = fu + (long long)ch * cw;
    float* o = out + (long long)k * 3 * npx;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        const int wq = w / 4;
        if (g >= (long long)ch * wq) return;
        const int cy = (int)(g / wq), x0 = (int)(g % wq) * 4;
        uint32_t nu[SY][4], nv[SY][4];
        chroma_numerators<SY, CX, CY, 4>(fu, ch, cw, cy, x0 / SX, px, nu);
        chroma_numerators<SY, CX, CY, 4>(fv, ch, cw, cy, x0 / SX, px, nv);
#pragma unroll
        for (int dy = 0; dy < SY; ++dy) {
            const int y = SY * cy + dy;
            if (SY > 1 && y >= h) break;
            const long long p = (long long)y * w + x0;
            uint32_t yy[4];
            load_samples(fy + p, yy);
            f32x4 rgb[3];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float c[3];
                px.rgb(px.clip(yy[e]), (float)nu[dy][e] * SCALE, (float)nv[dy][e] * SCALE, c);
#pragma unroll
                for (int q = 0; q < 3; ++q) rgb[q][e] = c[q];
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) *reinterpret_cast<f32x4*>(o + q * npx + p) = rgb[q];
        }
    } else {
        if (g >= (long long)ch * cw) return;
        const int cy = (int)(g / cw), cx = (int)(g % cw);
        uint32_t nu[SY][2], nv[SY][2];
        chroma_numerators<SY, CX, CY, 2>(fu, ch, cw, cy, cx, px, nu);
        chroma_numerators<SY, CX, CY, 2>(fv, ch, cw, cy, cx, px, nv);
#pragma unroll
        for (int dy = 0; dy < SY; ++dy) {
#pragma unroll
            for (int dx = 0; dx < SX; ++dx) {
                if (SY * cy + dy >= h || SX * cx + dx >= w) continue;
                const long long p = (long long)(SY * cy + dy) * w + SX * cx + dx;
                float c[3];
                px.rgb(px.clip(fy[p]), (float)nu[dy][dx] * SCALE, (float)nv[dy][dx] * SCALE, c);
#pragma unroll
                for (int q = 0; q < 3; ++q) o[q * npx + p] = c[q];
            }
        }
    }
}

// ---- From RGB --------------------------------------------------------------------------------------------------------------------------
// rgb2ycbcr's rows in 8-bit steps: every product and every sum rounded to float32 (yuv.py: _row).  Plain operators under this file's
// `fp contract(off)`: the header's __fmul_rn / __fadd_rn are compiled with contraction allowed and fuse again once inlined.
// CLIP (full range): the rounded value clipped to 0 .. 255 (yuv.py: rgb_to_i420); limited range stays inside 16 .. 240 by itself.
// DITHER (the entries with _d; dither.hpp, savsr_amd/dither.py): floor(t + th) in rint's place, th the sample's threshold; the clip
// follows as it follows rint.  Without DITHER th is not read.
template <bool CLIP, bool DITHER>
__device__ __forceinline__ uint32_t row3_u8(const float (&kk)[3], float off, float th, float r, float g, float b) {
    const float t = ((r * kk[0] + g * kk[1]) + b * kk[2]) + off;
    const float v = DITHER ? dither_add_floor(t, th) : rintf(t);
    return (uint32_t)(CLIP ? fminf(fmaxf(v, 0.f), 255.f) : v);
}
// rint(row * k): the 8-bit row's float32 value times k = 2^(d - 8), exact, then half to even.  Limited range stays inside 16 k .. 240 k
// by itself: no clip.
template <bool DITHER>
__device__ __forceinline__ uint32_t row3_u16(const float (&kk)[3], float off, float k, float th, float r, float g, float b) {
    const float t = (((r * kk[0] + g * kk[1]) + b * kk[2]) + off) * k;
    return (uint32_t)(DITHER ? dither_add_floor(t, th) : rintf(t));
}
// The policies: the three rows of colour space C, a template argument so that the coefficients are constants of the instantiation
// (immediates in the code).  k is the kernel's argument; 8 bits has no use for it.  D, th: the kernel's DITHER and the sample's threshold.
template <int C> struct Quant8 {
    typedef uint8_t Sample;
    template <bool D> static __device__ __forceinline__ uint32_t y(float, float th, float r, float g, float b) { constexpr YuvMatrix m = kYuv.m[C]; return row3_u8<m.full, D>(m.ky, m.oy, th, r, g, b); }
    template <bool D> static __device__ __forceinline__ uint32_t cb(float, float th, float r, float g, float b) { constexpr YuvMatrix m = kYuv.m[C]; return row3_u8<m.full, D>(m.kcb, m.oc, th, r, g, b); }
    template <bool D> static __device__ __forceinline__ uint32_t cr(float, float th, float r, float g, float b) { constexpr YuvMatrix m = kYuv.m[C]; return row3_u8<m.full, D>(m.kcr, m.oc, th, r, g, b); }
};
template <int C> struct Quant16 {
    static_assert(!kYuv.m[C].full, "high depth is defined for limited range only");
    typedef uint16_t Sample;
    template <bool D> static __device__ __forceinline__ uint32_t y(float k, float th, float r, float g, float b) { constexpr YuvMatrix m = kYuv.m[C]; return row3_u16<D>(m.ky, m.oy, k, th, r, g, b); }
    template <bool D> static __device__ __forceinline__ uint32_t cb(float k, float th, float r, float g, float b) { constexpr YuvMatrix m = kYuv.m[C]; return row3_u16<D>(m.kcb, m.oc, k, th, r, g, b); }
    template <bool D> static __device__ __forceinline__ uint32_t cr(float k, float th, float r, float g, float b) { constexpr YuvMatrix m = kYuv.m[C]; return row3_u16<D>(m.kcr, m.oc, k, th, r, g, b); }
};

// Mean of one channel over a block's in-image pixels, at(dy, dx) the clamped value (yuv.py: _block_mean): ((a + b) + (c + d)) * 0.25 with
// a b the upper row, (a + b) * 0.5 for a horizontal pair (4:2:2; the last row of an odd H in 4:2:0), (a + c) * 0.5 for a vertical pair
// (the last column of an odd W in 4:2:0), the pixel alone; in 4:4:4 always the pixel's own value.
template <int SX, int SY, class At>
__device__ __forceinline__ float block_mean(bool two_x, bool two_y, At at) {
    if constexpr (SX == 2 && SY == 2) { if (two_x && two_y) return ((at(0, 0) + at(0, 1)) + (at(1, 0) + at(1, 1))) * 0.25f; }
    if constexpr (SX == 2) { if (two_x) return (at(0, 0) + at(0, 1)) * 0.5f; }
    if constexpr (SY == 2) { if (two_y) return (at(0, 0) + at(1, 0)) * 0.5f; }
    return at(0, 0);
}

// fp32 planar RGB [n][3][H][W] -> frames [n][fb]: clamp(0, 1); Y per pixel; Cb / Cr from block_mean of the clamped RGB; rintf (round half
// to even).  VEC: a thread owns SY rows x 4 pixels -- one float4 per plane row in (nontemporal: the result is read once), 4 Y samples per
// row and the 4 / SX chroma samples under them out in one access per plane; otherwise a chroma sample and its SY x SX in-image pixels, scalar.
// DITHER (savsr_video_quantize_yuvs_d): every sample takes floor(t + theta) in rint's place, theta at its coordinates in its own plane --
// pixel (y, x) for Y, chroma sample (cy, cx) for Cb and Cr, which share it.
template <int SX, int SY, bool VEC, bool DITHER, class Q>
__global__ __launch_bounds__(256) void quantize_kernel(const float* __restrict__ in, int H, int W, long long fb, float k, uint8_t* __restrict__ out) {
    typedef typename Q::Sample S;
    auto th = [](int y, int x) { if constexpr (DITHER) return dither_theta((uint32_t)y, (uint32_t)x); else return 0.f; };
    const int f = blockIdx.y;
    const long long npx = (long long)H * W;
    const int ch = (H + SY - 1) / SY, cw = (W + SX - 1) / SX;
    const float* src = in + (long long)f * 3 * npx;
    S* fy = reinterpret_cast<S*>(out + (long long)f * fb);
    S* fu = fy + npx;
    S* fv = fu + (long long)ch * cw;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        constexpr int NC = 4 / SX;
        const int wq = W / 4;
        if (g >= (long long)ch * wq) return;
        const int cy = (int)(g / wq), x0 = (int)(g % wq) * 4;
        const bool two_y = SY == 2 && 2 * cy + 1 < H;
        f32x4 px[SY][3];
#pragma unroll
        for (int dy = 0; dy < SY; ++dy) {
            if (dy == 1 && !two_y) break;
            const long long p = (long long)(SY * cy + dy) * W + x0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const f32x4 x = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + c * npx + p));
#pragma unroll
                for (int e = 0; e < 4; ++e) px[dy][c][e] = clamp01(x[e]);
            }
            uint32_t yy[4];
            float ty[4] = {};
            if constexpr (DITHER) dither_theta4((uint32_t)(SY * cy + dy), (uint32_t)x0, ty);
#pragma unroll
            for (int e = 0; e < 4; ++e) yy[e] = Q::template y<DITHER>(k, ty[e], px[dy][0][e], px[dy][1][e], px[dy][2][e]);
            store_samples(fy + p, yy);
        }
        uint32_t u[NC], v[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            float m[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) m[c] = block_mean<SX, SY>(true, two_y, [&](int dy, int dx) { return px[dy][c][SX * j + dx]; });
            const float tc = th(cy, x0 / SX + j);
            u[j] = Q::template cb<DITHER>(k, tc, m[0], m[1], m[2]);
            v[j] = Q::template cr<DITHER>(k, tc, m[0], m[1], m[2]);
        }
        const long long coff = (long long)cy * cw + x0 / SX;
        store_samples(fu + coff, u);
        store_samples(fv + coff, v);
    } else {
        if (g >= (long long)ch * cw) return;
        const int cy = (int)(g / cw), cx = (int)(g % cw);
        const bool two_y = SY == 2 && 2 * cy + 1 < H, two_x = SX == 2 && 2 * cx + 1 < W;
        float q[SY][SX][3];
#pragma unroll
        for (int dy = 0; dy < SY; ++dy) {
#pragma unroll
            for (int dx = 0; dx < SX; ++dx) {
                if ((dy && !two_y) || (dx && !two_x)) continue;
                const long long p = (long long)(SY * cy + dy) * W + SX * cx + dx;
#pragma unroll
                for (int c = 0; c < 3; ++c) q[dy][dx][c] = clamp01(src[c * npx + p]);
                fy[p] = (S)Q::template y<DITHER>(k, th(SY * cy + dy, SX * cx + dx), q[dy][dx][0], q[dy][dx][1], q[dy][dx][2]);
            }
        }
        float m[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = block_mean<SX, SY>(two_x, two_y, [&](int dy, int dx) { return q[dy][dx][c]; });
        const float tc = th(cy, cx);
        fu[(long long)cy * cw + cx] = (S)Q::template cb<DITHER>(k, tc, m[0], m[1], m[2]);
        fv[(long long)cy * cw + cx] = (S)Q::template cr<DITHER>(k, tc, m[0], m[1], m[2]);
    }
}

// ---- From RGB, cosited chroma (yuv.py: filter_chroma_rgb) ----------------------------------------------------------------------------------
// [1 2 1] / 4 along a cosited axis, in float32 in this order.
__device__ __forceinline__ float h3(float l, float c, float r) { return ((l + r) + (c + c)) * 0.25f; }

// quantize_kernel with Cb / Cr from horizontally cosited chroma ("left"; TOP: vertically too, "topleft").  Hrow(y) = h3 of the clamped RGB
// at x = 2 cx - 1, 2 cx, 2 cx + 1, every index clamped into the image; 4:2:2: Hrow(y); 4:2:0 left: (Hrow(2 cy) + Hrow(2 cy + 1)) * 0.5,
// Hrow(2 cy) alone on the last row of an odd H; topleft: h3 of Hrow at rows 2 cy - 1, 2 cy, 2 cy + 1, clamped.  Same units and ownership:
// a thread writes the Y of its SY rows x 4 (VEC) or x 2 pixels and the chroma samples over them, and reads beside its own pixels the one
// left of them and, for TOP, the row above with plain loads (a neighbour's lines).  A clamped row or column repeats a value the thread
// already holds, and the same operations on the same values give the same bits, so those are reused and not loaded again.  DITHER: as in
// quantize_kernel, the thresholds at the same coordinates.
template <int SY, bool VEC, bool TOP, bool DITHER, class Q>
__global__ __launch_bounds__(256) void quantize_cosited_kernel(const float* __restrict__ in, int H, int W, long long fb, float k, uint8_t* __restrict__ out) {
    static_assert(SY == 2 || !TOP, "4:2:2 has no vertical subsampling");
    typedef typename Q::Sample S;
    auto th = [](int y, int x) { if constexpr (DITHER) return dither_theta((uint32_t)y, (uint32_t)x); else return 0.f; };
    constexpr int SX = 2;
    const int f = blockIdx.y;
    const long long npx = (long long)H * W;
    const int ch = (H + SY - 1) / SY, cw = (W + SX - 1) / SX;
    const float* src = in + (long long)f * 3 * npx;
    S* fy = reinterpret_cast<S*>(out + (long long)f * fb);
    S* fu = fy + npx;
    S* fv = fu + (long long)ch * cw;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    auto at = [&](int c, int y, int x) { return clamp01(src[c * npx + (long long)y * W + x]); };
    // the chroma sample's RGB from Hrow of its rows: own[dy], and for TOP the row above
    auto vertical = [&](bool two_y, float up, float h0, float h1) {
        if constexpr (SY == 1) return h0;
        else if constexpr (TOP) return h3(up, h0, two_y ? h1 : h0);
        else return two_y ? (h0 + h1) * 0.5f : h0;
    };
    if (VEC) {
        constexpr int NC = 2;
        const int wq = W / 4;
        if (g >= (long long)ch * wq) return;
        const int cy = (int)(g / wq), x0 = (int)(g % wq) * 4;
        const bool two_y = SY == 2 && 2 * cy + 1 < H;
        const int xl = max(x0 - 1, 0);
        float own[SY][3][NC] = {}, up[3][NC];
#pragma unroll
        for (int dy = 0; dy < SY; ++dy) {
            if (dy == 1 && !two_y) break;
            const int y = SY * cy + dy;
            const long long p = (long long)y * W + x0;
            f32x4 px[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const f32x4 x = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + c * npx + p));
#pragma unroll
                for (int e = 0; e < 4; ++e) px[c][e] = clamp01(x[e]);
            }
            uint32_t yy[4];
            float ty[4] = {};
            if constexpr (DITHER) dither_theta4((uint32_t)y, (uint32_t)x0, ty);
#pragma unroll
            for (int e = 0; e < 4; ++e) yy[e] = Q::template y<DITHER>(k, ty[e], px[0][e], px[1][e], px[2][e]);
            store_samples(fy + p, yy);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                own[dy][c][0] = h3(at(c, y, xl), px[c][0], px[c][1]);
                own[dy][c][1] = h3(px[c][1], px[c][2], px[c][3]);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (TOP && cy > 0) {
                const int y = 2 * cy - 1;
                const f32x4 x = *reinterpret_cast<const f32x4*>(src + c * npx + (long long)y * W + x0);
                up[c][0] = h3(at(c, y, xl), clamp01(x[0]), clamp01(x[1]));
                up[c][1] = h3(clamp01(x[1]), clamp01(x[2]), clamp01(x[3]));
            } else {
                up[c][0] = own[0][c][0];
                up[c][1] = own[0][c][1];
            }
        }
        uint32_t u[NC], v[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            float m[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) m[c] = vertical(two_y, up[c][j], own[0][c][j], own[SY - 1][c][j]);
            const float tc = th(cy, x0 / SX + j);
            u[j] = Q::template cb<DITHER>(k, tc, m[0], m[1], m[2]);
            v[j] = Q::template cr<DITHER>(k, tc, m[0], m[1], m[2]);
        }
        const long long coff = (long long)cy * cw + x0 / SX;
        store_samples(fu + coff, u);
        store_samples(fv + coff, v);
    } else {
        if (g >= (long long)ch * cw) return;
        const int cy = (int)(g / cw), cx = (int)(g % cw);
        const bool two_y = SY == 2 && 2 * cy + 1 < H, two_x = 2 * cx + 1 < W;
        const int xl = max(2 * cx - 1, 0), xc = 2 * cx, xr = two_x ? xc + 1 : xc;
        float own[SY][3] = {}, up[3];
#pragma unroll
        for (int dy = 0; dy < SY; ++dy) {
            if (dy == 1 && !two_y) break;
            const int y = SY * cy + dy;
            float q[2][3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                q[0][c] = at(c, y, xc);
                q[1][c] = at(c, y, xr);
                own[dy][c] = h3(at(c, y, xl), q[0][c], q[1][c]);
            }
            fy[(long long)y * W + xc] = (S)Q::template y<DITHER>(k, th(y, xc), q[0][0], q[0][1], q[0][2]);
            if (two_x) fy[(long long)y * W + xr] = (S)Q::template y<DITHER>(k, th(y, xr), q[1][0], q[1][1], q[1][2]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) up[c] = (TOP && cy > 0) ? h3(at(c, 2 * cy - 1, xl), at(c, 2 * cy - 1, xc), at(c, 2 * cy - 1, xr)) : own[0][c];
        float m[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = vertical(two_y, up[c], own[0][c], own[SY - 1][c]);
        const float tc = th(cy, cx);
        fu[(long long)cy * cw + cx] = (S)Q::template cb<DITHER>(k, tc, m[0], m[1], m[2]);
        fv[(long long)cy * cw + cx] = (S)Q::template cr<DITHER>(k, tc, m[0], m[1], m[2]);
    }
}

// ---- Host side -------------------------------------------------------------------------------------------------------------------------
// What the entries differ in when they refuse; everything else is one body per direction.
enum Rules {
    RULES_8,         // _i420, _yuv420: the depth is 8 by construction; no pointer is refused for its alignment
    RULES_16,        // _yuv420_16: depth 10 or 12, named as such
    RULES_LAYOUT,    // _yuvp: chroma and depth (8, 10 or 12) are checked before anything else
};

int fail(const char* what, const char* msg) {
    set_error("invalid argument: %s: %s", what, msg);
    return SAVSR_E_ARG;
}

int check_layout(const char* what, Rules rules, int depth, int chroma) {
    if (rules != RULES_LAYOUT) return 0;
    if (chroma < SAVSR_CHROMA_420 || chroma > SAVSR_CHROMA_444) {
        set_error("invalid argument: %s: chroma %d (0 = 4:2:0, 1 = 4:2:2, 2 = 4:4:4)", what, chroma);
        return SAVSR_E_ARG;
    }
    if (depth != 8 && depth != 10 && depth != 12) { set_error("invalid argument: %s: depth %d (8, 10 or 12)", what, depth); return SAVSR_E_ARG; }
    return 0;
}

// a colour space the depth is defined for, or the refusal that names the rule
int check_depth_colour(const char* what, Rules rules, int colour, int depth) {
    if (rules == RULES_16 && depth != 10 && depth != 12) {
        set_error("invalid argument: %s: depth %d (10 or 12; 8 bits: the entries without _16)", what, depth);
        return SAVSR_E_ARG;
    }
    if (depth == 8 && (colour < 0 || colour >= N_COLOURS)) {
        set_error("invalid argument: %s: colour %d (0 .. %d)", what, colour, N_COLOURS - 1);
        return SAVSR_E_ARG;
    }
    if (depth != 8 && (colour < 0 || colour >= N_COLOURS_16)) {
        set_error("invalid argument: %s: colour %d (0 .. %d: 10 and 12 bits are defined for limited range only)", what, colour, N_COLOURS_16 - 1);
        return SAVSR_E_ARG;
    }
    return 0;
}

inline bool aligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

int load_idx(const int32_t* idx, int n, int n_frames, YuvIdx* gi, const char* what) {
    if (!idx) { set_error("%s: null index list", what); return SAVSR_E_ARG; }
    if (n < 1 || n > SAVSR_VIDEO_MAX_SLOTS) { set_error("%s: %d slots (1 .. %d)", what, n, SAVSR_VIDEO_MAX_SLOTS); return SAVSR_E_ARG; }
    for (int i = 0; i < n; ++i) {
        if (idx[i] < 0 || idx[i] >= n_frames) { set_error("%s: slot %d names frame %d of %d", what, i, idx[i], n_frames); return SAVSR_E_ARG; }
        gi->f[i] = idx[i];
    }
    return 0;
}

// The launch of n frames / slots of h x w: the vector form where the alignment table above holds, a thread per unit, the frame's bytes.
struct Plan {
    bool vec;
    dim3 grid;
    long long fb;
};
Plan plan(int h, int w, int n, int depth, int chroma, const void* samples, const void* fp32) {
    const int sx = chroma == SAVSR_CHROMA_444 ? 1 : 2, sy = chroma == SAVSR_CHROMA_420 ? 2 : 1, s = depth == 8 ? 1 : 2;
    const int ch = (h + sy - 1) / sy, cw = (w + sx - 1) / sx;
    Plan p;
    p.vec = w % 4 == 0 && aligned(samples, 4 * s) && aligned(fp32, 16);
    p.grid = dim3(blocks_for((long long)ch * (p.vec ? w / 4 : cw)), n);
    p.fb = ((long long)h * w + 2LL * ch * cw) * s;
    return p;
}

template <int SX_, int SY_> struct Block { static constexpr int SX = SX_, SY = SY_; };
template <class F> void with_block(int chroma, F f) {
    switch (chroma) {
        case SAVSR_CHROMA_420: f(Block<2, 2>{}); break;
        case SAVSR_CHROMA_422: f(Block<2, 1>{}); break;
        default: f(Block<1, 1>{}); break;
    }
}

// The body of every gather entry: `what` names the one called in its messages.
int gather(const char* what, Rules rules, const uint8_t* frames, int n_frames, int h, int w, const int32_t* idx, int n_idx, int colour, int depth,
           int chroma, float* out, void* stream) {
    if (int rc = check_layout(what, rules, depth, chroma)) return rc;
    if (!frames || !out) return fail(what, "null pointer");
    if (h < 1 || w < 1 || n_frames < 1) return fail(what, "h, w, n_frames >= 1");
    if (int rc = check_depth_colour(what, rules, colour, depth)) return rc;
    if (rules != RULES_8) {
        if (depth != 8 && !aligned(frames, 2)) return fail(what, "frames must be 2-byte aligned (16-bit samples)");
        if (!aligned(out, 4)) return fail(what, "out must be 4-byte aligned");
    }
    YuvIdx gi;
    if (int rc = load_idx(idx, n_idx, n_frames, &gi, what)) return rc;
    const Plan pl = plan(h, w, n_idx, depth, chroma, frames, out);
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto launch = [&](auto pol) {
        with_block(chroma, [&](auto b) {
            typedef decltype(b) B;
            typedef decltype(pol) P;
            if (pl.vec) hipLaunchKernelGGL((gather_kernel<B::SX, B::SY, true, P>), pl.grid, dim3(256), 0, st, frames, h, w, pl.fb, gi, pol, out);
            else hipLaunchKernelGGL((gather_kernel<B::SX, B::SY, false, P>), pl.grid, dim3(256), 0, st, frames, h, w, pl.fb, gi, pol, out);
        });
    };
    if (depth == 8) launch(Rgb8{colour});
    else launch(Rgb16{colour, depth == 10 ? 0 : 1, (1u << depth) - 1u});
    return check_launch("gather_kernel");
}

// The body of every quantise entry.  dither: the DITHER instantiations (savsr_video_quantize_yuvs_d alone asks for them).
int quantize(const char* what, Rules rules, const float* in, int n, int H, int W, int colour, int depth, int chroma, uint8_t* out, void* stream,
             bool dither = false) {
    if (int rc = check_layout(what, rules, depth, chroma)) return rc;
    if (!in || !out) return fail(what, "null pointer");
    if (n < 1 || n > 65535 || H < 1 || W < 1) return fail(what, "n in 1 .. 65535, H, W >= 1");
    if (int rc = check_depth_colour(what, rules, colour, depth)) return rc;
    if (rules != RULES_8) {
        if (depth != 8 && !aligned(out, 2)) return fail(what, "out must be 2-byte aligned (16-bit samples)");
        if (!aligned(in, 4)) return fail(what, "in must be 4-byte aligned");
    }
    const Plan pl = plan(H, W, n, depth, chroma, out, in);
    const float k = (float)(1 << (depth - 8));
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto launch = [&](auto q) {
        with_block(chroma, [&](auto b) {
            typedef decltype(b) B;
            typedef decltype(q) Q;
            auto go = [&](auto d) {
                constexpr bool D = decltype(d)::value;
                if (pl.vec) hipLaunchKernelGGL((quantize_kernel<B::SX, B::SY, true, D, Q>), pl.grid, dim3(256), 0, st, in, H, W, pl.fb, k, out);
                else hipLaunchKernelGGL((quantize_kernel<B::SX, B::SY, false, D, Q>), pl.grid, dim3(256), 0, st, in, H, W, pl.fb, k, out);
            };
            if (dither) go(std::true_type{});
            else go(std::false_type{});
        });
    };
    switch (depth == 8 ? colour : N_COLOURS + colour) {
        case 0: launch(Quant8<0>{}); break;
        case 1: launch(Quant8<1>{}); break;
        case 2: launch(Quant8<2>{}); break;
        case 3: launch(Quant8<3>{}); break;
        case N_COLOURS: launch(Quant16<0>{}); break;
        default: launch(Quant16<1>{}); break;
    }
    return check_launch("quantize_kernel");
}

// ---- Chroma siting: the bodies of savsr_video_gather_yuvs / _quantize_yuvs -------------------------------------------------------------------
// A siting the layout has, or the refusal that names the rule; after check_layout, before anything else.
int check_siting(const char* what, int chroma, int siting) {
    if (siting < SAVSR_SITING_NONE || siting > SAVSR_SITING_TOPLEFT) {
        set_error("invalid argument: %s: siting %d (0 = not modelled, 1 = centre, 2 = left, 3 = topleft)", what, siting);
        return SAVSR_E_ARG;
    }
    if (siting == SAVSR_SITING_TOPLEFT && chroma == SAVSR_CHROMA_422) {
        set_error("invalid argument: %s: siting 3 (topleft) with chroma 1 (4:2:2): 4:2:2 has no vertical subsampling, its cosited form is siting 2 (left)", what);
        return SAVSR_E_ARG;
    }
    return 0;
}

int gather_sited(const char* what, const uint8_t* frames, int n_frames, int h, int w, const int32_t* idx, int n_idx, int colour, int depth, int chroma,
                 int siting, float* out, void* stream) {
    if (int rc = check_layout(what, RULES_LAYOUT, depth, chroma)) return rc;
    if (int rc = check_siting(what, chroma, siting)) return rc;
    // not modelled, or nothing to resample: the nearest gather, its instantiations and its bytes
    if (siting == SAVSR_SITING_NONE || chroma == SAVSR_CHROMA_444)
        return gather(what, RULES_LAYOUT, frames, n_frames, h, w, idx, n_idx, colour, depth, chroma, out, stream);
    if (!frames || !out) return fail(what, "null pointer");
    if (h < 1 || w < 1 || n_frames < 1) return fail(what, "h, w, n_frames >= 1");
    if (int rc = check_depth_colour(what, RULES_LAYOUT, colour, depth)) return rc;
    if (depth != 8 && !aligned(frames, 2)) return fail(what, "frames must be 2-byte aligned (16-bit samples)");
    if (!aligned(out, 4)) return fail(what, "out must be 4-byte aligned");
    YuvIdx gi;
    if (int rc = load_idx(idx, n_idx, n_frames, &gi, what)) return rc;
    const Plan pl = plan(h, w, n_idx, depth, chroma, frames, out);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int di = depth == 8 ? 0 : depth == 10 ? 1 : 2;
    const uint32_t top = (1u << depth) - 1u;
    auto launch = [&](auto sy, auto cx, auto cy) {
        constexpr int SY = decltype(sy)::value;
        constexpr bool CX = decltype(cx)::value, CY = decltype(cy)::value;
        auto go = [&](auto pol) {
            typedef decltype(pol) P;
            if (pl.vec) hipLaunchKernelGGL((gather_linear_kernel<SY, true, CX, CY, P>), pl.grid, dim3(256), 0, st, frames, h, w, pl.fb, gi, pol, out);
            else hipLaunchKernelGGL((gather_linear_kernel<SY, false, CX, CY, P>), pl.grid, dim3(256), 0, st, frames, h, w, pl.fb, gi, pol, out);
        };
        if (depth == 8) go(RgbLin<uint8_t>{colour, di, top});
        else go(RgbLin<uint16_t>{colour, di, top});
    };
    typedef std::integral_constant<int, 1> One;
    typedef std::integral_constant<int, 2> Two;
    if (chroma == SAVSR_CHROMA_422) {                           // (the vertical axis is not subsampled: CY has no meaning)
        if (siting == SAVSR_SITING_CENTRE) launch(One{}, std::false_type{}, std::false_type{});
        else launch(One{}, std::true_type{}, std::false_type{});
    } else if (siting == SAVSR_SITING_CENTRE) {
        launch(Two{}, std::false_type{}, std::false_type{});
    } else if (siting == SAVSR_SITING_LEFT) {
        launch(Two{}, std::true_type{}, std::false_type{});
    } else {
        launch(Two{}, std::true_type{}, std::true_type{});
    }
    return check_launch("gather_linear_kernel");
}

int quantize_sited(const char* what, const float* in, int n, int H, int W, int colour, int depth, int chroma, int siting, uint8_t* out, void* stream,
                   bool dither = false) {
    if (int rc = check_layout(what, RULES_LAYOUT, depth, chroma)) return rc;
    if (int rc = check_siting(what, chroma, siting)) return rc;
    // not modelled, centre-sited (the box is its filter) or nothing to resample: the box quantiser, its instantiations and its bytes
    if (siting <= SAVSR_SITING_CENTRE || chroma == SAVSR_CHROMA_444)
        return quantize(what, RULES_LAYOUT, in, n, H, W, colour, depth, chroma, out, stream, dither);
    if (!in || !out) return fail(what, "null pointer");
    if (n < 1 || n > 65535 || H < 1 || W < 1) return fail(what, "n in 1 .. 65535, H, W >= 1");
    if (int rc = check_depth_colour(what, RULES_LAYOUT, colour, depth)) return rc;
    if (depth != 8 && !aligned(out, 2)) return fail(what, "out must be 2-byte aligned (16-bit samples)");
    if (!aligned(in, 4)) return fail(what, "in must be 4-byte aligned");
    const Plan pl = plan(H, W, n, depth, chroma, out, in);
    const float k = (float)(1 << (depth - 8));
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto launch = [&](auto q) {
        typedef decltype(q) Q;
        auto go = [&](auto sy, auto top) {
            constexpr int SY = decltype(sy)::value;
            constexpr bool TOP = decltype(top)::value;
            auto with = [&](auto d) {
                constexpr bool D = decltype(d)::value;
                if (pl.vec) hipLaunchKernelGGL((quantize_cosited_kernel<SY, true, TOP, D, Q>), pl.grid, dim3(256), 0, st, in, H, W, pl.fb, k, out);
                else hipLaunchKernelGGL((quantize_cosited_kernel<SY, false, TOP, D, Q>), pl.grid, dim3(256), 0, st, in, H, W, pl.fb, k, out);
            };
            if (dither) with(std::true_type{});
            else with(std::false_type{});
        };
        if (chroma == SAVSR_CHROMA_422) go(std::integral_constant<int, 1>{}, std::false_type{});
        else if (siting == SAVSR_SITING_LEFT) go(std::integral_constant<int, 2>{}, std::false_type{});
        else go(std::integral_constant<int, 2>{}, std::true_type{});
    };
    switch (depth == 8 ? colour : N_COLOURS + colour) {
        case 0: launch(Quant8<0>{}); break;
        case 1: launch(Quant8<1>{}); break;
        case 2: launch(Quant8<2>{}); break;
        case 3: launch(Quant8<3>{}); break;
        case N_COLOURS: launch(Quant16<0>{}); break;
        default: launch(Quant16<1>{}); break;
    }
    return check_launch("quantize_cosited_kernel");
}

}  // namespace
}  // namespace savsr

using namespace savsr;

// Colour space 0, 8 bits, 4:2:0.
extern "C" int savsr_video_gather_i420(const uint8_t* frames, int n_frames, int h, int w, const int32_t* idx, int n_idx, float* out, void* stream) {
    return gather("video_gather_i420", RULES_8, frames, n_frames, h, w, idx, n_idx, SAVSR_YUV_BT601, 8, SAVSR_CHROMA_420, out, stream);
}

extern "C" int savsr_video_quantize_i420(const float* in, int n, int H, int W, uint8_t* out, void* stream) {
    return quantize("video_quantize_i420", RULES_8, in, n, H, W, SAVSR_YUV_BT601, 8, SAVSR_CHROMA_420, out, stream);
}

// The colour space as an argument.
extern "C" int savsr_video_gather_yuv420(const uint8_t* frames, int n_frames, int h, int w, const int32_t* idx, int n_idx, int colour, float* out,
                                         void* stream) {
    return gather("video_gather_yuv420", RULES_8, frames, n_frames, h, w, idx, n_idx, colour, 8, SAVSR_CHROMA_420, out, stream);
}

extern "C" int savsr_video_quantize_yuv420(const float* in, int n, int H, int W, int colour, uint8_t* out, void* stream) {
    return quantize("video_quantize_yuv420", RULES_8, in, n, H, W, colour, 8, SAVSR_CHROMA_420, out, stream);
}

// 10- and 12-bit frames, little-endian 16-bit samples in the I420 plane order.
extern "C" int savsr_video_gather_yuv420_16(const uint8_t* frames, int n_frames, int h, int w, const int32_t* idx, int n_idx, int colour, int depth,
                                            float* out, void* stream) {
    return gather("video_gather_yuv420_16", RULES_16, frames, n_frames, h, w, idx, n_idx, colour, depth, SAVSR_CHROMA_420, out, stream);
}

extern "C" int savsr_video_quantize_yuv420_16(const float* in, int n, int H, int W, int colour, int depth, uint8_t* out, void* stream) {
    return quantize("video_quantize_yuv420_16", RULES_16, in, n, H, W, colour, depth, SAVSR_CHROMA_420, out, stream);
}

// Every (chroma layout, depth).
extern "C" int savsr_video_gather_yuvp(const uint8_t* frames, int n_frames, int h, int w, const int32_t* idx, int n_idx, int colour, int depth,
                                       int chroma, float* out, void* stream) {
    return gather("video_gather_yuvp", RULES_LAYOUT, frames, n_frames, h, w, idx, n_idx, colour, depth, chroma, out, stream);
}

extern "C" int savsr_video_quantize_yuvp(const float* in, int n, int H, int W, int colour, int depth, int chroma, uint8_t* out, void* stream) {
    return quantize("video_quantize_yuvp", RULES_LAYOUT, in, n, H, W, colour, depth, chroma, out, stream);
}

// Every (chroma layout, depth) with the chroma siting (SAVSR_SITING_*): linear chroma reconstruction in, cosited filters out.
extern "C" int savsr_video_gather_yuvs(const uint8_t* frames, int n_frames, int h, int w, const int32_t* idx, int n_idx, int colour, int depth,
                                       int chroma, int siting, float* out, void* stream) {
    return gather_sited("video_gather_yuvs", frames, n_frames, h, w, idx, n_idx, colour, depth, chroma, siting, out, stream);
}

extern "C" int savsr_video_quantize_yuvs(const float* in, int n, int H, int W, int colour, int depth, int chroma, int siting, uint8_t* out,
                                         void* stream) {
    return quantize_sited("video_quantize_yuvs", in, n, H, W, colour, depth, chroma, siting, out, stream);
}

// savsr_video_quantize_yuvs with a dither (SAVSR_DITHER_*): 0 runs its kernels and gives its bytes, 1 the ordered dither of dither.hpp.
extern "C" int savsr_video_quantize_yuvs_d(const float* in, int n, int H, int W, int colour, int depth, int chroma, int siting, int dither,
                                           uint8_t* out, void* stream) {
    if (dither != SAVSR_DITHER_NONE && dither != SAVSR_DITHER_ORDERED) {
        set_error("invalid argument: video_quantize_yuvs_d: dither %d (0 = none, 1 = ordered)", dither);
        return SAVSR_E_ARG;
    }
    return quantize_sited("video_quantize_yuvs_d", in, n, H, W, colour, depth, chroma, siting, out, stream, dither == SAVSR_DITHER_ORDERED);
}
