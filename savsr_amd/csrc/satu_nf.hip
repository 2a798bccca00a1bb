// SATU at any num_feat C (a multiple of 32 up to 128; instantiated for C = 32 and, for cross-checks, C = 64), tail-projected
// 27-plane form: the same algebra as savsr_satu_lr_stage_tail + savsr_satu_hr_tail (satu.hip), written for a generic C as a plain
// tile walk -- no LDS windows, no persistent queue, no launch plans.  The tuned 64-wide kernels of satu.hip stay what a 64-wide
// checkpoint runs.
//
//   P[p] = G(Wt27 Wa sta, soff) + G(Wt27 Wb x, off) + sum_n r_n (Wt27 Wb E_n) (sum_m r_m C_m G(x, off)) + Wt27 b       p < 27
//
// (savsr_arch.py:315-376 followed by the tail conv's channel contraction, :738; Wt27[p = 3 (3 ky + kx) + o][c], rows 27 .. 31 zero.)
//
// LRcat record [64 + C/2] floats per LR pixel, the row order of savsr_satu_lr_stage_tail (at C = 64 the two records are the same):
//   [32 hh, 32 hh + 16)       (Wt27 Wa sta)[p] at r  <->  p = acc_row(r, hh)
//   [32 hh + 16, 32 hh + 32)  (Wt27 Wb x)[p]   same r
//   [64, 64 + C/2)            (C_m x)[j] at (C/8) m + j   (4 experts x C/8 compressed channels)
//
// LR stage: one wave = 32 LR pixels of one row (the MFMA N dimension), a workgroup = Nf<C>::ROWS such rows; the workgroup's x tile
// (rows +- 2, columns +- 2, replicate padding of :297-313 by clamping) sits in LDS.  kernel_conv (1x1, C -> 25C, :226-228) is
// 25 C / 32 GEMM tiles of 32 channels x 32 px x K = C on v_mfma_f32_32x32x16_bf16 with split-bf16 operands (hi*hi + hi*lo + lo*hi, see
// conv_mfma.hip); each tile holds ONE tap of 32 channels, so its LeakyReLU_0.1 and the 5x5 dynamic filter (:297-313) run straight
// from the accumulator registers: the 25C-channel kernel map never leaves them.  The projections are three more MFMA GEMMs in the
// same split form, sta consumed from its accumulators (k order = accumulator order).
// HR stage: one lane per HR pixel, 4 x 64-pixel tiles per workgroup, fp32 FMAs (the expert contraction has K = C/2 per output row).
#include "common.hpp"

namespace savsr {
namespace {

constexpr int NF_TABLE_LDS = 256;       // tables of up to this many entries are read as such, larger ones per pixel (as satu.hip)

template <int C>
struct Nf {
    static_assert(C % 32 == 0 && C >= 32 && C <= 128, "num_feat: a multiple of 32 up to 128");
    static constexpr int NCG = C / 32;                  // 32-channel groups
    static constexpr int NKS = C / 16;                  // MFMA k steps over C
    static constexpr int NCS = C / 2;                   // compressed channels (4 experts x C/8)
    static constexpr int NCT = (NCS + 31) / 32;         // 32-row tiles of the C-stack
    static constexpr int NXT = 1 + NCT;                 // x-side projection tiles: Wt27 Wb | C-stack
    static constexpr int REC = 64 + NCS;                // floats per LRcat record
    static constexpr int ROWS = C <= 32 ? 4 : (C <= 64 ? 2 : 1);   // LR rows (waves) per workgroup: the x tile stays <= 64 KiB up to C = 64
    static constexpr int XR = ROWS + 4, XC = 32 + 4;    // x tile rows / columns incl. the 5x5 halo
    static constexpr int XP = C + 4;                    // floats per pixel in LDS (the +4 keeps b128 reads of 32 lanes conflict-free)
    static constexpr int LDS_BYTES = XR * XC * XP * 4;
};

typedef __bf16 bf16x8_ __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void split8(const f32x4 a, const f32x4 b, bf16x8_& hi, bf16x8_& lo) {
    const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const __bf16 h = (__bf16)v[j];
        hi[j] = h;
        lo[j] = (__bf16)(v[j] - (float)h);
    }
}

__device__ __forceinline__ f32x16 mma3_(const bf16x8_ ah, const bf16x8_ al, const bf16x8_ bh, const bf16x8_ bl, f32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
}

// hi / lo A fragments of 512-element group g of a split-bf16 image ([group][part][64 lanes][8])
__device__ __forceinline__ void afrag(const unsigned short* img, int g, int lane, bf16x8_& hi, bf16x8_& lo) {
    const uint4* p = reinterpret_cast<const uint4*>(img + (size_t)g * 1024 + lane * 8);
    hi = __builtin_bit_cast(bf16x8_, p[0]);
    lo = __builtin_bit_cast(bf16x8_, p[64]);
}

struct NfLrParams {
    savsr_satu_nf_weights wt;
    const float* x;
    const float* st;
    int pix, row_px, h, w;
    float* lrcat;
};

template <int C>
__global__ __launch_bounds__(64 * Nf<C>::ROWS) void satu_nf_lr_kernel(const NfLrParams p) {
    using G = Nf<C>;
    extern __shared__ __attribute__((aligned(16))) float xs[];        // [XR][XC][XP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, px = lane & 31;
    const int x0 = blockIdx.x * 32, y0 = blockIdx.y * G::ROWS;
    // ---- x tile with the replicate padding of sta_conv (coordinates clamped into the crop) ----
    constexpr int Q = C / 4;
    for (int e = tid; e < G::XR * G::XC * Q; e += 64 * G::ROWS) {
        const int q = e % Q, pxl = e / Q;
        const int cx = pxl % G::XC, ry = pxl / G::XC;
        const int sy = min(max(y0 + ry - 2, 0), p.h - 1), sx = min(max(x0 + cx - 2, 0), p.w - 1);
        *reinterpret_cast<f32x4*>(xs + pxl * G::XP + 4 * q) =
            *reinterpret_cast<const f32x4*>(p.x + ((long long)sy * p.row_px + sx) * p.pix + 4 * q);
    }
    __syncthreads();
    const int y = y0 + wave;
    if (y >= p.h) return;                                              // (wave-uniform; no barrier follows)
    const int xg = x0 + px;
    const bool valid = xg < p.w;
    const int xc = valid ? xg : p.w - 1;                               // lanes beyond the row compute a real pixel, store nothing
    const unsigned short* kimg = static_cast<const unsigned short*>(p.wt.kconv_w);
    const unsigned short* pimg = static_cast<const unsigned short*>(p.wt.proj_w);

    // ---- B operand of kernel_conv: st at the lane's pixel, k = 16 ks + 8 half + j ----
    bf16x8_ sth[G::NKS], stl[G::NKS];
    {
        const float* s = p.st + ((long long)y * p.row_px + xc) * p.pix + 8 * half;
#pragma unroll
        for (int ks = 0; ks < G::NKS; ++ks)
            split8(*reinterpret_cast<const f32x4*>(s + 16 * ks), *reinterpret_cast<const f32x4*>(s + 16 * ks + 4), sth[ks], stl[ks]);
    }
    f32x16 pa;                                                         // Wt27 Wa sta, accumulated over the channel groups
#pragma unroll
    for (int r = 0; r < 16; ++r) pa[r] = 0.f;
    const float* xrow = xs + (wave * G::XC + px) * G::XP;              // (tap (0, 0) of the lane's pixel)
#pragma unroll 1
    for (int cg = 0; cg < G::NCG; ++cg) {
        f32x16 sta;
#pragma unroll
        for (int r = 0; r < 16; ++r) sta[r] = 0.f;
#pragma unroll 5
        for (int tap = 0; tap < 25; ++tap) {
            // K[25 c + tap] for c = 32 cg + acc_row(r, half), bias first (kconv_b is [tap][C])
            const f32x4* kb = reinterpret_cast<const f32x4*>(p.wt.kconv_b + tap * C + 32 * cg + 4 * half);
            f32x16 acc;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 b = kb[2 * g];
                acc[4 * g] = b[0]; acc[4 * g + 1] = b[1]; acc[4 * g + 2] = b[2]; acc[4 * g + 3] = b[3];
            }
#pragma unroll
            for (int ks = 0; ks < G::NKS; ++ks) {
                bf16x8_ ah, al;
                afrag(kimg, (tap * G::NCG + cg) * G::NKS + ks, lane, ah, al);
                acc = mma3_(ah, al, sth[ks], stl[ks], acc);
            }
            // LeakyReLU_0.1 (:227) times x at (y + ky - 2, x + kx - 2), channels 32 cg + 8 g + 4 half + i  (:297-313)
            const int ky = tap / 5, kx = tap - 5 * ky;
            const float* xv = xrow + (ky * G::XC + kx) * G::XP + 32 * cg + 4 * half;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(xv + 8 * g);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float k = acc[4 * g + i];
                    sta[4 * g + i] = fmaf(k > 0.f ? k : 0.1f * k, v[i], sta[4 * g + i]);
                }
            }
        }
        // Wt27 Wa sta: B operand = sta's accumulator registers 8 s .. 8 s + 7 (k step 2 cg + s)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bf16x8_ bh, bl, ah, al;
            split8(f32x4{sta[8 * s], sta[8 * s + 1], sta[8 * s + 2], sta[8 * s + 3]},
                   f32x4{sta[8 * s + 4], sta[8 * s + 5], sta[8 * s + 6], sta[8 * s + 7]}, bh, bl);
            afrag(pimg, 2 * cg + s, lane, ah, al);
            pa = mma3_(ah, al, bh, bl, pa);
        }
    }
    float* rec = p.lrcat + ((long long)y * p.w + xc) * G::REC;
    if (valid) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<f32x4*>(rec + 32 * half + 4 * g) = f32x4{pa[4 * g], pa[4 * g + 1], pa[4 * g + 2], pa[4 * g + 3]};
    }
    // ---- x-side projections: tile 0 = Wt27 Wb, tiles 1 .. NCT = the C-stack (rows (C/8) m + j) ----
    bf16x8_ xh[G::NKS], xl[G::NKS];
    {
        const float* xv = xrow + (2 * G::XC + 2) * G::XP + 8 * half;   // the lane's own pixel (tap (2, 2))
#pragma unroll
        for (int ks = 0; ks < G::NKS; ++ks)
            split8(*reinterpret_cast<const f32x4*>(xv + 16 * ks), *reinterpret_cast<const f32x4*>(xv + 16 * ks + 4), xh[ks], xl[ks]);
    }
#pragma unroll
    for (int t = 0; t < G::NXT; ++t) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < G::NKS; ++ks) {
            bf16x8_ ah, al;
            afrag(pimg, G::NKS + t * G::NKS + ks, lane, ah, al);
            acc = mma3_(ah, al, xh[ks], xl[ks], acc);
        }
        if (!valid) continue;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 v = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
            if (t == 0) {
                *reinterpret_cast<f32x4*>(rec + 32 * half + 16 + 4 * g) = v;
            } else {
                const int m = 32 * (t - 1) + 8 * g + 4 * half;             // rows m .. m + 3 of the C-stack
                if (m < G::NCS) *reinterpret_cast<f32x4*>(rec + 64 + m) = v;
            }
        }
    }
}

struct NfHrParams {
    savsr_satu_nf_weights wt;
    const float* lrcat;
    int h, w;
    const float* table;          // raw phase table (n_table <= NF_TABLE_LDS) ...
    int n_uw;
    const int* idx_h;
    const int* idx_w;
    const float* ptab;           // ... or the per-pixel expansion, offsets normalised (otherwise)
    const float* gyn;
    const float* gxn;
    int H, W;
    float* out;
    long long out_plane;
};

struct NfTaps {
    int y0, x0, dy, dx;
    float wgt[4];                // nw, ne, sw, se; 0 outside the image (zeros padding)
};

// grid_sample (bilinear, zeros padding, align_corners=True) of :262-295 at normalised base (gxn, gyn) + offset (onx, ony).
// An out-of-image tap has weight 0 and a coordinate clamped into the image, so it reads finite data.
__device__ __forceinline__ NfTaps nf_taps(float gxn, float gyn, float onx, float ony, int h, int w) {
    const float fw1 = (float)(w - 1), fh1 = (float)(h - 1);
    float ix = ((gxn + onx + 1.f) / 2.f) * fw1;
    float iy = ((gyn + ony + 1.f) / 2.f) * fh1;
    ix = fminf(fmaxf(ix, -2.f), (float)w + 1.f);
    iy = fminf(fmaxf(iy, -2.f), (float)h + 1.f);
    const float xw = floorf(ix), yn = floorf(iy);
    const float lx = ix - xw, ly = iy - yn;
    const int x0 = (int)xw, y0 = (int)yn;
    const float wx0 = (unsigned)x0 < (unsigned)w ? 1.f - lx : 0.f, wx1 = (unsigned)(x0 + 1) < (unsigned)w ? lx : 0.f;
    const float wy0 = (unsigned)y0 < (unsigned)h ? 1.f - ly : 0.f, wy1 = (unsigned)(y0 + 1) < (unsigned)h ? ly : 0.f;
    NfTaps t;
    t.x0 = min(max(x0, 0), w - 1);
    t.y0 = min(max(y0, 0), h - 1);
    t.dx = min(max(x0 + 1, 0), w - 1) - t.x0;
    t.dy = min(max(y0 + 1, 0), h - 1) - t.y0;
    t.wgt[0] = wy0 * wx0; t.wgt[1] = wy0 * wx1; t.wgt[2] = wy1 * wx0; t.wgt[3] = wy1 * wx1;
    return t;
}

// P[acc_row(r, hh)] += wgt * rec[32 hh + base + r] for the NP rows that are computed (27, or 9 nch: rows 9 nch .. 31 of Wt are zero)
template <int NP>
__device__ __forceinline__ void nf_gather_rows(float (&P)[NP], const float* rec, int base, float wgt) {
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (8 * g + 4 * hh >= NP) continue;
            const f32x4 v = *reinterpret_cast<const f32x4*>(rec + 32 * hh + base + 4 * g);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (8 * g + 4 * hh + i < NP) P[8 * g + 4 * hh + i] = fmaf(wgt, v[i], P[8 * g + 4 * hh + i]);
        }
}

// NP: planes computed and written -- 27 (savsr_satu_nf_hr), or the 9 nch live ones of an nch-channel checkpoint (savsr_satu_nf_hr_planes).
// Every plane's arithmetic is independent of NP: plane p of an NP-plane launch equals plane p of the 27-plane one bit for bit.
template <int C, int NP>
__global__ __launch_bounds__(256) void satu_nf_hr_kernel(const NfHrParams p) {
    using G = Nf<C>;
    constexpr int J = C / 8;                                           // compressed channels per expert
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int X = blockIdx.x * 64 + lane, Y = blockIdx.y * 4 + wave;
    if (Y >= p.H) return;
    const bool valid = X < p.W;
    const int Xc = valid ? X : p.W - 1;
    f32x4 rr, oo;
    if (p.ptab) {
        const f32x4* te = reinterpret_cast<const f32x4*>(p.ptab + ((long long)Y * p.W + Xc) * SAVSR_SATU_TABLE);
        rr = te[0];
        oo = te[1];
    } else {
        const f32x4* te = reinterpret_cast<const f32x4*>(p.table + ((long long)p.idx_h[Y] * p.n_uw + p.idx_w[Xc]) * SAVSR_SATU_TABLE);
        rr = te[0];
        oo = te[1];
        const float fw1 = (float)(p.w - 1), fh1 = (float)(p.h - 1);   // normalised as the reference does per pixel (:285-287)
        oo[0] = (oo[0] * 2.f) / fw1; oo[1] = (oo[1] * 2.f) / fh1; oo[2] = (oo[2] * 2.f) / fw1; oo[3] = (oo[3] * 2.f) / fh1;
    }
    const float gxn = p.gxn[Xc], gyn = p.gyn[Y];
    const NfTaps to = nf_taps(gxn, gyn, oo[0], oo[1], p.h, p.w);
    const NfTaps ts = nf_taps(gxn, gyn, oo[2], oo[3], p.h, p.w);
    float P[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) P[q] = p.wt.fusion_b[q];
    float z[J];
#pragma unroll
    for (int j = 0; j < J; ++j) z[j] = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {                                      // G(Wt27 Wb x, off) and z = sum_m r_m (C_m G(x, off))
        const float* rec = p.lrcat + ((long long)(to.y0 + (k >> 1) * to.dy) * p.w + to.x0 + (k & 1) * to.dx) * G::REC;
        const float wk = to.wgt[k];
        nf_gather_rows(P, rec, 16, wk);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float wr = wk * rr[m];
#pragma unroll
            for (int j4 = 0; j4 < J / 4; ++j4) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(rec + 64 + J * m + 4 * j4);
#pragma unroll
                for (int i = 0; i < 4; ++i) z[4 * j4 + i] = fmaf(wr, v[i], z[4 * j4 + i]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {                                      // G(Wt27 Wa sta, soff)
        const float* rec = p.lrcat + ((long long)(ts.y0 + (k >> 1) * ts.dy) * p.w + ts.x0 + (k & 1) * ts.dx) * G::REC;
        nf_gather_rows(P, rec, 0, ts.wgt[k]);
    }
    // sum_n r_n (Wt27 Wb E_n) z: wbe is [4 n][J j][32 p], the same for every lane (scalar loads)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const float u = rr[n] * z[j];
            const float* we = p.wt.wbe + (n * J + j) * 32;
#pragma unroll
            for (int q = 0; q < NP; ++q) P[q] = fmaf(we[q], u, P[q]);
        }
    if (!valid) return;
    float* o = p.out + (long long)Y * p.W + X;
#pragma unroll
    for (int q = 0; q < NP; ++q) o[q * p.out_plane] = P[q];
}

// What is left of savsr_arch.py:738-739 for an nch-channel tail (nch = num_in_ch in 1 .. 3) after an NP = 9 nch HR stage:
//     out[o][Y][X] = tail_b[o] + sum_{ky,kx} P[nch (3 ky + kx) + o][Y + ky - 1][X + kx - 1]  (zero outside)  + bilinear(center[o])
// One thread = one pixel of one output channel (grid z = nch), summed in savsr_tail_gather's order (ky, then kx) with the residual's
// roundings written out (lerp_fma): at nch = 3 the two agree bit for bit.
__device__ __forceinline__ void nf_bil_src(int dst, float scale, int in_size, int& i0, int& i1, float& l1) {
    float s = scale * ((float)dst + 0.5f) - 0.5f;                      // area_pixel_compute_source_index (F.interpolate, align_corners=False)
    if (s < 0.f) s = 0.f;
    i0 = (int)s;
    if (i0 > in_size - 1) i0 = in_size - 1;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l1 = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
}

__global__ __launch_bounds__(256) void tail_gather_nch_kernel(const float* __restrict__ P, long long PP, int nch, const float* __restrict__ bias,
                                                              const float* __restrict__ center, int h, int w, int H, int W, float* __restrict__ out) {
    const int X = blockIdx.x * 64 + (threadIdx.x & 63);
    const int Y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int o = blockIdx.z;
    if (X >= W || Y >= H) return;
    float acc = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int yy = Y + ky - 1;
        if (yy < 0 || yy >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int xx = X + kx - 1;
            if (xx >= 0 && xx < W) acc += P[(long long)(nch * (3 * ky + kx) + o) * PP + (long long)yy * W + xx];
        }
    }
    int y0, y1, x0, x1;
    float ly, lx;
    nf_bil_src(Y, (float)h / (float)H, h, y0, y1, ly);
    nf_bil_src(X, (float)w / (float)W, w, x0, x1, lx);
    const float* c = center + (long long)o * h * w;
    const float top = lerp_fma(lx, c[y0 * w + x0], c[y0 * w + x1]);
    const float bot = lerp_fma(lx, c[y1 * w + x0], c[y1 * w + x1]);
    out[(long long)o * H * W + (long long)Y * W + X] = (acc + bias[o]) + lerp_fma(ly, top, bot);
}

template <int C>
int nf_lr(const savsr_satu_nf_weights* wt, const float* x, const float* st, int32_t pix, int32_t row_px, int h, int w, float* lrcat,
          void* stream) {
    using G = Nf<C>;
    if (pix < C || (pix & 3) || row_px < w) return fail_arg("satu_nf_lr_stage: strides (pix >= C, a multiple of 4; row_px >= w)");
    NfLrParams p;
    p.wt = *wt; p.x = x; p.st = st; p.pix = pix; p.row_px = row_px; p.h = h; p.w = w; p.lrcat = lrcat;
    if (G::LDS_BYTES > 64 * 1024) {
        if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(&satu_nf_lr_kernel<C>), G::LDS_BYTES, "satu_nf_lr_stage")) return rc;
    }
    dim3 grid((w + 31) / 32, (h + G::ROWS - 1) / G::ROWS);
    hipLaunchKernelGGL((satu_nf_lr_kernel<C>), grid, dim3(64 * G::ROWS), G::LDS_BYTES, static_cast<hipStream_t>(stream), p);
    return check_launch("satu_nf_lr_kernel");
}

template <int C, int NP = 27>
int nf_hr(const NfHrParams& p, void* stream) {
    dim3 grid((p.W + 63) / 64, (p.H + 3) / 4);
    hipLaunchKernelGGL((satu_nf_hr_kernel<C, NP>), grid, dim3(256), 0, static_cast<hipStream_t>(stream), p);
    return check_launch("satu_nf_hr_kernel");
}

bool nf_weights_ok(const savsr_satu_nf_weights* w) {
    return w && w->kconv_w && w->kconv_b && w->proj_w && w->wbe && w->fusion_b;
}

bool aligned16(const void* a) { return (reinterpret_cast<uintptr_t>(a) & 15) == 0; }

}  // namespace
}  // namespace savsr

using namespace savsr;

extern "C" int savsr_satu_nf_lrcat_floats(int C) {
    return (C == 32 || C == 64) ? 64 + C / 2 : -1;
}

extern "C" int savsr_satu_nf_lr_stage(const savsr_satu_nf_weights* wt, const float* x, const float* st, int32_t pix, int32_t row_px, int h, int w,
                                      float* lrcat, void* stream) {
    if (!nf_weights_ok(wt) || !x || !st || !lrcat) return fail_arg("satu_nf_lr_stage: null pointer");
    if (savsr_satu_nf_lrcat_floats(wt->C) < 0) return fail_arg("satu_nf_lr_stage: num_feat C (built for 32 and 64)");
    if (h < 1 || w < 1) return fail_arg("satu_nf_lr_stage: shape");
    if (!aligned16(x) || !aligned16(st) || !aligned16(lrcat) || !aligned16(wt->kconv_w) || !aligned16(wt->kconv_b) || !aligned16(wt->proj_w)) {
        set_error("satu_nf_lr_stage: x / st / lrcat / kconv_w / kconv_b / proj_w must be 16-byte aligned");
        return SAVSR_E_ALIGN;
    }
    if (wt->C == 32) return nf_lr<32>(wt, x, st, pix, row_px, h, w, lrcat, stream);
    return nf_lr<64>(wt, x, st, pix, row_px, h, w, lrcat, stream);
}

extern "C" int savsr_satu_nf_hr(const savsr_satu_nf_weights* wt, const float* lrcat, int h, int w, const float* table, int n_uh, int n_uw,
                                const int32_t* idx_h, const int32_t* idx_w, const float* ptab, const float* gyn, const float* gxn, int H, int W,
                                float* out, int64_t out_plane, void* stream) {
    return savsr_satu_nf_hr_planes(wt, lrcat, h, w, table, n_uh, n_uw, idx_h, idx_w, ptab, gyn, gxn, H, W, out, out_plane, 27, stream);
}

extern "C" int savsr_satu_nf_hr_planes(const savsr_satu_nf_weights* wt, const float* lrcat, int h, int w, const float* table, int n_uh, int n_uw,
                                       const int32_t* idx_h, const int32_t* idx_w, const float* ptab, const float* gyn, const float* gxn, int H, int W,
                                       float* out, int64_t out_plane, int planes, void* stream) {
    if (planes != 9 && planes != 18 && planes != 27) return fail_arg("satu_nf_hr: planes (9 num_in_ch: 9, 18 or 27)");
    if (!nf_weights_ok(wt) || !lrcat || !table || !idx_h || !idx_w || !gyn || !gxn || !out) return fail_arg("satu_nf_hr: null pointer");
    if (savsr_satu_nf_lrcat_floats(wt->C) < 0) return fail_arg("satu_nf_hr: num_feat C (built for 32 and 64)");
    if (h < 2 || w < 2 || H < 1 || W < 1 || n_uh < 1 || n_uw < 1 || out_plane < (int64_t)H * W)
        return fail_arg("satu_nf_hr: shape (h, w >= 2, out_plane >= H*W required)");
    const bool small = (int64_t)n_uh * n_uw <= NF_TABLE_LDS;
    if (!small && !ptab) return fail_arg("satu_nf_hr: tables of more than 256 entries need the per-pixel expansion (savsr_satu_expand_table)");
    if (!aligned16(lrcat) || !aligned16(table) || (!small && !aligned16(ptab))) {
        set_error("satu_nf_hr: lrcat / table / ptab must be 16-byte aligned");
        return SAVSR_E_ALIGN;
    }
    NfHrParams p;
    p.wt = *wt; p.lrcat = lrcat; p.h = h; p.w = w; p.table = table; p.n_uw = n_uw; p.idx_h = idx_h; p.idx_w = idx_w;
    p.ptab = small ? nullptr : ptab;
    p.gyn = gyn; p.gxn = gxn; p.H = H; p.W = W; p.out = out; p.out_plane = out_plane;
    if (wt->C == 32) return planes == 9 ? nf_hr<32, 9>(p, stream) : planes == 18 ? nf_hr<32, 18>(p, stream) : nf_hr<32, 27>(p, stream);
    return planes == 9 ? nf_hr<64, 9>(p, stream) : planes == 18 ? nf_hr<64, 18>(p, stream) : nf_hr<64, 27>(p, stream);
}

extern "C" int savsr_tail_gather_nch(const float* planes, int64_t p_plane, int nch, const float* b, const float* center, int h, int wd, int H, int W,
                                     float* out, void* stream) {
    if (!planes || !b || !center || !out) return fail_arg("tail_gather_nch: null pointer");
    if (nch < 1 || nch > 3) return fail_arg("tail_gather_nch: nch in 1 .. 3");
    if (h < 1 || wd < 1 || H < 1 || W < 1 || p_plane < (int64_t)H * W) return fail_arg("tail_gather_nch: shape");
    dim3 grid((W + 63) / 64, (H + 3) / 4, nch);
    hipLaunchKernelGGL(tail_gather_nch_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), planes, (long long)p_plane, nch, b, center, h, wd, H, W, out);
    return check_launch("tail_gather_nch_kernel");
}
