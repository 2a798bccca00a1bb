/*
 * savsr_hip.h -- C ABI of libsavsr_hip.so, the MI355X (gfx950) kernel library behind
 * savsr_amd.archs.savsr_arch.SAVSR.forward().
 *
 * The reference (Weepingchestnut/SAVSR) has no native code on this path: every step of
 * lbasicsr/archs/savsr_arch.py is an un-fused ATen call.  Each entry point below therefore cites
 * the reference Python lines whose arithmetic it replaces, not a reference FFI symbol.
 *
 * Conventions:
 *   - plain C, raw DEVICE pointers + explicit int shapes/strides (in floats) + a hipStream_t
 *     passed as void*; no torch types anywhere in this file;
 *   - every call only ENQUEUES work on the caller's stream: no allocation, no host sync, no
 *     global mutable state => re-entrant across streams/threads and hipGraph-capturable;
 *   - return 0 = ok, <0 = invalid argument (SAVSR_E_*), >0 = hipError_t of the failed launch;
 *     the message is available from savsr_last_error() (thread-local);
 *   - LR feature maps are fp32 channel-last ([h][w][C]); the clip, the SATU output and the result
 *     are channel-planar ([C][h][w]);
 *   - output sizes H, W are computed by the CALLER with Python round() so that get_HW
 *     (savsr_arch.py:745-751) stays bit-exact;
 *   - specialisation: the tuned SATU entry points (savsr_satu_*, savsr_tail_*) and savsr_pack_windows are built for the shipped
 *     configuration of the reference constructor (savsr_arch.py:576-589): num_feat = 64, slid_win = 3, num_in_ch = 3.  The
 *     width-generic SATU (savsr_satu_nf_*, ABI 29) serves num_feat = 32 and, since ABI 30, every checkpoint with num_in_ch != 3
 *     (num_in_ch 1 .. 3: the tail's 9 num_in_ch rows live in the 32-row MFMA tile of the LRcat record; savsr_satu_nf_hr_planes +
 *     savsr_tail_gather_nch); savsr_pack_windows_nch (ABI 30) packs windows of any odd slid_win >= 3 with num_in_ch * slid_win <= 32.
 *     The conv / OSConv entry points take any channel counts that are multiples of 16 (32 for 1x1).  Checkpoints with another
 *     num_feat, num_in_ch >= 4 or another window do not run.
 */
#ifndef SAVSR_HIP_H
#define SAVSR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAVSR_ABI_VERSION 55

#define SAVSR_E_ARG   (-1)   /* bad shape / null pointer / unsupported combination */
#define SAVSR_E_ALIGN (-2)   /* pointer or stride alignment requirement violated  */

/* activation codes for the conv epilogue */
#define SAVSR_ACT_NONE    0
#define SAVSR_ACT_RELU    1
#define SAVSR_ACT_LRELU   2   /* slope in savsr_conv_desc.slope (0.2 in propagation, savsr_arch.py:426) */
#define SAVSR_ACT_SIGMOID 3

#define SAVSR_MAX_SRC 5

const char* savsr_version(void);
const char* savsr_last_error(void);
int savsr_abi_version(void);
/* One-time, per DEVICE (the current one), not a stream operation: sets the > 64 KiB dynamic-LDS attribute of every kernel of
 * the library, which the launch entry points otherwise do lazily on a kernel's first use.  Optional -- a caller that records
 * the launches into a hipGraph calls it before the capture so that no attribute call falls inside it.  Idempotent, thread-safe. */
int savsr_prepare_device(void);
/* First 16 hex digits of the sha256 over the kernel sources, headers and compile flags this library was built from (build.sh):
 * lets a measurement file name the build it was taken on (profiles/satu_traffic.json; bench.py drops `traffic` when it differs). */
const char* savsr_source_hash(void);
const char* savsr_source_hash_satu(void);     /* the same over the SATU + tail kernel sources only (satu.hip, tail.hip, common.hpp) */
/* Measurement aid (bench.py `clock_mhz`): ONE wave spins through `windows` (1 .. 64) consecutive windows of `window_ticks` ticks of the
 * 100 MHz s_memrealtime counter each and writes out[2 i] = s_memtime delta (shader cycles), out[2 i + 1] = s_memrealtime delta of window i:
 * shader clock = out[2 i] / out[2 i + 1] x 100 MHz (MI355X_MICROARCH.md, DVFS give-back item 6).  Launched on a side stream beside other
 * work it reads the clock of the CU it sits on while that work runs (one wave with s_sleep in its loop; no LDS, co-resides with any
 * workgroup).  window_ticks x windows <= 10^8 (1 s). */
int savsr_clock_probe(int64_t* out, int window_ticks, int windows, void* stream);

/* ------------------------------------------------------------------------------------------
 * Feature-map layout: every LR-resolution feature map is CHANNEL-LAST fp32, [h][w][C], addressed
 * as base + (y*w + x)*pix + c where `pix` (floats between pixels, multiple of 4) may exceed the
 * number of channels used, so a tensor can be read or written as a channel slice of a wider one.
 *
 * Dense conv (3x3 pad 1, or 1x1), stride 1: implicit GEMM on v_mfma_f32_32x32x16_bf16 with
 * split-bf16 ("bf16x3": hi*hi + hi*lo + lo*hi, fp32 accumulate) operands and a fused epilogue.
 * Replaces every nn.Conv2d / F.conv2d on the path:
 *   WindowUnit_l1/l2 convs   savsr_arch.py:429-442,456-462,480-483,488,498
 *   ResidualBlock convs      savsr_arch.py:388-397,402-415  (cat-free: the `torch.cat` inputs
 *                            of :404,:412,:462,:498,:721 are passed as separate sources)
 *   OSConv2d dynamic conv    savsr_arch.py:156-171 (weights produced on device by
 *                            savsr_osconv_weights; gates folded into the weights, :148-149)
 *   OSAdapt mask convs       savsr_arch.py:189-206 (eval BatchNorm folded by the caller)
 *   RCAB / ResidualGroup     savsr_arch.py:541-543,567, conv_last :733, h_win_conv_h :723
 *
 *   y   = act( sum_{src,ci,ky,kx} W[co][ci][ky][kx] * in[ci](y+ky-p, x+kx-p) + bias[co] )
 *   out = y * (mul_px ? mul_px[y*w+x] : 1) + (res1 ? res1[px][co] : 0) + (res2 ? res2_scale*res2[px][co] : 0)
 * Zero padding outside [0,h) x [0,w).  The input channel axis is the concatenation of `nsrc`
 * sources of `src_ch` channels each (src_ch a multiple of 16; of 32 for 1x1).
 * ------------------------------------------------------------------------------------------ */
typedef struct savsr_conv_desc {
    const float* src[SAVSR_MAX_SRC];   /* device pointers (channel offset already applied) */
    int32_t      src_pix[SAVSR_MAX_SRC];   /* floats between pixels of each source */
    int32_t      nsrc;
    int32_t      src_ch;
    int32_t      h, w;
    int32_t      cin;                  /* = nsrc * src_ch */
    int32_t      cout;
    int32_t      ksize;                /* 1 or 3 */
    const void*  wpacked;              /* device; split-bf16 weight image, see savsr_conv_pack_index() */
    const float* bias;                 /* [cout] or NULL */
    int32_t      act;
    float        slope;
    const float* mul_px;               /* [h*w] or NULL                   -- OSAdapt mask, :214 */
    const float* res1; int32_t res1_pix;   /* or NULL */
    const float* res2; int32_t res2_pix;   /* or NULL */
    float        res2_scale;           /* gamma (savsr_arch.py:732)                              */
    float*       out;                  /* channel offset already applied */
    int32_t      out_pix;
    float*       pool;                 /* optional: fused AdaptiveAvgPool2d(1) partials of the stored tensor,
                                          row t (t < savsr_conv_pool_blocks(h, w)) = channel sums of pixel tile t,
                                          written at pool[t * pool_stride + co]; consumers add rows in order */
    int32_t      pool_stride;
    int32_t      algo;                 /* SAVSR_CONV_DIRECT, SAVSR_CONV_DIRECT_THROUGHPUT (tiling only; same results), SAVSR_CONV_WINOGRAD_Y or
                                          SAVSR_CONV_WINOGRAD_Y_THROUGHPUT (tiling only; same results as WINOGRAD_Y) */
} savsr_conv_desc;

#define SAVSR_CONV_DIRECT   0
/* (1 was the Winograd F(2x2, 3x3) experiment of round 2: measured slower, archived under tools/experiments/) */
#define SAVSR_CONV_DIRECT_THROUGHPUT 2   /* the direct kernel, tiled for several launches in flight on different streams: 16-row
                                            tiles from 100 of them up (120 workgroups for a 64 -> 64 conv at 180x320: slower
                                            alone, faster in aggregate -- DESIGN.md 4a); results are bit-identical to DIRECT */

#define SAVSR_CONV_WINOGRAD_Y 3          /* 3x3, cout % 64 == 0: 1-D Winograd F(2,3) along y on the same split-bf16 matrix products (2/3 of the
                                            matrix work; conv_wy.hip).  `wpacked` must then be the Winograd-y image (savsr_conv_wy_pack_index):
                                            U0 = g0, U1 = (g0 + g1 + g2) / 2, U2 = (g0 - g1 + g2) / 2, U3 = g2 over the tap ROWS g_ky, per kx.
                                            Results differ from DIRECT by rounding only (max-abs error ~1.5 x DIRECT's) */
#define SAVSR_CONV_WINOGRAD_Y_THROUGHPUT 4   /* (ABI 28) WINOGRAD_Y for launches with other streams' launches in flight beside them.  The form's
                                            workgroups walk 16-row tiles; when h % 16 leaves at most 8 rows, those rows can go as STRIP tiles
                                            (their 1 / 2 / 4 row pairs side by side over 8 / 4 / 2 column segments per workgroup instead of
                                            one tile per segment with idle waves: 113 instead of 120 tiles per conv and 64 channels at 180
                                            rows).  WINOGRAD_Y takes strips when they save the persistent grid a round of tiles (what a
                                            launch running alone pays for); _THROUGHPUT also whenever at most 2 row pairs are left (the tile
                                            count decides when another launch fills the tail).  Results are bit-identical to WINOGRAD_Y. */

/* Elements PER PART (hi or lo) of the weight image of a (cout, cin, ksize) conv; the bf16 image
 * holds 2x that many 2-byte elements.  -1 for unsupported shapes. */
int64_t savsr_conv_packed_elems(int cout, int cin, int ksize);
/* Position p of W[co][ci][ky*ksize+kx] inside one part.  The image interleaves parts in groups of
 * 512 elements (one (tap, kstep, 32-row tile) MFMA A operand): bf16 index of the hi value is
 * (p/512)*1024 + p%512, of the lo value (p/512)*1024 + 512 + p%512.  An fp32 kernel bank for
 * savsr_osconv_weights stores W at index p directly.  Unaddressed entries must be zero. */
int64_t savsr_conv_pack_index(int cout, int cin, int ksize, int co, int ci, int tap);
/* The Winograd-y image of a 3x3 conv: elements per part (cout % 64 == 0, cin % 16 == 0, else -1) and the position of
 * U[pos][co][ci][kx] (pos = 0..3) inside one part; hi / lo interleaved in groups of 512 exactly as above. */
int64_t savsr_conv_wy_packed_elems(int cout, int cin);
int64_t savsr_conv_wy_pack_index(int cout, int cin, int co, int ci, int pos, int kx);
int savsr_conv_pool_blocks(int h, int w);
int savsr_conv2d(const savsr_conv_desc* d, void* stream);
/* n (1..savsr_conv2d_max_batch() = 24 since ABI 27; 18 in ABI 26, 6 before) independent convs of identical geometry (ksize, nsrc, src_ch, h, w, cout) in ONE launch:
 * e.g. the per-stream convs of a ResidualBlock (savsr_arch.py:402,413) of both propagation directions -- and, since ABI 26 / 27, of up to three / four
 * clips of one (shape, scale) whose launch sequences the caller runs as one (small clips are launch-latency-bound).  More workgroups than CUs, so workgroups run out of phase and the
 * load/store bursts of one overlap the MFMA phases of another. */
int savsr_conv2d_max_batch(void);
/* (ABI 28) Workgroup tiles a savsr_conv2d_batch launch of `nconv` convs walks in the Winograd-y form with `algo` (SAVSR_CONV_WINOGRAD_Y or
 * _THROUGHPUT): nconv x cout / 64 x (16-row x 32-px tiles, the image's last h % 16 <= 8 rows as strip tiles where the algo's rule takes
 * them).  Host arithmetic only -- the plan the launcher applies; -1 for shapes the form does not take. */
int64_t savsr_conv_wy_tile_count(int h, int w, int cout, int nconv, int algo);
int savsr_conv2d_batch(const savsr_conv_desc* descs, int n, void* stream);
/* (ABI 32) The precision mode "fp16" (SAVSR.set_precision): the same descriptors, forms, tiles and batch rules as savsr_conv2d_batch, with
 * fp16 operands -- the activations rounded to fp16 (RNE) in the staging (after the Winograd-y input transform, in fp32), `wpacked` an fp16
 * image: ONE part of savsr_conv_packed_elems / savsr_conv_wy_packed_elems elements holding fp16(W) (fp16(U)) at position p of
 * savsr_conv_pack_index / savsr_conv_wy_pack_index, no hi/lo interleave; unaddressed entries zero.  One v_mfma_f32_32x32x16_f16 per
 * product, fp32 accumulation, the same fp32 epilogue.  The operand range: a magnitude from 65520 on becomes an infinity (65504 .. 65520
 * rounds to 65504) -- the caller checks its weights (and U); the activations are NOT checked, and the two forms differ: the direct form
 * needs |x| < 65520, the Winograd-y form the same of V = x_a + x_b and x_a - x_b for rows one and two apart, so |x| <= 32752 is safe in
 * both.  An infinity reaches exactly the outputs whose receptive field holds it (Winograd-y: the row pair's four input rows x 3 columns)
 * with IEEE classes (+inf, -inf, NaN); every other output, and every other conv of the launch, is unaffected.  The epilogue's effect on
 * such an accumulator, the same on every path of both forms: bias, mask and residuals are IEEE; SAVSR_ACT_NONE, _RELU and _LRELU never
 * make it finite -- a NaN stays a NaN, RELU(+inf) = +inf and RELU(-inf) = -inf, NOT 0 (ReLU is v_max_f32(v, v * 0), and -inf * 0 is a NaN
 * the maximum ignores; LRELU with slope 0 likewise), otherwise LRELU(-inf) = slope * (-inf): -inf, or +inf for a negative slope;
 * SAVSR_ACT_SIGMOID gives exactly 0 for -inf, 1 for +inf and NaN for a NaN.  No finite value is affected: for finite v, ReLU is
 * max(v, 0) up to the sign of a zero (tests/test_gpu_conv_epilogue.py).  No lower limit: operands
 * below 2^-14 are kept as fp16 subnormals (steps of 2^-24, zero below 2^-25) by the staging's conversion and multiplied as such by the
 * matrix cores (tests/test_gpu_conv_range_f16.py, regimes `w_sub` / `x_sub` / `edge`). */
int savsr_conv2d_batch_f16(const savsr_conv_desc* descs, int n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-channel partial sums for the global average pools (AdaptiveAvgPool2d(1),
 * savsr_arch.py:129,146 for OSConv; :515 for RCAN): partial[blk][s*src_ch + c] over `nblk`
 * pixel ranges; consumers add the partials in block order and scale by 1/(h*w).
 * ------------------------------------------------------------------------------------------ */
int savsr_channel_sums(const float* const* src, const int32_t* src_pix, int nsrc, int src_ch, int64_t npx,
                       int nblk, float* partial, void* stream);

/* ------------------------------------------------------------------------------------------
 * OSConv scale routing + ScaleAttention + kernel aggregation (savsr_arch.py:143-163, 91-96, 69-89):
 *   v  = ReLU(L2 ReLU(L1 [1/sh, 1/sw, mean] + c1) + c2)
 *   a  = ReLU(bn_scale * (Wfc v) + bn_shift)            (eval BatchNorm folded by the caller)
 *   ca = sigmoid(Wc a + bc) (cin), fa = sigmoid(Wf a + bf) (cout), sa = sigmoid(Ws a + bs) (9),
 *   ka = softmax(Wk a + bk) (knum)
 *   W''[co][ci][tap] = fa[co] * ca[ci] * sa[tap] * sum_k ka[k] * W[k][co][ci][tap]
 * written as the split-bf16 weight image savsr_conv2d consumes (three launches, no host sync).
 * ------------------------------------------------------------------------------------------ */
typedef struct savsr_osconv_attn_desc {
    int32_t cin, cout, hidden /* A */, knum /* 8 */;
    float   inv_sh, inv_sw;
    const float* partial; int32_t nblk; float inv_n;   /* pooled input: savsr_channel_sums output, 1/(h*w) */
    const float* l1_w; const float* l1_b;    /* [2cin][cin+2], [2cin] */
    const float* l2_w; const float* l2_b;    /* [cin][2cin],   [cin]  */
    const float* fc_w;                       /* [A][cin] */
    const float* bn_scale; const float* bn_shift; /* [A] */
    const float* ch_w; const float* ch_b;    /* [cin][A],  [cin]  */
    const float* fl_w; const float* fl_b;    /* [cout][A], [cout] */
    const float* sp_w; const float* sp_b;    /* [9][A],    [9]    */
    const float* kn_w; const float* kn_b;    /* [knum][A], [knum] */
    float* v1; float* v2;                    /* scratch [2cin], [cin] */
    const float* bank;                       /* [knum][packed_elems] fp32, index = savsr_conv_pack_index */
    int64_t nunits;                          /* packed_elems / 8 */
    void*  wimg_out;                         /* split-bf16 weight image, 2 * packed_elems * 2 bytes */
    float* att;                              /* optional [cin + cout + 9 + knum] = ca | fa | sa | ka */
    int32_t wy;                              /* != 0: wimg_out receives the Winograd-y image (savsr_conv_wy_pack_index order, 4/3 of the direct size;
                                                cout % 64 == 0) for a conv launched with algo SAVSR_CONV_WINOGRAD_Y: the spatial gate sa[ky, kx] is
                                                applied per tap, then the F(2,3) weight transform over ky */
    int32_t fused;                           /* != 0: ONE launch -- every aggregation workgroup runs the scale routing (pooled mean, layers 1 and 2) itself
                                                instead of two launches in front of it; v2 comes out bit-identical (v1 is not written).  Measured SLOWER
                                                than the three launches on MI355X; the engine leaves it off */
} savsr_osconv_attn_desc;
int savsr_osconv_weights(const savsr_osconv_attn_desc* d, void* stream);
/* n (1..savsr_osconv_weights_max_batch() = 8 since ABI 27; 6 before) independent OSConvs of identical cin / cout / hidden / knum in one set of
 * launches (the two propagation directions of a ResidualBlock pair, savsr_arch.py:399-415, x up to four clips of a batched launch sequence). */
int savsr_osconv_weights_max_batch(void);     /* 8 */
int savsr_osconv_weights_batch(const savsr_osconv_attn_desc* descs, int n, void* stream);
/* (ABI 32) The same, with wimg_out receiving the fp16 image savsr_conv2d_batch_f16 consumes: W'' (U) of the same fp32 gates computed in float64,
 * rounded to fp32 and then to fp16 (RNE; within one fp16 step of the exact value at any bank scale, subnormals kept), one part (half
 * the bytes of the split image; the same buffer may serve both). */
int savsr_osconv_weights_batch_f16(const savsr_osconv_attn_desc* descs, int n, void* stream);

/* RCAN ChannelAttention gate (savsr_arch.py:514-520): gate = sigmoid(W2 ReLU(W1 mean + b1) + b2) */
int savsr_se_gate(const float* partial, int nblk, float inv_n, const float* w1, const float* b1,
                  const float* w2, const float* b2, int c, int cmid, float* gate, void* stream);
/* out[px][c] = r[px][c] * gate[c] + x[px][c]   (savsr_arch.py:524,548-549); contiguous [npx][c] */
int savsr_scale_residual(const float* r, const float* gate, const float* x, float* out, int c, int64_t npx, void* stream);
/* the two above in ONE launch (what SAVSR.forward runs, 32 x per frame): every workgroup re-evaluates the gate from the pooled
 * partial sums, then out = r * gate + x.  Bit-identical to savsr_se_gate followed by savsr_scale_residual. */
int savsr_se_scale_residual(const float* partial, int nblk, float inv_n, const float* w1, const float* b1,
                            const float* w2, const float* b2, int c, int cmid,
                            const float* r, const float* x, float* out, int64_t npx, void* stream);
/* The same for `nclip` clips of a batched launch sequence in ONE launch (ABI 26): clip b's partial / r / x / out lie b * the given byte strides
 * (multiples of 16) behind clip 0's; per clip bit-identical to savsr_se_scale_residual. */
int savsr_se_scale_residual_batch(const float* partial, int nblk, float inv_n, const float* w1, const float* b1,
                                  const float* w2, const float* b2, int c, int cmid, const float* r, const float* x, float* out,
                                  int64_t npx, int nclip, int64_t partial_stride, int64_t r_stride, int64_t x_stride, int64_t out_stride, void* stream);

/* (ABI 34) The RCAB (savsr_arch.py:527-549) with the SE gate folded into conv.2's weights.  The gate needs the global mean of conv.2's
 * output, and the mean of a zero-padded 3x3 conv's output is a function of its input r1 = ReLU(conv.0(x)):
 *   mean r2[co] = b[co] + (1/n) sum W[co][ci][ky][kx] S[ci][ky][kx],  S = r1[ci] summed over the pixels tap (ky, kx) sees = the channel's
 *   total (partial: conv.0's pool partials, [nblk][c]) less one border row and / or column, plus the corner both took away (read from r1,
 *   [h][w][pix] channel-last).
 * a [cmid][c * 9] = w1 W and cz [cmid] = w1 b + b1 are the gate's first layer composed with the conv on the host; w2 [c][cmid], b2 [c].
 * Per clip:  z = ReLU(a S * inv_n + cz),  g = sigmoid(w2 z + b2)  -> gate_out [c];  bias_out [c] = g * bias;  wimg_out = the weight image
 * of g[co] * master: master is ONE fp32 part in the element order of savsr_conv_pack_index (wy == 0) or savsr_conv_wy_pack_index (wy != 0,
 * c % 64 == 0: the transform U of W rounded to fp32), written as the split-bf16 image (hi, lo) or, f16 != 0, rounded once to fp16 -- what
 * savsr_conv2d_batch(_f16) takes as `wpacked` with `bias_out` as bias and res1 = x:  out = x + g (.) conv.2(r1).
 * c in {16, 32, 64}, cmid <= 16.  Clip b's partial / r1 / wimg_out / bias_out / gate_out lie b * the given byte strides (multiples of 16)
 * behind clip 0's.  Every summation order is fixed: the same bits in every workgroup, for any clip count and on any stream. */
int savsr_rcab_gate_weights_batch(const float* partial, int nblk, float inv_n, const float* r1, int h, int w, int pix,
                                  const float* a, const float* cz, const float* w2, const float* b2, int c, int cmid,
                                  const float* master, const float* bias, int wy, int f16, void* wimg_out, float* bias_out, float* gate_out,
                                  int nclip, int64_t partial_stride, int64_t r1_stride, int64_t wimg_stride, int64_t bias_stride,
                                  int64_t gate_stride, void* stream);

/* nn.AvgPool2d(2) (savsr_arch.py:193): [h][w][c] -> [h/2][w/2][c], h and w even, contiguous. */
int savsr_avgpool2(const float* in, float* out, int c, int h, int w, void* stream);
/* nn.Upsample(scale_factor=2, bilinear, align_corners=False) (savsr_arch.py:202), channel-last. */
int savsr_upsample2x(const float* in, float* out, int c, int h, int w, void* stream);
/* WindowUnit_l1 input windows (savsr_arch.py:448-454, :661-668) with SAVSR.pad_spatial's reflect
 * padding (:670-690) folded in.  lq: [T][3][h][w] planar -> out: [T-2][hp][wp][16] channel-last,
 * channels = frame t | frame t-1 | frame t+1 | 7 zeros for window centre t = position + 1. */
int savsr_pack_windows(const float* lq, float* out, int T, int h, int w, int hp, int wp, void* stream);
/* (ABI 30) The same for nch = num_in_ch channels and an odd window of sw >= 3 frames, nch * sw <= 32 (savsr_arch.py:448-454 with
 * c = nch, win_size = sw; :661-668; :670-690).  lq: [T][nch][h][w] planar -> out: [T-sw+1][hp][wp][RW] channel-last, RW = 16 if
 * nch * sw <= 16, else 32; channels = frame t | the sw-1 support frames in ascending time order (sup_index, :450-454), nch each |
 * zeros, for window centre t = position + sw/2.  At nch = 3, sw = 3 the output equals savsr_pack_windows'. */
int savsr_pack_windows_nch(const float* lq, float* out, int T, int nch, int sw, int h, int w, int hp, int wp, void* stream);

/* ------------------------------------------------------------------------------------------
 * SATU = STAUpsample.forward (savsr_arch.py:315-376), restructured:
 *   out = G(Wa sta, soff) + G(Wb x, off) + sum_n r_n (Wb E_n) (sum_m r_m C_m G(x, off)) + b
 * in three launches:
 *   savsr_satu_phase_table : coordinate MLP (:344-350) on the DISTINCT (coor_h, coor_w) values
 *   savsr_satu_expand_table: that table per HR pixel (both: once per size / scale / weights, not per frame)
 *   savsr_satu_lr_stage    : kernel_conv + LeakyReLU(0.1) + sta_conv (:226-228,297-313,319-320)
 *                            and the three LR-side projections -> LRcat [h][w][160]
 *   savsr_satu_hr_upsample : bilinear gathers (:262-295), expert mixing (:353-370), fusion (:374)
 * ------------------------------------------------------------------------------------------ */
#define SAVSR_SATU_C      64
#define SAVSR_SATU_LRCAT  160
#define SAVSR_SATU_TABLE  8    /* r0 r1 r2 r3 off_x off_y soff_x soff_y */
#define SAVSR_SATU_LRCAT_TAIL 96 /* LRcat record of the tail-projected form (savsr_satu_*_tail) */
#define SAVSR_TAIL_PLANES 27     /* 9 taps x 3 colours */

typedef struct savsr_satu_weights {      /* all device pointers; packed by the caller */
    const float* body0_w; const float* body0_b;   /* [64][4], [64]   savsr_arch.py:245 */
    const float* body2_w; const float* body2_b;   /* [64 in][64 out] (transposed), [64]  :247 */
    const float* head_w;  const float* head_b;    /* [8][64], [8]: routing(4) | offset(2) | st_offset(2)  :252,256,257 */
    const void*  kconv_w; const float* kconv_b;   /* split-bf16 image [25][2][4 ks][part][64 lanes][8], fp32 [25][64]  :227 */
    const void*  proj_w;                          /* split-bf16 image of the LR projections (Wa | Wb | C-stack) */
    const void*  wbe_w;                           /* split-bf16 image of (Wb E_n): [2 t][2 ks][part][64 lanes][8] */
    const float* fusion_b;                        /* [64] :260 */
} savsr_satu_weights;

/* table[uh][uw][8] for uh < n_uh, uw < n_uw.  uniq_ch/uniq_cw are the distinct fp32 values of
 * coor_h/coor_w (savsr_arch.py:331-333) computed by the caller; inv_sw, inv_sh are 1/scale. */
int savsr_satu_phase_table(const savsr_satu_weights* wt, const float* uniq_ch, int n_uh,
                           const float* uniq_cw, int n_uw, float inv_sw, float inv_sh,
                           float* table, void* stream);

/* x, st: channel-last crops [h][w][64] of padded tensors (savsr_arch.py:737): element (y, x, c) at
 * base + (y*row_px + x)*pix + c. */
int savsr_satu_lr_stage(const savsr_satu_weights* wt, const float* x, const float* st,
                        int32_t pix, int32_t row_px, int h, int w, float* lrcat, void* stream);

/* LDS staging plan of the HR stage (a pure performance hint; results never depend on it).  The HR kernel is persistent:
 * its workgroups walk tiles of tile_rows x (32 * tile_cols32) HR pixels and, for each, stage an lr_rows x lr_cols window of
 * LRcat records whose origin is the tile's base sampling coordinate + (off_min_x, off_min_y), double-buffered (the next tile's
 * window arrives by LDS-DMA while the current tile is computed).  Waves whose taps leave the window gather from global
 * memory instead.  NULL = 8 x 32 tiles without a window.  tile_rows must be a multiple of 4.  The LDS need is
 * savsr_satu_hr_lds_bytes(form, n_uh * n_uw, tile_rows, tile_cols32, lr_rows, lr_cols) <= 160 KiB (one workgroup per CU). */
typedef struct savsr_satu_tiling {
    int32_t tile_rows, tile_cols32, lr_rows, lr_cols;
    float   off_min_x, off_min_y;
    int32_t table_entries;   /* n_uh * n_uw; informational */
    float   step_x, step_y;  /* LR pixels per HR pixel (1 / scale_w, 1 / scale_h) for the window origin; <= 0: w / W, h / H */
    int32_t variant;         /* wave split of the workgroup, 0 .. savsr_satu_hr_variants() - 1 (0: 8 compute + 4 producer waves; 1, tail
                                form only: 10 + 6).  Which one is faster depends on size and scale; the caller may time both. */
} savsr_satu_tiling;
int savsr_satu_hr_variants(void);
int64_t savsr_satu_hr_lds_bytes(int tail_form, int n_table, int tile_rows, int tile_cols32, int lr_rows, int lr_cols);
/* resident workgroups per CU the HR kernel is written for (plan tiles so that this many fit 160 KiB of LDS) */
int savsr_satu_hr_occupancy_target(int tail_form);
/* compute waves of an HR workgroup: a tile of tile_rows x tile_cols32 "wave tiles" (one row x 32 pixels) is dealt over them */
int savsr_satu_hr_compute_waves(int variant);
int savsr_satu_hr_rows_per_wave_tile(int tail_form);   /* HR rows one wave tile covers (32 pixels wide) */

/* Per-pixel expansion of the phase table, once per (size, scale, weights): ptab[Y][X][8] = table[idx_h[Y]][idx_w[X]] with the
 * two offset pairs normalised as the reference normalises them per pixel ((off * 2) / (size - 1), savsr_arch.py:285-287).
 * Needed by the HR stage only for tables of more than 256 entries (smaller ones are kept whole in LDS). */
int savsr_satu_expand_table(const float* table, int n_uw, const int32_t* idx_h, const int32_t* idx_w,
                            int h, int w, int H, int W, float* ptab, void* stream);

/* table[n_uh][n_uw][8]: savsr_satu_phase_table's output; idx_h[H], idx_w[W]: index of each row's / column's (coor_h, coor_w)
 * value in it; gxn[W], gyn[H]: normalised base grid coordinates (savsr_arch.py:270-280) computed by the caller in fp32.
 * These four arrays are read in 16-byte groups: 16-byte aligned and READABLE up to the next multiple of 4 elements.
 * ptab: savsr_satu_expand_table's output (may be NULL when n_uh * n_uw <= 256).
 * sched: 16 int32 of device scratch for the kernel's tile queue, ZERO-FILLED ONCE by the caller (the kernel leaves them zero) and
 * not shared by launches that may run concurrently (one per stream); NULL = static tile walk (no scratch, ~10 % slower).
 * out: [64] planes of [H][W], `out_plane` floats apart (>= H*W; a pitch that is not a multiple of a few KiB keeps the
 * 64 planes of one pixel on different HBM channels). */
int savsr_satu_hr_upsample(const savsr_satu_weights* wt, const float* lrcat, int h, int w,
                           const float* table, int n_uh, int n_uw, const int32_t* idx_h, const int32_t* idx_w, const float* ptab,
                           const float* gyn, const float* gxn, int H, int W,
                           const savsr_satu_tiling* tiling, int32_t* sched, float* out, int64_t out_plane, void* stream);

/* ------------------------------------------------------------------------------------------
 * Tail-projected form of SATU + tail = savsr_arch.py:315-376 followed by :738-739, the form SAVSR.forward runs.
 * The tail conv is linear and a bilinear gather commutes with a channel contraction, so the tail's weights, regrouped as
 * Wt27[p = 3 (3 ky + kx) + o][c] (27 rows, padded to 32), are multiplied into every matrix of the stage by the caller:
 *   wt->proj_w   = LR projections (Wt27 Wa | Wt27 Wb | C-stack), wt->wbe_w = (Wt27 Wb E_n), wt->fusion_b = Wt27 b
 *   P[p] = G(Wt27 Wa sta, soff) + G(Wt27 Wb x, off) + sum_n r_n (Wt27 Wb E_n)(sum_m r_m C_m G(x, off)) + Wt27 b
 * savsr_satu_lr_stage_tail -> LRcat [h][w][96]; savsr_satu_hr_tail -> P: [27] planes of [H][W]; savsr_tail_gather adds
 * the nine shifted taps per colour, the tail bias and the bilinear residual of the unpadded centre frame.
 * The [64][H][W] SATU output never exists (236 MB written + re-read per 720x1280 frame in the two-kernel form).
 * Same argument meaning as the standalone entry points above. */
int savsr_satu_lr_stage_tail(const savsr_satu_weights* wt, const float* x, const float* st,
                             int32_t pix, int32_t row_px, int h, int w, float* lrcat, void* stream);
int savsr_satu_hr_tail(const savsr_satu_weights* wt, const float* lrcat, int h, int w,
                       const float* table, int n_uh, int n_uw, const int32_t* idx_h, const int32_t* idx_w, const float* ptab,
                       const float* gyn, const float* gxn, int H, int W,
                       const savsr_satu_tiling* tiling, int32_t* sched, float* out, int64_t out_plane, void* stream);
/* p27: [27] planes of [H][W], p_plane floats apart; center: [3][h][w]; out: [3][H][W] contiguous. */
int savsr_tail_gather(const float* p27, int64_t p_plane, const float* tail_b, const float* center,
                      int h, int w, int H, int W, float* out, void* stream);
/* The ROW-SUMMED tail form.  Same stage, with the rows of Wt27 in the order savsr_satu_hr_tail_q wants them -- the three horizontal
 * taps kx of group g = 3 ky + o at MFMA rows acc_row(3 gi + kx, half), gi = g (half 0) for g < 5, g - 5 (half 1) otherwise, where
 * acc_row(r, half) = 8 (r / 4) + 4 half + r % 4 -- in every tail-form matrix (LR stage included: savsr_satu_lr_stage_tail with those
 * weights).  The HR stage adds the three horizontal taps itself and writes q9: [9] planes Q[g] of [H][W] (q_plane floats apart) plus
 * seam: [H][ceil(W / 32)][2][9] floats (the terms that cross a 32-pixel segment border); savsr_tail_gather_q adds the vertical
 * taps, the seams, tail_b and the bilinear residual.  Results equal the 27-plane form's up to the summation order of the nine taps. */
int savsr_satu_hr_tail_q(const savsr_satu_weights* wt, const float* lrcat, int h, int w,
                         const float* table, int n_uh, int n_uw, const int32_t* idx_h, const int32_t* idx_w, const float* ptab,
                         const float* gyn, const float* gxn, int H, int W, const savsr_satu_tiling* tiling, int32_t* sched,
                         float* q9, int64_t q_plane, float* seam, int64_t seam_floats, void* stream);
int savsr_tail_gather_q(const float* q9, int64_t q_plane, const float* seam, int64_t seam_floats, const float* tail_b, const float* center,
                        int h, int w, int H, int W, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 29) Width-generic SATU, the tail-projected 27-plane form above for num_feat C in {32, 64} (satu_nf.hip; C = 64 only
 * to cross-check the tuned kernels).  Same algebra, same phase table / expanded table (savsr_satu_phase_table,
 * savsr_satu_expand_table: their coordinate MLP does not depend on C) and the same savsr_tail_gather behind it.
 *   savsr_satu_nf_lr_stage: kernel_conv + LeakyReLU(0.1) + sta_conv + the three projections (:226-228, 297-313, 319-320) ->
 *                           LRcat [h][w][64 + C/2]: (Wt27 Wa sta | Wt27 Wb x) in savsr_satu_lr_stage_tail's row order, then the
 *                           C-stack (C_m x)[j] at (C/8) m + j.  The [25 C] kernel map is never written.
 *   savsr_satu_nf_hr      : bilinear gathers at off / soff, expert mixing (K = C/2), -> P: [27] planes of [H][W], out_plane apart.
 * Both only enqueue (no allocation) and are capturable; an unsupported C or shape returns SAVSR_E_ARG.  The HR stage reads `table`
 * when n_uh * n_uw <= 256 and `ptab` otherwise, as savsr_satu_hr_tail does. */
typedef struct savsr_satu_nf_weights {  /* device pointers packed by the caller (savsr_amd/packing.py::_pack_satu_nf) */
    int32_t C;                           /* num_feat */
    int32_t reserved;
    const void*  kconv_w;   /* split-bf16 image [25 tap][C/32 cg][C/16 ks][2 part][64 lanes][8]: row 32 cg + (lane & 31) of tap `tap`,
                               k = 16 ks + 8 (lane >> 5) + j  (:227) */
    const float* kconv_b;   /* [25 tap][C] */
    const void*  proj_w;    /* split-bf16 image: C/16 groups of Wt27 Wa (k = 32 (g / 2) + 16 (g % 2) + 8 (j / 4) + 4 (lane >> 5) + j % 4),
                               then 1 + ceil(C / 64) tiles x C/16 groups of [Wt27 Wb ; C-stack rows zero-padded to 32] (k = 16 ks + 8 (lane >> 5) + j) */
    const float* wbe;       /* fp32 [4 n][C/8 j][32 p]: (Wt27 Wb E_n)[p][j] */
    const float* fusion_b;  /* fp32 [32]: Wt27 b */
} savsr_satu_nf_weights;
int savsr_satu_nf_lrcat_floats(int C);   /* floats per LRcat record, 64 + C/2, for an instantiated C; -1 otherwise (host only) */
int savsr_satu_nf_lr_stage(const savsr_satu_nf_weights* wt, const float* x, const float* st,
                           int32_t pix, int32_t row_px, int h, int w, float* lrcat, void* stream);
int savsr_satu_nf_hr(const savsr_satu_nf_weights* wt, const float* lrcat, int h, int w,
                     const float* table, int n_uh, int n_uw, const int32_t* idx_h, const int32_t* idx_w, const float* ptab,
                     const float* gyn, const float* gxn, int H, int W, float* out, int64_t out_plane, void* stream);
/* (ABI 30) num_in_ch = nch checkpoints: the tail conv (savsr_arch.py:738, 64 -> nch) leaves 9 nch live rows in Wt, row
 * p = nch (3 ky + kx) + o (rows 9 nch .. 31 zero: packing.py::fold_satu_nf).
 *   savsr_satu_nf_hr_planes: savsr_satu_nf_hr computing and writing the first `planes` (9, 18 or 27) planes only; each plane equals
 *                            the 27-plane call's bit for bit, and nothing beyond them is written (at 720x1280, 9 planes instead of 27
 *                            save ~66 MB of writes per frame).  savsr_satu_nf_hr is this entry with planes = 27.
 *   savsr_tail_gather_nch  : the rest of :738-739 for nch output channels: the nine shifted taps of P[nch (3 ky + kx) + o], the tail
 *                            bias and the bilinear residual (F.interpolate, :739) of the unpadded centre frame center [nch][h][w] ->
 *                            out [nch][H][W] contiguous.  At nch = 3 it agrees with savsr_tail_gather to rounding. */
int savsr_satu_nf_hr_planes(const savsr_satu_nf_weights* wt, const float* lrcat, int h, int w,
                            const float* table, int n_uh, int n_uw, const int32_t* idx_h, const int32_t* idx_w, const float* ptab,
                            const float* gyn, const float* gxn, int H, int W, float* out, int64_t out_plane, int planes, void* stream);
int savsr_tail_gather_nch(const float* planes, int64_t p_plane, int nch, const float* tail_b, const float* center,
                          int h, int w, int H, int W, float* out, void* stream);

/* tail conv 3x3 64->3 + bias at HR plus the bilinear residual of the (unpadded) centre frame
 * (savsr_arch.py:738-739).  feat: [64] planes of [H][W], feat_plane floats apart; center: [3][h][w];
 * out: [3][H][W] contiguous. */
int savsr_tail_residual(const float* feat, int64_t feat_plane, const float* tail_w /* [3][64][3][3] */, const float* tail_b,
                        const float* center, int h, int w, int H, int W, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 31) The sequence path's conversions (video.hip; SAVSR.upscale_video).  Not fused into the SATU / tail
 * kernels.  The slot -> frame list `idx` is a HOST array of n_idx int32 (1 .. SAVSR_VIDEO_MAX_SLOTS), copied into the kernel
 * arguments when the call enqueues: nb windows of num_frame frames each, in clip order (generate_frame_indices,
 * lbasicsr/data/data_util.py:63-112).  Every index must lie in [0, n_frames).
 * savsr_video_gather_u8:  frames [n_frames][h][w][c] uint8 (c = 1 .. 3 interleaved channels) -> out [n_idx][c][h][w] fp32, slot k =
 *                         frame idx[k] / 255 -- bit for bit numpy's float32(u8) / 255.0 (read_img_seq / img2tensor, data_util.py:29-60)
 *                         through a 256-entry table the compiler evaluates.  One pass: each byte is read once per slot that names it.
 * savsr_video_gather_f32: frames [n_frames][c][h][w] fp32 -> out [n_idx][c][h][w], a copy of frame idx[k] per slot.
 * savsr_video_quantize_u8: in [n][c][H][W] fp32 contiguous -> out [n][H][W][c] uint8: clamp(0, 1), x 255.0f, rintf (round half to
 *                         even) -- tensor2img(x, rgb2bgr=False), lbasicsr/utils/img_util.py:66-90.  16-byte stores when H * W % 16 == 0
 *                         and both pointers are 16-byte aligned. */
#define SAVSR_VIDEO_MAX_SLOTS 64
int savsr_video_gather_u8(const uint8_t* frames, int n_frames, int c, int h, int w, const int32_t* idx, int n_idx, float* out, void* stream);
int savsr_video_gather_f32(const float* frames, int n_frames, int c, int h, int w, const int32_t* idx, int n_idx, float* out, void* stream);
int savsr_video_quantize_u8(const float* in, int n, int c, int H, int W, uint8_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 35) Planar YUV 4:2:0 on either side of the sequence path (yuv.hip; SAVSR.upscale_video with pixel_format / out = "i420", the
 * Y4M path of python -m savsr_amd.upscale).  An I420 frame of an h x w picture is h * w Y bytes, then ch * cw U
 * (Cb) bytes, then ch * cw V (Cr) bytes, ch = (h + 1) / 2, cw = (w + 1) / 2; frames lie back to back.  Colour: ITU-R BT.601, limited
 * range, the constants of rgb2ycbcr / ycbcr2rgb (lbasicsr/utils/color_util.py:5-35, 71-97).  Both are float32 with a fixed operation
 * order and no fused multiply-add: savsr_amd/yuv.py restates them in numpy bit for bit.  Both only enqueue and allocate nothing;
 * arguments are checked before the device is touched (SAVSR_E_ARG + savsr_last_error()).
 * savsr_video_gather_i420:   frames [n_frames] I420 -> out [n_idx][3][h][w] fp32 planar RGB in [0, 1], slot k = frame idx[k] (the index
 *                         list of savsr_video_gather_u8).  Chroma replicated over its 2 x 2 block; per sample a 256-entry table the
 *                         compiler evaluates; R = y + rv, G = (y + gu) + gv, B = y + bu, clamped to [0, 1], not rounded to 8 bits.
 *                         Dword loads / 16-byte stores when w % 4 == 0, frames 4-byte and out 16-byte aligned.
 * savsr_video_quantize_i420: in [n][3][H][W] fp32 contiguous -> out [n] I420 frames: clamp(0, 1); Y per pixel; Cb / Cr from the mean RGB
 *                         of the block's in-image pixels (1, 2 or 4); rintf (round half to even).  16-byte loads / dword stores when
 *                         W % 4 == 0, in 16-byte and out 4-byte aligned. */
int savsr_video_gather_i420(const uint8_t* frames, int n_frames, int h, int w, const int32_t* idx, int n_idx, float* out, void* stream);
int savsr_video_quantize_i420(const float* in, int n, int H, int W, uint8_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 37) The same two conversions with the colour space as an argument (yuv.hip; colour / out_colour of SAVSR.upscale_video, --colour /
 * --out-colour of python -m savsr_amd.upscale).  colour = one of SAVSR_YUV_*:
 *   BT601       ITU-R BT.601 limited range with the reference's rounded constants: what the two entries above run, which are the
 *               colour = SAVSR_YUV_BT601 case of the same kernels
 *   BT709       Kr = 0.2126, Kb = 0.0722, limited range (Y 16 .. 235, chroma 16 .. 240): what players assume of untagged HD video
 *   BT601_FULL  Kr = 0.299, Kb = 0.114, full range (JFIF; Y4M's XCOLORRANGE=FULL)
 *   BT709_FULL  Kr = 0.2126, Kb = 0.0722, full range
 * The three are built in float64 from (Kr, Kb, range): Kg = 1 - Kr - Kb, Cb = (B - Y') / (2 (1 - Kb)), Cr = (R - Y') / (2 (1 - Kr)),
 * Y = 16 + 219 Y' and C = 128 + 224 C' limited, Y = 255 Y' and C = 128 + 255 C' full (savsr_amd/yuv.py `matrix` is the formula and
 * restates both kernels bit for bit).  Frame layout, index list, arithmetic, vector / scalar variants and alignment rules are those of
 * savsr_video_gather_i420 / savsr_video_quantize_i420; full range clips the rounded samples to 0 .. 255 (pure red / blue give a chroma
 * of 255.5).  The input and the output side are independent: BT.601 in, BT.709 out converts between the two at no extra cost.  A colour
 * outside 0 .. 3 is SAVSR_E_ARG, before the device is touched. */
#define SAVSR_YUV_BT601 0
#define SAVSR_YUV_BT709 1
#define SAVSR_YUV_BT601_FULL 2
#define SAVSR_YUV_BT709_FULL 3
int savsr_video_gather_yuv420(const uint8_t* frames, int n_frames, int h, int w, const int32_t* idx, int n_idx, int colour, float* out, void* stream);
int savsr_video_quantize_yuv420(const float* in, int n, int H, int W, int colour, uint8_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 36) The scene-cut detector's scores (scene.hip; savsr_amd.pair_sad / detect_cuts, upscale_video(cuts="auto"), DESIGN.md
 * section 1; savsr_amd/scenes.py restates them in numpy).  sad_out[k] (k = 0 .. n_frames - 2, int64 on the device) = the sum of absolute
 * differences of the 8-bit samples of frames k and k + 1: an exact integer, whatever the grid (integer atomics).  The entries zero
 * sad_out themselves (hipMemsetAsync on `stream`), only enqueue, allocate nothing and are capturable; arguments are checked before the
 * device is touched (SAVSR_E_ARG + savsr_last_error()).  n_frames = 1 is accepted and enqueues nothing (there is no pair).
 * savsr_video_pair_sad_u8:   frames [n_frames][h][w][c] uint8 (c = 1 .. 3): every byte, S = c * h * w samples per pair.
 * savsr_video_pair_sad_i420: frames [n_frames] I420 (the layout of savsr_video_gather_i420): the h * w Y bytes only.
 * savsr_video_pair_sad_f32:  frames [n_frames][c][h][w] fp32: every value quantised by savsr_video_quantize_u8's rule first (clamp to
 *                         [0, 1], x 255.0f, rintf; NaN -> 0), S = c * h * w.
 * 16-byte loads from both frames where the two frame pointers and the tail allow (a byte / float head and tail otherwise: odd sizes
 * and unaligned bases are served), 4 bytes per v_sad_u8, a wave reduction and one 64-bit vector atomic per workgroup. */
int savsr_video_pair_sad_u8(const uint8_t* frames, int n_frames, int c, int h, int w, int64_t* sad_out, void* stream);
int savsr_video_pair_sad_i420(const uint8_t* frames, int n_frames, int h, int w, int64_t* sad_out, void* stream);
int savsr_video_pair_sad_f32(const float* frames, int n_frames, int c, int h, int w, int64_t* sad_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 38) 10- and 12-bit 4:2:0 (yuv.hip, scene.hip; depth / out_depth of SAVSR.upscale_video, --out-depth of python -m savsr_amd.upscale,
 * DESIGN.md section 1).  A frame is the I420 frame above with every sample a little-endian 16-bit word, as it lies in a Y4M file tagged
 * C420p10 / C420p12: 2 * (h * w + 2 * ch * cw) bytes, frames back to back; `frames` / `out` stay byte pointers and must be 2-byte aligned
 * (an odd one is SAVSR_E_ARG).  depth = 10 or 12; colour = SAVSR_YUV_BT601 or SAVSR_YUV_BT709: high depth is defined for limited range
 * only (a sample is the 8-bit one times k = 2^(depth - 8); full range scales by 2^depth - 1 and has no definition here).  Anything else is
 * SAVSR_E_ARG + savsr_last_error(), before the device is touched.  The entries only enqueue, allocate nothing and are capturable;
 * savsr_amd/yuv.py (`i420_to_rgb` / `rgb_to_i420` with depth=) and scenes.py (`pair_sad` with depth=) restate them bit for bit.
 * savsr_video_gather_yuv420_16:   savsr_video_gather_yuv420's slots and index list.  No tables: with c = float(coef / k) and
 *                         o = float(offset / 255), Yt = y c_y, R = (Yt + v c_rv) + o_R, G = ((Yt + u c_gu) + v c_gv) + o_G,
 *                         B = (Yt + u c_bu) + o_B in float32 without fused multiply-add, clamped to [0, 1]; a sample above
 *                         2^depth - 1 reads as 2^depth - 1.  8-byte Y loads / 16-byte stores when w % 4 == 0, frames 8-byte and out
 *                         16-byte aligned; 16-bit loads otherwise.
 * savsr_video_quantize_yuv420_16: savsr_video_quantize_yuv420's float32 value of every sample times k (exact), then rintf (half to even);
 *                         Y in 16 k .. 235 k, chroma in 16 k .. 240 k, no clip.  16-byte loads / 8-byte Y stores when W % 4 == 0, in
 *                         16-byte and out 8-byte aligned; 16-bit stores otherwise.
 * savsr_video_pair_sad_i420_16:   savsr_video_pair_sad_i420 on the Y samples' 8 most significant bits, min(s, 2^depth - 1) >> (depth - 8):
 *                         the scores have the 8-bit scale, so a 10-bit video whose samples are an 8-bit video's x 4 gives that video's. */
int savsr_video_gather_yuv420_16(const uint8_t* frames, int n_frames, int h, int w, const int32_t* idx, int n_idx, int colour, int depth, float* out,
                                 void* stream);
int savsr_video_quantize_yuv420_16(const float* in, int n, int H, int W, int colour, int depth, uint8_t* out, void* stream);
int savsr_video_pair_sad_i420_16(const uint8_t* frames, int n_frames, int h, int w, int depth, int64_t* sad_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 39) 4:2:2 and 4:4:4 beside 4:2:0, at 8, 10 and 12 bits (yuv.hip, scene.hip; pixel_format / out = "i422", "i444" of
 * SAVSR.upscale_video, --out-chroma of python -m savsr_amd.upscale).  One entry per side serves every
 * (chroma, depth): chroma = one of SAVSR_CHROMA_*, depth = 8, 10 or 12.  A frame of an h x w picture is h * w Y samples, then ch * cw U
 * samples, then ch * cw V samples, (ch, cw) = ((h + 1) / 2, (w + 1) / 2) for 4:2:0, (h, (w + 1) / 2) for 4:2:2, (h, w) for 4:4:4; a byte
 * per sample at depth 8, a little-endian 16-bit word at 10 / 12 (2-byte aligned pointers; samples above 2^depth - 1 read as 2^depth - 1),
 * frames back to back.  The arithmetic is 4:2:0's with another block shape: to RGB a chroma sample serves its 1 x 2 (4:2:2) or 1 x 1
 * (4:4:4) block; from RGB, Cb / Cr come from (a + b) * 0.5 of a 4:2:2 pair (the pixel alone in the last column of an odd W) and from the
 * pixel's own clamped RGB in 4:4:4.  Chroma is centre-sited as in 4:2:0; MPEG-2's horizontally cosited 4:2:2 is not modelled.
 * savsr_amd/yuv.py (`chroma=`) restates all of it bit for bit.  SAVSR_CHROMA_420 is the 4:2:0 of the entries above and gives their
 * bytes.  Refused with SAVSR_E_ARG + savsr_last_error() before the device is touched: a chroma outside 0 .. 2, a depth other than
 * 8 / 10 / 12, a full-range colour at depth 10 / 12, a null pointer, an odd frame pointer at depth 10 / 12, an index outside the frames.
 * savsr_video_gather_yuvp:   frames -> out [n_idx][3][h][w] fp32 planar RGB, slot k = frame idx[k].  A thread owns 4 pixels of one row
 *                         (a Y dword or 8 bytes, the 2 or 4 chroma samples under them in one access, one 16-byte store per plane) when
 *                         w % 4 == 0, frames 4-byte (8-byte at depth 10 / 12) and out 16-byte aligned: every plane row then keeps the
 *                         alignment of its access (yuv.hip lists the offsets); a chroma sample and its pixels per thread otherwise.
 * savsr_video_quantize_yuvp: in [n][3][H][W] fp32 contiguous -> out [n] frames; the vector form under the same conditions, the input
 *                         loaded nontemporally.
 * savsr_video_pair_sad_yuvp: savsr_video_pair_sad_i420 / _i420_16 on frames of the given layout: the Y plane is the first h * w samples
 *                         of a frame in every layout, so this is the same kernels with another frame stride. */
#define SAVSR_CHROMA_420 0
#define SAVSR_CHROMA_422 1
#define SAVSR_CHROMA_444 2
int savsr_video_gather_yuvp(const uint8_t* frames, int n_frames, int h, int w, const int32_t* idx, int n_idx, int colour, int depth, int chroma,
                            float* out, void* stream);
int savsr_video_quantize_yuvp(const float* in, int n, int H, int W, int colour, int depth, int chroma, uint8_t* out, void* stream);
int savsr_video_pair_sad_yuvp(const uint8_t* frames, int n_frames, int h, int w, int depth, int chroma, int64_t* sad_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 40) Chroma siting and linear chroma reconstruction (yuv.hip; siting / out_siting of SAVSR.upscale_video, --siting / --out-siting of
 * python -m savsr_amd.upscale).  The arguments of savsr_video_gather_yuvp / savsr_video_quantize_yuvp with
 * siting = one of SAVSR_SITING_* after chroma.  NONE is "not modelled": the nearest-up / box-down pair of the entries above, their
 * kernels and their bytes.  Otherwise chroma sample (cy, cx) lies at luma position
 *   CENTRE    x = 2 cx + 0.5, y = 2 cy + 0.5 (4:2:0), y = cy (4:2:2)      JPEG, MPEG-1; Y4M's C420jpeg
 *   LEFT      x = 2 cx,       y = 2 cy + 0.5 (4:2:0), y = cy (4:2:2)      MPEG-2, H.264, HEVC 4:2:0, every standard 4:2:2; C420mpeg2
 *   TOPLEFT   x = 2 cx,       y = 2 cy (4:2:0 only)                       C420paldv, as ffmpeg maps it
 * 4:4:4 has nothing to resample: any siting there runs the entries above.  Refused with SAVSR_E_ARG + savsr_last_error() before the
 * device is touched: a siting outside 0 .. 3, TOPLEFT with SAVSR_CHROMA_422 (no vertical subsampling; LEFT is its cosited form), and
 * everything savsr_video_gather_yuvp / _quantize_yuvp refuse.  savsr_amd/yuv.py (`siting=`) restates both bit for bit.
 * savsr_video_gather_yuvs:   chroma at every luma pixel is the separable linear interpolation between the two nearest samples, edge
 *                         samples replicated, samples above 2^depth - 1 clipped first.  Per subsampled axis, pixels 2 c and 2 c + 1:
 *                         centre-sited (3 C[c] + C[c - 1]) / 4 and (3 C[c] + C[c + 1]) / 4; cosited C[c] and (C[c] + C[c + 1]) / 2 -- an
 *                         integer numerator times 2^-4 (4:2:0) or 2^-2 (4:2:2), exact in float32.  Then the arithmetic of
 *                         savsr_video_gather_yuv420_16 at every depth, 8 included (k = 1, all four colour spaces; no tables): within
 *                         1e-6 of the float64 closed form.  Constant chroma planes give the RGB of SITING_NONE bit for bit at 10 / 12
 *                         bits and within 1e-6 at 8.  Vector / scalar forms and alignment rules of savsr_video_gather_yuvp.
 * savsr_video_quantize_yuvs: NONE and CENTRE are savsr_video_quantize_yuvp (the box is the centre-sited filter).  Cosited axes take
 *                         h3(l, c, r) = ((l + r) + (c + c)) * 0.25f with every tap index clamped into the image: Hrow(y) = h3 of the
 *                         clamped RGB at x = 2 cx - 1, 2 cx, 2 cx + 1.  LEFT: Hrow(y) in 4:2:2, (Hrow(2 cy) + Hrow(2 cy + 1)) * 0.5f in
 *                         4:2:0 (Hrow(2 cy) alone on the last row of an odd H).  TOPLEFT: h3(Hrow(2 cy - 1), Hrow(2 cy), Hrow(2 cy + 1)),
 *                         rows clamped.  Y, the rows, the rounding and the full-range clip are savsr_video_quantize_yuvp's. */
#define SAVSR_SITING_NONE 0
#define SAVSR_SITING_CENTRE 1
#define SAVSR_SITING_LEFT 2
#define SAVSR_SITING_TOPLEFT 3
int savsr_video_gather_yuvs(const uint8_t* frames, int n_frames, int h, int w, const int32_t* idx, int n_idx, int colour, int depth, int chroma,
                            int siting, float* out, void* stream);
int savsr_video_quantize_yuvs(const float* in, int n, int H, int W, int colour, int depth, int chroma, int siting, uint8_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 41) Luma-only checkpoints (num_in_ch = 1) on planar YUV and grey-scale video (luma.hip; chroma_filter = "bicubic" and
 * pixel_format / out = "y400" of SAVSR.upscale_video, --chroma-filter of python -m savsr_amd.upscale).  The Y plane
 * goes through the network; Cb / Cr go from samples to samples through a separable, siting-aware cubic at the network's scale.  Samples
 * are bytes at depth 8 and little-endian 16-bit words at 10 / 12 (a sample above 2^depth - 1 reads as 2^depth - 1); frame pointers stay
 * byte pointers.  All float32 with a fixed operation order and no fused multiply-add: savsr_amd/yuv.py (`luma_to_unit`, `unit_to_luma`,
 * `chroma_axis_table`, `resample_chroma`) restates the three bit for bit.  They only enqueue, allocate nothing and are capturable.
 * Refused before the device is touched, with savsr_last_error() naming the reason: SAVSR_E_ARG for a null pointer, a size below 1, a
 * depth other than 8 / 10 / 12, a frame stride smaller than the plane, a plane that does not lie inside its frame, a bad index list;
 * SAVSR_E_ALIGN for 16-bit samples behind an odd pointer, frame stride or plane offset.
 * savsr_video_gather_luma:   the Y plane (the first h * w samples) of frames `frame_bytes` bytes apart -> out [n_idx][1][h][w] fp32, slot
 *                         k = float(min(s, 2^depth - 1)) / float(255 * 2^(depth - 8)) of frame idx[k] (the index list of
 *                         savsr_video_gather_u8): one IEEE division, savsr_video_gather_u8's value at depth 8; the same rule whatever
 *                         the colour space.  4 samples per access / one 16-byte store when w % 4 == 0, frames and frame_bytes 4-byte
 *                         (8-byte at depth 10 / 12) and out 16-byte aligned; a sample per access otherwise.
 * savsr_video_quantize_luma: in [n][1][H][W] fp32 contiguous -> the Y plane of n frames `out_frame_bytes` bytes apart:
 *                         rintf(clamp(v, 0, 1) * (255 * 2^(depth - 8))), half to even, NaN -> 0; savsr_video_quantize_u8's rule at depth
 *                         8.  The vector form under the same conditions, the input loaded nontemporally.
 * savsr_video_resample_chroma: one plane of n frames: ch x cw samples at src + f * src_frame_bytes + src_plane_offset -> cH x cW samples
 *                         at dst + f * dst_frame_bytes + dst_plane_offset.  ymin / ysize / wy[cH][taps_y] and xmin / xsize /
 *                         wx[cW][taps_x]: DEVICE arrays, the per-output windows and float32 weights of the two axes as for
 *                         savsr_resize_aa_axis (savsr_amd/yuv.py `chroma_axis_table`).  Samples clipped to 2^depth_in - 1; width first
 *                         (acc + w * s in tap order), then height over the filtered rows, x 2^(depth_out - depth_in), rintf, clipped
 *                         to 0 .. 2^depth_out - 1.  Both axes in one launch: a workgroup owns 16 x 64 output samples and stages the
 *                         filtered input rows they need in LDS, 32 rows (8 KiB) at a time; a tile that needs more rows loops, so any
 *                         taps_y is served.  Table indices are clamped into the plane: no table causes an access outside it.  A
 *                         window that runs past the plane (no table of chroma_axis_table does) re-reads the last column on the
 *                         horizontal axis and drops the taps beyond the last row on the vertical one.  4 samples per store when cW % 4 == 0 and dst,
 *                         its stride and offset are 4-byte (8-byte at depth 10 / 12) aligned. */
int savsr_video_gather_luma(const uint8_t* frames, int n_frames, int64_t frame_bytes, int h, int w, int depth, const int32_t* idx, int n_idx,
                            float* out, void* stream);
int savsr_video_quantize_luma(const float* in, int n, int H, int W, int depth, uint8_t* out, int64_t out_frame_bytes, void* stream);
int savsr_video_resample_chroma(const uint8_t* src, int n, int64_t src_frame_bytes, int64_t src_plane_offset, int ch, int cw, int depth_in,
                                uint8_t* dst, int64_t dst_frame_bytes, int64_t dst_plane_offset, int cH, int cW, int depth_out,
                                const int32_t* ymin, const int32_t* ysize, const float* wy, int taps_y, const int32_t* xmin,
                                const int32_t* xsize, const float* wx, int taps_x, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 42) The active-picture detector's line sums (active.hip; savsr_amd.line_sums / detect_active_area, upscale_video(crop="auto"),
 * --crop auto of python -m savsr_amd.upscale): per matrix of a batch the sum of the 8-bit samples of every row and
 * of every column, exact integers from one read of the samples (savsr_amd/active.py `line_sums` restates them; cropdetect's rule runs on
 * the host, `active_rect`).  row_sums [n][rows] and col_sums [n][cols] are 32-bit cells, zeroed by the call on the same stream.  The
 * entries only enqueue, allocate nothing, do not synchronise and are capturable.  Refused before the device is touched, with
 * savsr_last_error() naming the reason: SAVSR_E_ARG for a null pointer, n, rows or a width below 1, a line longer than 4194240 samples, a
 * frame stride smaller than the matrix, a depth other than 10 / 12 (_u16); SAVSR_E_ALIGN for 16-bit samples behind an odd pointer or stride
 * and floats behind a pointer that is not 4-byte aligned.  16-byte loads when the base pointer, the frame stride and a row's bytes are
 * multiples of 16, a sample per access otherwise (any pointer, stride and size).
 * savsr_video_line_sums_u8:  n matrices of rows x row_bytes bytes, frame_bytes apart: packed [n][h][w][c] uint8 frames as h x (w * c) (the
 *                         caller folds the c byte columns of a pixel into its column: `line_sums` on [N, h, w, c] frames) and the Y plane
 *                         of 8-bit planar frames as h x w at the start of a frame (`line_sums` with pixel_format= and size=).
 * savsr_video_line_sums_u16: n matrices of rows x cols little-endian 16-bit samples, frame_bytes apart: the Y plane of 10- / 12-bit planar
 *                         frames, every sample as min(s, 2^depth - 1) >> (depth - 8) (`line_sums` with depth=).
 * savsr_video_line_sums_f32: n_mats contiguous matrices of rows x cols fp32, the planes of [N][c][h][w] frames: every value quantised by
 *                         savsr_video_quantize_u8's rule first (clamp to [0, 1], x 255.0f, rintf, NaN -> 0); the caller sums the c planes
 *                         of a frame (`line_sums` on float frames). */
int savsr_video_line_sums_u8(const uint8_t* frames, int n, int64_t frame_bytes, int rows, int row_bytes, uint32_t* row_sums, uint32_t* col_sums,
                             void* stream);
int savsr_video_line_sums_u16(const uint8_t* frames, int n, int64_t frame_bytes, int rows, int cols, int depth, uint32_t* row_sums,
                              uint32_t* col_sums, void* stream);
int savsr_video_line_sums_f32(const float* mats, int n_mats, int rows, int cols, uint32_t* row_sums, uint32_t* col_sums, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 43) The motion-adaptive deinterlacer (deinterlace.hip; savsr_amd.deinterlace, upscale_video(fields=...), VideoUpscaler(fields=...),
 * --fields of python -m savsr_amd.upscale): interlaced frames -> progressive frames at the field rate by ffmpeg
 * yadif's rule in 32-bit integers (savsr_amd/deinterlace.py `deinterlace_matrix` restates it sample by sample; the kernels equal it bit
 * for bit).  One matrix (a plane, or the h x (w * c) bytes of packed frames) of every frame per call: matrix k of the n_frames resident
 * frames starts at frames + k * frame_bytes + plane_offset, its rows follow each other directly.  Source frames [from, to) become the
 * 2 * (to - from) output frames at out + o * out_frame_bytes + out_plane_offset: frame 2 (n - from) + f keeps the rows of parity f
 * (order 0, top field first) or 1 - f (order 1) of source frame n and interpolates the others from frames n, max(n - 1, 0) and
 * min(n + 1, n_frames - 1), so a streaming caller passes its context frames and the range.  The source and the output must not overlap.
 * The entries only enqueue (one launch), allocate nothing, do not synchronise and are capturable.  Refused before the device is touched
 * with SAVSR_E_ARG, savsr_last_error() naming the reason: a null pointer, n_frames < 1, rows < 2 (or above 524280), an empty row, a step
 * outside 1 .. 4 or not dividing row_bytes, an order other than 0 / 1, a range outside 0 <= from < to <= n_frames, a negative plane offset,
 * a frame stride smaller than the offset plus the plane (either side); _u16: a depth other than 10 / 12, an odd pointer, stride or offset.
 * 16-byte accesses when the plane pointers, the frame strides and a row's bytes of both sides are multiples of 16, a sample per access
 * otherwise (any pointer, stride and size).
 * savsr_video_deinterlace_u8:  matrices of rows x row_bytes bytes with pixel step `step` (1: a plane; c: packed [n][h][w][c] frames, so
 *                           that a channel only meets itself).
 * savsr_video_deinterlace_u16: matrices of rows x cols little-endian 16-bit samples, read as min(s, 2^depth - 1); kept rows are copied
 *                           as they are. */
int savsr_video_deinterlace_u8(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int row_bytes, int step,
                               int order, int from, int to, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset, void* stream);
int savsr_video_deinterlace_u16(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int depth,
                                int order, int from, int to, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset, void* stream);

/* (ABI 48) The same with a method and a rate (deinterlacer= / field_rate= of upscale_video and VideoUpscaler, method= / rate= of
 * savsr_amd.deinterlace, --deinterlacer / --field-rate of python -m savsr_amd.upscale).  The argument lists above plus, in front of
 * `stream`, `method` (0: yadif, the entries above; 1: ffmpeg bwdif's rule, yadif's temporal clamp around the w3fdif interpolation filters --
 * savsr_amd/deinterlace.py `bwdif_matrix` restates it sample by sample, the kernels equal it bit for bit) and `rate` (0: double, two
 * output frames per source frame as above; 1: same, output frame n - from is the first field in time of source frame n, so `out`
 * holds to - from frames and the second fields are not computed).  bwdif has no horizontal taps: `step` is checked as above and then
 * ignored by method 1.  Method 0 with rate 0 gives the bytes of the entries above.  Refused as above, and: a method or a rate other
 * than 0 / 1. */
int savsr_video_deinterlace_u8_m(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int row_bytes, int step,
                                 int order, int from, int to, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset, int method, int rate,
                                 void* stream);
int savsr_video_deinterlace_u16_m(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int depth,
                                  int order, int from, int to, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset, int method, int rate,
                                  void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 44) Inverse 3:2 pulldown (pulldown.hip; savsr_amd.field_scores, savsr_amd.remove_pulldown, upscale_video(pulldown=...),
 * VideoUpscaler(pulldown=...), --pulldown of python -m savsr_amd.upscale): the field-match scores and the weave of
 * telecined film (savsr_amd/pulldown.py `field_scores` and `weave` restate them; the kernels equal them bit for bit; the match, the
 * decimation and the cadence-free rule itself are host work on these scores and on savsr_video_pair_sad_*).  Matrices are addressed as for
 * savsr_video_deinterlace_*: matrix k of the n_frames resident frames starts at frames + k * frame_bytes + plane_offset, its rows follow
 * each other directly; the first field is the rows of parity `order` (0: top field first, 1: bottom field first).  The entries only
 * enqueue, allocate nothing, do not synchronise and are capturable.  Refused before the device is touched with SAVSR_E_ARG,
 * savsr_last_error() naming the reason: a null pointer, n_frames < 1, rows < 1, an empty row, a plane above 2147418112 bytes, an order
 * other than 0 / 1, a range outside 0 <= from <= to <= n_frames (from == to: nothing is done), a negative plane offset, a frame stride
 * smaller than the offset plus the plane, an `out` of scores that is not 8-byte aligned; _u16: a depth other than 10 / 12, an odd pointer,
 * stride or offset.  16-byte accesses when the plane pointers, the frame strides and a row's bytes are multiples of 16, a sample per
 * access otherwise (any pointer, stride and size).
 * savsr_video_field_scores_u8:  out[2 (n - from) + j], n in [from, to): the sum over the second field's rows y, 1 <= y <= rows - 2, and all
 *                           x of |a - b| + |c - b| - |a - c|, a / c = frame n at rows y - 1 / y + 1, b = row y of frame max(n - 1, 0)
 *                           (j = 0) or of frame n (j = 1); zeros when rows < 3.  `out` is zeroed by one hipMemsetAsync on `stream` first.
 *                           A streaming caller passes its context frame and the range.
 * savsr_video_field_scores_u16: the same on rows x cols little-endian 16-bit samples, each read as min(s, 2^depth - 1) >> (depth - 8).
 * savsr_video_weave:        output frame n - from at out + (n - from) * out_frame_bytes + out_plane_offset: the rows of parity `order` of
 *                           frame n, the others of frame n + delta[n - from] clamped into [0, n_frames).  delta: a DEVICE table of
 *                           to - from int32, -1 or 0; the entry cannot see it, so the kernel clamps the frame index: a wrong table reads
 *                           a wrong frame, never outside the buffer.  A byte copy, so it serves every depth (row_bytes = 2 * cols at
 *                           10 / 12 bits); one launch per plane.  The source and the output must not overlap. */
int savsr_video_field_scores_u8(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int row_bytes, int order,
                                int from, int to, int64_t* out, void* stream);
int savsr_video_field_scores_u16(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int depth,
                                 int order, int from, int to, int64_t* out, void* stream);
int savsr_video_weave(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int row_bytes, int order, int from,
                      int to, const int32_t* delta, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset, void* stream);

/* (ABI 49) Residual combing after the match (combed= of savsr_amd.remove_pulldown, upscale_video and VideoUpscaler, savsr_amd.comb_windows,
 * --combed of python -m savsr_amd.upscale; savsr_amd/pulldown.py `comb_windows` restates the measure, the kernels equal it bit for bit).
 * savsr_video_comb_windows_u8:  matrices addressed and refused as for savsr_video_field_scores_u8, plus `step` (the samples of a pixel,
 *                           1 .. 4: 1 for a plane, c for packed frames) and `threshold` (0 .. 255).  A sample (y, x) on a second-field
 *                           row, 1 <= y <= rows - 2, is combed iff |a - b| + |c - b| - |a - c| > 2 * threshold, a / b / c = frame n at
 *                           rows y - 1 / y / y + 1.  Cells of 8 rows x 8 * step samples anchored at (0, 0) count them; a window is
 *                           2 x 2 cells, one at every cell origin, counting what lies inside the matrix.  out[2 (n - from)]: the
 *                           largest window count of frame n, out[2 (n - from) + 1]: its total; zeros when rows < 3.  `out` is zeroed
 *                           by one hipMemsetAsync on `stream` first; one launch; every grid shape gives the same integers.
 * savsr_video_comb_windows_u16: the same on rows x cols little-endian 16-bit samples, each read as min(s, 2^depth - 1) >> (depth - 8);
 *                           step 1.
 * savsr_video_deinterlace_masked_u8 / _u16: the argument lists of savsr_video_deinterlace_u8_m / _u16_m without `rate`, plus `flags`, a
 *                           DEVICE table of to - from int32: output frame n - from is the rate 1 ("same") result for source frame n
 *                           where flags[n - from] != 0 and a byte copy of frame n elsewhere (the workgroups of an unflagged frame copy
 *                           and do nothing else); neighbours are clamped among the resident frames.  Refused as the _m entries, and:
 *                           null or misaligned flags, the source frames and the output overlapping. */
int savsr_video_comb_windows_u8(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int row_bytes, int step,
                                int order, int from, int to, int threshold, int64_t* out, void* stream);
int savsr_video_comb_windows_u16(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int depth,
                                 int order, int from, int to, int threshold, int64_t* out, void* stream);
int savsr_video_deinterlace_masked_u8(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int row_bytes,
                                      int step, int order, int from, int to, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset,
                                      int method, const int32_t* flags, void* stream);
int savsr_video_deinterlace_masked_u16(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int depth,
                                       int order, int from, int to, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset, int method,
                                       const int32_t* flags, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 50) Temporal noise reduction (denoise.hip; savsr_amd.denoise_video, prepass.TemporalDenoiser, upscale_video(denoise="ata", ...),
 * VideoUpscaler(denoise=...), --denoise of python -m savsr_amd.upscale): ffmpeg atadenoise's serial rule in 32-bit
 * integers (savsr_amd/denoise.py `denoise_matrix` restates it sample by sample; the kernels equal it bit for bit).  Matrices are addressed
 * as for savsr_video_deinterlace_*: matrix k of the n_frames resident frames starts at frames + k * frame_bytes + plane_offset, its rows
 * follow each other directly.  Output frame n - from, n in [from, to), at out + (n - from) * out_frame_bytes + out_plane_offset: every
 * sample x of frame n becomes (x + the taken taps + (k >> 1)) / k, k = 1 + the number of taken taps.  Taps are the same sample of frames
 * n - 1, n - 2, ... and, in a walk of its own, n + 1, n + 2, ...: a walk takes the tap at distance d = 1 .. radius while
 * |x - tap| <= A and its sum of these differences <= B, A = thr_a << (depth - 8), B = thr_b << (depth - 8), and ends at the first tap
 * that fails or where the resident frames [0, n_frames) end, so a streaming caller passes `radius` frames of context on either side
 * and the range.  The source and the output must not overlap.  The entries only enqueue (one launch for up to 65535 frames), allocate
 * nothing, do not synchronise and are capturable.  Refused before the device is touched with SAVSR_E_ARG, savsr_last_error() naming
 * the reason: a null pointer, n_frames < 1, rows < 1, an empty row, a plane above 2147418112 bytes, a range outside
 * 0 <= from < to <= n_frames, a negative plane offset, a frame stride smaller than the offset plus the plane (either side), a radius
 * outside 1 .. 16, thresholds outside 0 <= thr_a <= thr_b <= 255 (8-bit code units at every depth), overlapping source and output;
 * _u16: a depth other than 10 / 12, an odd pointer, stride or offset.  16-byte accesses when the plane pointers and the frame strides
 * of both sides and the plane's bytes are multiples of 16, a sample per access otherwise (any pointer, stride and size).
 * savsr_video_denoise_u8:  matrices of rows x row_bytes bytes (a plane, or the h x (w * c) bytes of packed frames).
 * savsr_video_denoise_u16: matrices of rows x cols little-endian 16-bit samples, every one read as min(s, 2^depth - 1). */
int savsr_video_denoise_u8(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int row_bytes, int radius,
                           int thr_a, int thr_b, int from, int to, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset, void* stream);
int savsr_video_denoise_u16(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int depth, int radius,
                            int thr_a, int thr_b, int from, int to, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 51) Spatial noise reduction (nlmeans.hip; savsr_amd.denoise_spatial, upscale_video(spatial_denoise="nlm", ...),
 * VideoUpscaler(spatial_denoise=...), --spatial-denoise of python -m savsr_amd.upscale): non-local means in 32-bit
 * integers, every frame on its own (savsr_amd/nlmeans.py `nlm_matrix` restates it; the kernels equal it bit for bit).  The plane of frame
 * k starts at frames + k * frame_bytes + plane_offset and has rows rows of cols * step samples that follow each other directly; sample x
 * of a row meets the samples x +- j * step only, so step = 1 filters a plane and step = c filters every channel of packed frames of c
 * samples per pixel (cols pixels a row) as a plane of its own.  Output frame k at out + k * out_frame_bytes + out_plane_offset, laid out
 * alike: sample p becomes (sum of w * v[q] + (sum of w >> 1)) / sum of w over the candidates q = p + (dy, dx), |dy|, |dx| <= search,
 * inside the plane, w = W[((SSD >> 2 (depth - 8)) * 64) / divisor] for an index below 577 and 0 above, W[i] = rint(4096 exp(-i / 64)),
 * SSD the sum of squared differences of the (2 patch + 1)^2 patches around p and q with coordinates clamped to the plane.  The callers'
 * divisor is rint((2 patch + 1)^2 h^2), h the strength in 8-bit code units; their defaults (patch 3, search 7, h 3.0) are parameters,
 * nothing is validated on footage.  The entries only enqueue (one launch for up to 16383 frames), allocate nothing, do not synchronise
 * and are capturable.  Refused before the device is touched with SAVSR_E_ARG, savsr_last_error() naming the reason: a null pointer,
 * n_frames < 1, rows < 1, cols < 1, a step outside 1 .. 4, a plane above 2147418112 bytes, a negative plane offset, a frame stride
 * smaller than the offset plus the plane (either side), a patch outside 1 .. 3, a search outside 1 .. 7, a divisor outside 1 .. 65536,
 * overlapping source and output; _u16: a depth other than 10 / 12, an odd pointer, stride or offset.
 * savsr_video_nlmeans_u8:  planes of rows x (cols * step) bytes.
 * savsr_video_nlmeans_u16: the same in little-endian 16-bit samples, every one read as min(s, 2^depth - 1). */
int savsr_video_nlmeans_u8(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step, int patch,
                           int search, int divisor, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset, void* stream);
int savsr_video_nlmeans_u16(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step, int depth,
                            int patch, int search, int divisor, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 52) Deblocking (deblock.hip; savsr_amd.deblock_video, upscale_video(deblock="weak" | "strong", ...), VideoUpscaler(deblock=...),
 * --deblock of python -m savsr_amd.upscale): a weak / strong filter across the edges of a block grid anchored at
 * the plane's origin, pass X (vertical edges, every row) then pass Y (horizontal edges, every column, reading pass X's result), in
 * integers, every frame on its own (savsr_amd/deblock.py `deblock_matrix` / `deblock_fields` restate it; the kernels equal them bit for
 * bit).  Planes are addressed as for savsr_video_nlmeans_*: rows rows of cols * step samples, sample x meeting x +- j * step only; the
 * output frames are laid out the same way and only the plane is written (out of place).  block: 4, 8 or 16 samples.  strong: 0 weak
 * (2 samples a side), 1 strong (3 a side; a direction whose block is below 8 takes the weak filter).  interlaced: 1 filters the rows
 * 0::2 and 1::2 as planes of their own with a vertical block of block / 2 (no pass Y at block 4).  thr_a, thr_b: the thresholds A (on
 * the step across the edge) and Bt (on the steps beside it) in the depth's codes, 0 .. 255 << (depth - 8); A = 0 copies min(s, top).
 * One launch for all frames (at most 65535 a launch) with both passes in it: a workgroup stages a tile of 32 rows x 256 / step samples
 * (64 at step 3) plus a halo of 3 samples and 3 field rows in LDS and pass X's result never reaches global memory.
 * Refused (SAVSR_E_ARG, before anything is launched, the message naming the entry): a null pointer, n_frames < 1, rows < 1, cols < 1,
 * a step outside 1 .. 4, a plane above 2147418112 bytes, a negative plane offset, a frame stride smaller than the offset plus the plane
 * (either side), a block other than 4 / 8 / 16, strong or interlaced other than 0 / 1, a threshold out of range, overlapping source and
 * output; _u16: a depth other than 10 / 12, an odd pointer, stride or offset.
 * savsr_video_deblock_u8:  planes of rows x (cols * step) bytes.
 * savsr_video_deblock_u16: the same in little-endian 16-bit samples, every one read as min(s, 2^depth - 1). */
int savsr_video_deblock_u8(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step, int block,
                           int strong, int interlaced, int thr_a, int thr_b, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset,
                           void* stream);
int savsr_video_deblock_u16(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step, int depth,
                            int block, int strong, int interlaced, int thr_a, int thr_b, uint8_t* out, int64_t out_frame_bytes,
                            int64_t out_plane_offset, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 53) Deblocking on a grid with an origin, and the statistics that find block size and origin (deblock.hip, grid.hip;
 * savsr_amd.deblock_video(origin=...), savsr_amd.grid_stats, savsr_amd.detect_grid, upscale_video(deblock_origin=..., deblock_grid="auto"),
 * --deblock-origin / --deblock-grid of python -m savsr_amd.upscale).
 * savsr_video_deblock_u8_o / _u16_o: savsr_video_deblock_u8 / _u16 with the grid's origin: pass X filters the edges e = origin_x + k block,
 * 1 <= e <= cols - 1, pass Y those at origin_y + k block (field-wise: origin_y / 2 + k block / 2 in either field); reads beyond the plane
 * clamp to it on either side, writes beyond it are dropped.  The result is that of origin (0, 0) on the plane padded by
 * (block - origin) % block copies of its first row and column, without the padding: the kernel works in coordinates shifted by that
 * much, its tile grid starting before the plane.  The entries without `_o` are these at (0, 0) and write the bytes they wrote.
 * Refused beyond what they refuse: an origin outside 0 .. block - 1, an odd origin_y with interlaced (it would swap the fields).
 * savsr_video_grid_stats_u8 / _u16: planes addressed as for savsr_video_deblock_* (rows rows of cols pixels of step samples, sample x
 * meeting x +- j * step only), every sample on the 8-bit scale (min(s, 2^depth - 1) >> (depth - 8)).  Along a line v, at every boundary
 * x with 2 <= x <= L - 2: s = |v[x] - v[x-1]|, l = |v[x-1] - v[x-2]|, r = |v[x+1] - v[x]|; a hit iff s > l + r and s <= cap.
 * out[32 n + x mod 16] += the hits along the rows of frame n (x in pixels), out[32 n + 16 + y mod 16] += those along its columns;
 * interlaced = 1 takes the rows 0::2 and 1::2 as planes of their own for the columns, y the field row (the rows' counts do not change).
 * out (n_frames x 32 int64, device) is ADDED to: the caller zeroes it once, so that several planes land in one table
 * (savsr_amd/grid.py `grid_stats_matrix` restates it; the kernels equal it bit for bit; the decision is host work).
 * One launch for up to 65535 frames; the entry only enqueues, allocates nothing, does not synchronise and is capturable.  16-byte loads
 * when the plane's base pointer, the frame stride and the row bytes are multiples of 16, a sample per access otherwise; a lane walks
 * 4 rows keeping the four a column boundary reads; at most 32 64-bit atomics leave a workgroup.
 * Refused (SAVSR_E_ARG, before anything is launched, the message naming the entry): a null pointer, n_frames < 1, rows < 1, cols < 1, a
 * step outside 1 .. 4, a plane above 2147418112 bytes, a negative plane offset, a frame stride smaller than the offset plus the plane,
 * an out that is not 8-byte aligned, interlaced other than 0 / 1, cap outside 0 .. 255; _u16: a depth other than 10 / 12, an odd
 * pointer, stride or offset. */
int savsr_video_deblock_u8_o(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step, int block,
                             int strong, int interlaced, int thr_a, int thr_b, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset,
                             int origin_y, int origin_x, void* stream);
int savsr_video_deblock_u16_o(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step, int depth,
                              int block, int strong, int interlaced, int thr_a, int thr_b, uint8_t* out, int64_t out_frame_bytes,
                              int64_t out_plane_offset, int origin_y, int origin_x, void* stream);
int savsr_video_grid_stats_u8(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step,
                              int interlaced, int cap, int64_t* out, void* stream);
int savsr_video_grid_stats_u16(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step, int depth,
                               int interlaced, int cap, int64_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 54) Deringing (dering.hip; savsr_amd.dering_video, upscale_video(dering="cdef", ...), VideoUpscaler(dering=...), --dering of
 * python -m savsr_amd.upscale): per 8 x 8 block of the plane (the grid starts at the plane's origin, the last blocks
 * may be partial) a direction search on eight sets of line sums, then for every sample a constrained filter of four taps along the
 * block's direction (strength P, scaled by the block's directional variance) and eight taps across it (strength S), the result clamped
 * to the minimum and maximum of the sample and the taps read, in integers, every frame on its own (savsr_amd/dering.py `dering_matrix` /
 * `dering_fields` restate it; the kernels equal them bit for bit).  Planes are addressed as for savsr_video_deblock_*: rows rows of
 * cols * step samples, sample x meeting x +- j * step only; the output frames are laid out the same way and only the plane is written
 * (out of place).  interlaced: 1 filters the rows 0::2 and 1::2 as planes of their own, each with its own blocks and clamp.  pri, sec:
 * the strengths p and s in the depth's codes, multiples of 1 << (depth - 8), 0 .. 15 << (depth - 8) and 0 .. 4 << (depth - 8); both 0
 * copies min(s, top).  damping: 3 .. 6 in 8-bit code units (depth - 8 is added inside).
 * One launch for all frames (at most 65535 a launch): a workgroup stages a tile of 32 rows x 256 / step pixels (64 at step 3) plus a halo
 * of 2 samples and 2 field rows in LDS, finds dir and the primary strength once per block into LDS, filters from LDS and writes once.
 * Refused (SAVSR_E_ARG, before anything is launched, the message naming the entry): a null pointer, n_frames < 1, rows < 1, cols < 1,
 * a step outside 1 .. 4, a plane above 2147418112 bytes, a negative plane offset, a frame stride smaller than the offset plus the plane
 * (either side), interlaced other than 0 / 1, a strength out of range or not a multiple of 1 << (depth - 8), a damping outside 3 .. 6,
 * overlapping source and output; _u16: a depth other than 10 / 12, an odd pointer, stride or offset.
 * savsr_video_dering_u8:  planes of rows x (cols * step) bytes.
 * savsr_video_dering_u16: the same in little-endian 16-bit samples, every one read as min(s, 2^depth - 1). */
int savsr_video_dering_u8(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step,
                          int interlaced, int pri, int sec, int damping, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset,
                          void* stream);
int savsr_video_dering_u16(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step, int depth,
                           int interlaced, int pri, int sec, int damping, uint8_t* out, int64_t out_frame_bytes, int64_t out_plane_offset,
                           void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 55) Noise statistics (noise.hip; savsr_amd.noise_stats, savsr_amd.estimate_noise, upscale_video(denoise_strength="auto",
 * spatial_strength="auto"), --denoise-strength auto / --spatial-strength auto of python -m savsr_amd.upscale).
 * Planes are addressed as for savsr_video_grid_stats_* (rows rows of cols pixels of step samples, sample x meeting x +- j * step only),
 * every sample v = min(s, 2^depth - 1) at its own depth.  h[y][x] = v[y][x-1] - 2 v[y][x] + v[y][x+1],
 * L[y][x] = |h[y-1][x] - 2 h[y][x] + h[y+1][x]| for 1 <= y <= rows - 2, 1 <= x <= cols - 2; cell (i, j), i < (rows - 2) / 8,
 * j < (cols - 2) / 8, holds the 64 values L[8i+1 .. 8i+8][8j+1 .. 8j+8] (a plane below 10 x 10 has no cell).  A cell one of whose 8 row
 * sums or 8 column sums is 0 is flat: out[512 n + 510] += 1.  Any other cell has S = (sum of L) >> (depth - 8), b = min(S >> 4, 254):
 * out[512 n + 2 b] += 1, out[512 n + 2 b + 1] += S.  interlaced = 1 takes the rows 0::2 and 1::2 as planes of their own, both adding
 * into the frame's table.  out (n_frames x 256 x 2 int64, device) is ADDED to: the caller zeroes it once, so that several planes land in
 * one table (savsr_amd/noise.py `noise_stats_matrix` restates it; the kernels equal it bit for bit; the decision is host work).
 * One launch for up to 65535 frames (none where no plane holds a cell); the entry only enqueues, allocates nothing, does not
 * synchronise and is capturable.  A lane owns one cell and walks its 10 rows; at step 1 it loads 8 samples and the dword behind them
 * when the plane's base pointer, the frame stride and the row bytes are multiples of 8 (_u16: of 16), a sample per access otherwise;
 * a per-wave LDS table, then 64-bit atomics on the rows that are not zero.
 * Refused (SAVSR_E_ARG, before anything is launched, the message naming the entry): a null pointer, n_frames < 1, rows < 1, cols < 1, a
 * step outside 1 .. 4, a plane above 2147418112 bytes, a negative plane offset, a frame stride smaller than the offset plus the plane,
 * an out that is not 8-byte aligned, interlaced other than 0 / 1; _u16: a depth other than 10 / 12, an odd pointer, stride or
 * offset. */
int savsr_video_noise_stats_u8(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step,
                               int interlaced, int64_t* out, void* stream);
int savsr_video_noise_stats_u16(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int step, int depth,
                                int interlaced, int64_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 45) Video surfaces (surface.hip; savsr_amd.unpack_surface, savsr_amd.pack_surface, upscale_video(surface=..., out_surface=...),
 * VideoUpscaler(surface=..., out_surface=...)): NV12 / NV21 / NV16, P010 / P012 / P210 / P212, UYVY / YUYV and
 * pitched planar frames <-> the tightly packed planar frames every other video entry takes (savsr_amd/surface.py `unpack_frames` /
 * `pack_frames` restate them; the kernels equal them bit for bit).  The planar side: n_frames frames of h x w samples, planar_frame_bytes
 * apart, Y then U and V in layout `chroma` (0: 4:2:0, 1: 4:2:2, 2: 4:4:4, 3: the Y plane alone), a byte per sample at depth 8, a
 * little-endian 16-bit word at 10 / 12.  The surface side: frames surface_frame_bytes apart, described by `planes`, a HOST array of
 * n_planes (1 .. 3) x 17 int64 words read before the call returns: the plane's byte offset in a frame, its pitch, rows and groups per
 * row, its step (1, 2 or 4 samples per group), then (plane, mul, add) of four component streams (those beyond `step` are not read):
 * group g of a row holds, at sample position k, sample mul * g + add of the same row of planar plane `plane` (0 Y, 1 U, 2 V); a group
 * whose sample lies past the planar row's end is padding.  msb = 1 (depth 10 / 12): a surface word carries its sample in the high
 * `depth` bits; unpack writes x >> (16 - depth), pack min(s, 2^depth - 1) << (16 - depth); every other sample is copied verbatim.
 * One launch for all planes of all frames (the descriptors travel by value in the kernel arguments); the entries only enqueue, allocate
 * nothing, do not synchronise and are capturable.  Refused before the device is touched with SAVSR_E_ARG, savsr_last_error() naming the
 * reason: a null pointer, n_frames < 1, h or w outside 1 .. 65536, a depth, chroma, msb, plane count or step outside the lists above, a
 * negative offset, no rows or groups, a pitch below the row's bytes, an odd pointer, stride, offset or pitch with 16-bit samples, a
 * stream of a plane the layout has not, a surface plane whose rows are not its planar planes' rows or that has more groups than they
 * have samples, surface planes that overlap, a frame stride below either side's frame, a frame above 2^31 work items.
 * 16-byte accesses (and v_perm_b32 to de-interleave) when the surface pointer, its frame stride and the plane's offset and pitch are
 * multiples of 16, a sample per access otherwise and in the tails of rows.  A row is read inside [row start, row start + row bytes) only.
 * savsr_video_unpack_surface: surface -> planar.  Bytes of the surface that hold no sample are not read.
 * savsr_video_pack_surface:   planar -> surface.  surface_bytes (from the planes' last byte to surface_frame_bytes): the resolved bytes
 *                             of a frame; every one of them that no sample maps to is written as 0 (one hipMemset2DAsync on `stream`
 *                             first when the planes' rows do not cover them all), nothing is written beyond them. */
int savsr_video_unpack_surface(const uint8_t* surface, int n_frames, int64_t surface_frame_bytes, int h, int w, int depth, int chroma, int msb,
                               const int64_t* planes, int n_planes, uint8_t* planar, int64_t planar_frame_bytes, void* stream);
int savsr_video_pack_surface(const uint8_t* planar, int n_frames, int64_t planar_frame_bytes, int h, int w, int depth, int chroma, int msb,
                             const int64_t* planes, int n_planes, uint8_t* surface, int64_t surface_frame_bytes, int64_t surface_bytes,
                             void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 46) Scan detection (scan.hip; savsr_amd.field_stats, savsr_amd.detect_scan, savsr_amd.ScanStats, upscale_video(scan="detect"),
 * --scan detect of python -m savsr_amd.upscale): the field statistics that tell progressive, interlaced and
 * telecined video apart (savsr_amd/scan.py `field_stats` restates them; the kernels equal it bit for bit; the decision is host work on
 * these sums, savsr_amd/scan.py `verdict_from_stats`).  Matrices are addressed as for savsr_video_field_scores_*: matrix k of the
 * n_frames resident frames starts at frames + k * frame_bytes + plane_offset, its rows follow each other directly.  The entries only
 * enqueue on `stream` (one hipMemsetAsync of `out`, then one launch for up to 65535 frames) and allocate nothing; arguments are checked
 * before the device is touched (SAVSR_E_ARG + savsr_last_error()): a null pointer, no frames, rows or samples, a plane above 2147418112
 * bytes, a range outside 0 <= lo <= hi <= n_frames, a negative offset, a frame stride smaller than the offset plus the plane, an `out`
 * that is not 8-byte aligned; _u16: a depth other than 10 / 12, an odd pointer, stride or offset.  16-byte accesses when the plane
 * pointers, the frame strides and a row's bytes are multiples of 16, a sample per access otherwise (any pointer, stride and size).
 * savsr_video_field_stats_u8:  out[8 (n - lo) + 2 k + q], n in [lo, hi), q the parity of the rows summed over.  k = 0, 1, 2: the sum over
 *                           the rows y of parity q, 1 <= y <= rows - 2, and all x of |a - b| + |c - b| - |a - c|, a / c = frame n at
 *                           rows y - 1 / y + 1, b = row y of frame max(n - 1, 0) (k = 0), of frame min(n + 1, n_frames - 1) (k = 1) or of
 *                           frame n (k = 2).  k = 3: the sum over all rows y of parity q and all x of |frame n - frame max(n - 1, 0)|.
 *                           The neighbours are taken among the resident frames and clamped there: a streaming caller passes one frame
 *                           of context on either side and the range.
 * savsr_video_field_stats_u16: the same on rows x cols little-endian 16-bit samples, each read as min(s, 2^depth - 1) >> (depth - 8). */
int savsr_video_field_stats_u8(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int row_bytes, int lo,
                               int hi, int64_t* out, void* stream);
int savsr_video_field_stats_u16(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int cols, int depth,
                                int lo, int hi, int64_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 47) Ordered dither in the quantisers behind the network (video.hip, yuv.hip, luma.hip with csrc/dither.hpp; dither= of
 * SAVSR.upscale_video and VideoUpscaler, --dither of python -m savsr_amd.upscale).  The three entries below take the
 * arguments of savsr_video_quantize_u8 / _quantize_yuvs / _quantize_luma with dither = one of SAVSR_DITHER_* in front of `out`; the
 * entries without _d stay as they are.  NONE runs the kernels of the entry without _d and gives its bytes.  ORDERED: where that entry
 * computes rintf(t), t the float32 value in output code units, the sample is floorf(t + theta(y, x)) with
 *   B[y][x] = sum over b = 0 .. 3 of 4^(3 - b) (2 (((x ^ y) >> b) & 1) + ((y >> b) & 1))      the 16 x 16 Bayer index matrix, 0 .. 255 once each
 *   theta(y, x) = (B[y & 15][x & 15] + 0.5) / 256                                              exact in float32, inside (0, 1)
 * and (y, x) the sample's coordinates in its own plane: pixel coordinates for Y and packed RGB (the channels of a pixel share one
 * threshold), chroma-sample coordinates (cy, cx) for Cb / Cr.  The sum is one float32 addition (round to nearest even), not contracted
 * with the multiply in front of it; floorf follows, then the clip that follows rintf (0 .. 255 in the full-range colour spaces, none in
 * limited range, which stays in 16 k .. 235 k / 240 k by itself).  The clamp in front makes a NaN 0 as before.  The pattern does not
 * depend on the frame, so any split of a video into calls gives the same bytes; an integer t is written as it is; a constant
 * t = i + j / 256 gives every aligned 16 x 16 block the sum 256 i + j.  savsr_amd/dither.py restates the rule and yuv.py
 * (`rgb_to_i420`, `unit_to_luma` with dither=) and dither.py (`rgb_to_u8`) the three entries, bit for bit.  Refused with SAVSR_E_ARG +
 * savsr_last_error() before the device is touched: a dither other than 0 or 1, and everything the entry without _d refuses (under
 * this entry's name).  Vector / scalar forms and alignment rules are those of the entries without _d; they only enqueue, allocate
 * nothing and are capturable.
 * savsr_video_quantize_u8_d:   the packed quantiser: t = clamp(v, 0, 1) * 255 at pixel (p / W, p % W).
 * savsr_video_quantize_yuvs_d: every layout, depth, colour space and siting of savsr_video_quantize_yuvs: t = the row's float32 value
 *                           times k = 2^(depth - 8), Y at its pixel, Cb and Cr at their chroma sample (one threshold for the two).
 * savsr_video_quantize_luma_d: the luma-only path's Y plane: t = clamp(v, 0, 1) * (255 * 2^(depth - 8)).  The Cb / Cr planes of that path
 *                           are resampled samples (savsr_video_resample_chroma) and keep rintf. */
#define SAVSR_DITHER_NONE 0
#define SAVSR_DITHER_ORDERED 1
int savsr_video_quantize_u8_d(const float* in, int n, int c, int H, int W, int dither, uint8_t* out, void* stream);
int savsr_video_quantize_yuvs_d(const float* in, int n, int H, int W, int colour, int depth, int chroma, int siting, int dither, uint8_t* out,
                                void* stream);
int savsr_video_quantize_luma_d(const float* in, int n, int H, int W, int depth, int dither, uint8_t* out, int64_t out_frame_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 33) Geometric self-ensemble (ensemble.hip; SAVSR.set_self_ensemble).  Variant k = 0 .. 7: fw = k & 1 flips
 * the width, fh = (k >> 1) & 1 the height, t = k >> 2 transposes the last two dims; forward = the flips then the transpose, inverse = the
 * transpose then the flips (lbasicsr/models/sr_model.py:141-190).  Both entries only enqueue and allocate nothing; arguments are checked
 * before the device is touched (SAVSR_E_ARG + savsr_last_error() for a null pointer, c outside 1 .. 3, k outside 0 .. 7, a bad index list).
 * savsr_ensemble_gather_u8 / _f32: the arguments of savsr_video_gather_u8 / _f32 plus the variant k: out [n_idx][c][h][w] fp32 of variant k,
 *                         [n_idx][c][w][h] when t is set (through an LDS tile).  Same byte table as the video gather: variant 0 is
 *                         savsr_video_gather_* bit for bit.
 * savsr_ensemble_merge:   the 8 network outputs of one clip, variant k at base + offs[k] floats (offs: a HOST array of 8 signed element
 *                         offsets, so the outputs may lie in different tensors): k < 4 [c][H][W], k >= 4 [c][W][H].  Undoes every
 *                         variant and writes ((((o0 + o1) + o2) + ... ) + o7) * 0.125f in fp32 in that order: out [c][H][W] fp32, or with
 *                         out_u8 = 1 [H][W][c] uint8 quantised by savsr_video_quantize_u8's rule.  One pass: 8 reads + 1 write. */
int savsr_ensemble_gather_u8(const uint8_t* frames, int n_frames, int c, int h, int w, const int32_t* idx, int n_idx, int k, float* out,
                             void* stream);
int savsr_ensemble_gather_f32(const float* frames, int n_frames, int c, int h, int w, const int32_t* idx, int n_idx, int k, float* out,
                              void* stream);
int savsr_ensemble_merge(const float* base, const int64_t* offs, int c, int H, int W, int out_u8, void* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * PSNR-Y / SSIM-Y of one output frame with the reference's numerics (SURVEY section 8, row f3 -- the step after the
 * hot path): tensor2img quantisation (lbasicsr/utils/img_util.py:66-90), BT.601 luma (metrics/metric_util.py:32-45,
 * utils/color_util.py:59-65), calculate_psnr / calculate_ssim (metrics/psnr_ssim.py:42-48, 172-200).
 * sr, gt: RGB planar fp32 [3] planes of [H][W] (*_plane floats apart), values in [0,1] before clamping.
 * partial: scratch of savsr_metrics_blocks(H, W, crop_border) * 2 doubles; out: 2 doubles = PSNR-Y (inf for
 * identical images), SSIM-Y.  Both stay on the device; the calls only enqueue. */
int savsr_metrics_blocks(int H, int W, int crop_border);       /* < 0: the cropped image is smaller than 11 x 11 */
int savsr_metrics_psnr_ssim_y(const float* sr, int64_t sr_plane, const float* gt, int64_t gt_plane, int H, int W,
                              int crop_border, double* partial, double* out, void* stream);
/* The same with `test_y_channel` as the YAML's metric option (psnr_ssim.py:12,85): != 0 is savsr_metrics_psnr_ssim_y; 0 takes the
 * three colour planes of the quantised image -- PSNR from the mean squared difference over H x W x 3, SSIM as the mean of the
 * planes' SSIM (psnr_ssim.py:115-129) -- and needs partial[3 * savsr_metrics_blocks(..) * 2]. */
int savsr_metrics_psnr_ssim(const float* sr, int64_t sr_plane, const float* gt, int64_t gt_plane, int H, int W, int crop_border,
                            int test_y_channel, double* partial, double* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * One axis of the anti-aliased bicubic resize behind the reference's LR synthesis (SURVEY section 8, row f2 -- the step
 * before the hot path): lbasicsr/data/data_util.py:371-420 -> torchvision T.Resize(BICUBIC, antialias=True) -> ATen
 * _upsample_bicubic2d_aa.  in: [planes][h][w] fp32; axis 0 resizes the width (out [planes][h][out_size]), axis 1 the
 * height (out [planes][out_size][w]).  xmin / xsize / weights[out_size][max_taps]: the per-output-index windows and
 * normalised weights as ATen computes them (savsr_amd/resize_gpu.py::aa_tables).  Width first, then height. */
int savsr_resize_aa_axis(const float* in, int planes, int h, int w, int axis, int out_size, const int32_t* xmin,
                         const int32_t* xsize, const float* weights, int max_taps, float* out, void* stream);

/* ---- diagnostics: compiled ONLY into the instrumented library (SAVSR_DIAG=1 savsr_amd/csrc/build.sh ->
 * libsavsr_hip_diag.so, loaded by the tools through SAVSR_LIB_PATH).  The product library libsavsr_hip.so carries neither
 * these entry points nor the DIAG kernel instantiations nor any process-global switch: every product call is a pure
 * function of its arguments.  Synchronous; while a stamps mode is on, the conv / SATU launches run INSTRUMENTED builds of their kernels (template parameter
 * DIAG); with the mode off (the default) the product kernels carry no diagnostic code at all.
 * Conv kernel, savsr_debug_conv_stamps(mode): 0 off; 1 per-workgroup s_memtime stamps [blk][6] = entry, after
 * the prologue, after the first K phase, after the first tile's K loop, after the stores drained,
 * s_memrealtime at entry; 3 + w: accumulated section times of wave w ([blk][0..4] = steps after the barrier,
 * steps before it, wait, barrier, epilogue); + 16 / + 32 / + 64 / + 128 / + 256 / + 512: timing experiments that skip
 * the staging / the fragment reads / the epilogue's stores / its LDS transpose / its whole body / its bias load
 * (results invalid). */
#ifdef SAVSR_DIAG
int savsr_debug_conv_stamps(int enable);
int savsr_debug_read_conv_stamps(long long* host, int nblocks);
/* SATU LR / HR kernels: [blk][8] accumulated section times of wave 0 (see satu.hip), last = total. */
int savsr_debug_satu_stamps(int enable);
int savsr_debug_read_satu_stamps(long long* host, int nblocks);
/* Resident workgroups per CU predicted by the runtime for the SATU HR (which = 0) / LR (1) kernel with
 * lds_bytes of dynamic LDS; < 0 = -hipError_t. */
int savsr_debug_satu_occupancy(int which, int lds_bytes);
#endif /* SAVSR_DIAG */

#ifdef __cplusplus
}
#endif
#endif /* SAVSR_HIP_H */
