// Video surfaces (ABI 45): NV12 / NV21 / NV16, P010 / P012 / P210 / P212, UYVY / YUYV and pitched planar frames <-> the project's tightly
// packed planar frames (savsr_amd/surface.py `unpack_frames` / `pack_frames` are the specification, byte by byte; the kernels equal it
// bit for bit).  A surface is one to three surface planes; a surface plane is a pitched byte matrix of `groups` groups per row, a group
// is `step` samples, one of each component stream; stream k carries sample mul * g + add of a row of one planar plane.
//
// One launch per call for all planes of all frames: grid = (items of a frame, frame).  The work item is a run of bytes of a SURFACE row,
// never of a planar row: on pack a thread owns its destination bytes outright and gathers them from up to three planar planes (two
// planes never meet in one dword); on unpack the interleaved chroma row is read once and feeds both U and V.
//   vector item   16 bytes (step 1) or 32 bytes (step 2, 4) of a surface row in 16-byte accesses (u32x4), the surface side aligned; bytes
//                 and 16-bit halves are de-interleaved / re-interleaved with v_perm_b32.  The planar side is tightly packed, so its rows
//                 start anywhere: its accesses are 16 / 8 bytes wide at their natural address (global memory takes unaligned accesses).
//                 Taken when the surface's base pointer, frame stride, plane offset and pitch are multiples of 16, for the items that lie
//                 wholly inside the row's bytes and whose samples all exist (not the pad Y of an odd-width packed row).
//   sample item   one sample (any pointer, stride and size), and the tails of the rows of the vector form (a loop over the item's samples).
// A thread never reads a source byte outside [row start, row start + row bytes) and never writes outside the rows of its plane; on pack
// the bytes no sample maps to (row padding, padded lines) are zeroed by one hipMemset2DAsync over the frames' resolved bytes before the
// launch when the surface is not tight, and by the kernel (the pad Y, the low bits of msb words) where they lie inside a row.
#include "common.hpp"
#include "video_samples.hpp"

#include <cstdint>

namespace savsr {
namespace {

constexpr int SF_THREADS = 256;
constexpr int SF_MAX_Y = 65535;                       // grid.y
constexpr int SF_DESC_WORDS = 17;                     // int64 words per plane of the descriptor

typedef uint32_t sf_u2 __attribute__((ext_vector_type(2)));
typedef u32x4 sf_u4_any __attribute__((aligned(1)));          // a 16-byte access at any address
typedef sf_u2 sf_u2_any __attribute__((aligned(1)));          // an 8-byte access at any address

// byte i of the result = byte sel.b[i] of {hi : lo} (lo = bytes 0 .. 3): one v_perm_b32
__device__ __forceinline__ uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if __has_builtin(__builtin_amdgcn_perm)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t v = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) r |= (uint32_t)((v >> (8 * ((sel >> (8 * i)) & 7u))) & 255u) << (8 * i);
    return r;
#endif
}

// What a launch works on.  Per plane and stream: where the planar plane lies in a planar frame, its row bytes and its samples per row.
struct SfPlane {
    long long off, pitch;                  // the surface plane: bytes into a surface frame, bytes between rows
    long long poff[4];
    int ppitch[4], pw[4], mul[4], add[4];
    int rows, step;
    int row_bytes;                         // groups * step * sample bytes
    int vec_bytes;                         // the leading bytes of a row that vector items may cover (0: a sample per item)
    int item_bytes, items, first;          // bytes of an item, items per row, the plane's first item among a frame's
    int ya, yb, c0, c1;                    // step 4: the streams of the even Y, the odd Y and the two chroma components
};

struct SfJob {
    const uint8_t* in;
    uint8_t* out;
    long long sstride, pstride;            // frame strides of the surface and the planar side
    int nplanes, total;                    // items of a frame
    int shift;                             // msb: 16 - depth
    uint32_t top;                          // msb: 2^depth - 1
    SfPlane pl[3];
};

// a sample / a dword of samples from one side to the other
template <bool PACK, int S, bool MSB>
__device__ __forceinline__ uint32_t conv1(uint32_t v, const SfJob& jb) {
    if constexpr (!MSB) return v;
    else if constexpr (PACK) return min(v, jb.top) << jb.shift;
    else return v >> jb.shift;
}

template <bool PACK, int S, bool MSB>
__device__ __forceinline__ uint32_t conv(uint32_t v, const SfJob& jb) {
    if constexpr (!MSB) return v;
    else if constexpr (PACK) return (min(v & 0xffffu, jb.top) | (min(v >> 16, jb.top) << 16)) << jb.shift;
    else return (v >> jb.shift) & ((0xffffu >> jb.shift) * 0x10001u);
}

template <int S>
__device__ __forceinline__ uint32_t load1(const uint8_t* p) {
    if constexpr (S == 1) return *p;
    else return *reinterpret_cast<const uint16_t*>(p);
}

template <int S>
__device__ __forceinline__ void store1(uint8_t* p, uint32_t v) {
    if constexpr (S == 1) *p = (uint8_t)v;
    else *reinterpret_cast<uint16_t*>(p) = (uint16_t)v;
}

// PACK: planar -> surface.  S: bytes of a sample.  MSB: 16-bit words carry the sample in their high bits.  VEC: some plane has vector items.
template <bool PACK, int S, bool MSB, bool VEC>
__global__ __launch_bounds__(SF_THREADS) void surface_kernel(SfJob jb) {
    const unsigned idx = blockIdx.x * SF_THREADS + threadIdx.x;
    if (idx >= (unsigned)jb.total) return;
    int p = 0;
    if (jb.nplanes > 1 && idx >= (unsigned)jb.pl[1].first) p = 1;
    if (jb.nplanes > 2 && idx >= (unsigned)jb.pl[2].first) p = 2;
    const SfPlane& P = jb.pl[p];
    const unsigned li = idx - (unsigned)P.first;
    const int r = (int)(li / (unsigned)P.items);
    const int b0 = (int)(li - (unsigned)r * (unsigned)P.items) * P.item_bytes;          // the item's first byte in its surface row
    const long long n = blockIdx.y;
    const long long srow = n * jb.sstride + P.off + r * P.pitch;
    const long long pfrm = n * jb.pstride;
    const uint8_t* sin = jb.in + srow;          // the surface row (the side that is the source)
    uint8_t* sout = jb.out + srow;
    if (VEC && b0 + P.item_bytes <= P.vec_bytes) {
        if (P.step == 1) {                      // 16 bytes of one stream
            const long long pa = pfrm + P.poff[0] + (long long)r * P.ppitch[0] + b0;
            u32x4 v;
            if constexpr (PACK) v = *reinterpret_cast<const sf_u4_any*>(jb.in + pa);
            else v = *reinterpret_cast<const u32x4*>(sin + b0);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = conv<PACK, S, MSB>(v[k], jb);
            if constexpr (PACK) *reinterpret_cast<u32x4*>(sout + b0) = v;
            else *reinterpret_cast<sf_u4_any*>(jb.out + pa) = v;
        } else if (P.step == 2) {               // 32 bytes: 16 of stream 0 and 16 of stream 1
            const long long pa = pfrm + P.poff[0] + (long long)r * P.ppitch[0] + (b0 >> 1);
            const long long pb = pfrm + P.poff[1] + (long long)r * P.ppitch[1] + (b0 >> 1);
            constexpr uint32_t EVEN = S == 1 ? 0x06040200u : 0x05040100u, ODD = S == 1 ? 0x07050301u : 0x07060302u;          // de-interleave
            constexpr uint32_t LOW = S == 1 ? 0x05010400u : 0x05040100u, HIGH = S == 1 ? 0x07030602u : 0x07060302u;          // interleave
            if constexpr (PACK) {
                const u32x4 a = *reinterpret_cast<const sf_u4_any*>(jb.in + pa), b = *reinterpret_cast<const sf_u4_any*>(jb.in + pb);
                u32x4 d0, d1;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const uint32_t a0 = conv<PACK, S, MSB>(a[j], jb), b0_ = conv<PACK, S, MSB>(b[j], jb);
                    const uint32_t a1 = conv<PACK, S, MSB>(a[2 + j], jb), b1 = conv<PACK, S, MSB>(b[2 + j], jb);
                    d0[2 * j] = perm(b0_, a0, LOW); d0[2 * j + 1] = perm(b0_, a0, HIGH);
                    d1[2 * j] = perm(b1, a1, LOW);  d1[2 * j + 1] = perm(b1, a1, HIGH);
                }
                *reinterpret_cast<u32x4*>(sout + b0) = d0;
                *reinterpret_cast<u32x4*>(sout + b0 + 16) = d1;
            } else {
                const u32x4 d0 = *reinterpret_cast<const u32x4*>(sin + b0), d1 = *reinterpret_cast<const u32x4*>(sin + b0 + 16);
                u32x4 a, b;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    a[j] = conv<PACK, S, MSB>(perm(d0[2 * j + 1], d0[2 * j], EVEN), jb);
                    b[j] = conv<PACK, S, MSB>(perm(d0[2 * j + 1], d0[2 * j], ODD), jb);
                    a[2 + j] = conv<PACK, S, MSB>(perm(d1[2 * j + 1], d1[2 * j], EVEN), jb);
                    b[2 + j] = conv<PACK, S, MSB>(perm(d1[2 * j + 1], d1[2 * j], ODD), jb);
                }
                *reinterpret_cast<sf_u4_any*>(jb.out + pa) = a;
                *reinterpret_cast<sf_u4_any*>(jb.out + pb) = b;
            }
        } else if (S == 1) {                    // step 4, 32 bytes = 8 groups: 16 Y, 8 and 8 chroma samples
            const long long py = pfrm + P.poff[P.ya] + (long long)r * P.ppitch[P.ya] + (b0 >> 1);
            const long long pa = pfrm + P.poff[P.c0] + (long long)r * P.ppitch[P.c0] + (b0 >> 2);
            const long long pb = pfrm + P.poff[P.c1] + (long long)r * P.ppitch[P.c1] + (b0 >> 2);
            if constexpr (PACK) {
                const u32x4 y = *reinterpret_cast<const sf_u4_any*>(jb.in + py);
                const sf_u2 a = *reinterpret_cast<const sf_u2_any*>(jb.in + pa), b = *reinterpret_cast<const sf_u2_any*>(jb.in + pb);
                // a group as [Y even, Y odd, c0, c1], then each byte to its place in the group
                const uint32_t place = ((0u << (8 * P.ya)) | (1u << (8 * P.yb)) | (2u << (8 * P.c0)) | (3u << (8 * P.c1)));
                uint32_t d[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) {          // groups 2j and 2j + 1: the Y dword j, chroma bytes 2j and 2j + 1
                    const uint32_t cc = perm(b[j >> 1], a[j >> 1], (j & 1) ? 0x07030602u : 0x05010400u);          // [a(2j) b(2j) a(2j+1) b(2j+1)]
                    d[2 * j] = perm(0u, perm(cc, y[j], 0x05040100u), place);
                    d[2 * j + 1] = perm(0u, perm(cc, y[j], 0x07060302u), place);
                }
                *reinterpret_cast<u32x4*>(sout + b0) = u32x4{d[0], d[1], d[2], d[3]};
                *reinterpret_cast<u32x4*>(sout + b0 + 16) = u32x4{d[4], d[5], d[6], d[7]};
            } else {
                const u32x4 d0 = *reinterpret_cast<const u32x4*>(sin + b0), d1 = *reinterpret_cast<const u32x4*>(sin + b0 + 16);
                const uint32_t d[8] = {d0[0], d0[1], d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]};
                const uint32_t sel_y = (uint32_t)P.ya | ((uint32_t)P.yb << 8) | ((uint32_t)(P.ya + 4) << 16) | ((uint32_t)(P.yb + 4) << 24);
                const uint32_t sel_c = (uint32_t)P.c0 | ((uint32_t)(P.c0 + 4) << 8) | ((uint32_t)P.c1 << 16) | ((uint32_t)(P.c1 + 4) << 24);
                u32x4 y;
                uint32_t t[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    y[j] = perm(d[2 * j + 1], d[2 * j], sel_y);
                    t[j] = perm(d[2 * j + 1], d[2 * j], sel_c);          // [a(2j) a(2j+1) b(2j) b(2j+1)]
                }
                *reinterpret_cast<sf_u4_any*>(jb.out + py) = y;
                *reinterpret_cast<sf_u2_any*>(jb.out + pa) = sf_u2{perm(t[1], t[0], 0x05040100u), perm(t[3], t[2], 0x05040100u)};
                *reinterpret_cast<sf_u2_any*>(jb.out + pb) = sf_u2{perm(t[1], t[0], 0x07060302u), perm(t[3], t[2], 0x07060302u)};
            }
        }
        return;
    }
    // the item's samples one at a time: element e of the row is stream e % step of group e / step
    const int e1 = min(b0 + P.item_bytes, P.row_bytes) / S;
    for (int e = b0 / S; e < e1; ++e) {
        const int g = e / P.step, k = e - g * P.step;
        const int x = P.mul[k] * g + P.add[k];
        const bool there = x < P.pw[k];
        const long long pa = pfrm + P.poff[k] + (long long)r * P.ppitch[k] + (long long)x * S;
        if constexpr (PACK) store1<S>(sout + (long long)e * S, there ? conv1<PACK, S, MSB>(load1<S>(jb.in + pa), jb) : 0u);
        else if (there) store1<S>(jb.out + pa, conv1<PACK, S, MSB>(load1<S>(sin + (long long)e * S), jb));
    }
}

template <bool PACK, int S, bool MSB>
void launch_form(const SfJob& jb, bool vec, dim3 grid, hipStream_t st) {
    if (vec) hipLaunchKernelGGL((surface_kernel<PACK, S, MSB, true>), grid, dim3(SF_THREADS), 0, st, jb);
    else hipLaunchKernelGGL((surface_kernel<PACK, S, MSB, false>), grid, dim3(SF_THREADS), 0, st, jb);
}

// The checks and the job the two entries share.  `surf` / `planar`: frame 0 of either side.  0, or SAVSR_E_ARG with the message set.
int build_job(const char* who, bool pack, const uint8_t* surf, const uint8_t* planar, int n_frames, int64_t surf_stride, int64_t planar_stride,
              int h, int w, int depth, int chroma, int msb, const int64_t* desc, int n_planes, SfJob& jb, int64_t& span, int64_t& covered,
              bool& vec) {
    char msg[200];
    const char* why = nullptr;
    const int S = depth == 8 ? 1 : 2;
    if (!surf || !planar || !desc) why = "null pointer";
    else if (n_frames < 1) why = "n_frames >= 1";
    else if (h < 1 || w < 1 || h > 65536 || w > 65536) why = "h, w in 1 .. 65536";
    else if (depth != 8 && depth != 10 && depth != 12) why = "depth 8, 10 or 12";
    else if (chroma < 0 || chroma > 3) why = "chroma 0 (4:2:0), 1 (4:2:2), 2 (4:4:4) or 3 (4:0:0, the Y plane alone)";
    else if (msb != 0 && (msb != 1 || depth == 8)) why = "msb 0 or 1, and 1 at depth 10 / 12 only";
    else if (n_planes < 1 || n_planes > 3) why = "1 .. 3 surface planes";
    else if (S == 2 && (((reinterpret_cast<uintptr_t>(surf) | reinterpret_cast<uintptr_t>(planar)) & 1) || ((surf_stride | planar_stride) & 1)))
        why = "the pointers and the frame strides must be 2-byte aligned (16-bit samples)";
    if (why) {
        snprintf(msg, sizeof msg, "%s: %s", who, why);
        return fail_arg(msg);
    }
    // the planar frame: Y, then U and V
    const int ch = chroma == 0 ? (h + 1) / 2 : h, cw = chroma <= 1 ? (w + 1) / 2 : w;
    const int prow[3] = {h, ch, ch}, pcol[3] = {w, cw, cw};
    const int64_t pbase[3] = {0, (int64_t)h * w * S, ((int64_t)h * w + (int64_t)ch * cw) * S};
    const int np = chroma == 3 ? 1 : 3;
    const int64_t frame_bytes = chroma == 3 ? pbase[1] : pbase[2] + (int64_t)ch * cw * S;
    if (planar_stride < frame_bytes) why = "planar_frame_bytes smaller than a planar frame";
    const bool surf16 = (reinterpret_cast<uintptr_t>(surf) & 15) == 0 && surf_stride % 16 == 0;
    int64_t first = 0, lo[3], hi[3];
    span = covered = 0;
    vec = false;
    jb = SfJob{};
    for (int i = 0; i < n_planes && !why; ++i) {
        const int64_t* d = desc + (size_t)i * SF_DESC_WORDS;
        SfPlane& P = jb.pl[i];
        const int64_t off = d[0], pitch = d[1], rows = d[2], groups = d[3], step = d[4];
        if (step != 1 && step != 2 && step != 4) { why = "step 1, 2 or 4"; break; }
        if (off < 0 || rows < 1 || groups < 1 || groups > 65536) { why = "a plane needs offset >= 0, rows >= 1 and 1 .. 65536 groups"; break; }
        const int64_t rb = groups * step * S;
        if (pitch < rb) { why = "pitch below the row's bytes"; break; }
        if (S == 2 && ((off | pitch) & 1)) { why = "odd plane offset or pitch with 16-bit samples"; break; }
        lo[i] = off;
        hi[i] = off + (rows - 1) * pitch + rb;
        if (hi[i] > surf_stride) { why = "surface_frame_bytes smaller than a plane's offset plus its rows"; break; }
        for (int j = 0; j < i; ++j)
            if (lo[i] < hi[j] && lo[j] < hi[i]) why = "surface planes overlap";
        int gfull = (int)groups;
        for (int k = 0; k < step; ++k) {
            const int64_t pl = d[5 + 3 * k], mul = d[6 + 3 * k], add = d[7 + 3 * k];
            if (pl < 0 || pl >= np || mul < 1 || mul > 2 || add < 0 || add >= mul) {
                why = "a stream needs a plane of the layout, mul 1 or 2 and 0 <= add < mul";
                break;
            }
            if (rows != prow[pl]) { why = "a surface plane has the rows of the planar planes it carries"; break; }
            if (mul * (groups - 1) >= pcol[pl] + mul - 1) { why = "more groups than the planar row has samples"; break; }
            P.poff[k] = pbase[pl];
            P.ppitch[k] = pcol[pl] * S;
            P.pw[k] = pcol[pl];
            P.mul[k] = (int)mul;
            P.add[k] = (int)add;
            const int full = pcol[pl] > (int)add ? (pcol[pl] - 1 - (int)add) / (int)mul + 1 : 0;          // groups whose sample of this stream exists
            gfull = full < gfull ? full : gfull;
        }
        if (why) break;
        P.off = off;
        P.pitch = pitch;
        P.rows = (int)rows;
        P.step = (int)step;
        P.row_bytes = (int)rb;
        // the vector form: the surface side aligned, and the streams in one of the three shapes it knows
        bool shape = surf16 && off % 16 == 0 && pitch % 16 == 0;
        if (step == 1) shape = shape && P.mul[0] == 1;
        else if (step == 2) shape = shape && P.mul[0] == 1 && P.mul[1] == 1 && d[5] != d[8];
        else {
            P.ya = P.yb = P.c0 = P.c1 = -1;
            for (int k = 0; k < 4; ++k) {
                if (P.mul[k] == 2) (P.add[k] == 0 ? P.ya : P.yb) = k;
                else (P.c0 < 0 ? P.c0 : P.c1) = k;
            }
            shape = shape && S == 1 && P.ya >= 0 && P.yb >= 0 && P.c0 >= 0 && P.c1 >= 0 && P.ya + P.yb + P.c0 + P.c1 == 6 &&
                    d[5 + 3 * P.ya] == d[5 + 3 * P.yb] && d[5 + 3 * P.c0] != d[5 + 3 * P.c1] && d[5 + 3 * P.c0] != d[5 + 3 * P.ya] &&
                    d[5 + 3 * P.c1] != d[5 + 3 * P.ya];
            if (!shape) P.ya = P.yb = P.c0 = P.c1 = 0;
        }
        const int ib = step == 1 ? 16 : 32;
        const int vb = shape ? (int)((int64_t)gfull * step * S / ib) * ib : 0;
        P.vec_bytes = vb;
        P.item_bytes = vb ? ib : S;
        P.items = (int)((rb + P.item_bytes - 1) / P.item_bytes);
        P.first = (int)first;
        first += (int64_t)P.items * rows;
        if (first > 0x7fffff00ll) { why = "a frame above 2^31 work items"; break; }
        vec = vec || vb > 0;
        span = hi[i] > span ? hi[i] : span;
        covered += rows * rb;
    }
    if (why) {
        snprintf(msg, sizeof msg, "%s: %s", who, why);
        return fail_arg(msg);
    }
    jb.in = pack ? planar : surf;
    jb.out = const_cast<uint8_t*>(pack ? surf : planar);
    jb.sstride = surf_stride;
    jb.pstride = planar_stride;
    jb.nplanes = n_planes;
    jb.total = (int)first;
    jb.shift = msb ? 16 - depth : 0;
    jb.top = (1u << depth) - 1u;
    return 0;
}

template <bool PACK>
int launch_surface(SfJob jb, int n_frames, int depth, int msb, bool vec, hipStream_t st) {
    const unsigned gx = (unsigned)((jb.total + SF_THREADS - 1) / SF_THREADS);
    const uint8_t* in = jb.in;
    uint8_t* out = jb.out;
    const long long sin = PACK ? jb.pstride : jb.sstride, sout = PACK ? jb.sstride : jb.pstride;
    for (int n0 = 0; n0 < n_frames; n0 += SF_MAX_Y) {          // (one launch up to 65535 frames)
        const int nn = n_frames - n0 < SF_MAX_Y ? n_frames - n0 : SF_MAX_Y;
        jb.in = in + (long long)n0 * sin;
        jb.out = out + (long long)n0 * sout;
        const dim3 grid(gx, (unsigned)nn);
        if (depth == 8) launch_form<PACK, 1, false>(jb, vec, grid, st);
        else if (msb) launch_form<PACK, 2, true>(jb, vec, grid, st);
        else launch_form<PACK, 2, false>(jb, vec, grid, st);
        if (int rc = check_launch("surface_kernel")) return rc;
    }
    return 0;
}

}  // namespace
}  // namespace savsr

using namespace savsr;

extern "C" int savsr_video_unpack_surface(const uint8_t* surface, int n_frames, int64_t surface_frame_bytes, int h, int w, int depth, int chroma,
                                          int msb, const int64_t* planes, int n_planes, uint8_t* planar, int64_t planar_frame_bytes, void* stream) {
    SfJob jb;
    int64_t span, covered;
    bool vec;
    if (int rc = build_job("video_unpack_surface", false, surface, planar, n_frames, surface_frame_bytes, planar_frame_bytes, h, w, depth, chroma, msb,
                           planes, n_planes, jb, span, covered, vec))
        return rc;
    return launch_surface<false>(jb, n_frames, depth, msb, vec, static_cast<hipStream_t>(stream));
}

extern "C" int savsr_video_pack_surface(const uint8_t* planar, int n_frames, int64_t planar_frame_bytes, int h, int w, int depth, int chroma, int msb,
                                        const int64_t* planes, int n_planes, uint8_t* surface, int64_t surface_frame_bytes, int64_t surface_bytes,
                                        void* stream) {
    SfJob jb;
    int64_t span, covered;
    bool vec;
    if (int rc = build_job("video_pack_surface", true, surface, planar, n_frames, surface_frame_bytes, planar_frame_bytes, h, w, depth, chroma, msb,
                           planes, n_planes, jb, span, covered, vec))
        return rc;
    if (surface_bytes < span || surface_bytes > surface_frame_bytes)
        return fail_arg("video_pack_surface: surface_bytes from the planes' last byte to surface_frame_bytes");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (covered != surface_bytes) {          // row padding or padded lines: zero the frames' resolved bytes, and only those
        hipError_t e = hipMemset2DAsync(surface, (size_t)surface_frame_bytes, 0, (size_t)surface_bytes, (size_t)n_frames, st);
        if (e != hipSuccess) { set_error("video_pack_surface: hipMemset2DAsync failed: %s", hipGetErrorString(e)); return (int)e; }
    }
    return launch_surface<true>(jb, n_frames, depth, msb, vec, st);
}
