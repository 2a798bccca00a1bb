// What the field kernels share (deinterlace.hip, pulldown.hip, scan.hip): all of them work on one matrix inside resident frames -- a
// plane, or the h x (w * c) bytes of packed frames -- over a range of frames, as a `_u8` entry (rows x row_bytes bytes) and a `_u16` one
// (rows x cols little-endian 16-bit samples of depth 10 or 12).  Here, once: the matrix's descriptor and its builder from the entry
// arguments, the argument checks with the refusals' wording (`check_matrix`, the 16-bit clause, the output-cell and device-table
// clauses, `refuse`), the vector form's alignment test, the grid helpers (`blocks`, `for_frame_chunks`: at most 65535 frames per launch),
// the memset in front of the reducing kernels, the sample reader of the one-sample forms and the workgroup reduction (wave __shfl_xor,
// K x 4 LDS words, one 64-bit vector atomic per sum; the comb kernel's maximum beside a sum stays with it).  Included after
// video_samples.hpp; compiles under tools/host_check/hip_stub.h.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace savsr {

constexpr int FM_THREADS = 256;                     // lanes of a workgroup of the reducing kernels and the weave
constexpr int FM_MAX_FRAMES = 65535;                // grid.y / grid.z: frames per launch
constexpr long long FM_MAX_PLANE = 0x7fff0000ll;    // bytes of a plane: the lane tiles of a frame fit grid.x and 32-bit counts

// A matrix inside resident frames.  Rows are `pitch` bytes apart.
struct FieldMatrix {
    const uint8_t* src;          // the matrix of resident frame 0
    long long stride, pitch;     // bytes between frames / rows
    int n_frames, from;          // resident frames; the first frame of the launch
    int cols, rows;              // cols: samples of a row
    uint32_t top;               // 2^depth - 1
    int shift;                   // depth - 8
};

// width: row_bytes of a _u8 entry, cols of a _u16 one; depth 8 for _u8.
template <int BYTES>
inline FieldMatrix field_matrix(const uint8_t* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows, int width, int depth, int from) {
    return FieldMatrix{frames + plane_offset, frame_bytes, (long long)BYTES * width, n_frames, from, width, rows, (1u << depth) - 1u, depth - 8};
}

// The vector forms' condition: the matrix's base, frame stride and row pitch are multiples of 16 bytes.
inline bool aligned16(const void* base, long long stride, long long pitch) {
    return (reinterpret_cast<uintptr_t>(base) & 15) == 0 && stride % 16 == 0 && pitch % 16 == 0;
}

// How an entry's matrix check differs: the fewest rows (1 or 2), the deinterlacer's row ceiling (0: the plane limit instead), the range's
// wording and whether it may be empty.
struct MatrixRule {
    int min_rows, max_rows;
    const char* max_rows_why;
    const char* range_why;
    bool empty_ok;
};

// The checks of a matrix inside resident frames; nullptr or the reason.  order: 0 where the entry has none; out_plane_offset: 0 likewise.
inline const char* check_matrix(const MatrixRule& rule, const void* frames, int n_frames, int64_t frame_bytes, int64_t plane_offset, int rows,
                                int64_t row_bytes, int order, int from, int to, int64_t out_plane_offset = 0) {
    if (!frames) return "null pointer";
    if (n_frames < 1) return "n_frames >= 1";
    if (rows < rule.min_rows) return rule.min_rows == 2 ? "rows >= 2 (a matrix of one row has no second field)" : "rows >= 1";
    if (rule.max_rows && rows > rule.max_rows) return rule.max_rows_why;
    if (row_bytes < 1) return "a row holds at least one sample";
    if (!rule.max_rows && (long long)rows * row_bytes > FM_MAX_PLANE) return "a plane of at most 2147418112 bytes";
    if (order != 0 && order != 1) return "order 0 (tff) or 1 (bff)";
    if (from < 0 || to > n_frames || (rule.empty_ok ? from > to : from >= to)) return rule.range_why;
    if (plane_offset < 0 || out_plane_offset < 0) return "plane offsets >= 0";
    if (frame_bytes < plane_offset + (int64_t)rows * row_bytes) return "frame_bytes smaller than plane_offset plus the rows x row_bytes plane";
    return nullptr;
}

// The output side of the entries that write frames.
inline const char* check_out_plane(int64_t out_frame_bytes, int64_t out_plane_offset, int rows, int64_t row_bytes) {
    if (out_plane_offset < 0) return "plane offsets >= 0";
    if (out_frame_bytes < out_plane_offset + (int64_t)rows * row_bytes) return "out_frame_bytes smaller than out_plane_offset plus the rows x row_bytes plane";
    return nullptr;
}

inline int refuse(const char* who, const char* why) {
    char msg[192];
    snprintf(msg, sizeof msg, "%s: %s", who, why);
    return fail_arg(msg);
}

// The clause of every _u16 entry `who`: depth 10 or 12 (the message names the _u8 sibling: `who` with its "u16" read as "u8"), and frames,
// the frame stride and the plane offset 2-byte aligned -- with_out: those of the output frames as well.  0 or the refusal.
inline int check_samples16(const char* who, int depth, const void* frames, int64_t frame_bytes, int64_t plane_offset, bool with_out = false,
                           const void* out = nullptr, int64_t out_frame_bytes = 0, int64_t out_plane_offset = 0) {
    if (depth != 10 && depth != 12) {
        char why[96];
        const char* u = strstr(who, "u16");
        if (u) snprintf(why, sizeof why, "depth 10 or 12 (8 bits: savsr_%.*su8%s)", (int)(u - who), who, u + 3);
        return refuse(who, u ? why : "depth 10 or 12");
    }
    bool odd = (reinterpret_cast<uintptr_t>(frames) & 1) || ((frame_bytes | plane_offset) & 1);
    if (with_out) odd = odd || (reinterpret_cast<uintptr_t>(out) & 1) || ((out_frame_bytes | out_plane_offset) & 1);
    if (odd)
        return refuse(who, with_out ? "frames, out, the frame strides and the plane offsets must be 2-byte aligned (16-bit samples)"
                                    : "frames, the frame stride and the plane offset must be 2-byte aligned (16-bit samples)");
    return 0;
}

// The int64 cells of the reducing entries: there when the range is not empty, 8-byte aligned.
inline const char* check_cells(const int64_t* out, bool needed) {
    if (!out && needed) return "null pointer";
    return reinterpret_cast<uintptr_t>(out) & 7 ? "out must be 8-byte aligned" : nullptr;
}

// An int32 device table (delta, flags): there, 4-byte aligned.
inline const char* check_table(const int32_t* table, bool missing, const char* misaligned) {
    if (missing) return "null pointer";
    return reinterpret_cast<uintptr_t>(table) & 3 ? misaligned : nullptr;
}

inline unsigned blocks(long long units, int per_block) { return (unsigned)((units + per_block - 1) / per_block); }

// body(f0, nf) for the n_out frames of a call in launches of at most `max` frames; the first rc that is not 0.
template <class F>
inline int for_frame_chunks(int n_out, int max, F body) {
    for (int f0 = 0; f0 < n_out; f0 += max)
        if (int rc = body(f0, n_out - f0 < max ? n_out - f0 : max)) return rc;
    return 0;
}

// The memset in front of a reducing kernel: `per_frame` int64 cells for each of n_out frames.
inline int clear_cells(int64_t* out, int per_frame, int n_out, hipStream_t st, const char* what) {
    hipError_t e = hipMemsetAsync(out, 0, sizeof(int64_t) * per_frame * (size_t)n_out, st);
    if (e == hipSuccess) return 0;
    set_error("%s: hipMemsetAsync failed: %s", what, hipGetErrorString(e));
    return (int)e;
}

// Sample x of a row on the detectors' 8-bit scale.
template <int BYTES>
__device__ __forceinline__ uint32_t sample8(const uint8_t* row, uint32_t x, uint32_t top, int shift) {
    if constexpr (BYTES == 1) return row[x];
    else return msb8(reinterpret_cast<const uint16_t*>(row)[x], top, shift);
}

// The K lane sums of a workgroup of FM_THREADS lanes -> one 64-bit vector atomic per sum on cell[0], cell[STEP], ...  32-bit partials: a
// lane holds at most one row piece (its sums stay below 2^14, a workgroup's below 2^22), whatever the frame size.  A sum of 0 is not sent.
template <int K, int STEP>
__device__ __forceinline__ void block_reduce(const uint32_t (&acc)[K], unsigned long long* cell) {
#ifdef SAVSR_HOST_CHECK          // the host check runs one thread at a time: every thread adds its own sums
    for (int k = 0; k < K; ++k)
        if (acc[k]) atomicAdd(cell + STEP * k, (unsigned long long)acc[k]);
#else
    __shared__ uint32_t part[K][FM_THREADS / 64];
    uint32_t v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += __shfl_xor(v[k], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) part[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < K) {
        unsigned long long s = 0;
#pragma unroll
        for (int i = 0; i < FM_THREADS / 64; ++i) s += part[threadIdx.x][i];
        if (s) atomicAdd(cell + STEP * threadIdx.x, s);
    }
#endif
}

}  // namespace savsr
