// Stand-alone host program around csrc/scan.hip (built and driven by tools/check_scan_host.py under -fsanitize=address,undefined).
// argv: op(0 stats_u8 | 1 stats_u16) n_frames frame_bytes plane_offset rows width depth lo hi misalign in out
// The frames are read from `in` into a heap block that ends with the last frame's last byte and starts `misalign` bytes past a 16-byte
// boundary; the sums go to a block of exactly their size, so an access outside either of them is a sanitizer report.
// SAVSR_HOST_CHECK: a launch runs one thread at a time, so scan.hip's workgroup reduction is replaced by its per-thread branch;
// everything else is the code the GPU runs.
#include "hip_stub.h"

#include "scan_device.inc"          // csrc/scan.hip with its include of common.hpp replaced by hip_stub.h

static uint8_t* place(size_t bytes, int misalign, uint8_t** raw) {
    for (size_t pad = 0; pad < 32; ++pad) {
        *raw = (uint8_t*)malloc(bytes + pad);
        if (((uintptr_t)(*raw + pad) & 15) == (unsigned)misalign) return *raw + pad;
        free(*raw);
    }
    return nullptr;
}

int main(int argc, char** argv) {
    if (argc != 13) return 2;
    const int op = atoi(argv[1]), n = atoi(argv[2]);
    const long long fb = atoll(argv[3]), po = atoll(argv[4]);
    const int rows = atoi(argv[5]), width = atoi(argv[6]), depth = atoi(argv[7]), lo = atoi(argv[8]), hi = atoi(argv[9]);
    const int mis = atoi(argv[10]);
    const size_t in_bytes = (size_t)n * fb;
    const size_t out_bytes = (size_t)(hi - lo) * 8 * sizeof(int64_t);
    uint8_t *raw_s, *raw_d;
    uint8_t* S = place(in_bytes, mis, &raw_s);
    uint8_t* D = place(out_bytes, 0, &raw_d);
    if (!S || !D) return 3;
    FILE* f = fopen(argv[11], "rb");
    if (!f || fread(S, 1, in_bytes, f) != in_bytes) return 4;
    fclose(f);
    memset(D, 0xA5, out_bytes);
    int rc;
    if (op == 0) rc = savsr_video_field_stats_u8(S, n, fb, po, rows, width, lo, hi, (int64_t*)D, nullptr);
    else rc = savsr_video_field_stats_u16(S, n, fb, po, rows, width, depth, lo, hi, (int64_t*)D, nullptr);
    if (rc) {
        fprintf(stderr, "rc %d: %s\n", rc, g_last_error);
        return 5;
    }
    f = fopen(argv[12], "wb");
    fwrite(D, 1, out_bytes, f);
    fclose(f);
    free(raw_s);
    free(raw_d);
    return 0;
}
