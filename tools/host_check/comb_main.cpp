// Stand-alone host programs around the comb kernels (built and driven by tools/check_comb_host.py under -fsanitize=address,undefined).
// COMB_PART 1: csrc/pulldown.hip, savsr_video_comb_windows_u8 / _u16.  COMB_PART 2: csrc/deinterlace.hip, savsr_video_deinterlace_masked_u8
// / _u16.  (Two programs: the two sources are two translation units in the library as well.)
// argv: kind(8|16) n_frames frame_bytes plane_offset rows width step|depth order from to out_frame_bytes out_plane_offset misalign in out
//       threshold|method [flags]
// The frames are read from `in` into a heap block that ends with the last frame's last byte and starts `misalign` bytes past a 16-byte
// boundary; the counts / the output frames go to a block of exactly their size and the flags (part 2: to - from int32 read from `flags`)
// lie in one of exactly its size, so an access outside any of them is a sanitizer report.  SAVSR_HOST_CHECK: a launch runs one thread at
// a time, so the comb kernel's LDS cells are a static array that the workgroup's first thread clears and whose windows its last thread
// sums; everything else is the code the GPU runs.
#include "hip_stub.h"

#if COMB_PART == 1
#include "pulldown_device.inc"          // csrc/pulldown.hip with its include of common.hpp replaced by hip_stub.h
#else
#include "deinterlace_device.inc"       // csrc/deinterlace.hip, likewise
#endif

static uint8_t* place(size_t bytes, int misalign, uint8_t** raw) {
    for (size_t pad = 0; pad < 32; ++pad) {
        *raw = (uint8_t*)malloc(bytes + pad);
        if (((uintptr_t)(*raw + pad) & 15) == (unsigned)misalign) return *raw + pad;
        free(*raw);
    }
    return nullptr;
}

int main(int argc, char** argv) {
    if (argc != (COMB_PART == 1 ? 17 : 18)) return 2;
    const int kind = atoi(argv[1]), n = atoi(argv[2]);
    const long long fb = atoll(argv[3]), po = atoll(argv[4]);
    const int rows = atoi(argv[5]), width = atoi(argv[6]), sd = atoi(argv[7]), order = atoi(argv[8]), from = atoi(argv[9]), to = atoi(argv[10]);
    const long long ofb = atoll(argv[11]), opo = atoll(argv[12]);
    const int mis = atoi(argv[13]), tm = atoi(argv[16]);
    const size_t in_bytes = (size_t)n * fb;
    const size_t out_bytes = COMB_PART == 1 ? (size_t)(to - from) * 2 * sizeof(int64_t) : (size_t)(to - from) * ofb;
    uint8_t *raw_s, *raw_d;
    uint8_t* S = place(in_bytes, mis, &raw_s);
    uint8_t* D = place(out_bytes, COMB_PART == 1 ? 0 : mis, &raw_d);
    if (!S || !D) return 3;
    FILE* f = fopen(argv[14], "rb");
    if (!f || fread(S, 1, in_bytes, f) != in_bytes) return 4;
    fclose(f);
    memset(D, 0xA5, out_bytes);
    int rc;
#if COMB_PART == 1
    (void)ofb;
    (void)opo;
    rc = kind == 8 ? savsr_video_comb_windows_u8(S, n, fb, po, rows, width, sd, order, from, to, tm, (int64_t*)D, nullptr)
                   : savsr_video_comb_windows_u16(S, n, fb, po, rows, width, sd, order, from, to, tm, (int64_t*)D, nullptr);
#else
    int32_t* flags = (int32_t*)malloc(sizeof(int32_t) * (size_t)(to - from));
    f = fopen(argv[17], "rb");
    if (!f || fread(flags, sizeof(int32_t), (size_t)(to - from), f) != (size_t)(to - from)) return 4;
    fclose(f);
    rc = kind == 8 ? savsr_video_deinterlace_masked_u8(S, n, fb, po, rows, width, sd, order, from, to, D, ofb, opo, tm, flags, nullptr)
                   : savsr_video_deinterlace_masked_u16(S, n, fb, po, rows, width, sd, order, from, to, D, ofb, opo, tm, flags, nullptr);
    free(flags);
#endif
    if (rc) {
        fprintf(stderr, "rc %d: %s\n", rc, g_last_error);
        return 5;
    }
    f = fopen(argv[15], "wb");
    fwrite(D, 1, out_bytes, f);
    fclose(f);
    free(raw_s);
    free(raw_d);
    return 0;
}
