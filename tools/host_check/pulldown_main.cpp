// Stand-alone host program around csrc/pulldown.hip (built and driven by tools/check_pulldown_host.py under -fsanitize=address,undefined).
// argv: op(0 scores_u8 | 1 scores_u16 | 2 weave) n_frames frame_bytes plane_offset rows width depth order from to out_frame_bytes
//       out_plane_offset misalign in delta out
// The frames are read from `in` into a heap block that ends with the last frame's last byte and starts `misalign` bytes past a 16-byte
// boundary; the scores / the woven frames go to a block of exactly their size, the delta table (op 2: to - from int32 read from `delta`)
// lies in one of exactly its size, so an access outside any of them is a sanitizer report.  SAVSR_HOST_CHECK: a launch runs one thread
// at a time, so pulldown.hip's workgroup reduction is replaced by its per-thread branch; everything else is the code the GPU runs.
#include "hip_stub.h"

#include "pulldown_device.inc"          // csrc/pulldown.hip with its include of common.hpp replaced by hip_stub.h

static uint8_t* place(size_t bytes, int misalign, uint8_t** raw) {
    for (size_t pad = 0; pad < 32; ++pad) {
        *raw = (uint8_t*)malloc(bytes + pad);
        if (((uintptr_t)(*raw + pad) & 15) == (unsigned)misalign) return *raw + pad;
        free(*raw);
    }
    return nullptr;
}

int main(int argc, char** argv) {
    if (argc != 17) return 2;
    const int op = atoi(argv[1]), n = atoi(argv[2]);
    const long long fb = atoll(argv[3]), po = atoll(argv[4]);
    const int rows = atoi(argv[5]), width = atoi(argv[6]), depth = atoi(argv[7]), order = atoi(argv[8]), from = atoi(argv[9]), to = atoi(argv[10]);
    const long long ofb = atoll(argv[11]), opo = atoll(argv[12]);
    const int mis = atoi(argv[13]);
    const size_t in_bytes = (size_t)n * fb;
    const size_t out_bytes = op == 2 ? (size_t)(to - from) * ofb : (size_t)(to - from) * 2 * sizeof(int64_t);
    uint8_t *raw_s, *raw_d;
    uint8_t* S = place(in_bytes, mis, &raw_s);
    uint8_t* D = place(out_bytes, op == 2 ? mis : 0, &raw_d);
    if (!S || !D) return 3;
    FILE* f = fopen(argv[14], "rb");
    if (!f || fread(S, 1, in_bytes, f) != in_bytes) return 4;
    fclose(f);
    memset(D, 0xA5, out_bytes);
    int32_t* delta = nullptr;
    if (op == 2) {
        delta = (int32_t*)malloc(sizeof(int32_t) * (size_t)(to - from));
        f = fopen(argv[15], "rb");
        if (!f || fread(delta, sizeof(int32_t), (size_t)(to - from), f) != (size_t)(to - from)) return 4;
        fclose(f);
    }
    int rc;
    if (op == 0) rc = savsr_video_field_scores_u8(S, n, fb, po, rows, width, order, from, to, (int64_t*)D, nullptr);
    else if (op == 1) rc = savsr_video_field_scores_u16(S, n, fb, po, rows, width, depth, order, from, to, (int64_t*)D, nullptr);
    else rc = savsr_video_weave(S, n, fb, po, rows, width, order, from, to, delta, D, ofb, opo, nullptr);
    if (rc) {
        fprintf(stderr, "rc %d: %s\n", rc, g_last_error);
        return 5;
    }
    f = fopen(argv[16], "wb");
    fwrite(D, 1, out_bytes, f);
    fclose(f);
    free(raw_s);
    free(raw_d);
    free(delta);
    return 0;
}
