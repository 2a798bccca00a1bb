// Stand-alone host program around csrc/grid.hip and the origin path of csrc/deblock.hip (built and driven by tools/check_grid_host.py
// under -fsanitize=address,undefined).
// argv: "stats" kind(8|16) n_frames frame_bytes plane_offset rows cols step depth interlaced cap calls misalign out_misalign in out
//       "deblock" kind(8|16) n_frames frame_bytes plane_offset rows cols step depth block strong interlaced thr_a thr_b origin_y origin_x misalign in out
// The frames are read from `in` into a heap block that ends with the last frame's last byte and starts `misalign` bytes past a 16-byte
// boundary, so an access outside it is a sanitizer report.  stats: the n_frames x 32 int64 cells are a heap block of exactly that size,
// zeroed once, and the entry is called `calls` times on it (the cells are added to); they are written to `out`.  deblock: the output
// frames go to a block of exactly their size pre-filled with 0xA5 (the bytes around the plane must come back as they were).  An entry's
// refusal is exit code 5 with the message on stderr.
#include "deblock_device.inc"          // csrc/deblock.hip with its include of common.hpp replaced by hip_stub.h
#include "grid_device.inc"             // csrc/grid.hip likewise

static uint8_t* place(size_t bytes, int misalign, uint8_t** raw) {
    for (size_t pad = 0; pad < 32; ++pad) {
        *raw = (uint8_t*)malloc(bytes + pad);
        if (((uintptr_t)(*raw + pad) & 15) == (unsigned)misalign) return *raw + pad;
        free(*raw);
    }
    return nullptr;
}

static int refused(int rc, uint8_t* a, uint8_t* b) {
    fprintf(stderr, "rc %d: %s\n", rc, g_last_error);
    free(a);
    free(b);
    return 5;
}

static int run_stats(char** v) {
    const int kind = atoi(v[0]), n = atoi(v[1]);
    const long long fb = atoll(v[2]), po = atoll(v[3]);
    const int rows = atoi(v[4]), cols = atoi(v[5]), step = atoi(v[6]), depth = atoi(v[7]), interlaced = atoi(v[8]), cap = atoi(v[9]);
    const int calls = atoi(v[10]), mis = atoi(v[11]), omis = atoi(v[12]);
    const size_t in_bytes = (size_t)(n > 0 ? n : 1) * (fb > 0 ? fb : 1), out_bytes = (size_t)(n > 0 ? n : 1) * 32 * sizeof(int64_t);
    uint8_t *raw_s, *raw_d;
    uint8_t* S = place(in_bytes, mis, &raw_s);
    uint8_t* D = place(out_bytes, omis, &raw_d);
    if (!S || !D) return 3;
    FILE* f = fopen(v[13], "rb");
    if (!f) return 4;
    const size_t got = fread(S, 1, in_bytes, f);
    fclose(f);
    if (got != in_bytes && n > 0 && fb > 0) return 4;
    memset(D, 0, out_bytes);
    for (int c = 0; c < calls; ++c) {
        const int rc = kind == 8 ? savsr_video_grid_stats_u8(S, n, fb, po, rows, cols, step, interlaced, cap, (int64_t*)D, nullptr)
                                 : savsr_video_grid_stats_u16(S, n, fb, po, rows, cols, step, depth, interlaced, cap, (int64_t*)D, nullptr);
        if (rc) return refused(rc, raw_s, raw_d);
    }
    f = fopen(v[14], "wb");
    fwrite(D, 1, out_bytes, f);
    fclose(f);
    free(raw_s);
    free(raw_d);
    return 0;
}

static int run_deblock(char** v) {
    const int kind = atoi(v[0]), n = atoi(v[1]);
    const long long fb = atoll(v[2]), po = atoll(v[3]);
    const int rows = atoi(v[4]), cols = atoi(v[5]), step = atoi(v[6]), depth = atoi(v[7]);
    const int block = atoi(v[8]), strong = atoi(v[9]), interlaced = atoi(v[10]), thr_a = atoi(v[11]), thr_b = atoi(v[12]);
    const int oy = atoi(v[13]), ox = atoi(v[14]), mis = atoi(v[15]);
    const size_t bytes = (size_t)n * fb;
    uint8_t *raw_s, *raw_d;
    uint8_t* S = place(bytes, mis, &raw_s);
    uint8_t* D = place(bytes, mis, &raw_d);
    if (!S || !D) return 3;
    FILE* f = fopen(v[16], "rb");
    if (!f || fread(S, 1, bytes, f) != bytes) return 4;
    fclose(f);
    memset(D, 0xA5, bytes);
    const int rc = kind == 8 ? savsr_video_deblock_u8_o(S, n, fb, po, rows, cols, step, block, strong, interlaced, thr_a, thr_b, D, fb, po, oy, ox, nullptr)
                             : savsr_video_deblock_u16_o(S, n, fb, po, rows, cols, step, depth, block, strong, interlaced, thr_a, thr_b, D, fb, po, oy, ox, nullptr);
    if (rc) return refused(rc, raw_s, raw_d);
    f = fopen(v[17], "wb");
    fwrite(D, 1, bytes, f);
    fclose(f);
    free(raw_s);
    free(raw_d);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 17 && !strcmp(argv[1], "stats")) return run_stats(argv + 2);
    if (argc == 20 && !strcmp(argv[1], "deblock")) return run_deblock(argv + 2);
    return 2;
}
