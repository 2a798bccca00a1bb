// Stand-alone host program around csrc/noise.hip (built and driven by tools/check_noise_host.py under -fsanitize=address,undefined).
// argv: kind(8|16) n_frames frame_bytes plane_offset rows cols step depth interlaced calls misalign out_misalign in out
// The frames are read from `in` into a heap block that ends with the last frame's last byte and starts `misalign` bytes past a 16-byte
// boundary, so an access outside it is a sanitizer report.  The n_frames x 256 x 2 int64 table is a heap block of exactly that size,
// zeroed once, and the entry is called `calls` times on it (the table is added to); it is written to `out`.  An entry's refusal is exit
// code 5 with the message on stderr.
#include "noise_device.inc"          // csrc/noise.hip with its include of common.hpp replaced by hip_stub.h

static uint8_t* place(size_t bytes, int misalign, uint8_t** raw) {
    for (size_t pad = 0; pad < 32; ++pad) {
        *raw = (uint8_t*)malloc(bytes + pad);
        if (((uintptr_t)(*raw + pad) & 15) == (unsigned)misalign) return *raw + pad;
        free(*raw);
    }
    return nullptr;
}

int main(int argc, char** argv) {
    if (argc != 15) return 2;
    char** v = argv + 1;
    const int kind = atoi(v[0]), n = atoi(v[1]);
    const long long fb = atoll(v[2]), po = atoll(v[3]);
    const int rows = atoi(v[4]), cols = atoi(v[5]), step = atoi(v[6]), depth = atoi(v[7]), interlaced = atoi(v[8]);
    const int calls = atoi(v[9]), mis = atoi(v[10]), omis = atoi(v[11]);
    const size_t in_bytes = (size_t)(n > 0 ? n : 1) * (fb > 0 ? fb : 1), out_bytes = (size_t)(n > 0 ? n : 1) * 512 * sizeof(int64_t);
    uint8_t *raw_s, *raw_d;
    uint8_t* S = place(in_bytes, mis, &raw_s);
    uint8_t* D = place(out_bytes, omis, &raw_d);
    if (!S || !D) return 3;
    FILE* f = fopen(v[12], "rb");
    if (!f) return 4;
    const size_t got = fread(S, 1, in_bytes, f);
    fclose(f);
    if (got != in_bytes && n > 0 && fb > 0) return 4;
    memset(D, 0, out_bytes);
    for (int c = 0; c < calls; ++c) {
        const int rc = kind == 8 ? savsr_video_noise_stats_u8(S, n, fb, po, rows, cols, step, interlaced, (int64_t*)D, nullptr)
                                 : savsr_video_noise_stats_u16(S, n, fb, po, rows, cols, step, depth, interlaced, (int64_t*)D, nullptr);
        if (rc) {
            fprintf(stderr, "rc %d: %s\n", rc, g_last_error);
            free(raw_s);
            free(raw_d);
            return 5;
        }
    }
    f = fopen(v[13], "wb");
    fwrite(D, 1, out_bytes, f);
    fclose(f);
    free(raw_s);
    free(raw_d);
    return 0;
}
