// Stand-alone host program around csrc/dering.hip (built and driven by tools/check_dering_host.py under -fsanitize=address,undefined).
// argv: kind(8|16) n_frames frame_bytes plane_offset rows cols step depth interlaced pri sec damping out_frame_bytes out_plane_offset misalign in out
// The frames are read from `in` into a heap block that ends with the last frame's last byte and starts `misalign` bytes past a 16-byte
// boundary, the output frames go to a block of exactly their size (pre-filled with 0xA5, so the bytes around the plane must come back as
// they were), so an access outside either is a sanitizer report.  An entry's refusal is exit code 5 with the message on stderr.
#include "dering_device.inc"          // csrc/dering.hip with its include of common.hpp replaced by hip_stub.h

static uint8_t* place(size_t bytes, int misalign, uint8_t** raw) {
    for (size_t pad = 0; pad < 32; ++pad) {
        *raw = (uint8_t*)malloc(bytes + pad);
        if (((uintptr_t)(*raw + pad) & 15) == (unsigned)misalign) return *raw + pad;
        free(*raw);
    }
    return nullptr;
}

int main(int argc, char** argv) {
    if (argc != 18) return 2;
    const int kind = atoi(argv[1]), n = atoi(argv[2]);
    const long long fb = atoll(argv[3]), po = atoll(argv[4]);
    const int rows = atoi(argv[5]), cols = atoi(argv[6]), step = atoi(argv[7]), depth = atoi(argv[8]);
    const int interlaced = atoi(argv[9]), pri = atoi(argv[10]), sec = atoi(argv[11]), damping = atoi(argv[12]);
    const long long ofb = atoll(argv[13]), opo = atoll(argv[14]);
    const int mis = atoi(argv[15]);
    const size_t in_bytes = (size_t)n * fb, out_bytes = (size_t)n * ofb;
    uint8_t *raw_s, *raw_d;
    uint8_t* S = place(in_bytes, mis, &raw_s);
    uint8_t* D = place(out_bytes, mis, &raw_d);
    if (!S || !D) return 3;
    FILE* f = fopen(argv[16], "rb");
    if (!f || fread(S, 1, in_bytes, f) != in_bytes) return 4;
    fclose(f);
    memset(D, 0xA5, out_bytes);
    const int rc = kind == 8 ? savsr_video_dering_u8(S, n, fb, po, rows, cols, step, interlaced, pri, sec, damping, D, ofb, opo, nullptr)
                             : savsr_video_dering_u16(S, n, fb, po, rows, cols, step, depth, interlaced, pri, sec, damping, D, ofb, opo, nullptr);
    if (rc) {
        fprintf(stderr, "rc %d: %s\n", rc, g_last_error);
        free(raw_s);
        free(raw_d);
        return 5;
    }
    f = fopen(argv[17], "wb");
    fwrite(D, 1, out_bytes, f);
    fclose(f);
    free(raw_s);
    free(raw_d);
    return 0;
}
