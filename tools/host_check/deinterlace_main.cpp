// Stand-alone host program around csrc/deinterlace.hip (built and driven by tools/check_deinterlace_host.py under -fsanitize=address,undefined).
// argv: kind(8|16) n_frames frame_bytes plane_offset rows width step|depth order from to out_frame_bytes out_plane_offset misalign in out
//       [method rate]
// The frames are read from `in` into a heap block that ends with the last frame's last byte and starts `misalign` bytes past a 16-byte
// boundary, the output frames go to a block of exactly their size, so an access outside either is a sanitizer report.  With method (0
// yadif, 1 bwdif) and rate (0 double, 1 same) the `_m` entries run, and rate 1 gives the output block one frame per source frame.
#include "deinterlace_device.inc"          // csrc/deinterlace.hip with its include of common.hpp replaced by hip_stub.h

static uint8_t* place(size_t bytes, int misalign, uint8_t** raw) {
    for (size_t pad = 0; pad < 32; ++pad) {
        *raw = (uint8_t*)malloc(bytes + pad);
        if (((uintptr_t)(*raw + pad) & 15) == (unsigned)misalign) return *raw + pad;
        free(*raw);
    }
    return nullptr;
}

int main(int argc, char** argv) {
    if (argc != 16 && argc != 18) return 2;
    const bool m = argc == 18;
    const int kind = atoi(argv[1]), n = atoi(argv[2]);
    const long long fb = atoll(argv[3]), po = atoll(argv[4]);
    const int rows = atoi(argv[5]), width = atoi(argv[6]), sd = atoi(argv[7]), order = atoi(argv[8]), from = atoi(argv[9]), to = atoi(argv[10]);
    const long long ofb = atoll(argv[11]), opo = atoll(argv[12]);
    const int mis = atoi(argv[13]);
    const int method = m ? atoi(argv[16]) : 0, rate = m ? atoi(argv[17]) : 0;
    const size_t in_bytes = (size_t)n * fb, out_bytes = (size_t)(rate == 1 ? 1 : 2) * (to - from) * ofb;
    uint8_t *raw_s, *raw_d;
    uint8_t* S = place(in_bytes, mis, &raw_s);
    uint8_t* D = place(out_bytes, mis, &raw_d);
    if (!S || !D) return 3;
    FILE* f = fopen(argv[14], "rb");
    if (!f || fread(S, 1, in_bytes, f) != in_bytes) return 4;
    fclose(f);
    memset(D, 0xA5, out_bytes);
    int rc;
    if (m)
        rc = kind == 8 ? savsr_video_deinterlace_u8_m(S, n, fb, po, rows, width, sd, order, from, to, D, ofb, opo, method, rate, nullptr)
                       : savsr_video_deinterlace_u16_m(S, n, fb, po, rows, width, sd, order, from, to, D, ofb, opo, method, rate, nullptr);
    else
        rc = kind == 8 ? savsr_video_deinterlace_u8(S, n, fb, po, rows, width, sd, order, from, to, D, ofb, opo, nullptr)
                       : savsr_video_deinterlace_u16(S, n, fb, po, rows, width, sd, order, from, to, D, ofb, opo, nullptr);
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
