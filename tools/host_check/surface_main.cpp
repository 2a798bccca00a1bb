// Stand-alone host program around csrc/surface.hip (built and driven by tools/check_surface_host.py under -fsanitize=address,undefined).
// argv: op(0 unpack | 1 pack) n_frames surface_stride surface_bytes span h w depth chroma msb n_planes misalign in desc out
// `desc`: n_planes x 17 int64 words.  Unpack: the surface frames are read from `in` into a heap block that ends with the last frame's
// last byte that holds a sample (`span` bytes into it) and starts `misalign` bytes past a 16-byte boundary; the planar frames go to a
// block of exactly their size.  Pack: the planar frames lie in a block of exactly their size, the surface frames go to a block that ends
// with the last frame's resolved bytes (surface_bytes), prefilled with 0xA5.  An access outside any block is a sanitizer report.
#include "hip_stub.h"

#include "surface_device.inc"          // csrc/surface.hip with its include of common.hpp removed

static uint8_t* place(size_t bytes, int misalign, uint8_t** raw) {
    for (size_t pad = 0; pad < 32; ++pad) {
        *raw = (uint8_t*)malloc(bytes + pad);
        if (((uintptr_t)(*raw + pad) & 15) == (unsigned)misalign) return *raw + pad;
        free(*raw);
    }
    return nullptr;
}

static bool read_all(const char* path, void* to, size_t bytes) {
    FILE* f = fopen(path, "rb");
    const bool ok = f && fread(to, 1, bytes, f) == bytes;
    if (f) fclose(f);
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 16) return 2;
    const int op = atoi(argv[1]), n = atoi(argv[2]);
    const long long stride = atoll(argv[3]), sbytes = atoll(argv[4]), span = atoll(argv[5]);
    const int h = atoi(argv[6]), w = atoi(argv[7]), depth = atoi(argv[8]), chroma = atoi(argv[9]), msb = atoi(argv[10]), np = atoi(argv[11]);
    const int mis = atoi(argv[12]);
    const int S = depth == 8 ? 1 : 2;
    const int ch = chroma == 0 ? (h + 1) / 2 : h, cw = chroma <= 1 ? (w + 1) / 2 : w;
    const size_t fb = (size_t)S * ((size_t)h * w + (chroma == 3 ? 0 : 2 * (size_t)ch * cw));
    const size_t surf_bytes = (size_t)(n - 1) * stride + (op == 0 ? span : sbytes), planar_bytes = (size_t)n * fb;
    int64_t* desc = (int64_t*)malloc(sizeof(int64_t) * 17 * np);
    uint8_t *raw_s, *raw_p;
    uint8_t* SF = place(surf_bytes, mis, &raw_s);
    uint8_t* PL = place(planar_bytes, mis ? S : 0, &raw_p);          // (the planar side is aligned to its samples only)
    if (!SF || !PL || !desc) return 3;
    if (!read_all(argv[14], desc, sizeof(int64_t) * 17 * np)) return 4;
    int rc;
    if (op == 0) {
        if (!read_all(argv[13], SF, surf_bytes)) return 4;
        memset(PL, 0xA5, planar_bytes);
        rc = savsr_video_unpack_surface(SF, n, stride, h, w, depth, chroma, msb, desc, np, PL, (int64_t)fb, nullptr);
    } else {
        if (!read_all(argv[13], PL, planar_bytes)) return 4;
        memset(SF, 0xA5, surf_bytes);
        rc = savsr_video_pack_surface(PL, n, (int64_t)fb, h, w, depth, chroma, msb, desc, np, SF, stride, sbytes, nullptr);
    }
    if (rc) {
        fprintf(stderr, "rc %d: %s\n", rc, g_last_error);
        return 5;
    }
    FILE* f = fopen(argv[15], "wb");
    if (!f) return 6;
    if (op == 0) fwrite(PL, 1, planar_bytes, f);
    else fwrite(SF, 1, surf_bytes, f);
    fclose(f);
    free(raw_s);
    free(raw_p);
    free(desc);
    return 0;
}
