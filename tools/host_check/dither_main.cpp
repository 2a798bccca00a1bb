// Stand-alone host program around csrc/dither.hpp (built and driven by tools/check_dither_host.py under -fsanitize=address,undefined).
// argv: op out [in n [mul]]
//   0  the 256 thresholds theta(y, x), y-major, as float32
//   1  n float32 values t from `in`: dither_floor(t, y, x) at all 256 positions -> n * 256 float32
//   2  n float32 values v from `in`: dither_quant_unit(v, mul, theta(y, x)) at all 256 positions -> n * 256 uint32
//   3  n pairs (int64 p, int64 W) from `in`: dither_row_col -> n pairs of uint32 (y, x)
// Every buffer is a heap block of exactly its size, so an access outside one is a sanitizer report.  Positions are given as
// (y + 16 a, x + 16 b) for a few a, b as well: the rule reads the coordinates' low four bits only.
#include <cstdio>
#include <cstdlib>

#include "dither.hpp"

template <class T> static T* read_block(const char* path, size_t n) {
    T* p = (T*)malloc(n * sizeof(T));
    FILE* f = fopen(path, "rb");
    if (!p || !f || fread(p, sizeof(T), n, f) != n) exit(4);
    fclose(f);
    return p;
}

template <class T> static void write_block(const char* path, const T* p, size_t n) {
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(p, sizeof(T), n, f) != n) exit(5);
    fclose(f);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const int op = atoi(argv[1]);
    const char* out = argv[2];
    if (op == 0) {
        float* th = (float*)malloc(256 * sizeof(float));
        for (uint32_t y = 0; y < 16; ++y)
            for (uint32_t x = 0; x < 16; ++x) {
                th[16 * y + x] = savsr::dither_theta(y, x);
                float t4[4];
                savsr::dither_theta4(y + 32, (x & ~3u) + 16, t4);          // (the vector forms' four thresholds from one matrix entry)
                if (t4[x & 3u] != th[16 * y + x]) return 7;
                for (uint32_t a = 1; a < 4; ++a)
                    if (savsr::dither_theta(y + 16 * a, x + 48 * a) != th[16 * y + x]) return 6;          // (the pattern's period)
            }
        write_block(out, th, 256);
        free(th);
        return 0;
    }
    if (argc < 5) return 2;
    const size_t n = (size_t)atoll(argv[4]);
    if (op == 1 || op == 2) {
        const float mul = argc > 5 ? (float)atof(argv[5]) : 0.f;
        float* t = read_block<float>(argv[3], n);
        float* qf = op == 1 ? (float*)malloc(n * 256 * sizeof(float)) : nullptr;
        uint32_t* qu = op == 2 ? (uint32_t*)malloc(n * 256 * sizeof(uint32_t)) : nullptr;
        for (size_t i = 0; i < n; ++i)
            for (uint32_t y = 0; y < 16; ++y)
                for (uint32_t x = 0; x < 16; ++x) {
                    if (op == 1) qf[i * 256 + 16 * y + x] = savsr::dither_floor(t[i], y + 16 * (uint32_t)(i & 3), x + 16 * (uint32_t)(i & 7));
                    else qu[i * 256 + 16 * y + x] = savsr::dither_quant_unit(t[i], mul, savsr::dither_theta(y, x + 32));
                }
        if (op == 1) write_block(out, qf, n * 256);
        else write_block(out, qu, n * 256);
        free(t);
        free(qf);
        free(qu);
        return 0;
    }
    if (op == 3) {
        long long* pw = read_block<long long>(argv[3], 2 * n);
        uint32_t* yx = (uint32_t*)malloc(2 * n * sizeof(uint32_t));
        for (size_t i = 0; i < n; ++i) savsr::dither_row_col(pw[2 * i], savsr::dither_div((int)pw[2 * i + 1]), yx[2 * i], yx[2 * i + 1]);
        write_block(out, yx, 2 * n);
        free(pw);
        free(yx);
        return 0;
    }
    return 2;
}
