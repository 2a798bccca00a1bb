// Host stand-ins for the few HIP and common.hpp names csrc/deinterlace.hip, csrc/pulldown.hip, csrc/surface.hip, csrc/scan.hip and their
// headers (csrc/video_samples.hpp, csrc/field_matrix.hpp) use, so that their device functions compile unchanged into a stand-alone host
// program (tools/check_deinterlace_host.py, check_pulldown_host.py, check_comb_host.py, check_surface_host.py, check_scan_host.py):
// a launch runs the kernel body one thread at a time over the grid, a memset is a memset, an atomic a plain read-modify-write, and
// set_error writes the message the program prints.  Host only; nothing here is loaded into Python or run on a GPU.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#define SAVSR_HOST_CHECK 1          // one thread at a time: the workgroup reductions take their per-thread branch
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
struct dim3 {
    unsigned x, y, z;
    dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
static dim3 threadIdx, blockIdx;
using std::max;
using std::min;
typedef void* hipStream_t;
typedef int hipError_t;
constexpr hipError_t hipSuccess = 0;
inline const char* hipGetErrorString(hipError_t) { return "host"; }
inline hipError_t hipMemsetAsync(void* p, int v, size_t bytes, hipStream_t) {
    memset(p, v, bytes);
    return hipSuccess;
}
inline hipError_t hipMemset2DAsync(void* p, size_t pitch, int v, size_t width, size_t height, hipStream_t) {
    for (size_t r = 0; r < height; ++r) memset((uint8_t*)p + r * pitch, v, width);
    return hipSuccess;
}
template <class T>
inline T atomicAdd(T* cell, T v) {
    const T old = *cell;
    *cell = old + v;
    return old;
}
template <class T>
inline T atomicMax(T* cell, T v) {
    const T old = *cell;
    *cell = old > v ? old : v;
    return old;
}
#define SAVSR_E_ARG (-1)
static char g_last_error[256];
namespace savsr {
typedef float f32x4 __attribute__((ext_vector_type(4)));
inline void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof g_last_error, fmt, ap);
    va_end(ap);
}
inline int fail_arg(const char* what) {
    snprintf(g_last_error, sizeof g_last_error, "invalid argument: %s", what);
    return SAVSR_E_ARG;
}
inline int check_launch(const char*) { return 0; }
}  // namespace savsr
template <class F>
void run_grid(F body, dim3 grid, dim3 block) {
    for (unsigned z = 0; z < grid.z; ++z)
        for (unsigned y = 0; y < grid.y; ++y)
            for (unsigned x = 0; x < grid.x; ++x)
                for (unsigned t = 0; t < block.x; ++t) {
                    blockIdx = dim3(x, y, z);
                    threadIdx = dim3(t, 0, 0);
                    body();
                }
}
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) run_grid([&]() { kernel(__VA_ARGS__); }, grid, block)
