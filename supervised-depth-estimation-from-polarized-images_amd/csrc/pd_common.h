// Shared host-side helpers for libpolardepth.so (error reporting, launch checks, pointer alignment, grid sizes).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include "../../include/polardepth.h"

namespace pd {
char* err_buf();
int fail(int code, const char* fmt, ...);
inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(PD_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
    return PD_OK;
}
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Grids of the grid-stride kernels with 256 threads per workgroup.
constexpr int GRID_THREADS = 256;
// flat kernel over n work items: at most 2048 workgroups, at least 1
inline unsigned flat_grid(long n) {
    long b = (n + GRID_THREADS - 1) / GRID_THREADS;
    if (b > 2048) b = 2048;
    if (b < 1) b = 1;
    return (unsigned)b;
}
// blocks along x of a per-item grid (blockIdx.y = item, `per_item` work items each): about 4096 workgroups over the N
// items in all, the rest by grid stride; 1 for an empty shape
inline unsigned item_grid(int N, long per_item) {
    if (N <= 0 || per_item <= 0) return 1;
    long b = (per_item + GRID_THREADS - 1) / GRID_THREADS;
    const long cap = N >= 4096 ? 1 : 4096 / N;
    if (b > cap) b = cap;
    return (unsigned)(b < 1 ? 1 : b);
}
// PD_CONV_* flags of the convolution entry points: known bits only, and not two arithmetic requests at once
inline bool conv_flags_ok(unsigned f) {
    return (f & ~PD_CONV_FLAGS_ALL) == 0 && (f & (PD_CONV_FP32_MFMA | PD_CONV_BF16X3)) != (PD_CONV_FP32_MFMA | PD_CONV_BF16X3) &&
           !((f & PD_CONV_BF16) && (f & (PD_CONV_FP32_MFMA | PD_CONV_BF16X3)));
}
}  // namespace pd

#define PD_REQUIRE(cond, ...) \
    do { if (!(cond)) return pd::fail(PD_EINVAL, __VA_ARGS__); } while (0)
