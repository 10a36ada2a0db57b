// Reductions over the 64 lanes of a wavefront, and the index decode of the flat grid-stride kernels.
//
// Every reducer is the xor butterfly with offsets 32, 16, ... 1: lane l combines with lane l ^ 32, the result with
// l ^ 16, and so on, so every lane ends with the same bits and the order of the operands is fixed.  The sums of
// frame_reduce.hpp, loss.hip and pose.hip are bit-reproducible because of that order: do not replace one of these with a
// __shfl_down tree (class_records.hpp has its own), whose order differs.
#pragma once
#include <hip/hip_runtime.h>

namespace pd_wave {

template <class T, class Op>
__device__ __forceinline__ T butterfly(T v, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) { return butterfly(v, [](float a, float b) { return a + b; }); }
__device__ __forceinline__ double wave_sum(double v) { return butterfly(v, [](double a, double b) { return a + b; }); }
// fminf / fmaxf: a NaN operand is skipped
__device__ __forceinline__ float wave_min(float v) { return butterfly(v, [](float a, float b) { return fminf(a, b); }); }
__device__ __forceinline__ float wave_max(float v) { return butterfly(v, [](float a, float b) { return fmaxf(a, b); }); }
__device__ __forceinline__ int wave_or(int v) { return butterfly(v, [](int a, int b) { return a | b; }); }

// i -> (i / d, i % d) for a positive divisor: 32-bit unsigned arithmetic whenever the index fits (every grid-stride index
// of the training step does); a 64-bit division is ~5x the instructions, and a pixel decode needs two or three
__device__ __forceinline__ long divmod(long i, int d, int& rem) {
    if (i >> 32) { const long q = i / d; rem = (int)(i - q * d); return q; }
    const unsigned u = (unsigned)i, q = u / (unsigned)d;
    rem = (int)(u - q * (unsigned)d);
    return (long)q;
}

}  // namespace pd_wave
