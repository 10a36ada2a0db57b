// Shared by csrc/reproj.hip (pd_reproj_combine_*) and csrc/student.hip (pd_student_combine_*): the per-pixel minimum / mean
// over the valid neighbouring frames, the two-stage fp64 reduction of K masked sums in a fixed order, and the argument check
// of their entry points.
//
// Order of the sums (what makes them bit-reproducible): per thread over its grid-stride pixels, per wavefront by xor
// shuffles (32, 16, ... 1), per workgroup ((w0 + w1) + w2) + w3 over its four wavefronts, one row of K doubles per
// workgroup; then ONE workgroup of 256 threads: thread t adds rows t, t + 256, ... and a binary tree over LDS adds the 256.
#pragma once
#include "pd_common.h"
#include "wave_ops.hpp"

namespace pd_frames {

constexpr int RT = pd::GRID_THREADS;   // threads per workgroup of every kernel that uses block_rows / finalize_rows
constexpr int MAX_FRAMES = 8;      // = PD_REPROJ_MAX_FRAMES

struct FrameArgs {
    const float* reproj[MAX_FRAMES];
    const float* identity[MAX_FRAMES];
    float* greproj[MAX_FRAMES];
};

// one value over the valid frames of a pixel: the minimum and its frame (the first valid frame is taken, a later one only
// when it is strictly smaller: the earlier frame wins a tie), or the mean (sum in frame order / number of valid frames,
// frame 0 reported).  Without a valid frame: 0, arg 255.
struct OverFrames {
    float m = 0.f;
    int nvalid = 0, arg = 255;
    __device__ __forceinline__ void add(float r, int f, int avg) {
        ++nvalid;
        if (avg) m += r;
        else if (arg == 255 || r < m) { m = r; arg = f; }
    }
    __device__ __forceinline__ void finish(int avg) {
        if (avg && nvalid) { m = m / (float)nvalid; arg = 0; }
    }
};

__device__ __forceinline__ float over_frames(const float* const* maps, const float* __restrict__ vrow, int F, long i, int avg,
                                             int& nvalid, int& arg) {
    OverFrames o;
    for (int f = 0; f < F; ++f) {
        if (vrow && vrow[f] == 0.f) continue;
        o.add(maps[f][i], f, avg);
    }
    o.finish(avg);
    nvalid = o.nvalid;
    arg = o.arg;
    return o.m;
}

// the workgroup's K sums -> partial[blockIdx.x * K + k]; sm: RT / 64 * K doubles of LDS.  Every thread must call it.
template <int K>
__device__ __forceinline__ void block_rows(double (&acc)[K], double* sm, double* __restrict__ partial) {
    static_assert(RT == 256, "four wavefronts per workgroup");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double v = pd_wave::wave_sum(acc[k]);
        if (lane == 0) sm[wave * K + k] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            partial[blockIdx.x * (long)K + k] = ((sm[k] + sm[K + k]) + sm[2 * K + k]) + sm[3 * K + k];
    }
}

// one workgroup of 256 threads: out[k] (valid in thread 0) = the sum of column k over the rows; sm: K * 256 doubles of LDS
template <int K>
__device__ __forceinline__ void finalize_rows(const double* __restrict__ partial, int rows, double* sm, double (&out)[K]) {
    double a[K];
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = 0.0;
    for (int r = threadIdx.x; r < rows; r += 256) {
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] += partial[(long)K * r + k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) sm[k * 256 + threadIdx.x] = a[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int k = 0; k < K; ++k) sm[k * 256 + threadIdx.x] += sm[k * 256 + threadIdx.x + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = sm[k * 256];
}

// the frame count, shape and `avg` of the pd_*_combine_* entry points
inline int combine_args(const char* who, int F, int N, int H, int W, int avg) {
    PD_REQUIRE(F >= 1 && F <= MAX_FRAMES, "%s: 1 <= F <= %d frames, got %d", who, MAX_FRAMES, F);
    PD_REQUIRE(N >= 0 && H > 0 && W > 0, "%s: bad shape N=%d H=%d W=%d", who, N, H, W);
    PD_REQUIRE((long)H * W <= (1L << 30), "%s: image too large (%d x %d)", who, H, W);
    PD_REQUIRE(avg == 0 || avg == 1, "%s: avg must be 0 or 1, got %d", who, avg);
    return PD_OK;
}

}  // namespace pd_frames
