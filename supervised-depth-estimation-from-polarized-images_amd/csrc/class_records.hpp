// Per-image, per-class records: what pd_normals_stats (normals_stats.hip), pd_cloud_stats (pointcloud.hip), pd_depth_stats
// (depth_stats.hip) and pd_depth_consistency (consistency.hip) share.
//
// A record is: int64 n, `Counters` further int64 counters, `Sums` fp64 sums (two unless the evaluator asks for more), padding
// to 16 bytes, a uint32 histogram of `Bins` bins (Layout).  An evaluator fills its [N][K] records in three launches (run_records):
//   records_zero_kernel      clears the records (the integer fields are filled by atomic adds).
//   the evaluator's kernel   a workgroup of kThreads lanes belongs to one image; the image's work items go round-robin over
//                            its G workgroups (groups_for), a lane takes its items in increasing order.  Per workgroup: an
//                            LDS histogram [K][Bins] and LDS counters [Counters][kMaxK], filled with LDS integer atomics.
//                            Per lane: the fp64 sums of every class.  flush_records ends the kernel: the sums are
//                            reduced lane -> wave by a fixed shuffle tree and wave -> workgroup in index order, the
//                            workgroup's [K][Sums] partial sums go to the workspace with plain stores, and the counters and the
//                            histogram are flushed with one global add per non-zero word.
//   records_finalize_kernel  one workgroup per record: n = the sum of the record's bins, and the fp64 sums from the
//                            image's partials in index order.
// n, the counters and hist are integer sums: no order can change them.  The fp64 sums are bit-reproducible: the item ->
// lane assignment depends on the shape only, a lane adds its items in order, and every later step has a fixed order.  No
// floating-point atomics, no cross-workgroup ticket.
//
// A class is an inclusive range of the mask value, or every pixel (Classes, in_class, parse_classes).
#pragma once
#include "pd_common.h"

#include <algorithm>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxK = 16;                           // classes per call
constexpr int kMaxGroups = 64;                      // workgroups per image
constexpr long kItemsPerGroup = 4L * kThreads;      // below the cap a lane gets about four items
constexpr long kMaxImagesPerLaunch = 1L << 20;      // keeps gridDim.x = images * groups below 2^31

// lo > hi: every pixel.  By value in the kernel arguments: wave-uniform
struct Classes { int lo[kMaxK], hi[kMaxK]; };

__device__ __forceinline__ bool in_class(const Classes& cls, int k, int m) {
    return cls.lo[k] > cls.hi[k] || (m >= cls.lo[k] && m <= cls.hi[k]);
}

__device__ __forceinline__ bool in_range(float d, float lo, float hi) { return d >= lo && d <= hi; }      // NaN fails

// the caller's int[K][2] -> Classes, with the two refusals every entry point makes
inline int parse_classes(const char* who, const int* classes, int K, bool have_mask, Classes* cls) {
    PD_REQUIRE(K >= 1 && K <= kMaxK, "%s: K = %d classes, 1 .. %d are supported", who, K, kMaxK);
    for (int k = 0; k < kMaxK; ++k) {
        cls->lo[k] = k < K ? classes[2 * k] : 1;
        cls->hi[k] = k < K ? classes[2 * k + 1] : 0;
        PD_REQUIRE(k >= K || have_mask || cls->lo[k] > cls->hi[k],
                   "%s: class %d is the range [%d, %d] of the mask value, but mask is null", who, k, cls->lo[k], cls->hi[k]);
    }
    return PD_OK;
}

// Bins, the 64-bit counters after n, the 32-bit word where the histogram starts, the fp64 sums
template <int Bins, int Counters, int HistWord, int Sums = 2>
struct Layout {
    static constexpr int kBins = Bins, kCounters = Counters, kHistWord = HistWord, kNumSums = Sums;
    static constexpr int kSums = 1 + Counters;      // where the fp64 sums start, in 8-byte units
    static constexpr int kWords = HistWord + Bins, kBytes = 4 * kWords;
    static_assert(Sums >= 1 && Sums <= kWaves, "the finalize kernel adds one sum per wave");
    static_assert(4 * HistWord >= 8 * (kSums + Sums) && kBytes % 16 == 0, "record layout");
};

__global__ __launch_bounds__(kThreads) void records_zero_kernel(uint4* __restrict__ stats, long n16) {
    for (long i = blockIdx.x * (long)kThreads + threadIdx.x; i < n16; i += (long)gridDim.x * kThreads)
        stats[i] = make_uint4(0u, 0u, 0u, 0u);
}

// The end of an evaluator's kernel, called by every lane of workgroup blockIdx.x = img * G + grp.  s: the lane's sums;
// wsum: LDS [kWaves][kMaxK][Sums]; counters: LDS [Counters][kMaxK]; hist: LDS [K][Bins]; stats: the launch's records
template <class L>
__device__ __forceinline__ void flush_records(double (&s)[kMaxK][L::kNumSums], double* wsum, const unsigned* counters,
                                              const unsigned* hist, unsigned* __restrict__ stats, double* __restrict__ ws,
                                              unsigned img, int K) {
    constexpr int S = L::kNumSums;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // lanes -> wave by a fixed tree, waves -> workgroup in order
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
        if (k < K) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
                for (int j = 0; j < S; ++j) s[k][j] += __shfl_down(s[k][j], off);
            }
            if (lane == 0) {
#pragma unroll
                for (int j = 0; j < S; ++j) wsum[(wave * kMaxK + k) * S + j] = s[k][j];
            }
        }
    }
    __syncthreads();
    if (tid < S * K) {
        double t = 0.0;
        for (int w = 0; w < kWaves; ++w) t += wsum[w * kMaxK * S + tid];
        ws[((size_t)blockIdx.x * K) * S + tid] = t;      // [img][grp][k][Sums]
    }
    unsigned* rec = stats + (size_t)img * K * L::kWords;
#pragma unroll
    for (int c = 0; c < L::kCounters; ++c)
        if (tid < K && counters[c * kMaxK + tid])
            atomicAdd(reinterpret_cast<unsigned long long*>(rec + (size_t)tid * L::kWords) + 1 + c,
                      (unsigned long long)counters[c * kMaxK + tid]);
    for (int i = tid; i < K * L::kBins; i += kThreads) {
        const unsigned v = hist[i];
        if (v) {
            const int k = i / L::kBins;
            atomicAdd(rec + (size_t)k * L::kWords + L::kHistWord + (i - k * L::kBins), v);
        }
    }
}

// one workgroup per record [img][k]
template <class L>
__global__ __launch_bounds__(kThreads) void records_finalize_kernel(unsigned* __restrict__ stats, const double* __restrict__ ws,
                                                                    int K, int G) {
    __shared__ unsigned long long red[kThreads];
    const int tid = threadIdx.x;
    const unsigned img = blockIdx.x / K, k = blockIdx.x - img * K;
    unsigned* rec = stats + (size_t)blockIdx.x * L::kWords;
    unsigned long long acc = 0;
    for (int i = tid; i < L::kBins; i += kThreads) acc += rec[L::kHistWord + i];
    red[tid] = acc;
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    if (tid == 0) *reinterpret_cast<long long*>(rec) = (long long)red[0];
    constexpr int S = L::kNumSums;
    if ((tid & 63) == 0 && (tid >> 6) < S) {           // the first lane of wave j adds sum j, workgroups in index order
        const int which = tid >> 6;
        double t = 0.0;
        for (int gi = 0; gi < G; ++gi) t += ws[(((size_t)img * G + gi) * K + k) * S + which];
        reinterpret_cast<double*>(rec)[L::kSums + which] = t;
    }
}

// workgroups per image for `items` work items per image
inline int groups_for(long items) {
    return (int)std::min<long>(kMaxGroups, std::max<long>(1, (items + kItemsPerGroup - 1) / kItemsPerGroup));
}

// [N][G][K][sums] fp64 partial sums; never zero, a multiple of 16
inline size_t records_workspace(int N, int K, int G, int sums = 2) {
    const size_t n = N > 0 ? (size_t)N : 1, k = (size_t)std::min(std::max(K, 1), kMaxK);
    return n * (size_t)G * k * 8 * (size_t)((sums + 1) & ~1);
}

// zero -> stat -> finalize over the batch in chunks of kMaxImagesPerLaunch images.  stat(n0, nb, records, partials)
// launches the evaluator's kernel for images n0 .. n0 + nb - 1 on nb * G workgroups
template <class L, class Stat>
inline void run_records(void* stats, void* workspace, int N, int K, int G, hipStream_t st, Stat&& stat) {
    for (long n0 = 0; n0 < N; n0 += kMaxImagesPerLaunch) {
        const long nb = std::min<long>(kMaxImagesPerLaunch, N - n0);
        unsigned* rec = reinterpret_cast<unsigned*>(static_cast<unsigned char*>(stats) + (size_t)n0 * K * L::kBytes);
        double* part = static_cast<double*>(workspace) + (size_t)n0 * G * K * L::kNumSums;
        const long n16 = nb * K * (L::kBytes / 16);
        const int zgrid = (int)std::min<long>(1024, (n16 + kThreads - 1) / kThreads);
        hipLaunchKernelGGL(records_zero_kernel, dim3(zgrid), dim3(kThreads), 0, st, reinterpret_cast<uint4*>(rec), n16);
        stat(n0, nb, rec, part);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(records_finalize_kernel<L>), dim3((unsigned)(nb * K)), dim3(kThreads), 0, st, rec,
                           part, K, G);
    }
}

}  // namespace
