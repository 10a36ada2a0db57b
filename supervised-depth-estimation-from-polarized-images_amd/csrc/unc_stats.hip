// Calibration and sparsification of the depth uncertainty per pixel class in ONE read of the batch (pd_unc_stats): is the
// scale b the network states for a pixel the size of the error it makes there, and does removing the pixels it trusts least
// remove the error?  Definition, record and tables: include/polardepth.h; NumPy statement: tests/unc_stats_ref.py.  The
// records, their three launches and why the sums are bit-reproducible: class_records.hpp.
//
// ustat_kernel: one work item = one pixel; the pixel set, the clamp and the 0.5 mm error bin are those of dstat_kernel
// (depth_stats.hip).  Besides the record (counters bad, cover50, cover90; fp64 sums of the negative log-likelihood, of b and
// of the error; the histogram of the uncertainty bin ub) a class has three 512-entry tables of 64-bit integers from which
// the host draws the sparsification curves: sum e_um by ub, count by eb, sum e_um by eb (e_um = the error in whole
// micrometres).  A class's histogram and tables take 14 KiB of LDS, so the classes are served kChunk at a time: per chunk
// the workgroup clears its LDS, goes over its pixels again (a pixel in none of the chunk's classes costs four loads), fills
// the LDS with integer atomics and adds every non-zero word to global memory with one integer atomic.  Integer sums: no
// order can change them.
#include "class_records.hpp"

#include <cmath>

namespace {

using Rec = Layout<PD_USTAT_BINS, PD_USTAT_COUNTERS, 16, PD_USTAT_SUMS>;      // the histogram starts at byte 64
constexpr int kBins = Rec::kBins;
constexpr int kEdges = kBins - 1;
constexpr int kSums = Rec::kNumSums;
constexpr int kCounters = Rec::kCounters;
constexpr int kRows = PD_USTAT_TABLE_ROWS;
constexpr int kChunk = 4;                           // classes per LDS fill
constexpr double kLn2 = 0.6931471805599453, kLn10 = 2.302585092994046;      // M_LN2, M_LN10

static_assert(64 + 4 * kBins == PD_USTAT_RECORD_BYTES && Rec::kBytes == PD_USTAT_RECORD_BYTES, "record layout");
static_assert(kSums == 3 && kCounters == 3 && kRows == 3 && kBins == 512 && kBins == PD_DSTAT_BINS, "record layout");
static_assert(kMaxK == PD_DSTAT_MAX_CLASSES, "class limit");
enum { cBad = 0, cCover50 = 1, cCover90 = 2 };

struct Geo {
    unsigned P;                   // pixels per image
    unsigned G;                   // workgroups per image
    int K;
    float min_d, max_d;
    double log_lo, log_ratio;     // log b_lo, log(b_hi / b_lo)
};

// tables: [image][K][3][512] of this launch
__global__ __launch_bounds__(kThreads) void ustat_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                         const float* __restrict__ unc, const int* __restrict__ mask,
                                                         const double* __restrict__ edges_g, unsigned* __restrict__ stats,
                                                         unsigned long long* __restrict__ tables, double* __restrict__ ws,
                                                         Classes cls, Geo g) {
    extern __shared__ __align__(16) unsigned char smem[];
    double* edges = reinterpret_cast<double*>(smem);                                        // [512], the last one is padding
    double* wsum = edges + kBins;                                                           // [kWaves][kMaxK][3]
    unsigned long long* tab = reinterpret_cast<unsigned long long*>(wsum + kWaves * kMaxK * kSums);      // [kChunk][3][512]
    unsigned* hist = reinterpret_cast<unsigned*>(tab + kChunk * kRows * kBins);             // [kChunk][512]
    unsigned* counters = hist + kChunk * kBins;                                             // [3][kMaxK]
    const int tid = threadIdx.x;
    const int K = g.K;
    const unsigned img = blockIdx.x / g.G, grp = blockIdx.x - img * g.G;
    for (int i = tid; i < kBins; i += kThreads) edges[i] = i < kEdges ? edges_g[i] : (double)INFINITY;
    if (tid < kCounters * kMaxK) counters[tid] = 0;

    const size_t base = (size_t)img * g.P;
    const float* gt_f = gt + base;
    const float* pred_f = pred + base;
    const float* unc_f = unc + base;
    const int* mask_f = mask ? mask + base : nullptr;
    unsigned* rec = stats + (size_t)img * K * Rec::kWords;
    unsigned long long* tab_g = tables + (size_t)img * K * kRows * kBins;

    double s[kMaxK][kSums];
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
#pragma unroll
        for (int j = 0; j < kSums; ++j) s[k][j] = 0.0;

    for (int c0 = 0; c0 < K; c0 += kChunk) {
        const int nc = min(kChunk, K - c0);
        __syncthreads();                                                                    // the previous chunk's flush is over
        for (int i = tid; i < kChunk * kRows * kBins; i += kThreads) tab[i] = 0ull;
        for (int i = tid; i < kChunk * kBins; i += kThreads) hist[i] = 0u;
        __syncthreads();

        // pixels of this image go round-robin over its G workgroups, a lane takes them in increasing order
        for (unsigned item = grp * kThreads + tid; item < g.P; item += g.G * kThreads) {
            const float gv = gt_f[item];
            const float pv = pred_f[item];
            const float uv = unc_f[item];
            const int m = mask_f ? mask_f[item] : 0;
            if (!(gv > g.min_d && gv < g.max_d)) continue;                                   // NaN fails
            unsigned member = 0;
#pragma unroll
            for (int j = 0; j < kChunk; ++j)
                if (j < nc && in_class(cls, c0 + j, m)) member |= 1u << j;
            if (!member) continue;
            const bool ok = __builtin_isfinite(pv) && uv >= 0.f && uv <= 1.f;               // a NaN u fails
            if (!ok) {
#pragma unroll
                for (int j = 0; j < kChunk; ++j)
                    if (member >> j & 1u) atomicAdd(&counters[cBad * kMaxK + c0 + j], 1u);
                continue;
            }
            const float p0 = fminf(fmaxf(pv, g.min_d), g.max_d);
            const double e = fabs(__dadd_rn((double)gv, -(double)p0));
            const double logb = fma((double)uv, g.log_ratio, g.log_lo);
            const double b = exp(logb);
            const double t[kSums] = {e / b + (logb + kLn2), b, e};
            const bool c50 = e <= __dmul_rn(b, kLn2), c90 = e <= __dmul_rn(b, kLn10);
            const unsigned long long e_um = (unsigned long long)rint(__dmul_rn(e, 1e6));
            const int ub = min(kBins - 1, (int)(uv * 512.f));
            int lo = 0, hi = kEdges;
#pragma unroll 1
            for (int it = 0; it < 9; ++it) {              // 2^9 > 511; the search of dstat_kernel
                const int mid = (lo + hi) >> 1;
                const bool le = lo < hi && edges[mid] <= e;
                const bool gtb = lo < hi && !le;
                lo = le ? mid + 1 : lo;
                hi = gtb ? mid : hi;
            }
            const int eb = lo;
#pragma unroll
            for (int j = 0; j < kChunk; ++j) {
                if (member >> j & 1u) {
                    atomicAdd(&hist[j * kBins + ub], 1u);
                    atomicAdd(&tab[(j * kRows + 0) * kBins + ub], e_um);
                    atomicAdd(&tab[(j * kRows + 1) * kBins + eb], 1ull);
                    atomicAdd(&tab[(j * kRows + 2) * kBins + eb], e_um);
                    if (c50) atomicAdd(&counters[cCover50 * kMaxK + c0 + j], 1u);
                    if (c90) atomicAdd(&counters[cCover90 * kMaxK + c0 + j], 1u);
                }
            }
#pragma unroll
            for (int k = 0; k < kMaxK; ++k) {             // the register file is indexed at compile time
                const int j = k - c0;
                if (j >= 0 && j < kChunk && (member >> (j & (kChunk - 1)) & 1u)) {
#pragma unroll
                    for (int q = 0; q < kSums; ++q) s[k][q] += t[q];
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < nc * kBins; i += kThreads) {
            const unsigned v = hist[i];
            if (v) {
                const int j = i / kBins;
                atomicAdd(rec + (size_t)(c0 + j) * Rec::kWords + Rec::kHistWord + (i - j * kBins), v);
            }
        }
        for (int i = tid; i < nc * kRows * kBins; i += kThreads) {
            const unsigned long long v = tab[i];
            if (v) atomicAdd(tab_g + (size_t)c0 * kRows * kBins + i, v);
        }
    }

    // the sums and the counters, as flush_records does them: lanes -> wave by a fixed tree, waves -> workgroup in order
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
        if (k < K) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
                for (int j = 0; j < kSums; ++j) s[k][j] += __shfl_down(s[k][j], off);
            }
            if (lane == 0) {
#pragma unroll
                for (int j = 0; j < kSums; ++j) wsum[(wave * kMaxK + k) * kSums + j] = s[k][j];
            }
        }
    }
    __syncthreads();
    if (tid < kSums * K) {
        double t = 0.0;
        for (int w = 0; w < kWaves; ++w) t += wsum[w * kMaxK * kSums + tid];
        ws[((size_t)blockIdx.x * K) * kSums + tid] = t;      // [img][grp][k][3]
    }
#pragma unroll
    for (int c = 0; c < kCounters; ++c)
        if (tid < K && counters[c * kMaxK + tid])
            atomicAdd(reinterpret_cast<unsigned long long*>(rec + (size_t)tid * Rec::kWords) + 1 + c,
                      (unsigned long long)counters[c * kMaxK + tid]);
}

inline int groups_of(int H, int W) { return groups_for(H > 0 && W > 0 ? (long)H * W : 0); }      // items: pixels

constexpr size_t kLdsBytes = (size_t)kBins * 8 + (size_t)kWaves * kMaxK * kSums * 8 + (size_t)kChunk * kRows * kBins * 8 +
                             (size_t)kChunk * kBins * 4 + (size_t)kCounters * kMaxK * 4;
static_assert(kLdsBytes <= 64 * 1024, "one workgroup's LDS");

}  // namespace

extern "C" size_t pd_unc_stats_workspace(int N, int H, int W, int K) {
    return records_workspace(N, K, groups_of(H, W), kSums);
}

extern "C" int pd_unc_stats(const void* gt, const void* pred, const void* unc, const void* mask, const int* classes, int K,
                            const void* edges, double b_lo, double b_hi, void* stats, void* tables, void* workspace,
                            size_t ws_bytes, int N, int H, int W, float min_depth, float max_depth, void* stream) {
    const char* who = "pd_unc_stats";
    PD_REQUIRE(N >= 0 && H > 0 && W > 0, "%s: bad shape (N = %d, H = %d, W = %d)", who, N, H, W);
    PD_REQUIRE(gt && pred && unc && classes, "%s: gt, pred, unc and classes must not be null", who);
    PD_REQUIRE(min_depth > 0.f, "%s: min_depth = %g must be positive", who, (double)min_depth);
    PD_REQUIRE(max_depth > min_depth, "%s: max_depth = %g must be above min_depth = %g", who, (double)max_depth, (double)min_depth);
    PD_REQUIRE(max_depth <= (float)PD_USTAT_MAX_DEPTH,
               "%s: max_depth = %g must be finite and at most %d m: the tables add errors in whole micrometres", who,
               (double)max_depth, PD_USTAT_MAX_DEPTH);
    PD_REQUIRE(b_lo > 0.0 && b_lo < b_hi && std::isfinite(b_hi), "%s: the scale range needs 0 < b_lo < b_hi < inf, got (%g, %g)", who,
               b_lo, b_hi);
    PD_REQUIRE((long)H * W <= (1L << 30), "%s: a frame of %d x %d is too large for the kernel's index arithmetic", who, H, W);
    PD_REQUIRE(edges && stats && tables && workspace, "%s: edges, stats, tables and workspace must not be null", who);
    Classes cls;
    if (int e = parse_classes(who, classes, K, mask != nullptr, &cls)) return e;
    PD_REQUIRE(pd::aligned16(stats) && pd::aligned16(tables) && pd::aligned16(workspace),
               "%s: stats, tables and workspace must be 16-byte aligned", who);
    const size_t need = pd_unc_stats_workspace(N, H, W, K);
    PD_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu bytes, pd_unc_stats_workspace asks for %zu)", who, ws_bytes, need);
    if (N == 0) return PD_OK;
    hipStream_t st = (hipStream_t)stream;
    Geo g;
    g.P = (unsigned)((long)H * W); g.G = (unsigned)groups_of(H, W); g.K = K; g.min_d = min_depth; g.max_d = max_depth;
    g.log_lo = std::log(b_lo); g.log_ratio = std::log(b_hi / b_lo);
    run_records<Rec>(stats, workspace, N, K, (int)g.G, st, [&](long n0, long nb, unsigned* rec, double* part) {
        unsigned long long* tab = static_cast<unsigned long long*>(tables) + (size_t)n0 * K * kRows * kBins;
        const long n16 = nb * K * (long)(kRows * kBins * 8 / 16);
        const int zgrid = (int)std::min<long>(1024, (n16 + kThreads - 1) / kThreads);
        hipLaunchKernelGGL(records_zero_kernel, dim3(zgrid), dim3(kThreads), 0, st, reinterpret_cast<uint4*>(tab), n16);
        hipLaunchKernelGGL(ustat_kernel, dim3((unsigned)(nb * g.G)), dim3(kThreads), kLdsBytes, st,
                           static_cast<const float*>(gt) + (size_t)n0 * g.P, static_cast<const float*>(pred) + (size_t)n0 * g.P,
                           static_cast<const float*>(unc) + (size_t)n0 * g.P,
                           mask ? static_cast<const int*>(mask) + (size_t)n0 * g.P : nullptr, static_cast<const double*>(edges),
                           rec, tab, part, cls, g);
    });
    return pd::check_launch(who);
}
