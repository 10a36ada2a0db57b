// Depth accuracy per pixel class in ONE read of the batch (pd_depth_stats), and the exact per-class medians that median
// scaling needs (pd_depth_medians).  Definition, record and the selection scheme: include/polardepth.h.  The records, their
// three launches and why the sums are bit-reproducible: class_records.hpp.
//
// dstat_kernel: one work item = one pixel, so every load of a wave is one contiguous 256-byte run.  Without a scale the
// pixel's terms are computed once and added to each of its classes; with a scale the prediction differs from class to class
// and the terms are computed per class.  The counters are a1, a2, a3, bad.  The bin of a pixel is the number of table entries
// edges[j] <= |d|, found by a nine-step binary search over a copy of the caller's 511 doubles in LDS.
//
// dmed_hist_kernel / dmed_select_kernel: a radix selection over the fp32 bit pattern, eight bits a pass.  Per (image, class)
// four selections run side by side -- c = 0, 1: ranks (n-1)/2 and n/2 of gt; c = 2, 3: the same of the clamped prediction --
// each with its own prefix of chosen digits and its own rank among the values that match the prefix.  In the first pass the
// two ranks of a quantity share one histogram (c = 0 and c = 2), since no digit is chosen yet.
#include "class_records.hpp"

#include <cmath>

namespace {

using Rec = Layout<PD_DSTAT_BINS, PD_DSTAT_COUNTERS, 20, PD_DSTAT_SUMS>;      // the histogram starts at byte 80
constexpr int kBins = Rec::kBins;
constexpr int kEdges = kBins - 1;
constexpr int kSums = Rec::kNumSums;
constexpr int kCounters = Rec::kCounters;

static_assert(80 + 4 * kBins == PD_DSTAT_RECORD_BYTES && Rec::kBytes == PD_DSTAT_RECORD_BYTES, "record layout");
static_assert(8 * (1 + kCounters) == 40 && 8 * (Rec::kSums + kSums) == 72 && 4 * Rec::kHistWord == 80, "record layout");
static_assert(kMaxK == PD_DSTAT_MAX_CLASSES, "class limit");

struct Geo {
    unsigned P;                   // pixels per image
    unsigned G;                   // workgroups per image
    int K;
    float min_d, max_d;
};

// what one (g, p) pair adds: the three threshold flags, the four terms, the bin
struct Terms {
    bool a1, a2, a3;
    double t[kSums];
    double ad;
    int bin;
};

__device__ __forceinline__ Terms terms_of(float g, float p, const double* edges) {
    Terms r;
    const float ratio = fmaxf(__fdiv_rn(g, p), __fdiv_rn(p, g));
    r.a1 = ratio < 1.25f;
    r.a2 = ratio < 1.5625f;
    r.a3 = ratio < 1.953125f;
    const double gd = (double)g, pd = (double)p;
    const double d = __dadd_rn(gd, -pd);
    const double dd = __dmul_rn(d, d);
    const double l = log1p(d / pd);
    r.ad = fabs(d);
    r.t[0] = r.ad / gd;
    r.t[1] = dd / gd;
    r.t[2] = dd;
    r.t[3] = __dmul_rn(l, l);
    int lo = 0, hi = kEdges;
#pragma unroll 1
    for (int it = 0; it < 9; ++it) {                  // 2^9 > 511
        const int mid = (lo + hi) >> 1;               // lo == hi: the padding entry or one already decided, harmless
        const bool le = lo < hi && edges[mid] <= r.ad;
        const bool gtb = lo < hi && !le;
        lo = le ? mid + 1 : lo;
        hi = gtb ? mid : hi;
    }
    r.bin = lo;
    return r;
}

template <bool Scaled>
__global__ __launch_bounds__(kThreads) void dstat_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                         const int* __restrict__ mask, const float* __restrict__ scale,
                                                         const double* __restrict__ edges_g, float* __restrict__ err,
                                                         unsigned* __restrict__ stats, double* __restrict__ ws, Classes cls,
                                                         Geo g) {
    extern __shared__ __align__(16) unsigned char smem[];
    double* edges = reinterpret_cast<double*>(smem);                                  // [512], the last one is padding
    double* wsum = edges + kBins;                                                     // [kWaves][kMaxK][4]
    unsigned* counters = reinterpret_cast<unsigned*>(wsum + kWaves * kMaxK * kSums);  // [4][kMaxK]: a1, a2, a3, bad
    float* sc = reinterpret_cast<float*>(counters + kCounters * kMaxK);               // [kMaxK]: this image's scales
    unsigned* hist = reinterpret_cast<unsigned*>(sc + kMaxK);                         // [K][512]
    const int tid = threadIdx.x;
    const int K = g.K;
    const unsigned img = blockIdx.x / g.G, grp = blockIdx.x - img * g.G;
    for (int i = tid; i < kBins; i += kThreads) edges[i] = i < kEdges ? edges_g[i] : (double)INFINITY;
    if (tid < kCounters * kMaxK) counters[tid] = 0;
    if (tid < kMaxK) sc[tid] = (Scaled && tid < K) ? scale[(size_t)img * K + tid] : 1.f;
    for (int i = tid; i < K * kBins; i += kThreads) hist[i] = 0;
    __syncthreads();

    const size_t base = (size_t)img * g.P;
    const float* gt_f = gt + base;
    const float* pred_f = pred + base;
    const int* mask_f = mask ? mask + base : nullptr;
    float* err_f = err ? err + base : nullptr;

    double s[kMaxK][kSums];
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
#pragma unroll
        for (int j = 0; j < kSums; ++j) s[k][j] = 0.0;

    // pixels of this image go round-robin over its G workgroups, a lane takes them in increasing order
    for (unsigned item = grp * kThreads + tid; item < g.P; item += g.G * kThreads) {
        const float gv = gt_f[item];
        const float pv = pred_f[item];
        const bool pass = gv > g.min_d && gv < g.max_d;                               // NaN fails
        const bool fin = __builtin_isfinite(pv);
        const float p0 = fminf(fmaxf(pv, g.min_d), g.max_d);
        if (!Scaled) {
            const bool ok = pass && fin;
            Terms r = {};
            if (ok) r = terms_of(gv, p0, edges);
            if (err_f) err_f[item] = ok ? (float)r.ad : __builtin_nanf("");
            if (!pass) continue;
            const int m = mask_f ? mask_f[item] : 0;
#pragma unroll
            for (int k = 0; k < kMaxK; ++k) {
                if (k < K) {
                    if (in_class(cls, k, m)) {
                        if (ok) {
                            atomicAdd(&hist[k * kBins + r.bin], 1u);
                            if (r.a1) atomicAdd(&counters[0 * kMaxK + k], 1u);
                            if (r.a2) atomicAdd(&counters[1 * kMaxK + k], 1u);
                            if (r.a3) atomicAdd(&counters[2 * kMaxK + k], 1u);
#pragma unroll
                            for (int j = 0; j < kSums; ++j) s[k][j] += r.t[j];
                        } else {
                            atomicAdd(&counters[3 * kMaxK + k], 1u);
                        }
                    }
                }
            }
        } else {
            if (!pass) continue;
            const int m = mask_f ? mask_f[item] : 0;
#pragma unroll
            for (int k = 0; k < kMaxK; ++k) {
                if (k < K) {
                    if (in_class(cls, k, m)) {
                        const float f = sc[k];
                        if (fin && __builtin_isfinite(f)) {
                            const float p = fminf(fmaxf(p0 * f, g.min_d), g.max_d);
                            const Terms r = terms_of(gv, p, edges);
                            atomicAdd(&hist[k * kBins + r.bin], 1u);
                            if (r.a1) atomicAdd(&counters[0 * kMaxK + k], 1u);
                            if (r.a2) atomicAdd(&counters[1 * kMaxK + k], 1u);
                            if (r.a3) atomicAdd(&counters[2 * kMaxK + k], 1u);
#pragma unroll
                            for (int j = 0; j < kSums; ++j) s[k][j] += r.t[j];
                        } else {
                            atomicAdd(&counters[3 * kMaxK + k], 1u);
                        }
                    }
                }
            }
        }
    }

    flush_records<Rec>(s, wsum, counters, hist, stats, ws, img, K);
}

inline int groups_of(int H, int W) { return groups_for(H > 0 && W > 0 ? (long)H * W : 0); }      // items: pixels

inline size_t lds_bytes(int K) {
    return (size_t)kBins * 8 + (size_t)kWaves * kMaxK * kSums * 8 + (size_t)kCounters * kMaxK * 4 + (size_t)kMaxK * 4 +
           (size_t)K * kBins * 4;
}

// ---------------------------------------------------------------------------------------------------- the medians
constexpr int kSel = 4;                             // selections per (image, class): gt lo, gt hi, pred lo, pred hi
constexpr int kDigits = 256;                        // eight bits a pass
constexpr int kPasses = 4;
constexpr int kStateWords = 2 * kSel;               // per (image, class): prefix[4], rank[4]

struct MGeo {
    unsigned P, G;
    int K, pass;
    float min_d, max_d;
};

// ghist: [image][pass][K][4][256]; state: [image][K][8]
__global__ __launch_bounds__(kThreads) void dmed_hist_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                             const int* __restrict__ mask, const unsigned* __restrict__ state,
                                                             unsigned* __restrict__ ghist, Classes cls, MGeo g) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned* hist = reinterpret_cast<unsigned*>(smem);                               // [K][4][256]: 64 KiB at K = 16
    const int tid = threadIdx.x;
    const int K = g.K, pass = g.pass;
    const unsigned img = blockIdx.x / g.G, grp = blockIdx.x - img * g.G;
    unsigned prefix[kMaxK][kSel];                   // the digits chosen so far: uniform over the workgroup
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
#pragma unroll
        for (int c = 0; c < kSel; ++c)
            prefix[k][c] = (pass > 0 && k < K) ? state[((size_t)img * K + k) * kStateWords + c] : 0u;
    for (int i = tid; i < K * kSel * kDigits; i += kThreads) hist[i] = 0;
    __syncthreads();

    const size_t base = (size_t)img * g.P;
    const float* gt_f = gt + base;
    const float* pred_f = pred + base;
    const int* mask_f = mask ? mask + base : nullptr;
    const int shift = 24 - 8 * pass;                // of this pass's digit; the chosen digits lie above bit shift + 8

    for (unsigned item = grp * kThreads + tid; item < g.P; item += g.G * kThreads) {
        const float gv = gt_f[item];
        const float pv = pred_f[item];
        if (!(gv > g.min_d && gv < g.max_d) || !__builtin_isfinite(pv)) continue;
        const int m = mask_f ? mask_f[item] : 0;
        const unsigned key[2] = {__float_as_uint(gv), __float_as_uint(fminf(fmaxf(pv, g.min_d), g.max_d))};
#pragma unroll
        for (int k = 0; k < kMaxK; ++k) {
            if (k < K) {
                if (in_class(cls, k, m)) {
#pragma unroll
                    for (int c = 0; c < kSel; ++c) {
                        const unsigned v = key[c >> 1];
                        const bool counts = pass == 0 ? (c & 1) == 0 : ((v ^ prefix[k][c]) >> (shift + 8)) == 0u;
                        if (counts) atomicAdd(&hist[(k * kSel + c) * kDigits + ((v >> shift) & 255u)], 1u);
                    }
                }
            }
        }
    }
    __syncthreads();
    unsigned* gh = ghist + ((size_t)img * kPasses + pass) * K * kSel * kDigits;
    for (int i = tid; i < K * kSel * kDigits; i += kThreads) {
        const unsigned v = hist[i];
        if (v) atomicAdd(gh + i, v);
    }
}

// one workgroup per (image, class): the digit that holds each selection's rank
__global__ __launch_bounds__(kDigits) void dmed_select_kernel(const unsigned* __restrict__ ghist, unsigned* __restrict__ state,
                                                              long long* __restrict__ count, float* __restrict__ med, int K,
                                                              int pass) {
    __shared__ unsigned cum[kSel][kDigits];
    const int j = threadIdx.x;
    const unsigned img = blockIdx.x / K, k = blockIdx.x - img * K;
    const unsigned* h = ghist + (((size_t)img * kPasses + pass) * K + k) * kSel * kDigits;
    unsigned* st = state + (size_t)blockIdx.x * kStateWords;
    unsigned v[kSel], prefix[kSel], rank[kSel];
#pragma unroll
    for (int c = 0; c < kSel; ++c) {
        v[c] = h[(pass == 0 ? (c & 2) : c) * kDigits + j];
        prefix[c] = pass > 0 ? st[c] : 0u;
        rank[c] = pass > 0 ? st[kSel + c] : 0u;
        cum[c][j] = v[c];
    }
    __syncthreads();
    for (int off = 1; off < kDigits; off <<= 1) {     // inclusive scan of the four histograms
        unsigned t[kSel];
#pragma unroll
        for (int c = 0; c < kSel; ++c) t[c] = j >= off ? cum[c][j - off] : 0u;
        __syncthreads();
#pragma unroll
        for (int c = 0; c < kSel; ++c) cum[c][j] += t[c];
        __syncthreads();
    }
    const unsigned n = cum[0][kDigits - 1];           // pass 0: the size of the pixel set
    if (pass == 0) {
        if (j == 0) count[blockIdx.x] = (long long)n;
#pragma unroll
        for (int c = 0; c < kSel; ++c) rank[c] = n ? ((c & 1) ? n / 2u : (n - 1u) / 2u) : 0u;
    }
    const int shift = 24 - 8 * pass;
#pragma unroll
    for (int c = 0; c < kSel; ++c) {
        const unsigned incl = cum[c][j], excl = incl - v[c];
        if (v[c] && excl <= rank[c] && rank[c] < incl) {      // exactly one digit per selection, none when the set is empty
            const unsigned p = prefix[c] | ((unsigned)j << shift);
            st[c] = p;
            st[kSel + c] = rank[c] - excl;
            if (pass == kPasses - 1) med[(size_t)blockIdx.x * kSel + c] = __uint_as_float(p);
        }
        if (pass == kPasses - 1 && j == 0 && cum[c][kDigits - 1] == 0u) med[(size_t)blockIdx.x * kSel + c] = __builtin_nanf("");
    }
}

inline size_t med_lds_bytes(int K) { return (size_t)K * kSel * kDigits * 4; }
inline size_t med_hist_bytes(size_t images, size_t K) { return images * kPasses * K * kSel * kDigits * 4; }

// the checks the two entry points share
inline int check_common(const char* who, const void* gt, const void* pred, const int* classes, int N, int H, int W,
                        float min_depth, float max_depth) {
    PD_REQUIRE(N >= 0 && H > 0 && W > 0, "%s: bad shape (N = %d, H = %d, W = %d)", who, N, H, W);
    PD_REQUIRE(gt && pred && classes, "%s: gt, pred and classes must not be null", who);
    PD_REQUIRE(min_depth > 0.f, "%s: min_depth = %g must be positive", who, (double)min_depth);
    PD_REQUIRE(max_depth > min_depth, "%s: max_depth = %g must be above min_depth = %g", who, (double)max_depth,
               (double)min_depth);
    PD_REQUIRE((long)H * W <= (1L << 30), "%s: a frame of %d x %d is too large for the kernel's index arithmetic", who, H, W);
    return PD_OK;
}

}  // namespace

extern "C" size_t pd_depth_medians_workspace(int N, int K) {
    const size_t n = N > 0 ? (size_t)N : 1, k = (size_t)std::min(std::max(K, 1), kMaxK);
    return med_hist_bytes(n, k) + n * k * kStateWords * 4;
}

extern "C" int pd_depth_medians(const void* gt, const void* pred, const void* mask, const int* classes, int K, void* count,
                                void* med, void* workspace, size_t ws_bytes, int N, int H, int W, float min_depth,
                                float max_depth, void* stream) {
    if (int e = check_common("pd_depth_medians", gt, pred, classes, N, H, W, min_depth, max_depth)) return e;
    PD_REQUIRE(count && med && workspace, "pd_depth_medians: count, med and workspace must not be null");
    Classes cls;
    if (int e = parse_classes("pd_depth_medians", classes, K, mask != nullptr, &cls)) return e;
    PD_REQUIRE(pd::aligned16(count) && pd::aligned16(med) && pd::aligned16(workspace),
               "pd_depth_medians: count, med and workspace must be 16-byte aligned");
    const size_t need = pd_depth_medians_workspace(N, K);
    PD_REQUIRE(ws_bytes >= need, "pd_depth_medians: workspace too small (%zu bytes, pd_depth_medians_workspace asks for %zu)",
               ws_bytes, need);
    if (N == 0) return PD_OK;
    hipStream_t st = (hipStream_t)stream;
    MGeo g;
    g.P = (unsigned)((long)H * W); g.G = (unsigned)groups_of(H, W); g.K = K; g.pass = 0; g.min_d = min_depth; g.max_d = max_depth;
    unsigned* hist_all = static_cast<unsigned*>(workspace);
    unsigned* state_all = hist_all + med_hist_bytes((size_t)N, (size_t)K) / 4;
    for (long n0 = 0; n0 < N; n0 += kMaxImagesPerLaunch) {
        const long nb = std::min<long>(kMaxImagesPerLaunch, N - n0);
        unsigned* gh = hist_all + med_hist_bytes((size_t)n0, (size_t)K) / 4;
        unsigned* state = state_all + (size_t)n0 * K * kStateWords;
        const long n16 = (long)(med_hist_bytes((size_t)nb, (size_t)K) / 16);
        const int zgrid = (int)std::min<long>(1024, (n16 + kThreads - 1) / kThreads);
        hipLaunchKernelGGL(records_zero_kernel, dim3(zgrid), dim3(kThreads), 0, st, reinterpret_cast<uint4*>(gh), n16);
        for (int pass = 0; pass < kPasses; ++pass) {
            g.pass = pass;
            hipLaunchKernelGGL(dmed_hist_kernel, dim3((unsigned)(nb * g.G)), dim3(kThreads), med_lds_bytes(K), st,
                               static_cast<const float*>(gt) + (size_t)n0 * g.P, static_cast<const float*>(pred) + (size_t)n0 * g.P,
                               mask ? static_cast<const int*>(mask) + (size_t)n0 * g.P : nullptr, state, gh, cls, g);
            hipLaunchKernelGGL(dmed_select_kernel, dim3((unsigned)(nb * K)), dim3(kDigits), 0, st, gh, state,
                               static_cast<long long*>(count) + (size_t)n0 * K, static_cast<float*>(med) + (size_t)n0 * K * kSel, K,
                               pass);
        }
    }
    return pd::check_launch("pd_depth_medians");
}

extern "C" size_t pd_depth_stats_workspace(int N, int H, int W, int K) {
    return records_workspace(N, K, groups_of(H, W), kSums);
}

extern "C" int pd_depth_stats(const void* gt, const void* pred, const void* mask, const int* classes, int K, const void* scale,
                              const void* edges, void* err, void* stats, void* workspace, size_t ws_bytes, int N, int H, int W,
                              float min_depth, float max_depth, void* stream) {
    if (int e = check_common("pd_depth_stats", gt, pred, classes, N, H, W, min_depth, max_depth)) return e;
    PD_REQUIRE(edges && stats && workspace, "pd_depth_stats: edges, stats and workspace must not be null");
    Classes cls;
    if (int e = parse_classes("pd_depth_stats", classes, K, mask != nullptr, &cls)) return e;
    PD_REQUIRE(!(err && scale), "pd_depth_stats: err is written by the unscaled call only (a scaled error is per class)");
    PD_REQUIRE(pd::aligned16(stats) && pd::aligned16(workspace), "pd_depth_stats: stats and workspace must be 16-byte aligned");
    const size_t need = pd_depth_stats_workspace(N, H, W, K);
    PD_REQUIRE(ws_bytes >= need, "pd_depth_stats: workspace too small (%zu bytes, pd_depth_stats_workspace asks for %zu)",
               ws_bytes, need);
    if (N == 0) return PD_OK;
    hipStream_t st = (hipStream_t)stream;
    Geo g;
    g.P = (unsigned)((long)H * W); g.G = (unsigned)groups_of(H, W); g.K = K; g.min_d = min_depth; g.max_d = max_depth;
    run_records<Rec>(stats, workspace, N, K, (int)g.G, st, [&](long n0, long nb, unsigned* rec, double* part) {
        const float* gt_c = static_cast<const float*>(gt) + (size_t)n0 * g.P;
        const float* pred_c = static_cast<const float*>(pred) + (size_t)n0 * g.P;
        const int* mask_c = mask ? static_cast<const int*>(mask) + (size_t)n0 * g.P : nullptr;
        const double* edges_c = static_cast<const double*>(edges);
        if (scale)
            hipLaunchKernelGGL(dstat_kernel<true>, dim3((unsigned)(nb * g.G)), dim3(kThreads), lds_bytes(K), st, gt_c, pred_c,
                               mask_c, static_cast<const float*>(scale) + (size_t)n0 * K, edges_c, (float*)nullptr, rec, part,
                               cls, g);
        else
            hipLaunchKernelGGL(dstat_kernel<false>, dim3((unsigned)(nb * g.G)), dim3(kThreads), lds_bytes(K), st, gt_c, pred_c,
                               mask_c, (const float*)nullptr, edges_c, err ? static_cast<float*>(err) + (size_t)n0 * g.P : nullptr,
                               rec, part, cls, g);
    });
    return pd::check_launch("pd_depth_stats");
}
