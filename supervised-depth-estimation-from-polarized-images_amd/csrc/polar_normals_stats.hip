// Does a predicted surface agree with the polarisation that was measured?  pd_polar_normals_stats scores predicted normals
// against the three physical normal candidates K1 derives from DoLP / AoLP (N_diff, N_spec1, N_spec2), for up to 16 pixel
// classes at once, as TWO sets of per-image, per-class records: the angle to the best of the six candidates (each candidate
// and its pi flip), and the azimuth residual modulo pi.  Definition and records: include/polardepth.h.  The records, the
// launches around the evaluator's and why the sums are bit-reproducible: class_records.hpp.
//
// pnstat_kernel: one work item = one PIXEL; blockIdx.x = image * G + workgroup of the image, blockIdx.y = the record set.  The
// two sets are filled by the SAME launch but by different workgroups: a lane carries the fp64 sums of every class in
// registers (16 classes x 4 sums = 128 VGPRs per set), and a workgroup the LDS histogram of its set ([16][720] or [16][360]
// words).  Both sets in one workgroup would need 256 VGPRs of sums and 69 KB of histograms, which is beyond the 64 KB a
// launch gets without an attribute call that cannot be made while a stream is being captured.  The second reader of a pixel
// finds it in L2 / MALL; the gates are evaluated twice, the arithmetic of the two sets (six divisions and an acos; two
// divisions and an acos) is disjoint.
//
// A bin is the number of table entries cos_edges[j] >= c, found by binary search over a copy of the caller's table in LDS:
// acos takes no part in any decision.
#include "class_records.hpp"
#include "ray_frame.hpp"

#include <cmath>

namespace {

using RecN = Layout<PD_PNSTAT_NORMAL_BINS, PD_PNSTAT_COUNTERS, 20, PD_PNSTAT_SUMS>;       // the histogram starts at byte 80
using RecA = Layout<PD_PNSTAT_AZIMUTH_BINS, PD_PNSTAT_COUNTERS, 20, PD_PNSTAT_SUMS>;
constexpr int kSums = PD_PNSTAT_SUMS;
constexpr int kCounters = PD_PNSTAT_COUNTERS;
constexpr int kEdgesN = RecN::kBins - 1;             // 719: the caller's table
constexpr int kEdgesA = RecA::kBins - 1;             // 359: its first half
constexpr double kDegPerRad = 57.29577951308232;

static_assert(RecN::kBytes == PD_PNSTAT_NORMAL_RECORD_BYTES && 80 + 4 * RecN::kBins == PD_PNSTAT_NORMAL_RECORD_BYTES, "record layout");
static_assert(RecA::kBytes == PD_PNSTAT_AZIMUTH_RECORD_BYTES && 80 + 4 * RecA::kBins == PD_PNSTAT_AZIMUTH_RECORD_BYTES, "record layout");
static_assert(8 * (1 + kCounters) == 40 && 8 * (RecN::kSums + kSums) == 72, "record layout");
static_assert(kMaxK == PD_PNSTAT_MAX_CLASSES && PD_PNSTAT_NORMAL_BINS == PD_NSTAT_BINS, "class limit, cos_edges table");

// the counters after n; the first two are the gates, shared by the two sets
enum { cBad = 0, cDolpOut = 1, cSpecN = 2, cFlipped = 3, cFrontal = 2, cSpecA = 3 };
enum { setNormal = 0, setAzimuth = 1 };

struct Geo {
    unsigned P, W;                // pixels per image, columns
    unsigned G;                   // workgroups per image
    int K, first_set;             // blockIdx.y + first_set is the set
    int vec4;                     // pred is read with 16-byte loads (ld == 4, aligned)
    long ld;
    size_t ldp, plane;            // row pitch of the planar inputs; one plane = H * ldp
    double rho_min, rho_max, tilt2_min, sign;
};

// #{ j < n : c <= edges[j] } over the strictly decreasing table; 2^10 > 719
__device__ __forceinline__ int bin_of(const double* edges, double c, int n) {
    int lo = 0, hi = n;
#pragma unroll 1
    for (int it = 0; it < 10; ++it) {
        const int mid = (lo + hi) >> 1;               // lo == hi: nothing moves
        const bool le = lo < hi && c <= edges[mid];
        const bool gt = lo < hi && !le;
        lo = le ? mid + 1 : lo;
        hi = gt ? mid : hi;
    }
    return lo;
}

// RAY: the prediction is scored in the frame of its pixel's viewing ray (ray_frame.hpp): p' = R(x, y) p replaces p from the
// `bad` gate on, and the pol_normal map leaves as R^T of the winner.  The frame is three doubles next to 128 VGPRs of sums:
// it is formed, used and dropped before the accumulators are touched, and formed again for the pol_normal map.
template <bool RAY>
__global__ __launch_bounds__(kThreads) void pnstat_kernel(const float* __restrict__ pred, const float* __restrict__ pol,
                                                          const float* __restrict__ xolp, const int* __restrict__ mask,
                                                          const unsigned char* __restrict__ valid,
                                                          const double* __restrict__ cos_edges, float* __restrict__ az_deg,
                                                          float* __restrict__ n_deg, unsigned char* __restrict__ choice,
                                                          float4* __restrict__ pol_normal, unsigned* __restrict__ stats_n,
                                                          unsigned* __restrict__ stats_a, double* __restrict__ ws_n,
                                                          double* __restrict__ ws_a, Classes cls, Geo g,
                                                          const float* __restrict__ Kmat) {
    extern __shared__ __align__(16) unsigned char smem[];
    double* edges = reinterpret_cast<double*>(smem);                                  // [720], the last one is padding
    double* wsum = edges + RecN::kBins;                                               // [kWaves][kMaxK][4]
    unsigned* counters = reinterpret_cast<unsigned*>(wsum + kWaves * kMaxK * kSums);  // [4][kMaxK]
    unsigned* hist = counters + kCounters * kMaxK;                                    // [K][720] or [K][360]
    const int tid = threadIdx.x;
    const int K = g.K;
    const int set = g.first_set + (int)blockIdx.y;
    const int bins = set == setNormal ? RecN::kBins : RecA::kBins;
    for (int i = tid; i < RecN::kBins; i += kThreads) edges[i] = i < kEdgesN ? cos_edges[i] : -2.0;
    if (tid < kCounters * kMaxK) counters[tid] = 0;
    for (int i = tid; i < K * bins; i += kThreads) hist[i] = 0;
    __syncthreads();

    const unsigned img = blockIdx.x / g.G, grp = blockIdx.x - img * g.G;
    const size_t base = (size_t)img * g.P;
    const float* pred_f = pred + base * (size_t)g.ld;
    const float* pol_f = pol + (size_t)img * 9 * g.plane;
    const float* rho_f = xolp + (size_t)img * 2 * g.plane;                            // channel 0
    const int* mask_f = mask ? mask + base : nullptr;
    const unsigned char* valid_f = valid ? valid + base : nullptr;
    const float nanf_ = __builtin_nanf("");
    pd_dn::Cam cam{1.f, 1.f, 0.f, 0.f};
    if constexpr (RAY) cam = pd_dn::load_cam(Kmat, (long)img);      // uniform: once per workgroup

    double s[kMaxK][kSums];
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
#pragma unroll
        for (int j = 0; j < kSums; ++j) s[k][j] = 0.0;

    // pixels of this image go round-robin over its G workgroups, a lane takes them in increasing order
    for (unsigned item = grp * kThreads + tid; item < g.P; item += g.G * kThreads) {
        const unsigned y = item / g.W, x = item - y * g.W;
        const size_t po = (size_t)y * g.ldp + x;
        int reason = -2;                              // -2: not to be counted; -1: counts; else the gate's counter
        int m = 0;
        double rho = 0.0, px = 0.0, py = 0.0, pz = 0.0, a2 = 0.0;
        double cx[3], cy[3], cz[3], b2[3];
        bool neg = false;
        if (!valid_f || valid_f[item]) {
            if (mask_f) m = mask_f[item];
            rho = (double)rho_f[po];
            if (!__builtin_isfinite(rho) || rho < g.rho_min || rho > g.rho_max) {
                reason = cDolpOut;
            } else {
                if (g.vec4) {
                    const float4 q = reinterpret_cast<const float4*>(pred_f)[item];
                    px = (double)q.x; py = (double)q.y; pz = (double)q.z;
                } else {
                    const float* pp = pred_f + (size_t)item * (size_t)g.ld;
                    px = (double)pp[0]; py = (double)pp[1]; pz = (double)pp[2];
                }
                if constexpr (RAY) pd_ray::rotate(pd_ray::make(cam, (int)x, (int)y), px, py, pz);
                // fp32 products are exact in fp64; the sums keep the order of the definition (the file is built without
                // contraction)
                a2 = (px * px + py * py) + pz * pz;
                bool fin = true, any = false;
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    cx[b] = (double)pol_f[(size_t)(3 * b) * g.plane + po];
                    cy[b] = g.sign * (double)pol_f[(size_t)(3 * b + 1) * g.plane + po];
                    cz[b] = (double)pol_f[(size_t)(3 * b + 2) * g.plane + po];
                    fin = fin && __builtin_isfinite(cx[b]) && __builtin_isfinite(cy[b]) && __builtin_isfinite(cz[b]);
                    b2[b] = (cx[b] * cx[b] + cy[b] * cy[b]) + cz[b] * cz[b];
                    any = any || b2[b] > 0.0;
                }
                reason = (__builtin_isfinite(a2) && a2 > 0.0 && fin && any) ? -1 : cBad;
                if (reason == -1 && pz < 0.0) {
                    neg = true;
                    px = -px; py = -py; pz = -pz;
                }
            }
        }

        double deg = 0.0;
        int bin = 0;
        bool c2 = false, c3 = false;                  // the set's two own counters, for a pixel that counts
        if (set == setNormal) {
            int win = -1;
            if (reason == -1) {
                const double sa = sqrt(a2);
                double best = -HUGE_VAL;
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    if (b2[b] > 0.0) {
                        const double mm = px * cx[b] + py * cy[b], q = pz * cz[b];
                        const double den = sa * sqrt(b2[b]);
                        const double cp = (mm + q) / den, cm = (-mm + q) / den;
                        if (__builtin_isfinite(cp) && cp > best) { best = cp; win = 2 * b; }
                        if (__builtin_isfinite(cm) && cm > best) { best = cm; win = 2 * b + 1; }
                    }
                }
                if (win < 0) {
                    reason = cBad;                    // every cosine non-finite: not reachable from fp32 inputs
                } else {
                    const double c = fmin(fmax(best, -1.0), 1.0);
                    bin = bin_of(edges, c, kEdgesN);
                    deg = acos(c) * kDegPerRad;
                    c2 = win >= 2;
                    c3 = (win & 1) != 0;
                }
            }
            const bool counts = reason == -1;
            if (n_deg) n_deg[base + item] = counts ? (float)deg : nanf_;
            if (choice) choice[base + item] = counts ? (unsigned char)(1 + win) : (unsigned char)0;
            if (pol_normal) {
                float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
                if (counts) {
                    const int b = win >> 1;
                    double ox = cx[b], oy = cy[b], oz = cz[b];
                    if (win & 1) { ox = -ox; oy = -oy; }
                    if (neg) { ox = -ox; oy = -oy; oz = -oz; }
                    if constexpr (RAY) pd_ray::rotate_t(pd_ray::make(cam, (int)x, (int)y), ox, oy, oz);   // camera coordinates
                    o = make_float4((float)ox, (float)oy, (float)oz, 0.f);
                }
                pol_normal[base + item] = o;
            }
        } else {
            if (reason == -1) {
                const double t2 = px * px + py * py;
                const double ud = cx[0] * cx[0] + cy[0] * cy[0], us = cx[1] * cx[1] + cy[1] * cy[1];
                if (t2 <= g.tilt2_min * a2 || !(ud > 0.0 || us > 0.0)) {
                    reason = cFrontal;
                } else {
                    const double st = sqrt(t2);
                    double cd = -1.0, cs = -1.0;
                    if (ud > 0.0) cd = fmin(fabs(px * cx[0] + py * cy[0]) / (st * sqrt(ud)), 1.0);
                    if (us > 0.0) cs = fmin(fabs(px * cx[1] + py * cy[1]) / (st * sqrt(us)), 1.0);
                    const double c = fmax(cd, cs);
                    bin = bin_of(edges, c, kEdgesA);
                    deg = acos(c) * kDegPerRad;
                    c3 = cs > cd;
                }
            }
            if (az_deg) az_deg[base + item] = reason == -1 ? (float)deg : nanf_;
        }

        if (reason == -2) continue;
        const double t[kSums] = {deg, deg * deg, rho * deg, rho};
#pragma unroll
        for (int k = 0; k < kMaxK; ++k) {
            if (k < K) {
                if (in_class(cls, k, m)) {
                    if (reason == -1) {
                        atomicAdd(&hist[k * bins + bin], 1u);
                        if (c2) atomicAdd(&counters[2 * kMaxK + k], 1u);
                        if (c3) atomicAdd(&counters[3 * kMaxK + k], 1u);
#pragma unroll
                        for (int j = 0; j < kSums; ++j) s[k][j] += t[j];
                    } else {
                        atomicAdd(&counters[reason * kMaxK + k], 1u);
                    }
                }
            }
        }
    }

    // uniform per workgroup: a set without records still writes its maps
    if (set == setNormal) {
        if (stats_n) flush_records<RecN>(s, wsum, counters, hist, stats_n, ws_n, img, K);
    } else {
        if (stats_a) flush_records<RecA>(s, wsum, counters, hist, stats_a, ws_a, img, K);
    }
}

inline int groups_of(int H, int W) { return groups_for(H > 0 && W > 0 ? (long)H * W : 0); }      // items: pixels

inline size_t lds_bytes(int K, int bins) {
    return (size_t)RecN::kBins * 8 + (size_t)kWaves * kMaxK * kSums * 8 + (size_t)kCounters * kMaxK * 4 + (size_t)K * bins * 4;
}
static_assert(720 * 8 + 4 * 16 * 4 * 8 + 4 * 16 * 4 + 16 * 720 * 4 <= 64 * 1024, "the launch needs no LDS attribute call");

template <class L>
inline void zero_records(unsigned* rec, long nb, int K, hipStream_t st) {
    const long n16 = nb * K * (L::kBytes / 16);
    const int zgrid = (int)std::min<long>(1024, (n16 + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(records_zero_kernel, dim3(zgrid), dim3(kThreads), 0, st, reinterpret_cast<uint4*>(rec), n16);
}

}  // namespace

extern "C" size_t pd_polar_normals_stats_workspace(int N, int H, int W, int K) {
    return 2 * records_workspace(N, K, groups_of(H, W), kSums);      // the normal set's partial sums, then the azimuth set's
}

namespace {

int pnstat_call(const char* who, const void* pred, long ld, const void* intrinsics, int ray_frame, const void* pol_normals,
                const void* xolp, long ldp, const void* mask, const int* classes, int K, const void* valid, const void* cos_edges,
                float rho_min, float rho_max, double tilt2_min, int aolp_sign, void* stats_normal, void* stats_azimuth,
                void* az_deg, void* n_deg, void* choice, void* pol_normal, void* workspace, size_t ws_bytes, int N, int H, int W,
                void* stream) {
    PD_REQUIRE(ray_frame == 0 || ray_frame == 1, "%s: ray_frame = %d must be 0 or 1", who, ray_frame);
    PD_REQUIRE(ray_frame == 0 || intrinsics, "%s: ray_frame = 1 needs the intrinsics K [N,4,4], K must not be null", who);
    PD_REQUIRE(N >= 0 && H > 0 && W > 0, "%s: bad shape (N = %d, H = %d, W = %d)", who, N, H, W);
    PD_REQUIRE(pred && pol_normals && xolp && classes && cos_edges && workspace,
               "%s: pred, pol_normals, xolp, classes, cos_edges and workspace must not be null", who);
    PD_REQUIRE(stats_normal || stats_azimuth, "%s: stats_normal and stats_azimuth are both null: nothing to fill", who);
    Classes cls;
    if (int e = parse_classes(who, classes, K, mask != nullptr, &cls)) return e;
    PD_REQUIRE(ld >= 3, "%s: the pixel stride ld = %ld must be at least 3", who, ld);
    PD_REQUIRE(ldp >= W, "%s: the row pitch ldp = %ld must be at least W = %d", who, ldp, W);
    PD_REQUIRE(aolp_sign == 1 || aolp_sign == -1, "%s: aolp_sign = %d must be +1 or -1", who, aolp_sign);
    PD_REQUIRE(std::isfinite(rho_min) && std::isfinite(rho_max) && rho_min <= rho_max,
               "%s: the DoLP range [rho_min = %g, rho_max = %g] must be finite and not inverted", who, (double)rho_min,
               (double)rho_max);
    PD_REQUIRE(tilt2_min >= 0.0 && tilt2_min < 1.0, "%s: tilt2_min = %g must be in [0, 1): it is a squared sine", who, tilt2_min);
    PD_REQUIRE(pd::aligned16(pol_normals) && pd::aligned16(stats_normal) && pd::aligned16(stats_azimuth) &&
               pd::aligned16(pol_normal) && pd::aligned16(workspace),
               "%s: pol_normals, the records, pol_normal and workspace must be 16-byte aligned", who);
    PD_REQUIRE((long)H * W <= (1L << 30), "%s: a frame of %d x %d is too large for the kernel's index arithmetic", who, H, W);
    const size_t need = pd_polar_normals_stats_workspace(N, H, W, K);
    PD_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu bytes, pd_polar_normals_stats_workspace asks for %zu)", who,
               ws_bytes, need);
    if (N == 0) return PD_OK;
    hipStream_t st = (hipStream_t)stream;
    const bool run_n = stats_normal || n_deg || choice || pol_normal, run_a = stats_azimuth || az_deg;
    Geo g;
    g.P = (unsigned)((long)H * W); g.W = (unsigned)W; g.G = (unsigned)groups_of(H, W); g.K = K;
    g.first_set = run_n ? setNormal : setAzimuth;
    g.vec4 = ld == 4 && pd::aligned16(pred);
    g.ld = ld; g.ldp = (size_t)ldp; g.plane = (size_t)H * (size_t)ldp;
    g.rho_min = (double)rho_min; g.rho_max = (double)rho_max; g.tilt2_min = tilt2_min; g.sign = (double)aolp_sign;
    const int sets = (run_n ? 1 : 0) + (run_a ? 1 : 0);
    const size_t lds = lds_bytes(K, run_n ? RecN::kBins : RecA::kBins);
    const size_t half = records_workspace(N, K, (int)g.G, kSums);
    for (long n0 = 0; n0 < N; n0 += kMaxImagesPerLaunch) {
        const long nb = std::min<long>(kMaxImagesPerLaunch, N - n0);
        const size_t o = (size_t)n0 * g.P, part = (size_t)n0 * g.G * K * kSums;
        unsigned* rec_n = stats_normal ? reinterpret_cast<unsigned*>(static_cast<unsigned char*>(stats_normal) +
                                                                     (size_t)n0 * K * RecN::kBytes) : nullptr;
        unsigned* rec_a = stats_azimuth ? reinterpret_cast<unsigned*>(static_cast<unsigned char*>(stats_azimuth) +
                                                                      (size_t)n0 * K * RecA::kBytes) : nullptr;
        double* ws_n = static_cast<double*>(workspace) + part;
        double* ws_a = reinterpret_cast<double*>(static_cast<unsigned char*>(workspace) + half) + part;
        if (rec_n) zero_records<RecN>(rec_n, nb, K, st);
        if (rec_a) zero_records<RecA>(rec_a, nb, K, st);
        const float* Kn = ray_frame ? static_cast<const float*>(intrinsics) + (size_t)n0 * 16 : nullptr;
        const auto kern = ray_frame ? pnstat_kernel<true> : pnstat_kernel<false>;
        hipLaunchKernelGGL(kern, dim3((unsigned)(nb * g.G), (unsigned)sets), dim3(kThreads), lds, st,
                           static_cast<const float*>(pred) + o * (size_t)ld,
                           static_cast<const float*>(pol_normals) + (size_t)n0 * 9 * g.plane,
                           static_cast<const float*>(xolp) + (size_t)n0 * 2 * g.plane,
                           mask ? static_cast<const int*>(mask) + o : nullptr,
                           valid ? static_cast<const unsigned char*>(valid) + o : nullptr,
                           static_cast<const double*>(cos_edges), az_deg ? static_cast<float*>(az_deg) + o : nullptr,
                           n_deg ? static_cast<float*>(n_deg) + o : nullptr,
                           choice ? static_cast<unsigned char*>(choice) + o : nullptr,
                           pol_normal ? static_cast<float4*>(pol_normal) + o : nullptr, rec_n, rec_a, ws_n, ws_a, cls, g, Kn);
        if (rec_n) hipLaunchKernelGGL(HIP_KERNEL_NAME(records_finalize_kernel<RecN>), dim3((unsigned)(nb * K)), dim3(kThreads),
                                      0, st, rec_n, ws_n, K, (int)g.G);
        if (rec_a) hipLaunchKernelGGL(HIP_KERNEL_NAME(records_finalize_kernel<RecA>), dim3((unsigned)(nb * K)), dim3(kThreads),
                                      0, st, rec_a, ws_a, K, (int)g.G);
    }
    return pd::check_launch(who);
}

}  // namespace

extern "C" int pd_polar_normals_stats(const void* pred, long ld, const void* pol_normals, const void* xolp, long ldp,
                                      const void* mask, const int* classes, int K, const void* valid, const void* cos_edges,
                                      float rho_min, float rho_max, double tilt2_min, int aolp_sign, void* stats_normal,
                                      void* stats_azimuth, void* az_deg, void* n_deg, void* choice, void* pol_normal,
                                      void* workspace, size_t ws_bytes, int N, int H, int W, void* stream) {
    return pnstat_call("pd_polar_normals_stats", pred, ld, nullptr, 0, pol_normals, xolp, ldp, mask, classes, K, valid, cos_edges,
                       rho_min, rho_max, tilt2_min, aolp_sign, stats_normal, stats_azimuth, az_deg, n_deg, choice, pol_normal,
                       workspace, ws_bytes, N, H, W, stream);
}

extern "C" int pd_polar_normals_stats_ray(const void* pred, long ld, const void* K_intrinsics, int ray_frame,
                                          const void* pol_normals, const void* xolp, long ldp, const void* mask,
                                          const int* classes, int K, const void* valid, const void* cos_edges, float rho_min,
                                          float rho_max, double tilt2_min, int aolp_sign, void* stats_normal,
                                          void* stats_azimuth, void* az_deg, void* n_deg, void* choice, void* pol_normal,
                                          void* workspace, size_t ws_bytes, int N, int H, int W, void* stream) {
    return pnstat_call("pd_polar_normals_stats_ray", pred, ld, K_intrinsics, ray_frame, pol_normals, xolp, ldp, mask, classes, K,
                       valid, cos_edges, rho_min, rho_max, tilt2_min, aolp_sign, stats_normal, stats_azimuth, az_deg, n_deg,
                       choice, pol_normal, workspace, ws_bytes, N, H, W, stream);
}
