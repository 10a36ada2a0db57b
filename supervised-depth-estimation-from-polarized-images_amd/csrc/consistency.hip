// Multi-view depth consistency per pixel class in ONE read of the batch (pd_depth_consistency).  Definition and record:
// include/polardepth.h.  The camera pieces: view_geom.hpp.  The records, their three launches and why the sums are
// bit-reproducible: class_records.hpp.
//
// cons_kernel: one work item = one PIXEL of the current view; its lane loops over the F source views, so level, n_cons and
// fused are written by the lane that owns the pixel, with plain stores.  A workgroup belongs to one image: the cameras of
// its F views -- P = K T_f, P' = K T_f^-1 and inv_K, all fp64 -- are formed once per workgroup in LDS.  Per pixel the lane
// keeps the outcome counts and the four terms of its views in registers and adds them to each of the pixel's classes after
// the view loop; only the bin of a compared pair is counted inside the loop.
#include "class_records.hpp"
#include "view_geom.hpp"

#include <cmath>

namespace {

using Rec = Layout<PD_CONS_BINS, PD_CONS_COUNTERS, 28, PD_CONS_SUMS>;      // the histogram starts at byte 112
constexpr int kBins = Rec::kBins;
constexpr int kSums = Rec::kNumSums;
constexpr int kCounters = Rec::kCounters;
constexpr int kMaxF = PD_REPROJ_MAX_FRAMES;

static_assert(112 + 4 * kBins == PD_CONS_RECORD_BYTES && Rec::kBytes == PD_CONS_RECORD_BYTES, "record layout");
static_assert(8 * (1 + kCounters) == 72 && 8 * (Rec::kSums + kSums) == 104 && 4 * Rec::kHistWord == 112, "record layout");
static_assert(kMaxK == PD_DSTAT_MAX_CLASSES, "class limit");

// the counters after n
enum { cLoose = 0, cMid, cTight, cInvalid, cAbsent, cFiltered, cOutside, cHole };

struct Geo {
    unsigned P;                   // pixels per image
    unsigned G;                   // workgroups per image
    int K, F, H, W;
    int fuse_level;
    float min_d, max_d;
    double tp2[3];                // tau_px[j]^2
    double trel[3];
};

// entry t = 4 i + j of P' = K Ti, Ti = [R^T | -(R^T t)] the rigid inverse of T ([4][4] fp32 row-major), in fp64:
// Ti[k][j] = R[j][k] (j < 3);  Ti[k][3] = -((R[0][k] t0 + R[1][k] t1) + R[2][k] t2);  Ti[3] = (0, 0, 0, 1);
// P'[i][j] = ((K[i][0] Ti[0][j] + K[i][1] Ti[1][j]) + K[i][2] Ti[2][j]) + K[i][3] Ti[3][j]: cam_P's order
__device__ __forceinline__ double cam_P_inv(const float* K, const float* T, int t) {
    const float* k = K + (t >> 2) * 4;
    const int j = t & 3;
    double c[4];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        if (j < 3) {
            c[r] = (double)T[4 * j + r];
        } else {
            c[r] = -(((double)T[0 + r] * (double)T[3] + (double)T[4 + r] * (double)T[7]) + (double)T[8 + r] * (double)T[11]);
        }
    }
    c[3] = j < 3 ? 0.0 : 1.0;
    return (((double)k[0] * c[0] + (double)k[1] * c[1]) + (double)k[2] * c[2]) + (double)k[3] * c[3];
}

__global__ __launch_bounds__(kThreads) void cons_kernel(const float* __restrict__ depth0, const float* __restrict__ depths,
                                                        const float* __restrict__ T, const float* __restrict__ Kc,
                                                        const float* __restrict__ iKc, const float* __restrict__ frame_valid,
                                                        const unsigned char* __restrict__ visible,
                                                        const int* __restrict__ mask, unsigned char* __restrict__ level,
                                                        unsigned char* __restrict__ n_cons, float* __restrict__ fused,
                                                        unsigned* __restrict__ stats, double* __restrict__ ws, Classes cls,
                                                        Geo g) {
    __shared__ double camP[kMaxF][12];                // (K T_f)[:3,:]
    __shared__ double camQ[kMaxF][12];                // (K T_f^-1)[:3,:]
    __shared__ double camiK[9];
    __shared__ double wsum[kWaves * kMaxK * kSums];
    __shared__ unsigned counters[kCounters * kMaxK];
    __shared__ unsigned hist[kMaxK * kBins];
    __shared__ float fvalid[kMaxF];
    const int tid = threadIdx.x;
    const int K = g.K, F = g.F;
    const unsigned img = blockIdx.x / g.G, grp = blockIdx.x - img * g.G;

    for (int e = tid; e < F * 24 + 9; e += kThreads) {
        if (e < F * 24) {
            const int f = e / 24, t = e - f * 24;
            const float* Km = Kc + (size_t)img * 16;
            const float* Tm = T + ((size_t)img * F + f) * 16;
            if (t < 12) camP[f][t] = pd_geom::cam_P(Km, Tm, t);
            else camQ[f][t - 12] = cam_P_inv(Km, Tm, t - 12);
        } else {
            camiK[e - F * 24] = pd_geom::cam_iK(iKc, (long)img, e - F * 24);
        }
    }
    if (tid < kMaxF) fvalid[tid] = (tid < F && frame_valid) ? frame_valid[(size_t)img * F + tid] : 1.f;
    if (tid < kCounters * kMaxK) counters[tid] = 0;
    for (int i = tid; i < K * kBins; i += kThreads) hist[i] = 0;
    __syncthreads();

    const size_t base = (size_t)img * g.P;
    const size_t vbase = (size_t)img * F * g.P;       // of the [N][F][H][W] arrays
    const float* d0_f = depth0 + base;
    const int* mask_f = mask ? mask + base : nullptr;
    const float hiu = (float)(g.W - 1), hiv = (float)(g.H - 1);

    double s[kMaxK][kSums];
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
#pragma unroll
        for (int j = 0; j < kSums; ++j) s[k][j] = 0.0;

    // pixels of this image go round-robin over its G workgroups, a lane takes them in increasing order
    for (unsigned item = grp * kThreads + tid; item < g.P; item += g.G * kThreads) {
        const int y = (int)(item / (unsigned)g.W), x = (int)(item - (unsigned)y * (unsigned)g.W);
        const float d0 = d0_f[item];
        const int m = mask_f ? mask_f[item] : 0;
        const bool valid = in_range(d0, g.min_d, g.max_d);
        const double d0d = (double)d0;
        double r0[3];
        pd_geom::ray(camiK, x, y, r0);

        unsigned cnt[kCounters];                      // this pixel's views per counter
#pragma unroll
        for (int c = 0; c < kCounters; ++c) cnt[c] = 0;
        double t[kSums] = {0.0, 0.0, 0.0, 0.0};       // its terms, f ascending
        double acc = d0d;
        unsigned nc = 0;

#pragma unroll 1
        for (int f = 0; f < F; ++f) {
            const size_t voff = vbase + (size_t)f * g.P;
            unsigned char lv = 0;
            int reason = -1;
            double u2 = 0.0, v2 = 0.0, hz2 = 0.0;
            if (!valid) reason = cInvalid;
            else if (fvalid[f] == 0.f) reason = cAbsent;
            else if (visible && visible[voff + item] == 0) reason = cFiltered;
            else {
                double u, v, hz, q[3], p[3];
                pd_geom::project_ray(camP[f], r0, d0d, u, v, hz, q, p);
                const float uf = (float)u, vf = (float)v;
                if (!(hz > 1e-3 && uf >= 0.f && uf <= hiu && vf >= 0.f && vf <= hiv)) reason = cOutside;
                else {
                    const pd_geom::Axis ax = pd_geom::axis_of(uf, g.W), ay = pd_geom::axis_of(vf, g.H);
                    const float* src = depths + voff;
                    const float v00 = src[(size_t)ay.i0 * g.W + ax.i0], v10 = src[(size_t)ay.i0 * g.W + ax.i1];
                    const float v01 = src[(size_t)ay.i1 * g.W + ax.i0], v11 = src[(size_t)ay.i1 * g.W + ax.i1];
                    if (!(in_range(v00, g.min_d, g.max_d) && in_range(v10, g.min_d, g.max_d) &&
                          in_range(v01, g.min_d, g.max_d) && in_range(v11, g.min_d, g.max_d))) reason = cHole;
                    else {
                        const float d1 = pd_geom::Bilinear(ax.w1, ay.w1).blend(v00, v10, v01, v11);
                        double r1[3];
                        pd_geom::ray(camiK, (double)uf, (double)vf, r1);
                        pd_geom::project_ray(camQ[f], r1, (double)d1, u2, v2, hz2, q, p);
                        if (!(hz2 > 1e-3)) reason = cOutside;
                    }
                }
            }
            if (reason >= 0) {
#pragma unroll
                for (int c = cInvalid; c < kCounters; ++c) cnt[c] += (reason == c);
            } else {
                const double du = u2 - (double)x, dv = v2 - (double)y;
                const double e2 = du * du + dv * dv;
                const double e_px = sqrt(e2);
                const double e_rel = fabs(hz2 - d0d) / d0d;
                lv = 1;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const bool met = e2 < g.tp2[j] && e_rel < g.trel[j];
                    cnt[j] += met;
                    if (met) lv = (unsigned char)(2 + j);
                }
                t[0] += e_px;
                t[1] += e_rel;
                t[2] += e2;
                t[3] += e_rel * e_rel;
                const double b = floor(e_rel * 1024.0);
                const int bin = b < (double)(kBins - 1) ? (int)b : kBins - 1;      // NaN: the open bin
                if ((int)lv >= g.fuse_level) {
                    acc += hz2;
                    ++nc;
                }
#pragma unroll
                for (int k = 0; k < kMaxK; ++k) {
                    if (k < K) {
                        if (in_class(cls, k, m)) atomicAdd(&hist[k * kBins + bin], 1u);
                    }
                }
            }
            if (level) level[voff + item] = lv;
        }
        if (n_cons) n_cons[base + item] = (unsigned char)nc;
        if (fused) fused[base + item] = valid ? (float)(acc / (double)(1u + nc)) : 0.f;

#pragma unroll
        for (int k = 0; k < kMaxK; ++k) {
            if (k < K) {
                if (in_class(cls, k, m)) {
#pragma unroll
                    for (int c = 0; c < kCounters; ++c)
                        if (cnt[c]) atomicAdd(&counters[c * kMaxK + k], cnt[c]);
#pragma unroll
                    for (int j = 0; j < kSums; ++j) s[k][j] += t[j];
                }
            }
        }
    }

    flush_records<Rec>(s, wsum, counters, hist, stats, ws, img, K);
}

inline int groups_of(int H, int W) { return groups_for(H > 0 && W > 0 ? (long)H * W : 0); }      // items: pixels

}  // namespace

extern "C" size_t pd_depth_consistency_workspace(int N, int H, int W, int K) {
    return records_workspace(N, K, groups_of(H, W), kSums);
}

extern "C" int pd_depth_consistency(const void* depth0, const void* depths, const void* T, const void* K, const void* inv_K,
                                    const void* frame_valid, const void* visible, const void* mask, const int* classes,
                                    int n_classes, float min_depth, float max_depth, const double* tau_px,
                                    const double* tau_rel, int fuse_level, void* level, void* n_cons, void* fused, void* stats,
                                    void* workspace, size_t ws_bytes, int N, int F, int H, int W, void* stream) {
    const char* who = "pd_depth_consistency";
    PD_REQUIRE(N >= 0 && H > 0 && W > 0, "%s: bad shape (N = %d, H = %d, W = %d)", who, N, H, W);
    PD_REQUIRE(F >= 1 && F <= kMaxF, "%s: F = %d source views, 1 .. %d are supported", who, F, kMaxF);
    PD_REQUIRE(depth0 && depths && T && K && inv_K && classes && tau_px && tau_rel && stats && workspace,
               "%s: depth0, depths, T, K, inv_K, classes, tau_px, tau_rel, stats and workspace must not be null", who);
    PD_REQUIRE(min_depth > 0.f, "%s: min_depth = %g must be positive", who, (double)min_depth);
    PD_REQUIRE(max_depth > min_depth, "%s: max_depth = %g must be above min_depth = %g", who, (double)max_depth,
               (double)min_depth);
    PD_REQUIRE((long)H * W <= (1L << 30), "%s: a frame of %d x %d is too large for the kernel's index arithmetic", who, H, W);
    Classes cls;
    if (int e = parse_classes(who, classes, n_classes, mask != nullptr, &cls)) return e;
    for (int j = 0; j < 3; ++j) {
        PD_REQUIRE(tau_px[j] > 0.0 && tau_rel[j] > 0.0 && std::isfinite(tau_px[j]) && std::isfinite(tau_rel[j]),
                   "%s: the thresholds of level %d (tau_px = %g, tau_rel = %g) must be positive and finite", who, j + 2, tau_px[j],
                   tau_rel[j]);
        PD_REQUIRE(j == 0 || (tau_px[j] <= tau_px[j - 1] && tau_rel[j] <= tau_rel[j - 1]),
                   "%s: the thresholds must be nested, loose to tight (level %d: tau_px = %g, tau_rel = %g)", who, j + 2,
                   tau_px[j], tau_rel[j]);
    }
    PD_REQUIRE(fuse_level >= 2 && fuse_level <= 4, "%s: fuse_level = %d must be 2, 3 or 4", who, fuse_level);
    PD_REQUIRE(pd::aligned16(stats) && pd::aligned16(workspace), "%s: stats and workspace must be 16-byte aligned", who);
    const size_t need = pd_depth_consistency_workspace(N, H, W, n_classes);
    PD_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu bytes, pd_depth_consistency_workspace asks for %zu)", who,
               ws_bytes, need);
    if (N == 0) return PD_OK;
    hipStream_t st = (hipStream_t)stream;
    Geo g;
    g.P = (unsigned)((long)H * W); g.G = (unsigned)groups_of(H, W); g.K = n_classes; g.F = F; g.H = H; g.W = W;
    g.fuse_level = fuse_level; g.min_d = min_depth; g.max_d = max_depth;
    for (int j = 0; j < 3; ++j) {
        g.tp2[j] = tau_px[j] * tau_px[j];
        g.trel[j] = tau_rel[j];
    }
    run_records<Rec>(stats, workspace, N, n_classes, (int)g.G, st, [&](long n0, long nb, unsigned* rec, double* part) {
        const size_t o = (size_t)n0 * g.P, of = o * F;
        hipLaunchKernelGGL(cons_kernel, dim3((unsigned)(nb * g.G)), dim3(kThreads), 0, st,
                           static_cast<const float*>(depth0) + o, static_cast<const float*>(depths) + of,
                           static_cast<const float*>(T) + (size_t)n0 * F * 16, static_cast<const float*>(K) + (size_t)n0 * 16,
                           static_cast<const float*>(inv_K) + (size_t)n0 * 16,
                           frame_valid ? static_cast<const float*>(frame_valid) + (size_t)n0 * F : nullptr,
                           visible ? static_cast<const unsigned char*>(visible) + of : nullptr,
                           mask ? static_cast<const int*>(mask) + o : nullptr,
                           level ? static_cast<unsigned char*>(level) + of : nullptr,
                           n_cons ? static_cast<unsigned char*>(n_cons) + o : nullptr,
                           fused ? static_cast<float*>(fused) + o : nullptr, rec, part, cls, g);
    });
    return pd::check_launch(who);
}
