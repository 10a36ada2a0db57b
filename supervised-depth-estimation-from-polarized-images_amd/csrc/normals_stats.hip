// Angular error of predicted surface normals against the normals of the ground-truth depth, for up to 16 pixel classes
// (the whole frame, all objects, each material of the instance mask) in ONE read of the batch: counts, fp64 sums of the
// angle and its square, and a 0.25-degree histogram per image and class.  Definition and record: include/polardepth.h,
// pd_normals_stats.  The records, their three launches and why the sums are bit-reproducible: class_records.hpp.
//
// nstat_kernel: one work item = one quad (4 consecutive pixels of a row: per pixel three pred floats, one 16-byte gtn load,
// the depth, the mask value; with gate 1 the 3 x 6 depths around the quad from L1 / L2).  The one counter is `bad`.
//
// The bin of a pixel is the number of table entries cos_edges[j] >= c, found by a ten-step binary search over a copy of the
// caller's 719 doubles in LDS: acos takes no part in a bin decision.
#include "class_records.hpp"

#include <cmath>

namespace {

using Rec = Layout<PD_NSTAT_BINS, 1, 8>;            // one counter (`bad`), the histogram starts at byte 32
constexpr int kBins = Rec::kBins;
constexpr int kEdges = kBins - 1;
constexpr double kDegPerRad = 57.29577951308232;

static_assert(32 + 4 * kBins == PD_NSTAT_RECORD_BYTES && Rec::kBytes == PD_NSTAT_RECORD_BYTES, "record layout");
static_assert(kMaxK == PD_NSTAT_MAX_CLASSES, "class limit");

struct Geo {
    unsigned H, W, Q, items;      // rows, columns, quads per row, quads per image
    unsigned G;                   // workgroups per image
    int K, gate;
    long ld;
    float min_d, max_d;
};

__global__ __launch_bounds__(kThreads) void nstat_kernel(const float* __restrict__ pred, const float4* __restrict__ gtn,
                                                         const float* __restrict__ gt, const int* __restrict__ mask,
                                                         const double* __restrict__ cos_edges, float* __restrict__ err_deg,
                                                         unsigned* __restrict__ stats, double* __restrict__ ws, Classes cls,
                                                         Geo g) {
    extern __shared__ __align__(16) unsigned char smem[];
    double* edges = reinterpret_cast<double*>(smem);                                  // [720], the last one is padding
    double* wsum = edges + kBins;                                                     // [kWaves][kMaxK][2]
    unsigned* bad = reinterpret_cast<unsigned*>(wsum + kWaves * kMaxK * 2);           // [kMaxK]
    unsigned* hist = bad + kMaxK;                                                     // [K][720]
    const int tid = threadIdx.x;
    const int K = g.K;
    for (int i = tid; i < kBins; i += kThreads) edges[i] = i < kEdges ? cos_edges[i] : -2.0;
    if (tid < kMaxK) bad[tid] = 0;
    for (int i = tid; i < K * kBins; i += kThreads) hist[i] = 0;
    __syncthreads();

    const unsigned img = blockIdx.x / g.G, grp = blockIdx.x - img * g.G;
    const size_t frame = (size_t)g.H * g.W, base = (size_t)img * frame;
    const float* gt_f = gt + base;
    const float4* gtn_f = gtn + base;
    const int* mask_f = mask ? mask + base : nullptr;
    const float* pred_f = pred + base * (size_t)g.ld;
    float* err_f = err_deg ? err_deg + base : nullptr;

    double s[kMaxK][2];
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) s[k][0] = s[k][1] = 0.0;

    // items of this image go round-robin over its G workgroups, a lane takes them in increasing order
    for (unsigned item = grp * kThreads + tid; item < g.items; item += g.G * kThreads) {
        const unsigned y = item / g.Q, x0 = 4u * (item - y * g.Q);
        const unsigned row = y * g.W;
        bool pass[4], valid[4];
        double c[4];
        int m[4];
        float win[3][6];                              // gate 1: the depths of rows y-1 .. y+1, columns x0-1 .. x0+4, clamped
        if (g.gate) {
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const unsigned yy = (unsigned)min(max((int)y + dy - 1, 0), (int)g.H - 1);
#pragma unroll
                for (int dx = 0; dx < 6; ++dx) {
                    const unsigned xx = (unsigned)min(max((int)x0 + dx - 1, 0), (int)g.W - 1);
                    win[dy][dx] = gt_f[yy * g.W + xx];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned x = x0 + j;
            pass[j] = valid[j] = false;
            c[j] = 0.0;
            m[j] = 0;
            if (x >= g.W) continue;
            const unsigned p = row + x;              // < 2^30
            bool ok;
            if (g.gate) {
                ok = true;
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) ok = ok && in_range(win[dy][j + dx], g.min_d, g.max_d);
            } else {
                ok = in_range(gt_f[p], g.min_d, g.max_d);
            }
            pass[j] = ok;
            if (!ok) continue;
            const float* pp = pred_f + (size_t)p * (size_t)g.ld;
            const float4 q = gtn_f[p];
            const double px = (double)pp[0], py = (double)pp[1], pz = (double)pp[2];
            const double gx = (double)q.x, gy = (double)q.y, gz = (double)q.z;
            // fp32 products are exact in fp64; the sums keep the order of the definition (no contraction)
            const double d = __dadd_rn(__dadd_rn(__dmul_rn(px, gx), __dmul_rn(py, gy)), __dmul_rn(pz, gz));
            const double a2 = __dadd_rn(__dadd_rn(__dmul_rn(px, px), __dmul_rn(py, py)), __dmul_rn(pz, pz));
            const double b2 = __dadd_rn(__dadd_rn(__dmul_rn(gx, gx), __dmul_rn(gy, gy)), __dmul_rn(gz, gz));
            const double cc = d / __dmul_rn(sqrt(a2), sqrt(b2));
            valid[j] = a2 > 0.0 && b2 > 0.0 && __builtin_isfinite(cc);
            c[j] = valid[j] ? fmin(fmax(cc, -1.0), 1.0) : 0.0;
            if (mask_f) m[j] = mask_f[p];
        }
        // bin = #{ j : c <= edges[j] } over the strictly decreasing table: four searches in step
        int lo[4] = {0, 0, 0, 0}, hi[4] = {kEdges, kEdges, kEdges, kEdges};
#pragma unroll 1
        for (int it = 0; it < 10; ++it) {            // 2^10 > 719
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int mid = (lo[j] + hi[j]) >> 1;      // lo == hi: mid == lo <= 719, the padding entry, never "<="
                const bool le = lo[j] < hi[j] && c[j] <= edges[mid];
                const bool gtb = lo[j] < hi[j] && !le;
                lo[j] = le ? mid + 1 : lo[j];
                hi[j] = gtb ? mid : hi[j];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double th = 0.0;
            if (valid[j]) th = acos(c[j]) * kDegPerRad;
            if (err_f && x0 + j < g.W) err_f[row + x0 + j] = valid[j] ? (float)th : __builtin_nanf("");
            if (!pass[j]) continue;
            const double th2 = __dmul_rn(th, th);
#pragma unroll
            for (int k = 0; k < kMaxK; ++k) {
                if (k < K) {
                    if (in_class(cls, k, m[j])) {
                        if (valid[j]) {
                            atomicAdd(&hist[k * kBins + lo[j]], 1u);
                            s[k][0] += th;
                            s[k][1] += th2;
                        } else {
                            atomicAdd(&bad[k], 1u);
                        }
                    }
                }
            }
        }
    }

    flush_records<Rec>(s, wsum, bad, hist, stats, ws, img, K);
}

inline int groups_of(int H, int W) { return groups_for(H > 0 && W > 0 ? (long)H * ((W + 3L) / 4) : 0); }      // items: quads

inline size_t lds_bytes(int K) {
    return (size_t)kBins * 8 + (size_t)kWaves * kMaxK * 2 * 8 + (size_t)kMaxK * 4 + (size_t)K * kBins * 4;
}

}  // namespace

extern "C" size_t pd_normals_stats_workspace(int N, int H, int W, int K) {
    return records_workspace(N, K, groups_of(H, W));
}

extern "C" int pd_normals_stats(const void* pred, long ld, const void* gtn, const void* gt, const void* mask,
                                const int* classes, int K, const void* cos_edges, int gate, void* err_deg, void* stats,
                                void* workspace, size_t ws_bytes, int N, int H, int W, float min_depth, float max_depth,
                                void* stream) {
    PD_REQUIRE(N >= 0 && H > 0 && W > 0, "pd_normals_stats: bad shape (N = %d, H = %d, W = %d)", N, H, W);
    PD_REQUIRE(pred && gtn && gt && classes && cos_edges && stats && workspace,
               "pd_normals_stats: pred, gtn, gt, classes, cos_edges, stats and workspace must not be null");
    Classes cls;
    if (int e = parse_classes("pd_normals_stats", classes, K, mask != nullptr, &cls)) return e;
    PD_REQUIRE(ld >= 3, "pd_normals_stats: the pixel stride ld = %ld must be at least 3", ld);
    PD_REQUIRE(gate == 0 || gate == 1, "pd_normals_stats: gate = %d, must be 0 (centre) or 1 (3x3 window)", gate);
    PD_REQUIRE(pd::aligned16(gtn) && pd::aligned16(stats) && pd::aligned16(workspace),
               "pd_normals_stats: gtn, stats and workspace must be 16-byte aligned");
    PD_REQUIRE((long)H * W <= (1L << 30), "pd_normals_stats: a frame of %d x %d is too large for the kernel's index arithmetic",
               H, W);
    const size_t need = pd_normals_stats_workspace(N, H, W, K);
    PD_REQUIRE(ws_bytes >= need, "pd_normals_stats: workspace too small (%zu bytes, pd_normals_stats_workspace asks for %zu)",
               ws_bytes, need);
    if (N == 0) return PD_OK;
    hipStream_t st = (hipStream_t)stream;
    Geo g;
    g.H = (unsigned)H; g.W = (unsigned)W; g.Q = (unsigned)((W + 3) / 4); g.items = g.H * g.Q;
    g.G = (unsigned)groups_of(H, W);
    g.K = K; g.gate = gate; g.ld = ld; g.min_d = min_depth; g.max_d = max_depth;
    const size_t frame = (size_t)H * W;
    run_records<Rec>(stats, workspace, N, K, (int)g.G, st, [&](long n0, long nb, unsigned* rec, double* part) {
        hipLaunchKernelGGL(nstat_kernel, dim3((unsigned)(nb * g.G)), dim3(kThreads), lds_bytes(K), st,
                           static_cast<const float*>(pred) + (size_t)n0 * frame * (size_t)ld,
                           static_cast<const float4*>(gtn) + (size_t)n0 * frame, static_cast<const float*>(gt) + (size_t)n0 * frame,
                           mask ? static_cast<const int*>(mask) + (size_t)n0 * frame : nullptr,
                           static_cast<const double*>(cos_edges),
                           err_deg ? static_cast<float*>(err_deg) + (size_t)n0 * frame : nullptr, rec, part, cls, g);
    });
    return pd::check_launch("pd_normals_stats");
}
