// The depth-uncertainty loss: the decoder's sigmoid uncertainty head u in [0, 1] read as the scale b of a Laplace error model
// of the predicted depth, log b = log b_lo + u log(b_hi / b_lo), and trained with the negative log-likelihood of the
// ground truth,
//     L = sum m (|g - d| / b + log 2b) / sum m,      m = (min_depth <= g <= max_depth) and valid and u finite.
// Definition: include/polardepth.h; NumPy statement: tests/unc_loss_ref.py.
//
// uloss_fwd_kernel: purely streaming.  One work item = one pixel, or four neighbours of a row where the width, the pitch and
// the pointers allow 16-byte accesses (PX = 4).  u is sampled from its [hs, ws] map by pd_up::sample (the align_corners=False
// rule of pd_disp_to_depth, fp32); a non-finite sample takes the pixel out; everything after it is fp64.  A lane carries four fp64 sums, reduced in the fixed lane / wave /
// workgroup order of frame_reduce.hpp into one row per workgroup; uloss_finalize_kernel (one workgroup) adds the rows and
// forms the value.  No atomics.
//
// uloss_bwd_kernel: the same decode and the same per-pixel quantities formed again (no state passes between the two
// kernels but the forward's sum m), the two gradients rounded once to fp32.  g_up is the gradient at full resolution;
// pd_up_gather_bwd folds it to the head's size.
#include "pd_common.h"
#include "frame_reduce.hpp"
#include "up_index.hpp"
#include "wave_ops.hpp"

#include <cmath>

namespace {

using pd_frames::block_rows;
using pd_frames::finalize_rows;
using pd_wave::divmod;

constexpr int LT = pd_frames::RT;
constexpr int kSums = PD_ULOSS_SUMS;
static_assert(kSums == 4, "sum e / b, sum log 2b, sum m, sum b");
constexpr double kLn2 = 0.6931471805599453;                     // M_LN2

struct Geo {
    int N, H, W, hs, ws;
    size_t ldg;                   // row pitch of gt, in elements
    float min_d, max_d, sh, sw;
    double log_lo, log_ratio;     // log b_lo, log(b_hi / b_lo)
};

// what a pixel under the mask contributes
struct Pix {
    double e, b, logb, diff;      // |g - d|, the scale, its logarithm, d - g
};
__device__ __forceinline__ Pix pix_of(float g, float d, float u, const Geo& q) {
    Pix p;
    p.logb = fma((double)u, q.log_ratio, q.log_lo);
    p.b = exp(p.logb);
    p.diff = (double)d - (double)g;
    p.e = fabs(p.diff);
    return p;
}

template <int PX>
__device__ __forceinline__ void load(const float* p, float (&v)[PX]) {
    if constexpr (PX == 4) { const float4 t = *reinterpret_cast<const float4*>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    else v[0] = *p;
}
template <int PX>
__device__ __forceinline__ void store(float* p, const float (&v)[PX]) {
    if constexpr (PX == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}
template <int PX>
__device__ __forceinline__ void load_valid(const unsigned char* p, bool (&v)[PX]) {
    if constexpr (PX == 4) { const uchar4 t = *reinterpret_cast<const uchar4*>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    else v[0] = *p != 0;
}

// item -> (n, y, x0) of its first pixel, the offsets of that pixel in the contiguous maps and in gt
template <int PX>
__device__ __forceinline__ void decode(long item, const Geo& q, long& n, int& y, int& x0, size_t& i, size_t& ig) {
    int xq;
    const long t = divmod(item, q.W / PX, xq);
    n = divmod(t, q.H, y);
    x0 = xq * PX;
    i = ((size_t)n * q.H + y) * (size_t)q.W + x0;
    ig = ((size_t)n * q.H + y) * q.ldg + x0;
}

template <int PX>
__global__ __launch_bounds__(LT) void uloss_fwd_kernel(const float* __restrict__ depth, const float* __restrict__ gt,
                                                       const float* __restrict__ unc, const unsigned char* __restrict__ valid,
                                                       float2* __restrict__ maps, double* __restrict__ partial, Geo q) {
    __shared__ double sm[4 * kSums];
    const long items = (long)q.N * q.H * (q.W / PX);
    const float nanf_ = __builtin_nanf("");
    double acc[kSums] = {0.0, 0.0, 0.0, 0.0};
    for (long item = blockIdx.x * (long)LT + threadIdx.x; item < items; item += (long)gridDim.x * LT) {
        long n; int y, x0; size_t i, ig;
        decode<PX>(item, q, n, y, x0, i, ig);
        float g[PX], d[PX];
        bool ok[PX] = {};
        load<PX>(gt + ig, g);
        load<PX>(depth + i, d);
        if (valid) load_valid<PX>(valid + i, ok);
        const float* um = unc + (size_t)n * q.hs * q.ws;
        float term[PX], bm[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const bool m = g[j] >= q.min_d && g[j] <= q.max_d && (!valid || ok[j]);      // NaN fails
            const float u = m ? pd_up::sample(um, q.hs, q.ws, q.sh, q.sw, x0 + j, y) : 0.f;
            term[j] = bm[j] = nanf_;
            if (m && __builtin_isfinite(u)) {            // a non-finite u takes the pixel out
                const Pix p = pix_of(g[j], d[j], u, q);
                const double r = p.e / p.b, l2b = p.logb + kLn2;
                acc[0] += r;
                acc[1] += l2b;
                acc[2] += 1.0;
                acc[3] += p.b;
                term[j] = (float)(r + l2b);
                bm[j] = (float)p.b;
            }
        }
        if (maps) {
            if constexpr (PX == 4) {
                float4* o = reinterpret_cast<float4*>(maps + i);
                o[0] = make_float4(term[0], bm[0], term[1], bm[1]);
                o[1] = make_float4(term[2], bm[2], term[3], bm[3]);
            } else {
                maps[i] = make_float2(term[0], bm[0]);
            }
        }
    }
    block_rows<kSums>(acc, sm, partial);
}

// sums[0..3]; value = (sums[0] + sums[1]) / sums[2], 0 where no pixel is under the mask
__global__ __launch_bounds__(256) void uloss_finalize_kernel(const double* __restrict__ partial, int rows, double* __restrict__ sums,
                                                             float* __restrict__ value) {
    __shared__ double sm[kSums * 256];
    double out[kSums];
    finalize_rows<kSums>(partial, rows, sm, out);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) sums[k] = out[k];
        value[0] = out[2] > 0.0 ? (float)((out[0] + out[1]) / out[2]) : 0.f;
    }
}

template <int PX>
__global__ __launch_bounds__(LT) void uloss_bwd_kernel(const float* __restrict__ depth, const float* __restrict__ gt,
                                                       const float* __restrict__ unc, const unsigned char* __restrict__ valid,
                                                       const float* __restrict__ gvalue, const double* __restrict__ sums,
                                                       float* __restrict__ gdepth, float* __restrict__ gup, Geo q) {
    const long items = (long)q.N * q.H * (q.W / PX);
    const double c = sums[2] > 0.0 ? (double)gvalue[0] / sums[2] : 0.0;       // gout / sum m
    for (long item = blockIdx.x * (long)LT + threadIdx.x; item < items; item += (long)gridDim.x * LT) {
        long n; int y, x0; size_t i, ig;
        decode<PX>(item, q, n, y, x0, i, ig);
        float g[PX], d[PX];
        bool ok[PX] = {};
        load<PX>(gt + ig, g);
        load<PX>(depth + i, d);
        if (valid) load_valid<PX>(valid + i, ok);
        const float* um = unc + (size_t)n * q.hs * q.ws;
        float gd[PX], gu[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const bool m = g[j] >= q.min_d && g[j] <= q.max_d && (!valid || ok[j]);
            const float u = m ? pd_up::sample(um, q.hs, q.ws, q.sh, q.sw, x0 + j, y) : 0.f;
            gd[j] = gu[j] = 0.f;
            if (m && __builtin_isfinite(u)) {
                const Pix p = pix_of(g[j], d[j], u, q);
                const double s = p.diff > 0.0 ? 1.0 : (p.diff < 0.0 ? -1.0 : p.diff);      // 0 at d == g, NaN stays NaN
                gd[j] = (float)(c * s / p.b);
                gu[j] = (float)(c * (1.0 - p.e / p.b) * q.log_ratio);
            }
        }
        if (gdepth) store<PX>(gdepth + i, gd);
        store<PX>(gup + i, gu);
    }
}

// what both entry points refuse
inline int common_args(const char* who, const void* depth, const void* gt, long ldg, const void* unc, int hs, int ws,
                       float min_depth, float max_depth, double b_lo, double b_hi, int N, int H, int W) {
    PD_REQUIRE(N >= 0 && H > 0 && W > 0, "%s: bad shape (N = %d, H = %d, W = %d)", who, N, H, W);
    PD_REQUIRE(hs > 0 && ws > 0 && hs <= H && ws <= W, "%s: bad shape of the uncertainty map (%d x %d for a frame of %d x %d)", who,
               hs, ws, H, W);
    PD_REQUIRE(depth && gt && unc, "%s: depth, gt and unc must not be null", who);
    PD_REQUIRE(ldg >= W, "%s: the row pitch ldg = %ld must be at least W = %d", who, ldg, W);
    PD_REQUIRE(min_depth > 0.f && max_depth > min_depth, "%s: the depth range [%g, %g] must be positive and not empty", who,
               (double)min_depth, (double)max_depth);
    PD_REQUIRE(b_lo > 0.0 && b_lo < b_hi && std::isfinite(b_hi), "%s: the scale range needs 0 < b_lo < b_hi < inf, got (%g, %g)", who,
               b_lo, b_hi);
    PD_REQUIRE((long)H * W <= (1L << 30), "%s: a frame of %d x %d is too large for the kernel's index arithmetic", who, H, W);
    return PD_OK;
}

inline Geo geo_of(long ldg, int hs, int ws, float min_depth, float max_depth, double b_lo, double b_hi, int N, int H, int W) {
    Geo q;
    q.N = N; q.H = H; q.W = W; q.hs = hs; q.ws = ws;
    q.ldg = (size_t)ldg;
    q.min_d = min_depth; q.max_d = max_depth;
    q.sh = (float)hs / H; q.sw = (float)ws / W;
    q.log_lo = std::log(b_lo); q.log_ratio = std::log(b_hi / b_lo);
    return q;
}

inline bool quads_ok(int W, long ldg, std::initializer_list<const void*> p16, const void* valid) {
    if (W % 4 != 0 || ldg % 4 != 0 || !pd::aligned4(valid)) return false;
    for (const void* p : p16)
        if (!pd::aligned16(p)) return false;
    return true;
}

}  // namespace

extern "C" int pd_unc_loss_rows(int N, int H, int W) {
    return (int)pd::flat_grid(N > 0 && H > 0 && W > 0 ? (long)N * H * W : 0);
}

extern "C" int pd_unc_loss_fwd(const void* depth, const void* gt, long ldg, const void* unc, int hs, int ws, const void* valid,
                               float min_depth, float max_depth, double b_lo, double b_hi, void* sums, void* value, void* maps,
                               void* workspace, size_t ws_bytes, int N, int H, int W, void* stream) {
    const char* who = "pd_unc_loss_fwd";
    if (int e = common_args(who, depth, gt, ldg, unc, hs, ws, min_depth, max_depth, b_lo, b_hi, N, H, W)) return e;
    PD_REQUIRE(sums && value && workspace, "%s: sums, value and workspace must not be null", who);
    PD_REQUIRE(pd::aligned16(workspace) && pd::aligned8(sums) && pd::aligned8(maps) && pd::aligned4(depth) && pd::aligned4(gt),
               "%s: workspace must be 16-byte aligned, sums and maps 8-byte aligned, depth and gt 4-byte aligned", who);
    const int rows_max = pd_unc_loss_rows(N, H, W);
    const size_t need = (size_t)rows_max * kSums * sizeof(double);
    PD_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu bytes, pd_unc_loss_rows(N, H, W) * %d * 8 = %zu are needed)", who,
               ws_bytes, kSums, need);
    if (N == 0) return PD_OK;
    hipStream_t st = (hipStream_t)stream;
    const Geo q = geo_of(ldg, hs, ws, min_depth, max_depth, b_lo, b_hi, N, H, W);
    const bool vec = quads_ok(W, ldg, {depth, gt, maps}, valid);
    const int rows = (int)pd::flat_grid((long)N * H * (vec ? W / 4 : W));       // <= rows_max
    hipLaunchKernelGGL(vec ? uloss_fwd_kernel<4> : uloss_fwd_kernel<1>, dim3((unsigned)rows), dim3(LT), 0, st,
                       static_cast<const float*>(depth), static_cast<const float*>(gt), static_cast<const float*>(unc),
                       static_cast<const unsigned char*>(valid), static_cast<float2*>(maps), static_cast<double*>(workspace), q);
    hipLaunchKernelGGL(uloss_finalize_kernel, dim3(1), dim3(256), 0, st, static_cast<const double*>(workspace), rows,
                       static_cast<double*>(sums), static_cast<float*>(value));
    return pd::check_launch(who);
}

extern "C" int pd_unc_loss_bwd(const void* depth, const void* gt, long ldg, const void* unc, int hs, int ws, const void* valid,
                               float min_depth, float max_depth, double b_lo, double b_hi, const void* gvalue, const void* sums,
                               void* gdepth, void* gup, int N, int H, int W, void* stream) {
    const char* who = "pd_unc_loss_bwd";
    if (int e = common_args(who, depth, gt, ldg, unc, hs, ws, min_depth, max_depth, b_lo, b_hi, N, H, W)) return e;
    PD_REQUIRE(gvalue && sums && gup, "%s: gvalue, sums and gup must not be null (gdepth may be: the detached mode)", who);
    PD_REQUIRE(pd::aligned8(sums) && pd::aligned4(depth) && pd::aligned4(gt) && pd::aligned4(gdepth) && pd::aligned4(gup),
               "%s: sums must be 8-byte aligned, the maps 4-byte aligned", who);
    if (N == 0) return PD_OK;
    const Geo q = geo_of(ldg, hs, ws, min_depth, max_depth, b_lo, b_hi, N, H, W);
    const bool vec = quads_ok(W, ldg, {depth, gt, gdepth, gup}, valid);
    const unsigned grid = pd::flat_grid((long)N * H * (vec ? W / 4 : W));
    hipLaunchKernelGGL(vec ? uloss_bwd_kernel<4> : uloss_bwd_kernel<1>, dim3(grid), dim3(LT), 0, (hipStream_t)stream,
                       static_cast<const float*>(depth), static_cast<const float*>(gt), static_cast<const float*>(unc),
                       static_cast<const unsigned char*>(valid), static_cast<const float*>(gvalue),
                       static_cast<const double*>(sums), static_cast<float*>(gdepth), static_cast<float*>(gup), q);
    return pd::check_launch(who);
}
