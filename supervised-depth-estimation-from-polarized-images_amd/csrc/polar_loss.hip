// The polarimetric normals loss: pd_polar_normals_stats (csrc/polar_normals_stats.hip) turned into a training term on a depth
// map.  Per pixel, p = the fp32 normal of the depth map exactly as pd_gt_normals forms it without a depth range
// (depth_normals.hpp: sobel_xyz, cross, normalize12); from p on, the gates, the orientation, the six candidates, the azimuth
// branch and aolp_sign are the evaluator's, decision for decision, in fp64 in the header's operation order.  The two figures
// of the evaluator become two smooth per-pixel terms on those decisions,
//     l_n = 1 - c*                   (1 - cos of the evaluator's n_deg)
//     l_a = 1 - m^2 / (t2 u2)        (sin^2 of the evaluator's az_deg, smooth at m = 0, clamped to [0, 1])
// and L_n = sum w l_n / sum w, L_a = sum w l_a / sum w with w = rho or 1.  Definition: include/polardepth.h; NumPy statement:
// tests/polar_loss_ref.py.
//
// ploss_fwd_kernel: one work item = one pixel, grid-stride over the batch; a lane carries four fp64 sums and seven counts
// (as doubles: integers below 2^53 add exactly), reduced in the fixed lane / wave / workgroup order of frame_reduce.hpp into
// one row per workgroup; ploss_finalize_kernel (one workgroup) adds the rows and forms the two values.  No atomics.
// The decisions of a pixel leave the forward pass as one byte of `state`.
//
// ploss_bwd_kernel: built like sup_bwd_fused_kernel of loss.hip.  Per 8 x 64 tile, every pixel of the 10 x 66 halo reads its
// state byte; a counted pixel forms dL/dp in fp64 from the winner and the branch the byte names (data, not decisions made
// again), rounds it once to fp32 and takes it through normalize12 and the cross product to (dA, dB) in LDS; the 3 x 3
// transposed Sobel gather runs from there.  No [N,H,W,6] intermediate reaches memory.
//
// RAY (a compile-time parameter of both kernels): the terms are formed in the frame of the pixel's viewing ray
// (ray_frame.hpp).  Forward: p' = R(x, y) p right after the conversion to fp64, and p' stands for p from the `bad` gate on.
// Backward: the halo evaluation rebuilds p' from p, forms dL/dp' as before and takes it back with R^T in fp64 before the
// single rounding.  There is no gradient with respect to K.
#include "pd_common.h"
#include "depth_normals.hpp"
#include "ray_frame.hpp"
#include "frame_reduce.hpp"
#include "wave_ops.hpp"

#include <cfloat>
#include <cmath>

namespace {

using namespace pd_dn;
using pd_frames::block_rows;
using pd_frames::finalize_rows;
using pd_wave::divmod;

constexpr int LT = pd_frames::RT;
constexpr int kSums = PD_PLOSS_SUMS, kCounters = PD_PLOSS_COUNTERS, kRow = kSums + kCounters;
static_assert(kRow == 11 && PD_PLOSS_RECORD_BYTES == 8 * (kRow + 1), "record layout");
// the counters, in the record's order
enum { cN = 0, cA = 1, cDolpOut = 2, cBad = 3, cFrontal = 4, cSpec = 5, cFlipped = 6 };
enum { gateNone = 0, gateInvalid = 1, gateDolpOut = 2, gateBad = 3 };
enum { brNone = 0, brD = 1, brS = 2 };
static_assert(PD_PLOSS_STATE_WINNER == 0x07 && PD_PLOSS_STATE_NEGATED == 0x08 && PD_PLOSS_STATE_BRANCH_SHIFT == 4 &&
              PD_PLOSS_STATE_GATE_SHIFT == 6, "state byte");

struct Geo {
    int N, H, W;
    int weighted;
    size_t ldp, plane;            // row pitch of the planar inputs; one plane = H * ldp
    double rho_min, rho_max, tilt2_min, sign;
};

// p of pixel (x, y): what gt_normals_kernel writes when its depth range is the whole of fp32 (a non-finite depth gives zero)
__device__ __forceinline__ V3 depth_normal(const float* __restrict__ D, int H, int W, int x, int y, Cam c, V3& A, V3& B, float& nv) {
    const float d = D[(long)y * W + x];
    A = V3{0, 0, 0}; B = V3{0, 0, 0}; nv = 0.f;
    if (!(d >= -FLT_MAX && d <= FLT_MAX)) return V3{0, 0, 0};
    sobel_xyz(D, H, W, x, y, c, A, B);
    return normalize12(cross(A, B), nv);
}

// the fp64 view of a pixel: p (oriented), the candidates with cy' = aolp_sign * cy
struct Pix {
    double px, py, pz, a2;
    double cx[3], cy[3], cz[3], b2[3];
    bool fin, any;
};
template <bool RAY>
__device__ __forceinline__ void load_pix(Pix& q, V3 p, Cam c, int x, int y, const float* __restrict__ pol_f, size_t plane,
                                         size_t po, double sign) {
    q.px = (double)p.x; q.py = (double)p.y; q.pz = (double)p.z;
    if constexpr (RAY) pd_ray::rotate(pd_ray::make(c, x, y), q.px, q.py, q.pz);
    q.a2 = (q.px * q.px + q.py * q.py) + q.pz * q.pz;
    q.fin = true; q.any = false;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        q.cx[b] = (double)pol_f[(size_t)(3 * b) * plane + po];
        q.cy[b] = sign * (double)pol_f[(size_t)(3 * b + 1) * plane + po];
        q.cz[b] = (double)pol_f[(size_t)(3 * b + 2) * plane + po];
        q.fin = q.fin && __builtin_isfinite(q.cx[b]) && __builtin_isfinite(q.cy[b]) && __builtin_isfinite(q.cz[b]);
        q.b2[b] = (q.cx[b] * q.cx[b] + q.cy[b] * q.cy[b]) + q.cz[b] * q.cz[b];
        q.any = q.any || q.b2[b] > 0.0;
    }
}
__device__ __forceinline__ void negate(Pix& q) { q.px = -q.px; q.py = -q.py; q.pz = -q.pz; }

template <bool RAY>
__global__ __launch_bounds__(LT) void ploss_fwd_kernel(const float* __restrict__ depth, const float* __restrict__ K,
                                                       const float* __restrict__ pol, const float* __restrict__ xolp,
                                                       const unsigned char* __restrict__ valid,
                                                       unsigned char* __restrict__ state, float2* __restrict__ maps,
                                                       double* __restrict__ partial, Geo g) {
    __shared__ double sm[4 * kRow];
    const long total = (long)g.N * g.H * g.W;
    const float nanf_ = __builtin_nanf("");
    double acc[kRow];
#pragma unroll
    for (int k = 0; k < kRow; ++k) acc[k] = 0.0;

    for (long i = blockIdx.x * (long)LT + threadIdx.x; i < total; i += (long)gridDim.x * LT) {
        int x, y;
        const long t = divmod(i, g.W, x);
        const long n = divmod(t, g.H, y);
        const size_t po = (size_t)y * g.ldp + x;
        int gate = gateNone, win = 0, branch = brNone;
        bool neg = false;
        float ln = nanf_, la = nanf_;
        if (valid && !valid[i]) {
            gate = gateInvalid;
        } else {
            const double rho = (double)xolp[(size_t)n * 2 * g.plane + po];                 // channel 0
            if (!__builtin_isfinite(rho) || rho < g.rho_min || rho > g.rho_max) {
                gate = gateDolpOut;
                acc[kSums + cDolpOut] += 1.0;
            } else {
                V3 A, B; float nv;
                const Cam c = load_cam(K, n);
                const V3 p = depth_normal(depth + n * g.H * g.W, g.H, g.W, x, y, c, A, B, nv);
                Pix q;
                load_pix<RAY>(q, p, c, x, y, pol + (size_t)n * 9 * g.plane, g.plane, po, g.sign);
                if (!(__builtin_isfinite(q.a2) && q.a2 > 0.0 && q.fin && q.any)) {
                    gate = gateBad;
                    acc[kSums + cBad] += 1.0;
                } else {
                    const double w = g.weighted ? rho : 1.0;
                    if (q.pz < 0.0) { neg = true; negate(q); }
                    // ---- normal term: the evaluator's six cosines, first strict maximum
                    const double sa = sqrt(q.a2);
                    double best = -HUGE_VAL;
                    int wi = -1;
#pragma unroll
                    for (int b = 0; b < 3; ++b) {
                        if (q.b2[b] > 0.0) {
                            const double mm = q.px * q.cx[b] + q.py * q.cy[b], qq = q.pz * q.cz[b];
                            const double den = sa * sqrt(q.b2[b]);
                            const double cp = (mm + qq) / den, cm = (-mm + qq) / den;
                            if (__builtin_isfinite(cp) && cp > best) { best = cp; wi = 2 * b; }
                            if (__builtin_isfinite(cm) && cm > best) { best = cm; wi = 2 * b + 1; }
                        }
                    }
                    if (wi >= 0) {                    // else: every cosine non-finite, not reachable from fp32 inputs
                        win = 1 + wi;
                        const double l = 1.0 - fmin(fmax(best, -1.0), 1.0);
                        ln = (float)l;
                        acc[0] += w * l;
                        acc[1] += w;
                        acc[kSums + cN] += 1.0;
                        if (wi >= 2) acc[kSums + cSpec] += 1.0;
                        if (wi & 1) acc[kSums + cFlipped] += 1.0;
                    }
                    // ---- azimuth term: the evaluator's frontal gate and branch, then sin^2 without a square root
                    const double t2 = q.px * q.px + q.py * q.py;
                    const double ud = q.cx[0] * q.cx[0] + q.cy[0] * q.cy[0], us = q.cx[1] * q.cx[1] + q.cy[1] * q.cy[1];
                    if (t2 <= g.tilt2_min * q.a2 || !(ud > 0.0 || us > 0.0)) {
                        acc[kSums + cFrontal] += 1.0;
                    } else {
                        const double st = sqrt(t2);
                        const double md = q.px * q.cx[0] + q.py * q.cy[0], ms = q.px * q.cx[1] + q.py * q.cy[1];
                        double cd = -1.0, cs = -1.0;
                        if (ud > 0.0) cd = fmin(fabs(md) / (st * sqrt(ud)), 1.0);
                        if (us > 0.0) cs = fmin(fabs(ms) / (st * sqrt(us)), 1.0);
                        const bool spec = cs > cd;
                        branch = spec ? brS : brD;
                        const double m = spec ? ms : md, u2 = spec ? us : ud;
                        const double l = fmin(fmax(1.0 - (m * m) / (t2 * u2), 0.0), 1.0);
                        la = (float)l;
                        acc[2] += w * l;
                        acc[3] += w;
                        acc[kSums + cA] += 1.0;
                    }
                }
            }
        }
        state[i] = (unsigned char)(win | (neg ? PD_PLOSS_STATE_NEGATED : 0) | (branch << PD_PLOSS_STATE_BRANCH_SHIFT) |
                                   (gate << PD_PLOSS_STATE_GATE_SHIFT));
        if (maps) maps[i] = make_float2(ln, la);
    }
    block_rows<kRow>(acc, sm, partial);
}

// sums[0..3] doubles, sums[4..10] int64 counters, sums[11] zero; values = (L_n, L_a), 0 where sum w is 0
__global__ __launch_bounds__(256) void ploss_finalize_kernel(const double* __restrict__ partial, int rows, double* __restrict__ sums,
                                                             float* __restrict__ values) {
    __shared__ double sm[kRow * 256];
    double out[kRow];
    finalize_rows<kRow>(partial, rows, sm, out);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) sums[k] = out[k];
        long long* cnt = reinterpret_cast<long long*>(sums);
#pragma unroll
        for (int k = kSums; k < kRow; ++k) cnt[k] = (long long)out[k];
        cnt[kRow] = 0;
        values[0] = out[1] > 0.0 ? (float)(out[0] / out[1]) : 0.f;
        values[1] = out[3] > 0.0 ? (float)(out[2] / out[3]) : 0.f;
    }
}

// dL/d(nn) of a counted pixel, fp64, rounded once: the winner and the branch are what `st` says, so only their candidates are
// read.  cand = the pixel's entry of plane 0; wn_ = g_n w / sum w, wa_ = g_a w / sum w
template <bool RAY>
__device__ __forceinline__ V3 grad_normal(V3 nn, Cam c, int x, int y, const float* __restrict__ cand, size_t plane, double sign,
                                          int st, double wn_, double wa_) {
    const bool neg = (st & PD_PLOSS_STATE_NEGATED) != 0;
    double ux = (double)nn.x, uy = (double)nn.y, uz = (double)nn.z;
    pd_ray::Frame fr{0.0, 0.0, 1.0};
    if constexpr (RAY) {
        fr = pd_ray::make(c, x, y);
        pd_ray::rotate(fr, ux, uy, uz);               // the forward pass's p', before the orientation
    }
    const double a2 = (ux * ux + uy * uy) + uz * uz;                  // negation is exact: the forward pass's a2
    const double px = neg ? -ux : ux, py = neg ? -uy : uy, pz = neg ? -uz : uz;
    double gx = 0.0, gy = 0.0, gz = 0.0;
    const int win = st & PD_PLOSS_STATE_WINNER;
    if (win != 0 && wn_ != 0.0) {
        const float* cb = cand + (size_t)(3 * ((win - 1) >> 1)) * plane;
        const double sg = ((win - 1) & 1) ? -1.0 : 1.0;
        const double cx = sg * (double)cb[0], cy = sg * (sign * (double)cb[plane]), cz = (double)cb[2 * plane];
        const double b2 = (cx * cx + cy * cy) + cz * cz;
        const double sa = sqrt(a2), sb = sqrt(b2);
        const double c = ((px * cx + py * cy) + pz * cz) / (sa * sb);
        if (c >= -1.0 && c <= 1.0) {                  // a clamped c* has no gradient
            const double f = -wn_ / sa, ca = c / sa;
            gx = f * (cx / sb - ca * px); gy = f * (cy / sb - ca * py); gz = f * (cz / sb - ca * pz);
        }
    }
    const int branch = (st >> PD_PLOSS_STATE_BRANCH_SHIFT) & 3;
    if (branch != brNone && wa_ != 0.0) {
        const float* cb = cand + (branch == brS ? 3 * plane : (size_t)0);
        const double cx = (double)cb[0], cy = sign * (double)cb[plane];
        const double t2 = px * px + py * py, u2 = cx * cx + cy * cy;
        const double m = px * cx + py * cy;
        if (1.0 - (m * m) / (t2 * u2) >= 0.0) {       // a clamped l_a has no gradient
            // l_a = 1 - m^2 / (t2 u2):  d l_a / d(px, py) = -2 m / (t2 u2) ((cx, cy) - m / t2 (px, py))
            const double f = -wa_ * 2.0 * m / (t2 * u2), mt = m / t2;
            gx += f * (cx - mt * px); gy += f * (cy - mt * py);
        }
    }
    if constexpr (RAY) pd_ray::rotate_t(fr, gx, gy, gz);              // dL/dp = R^T dL/dp'
    if (neg) { gx = -gx; gy = -gy; gz = -gz; }
    return V3{(float)gx, (float)gy, (float)gz};
}

template <bool RAY>
__global__ __launch_bounds__(LT) void ploss_bwd_kernel(const float* __restrict__ depth, const float* __restrict__ K,
                                                       const float* __restrict__ pol, const float* __restrict__ xolp,
                                                       const unsigned char* __restrict__ state, const float* __restrict__ gv,
                                                       const double* __restrict__ sums, float* __restrict__ gdepth, Geo g,
                                                       int tiles_h, int tiles_w, int ntiles) {
    __shared__ float abl[6][SB_HP];
    const int H = g.H, W = g.W;
    // g_n / sum w and g_a / sum w; a term without weight has no gradient
    const double cn = sums[1] > 0.0 ? (double)gv[0] / sums[1] : 0.0;
    const double ca = sums[3] > 0.0 ? (double)gv[1] / sums[3] : 0.0;
    for (int tile = (int)blockIdx.x; tile < ntiles; tile += (int)gridDim.x) {
        const int tw = tile % tiles_w, th = (tile / tiles_w) % tiles_h;
        const long n = tile / (tiles_w * tiles_h);
        const int h0 = th * SB_TR, w0 = tw * SB_TW;
        const Cam c = load_cam(K, n);
        const float* dn = depth + n * H * W;
        const float* pol_f = pol + (size_t)n * 9 * g.plane;
        const float* rho_f = xolp + (size_t)n * 2 * g.plane;
        __syncthreads();
        for (int s = threadIdx.x; s < SB_HP; s += LT) {
            const int r = s / SB_HC, cc = s - r * SB_HC;
            const int y = h0 - 1 + r, x = w0 - 1 + cc;
            V3 dA{0, 0, 0}, dB{0, 0, 0};
            if (y >= 0 && y < H && x >= 0 && x < W) {
                const int st = state[(n * H + y) * (long)W + x];
                if ((st >> PD_PLOSS_STATE_GATE_SHIFT) == gateNone && (st & (PD_PLOSS_STATE_WINNER | PD_PLOSS_STATE_BRANCH)) != 0) {
                    const size_t po = (size_t)y * g.ldp + x;
                    V3 A, B; float nv;
                    const V3 nn = depth_normal(dn, H, W, x, y, c, A, B, nv);
                    const double w = g.weighted ? (double)rho_f[po] : 1.0;
                    const V3 wn = grad_normal<RAY>(nn, c, x, y, pol_f + po, g.plane, g.sign, st, cn * w, ca * w);
                    normal_grad_to_ab(wn, nn, nv, A, B, dA, dB);
                }
            }
            abl[0][s] = dA.x; abl[1][s] = dA.y; abl[2][s] = dA.z; abl[3][s] = dB.x; abl[4][s] = dB.y; abl[5][s] = dB.z;
        }
        __syncthreads();
        for (int o = threadIdx.x; o < SB_TR * SB_TW; o += LT) {
            const int r = o / SB_TW, cc = o - r * SB_TW;
            const int y = h0 + r, x = w0 + cc;
            if (y >= H || x >= W) continue;
            const V3 s = gather_ab(abl, x, y, h0, w0, H, W);
            gdepth[(n * H + y) * (long)W + x] = (x - c.cx) / c.fx * s.x + (y - c.cy) / c.fy * s.y + s.z;
        }
    }
}

// what both entry points refuse
inline int common_args(const char* who, const void* depth, const void* K, const void* pol_normals, const void* xolp, long ldp,
                       int aolp_sign, int dolp_weighted, int ray_frame, int N, int H, int W) {
    PD_REQUIRE(ray_frame == 0 || ray_frame == 1, "%s: ray_frame = %d must be 0 or 1", who, ray_frame);
    PD_REQUIRE(N >= 0 && H > 0 && W > 0, "%s: bad shape (N = %d, H = %d, W = %d)", who, N, H, W);
    PD_REQUIRE(depth && K && pol_normals && xolp, "%s: depth, K, pol_normals and xolp must not be null", who);
    PD_REQUIRE(ldp >= W, "%s: the row pitch ldp = %ld must be at least W = %d", who, ldp, W);
    PD_REQUIRE(aolp_sign == 1 || aolp_sign == -1, "%s: aolp_sign = %d must be +1 or -1", who, aolp_sign);
    PD_REQUIRE(dolp_weighted == 0 || dolp_weighted == 1, "%s: dolp_weighted = %d must be 0 or 1", who, dolp_weighted);
    PD_REQUIRE(pd::aligned16(pol_normals), "%s: pol_normals must be 16-byte aligned", who);
    PD_REQUIRE((long)H * W <= (1L << 30), "%s: a frame of %d x %d is too large for the kernel's index arithmetic", who, H, W);
    return PD_OK;
}

inline Geo geo_of(long ldp, int aolp_sign, int dolp_weighted, int N, int H, int W) {
    Geo g;
    g.N = N; g.H = H; g.W = W; g.weighted = dolp_weighted;
    g.ldp = (size_t)ldp; g.plane = (size_t)H * (size_t)ldp;
    g.rho_min = g.rho_max = g.tilt2_min = 0.0;
    g.sign = (double)aolp_sign;
    return g;
}

int fwd_call(const char* who, const void* depth, const void* K, const void* pol_normals, const void* xolp, long ldp,
             const void* valid, float rho_min, float rho_max, double tilt2_min, int aolp_sign, int dolp_weighted, int ray_frame,
             void* state, void* sums, void* values, void* maps, void* workspace, size_t ws_bytes, int N, int H, int W,
             void* stream);
int bwd_call(const char* who, const void* depth, const void* K, const void* pol_normals, const void* xolp, long ldp,
             const void* state, const void* gvalues, const void* sums, int aolp_sign, int dolp_weighted, int ray_frame,
             void* gdepth, int N, int H, int W, void* stream);

}  // namespace

extern "C" int pd_polar_loss_rows(int N, int H, int W) {
    return (int)pd::flat_grid(N > 0 && H > 0 && W > 0 ? (long)N * H * W : 0);
}

extern "C" int pd_polar_loss_fwd(const void* depth, const void* K, const void* pol_normals, const void* xolp, long ldp,
                                 const void* valid, float rho_min, float rho_max, double tilt2_min, int aolp_sign,
                                 int dolp_weighted, void* state, void* sums, void* values, void* maps, void* workspace,
                                 size_t ws_bytes, int N, int H, int W, void* stream) {
    return fwd_call("pd_polar_loss_fwd", depth, K, pol_normals, xolp, ldp, valid, rho_min, rho_max, tilt2_min, aolp_sign,
                    dolp_weighted, 0, state, sums, values, maps, workspace, ws_bytes, N, H, W, stream);
}

extern "C" int pd_polar_loss_fwd_ray(const void* depth, const void* K, const void* pol_normals, const void* xolp, long ldp,
                                     const void* valid, float rho_min, float rho_max, double tilt2_min, int aolp_sign,
                                     int dolp_weighted, int ray_frame, void* state, void* sums, void* values, void* maps,
                                     void* workspace, size_t ws_bytes, int N, int H, int W, void* stream) {
    return fwd_call("pd_polar_loss_fwd_ray", depth, K, pol_normals, xolp, ldp, valid, rho_min, rho_max, tilt2_min, aolp_sign,
                    dolp_weighted, ray_frame, state, sums, values, maps, workspace, ws_bytes, N, H, W, stream);
}

extern "C" int pd_polar_loss_bwd(const void* depth, const void* K, const void* pol_normals, const void* xolp, long ldp,
                                 const void* state, const void* gvalues, const void* sums, int aolp_sign, int dolp_weighted,
                                 void* gdepth, int N, int H, int W, void* stream) {
    return bwd_call("pd_polar_loss_bwd", depth, K, pol_normals, xolp, ldp, state, gvalues, sums, aolp_sign, dolp_weighted, 0,
                    gdepth, N, H, W, stream);
}

extern "C" int pd_polar_loss_bwd_ray(const void* depth, const void* K, const void* pol_normals, const void* xolp, long ldp,
                                     const void* state, const void* gvalues, const void* sums, int aolp_sign, int dolp_weighted,
                                     int ray_frame, void* gdepth, int N, int H, int W, void* stream) {
    return bwd_call("pd_polar_loss_bwd_ray", depth, K, pol_normals, xolp, ldp, state, gvalues, sums, aolp_sign, dolp_weighted,
                    ray_frame, gdepth, N, H, W, stream);
}

namespace {

int fwd_call(const char* who, const void* depth, const void* K, const void* pol_normals, const void* xolp, long ldp,
             const void* valid, float rho_min, float rho_max, double tilt2_min, int aolp_sign, int dolp_weighted, int ray_frame,
             void* state, void* sums, void* values, void* maps, void* workspace, size_t ws_bytes, int N, int H, int W,
             void* stream) {
    if (int e = common_args(who, depth, K, pol_normals, xolp, ldp, aolp_sign, dolp_weighted, ray_frame, N, H, W)) return e;
    PD_REQUIRE(state && sums && values && workspace, "%s: state, sums, values and workspace must not be null", who);
    PD_REQUIRE(std::isfinite(rho_min) && std::isfinite(rho_max) && rho_min <= rho_max,
               "%s: the DoLP range [rho_min = %g, rho_max = %g] must be finite and not inverted", who, (double)rho_min,
               (double)rho_max);
    PD_REQUIRE(tilt2_min >= 0.0 && tilt2_min < 1.0, "%s: tilt2_min = %g must be in [0, 1): it is a squared sine", who, tilt2_min);
    PD_REQUIRE(pd::aligned16(workspace) && pd::aligned8(sums) && pd::aligned8(maps),
               "%s: workspace must be 16-byte aligned, sums and maps 8-byte aligned", who);
    const int rows = pd_polar_loss_rows(N, H, W);
    const size_t need = (size_t)rows * kRow * sizeof(double);
    PD_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu bytes, pd_polar_loss_rows(N, H, W) * %d * 8 = %zu are needed)", who,
               ws_bytes, kRow, need);
    if (N == 0) return PD_OK;
    hipStream_t st = (hipStream_t)stream;
    Geo g = geo_of(ldp, aolp_sign, dolp_weighted, N, H, W);
    g.rho_min = (double)rho_min; g.rho_max = (double)rho_max; g.tilt2_min = tilt2_min;
    hipLaunchKernelGGL(ray_frame ? ploss_fwd_kernel<true> : ploss_fwd_kernel<false>, dim3((unsigned)rows), dim3(LT), 0, st, static_cast<const float*>(depth),
                       static_cast<const float*>(K), static_cast<const float*>(pol_normals), static_cast<const float*>(xolp),
                       static_cast<const unsigned char*>(valid), static_cast<unsigned char*>(state), static_cast<float2*>(maps),
                       static_cast<double*>(workspace), g);
    hipLaunchKernelGGL(ploss_finalize_kernel, dim3(1), dim3(256), 0, st, static_cast<const double*>(workspace), rows,
                       static_cast<double*>(sums), static_cast<float*>(values));
    return pd::check_launch(who);
}

int bwd_call(const char* who, const void* depth, const void* K, const void* pol_normals, const void* xolp, long ldp,
             const void* state, const void* gvalues, const void* sums, int aolp_sign, int dolp_weighted, int ray_frame,
             void* gdepth, int N, int H, int W, void* stream) {
    if (int e = common_args(who, depth, K, pol_normals, xolp, ldp, aolp_sign, dolp_weighted, ray_frame, N, H, W)) return e;
    PD_REQUIRE(state && gvalues && sums && gdepth, "%s: state, gvalues, sums and gdepth must not be null", who);
    PD_REQUIRE(pd::aligned8(sums), "%s: sums must be 8-byte aligned", who);
    const int tiles_h = (H + SB_TR - 1) / SB_TR, tiles_w = (W + SB_TW - 1) / SB_TW;
    const long ntiles = (long)N * tiles_h * tiles_w;
    PD_REQUIRE(ntiles < (1L << 31), "%s: a batch of %d frames of %d x %d has too many tiles", who, N, H, W);
    if (N == 0) return PD_OK;
    const Geo g = geo_of(ldp, aolp_sign, dolp_weighted, N, H, W);
    hipLaunchKernelGGL(ray_frame ? ploss_bwd_kernel<true> : ploss_bwd_kernel<false>, dim3((unsigned)(ntiles > PD_PLOSS_BWD_TILES_PER_TRIP ? PD_PLOSS_BWD_TILES_PER_TRIP : ntiles)),
                       dim3(LT), 0, (hipStream_t)stream, static_cast<const float*>(depth), static_cast<const float*>(K),
                       static_cast<const float*>(pol_normals), static_cast<const float*>(xolp),
                       static_cast<const unsigned char*>(state), static_cast<const float*>(gvalues),
                       static_cast<const double*>(sums), static_cast<float*>(gdepth), g, tiles_h, tiles_w, (int)ntiles);
    return pd::check_launch(who);
}

}  // namespace
