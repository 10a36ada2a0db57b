// Pose network tail: transformation_from_parameters and the end of PoseDecoder.forward, forward and backward.
//
// Reference restated:
//   layers.py:74-149        transformation_from_parameters / get_translation_matrix / rot_from_axisangle (angle + 1e-7)
//   pose_decoder.py:39-52   ("pose", 2) 1x1 convolution, mean over the plane, * 0.01, split into axisangle / translation
//   trainer.py:689-707      cam_T_cam (invert for f < 0) and cam_T_cam_inv from slot 0
// Written with tensor ops this is several hundred launches of a few elements each per step (norm, sin / cos, forty indexed
// assignments, two 4x4 products, each again for the inverse, and autograd's mirror of all that).  Here a pose is one thread
// and a decoder tail one workgroup per item: the spatial mean commutes with the 1x1 convolution, so the workgroup reduces
// the plane per channel first and multiplies a [Co, Cin] matrix with ONE vector.  Everything is fp64 inside from the fp32
// inputs and rounded once; every sum has a stated order; no atomics, no host synchronisation, capturable.
#include "pd_common.h"
#include "wave_ops.hpp"

namespace {

constexpr int PT = 256;                 // threads per workgroup of the head kernels (four wavefronts)
constexpr int POSE_MAX_CIN = 1024;

// ------------------------------------------------------------------ one pose, fp64
// everything the backward pass needs again is recomputed from (a, t): 20 flops and one sincos
struct Rot {
    double x, y, z, sa, ca, C, s, angle;   // axis, sin / cos(angle), 1 - cos, angle + 1e-7, angle
    double R[3][3];
};

__device__ __forceinline__ Rot rot_of(const double (&a)[3]) {
    Rot r;
    r.angle = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    r.s = r.angle + 1e-7;
    r.x = a[0] / r.s; r.y = a[1] / r.s; r.z = a[2] / r.s;
    r.ca = cos(r.angle);
    r.sa = sin(r.angle);
    r.C = 1.0 - r.ca;
    const double xs = r.x * r.sa, ys = r.y * r.sa, zs = r.z * r.sa;
    const double xC = r.x * r.C, yC = r.y * r.C, zC = r.z * r.C;
    const double xyC = r.x * yC, yzC = r.y * zC, zxC = r.z * xC;
    r.R[0][0] = r.x * xC + r.ca; r.R[0][1] = xyC - zs;        r.R[0][2] = zxC + ys;
    r.R[1][0] = xyC + zs;        r.R[1][1] = r.y * yC + r.ca; r.R[1][2] = yzC - xs;
    r.R[2][0] = zxC - ys;        r.R[2][1] = yzC + xs;        r.R[2][2] = r.z * zC + r.ca;
    return r;
}

// M [4][4] fp32 row-major.  invert == 0: Trans(t) R = [R | t];  else R^T Trans(-t) = [R^T | R^T (-t)], the products of
// the last column summed left to right as torch.matmul's row-times-column reads (its fourth term, 0 * 1, adds nothing)
__device__ __forceinline__ void pose_matrix(const double (&a)[3], const double (&t)[3], int invert, float* __restrict__ M) {
    const Rot r = rot_of(a);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) M[4 * i + j] = (float)(invert ? r.R[j][i] : r.R[i][j]);
        M[4 * i + 3] = (float)(invert ? (r.R[0][i] * -t[0] + r.R[1][i] * -t[1]) + r.R[2][i] * -t[2] : t[i]);
    }
    M[12] = 0.f; M[13] = 0.f; M[14] = 0.f; M[15] = 1.f;
}

// ga, gt += the gradient of sum(gM * M) w.r.t. (a, t); gM [4][4] fp32 (row 3 is constant and ignored)
__device__ __forceinline__ void pose_matrix_grad(const double (&a)[3], const double (&t)[3], int invert,
                                                 const float* __restrict__ gM, double (&ga)[3], double (&gt)[3]) {
    const Rot r = rot_of(a);
    double g[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) g[i][j] = invert ? (double)gM[4 * j + i] : (double)gM[4 * i + j];
    if (invert) {
        // M[i][3] = -sum_k R[k][i] t[k]
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            gt[k] -= ((double)gM[3] * r.R[k][0] + (double)gM[7] * r.R[k][1]) + (double)gM[11] * r.R[k][2];
#pragma unroll
            for (int i = 0; i < 3; ++i) g[k][i] -= (double)gM[4 * i + 3] * t[k];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) gt[i] += (double)gM[4 * i + 3];
    }
    const double x = r.x, y = r.y, z = r.z, C = r.C, sa = r.sa, ca = r.ca;
    const double sxy = g[0][1] + g[1][0], szx = g[0][2] + g[2][0], syz = g[1][2] + g[2][1];   // symmetric parts
    const double dx = g[2][1] - g[1][2], dy = g[0][2] - g[2][0], dz = g[1][0] - g[0][1];      // what multiplies sin
    const double gx = ((2.0 * g[0][0] * x + sxy * y) + szx * z) * C + dx * sa;
    const double gy = ((2.0 * g[1][1] * y + sxy * x) + syz * z) * C + dy * sa;
    const double gz = ((2.0 * g[2][2] * z + szx * x) + syz * y) * C + dz * sa;
    const double gC = ((((g[0][0] * x * x + g[1][1] * y * y) + g[2][2] * z * z) + sxy * x * y) + szx * z * x) + syz * y * z;
    const double gsa = (dx * x + dy * y) + dz * z;
    const double gca = ((g[0][0] + g[1][1]) + g[2][2]) - gC;
    // axis = a / s, s = angle + 1e-7;  d angle / d a = a / angle, taken as 0 at angle == 0 (PyTorch's rule for norm)
    double gangle = (gsa * ca - gca * sa) - ((gx * a[0] + gy * a[1]) + gz * a[2]) / (r.s * r.s);
    const double k = r.angle > 0.0 ? gangle / r.angle : 0.0;
    ga[0] += gx / r.s + k * a[0];
    ga[1] += gy / r.s + k * a[1];
    ga[2] += gz / r.s + k * a[2];
}

__global__ __launch_bounds__(64) void pose_matrix_fwd_kernel(const float* __restrict__ aa, const float* __restrict__ tr,
                                                             float* __restrict__ T, int N, int invert) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const double a[3] = {(double)aa[3 * n], (double)aa[3 * n + 1], (double)aa[3 * n + 2]};
    const double t[3] = {(double)tr[3 * n], (double)tr[3 * n + 1], (double)tr[3 * n + 2]};
    pose_matrix(a, t, invert, T + 16L * n);
}

__global__ __launch_bounds__(64) void pose_matrix_bwd_kernel(const float* __restrict__ gT, const float* __restrict__ aa,
                                                             const float* __restrict__ tr, float* __restrict__ gaa,
                                                             float* __restrict__ gtr, int N, int invert) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const double a[3] = {(double)aa[3 * n], (double)aa[3 * n + 1], (double)aa[3 * n + 2]};
    const double t[3] = {(double)tr[3 * n], (double)tr[3 * n + 1], (double)tr[3 * n + 2]};
    double ga[3] = {0.0, 0.0, 0.0}, gt[3] = {0.0, 0.0, 0.0};
    pose_matrix_grad(a, t, invert, gT + 16L * n, ga, gt);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        gaa[3 * n + i] = (float)ga[i];
        gtr[3 * n + i] = (float)gt[i];
    }
}

// ------------------------------------------------------------------ matching poses: all links of a chain, one thread per item
// The second half of predict_poses (trainer.py:708-746): rel[k] = M_k A_{k-1} with A_{-1} = init (or A_0 = M_0), each entry
// ((m_i0 a_0c + m_i1 a_1c) + m_i2 a_2c) + m_i3 a_3c in fp64 from the fp32 values of M_k and of the STORED A_{k-1}, rounded
// once; an absent frame stores sixteen zeros, which the next link multiplies.  rel_inv[k] is the link's own inverse.  The
// stored matrix stays in registers between the links: what is multiplied is what was written.
__global__ __launch_bounds__(64) void pose_chain_kernel(const float* __restrict__ aa, const float* __restrict__ tr,
                                                        const float* __restrict__ present, const float* __restrict__ init,
                                                        float* __restrict__ rel, float* __restrict__ rel_inv, int L, int N,
                                                        int invert) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    float A[16], M[16], Mi[16];
    bool have = init != nullptr;
    if (have) {
#pragma unroll
        for (int e = 0; e < 16; ++e) A[e] = init[16L * n + e];
    }
    for (int k = 0; k < L; ++k) {
        const long i = (long)k * N + n;
        const double a[3] = {(double)aa[3 * i], (double)aa[3 * i + 1], (double)aa[3 * i + 2]};
        const double t[3] = {(double)tr[3 * i], (double)tr[3 * i + 1], (double)tr[3 * i + 2]};
        pose_matrix(a, t, invert, M);
        pose_matrix(a, t, !invert, Mi);
        if (have) {
            float P[16];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    P[4 * r + c] = (float)((((double)M[4 * r] * (double)A[c] + (double)M[4 * r + 1] * (double)A[4 + c]) +
                                            (double)M[4 * r + 2] * (double)A[8 + c]) + (double)M[4 * r + 3] * (double)A[12 + c]);
#pragma unroll
            for (int e = 0; e < 16; ++e) A[e] = P[e];
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) A[e] = M[e];
            have = true;
        }
        if (present && present[i] == 0.f) {
#pragma unroll
            for (int e = 0; e < 16; ++e) A[e] = 0.f;
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            rel[16 * i + e] = A[e];
            rel_inv[16 * i + e] = Mi[e];
        }
    }
}

// ------------------------------------------------------------------ decoder tail, one workgroup per item
using pd_wave::wave_sum;

// mean[c]: thread t owns channels t, t + 256, ...; pixels ascending, then / (h w).  A wavefront reads 64 consecutive
// channels of one pixel: coalesced.  o[k]: wavefront k % 4 takes output k; lane l sums w[k][c] mean[c] over c = l, l + 64,
// ... ascending, the 64 lanes by xor shuffles (32, 16, ... 1); o[k] = 0.01 * (b[k] + that), rounded once.
__global__ __launch_bounds__(PT) void pose_head_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ b, float* __restrict__ aa,
                                                           float* __restrict__ tr, float* __restrict__ T,
                                                           float* __restrict__ Tinv, double* __restrict__ mean, int hw,
                                                           int Cin, int Co, int invert) {
    __shared__ double m[POSE_MAX_CIN];
    __shared__ float o0[6];
    const long n = blockIdx.x;
    const float* xn = x + n * (long)hw * Cin;
    for (int c = threadIdx.x; c < Cin; c += PT) {
        double s = 0.0;
        for (int p = 0; p < hw; ++p) s += (double)xn[(long)p * Cin + c];
        s = s / (double)hw;
        m[c] = s;
        mean[n * Cin + c] = s;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = wave; k < Co; k += PT / 64) {
        double s = 0.0;
        for (int c = lane; c < Cin; c += 64) s += (double)w[(long)k * Cin + c] * m[c];
        s = wave_sum(s);
        if (lane == 0) {
            const float o = (float)(0.01 * ((double)b[k] + s));
            const int f = k / 6, i = k - 6 * f;                      // [N, nf, 1, 6] -> axisangle | translation
            if (i < 3) aa[(n * (Co / 6) + f) * 3 + i] = o;
            else tr[(n * (Co / 6) + f) * 3 + i - 3] = o;
            if (k < 6) o0[k] = o;
        }
    }
    __syncthreads();
    if (threadIdx.x < 2) {                                            // cam_T_cam and cam_T_cam_inv from slot 0
        const double a[3] = {(double)o0[0], (double)o0[1], (double)o0[2]};
        const double t[3] = {(double)o0[3], (double)o0[4], (double)o0[5]};
        pose_matrix(a, t, threadIdx.x ? !invert : invert, (threadIdx.x ? Tinv : T) + 16 * n);
    }
}

// gpre[n][k] = 0.01 * d loss / d o[n][k] (what reaches b[k] + w[k] . mean) into the workspace, and
// gx[n][p][c] = (sum_k w[k][c] gpre[k], k ascending) / (h w), the same value for every pixel
__global__ __launch_bounds__(PT) void pose_head_bwd_item_kernel(const float* __restrict__ gT, const float* __restrict__ gTinv,
                                                                const float* __restrict__ gaa, const float* __restrict__ gtr,
                                                                const float* __restrict__ aa, const float* __restrict__ tr,
                                                                const float* __restrict__ w, float* __restrict__ gx,
                                                                double* __restrict__ gpre, int hw, int Cin, int Co,
                                                                int invert) {
    extern __shared__ double go[];                                    // Co doubles
    const long n = blockIdx.x;
    const int nf = Co / 6;
    for (int k = threadIdx.x; k < Co; k += PT) {
        const int f = k / 6, i = k - 6 * f;
        double g = 0.0;
        if (i < 3) { if (gaa) g = (double)gaa[(n * nf + f) * 3 + i]; }
        else if (gtr) g = (double)gtr[(n * nf + f) * 3 + i - 3];
        go[k] = g;
    }
    __syncthreads();
    if (threadIdx.x == 0 && (gT || gTinv)) {
        const float* a0 = aa + n * nf * 3;
        const float* t0 = tr + n * nf * 3;
        const double a[3] = {(double)a0[0], (double)a0[1], (double)a0[2]};
        const double t[3] = {(double)t0[0], (double)t0[1], (double)t0[2]};
        double ga[3] = {0.0, 0.0, 0.0}, gt[3] = {0.0, 0.0, 0.0};
        if (gT) pose_matrix_grad(a, t, invert, gT + 16 * n, ga, gt);
        if (gTinv) pose_matrix_grad(a, t, !invert, gTinv + 16 * n, ga, gt);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            go[i] += ga[i];
            go[3 + i] += gt[i];
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < Co; k += PT) {
        const double g = 0.01 * go[k];
        go[k] = g;
        gpre[n * Co + k] = g;
    }
    __syncthreads();
    float* gxn = gx + n * (long)hw * Cin;
    for (int c = threadIdx.x; c < Cin; c += PT) {
        double s = 0.0;
        for (int k = 0; k < Co; ++k) s += (double)w[(long)k * Cin + c] * go[k];
        const float v = (float)(s / (double)hw);
        for (int p = 0; p < hw; ++p) gxn[(long)p * Cin + c] = v;
    }
}

// gw[k][c] (+)= sum_n gpre[n][k] mean[n][c], gb[k] (+)= sum_n gpre[n][k]: items ascending, one thread per element
__global__ __launch_bounds__(PT) void pose_head_bwd_weight_kernel(const double* __restrict__ gpre,
                                                                  const double* __restrict__ mean, float* __restrict__ gw,
                                                                  float* __restrict__ gb, int N, int Cin, int Co,
                                                                  int accumulate) {
    const int e = blockIdx.x * PT + threadIdx.x;
    if (e < Co * Cin) {
        const int k = e / Cin, c = e - k * Cin;
        double s = 0.0;
        for (int n = 0; n < N; ++n) s += gpre[(long)n * Co + k] * mean[(long)n * Cin + c];
        gw[e] = accumulate ? (float)((double)gw[e] + s) : (float)s;
    } else if (e < Co * Cin + Co) {
        const int k = e - Co * Cin;
        double s = 0.0;
        for (int n = 0; n < N; ++n) s += gpre[(long)n * Co + k];
        gb[k] = accumulate ? (float)((double)gb[k] + s) : (float)s;
    }
}

}  // namespace

// ============================================================================ C ABI
extern "C" int pd_pose_matrix_fwd(const void* axisangle, const void* translation, void* T, int N, int invert, void* stream) {
    PD_REQUIRE(axisangle && translation && T, "pd_pose_matrix_fwd: axisangle, translation and T must not be null");
    PD_REQUIRE(N >= 0, "pd_pose_matrix_fwd: bad item count N=%d", N);
    PD_REQUIRE(invert == 0 || invert == 1, "pd_pose_matrix_fwd: invert must be 0 or 1, got %d", invert);
    if (N == 0) return PD_OK;
    hipLaunchKernelGGL(pose_matrix_fwd_kernel, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const float*)axisangle,
                       (const float*)translation, (float*)T, N, invert);
    return pd::check_launch("pd_pose_matrix_fwd");
}

extern "C" int pd_pose_matrix_bwd(const void* gT, const void* axisangle, const void* translation, void* gaxisangle,
                                  void* gtranslation, int N, int invert, void* stream) {
    PD_REQUIRE(gT && axisangle && translation && gaxisangle && gtranslation,
               "pd_pose_matrix_bwd: gT, axisangle, translation, gaxisangle and gtranslation must not be null");
    PD_REQUIRE(N >= 0, "pd_pose_matrix_bwd: bad item count N=%d", N);
    PD_REQUIRE(invert == 0 || invert == 1, "pd_pose_matrix_bwd: invert must be 0 or 1, got %d", invert);
    if (N == 0) return PD_OK;
    hipLaunchKernelGGL(pose_matrix_bwd_kernel, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const float*)gT,
                       (const float*)axisangle, (const float*)translation, (float*)gaxisangle, (float*)gtranslation, N, invert);
    return pd::check_launch("pd_pose_matrix_bwd");
}

extern "C" int pd_pose_chain(const void* axisangle, const void* translation, const void* present, const void* init, void* rel,
                             void* rel_inv, int L, int N, int direction, void* stream) {
    PD_REQUIRE(axisangle && translation && rel && rel_inv,
               "pd_pose_chain: axisangle, translation, rel and rel_inv must not be null");
    PD_REQUIRE(L >= 1 && L <= PD_POSE_CHAIN_MAX_LINKS, "pd_pose_chain: 1 .. %d links, got L=%d", PD_POSE_CHAIN_MAX_LINKS, L);
    PD_REQUIRE(N >= 1, "pd_pose_chain: bad item count N=%d", N);
    PD_REQUIRE(direction == -1 || direction == 1, "pd_pose_chain: direction must be -1 or 1, got %d", direction);
    hipLaunchKernelGGL(pose_chain_kernel, dim3((N - 1) / 64 + 1), dim3(64), 0, (hipStream_t)stream, (const float*)axisangle,
                       (const float*)translation, (const float*)present, (const float*)init, (float*)rel, (float*)rel_inv, L, N,
                       direction < 0 ? 1 : 0);
    return pd::check_launch("pd_pose_chain");
}

static int pose_head_args(const char* who, int N, int h, int w, int Cin, int Co, int invert) {
    PD_REQUIRE(N >= 0 && N <= 65535 && h > 0 && w > 0 && (long)h * w <= (1L << 20),
               "%s: bad shape N=%d h=%d w=%d (0 <= N <= 65535, h * w <= 2^20)", who, N, h, w);
    PD_REQUIRE(Cin > 0 && Cin % 64 == 0 && Cin <= POSE_MAX_CIN, "%s: Cin must be a multiple of 64, at most %d, got %d", who,
               POSE_MAX_CIN, Cin);
    PD_REQUIRE(Co > 0 && Co % 6 == 0 && Co <= 6 * 64, "%s: Co must be a multiple of 6, at most 384, got %d", who, Co);
    PD_REQUIRE(invert == 0 || invert == 1, "%s: invert must be 0 or 1, got %d", who, invert);
    return PD_OK;
}

extern "C" int pd_pose_head_fwd(const void* x, const void* w, const void* b, void* axisangle, void* translation, void* T,
                                void* T_inv, void* mean, int N, int h, int wd, int Cin, int Co, int invert, void* stream) {
    if (int rc = pose_head_args("pd_pose_head_fwd", N, h, wd, Cin, Co, invert)) return rc;
    PD_REQUIRE(x && w && b && axisangle && translation && T && T_inv && mean,
               "pd_pose_head_fwd: x, w, b, axisangle, translation, T, T_inv and mean must not be null");
    PD_REQUIRE(pd::aligned8(mean), "pd_pose_head_fwd: mean must be 8-byte aligned");
    if (N == 0) return PD_OK;
    hipLaunchKernelGGL(pose_head_fwd_kernel, dim3(N), dim3(PT), 0, (hipStream_t)stream, (const float*)x, (const float*)w,
                       (const float*)b, (float*)axisangle, (float*)translation, (float*)T, (float*)T_inv, (double*)mean, h * wd,
                       Cin, Co, invert);
    return pd::check_launch("pd_pose_head_fwd");
}

extern "C" int pd_pose_head_bwd(const void* gT, const void* gT_inv, const void* gaxisangle, const void* gtranslation,
                                const void* axisangle, const void* translation, const void* w, const void* mean, void* gx,
                                void* gw, void* gb, void* gpre_ws, int N, int h, int wd, int Cin, int Co, int invert,
                                int accumulate, void* stream) {
    if (int rc = pose_head_args("pd_pose_head_bwd", N, h, wd, Cin, Co, invert)) return rc;
    PD_REQUIRE(axisangle && translation && w && mean && gx && gw && gb && gpre_ws,
               "pd_pose_head_bwd: axisangle, translation, w, mean, gx, gw, gb and gpre_ws must not be null");
    PD_REQUIRE(pd::aligned8(mean) && pd::aligned8(gpre_ws),
               "pd_pose_head_bwd: mean and gpre_ws must be 8-byte aligned");
    PD_REQUIRE(accumulate == 0 || accumulate == 1, "pd_pose_head_bwd: accumulate must be 0 or 1, got %d", accumulate);
    if (N == 0) return PD_OK;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pose_head_bwd_item_kernel, dim3(N), dim3(PT), Co * sizeof(double), st, (const float*)gT,
                       (const float*)gT_inv, (const float*)gaxisangle, (const float*)gtranslation, (const float*)axisangle,
                       (const float*)translation, (const float*)w, (float*)gx, (double*)gpre_ws, h * wd, Cin, Co, invert);
    hipLaunchKernelGGL(pose_head_bwd_weight_kernel, dim3((Co * Cin + Co + PT - 1) / PT), dim3(PT), 0, st,
                       (const double*)gpre_ws, (const double*)mean, (float*)gw, (float*)gb, N, Cin, Co, accumulate);
    return pd::check_launch("pd_pose_head_bwd");
}
