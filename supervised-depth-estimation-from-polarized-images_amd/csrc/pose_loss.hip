// Pose supervision: the predicted cam_T_cam against the ground-truth relative pose, rotations compared as rotation vectors
// (forward, gradient, and the per-pair records of the pose evaluator).
//
// Reference restated:
//   trainer.py:1267-1285    --supervise_pose: 0.1 * mean((rv(R_pred) - rv(R_gt))^2) + mean((t_pred - t_gt)^2) per frame
//   roma.rotmat_to_rotvec   = rotmat_to_unitquat, then unitquat_to_rotvec (adapted from SciPy's Rotation.from_matrix /
//                             as_rotvec): argmax over (M00, M11, M22, trace), four branches, a normalisation, a sign flip,
//                             atan2, and a small-angle polynomial
// Written with tensor ops that is several dozen launches of N x 3 elements per frame, twice, and autograd's mirror of them.
// Here all frames are ONE workgroup forward (an item is one thread's loop iteration) and one launch backward (an item of a
// frame is one thread).  Everything is fp64 inside from the fp32 inputs and rounded once; every sum has a stated order
// (include/polardepth.h); no atomics, no host synchronisation, capturable.
#include "pd_common.h"
#include "wave_ops.hpp"

namespace {

constexpr int LT = 256;                              // threads per workgroup (four wavefronts)
constexpr int MAX_FRAMES = PD_REPROJ_MAX_FRAMES;

struct PoseLossArgs {
    const float* pred[MAX_FRAMES];
    const float* gt[MAX_FRAMES];
    float* gpred[MAX_FRAMES];
    float weight[MAX_FRAMES];
};

// ------------------------------------------------------------------ rv(M), fp64
// what the gradient needs again is kept: the branch, the unnormalised quaternion and its norm, the sign, s, angle, scale
struct RotVec {
    double rv[3];
    double qu[4], q[4];          // before the normalisation; normalised and sign-flipped
    double nq, sign, s, angle, scale;
    int c;
};

__device__ __forceinline__ void load_rot(const float* __restrict__ T, double (&M)[3][3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[i][j] = (double)T[4 * i + j];
}

__device__ __forceinline__ RotVec rotvec_of(const double (&M)[3][3]) {
    RotVec r;
    const double tr = (M[0][0] + M[1][1]) + M[2][2];
    const double d[4] = {M[0][0], M[1][1], M[2][2], tr};
    int c = 0;
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (d[i] > d[c]) c = i;                      // the first maximum
    r.c = c;
    if (c < 3) {
        const int i = c, j = (i + 1) % 3, k = (j + 1) % 3;
        r.qu[i] = 1.0 - tr + 2.0 * M[i][i];
        r.qu[j] = M[j][i] + M[i][j];
        r.qu[k] = M[k][i] + M[i][k];
        r.qu[3] = M[k][j] - M[j][k];
    } else {
        r.qu[0] = M[2][1] - M[1][2];
        r.qu[1] = M[0][2] - M[2][0];
        r.qu[2] = M[1][0] - M[0][1];
        r.qu[3] = 1.0 + tr;
    }
    r.nq = sqrt(((r.qu[0] * r.qu[0] + r.qu[1] * r.qu[1]) + r.qu[2] * r.qu[2]) + r.qu[3] * r.qu[3]);
#pragma unroll
    for (int i = 0; i < 4; ++i) r.q[i] = r.qu[i] / r.nq;
    r.sign = r.q[3] < 0.0 ? -1.0 : 1.0;
    if (r.q[3] < 0.0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) r.q[i] = -r.q[i];
    }
    r.s = sqrt((r.q[0] * r.q[0] + r.q[1] * r.q[1]) + r.q[2] * r.q[2]);
    r.angle = 2.0 * atan2(r.s, r.q[3]);
    if (r.angle <= 1e-3) {
        const double a2 = r.angle * r.angle;
        r.scale = (2.0 + a2 / 12.0) + 7.0 * (a2 * a2) / 2880.0;
    } else {
        r.scale = r.angle / sin(r.angle / 2.0);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) r.rv[i] = r.scale * r.q[i];
    return r;
}

// gM = J^T g, J = d rv / d M of the expressions above: the branch is fixed, the sign flip a constant factor, the polynomial
// differentiated in its own branch, d sqrt(.) / d(.) := 0 at 0 (PyTorch's rule for norm)
__device__ __forceinline__ void rotvec_grad(const RotVec& r, const double (&g)[3], double (&gM)[3][3]) {
    double gq[4];
    const double gscale = (g[0] * r.q[0] + g[1] * r.q[1]) + g[2] * r.q[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) gq[i] = r.scale * g[i];
    double dscale;
    if (r.angle <= 1e-3) {
        dscale = r.angle / 6.0 + 7.0 * ((r.angle * r.angle) * r.angle) / 720.0;
    } else {
        const double sh = sin(r.angle / 2.0), ch = cos(r.angle / 2.0);
        dscale = 1.0 / sh - (r.angle * ch * 0.5) / (sh * sh);
    }
    const double gangle = gscale * dscale;
    const double den = r.s * r.s + r.q[3] * r.q[3];           // angle = 2 atan2(s, q3)
    const double gs = gangle * (2.0 * r.q[3] / den);
    gq[3] = gangle * (-2.0 * r.s / den);
    if (r.s > 0.0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) gq[i] += gs * (r.q[i] / r.s);
    }
    // q = sign * qu / nq, nq = |qu|
    double gp[4], gqu[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) gp[i] = r.sign * gq[i];
    const double dot = ((gp[0] * r.qu[0] + gp[1] * r.qu[1]) + gp[2] * r.qu[2]) + gp[3] * r.qu[3];
    const double gnq = -dot / (r.nq * r.nq);
#pragma unroll
    for (int i = 0; i < 4; ++i) gqu[i] = gp[i] / r.nq + (r.nq > 0.0 ? gnq * (r.qu[i] / r.nq) : 0.0);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) gM[i][j] = 0.0;
    double gtr;
    if (r.c < 3) {
        const int i = r.c, j = (i + 1) % 3, k = (j + 1) % 3;
        gtr = -gqu[i];
        gM[i][i] += 2.0 * gqu[i];
        gM[j][i] += gqu[j]; gM[i][j] += gqu[j];
        gM[k][i] += gqu[k]; gM[i][k] += gqu[k];
        gM[k][j] += gqu[3]; gM[j][k] -= gqu[3];
    } else {
        gtr = gqu[3];
        gM[2][1] += gqu[0]; gM[1][2] -= gqu[0];
        gM[0][2] += gqu[1]; gM[2][0] -= gqu[1];
        gM[1][0] += gqu[2]; gM[0][1] -= gqu[2];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) gM[i][i] += gtr;
}

// e_r, e_t of one item; rec != nullptr: its ten record values as well
__device__ __forceinline__ void item_errors(const float* __restrict__ Tp, const float* __restrict__ Tg, double& er, double& et,
                                            double* __restrict__ rec) {
    double Mp[3][3], Mg[3][3];
    load_rot(Tp, Mp);
    load_rot(Tg, Mg);
    const RotVec a = rotvec_of(Mp), b = rotvec_of(Mg);
    er = 0.0;
    et = 0.0;
    double tp[3], tg[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double d = a.rv[k] - b.rv[k];
        er += d * d;
        tp[k] = (double)Tp[4 * k + 3];
        tg[k] = (double)Tg[4 * k + 3];
        const double e = tp[k] - tg[k];
        et += e * e;
    }
    if (rec) {
        double D[3][3];                              // R_pred^T R_gt
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) D[i][j] = (Mp[0][i] * Mg[0][j] + Mp[1][i] * Mg[1][j]) + Mp[2][i] * Mg[2][j];
        const RotVec g = rotvec_of(D);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            rec[k] = a.rv[k];
            rec[3 + k] = b.rv[k];
        }
        rec[6] = sqrt((g.rv[0] * g.rv[0] + g.rv[1] * g.rv[1]) + g.rv[2] * g.rv[2]);
        rec[7] = sqrt(et);
        rec[8] = sqrt((tp[0] * tp[0] + tp[1] * tp[1]) + tp[2] * tp[2]);
        rec[9] = sqrt((tg[0] * tg[0] + tg[1] * tg[1]) + tg[2] * tg[2]);
    }
}

// ONE workgroup.  Per frame: thread t sums its items t, t + 256, ... ascending, the 64 lanes by the xor butterfly, the four
// wavefronts ((w0 + w1) + w2) + w3; thread 0 then forms r_f, t_f and, after the last frame, the three sums over the frames.
__global__ __launch_bounds__(LT) void pose_loss_fwd_kernel(PoseLossArgs a, int F, const float* __restrict__ valid,
                                                           double* __restrict__ records, float* __restrict__ vals, int N) {
    __shared__ double sm[LT / 64][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double sum_r = 0.0, sum_t = 0.0, sum_w = 0.0;    // thread 0 only
    for (int f = 0; f < F; ++f) {
        double er = 0.0, et = 0.0, cnt = 0.0;
        for (int n = threadIdx.x; n < N; n += LT) {
            const bool ok = !valid || valid[(long)n * F + f] != 0.f;
            if (!ok && !records) continue;
            double e_r, e_t;
            item_errors(a.pred[f] + 16L * n, a.gt[f] + 16L * n, e_r, e_t, records ? records + ((long)f * N + n) * 10 : nullptr);
            if (ok) {
                er += e_r;
                et += e_t;
                cnt += 1.0;
            }
        }
        er = pd_wave::wave_sum(er);
        et = pd_wave::wave_sum(et);
        cnt = pd_wave::wave_sum(cnt);
        __syncthreads();                             // the previous frame's sums have been read
        if (lane == 0) {
            sm[wave][0] = er;
            sm[wave][1] = et;
            sm[wave][2] = cnt;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const double c = ((sm[0][2] + sm[1][2]) + sm[2][2]) + sm[3][2];
            double rf = 0.0, tf = 0.0;
            if (c > 0.0) {
                rf = 0.1 * ((((sm[0][0] + sm[1][0]) + sm[2][0]) + sm[3][0]) / (3.0 * c));
                tf = (((sm[0][1] + sm[1][1]) + sm[2][1]) + sm[3][1]) / (3.0 * c);
            }
            sum_r += rf;
            sum_t += tf;
            sum_w += (double)a.weight[f] * (rf + tf);
            vals[3 + 2 * f] = (float)rf;
            vals[4 + 2 * f] = (float)tf;
        }
    }
    if (threadIdx.x == 0) {
        vals[0] = (float)sum_r;
        vals[1] = (float)sum_t;
        vals[2] = (float)sum_w;
    }
}

// blockIdx.y = frame, one thread per item.  Every workgroup counts its frame's valid items itself (an integer: any order).
__global__ __launch_bounds__(LT) void pose_loss_bwd_kernel(PoseLossArgs a, int F, const float* __restrict__ gvals,
                                                           const float* __restrict__ valid, int N) {
    __shared__ int scnt[LT / 64];
    const int f = blockIdx.y;
    int cnt = N;
    if (valid) {
        int c = 0;
        for (int n = threadIdx.x; n < N; n += LT) c += valid[(long)n * F + f] != 0.f ? 1 : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        if ((threadIdx.x & 63) == 0) scnt[threadIdx.x >> 6] = c;
        __syncthreads();
        cnt = ((scnt[0] + scnt[1]) + scnt[2]) + scnt[3];
    }
    const int n = blockIdx.x * LT + threadIdx.x;
    if (n >= N) return;
    float* __restrict__ g = a.gpred[f] + 16L * n;
    if (valid && valid[(long)n * F + f] == 0.f) {
#pragma unroll
        for (int i = 0; i < 16; ++i) g[i] = 0.f;
        return;
    }
    const float* __restrict__ Tp = a.pred[f] + 16L * n;
    const float* __restrict__ Tg = a.gt[f] + 16L * n;
    const double w = (double)a.weight[f];
    const double a_r = (double)gvals[0] + w * (double)gvals[2];
    const double a_t = (double)gvals[1] + w * (double)gvals[2];
    const double c3 = 3.0 * (double)cnt;
    const double kr = a_r * 0.1 * 2.0 / c3, kt = a_t * 2.0 / c3;
    double Mp[3][3], Mg[3][3], d[3], gM[3][3];
    load_rot(Tp, Mp);
    load_rot(Tg, Mg);
    const RotVec p = rotvec_of(Mp), q = rotvec_of(Mg);
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = p.rv[k] - q.rv[k];
    rotvec_grad(p, d, gM);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) g[4 * i + j] = (float)(kr * gM[i][j]);
        g[4 * i + 3] = (float)(kt * ((double)Tp[4 * i + 3] - (double)Tg[4 * i + 3]));
    }
    g[12] = 0.f; g[13] = 0.f; g[14] = 0.f; g[15] = 0.f;
}

int pose_loss_args(const char* who, const void* const* T_pred, const void* const* T_gt, int F, const float* frame_weight, int N,
                   PoseLossArgs& a) {
    PD_REQUIRE(F >= 1 && F <= MAX_FRAMES, "%s: 1 <= F <= %d frames, got %d", who, MAX_FRAMES, F);
    PD_REQUIRE(N >= 0 && N <= 65535, "%s: bad item count N=%d (0 <= N <= 65535)", who, N);
    PD_REQUIRE(T_pred && T_gt && frame_weight, "%s: T_pred, T_gt and frame_weight must not be null", who);
    for (int f = 0; f < F; ++f) {
        PD_REQUIRE(N == 0 || (T_pred[f] && T_gt[f]), "%s: the matrices of frame %d are null", who, f);
        a.pred[f] = (const float*)T_pred[f];
        a.gt[f] = (const float*)T_gt[f];
        a.weight[f] = frame_weight[f];
    }
    return PD_OK;
}

}  // namespace

// ============================================================================ C ABI
extern "C" int pd_pose_loss_fwd(const void* const* T_pred, const void* const* T_gt, int F, const float* frame_weight,
                                const void* valid, void* records, void* vals, int N, void* stream) {
    PoseLossArgs a = {};
    if (int rc = pose_loss_args("pd_pose_loss_fwd", T_pred, T_gt, F, frame_weight, N, a)) return rc;
    PD_REQUIRE(vals, "pd_pose_loss_fwd: vals must not be null");
    PD_REQUIRE(pd::aligned8(records), "pd_pose_loss_fwd: records must be 8-byte aligned");
    // N == 0: no item is read and no record written; the kernel writes the zeros
    hipLaunchKernelGGL(pose_loss_fwd_kernel, dim3(1), dim3(LT), 0, (hipStream_t)stream, a, F, (const float*)valid,
                       (double*)records, (float*)vals, N);
    return pd::check_launch("pd_pose_loss_fwd");
}

extern "C" int pd_pose_loss_bwd(const void* gvals, const void* const* T_pred, const void* const* T_gt, int F,
                                const float* frame_weight, const void* valid, void* const* gT, int N, void* stream) {
    PoseLossArgs a = {};
    if (int rc = pose_loss_args("pd_pose_loss_bwd", T_pred, T_gt, F, frame_weight, N, a)) return rc;
    PD_REQUIRE(gvals && gT, "pd_pose_loss_bwd: gvals and gT must not be null");
    for (int f = 0; f < F; ++f) {
        PD_REQUIRE(N == 0 || gT[f], "pd_pose_loss_bwd: the gradient of frame %d is null", f);
        a.gpred[f] = (float*)gT[f];
    }
    if (N == 0) return PD_OK;
    hipLaunchKernelGGL(pose_loss_bwd_kernel, dim3((N + LT - 1) / LT, F), dim3(LT), 0, (hipStream_t)stream, a, F,
                       (const float*)gvals, (const float*)valid, N);
    return pd::check_launch("pd_pose_loss_bwd");
}
