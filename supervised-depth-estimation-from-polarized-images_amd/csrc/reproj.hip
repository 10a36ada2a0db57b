// Photometric multi-view term: view synthesis from depth and a known relative pose, and the minimum / automask
// reduction over the neighbouring frames.
//
// Reference restated:
//   layers.py:383-413     BackprojectDepth   cam = depth * (inv_K[:3,:3] (x, y, 1))
//   layers.py:416-443     Project3D          pix = (K T)[:3,:] (cam, 1);  (u, v) = pix.xy / (pix.z + 1e-7), normalised
//   trainer.py:1041-1044  F.grid_sample(source, pix, padding_mode="border", align_corners=True)
//   trainer.py:1084-1098  compute_loss_masks (argmin over [reprojection, identity])
//   trainer.py:1163-1215  minimum (or mean) over the frames, identity + noise, masked mean
// With align_corners=True the division by W-1 / H-1, the (. - 0.5) * 2 of Project3D and grid_sample's own
// un-normalisation cancel: (u, v) ARE source pixel coordinates, and that is what `coords` holds.
//
// The projection (steps in fp64, their order of operations) and the border rule of a tap are in view_geom.hpp, which
// csrc/matching.hip shares.
//
// Gather / stream kernels.  blockIdx.y is the batch item, so K, inv_K and T are the same for a whole workgroup: the first
// 12 + 9 threads form (K T)[:3,:] and inv_K[:3,:3] in fp64 into LDS once, every pixel reads them back as broadcasts.
// Depth reads and warped / coords / gdepth writes are coalesced (thread = pixel, x fastest); the four taps of a pixel
// are gathers whose locality is that of the warp itself.  No atomics: an output pixel depends on its own depth alone.
// The gradient w.r.t. a PREDICTED pose (view_synth_bwd_pose_kernel) is the one reduction here: every pixel of an item into
// the 12 entries of d loss / d (K T)[:3,:], formed from the same taps in the same pass as the depth gradient and summed in
// fp64 in the fixed order of frame_reduce.hpp (rows per item, then one finalising workgroup per item that applies K^T).
#include "pd_common.h"
#include "frame_reduce.hpp"
#include "view_geom.hpp"

namespace {

using pd_geom::Axis;
using pd_geom::axis_of;
using pd_geom::CamLds;
constexpr int RT = pd_frames::RT;

__global__ __launch_bounds__(RT) void view_synth_fwd_kernel(const float* __restrict__ depth, const float* __restrict__ src,
                                                            const float* __restrict__ K, const float* __restrict__ iK,
                                                            const float* __restrict__ T, float* __restrict__ warped,
                                                            float2* __restrict__ coords, int C, int H, int W) {
    __shared__ CamLds cam;
    const long n = blockIdx.y;
    pd_geom::load_cam(cam, K, iK, T, n);
    const int HW = H * W;
    const float* s = src + n * C * (long)HW;
    for (int i = blockIdx.x * RT + threadIdx.x; i < HW; i += gridDim.x * RT) {
        const int y = i / W, x = i - y * W;
        double u, v, hz, q[3], p[3];
        pd_geom::project(cam, x, y, (double)depth[n * HW + i], u, v, hz, q, p);
        const float uf = (float)u, vf = (float)v;
        coords[n * HW + i] = make_float2(uf, vf);
        const Axis ax = axis_of(uf, W), ay = axis_of(vf, H);
        const pd_geom::Bilinear b(ax.w1, ay.w1);
        const int o00 = ay.i0 * W + ax.i0, o10 = ay.i0 * W + ax.i1, o01 = ay.i1 * W + ax.i0, o11 = ay.i1 * W + ax.i1;
        for (int c = 0; c < C; ++c) {
            const float* pc = s + (long)c * HW;
            warped[(n * C + c) * (long)HW + i] = b.blend(pc[o00], pc[o10], pc[o01], pc[o11]);
        }
    }
}

// The backward warp of item blockIdx.y: gdepth of every pixel and, with POSE, that thread's part of the 12 sums of
// d loss / d P in `acc`.  Both kernels below are this body, so the pose form's gdepth has the bits of the plain form's.
template <bool POSE>
__device__ __forceinline__ void view_synth_bwd_item(const float* __restrict__ gw, const float* __restrict__ src,
                                                    const float2* __restrict__ coords, const float* __restrict__ depth,
                                                    const float* __restrict__ K, const float* __restrict__ iK,
                                                    const float* __restrict__ T, float* __restrict__ gdepth, int C, int H,
                                                    int W, int accumulate, double (&acc)[POSE ? 12 : 1]) {
    __shared__ CamLds cam;
    const long n = blockIdx.y;
    pd_geom::load_cam(cam, K, iK, T, n);
    const int HW = H * W;
    const float* s = src + n * C * (long)HW;
    for (int i = blockIdx.x * RT + threadIdx.x; i < HW; i += gridDim.x * RT) {
        const int y = i / W, x = i - y * W;
        const float2 uv = coords[n * HW + i];
        const Axis ax = axis_of(uv.x, W), ay = axis_of(uv.y, H);
        float g = 0.f;
        if (ax.free_axis || ay.free_axis) {
            const float wx0 = 1.f - ax.w1, wy0 = 1.f - ay.w1;
            const int o00 = ay.i0 * W + ax.i0, o10 = ay.i0 * W + ax.i1, o01 = ay.i1 * W + ax.i0, o11 = ay.i1 * W + ax.i1;
            float gu = 0.f, gv = 0.f;             // sum_c gw_c * d warped_c / d(u, v)
            for (int c = 0; c < C; ++c) {
                const float* pc = s + (long)c * HW;
                const float v00 = pc[o00], v10 = pc[o10], v01 = pc[o01], v11 = pc[o11];
                const float gc = gw[(n * C + c) * (long)HW + i];
                gu += gc * ((v10 - v00) * wy0 + (v11 - v01) * ay.w1);
                gv += gc * ((v01 - v00) * wx0 + (v11 - v10) * ax.w1);
            }
            double u, v, hz, q[3], p[3];
            pd_geom::project(cam, x, y, (double)depth[n * HW + i], u, v, hz, q, p);
            // h = depth * q + b:  d u / d depth = (q.x - u q.z) / (h.z + 1e-7), likewise v
            const double du = ax.free_axis ? (q[0] - u * q[2]) / hz : 0.0;
            const double dv = ay.free_axis ? (q[1] - v * q[2]) / hz : 0.0;
            g = (float)((double)gu * du + (double)gv * dv);
            if constexpr (POSE) {
                // d loss / d h = (a0, a1, a2); h = P (p, 1).  A clamped axis adds nothing (never 0 * inf)
                double a2 = 0.0;
                if (ax.free_axis) {
                    const double a0 = (double)gu / hz;
                    acc[0] += a0 * p[0]; acc[1] += a0 * p[1]; acc[2] += a0 * p[2]; acc[3] += a0;
                    a2 = a0 * u;
                }
                if (ay.free_axis) {
                    const double a1 = (double)gv / hz;
                    acc[4] += a1 * p[0]; acc[5] += a1 * p[1]; acc[6] += a1 * p[2]; acc[7] += a1;
                    a2 = a2 + a1 * v;
                }
                a2 = -a2;
                acc[8] += a2 * p[0]; acc[9] += a2 * p[1]; acc[10] += a2 * p[2]; acc[11] += a2;
            }
        }
        if (!POSE || gdepth) gdepth[n * HW + i] = accumulate ? gdepth[n * HW + i] + g : g;
    }
}

__global__ __launch_bounds__(RT) void view_synth_bwd_kernel(const float* __restrict__ gw, const float* __restrict__ src,
                                                            const float2* __restrict__ coords, const float* __restrict__ depth,
                                                            const float* __restrict__ K, const float* __restrict__ iK,
                                                            const float* __restrict__ T, float* __restrict__ gdepth, int C,
                                                            int H, int W, int accumulate) {
    double none[1];
    view_synth_bwd_item<false>(gw, src, coords, depth, K, iK, T, gdepth, C, H, W, accumulate, none);
}

// one row of 12 doubles per workgroup (frame_reduce.hpp), gridDim.x rows per item; gdepth may be null
__global__ __launch_bounds__(RT) void view_synth_bwd_pose_kernel(const float* __restrict__ gw, const float* __restrict__ src,
                                                                 const float2* __restrict__ coords,
                                                                 const float* __restrict__ depth, const float* __restrict__ K,
                                                                 const float* __restrict__ iK, const float* __restrict__ T,
                                                                 float* __restrict__ gdepth, double* __restrict__ partial,
                                                                 int C, int H, int W, int accumulate) {
    __shared__ double sm[4 * 12];
    double acc[12] = {};
    view_synth_bwd_item<true>(gw, src, coords, depth, K, iK, T, gdepth, C, H, W, accumulate, acc);
    pd_frames::block_rows<12>(acc, sm, partial + blockIdx.y * (long)gridDim.x * 12);
}

// one workgroup per item: the rows of that item in the order of finalize_rows, then gT = K[:3,:]^T gP, rounded once
__global__ __launch_bounds__(256) void view_synth_pose_finalize_kernel(const double* __restrict__ partial, int rows,
                                                                       const float* __restrict__ K, double* __restrict__ gP,
                                                                       float* __restrict__ gT) {
    __shared__ double sm[12 * 256];
    const long n = blockIdx.x;
    double s[12];
    pd_frames::finalize_rows<12>(partial + n * (long)rows * 12, rows, sm, s);
    if (threadIdx.x == 0) {
        if (gP) {
#pragma unroll
            for (int k = 0; k < 12; ++k) gP[n * 12 + k] = s[k];
        }
        const float* k = K + n * 16;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                gT[n * 16 + r * 4 + j] =
                    (float)(((double)k[r] * s[j] + (double)k[4 + r] * s[4 + j]) + (double)k[8 + r] * s[8 + j]);
    }
}

// gup = -gdepth * depth^2 * (1/min_depth - 1/max_depth): depth = 1 / (min_disp + (max_disp - min_disp) * up) backwards
__global__ __launch_bounds__(RT) void depth_to_updisp_bwd_kernel(const float* __restrict__ gdepth, const float* __restrict__ depth,
                                                                 float* __restrict__ gup, long total, float disp_range) {
    for (long i = blockIdx.x * (long)RT + threadIdx.x; i < total; i += (long)gridDim.x * RT) {
        const float d = depth[i];
        gup[i] = gdepth[i] * (-disp_range * d * d);
    }
}

// ------------------------------------------------------------------ minimum / mean over frames, automask, masked sums
// FrameArgs, over_frames and the two-stage fp64 reducer live in frame_reduce.hpp (csrc/student.hip shares them)
using pd_frames::FrameArgs;
using pd_frames::over_frames;

__global__ __launch_bounds__(RT) void combine_fwd_kernel(const FrameArgs a, int F, int has_identity,
                                                         const float* __restrict__ noise, const float* __restrict__ valid,
                                                         unsigned char* __restrict__ sel, double* __restrict__ partial, int N,
                                                         int HW, int avg) {
    __shared__ double sm[4 * 2];
    const long total = (long)N * HW;
    double acc_s = 0.0, acc_c = 0.0;
    for (long i = blockIdx.x * (long)RT + threadIdx.x; i < total; i += (long)gridDim.x * RT) {
        const long n = i / HW;
        const float* vrow = valid ? valid + n * F : nullptr;
        int nv, arg, nvi, argi;
        const float m = over_frames(a.reproj, vrow, F, i, avg, nv, arg);
        bool keep = nv > 0;
        if (keep && has_identity) {
            float idm = over_frames(a.identity, vrow, F, i, avg, nvi, argi);
            if (noise) idm += noise[i];
            keep = m <= idm;                      // argmin index 0: a tie goes to the reprojection
        }
        sel[i] = keep ? (unsigned char)arg : (unsigned char)255;
        if (keep) { acc_s += (double)m; acc_c += 1.0; }
    }
    double acc[2] = {acc_s, acc_c};
    pd_frames::block_rows<2>(acc, sm, partial);
}

// one workgroup sums the rows (the order of loss_finalize_kernel)
__global__ __launch_bounds__(256) void combine_finalize_kernel(const double* __restrict__ partial, int rows,
                                                               double* __restrict__ sums, float* __restrict__ loss) {
    __shared__ double sm[2 * 256];
    double s[2];
    pd_frames::finalize_rows<2>(partial, rows, sm, s);
    if (threadIdx.x == 0) {
        sums[0] = s[0];
        sums[1] = s[1];
        loss[0] = (float)(s[0] / (s[1] + 1e-7));
    }
}

__global__ __launch_bounds__(RT) void combine_bwd_kernel(const FrameArgs a, int F, const float* __restrict__ gloss,
                                                         const unsigned char* __restrict__ sel, const double* __restrict__ sums,
                                                         const float* __restrict__ valid, int N, int HW, int avg) {
    const long total = (long)N * HW;
    const float g = (float)((double)gloss[0] / (sums[1] + 1e-7));
    for (long i = blockIdx.x * (long)RT + threadIdx.x; i < total; i += (long)gridDim.x * RT) {
        const int s = sel[i];
        if (!avg) {
            for (int f = 0; f < F; ++f) a.greproj[f][i] = (s == f) ? g : 0.f;
            continue;
        }
        const float* vrow = valid ? valid + (i / HW) * F : nullptr;
        int nv = 0;
        for (int f = 0; f < F; ++f) nv += !(vrow && vrow[f] == 0.f);
        const float ga = (s != 255 && nv) ? g / (float)nv : 0.f;
        for (int f = 0; f < F; ++f) a.greproj[f][i] = (vrow && vrow[f] == 0.f) ? 0.f : ga;
    }
}

}  // namespace

// ============================================================================ C ABI
static int view_synth_args(const char* who, const void* depth, const void* src, const void* K, const void* inv_K, const void* T,
                           int N, int C, int H, int W) {
    PD_REQUIRE(depth && src && K && inv_K && T, "%s: depth, src, K, inv_K and T must not be null", who);
    PD_REQUIRE(N >= 0 && N <= 65535 && C > 0 && H > 0 && W > 0, "%s: bad shape N=%d C=%d H=%d W=%d (0 <= N <= 65535)", who, N, C, H, W);
    PD_REQUIRE((long)H * W <= (1L << 30), "%s: image too large (%d x %d): offsets inside a plane are 32-bit", who, H, W);
    return PD_OK;
}

extern "C" int pd_view_synth_fwd(const void* depth, const void* src, const void* K, const void* inv_K, const void* T,
                                 void* warped, void* coords, int N, int C, int H, int W, void* stream) {
    if (int rc = view_synth_args("pd_view_synth_fwd", depth, src, K, inv_K, T, N, C, H, W)) return rc;
    PD_REQUIRE(warped && coords, "pd_view_synth_fwd: warped and coords must not be null");
    PD_REQUIRE(pd::aligned8(coords), "pd_view_synth_fwd: coords must be 8-byte aligned");
    if (N == 0) return PD_OK;
    hipLaunchKernelGGL(view_synth_fwd_kernel, dim3(pd::item_grid(N, (long)H * W), N), dim3(RT), 0, (hipStream_t)stream,
                       (const float*)depth, (const float*)src, (const float*)K, (const float*)inv_K, (const float*)T,
                       (float*)warped, (float2*)coords, C, H, W);
    return pd::check_launch("pd_view_synth_fwd");
}

extern "C" int pd_view_synth_bwd(const void* gwarped, const void* src, const void* coords, const void* depth, const void* K,
                                 const void* inv_K, const void* T, void* gdepth, int N, int C, int H, int W, int accumulate,
                                 void* stream) {
    if (int rc = view_synth_args("pd_view_synth_bwd", depth, src, K, inv_K, T, N, C, H, W)) return rc;
    PD_REQUIRE(gwarped && coords && gdepth, "pd_view_synth_bwd: gwarped, coords and gdepth must not be null");
    PD_REQUIRE(pd::aligned8(coords), "pd_view_synth_bwd: coords must be 8-byte aligned");
    if (N == 0) return PD_OK;
    hipLaunchKernelGGL(view_synth_bwd_kernel, dim3(pd::item_grid(N, (long)H * W), N), dim3(RT), 0, (hipStream_t)stream,
                       (const float*)gwarped, (const float*)src, (const float2*)coords, (const float*)depth, (const float*)K,
                       (const float*)inv_K, (const float*)T, (float*)gdepth, C, H, W, accumulate);
    return pd::check_launch("pd_view_synth_bwd");
}

// rows of partial_ws per item: one per workgroup, at most 512 (a thread then strides over its pixels)
extern "C" int pd_view_synth_pose_rows(int H, int W) {
    if (H <= 0 || W <= 0) return 1;
    const long b = ((long)H * W + RT - 1) / RT;
    return (int)(b > 512 ? 512 : b);
}

extern "C" int pd_view_synth_bwd_pose(const void* gwarped, const void* src, const void* coords, const void* depth,
                                      const void* K, const void* inv_K, const void* T, void* gdepth, void* partial_ws,
                                      void* gP, void* gT, int N, int C, int H, int W, int accumulate, void* stream) {
    if (int rc = view_synth_args("pd_view_synth_bwd_pose", depth, src, K, inv_K, T, N, C, H, W)) return rc;
    PD_REQUIRE(gwarped && coords && partial_ws && gT,
               "pd_view_synth_bwd_pose: gwarped, coords, partial_ws and gT must not be null");
    PD_REQUIRE(pd::aligned8(coords) && pd::aligned8(partial_ws) && pd::aligned8(gP),
               "pd_view_synth_bwd_pose: coords, partial_ws and gP must be 8-byte aligned");
    if (N == 0) return PD_OK;
    const int rows = pd_view_synth_pose_rows(H, W);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(view_synth_bwd_pose_kernel, dim3(rows, N), dim3(RT), 0, st, (const float*)gwarped, (const float*)src,
                       (const float2*)coords, (const float*)depth, (const float*)K, (const float*)inv_K, (const float*)T,
                       (float*)gdepth, (double*)partial_ws, C, H, W, accumulate);
    hipLaunchKernelGGL(view_synth_pose_finalize_kernel, dim3(N), dim3(256), 0, st, (const double*)partial_ws, rows,
                       (const float*)K, (double*)gP, (float*)gT);
    return pd::check_launch("pd_view_synth_bwd_pose");
}

extern "C" int pd_depth_to_updisp_bwd(const void* gdepth, const void* depth, void* gup, long n, float min_depth, float max_depth,
                                      void* stream) {
    PD_REQUIRE(gdepth && depth && gup, "pd_depth_to_updisp_bwd: gdepth, depth and gup must not be null");
    PD_REQUIRE(n >= 0, "pd_depth_to_updisp_bwd: bad element count %ld", n);
    PD_REQUIRE(min_depth > 0 && max_depth > min_depth, "pd_depth_to_updisp_bwd: bad depth range");
    if (n == 0) return PD_OK;
    hipLaunchKernelGGL(depth_to_updisp_bwd_kernel, dim3(pd::flat_grid(n)), dim3(RT), 0, (hipStream_t)stream,
                       (const float*)gdepth, (const float*)depth, (float*)gup, n, 1.f / min_depth - 1.f / max_depth);
    return pd::check_launch("pd_depth_to_updisp_bwd");
}

extern "C" int pd_reproj_combine_rows(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 1;
    return (int)pd::flat_grid((long)N * H * W);
}

extern "C" int pd_reproj_combine_fwd(const void* const* reproj, const void* const* identity, int F, const void* noise,
                                     const void* valid, void* sel, void* partial_ws, void* sums, void* loss, int N, int H,
                                     int W, int avg, void* stream) {
    if (int rc = pd_frames::combine_args("pd_reproj_combine_fwd", F, N, H, W, avg)) return rc;
    PD_REQUIRE(reproj && sel && partial_ws && sums && loss,
               "pd_reproj_combine_fwd: reproj, sel, partial_ws, sums and loss must not be null");
    PD_REQUIRE(identity || !noise, "pd_reproj_combine_fwd: noise is added to the identity maps, which are null");
    PD_REQUIRE(pd::aligned8(partial_ws) && pd::aligned8(sums), "pd_reproj_combine_fwd: partial_ws and sums must be 8-byte aligned");
    FrameArgs a = {};
    for (int f = 0; f < F; ++f) {
        PD_REQUIRE(reproj[f] && (!identity || identity[f]), "pd_reproj_combine_fwd: map %d is null", f);
        a.reproj[f] = (const float*)reproj[f];
        a.identity[f] = identity ? (const float*)identity[f] : nullptr;
    }
    const int rows = pd_reproj_combine_rows(N, H, W);
    hipStream_t st = (hipStream_t)stream;
    // N == 0: one workgroup writes a zero partial row, the loss is 0 / 1e-7 = 0
    hipLaunchKernelGGL(combine_fwd_kernel, dim3(rows), dim3(RT), 0, st, a, F, identity ? 1 : 0, (const float*)noise,
                       (const float*)valid, (unsigned char*)sel, (double*)partial_ws, N, H * W, avg);
    hipLaunchKernelGGL(combine_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)partial_ws, rows, (double*)sums,
                       (float*)loss);
    return pd::check_launch("pd_reproj_combine_fwd");
}

extern "C" int pd_reproj_combine_bwd(const void* gloss, const void* sel, const void* sums, const void* valid,
                                     void* const* greproj, int F, int N, int H, int W, int avg, void* stream) {
    if (int rc = pd_frames::combine_args("pd_reproj_combine_bwd", F, N, H, W, avg)) return rc;
    PD_REQUIRE(gloss && sel && sums && greproj, "pd_reproj_combine_bwd: gloss, sel, sums and greproj must not be null");
    PD_REQUIRE(pd::aligned8(sums), "pd_reproj_combine_bwd: sums must be 8-byte aligned");
    FrameArgs a = {};
    for (int f = 0; f < F; ++f) {
        PD_REQUIRE(greproj[f], "pd_reproj_combine_bwd: map %d is null", f);
        a.greproj[f] = (float*)greproj[f];
    }
    if (N == 0) return PD_OK;
    hipLaunchKernelGGL(combine_bwd_kernel, dim3(pd::flat_grid((long)N * H * W)), dim3(RT), 0, (hipStream_t)stream, a,
                       F, (const float*)gloss, (const unsigned char*)sel, (const double*)sums, (const float*)valid, N, H * W, avg);
    return pd::check_launch("pd_reproj_combine_bwd");
}
