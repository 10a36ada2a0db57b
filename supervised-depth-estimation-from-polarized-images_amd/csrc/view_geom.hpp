// The camera geometry of the multi-view kernels (csrc/reproj.hip, csrc/matching.hip, csrc/consistency.hip): a pixel of the
// current view at a depth to its coordinates (u, v) in a source view, and the bilinear taps there.  Each expression is
// written here once, its order of operations in the comment above it; the files are built with -ffp-contract=off, so no
// product is fused into a sum and two kernels that call the same piece produce the same bits.  (u, v) are source PIXEL
// coordinates (align_corners=True).  What becomes of a tap outside the image is the caller's rule: clamped (axis_of:
// grid_sample's "border"), the sample dropped (matching.hip: "zeros" plus the edge mask) or the pair not compared
// (consistency.hip).
// Camera operands are references to arrays: called on __shared__ arrays they stay LDS reads after inlining.
#pragma once
#include <hip/hip_runtime.h>

namespace pd_geom {

// entry t = 4 i + j of P from one item's K and T ([4][4] fp32 row-major): sum_k K[i][k] T[k][j], k ascending, the products
// summed left to right
__device__ __forceinline__ double cam_P(const float* K, const float* T, int t) {
    const float* k = K + (t >> 2) * 4;
    const float* c = T + (t & 3);
    return (((double)k[0] * (double)c[0] + (double)k[1] * (double)c[4]) + (double)k[2] * (double)c[8]) +
           (double)k[3] * (double)c[12];
}
// entry q = 3 i + j of inv_K[:3,:3] of item n (inv_K: [N][4][4])
__device__ __forceinline__ double cam_iK(const float* iK, long n, int q) { return (double)iK[n * 16 + (q / 3) * 4 + q % 3]; }

// r[i] = (iK[i][0] x + iK[i][1] y) + iK[i][2]
__device__ __forceinline__ void ray(const double (&iK)[9], int x, int y, double (&r)[3]) {
    const double xd = (double)x, yd = (double)y;
#pragma unroll
    for (int i = 0; i < 3; ++i) r[i] = (iK[3 * i] * xd + iK[3 * i + 1] * yd) + iK[3 * i + 2];
}
// the same at a FRACTIONAL pixel (csrc/consistency.hip: the return leg starts where the forward leg landed)
__device__ __forceinline__ void ray(const double (&iK)[9], double xd, double yd, double (&r)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) r[i] = (iK[3 * i] * xd + iK[3 * i + 1] * yd) + iK[3 * i + 2];
}

// p = d r;  h[i] = ((P[i][0] p.x + P[i][1] p.y) + P[i][2] p.z) + P[i][3];  hz = h.z + 1e-7;  u = h.x / hz, v = h.y / hz
// q[i] = (P[i][0] r.x + P[i][1] r.y) + P[i][2] r.z, so that h = d q + P[:, 3]: with the camera point p what the depth and
// pose gradients need (a caller that uses neither pays nothing for them)
__device__ __forceinline__ void project_ray(const double (&P)[12], const double (&r)[3], double d, double& u, double& v,
                                            double& hz, double (&q)[3], double (&p)[3]) {
    double h[3];
    const double p0 = d * r[0], p1 = d * r[1], p2 = d * r[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        h[i] = ((P[4 * i] * p0 + P[4 * i + 1] * p1) + P[4 * i + 2] * p2) + P[4 * i + 3];
        q[i] = (P[4 * i] * r[0] + P[4 * i + 1] * r[1]) + P[4 * i + 2] * r[2];
    }
    hz = h[2] + 1e-7;
    u = h[0] / hz;
    v = h[1] / hz;
    p[0] = p0; p[1] = p1; p[2] = p2;
}
// the weights of the taps (x0, y0), (x1, y0), (x0, y1), (x1, y1) from the weights of the upper taps, and
// blend = ((a w00 + b w10) + c w01) + d w11
struct Bilinear {
    float w00, w10, w01, w11;
    __device__ __forceinline__ Bilinear(float wx1, float wy1) {
        const float wx0 = 1.f - wx1, wy0 = 1.f - wy1;
        w00 = wx0 * wy0; w10 = wx1 * wy0; w01 = wx0 * wy1; w11 = wx1 * wy1;
    }
    __device__ __forceinline__ float blend(float a, float b, float c, float d) const {
        return ((a * w00 + b * w10) + c * w01) + d * w11;
    }
};

// ------------------------------------------------------------------ one camera per workgroup, in LDS
struct CamLds {
    double P[12];   // (K T)[:3,:], row-major 3x4
    double iK[9];   // inv_K[:3,:3]
};

// the first 12 + 9 threads fill `cam` for item n (K, inv_K, T: [N][4][4]); every thread of the workgroup must call it
__device__ __forceinline__ void load_cam(CamLds& cam, const float* __restrict__ K, const float* __restrict__ iK,
                                         const float* __restrict__ T, long n) {
    const int t = threadIdx.x;
    if (t < 12) cam.P[t] = cam_P(K + n * 16, T + n * 16, t);
    else if (t < 21) cam.iK[t - 12] = cam_iK(iK, n, t - 12);
    __syncthreads();
}

// ray and project_ray for pixel (x, y) at depth d
__device__ __forceinline__ void project(const CamLds& cam, int x, int y, double d, double& u, double& v, double& hz,
                                        double (&q)[3], double (&p)[3]) {
    double r[3];
    ray(cam.iK, x, y, r);
    project_ray(cam.P, r, d, u, v, hz, q, p);
}

// border padding of one axis: the clamped coordinate, its cell and the weight of the upper tap; `free_axis` is false where
// the coordinate was clamped (PyTorch's rule: c <= 0 or c >= size-1) or is not finite -- the gradient is then exactly zero
struct Axis {
    int i0, i1;
    float w1;
    bool free_axis;
};
__device__ __forceinline__ Axis axis_of(float c, int size) {
    Axis a;
    const float hi = (float)(size - 1);
    a.free_axis = (c > 0.f) && (c < hi);          // false for NaN and both infinities as well
    float cc = c;
    if (!(fabsf(c) <= 3.0e38f)) cc = 0.f;         // non-finite -> 0
    cc = fminf(fmaxf(cc, 0.f), hi);
    const float f = floorf(cc);
    a.i0 = (int)f;
    a.i1 = a.i0 + (a.i0 < size - 1);              // cc == size-1: the upper tap has weight 0, keep it in bounds
    a.w1 = cc - f;
    return a;
}

}  // namespace pd_geom
