// Shared by csrc/loss.hip (the supervised normals term, pd_gt_normals) and csrc/polar_loss.hip (the polarimetric term): the
// depth -> normal chain of kornia.geometry.depth.depth_to_normals (unproject with K, Sobel/8 with replicate padding, cross
// product, L2 normalise) in fp32, and its transpose: dL/d(normal) -> (dL/dA, dL/dB) per pixel, then the 3 x 3 gather of those
// back to the depth.  Both translation units are built without contraction, so a depth map gives the same bits in both.
#pragma once
#include <hip/hip_runtime.h>

namespace pd_dn {

struct Cam { float fx, fy, cx, cy; };
__device__ __forceinline__ Cam load_cam(const float* K, long n) {
    const float* k = K + n * 16;  // [4][4]
    return Cam{k[0], k[5], k[2], k[6]};
}

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// Sobel/8 gradients of the unprojected points around (x,y) with replicate padding
__device__ __forceinline__ void sobel_xyz(const float* __restrict__ D, int H, int W, int x, int y, Cam c, V3& A, V3& B) {
    A = V3{0, 0, 0}; B = V3{0, 0, 0};
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = min(max(y + dy, 0), H - 1);
        const float sy = dy == 0 ? 2.f : 1.f, ddy = (float)dy;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = min(max(x + dx, 0), W - 1);
            const float sx = dx == 0 ? 2.f : 1.f, ddx = (float)dx;
            const float d = D[(long)yy * W + xx];
            const float X = (xx - c.cx) / c.fx * d, Y = (yy - c.cy) / c.fy * d;
            const float kx = sy * ddx * 0.125f, ky = ddy * sx * 0.125f;
            A.x += kx * X; A.y += kx * Y; A.z += kx * d;
            B.x += ky * X; B.y += ky * Y; B.z += ky * d;
        }
    }
}

__device__ __forceinline__ V3 normalize12(V3 v, float& nv) {
    nv = sqrtf(dot(v, v));
    const float inv = 1.f / fmaxf(nv, 1e-12f);
    return V3{v.x * inv, v.y * inv, v.z * inv};
}

// wn = dL/d nn with nn = normalize12(A x B), nv = |A x B|  ->  (dL/dA, dL/dB)
__device__ __forceinline__ void normal_grad_to_ab(V3 wn, V3 nn, float nv, V3 A, V3 B, V3& dA, V3& dB) {
    V3 wv;   // dL/d v, v -> nn = v / max(|v|, 1e-12)
    if (nv > 1e-12f) {
        const float inv = 1.f / nv, pr = dot(wn, nn);
        wv = V3{(wn.x - pr * nn.x) * inv, (wn.y - pr * nn.y) * inv, (wn.z - pr * nn.z) * inv};
    } else {
        wv = V3{wn.x * 1e12f, wn.y * 1e12f, wn.z * 1e12f};
    }
    dA = cross(B, wv);   // d(A x B).w / dA = B x w
    dB = cross(wv, A);   // d(A x B).w / dB = w x A
}

// separable replicate-padding weights: sum of taps delta in {-1,0,1} of p that land on q
__device__ __forceinline__ void tap_weights(int q, int p, int n, float& wd, float& ws) {
    wd = 0.f; ws = 0.f;
#pragma unroll
    for (int d = -1; d <= 1; ++d) {
        const int t = min(max(p + d, 0), n - 1);
        if (t == q) { wd += (float)d; ws += d == 0 ? 2.f : 1.f; }
    }
}

// The fused backward kernels evaluate (dA, dB) for the 10 x 66 halo of an 8 x 64 pixel tile into LDS (1.29x the evaluations)
// and gather from there, so that the [N,H,W,6] intermediate never reaches memory.
constexpr int SB_TR = 8, SB_TW = 64, SB_HR = SB_TR + 2, SB_HC = SB_TW + 2, SB_HP = SB_HR * SB_HC;

// sum over the pixels p around q = (x, y) of the taps of (dA_p, dB_p) that land on q; (h0, w0) = the tile's first pixel
__device__ __forceinline__ V3 gather_ab(const float (&abl)[6][SB_HP], int x, int y, int h0, int w0, int H, int W) {
    V3 s{0, 0, 0};
    for (int py = max(y - 1, 0); py <= min(y + 1, H - 1); ++py) {
        float dyw, syw;
        tap_weights(y, py, H, dyw, syw);
        for (int px = max(x - 1, 0); px <= min(x + 1, W - 1); ++px) {
            float dxw, sxw;
            tap_weights(x, px, W, dxw, sxw);
            const float ka = syw * dxw * 0.125f, kb = dyw * sxw * 0.125f;
            const int q = (py - h0 + 1) * SB_HC + (px - w0 + 1);
            s.x += ka * abl[0][q] + kb * abl[3][q]; s.y += ka * abl[1][q] + kb * abl[4][q];
            s.z += ka * abl[2][q] + kb * abl[5][q];
        }
    }
    return s;
}

}  // namespace pd_dn
