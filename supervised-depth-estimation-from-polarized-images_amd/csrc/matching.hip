// Multi-frame cost volume from known poses: the plane sweep of ManyDepth's ResnetEncoderMatching, fused.
//
// Reference restated (include/polardepth.h, "multi-frame cost volume", states the arithmetic):
//   resnet_encoder.py:430-511  match_features     per item and lookup frame: repeat the feature map D times, BackprojectDepth at
//                                                 the D hypothesised depths, Project3D, grid_sample(zeros, align_corners=True),
//                                                 edge mask, mean_c |warped - cur|, sum / count over the frames, fill missing
//   resnet_encoder.py:534-541  compute_confidence_mask
//   resnet_encoder.py:623-630  argmin over (0 -> 100), indices_to_disparity, cost *= confidence
// The reference materialises D x C x h x w warped features per item and frame; here a (pixel, bin, frame) entry is four
// C-float taps, read where the edge mask is 1 and nowhere else, and the per-pixel finish needs that pixel's D sums only.
//
// One workgroup (256 threads) owns MP = 8 consecutive pixels of one batch item (blockIdx.y) and ALL their bins:
//   phase A  one lane per (pixel, bin): the fp64 projection (view_geom.hpp, the expressions csrc/reproj.hip warps with) and
//            the edge mask of the frame -> LDS (u, v), u = -1 where masked
//   phase B  a wavefront owns a pixel (pixels w and w + 4 in turn), its four 16-lane rows take bins d = row, row + 4, ...:
//            lane l of a row holds channels 4l..4l+3 (+64k) of the pixel's `cur` in registers across all bins and frames, a tap
//            is one 16-byte load per lane (256 B per row at C = 64), the L1 distance is summed per lane and by a 4-step
//            butterfly inside the row; lane 0 adds it to the entry's sum in LDS.  A masked entry costs one LDS read.
//   finish   32 lanes per pixel: c = s / (n + 1e-7), maximum, count of c > 0, first minimum, stores.
// No atomics, no second launch, no inline assembly; nothing but `cost`, `missing` and three maps is written.
#include "pd_common.h"
#include "view_geom.hpp"

namespace {

constexpr int MT = 256;            // threads per workgroup
constexpr int MP = 8;              // pixels per workgroup
constexpr int MD = 128;            // most depth bins
constexpr int MF = 8;              // = PD_REPROJ_MAX_FRAMES

struct MatchArgs {
    const float* cur;
    const float* lookup;
    const float* T;
    const float* K;
    const float* iK;
    const float* bins;
    const float* valid;
    float* cost;
    unsigned char* missing;
    float* confidence;
    int* argmin;
    float* lowest;
    int F, h, w, C, D;
    long ldc;
    int apply_confidence;
};

__device__ __forceinline__ float row_sum16(float v) {
    // lanes l and l ^ 1, then ^ 2, ^ 4, ^ 8: a binary tree over the 16 lanes of a row, every lane ends with the same bits
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 16);
    return v;
}

__device__ __forceinline__ float l1_4(float4 a, float4 b, float4 c, float4 d, const pd_geom::Bilinear& bl, float4 cur,
                                      float acc) {
    acc += fabsf(bl.blend(a.x, b.x, c.x, d.x) - cur.x);
    acc += fabsf(bl.blend(a.y, b.y, c.y, d.y) - cur.y);
    acc += fabsf(bl.blend(a.z, b.z, c.z, d.z) - cur.z);
    acc += fabsf(bl.blend(a.w, b.w, c.w, d.w) - cur.w);
    return acc;
}

__global__ __launch_bounds__(MT) void cost_volume_kernel(const MatchArgs a) {
    __shared__ double sP[MF][12];      // (K T)[:3,:] of every frame, row-major 3x4
    __shared__ double sIK[9];          // inv_K[:3,:3]
    __shared__ float sValid[MF];
    __shared__ float sBins[MD];
    __shared__ float2 sUV[MP * MD];
    __shared__ float sSum[MP * MD];
    __shared__ int sCnt[MP * MD];

    const int t = threadIdx.x;
    const long b = blockIdx.y;
    const int F = a.F, D = a.D, w = a.w, h = a.h, C = a.C;
    const int HW = h * w;
    const int pix0 = blockIdx.x * MP;
    const int E = MP * D;

    if (t < 12 * F) {
        const int f = t / 12, q = t - 12 * f;
        sP[f][q] = pd_geom::cam_P(a.K + b * 16, a.T + (b * F + f) * 16, q);
    } else if (t >= 128 && t < 137) {
        sIK[t - 128] = pd_geom::cam_iK(a.iK, b, t - 128);
    } else if (t >= 160 && t < 160 + F) {
        sValid[t - 160] = a.valid ? a.valid[b * F + (t - 160)] : 1.f;
    }
    if (t < D) sBins[t] = a.bins[t];
    for (int e = t; e < E; e += MT) { sSum[e] = 0.f; sCnt[e] = 0; }
    __syncthreads();

    const int wave = t >> 6, row = (t >> 4) & 3, sub = t & 15;
    const int C4 = C >> 2;
    const float xhi = (float)(w - 2), yhi = (float)(h - 2);

    for (int f = 0; f < F; ++f) {
        if (sValid[f] == 0.f) continue;                       // the same for the whole workgroup
        // ---- phase A: project every (pixel, bin) of this frame
        for (int e = t; e < E; e += MT) {
            const int pl = e / D, d = e - pl * D;
            const int pix = pix0 + pl;
            float2 uv = make_float2(-1.f, 0.f);
            if (pix < HW) {
                const int y = pix / w, x = pix - y * w;
                if (x >= 2 && x < w - 2 && y >= 2 && y < h - 2) {
                    double r[3], q[3], p[3], u, v, hz;
                    pd_geom::ray(sIK, x, y, r);
                    pd_geom::project_ray(sP[f], r, (double)sBins[d], u, v, hz, q, p);
                    const float uf = (float)u, vf = (float)v;
                    if (uf >= 2.f && uf <= xhi && vf >= 2.f && vf <= yhi) uv = make_float2(uf, vf);   // false for NaN
                }
            }
            sUV[e] = uv;
        }
        __syncthreads();
        // ---- phase B: gather, L1 distance
        const float* src = a.lookup + (b * F + f) * (long)HW * C;
        for (int pl = wave; pl < MP; pl += 4) {
            const int pix = pix0 + pl;
            if (pix >= HW) break;
            const float* cp = a.cur + (b * HW + pix) * (long)C;
            float4 cur0 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (sub < C4) cur0 = *reinterpret_cast<const float4*>(cp + 4 * sub);
            for (int d = row; d < D; d += 4) {
                const int e = pl * D + d;
                const float2 uv = sUV[e];
                if (uv.x < 0.f) continue;                     // (pixel, bin) granularity: the 16 lanes of a row agree
                const float fx = floorf(uv.x), fy = floorf(uv.y);
                const pd_geom::Bilinear bl(uv.x - fx, uv.y - fy);
                // 2 <= u <= w-2 and 2 <= v <= h-2: all four taps are inside the image
                const float* s00 = src + ((long)(int)fy * w + (int)fx) * C;
                const float* s01 = s00 + (long)w * C;
                float acc = 0.f;
                if (sub < C4)
                    acc = l1_4(*reinterpret_cast<const float4*>(s00 + 4 * sub), *reinterpret_cast<const float4*>(s00 + C + 4 * sub),
                               *reinterpret_cast<const float4*>(s01 + 4 * sub), *reinterpret_cast<const float4*>(s01 + C + 4 * sub),
                               bl, cur0, acc);
                for (int q = sub + 16; q < C4; q += 16)
                    acc = l1_4(*reinterpret_cast<const float4*>(s00 + 4 * q), *reinterpret_cast<const float4*>(s00 + C + 4 * q),
                               *reinterpret_cast<const float4*>(s01 + 4 * q), *reinterpret_cast<const float4*>(s01 + C + 4 * q),
                               bl, *reinterpret_cast<const float4*>(cp + 4 * q), acc);
                const float diff = row_sum16(acc) / (float)C;
                if (sub == 0) {
                    sSum[e] += diff;
                    sCnt[e] += (diff > 0.f) ? 1 : 0;
                }
            }
        }
        __syncthreads();
    }

    // ---- finish: 32 lanes per pixel, lane j holds bins j, j + 32, j + 64, j + 96
    const int pl = t >> 5, j = t & 31;
    const int pix = pix0 + pl;
    if (pix >= HW) return;                                    // no barrier below
    float c[4];
    bool any_nan = false;
    float mx = 0.f;                                           // c >= 0 wherever it is a number
    int pos = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int d = j + 32 * k;
        c[k] = 0.f;
        if (d < D) {
            const int e = pl * D + d;
            c[k] = sSum[e] / ((float)sCnt[e] + 1e-7f);
            any_nan |= (c[k] != c[k]);
            mx = fmaxf(mx, c[k]);                             // skips a NaN operand
            pos += (c[k] > 0.f) ? 1 : 0;
        }
    }
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, o, 32));
        pos += __shfl_xor(pos, o, 32);
        any_nan |= (__shfl_xor((int)any_nan, o, 32) != 0);
    }
    if (any_nan) mx = __int_as_float(0x7fc00000);             // the maximum propagates a NaN, as torch's and NumPy's do
    const float conf = (pos == D) ? 1.f : 0.f;
    // first minimum of (filled == 0 ? 100 : filled); a NaN counts as smaller than every number, the first NaN wins
    float best = 0.f;
    int arg = 0x7fffffff;
    const long o0 = b * HW + pix;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int d = j + 32 * k;
        if (d < D) {
            const bool miss = (c[k] == 0.f);
            const float filled = miss ? mx : c[k];
            float key = (filled == 0.f) ? 100.f : filled;
            if (key != key) key = -1.f;
            if (arg == 0x7fffffff || key < best) { best = key; arg = d; }    // d ascending: ties keep the earlier bin
            a.cost[o0 * a.ldc + d] = a.apply_confidence ? filled * conf : filled;
            if (a.missing) a.missing[o0 * D + d] = miss ? 1 : 0;
        }
    }
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
        const float ob = __shfl_xor(best, o, 32);
        const int oa = __shfl_xor(arg, o, 32);
        if (oa != 0x7fffffff && (arg == 0x7fffffff || ob < best || (ob == best && oa < arg))) { best = ob; arg = oa; }
    }
    if (j == 0) {
        a.confidence[o0] = conf;
        a.argmin[o0] = arg;
        a.lowest[o0] = 1.f / sBins[arg];
    }
}

}  // namespace

// ============================================================================ C ABI
extern "C" int pd_cost_volume(const void* cur, const void* lookup, const void* T, const void* K, const void* inv_K,
                              const void* bins, const void* valid, void* cost, long ldc, void* missing, void* confidence,
                              void* argmin, void* lowest, int B, int F, int h, int w, int C, int D, int apply_confidence,
                              void* stream) {
    PD_REQUIRE(B >= 0 && B <= 65535 && h >= 1 && w >= 1, "pd_cost_volume: bad shape B=%d h=%d w=%d (0 <= B <= 65535)", B, h, w);
    PD_REQUIRE((long)h * w <= (1L << 30), "pd_cost_volume: image too large (%d x %d)", h, w);
    PD_REQUIRE(C >= 4 && C % 4 == 0, "pd_cost_volume: C must be a positive multiple of 4 channels, got %d", C);
    PD_REQUIRE(D >= 1 && D <= MD, "pd_cost_volume: 1 <= D <= %d depth bins, got %d", MD, D);
    PD_REQUIRE(F >= 0 && F <= MF, "pd_cost_volume: 0 <= F <= %d frames, got %d", MF, F);
    PD_REQUIRE(ldc >= D, "pd_cost_volume: the pixel stride ldc = %ld is smaller than D = %d", ldc, D);
    PD_REQUIRE(cur && K && inv_K && bins && cost && confidence && argmin && lowest,
               "pd_cost_volume: cur, K, inv_K, bins, cost, confidence, argmin and lowest must not be null");
    PD_REQUIRE(F == 0 || (lookup && T), "pd_cost_volume: lookup and T must not be null when F > 0");
    PD_REQUIRE(pd::aligned16(cur) && pd::aligned16(lookup), "pd_cost_volume: cur and lookup must be 16-byte aligned");
    PD_REQUIRE(apply_confidence == 0 || apply_confidence == 1, "pd_cost_volume: apply_confidence must be 0 or 1, got %d",
               apply_confidence);
    if (B == 0) return PD_OK;
    MatchArgs a;
    a.cur = (const float*)cur; a.lookup = (const float*)lookup; a.T = (const float*)T; a.K = (const float*)K;
    a.iK = (const float*)inv_K; a.bins = (const float*)bins; a.valid = (const float*)valid;
    a.cost = (float*)cost; a.missing = (unsigned char*)missing; a.confidence = (float*)confidence; a.argmin = (int*)argmin;
    a.lowest = (float*)lowest;
    a.F = F; a.h = h; a.w = w; a.C = C; a.D = D; a.ldc = ldc; a.apply_confidence = apply_confidence;
    const long HW = (long)h * w;
    hipLaunchKernelGGL(cost_volume_kernel, dim3((unsigned)((HW + MP - 1) / MP), B), dim3(MT), 0, (hipStream_t)stream, a);
    return pd::check_launch("pd_cost_volume");
}
