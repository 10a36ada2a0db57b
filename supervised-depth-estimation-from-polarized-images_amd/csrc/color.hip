// Colour half of the loader on the device: torchvision 0.8.2's PIL ColorJitter (indoor_dataset.py:92-106, 226-233,
// 404-407) on uint8 planar RGB, Pillow-exact, fused with the loader's uint8 -> float32 / 255 conversion
// (indoor_dataset.py:192-233 to_tensor).  The per-pixel arithmetic is color_math.hpp.
//
// Two launches per call at most:
//   reduce  (only with params): the contrast degenerate is int(mean L + 0.5) of the sample as it stands when contrast is
//           reached; the operations in front of it are pointwise, so every workgroup recomputes them from src, sums L in
//           integers and adds its partial to the sample's 64-bit word with one integer atomic (exact, order-free).  The
//           workgroup that arrives last turns the sum into the mean and leaves sum and ticket zero for the next call.
//   apply   reads 3 B, writes 3 B (uint8) and / or 12 B (fp32) per pixel: four pixels per lane (one dword load per plane,
//           one 16-byte store per plane) when H*W is a multiple of 4, one pixel per lane otherwise.
// The chain codes are device data (one fp64 row per sample), so a captured step replays with new draws.
#include "pd_common.h"
#include "color_math.hpp"

namespace {

using namespace pdcolor;

struct SampleWs {             // 16 bytes per sample in sum_ws
    unsigned long long sum;   // zero on entry, zero on exit
    unsigned ticket;          // zero on entry, zero on exit
    int mean;                 // written by reduce, read by apply
};

constexpr int kThreads = 256;

template <int V> __device__ __forceinline__ void load_px(const uint8_t* p, int (&c)[V]);
template <> __device__ __forceinline__ void load_px<1>(const uint8_t* p, int (&c)[1]) { c[0] = *p; }
template <> __device__ __forceinline__ void load_px<4>(const uint8_t* p, int (&c)[4]) {
    const uchar4 v = *reinterpret_cast<const uchar4*>(p);
    c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
}

template <int V> __device__ __forceinline__ void store_u8(uint8_t* p, const int (&c)[V]);
template <> __device__ __forceinline__ void store_u8<1>(uint8_t* p, const int (&c)[1]) { *p = (uint8_t)c[0]; }
template <> __device__ __forceinline__ void store_u8<4>(uint8_t* p, const int (&c)[4]) {
    *reinterpret_cast<uchar4*>(p) = make_uchar4((uint8_t)c[0], (uint8_t)c[1], (uint8_t)c[2], (uint8_t)c[3]);
}

// (float)u / 255.0f, IEEE division: np.float32(u) / 255.0 for all 256 values (tests/test_color_gpu.py)
__device__ __forceinline__ float unit(int u) { return __fdiv_rn((float)u, 255.0f); }

template <int V> __device__ __forceinline__ void store_f32(float* p, const int (&c)[V]);
template <> __device__ __forceinline__ void store_f32<1>(float* p, const int (&c)[1]) { *p = unit(c[0]); }
template <> __device__ __forceinline__ void store_f32<4>(float* p, const int (&c)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(unit(c[0]), unit(c[1]), unit(c[2]), unit(c[3]));
}

// src [B][3][HW]; grid (x: pixel groups of the sample, y: samples)
template <int V>
__global__ __launch_bounds__(kThreads) void color_reduce_kernel(const uint8_t* __restrict__ src, const double* __restrict__ params,
                                                                SampleWs* __restrict__ ws, int B, long HW) {
    __shared__ unsigned long long part[kThreads / 64];
    const long groups = HW / V;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const Chain ch = decode_row(params + 8L * b);
        if (ch.contrast_at == 4) continue;            // uniform over the workgroup
        const uint8_t* s = src + 3L * b * HW;
        unsigned long long acc = 0;
        for (long gi = blockIdx.x * (long)kThreads + threadIdx.x; gi < groups; gi += (long)gridDim.x * kThreads) {
            int r[V], g[V], bl[V];
            load_px<V>(s + gi * V, r);
            load_px<V>(s + HW + gi * V, g);
            load_px<V>(s + 2 * HW + gi * V, bl);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                apply_ops(ch, 0, ch.contrast_at, 0, r[j], g[j], bl[j]);
                acc += (unsigned)luma(r[j], g[j], bl[j]);
            }
        }
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        __syncthreads();                              // part[] of the previous sample has been read
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long total = 0;
            for (int w = 0; w < kThreads / 64; ++w) total += part[w];
            atomicAdd(&ws[b].sum, total);
            __threadfence();
            if (atomicAdd(&ws[b].ticket, 1u) == gridDim.x - 1) {     // every workgroup of the sample has added its partial
                __threadfence();
                const unsigned long long sum = atomicExch(&ws[b].sum, 0ull);
                ws[b].mean = contrast_mean(sum, HW);
                atomicExch(&ws[b].ticket, 0u);
            }
        }
    }
}

template <int V>
__global__ __launch_bounds__(kThreads) void color_apply_kernel(const uint8_t* __restrict__ src, const double* __restrict__ params,
                                                               const SampleWs* __restrict__ ws, uint8_t* __restrict__ dst_u8,
                                                               float* __restrict__ dst_f32, int B, long HW) {
    const long groups = HW / V;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        Chain ch = {};
        int mean = 0;
        bool identity = true;
        if (params) {
            ch = decode_row(params + 8L * b);
            identity = (ch.code[0] | ch.code[1] | ch.code[2] | ch.code[3]) == 0;
            if (ch.contrast_at < 4) mean = ws[b].mean;
        }
        const long base = 3L * b * HW;
        for (long gi = blockIdx.x * (long)kThreads + threadIdx.x; gi < groups; gi += (long)gridDim.x * kThreads) {
            const long i = base + gi * V;
            int r[V], g[V], bl[V];
            load_px<V>(src + i, r);
            load_px<V>(src + i + HW, g);
            load_px<V>(src + i + 2 * HW, bl);
            if (!identity) {
#pragma unroll
                for (int j = 0; j < V; ++j) apply_ops(ch, 0, 4, mean, r[j], g[j], bl[j]);
            }
            if (dst_u8) {
                store_u8<V>(dst_u8 + i, r);
                store_u8<V>(dst_u8 + i + HW, g);
                store_u8<V>(dst_u8 + i + 2 * HW, bl);
            }
            if (dst_f32) {
                store_f32<V>(dst_f32 + i, r);
                store_f32<V>(dst_f32 + i + HW, g);
                store_f32<V>(dst_f32 + i + 2 * HW, bl);
            }
        }
    }
}

inline unsigned blocks_for(long groups, long cap) {
    const long b = (groups + kThreads - 1) / kThreads;
    return (unsigned)(b > cap ? cap : (b < 1 ? 1 : b));
}

}  // namespace

static_assert(sizeof(SampleWs) == 16, "sum_ws is documented as 16 bytes per sample (include/polardepth.h)");

extern "C" int pd_color_jitter_u8(const void* src, const void* params, void* dst_u8, void* dst_f32, void* sum_ws,
                                  int B, int H, int W, void* stream) {
    PD_REQUIRE(B >= 0 && H > 0 && W > 0, "pd_color_jitter_u8: bad shape (B=%d H=%d W=%d)", B, H, W);
    if (B == 0) return PD_OK;
    PD_REQUIRE(src, "pd_color_jitter_u8: null src");
    PD_REQUIRE(dst_u8 || dst_f32, "pd_color_jitter_u8: both outputs are null");
    PD_REQUIRE(!params || sum_ws, "pd_color_jitter_u8: params need the sum_ws workspace");
    PD_REQUIRE(!params || (((uintptr_t)params | (uintptr_t)sum_ws) & 7u) == 0,
               "pd_color_jitter_u8: params and sum_ws must be 8-byte aligned");
    PD_REQUIRE(!dst_f32 || ((uintptr_t)dst_f32 & 3u) == 0, "pd_color_jitter_u8: dst_f32 must be 4-byte aligned");
    const long HW = (long)H * W;
    // four pixels per lane: every plane of every sample then starts on a dword (uint8) / 16-byte (fp32) boundary
    const bool wide = HW % 4 == 0 && ((uintptr_t)src & 3u) == 0 && (!dst_u8 || ((uintptr_t)dst_u8 & 3u) == 0) &&
                      (!dst_f32 || pd::aligned16(dst_f32));
    const long groups = wide ? HW / 4 : HW;
    const unsigned gy = (unsigned)(B > 65535 ? 65535 : B);
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* s = (const uint8_t*)src;
    const double* p = (const double*)params;
    SampleWs* ws = (SampleWs*)sum_ws;
    if (params) {
        const dim3 grid(blocks_for(groups, 256), gy);
        if (wide) hipLaunchKernelGGL(color_reduce_kernel<4>, grid, dim3(kThreads), 0, st, s, p, ws, B, HW);
        else hipLaunchKernelGGL(color_reduce_kernel<1>, grid, dim3(kThreads), 0, st, s, p, ws, B, HW);
        const int rc = pd::check_launch("pd_color_jitter_u8 (reduce)");
        if (rc != PD_OK) return rc;
    }
    const dim3 grid(blocks_for(groups, 4096), gy);
    if (wide)
        hipLaunchKernelGGL(color_apply_kernel<4>, grid, dim3(kThreads), 0, st, s, p, ws, (uint8_t*)dst_u8, (float*)dst_f32, B, HW);
    else
        hipLaunchKernelGGL(color_apply_kernel<1>, grid, dim3(kThreads), 0, st, s, p, ws, (uint8_t*)dst_u8, (float*)dst_f32, B, HW);
    return pd::check_launch("pd_color_jitter_u8");
}
