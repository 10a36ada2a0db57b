// Pillow-compatible 8-bit LANCZOS resampling of the polarizer planes on the device
// (Image.resize((W,H), Image.ANTIALIAS) in indoor_dataset.py:335-349 = ImagingResample, 8bpc branch):
// a horizontal pass and a vertical pass with fixed-point (22-bit) coefficients,
//   out = clip8((2^21 + sum_x in[xmin + x] * k[x]) >> 22),
// the intermediate image rounded to uint8 like Pillow.  The coefficient / bound tables are built on the host
// (polardepth/resize.py, Pillow's precompute_coeffs + normalize_coeffs_8bpc in double precision) -- with them the
// result is bit-identical to PIL (tests/test_resize_gpu.py).  Used when the loader hands over the raw frames
// (decode on the host, resize + K1 on the device).
// 16-bit and float planes (modes I;16 and F) take the second entry point below: double coefficients, double accumulation,
// Pillow's store per mode (tests/test_resize_wide_gpu.py).
#include "pd_common.h"

namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;

__device__ __forceinline__ uint8_t clip8(int acc) {
    const int v = acc >> kPrecisionBits;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// src [P][H][Ws] -> dst [P][H][Wd]
__global__ __launch_bounds__(256) void resize_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                       const int* __restrict__ kk, const int* __restrict__ bounds,
                                                       int ksize, long rows, int Ws, int Wd) {
    const long total = rows * Wd;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / Wd;
        const int xx = (int)(i - r * Wd);
        const int xmin = bounds[2 * xx], xn = bounds[2 * xx + 1];
        const uint8_t* s = src + r * Ws + xmin;
        const int* k = kk + (long)xx * ksize;
        int acc = 1 << (kPrecisionBits - 1);
        for (int x = 0; x < xn; ++x) acc += (int)s[x] * k[x];
        dst[i] = clip8(acc);
    }
}

// src [P][Hs][W] -> dst [P][Hd][W]
__global__ __launch_bounds__(256) void resize_v_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                       const int* __restrict__ kk, const int* __restrict__ bounds,
                                                       int ksize, int P, int Hs, int Hd, int W) {
    const long total = (long)P * Hd * W;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int x = (int)(i % W);
        const long t = i / W;
        const int yy = (int)(t % Hd);
        const long p = t / Hd;
        const int ymin = bounds[2 * yy], yn = bounds[2 * yy + 1];
        const uint8_t* s = src + (p * Hs + ymin) * W + x;
        const int* k = kk + (long)yy * ksize;
        int acc = 1 << (kPrecisionBits - 1);
        for (int y = 0; y < yn; ++y) acc += (int)s[(long)y * W] * k[y];
        dst[i] = clip8(acc);
    }
}

inline unsigned grid_for(long n) {
    const long b = (n + 255) / 256;
    return (unsigned)(b > 65536 ? 65536 : (b < 1 ? 1 : b));
}

// ---- 16-bit and float planes: ImagingResampleHorizontal_16bpc / Vertical_16bpc (mode I;16) and the IMAGING_TYPE_FLOAT32
// case of ImagingResampleHorizontal_32bpc / Vertical_32bpc (mode F) of Pillow's Resample.c.  Double coefficients
// (precompute_coeffs without normalize_coeffs_8bpc), ss = 0; ss += (double)in[x] * k[x] in tap order -- multiply and add
// stay separate (the Makefile's -ffp-contract=off; no fma is written here) --, then one store per mode.
__device__ __forceinline__ int clip255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

template <typename T>
__device__ __forceinline__ T wide_store(double ss);
// mode F: IMAGING_PIXEL_F(imOut, xx, yy) = ss
template <>
__device__ __forceinline__ float wide_store<float>(double ss) {
    return (float)ss;
}
// mode I;16: ss_int = ROUND_UP(ss), then BYTEWISE low = CLIP8(ss_int % 256), high = CLIP8(ss_int >> 8).  C's remainder is
// negative for a negative ss_int, so undershoot stores 0; past 65535 the high byte clips to 255 and the low byte WRAPS
// (65536 + 300 -> 0xff2c, not 0xffff).  That is what PIL returns, so that is what the device returns.
template <>
__device__ __forceinline__ uint16_t wide_store<uint16_t>(double ss) {
    const int v = ss >= 0.0 ? (int)(ss + 0.5) : (int)(ss - 0.5);
    return (uint16_t)(clip255(v % 256) | (clip255(v >> 8) << 8));
}

// (first, count) of one output index, held inside [0, n) and the table's row length whatever the table says
__device__ __forceinline__ void tap_range(const int* __restrict__ bounds, int i, int n, int ksize, int& first, int& count) {
    first = bounds[2 * i];
    count = bounds[2 * i + 1];
    if (first < 0) first = 0;
    if (first > n) first = n;
    if (count > ksize) count = ksize;
    if (count > n - first) count = n - first;
}

// src [rows][Ws] -> dst [rows][Wd]
template <typename T>
__global__ __launch_bounds__(256) void resize_wide_h_kernel(const T* __restrict__ src, T* __restrict__ dst,
                                                            const double* __restrict__ kk, const int* __restrict__ bounds,
                                                            int ksize, long rows, int Ws, int Wd) {
    const long total = rows * Wd;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / Wd;
        const int xx = (int)(i - r * Wd);
        int xmin, xn;
        tap_range(bounds, xx, Ws, ksize, xmin, xn);
        const T* s = src + r * Ws + xmin;
        const double* k = kk + (long)xx * ksize;
        double ss = 0.0;
        for (int x = 0; x < xn; ++x) ss += (double)s[x] * k[x];
        dst[i] = wide_store<T>(ss);
    }
}

// src [P][Hs][W] -> dst [P][Hd][W]
template <typename T>
__global__ __launch_bounds__(256) void resize_wide_v_kernel(const T* __restrict__ src, T* __restrict__ dst,
                                                            const double* __restrict__ kk, const int* __restrict__ bounds,
                                                            int ksize, int P, int Hs, int Hd, int W) {
    const long total = (long)P * Hd * W;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int x = (int)(i % W);
        const long t = i / W;
        const int yy = (int)(t % Hd);
        const long p = t / Hd;
        int ymin, yn;
        tap_range(bounds, yy, Hs, ksize, ymin, yn);
        const T* s = src + (p * Hs + ymin) * W + x;
        const double* k = kk + (long)yy * ksize;
        double ss = 0.0;
        for (int y = 0; y < yn; ++y) ss += (double)s[(long)y * W] * k[y];
        dst[i] = wide_store<T>(ss);
    }
}

template <typename T>
void launch_wide(const void* src, void* dst, const void* coeffs, const void* bounds, int ksize, int P, int Hs, int Ws,
                 int out_size, int vertical, hipStream_t st) {
    if (vertical)
        hipLaunchKernelGGL(resize_wide_v_kernel<T>, dim3(grid_for((long)P * out_size * Ws)), dim3(256), 0, st, (const T*)src,
                           (T*)dst, (const double*)coeffs, (const int*)bounds, ksize, P, Hs, out_size, Ws);
    else
        hipLaunchKernelGGL(resize_wide_h_kernel<T>, dim3(grid_for((long)P * Hs * out_size)), dim3(256), 0, st, (const T*)src,
                           (T*)dst, (const double*)coeffs, (const int*)bounds, ksize, (long)P * Hs, Ws, out_size);
}

}  // namespace

extern "C" int pd_resize_wide_pass(const void* src, void* dst, int dtype, const void* coeffs, const void* bounds, int ksize,
                                   int P, int Hs, int Ws, int out_size, int vertical, void* stream) {
    PD_REQUIRE(P >= 0 && Hs > 0 && Ws > 0 && out_size > 0 && ksize > 0, "pd_resize_wide_pass: bad shape");
    PD_REQUIRE(dtype == PD_POLAR_U16 || dtype == PD_POLAR_F32,
               "pd_resize_wide_pass: dtype %d is neither PD_POLAR_U16 nor PD_POLAR_F32 (uint8 planes: pd_resize_u8_pass)", dtype);
    if (P == 0) return PD_OK;
    PD_REQUIRE(src && dst && coeffs && bounds, "pd_resize_wide_pass: null pointer");
    const uintptr_t elem = dtype == PD_POLAR_U16 ? 2 : 4;
    PD_REQUIRE(((uintptr_t)src | (uintptr_t)dst) % elem == 0 && (uintptr_t)coeffs % 8 == 0 && (uintptr_t)bounds % 4 == 0,
               "pd_resize_wide_pass: a pointer is not aligned to its element type");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == PD_POLAR_U16)
        launch_wide<uint16_t>(src, dst, coeffs, bounds, ksize, P, Hs, Ws, out_size, vertical, st);
    else
        launch_wide<float>(src, dst, coeffs, bounds, ksize, P, Hs, Ws, out_size, vertical, st);
    return pd::check_launch("pd_resize_wide_pass");
}

extern "C" int pd_resize_u8_pass(const void* src, void* dst, const void* coeffs, const void* bounds, int ksize,
                                 int P, int Hs, int Ws, int out_size, int vertical, void* stream) {
    PD_REQUIRE(P >= 0 && Hs > 0 && Ws > 0 && out_size > 0 && ksize > 0, "pd_resize_u8_pass: bad shape");
    if (P == 0) return PD_OK;
    PD_REQUIRE(src && dst && coeffs && bounds, "pd_resize_u8_pass: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (vertical)
        hipLaunchKernelGGL(resize_v_kernel, dim3(grid_for((long)P * out_size * Ws)), dim3(256), 0, st, (const uint8_t*)src,
                           (uint8_t*)dst, (const int*)coeffs, (const int*)bounds, ksize, P, Hs, out_size, Ws);
    else
        hipLaunchKernelGGL(resize_h_kernel, dim3(grid_for((long)P * Hs * out_size)), dim3(256), 0, st, (const uint8_t*)src,
                           (uint8_t*)dst, (const int*)coeffs, (const int*)bounds, ksize, (long)P * Hs, Ws, out_size);
    return pd::check_launch("pd_resize_u8_pass");
}
