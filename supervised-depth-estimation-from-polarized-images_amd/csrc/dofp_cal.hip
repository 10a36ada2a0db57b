// Super-pixel calibration of division-of-focal-plane (DoFP) polarizer frames on the device (Powell & Gruev, "Calibration
// methods for division-of-focal-plane polarimeters", Opt. Express 2013): a dark frame plus one 4x4 matrix per 2x2 polarizer
// cell that maps the four measured samples to what an ideal cell would have measured.
//   pd_frame_moments   weighted sums over a stack of frames (the mean dark frame; the three moments of a flat-field series)
//   pd_dofp_cal_solve  the per-cell matrices from those moments
//   pd_dofp_calibrate  dark + matrix (or dark + per-pixel gain) applied to incoming frames, before the demosaic
// Definition: include/polardepth.h; fp64 statement: tests/dofp_cal_ref.py.  Every step is fp64 in the header's order, rounded
// once where a narrower type is stored; -ffp-contract=off (Makefile) keeps each product and sum an operation of its own.
//
// All four kernels stream: capped grid, grid-stride loop, no LDS, no cross-thread reduction.
//   - apply, CELL: a lane owns two adjacent cells (one where W2 % 4 == 2), loads their matrices and dark ONCE and loops over
//     the B frames, so the 16 bytes / pixel of matrices are read once per launch, not B times.  Per frame a lane loads two
//     row pieces of 4 (2) samples and stores two of 16 (8) bytes.
//   - apply, PIXEL and the moments: a frame is H2 x W2 with both sides even, so it is a whole number of 4-pixel groups and a
//     group never needs its row: a lane owns 4 consecutive pixels of the flat frame, always aligned to 4 elements.
//   - solve: one cell per lane, six 16-byte loads of moments, four 16-byte stores of the matrix.
#include <cmath>
#include "pd_common.h"

namespace {

constexpr int kThreads = 256;
constexpr long kMaxBlocks = 2048;      // 256 CUs x 8 workgroups; the rest of the work is grid-strided

inline unsigned grid_for(long items) {
    const long b = (items + kThreads - 1) / kThreads;
    return (unsigned)(b > kMaxBlocks ? kMaxBlocks : (b < 1 ? 1 : b));
}

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

template <int BYTES> struct vec_of;
template <> struct vec_of<2> { using type = uint16_t; };
template <> struct vec_of<4> { using type = uint32_t; };
template <> struct vec_of<8> { using type = u32x2; };
template <> struct vec_of<16> { using type = u32x4; };

// K elements of T at p (aligned to K * sizeof(T) bytes) as doubles
template <typename T, int K>
__device__ __forceinline__ void load_as_double(const T* __restrict__ p, double (&e)[K]) {
    using V = typename vec_of<K * (int)sizeof(T)>::type;
    union { V v; T t[K]; } u;
    u.v = *reinterpret_cast<const V*>(p);
#pragma unroll
    for (int j = 0; j < K; ++j) e[j] = (double)u.t[j];
}

template <int K>
__device__ __forceinline__ void store_floats(float* __restrict__ p, const float (&o)[K]) {
    if constexpr (K == 4) *reinterpret_cast<f32x4*>(p) = f32x4{o[0], o[1], o[2], o[3]};
    else *reinterpret_cast<f32x2*>(p) = f32x2{o[0], o[1]};
}

// -------------------------------------------------------------------------------------------------------- moments
// out[q][i] = (accumulate ? out[q][i] : 0) + sum_n w[n][q] * (f[n][i] - dark[i]), n ascending.  groups = H2 * W2 / 4.
template <typename T, int Q>
__global__ __launch_bounds__(kThreads) void frame_moments_kernel(const T* __restrict__ frames, const float* __restrict__ dark,
                                                                 const double* __restrict__ weights, double* __restrict__ out,
                                                                 int N, int groups, int accumulate) {
    const long plane = 4L * groups;
    for (int g = blockIdx.x * kThreads + threadIdx.x; g < groups; g += gridDim.x * kThreads) {
        const int i = 4 * g;                                   // < H2 * W2 <= 2^30
        double d[4] = {0.0, 0.0, 0.0, 0.0};
        if (dark) load_as_double<float, 4>(dark + i, d);
        double acc[Q][4];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            if (accumulate) {
                const f64x2 a = *reinterpret_cast<const f64x2*>(out + q * plane + i);
                const f64x2 b = *reinterpret_cast<const f64x2*>(out + q * plane + i + 2);
                acc[q][0] = a.x, acc[q][1] = a.y, acc[q][2] = b.x, acc[q][3] = b.y;
            } else {
                acc[q][0] = acc[q][1] = acc[q][2] = acc[q][3] = 0.0;
            }
        }
        for (int n = 0; n < N; ++n) {
            double f[4];
            load_as_double<T, 4>(frames + n * plane + i, f);
            double w[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) w[q] = weights[(long)n * Q + q];      // the same address in every lane
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double e = dark ? f[j] - d[j] : f[j];
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const double t = w[q] * e;
                    acc[q][j] = acc[q][j] + t;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            *reinterpret_cast<f64x2*>(out + q * plane + i) = f64x2{acc[q][0], acc[q][1]};
            *reinterpret_cast<f64x2*>(out + q * plane + i + 2) = f64x2{acc[q][2], acc[q][3]};
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- solve
struct SolveArgs {
    double rinv[9];
    double a_nom[12];
    double qmin;
};

__global__ __launch_bounds__(kThreads) void dofp_cal_solve_kernel(const double* __restrict__ moments, float* __restrict__ gain,
                                                                  float* __restrict__ quality, SolveArgs k, int h, int w) {
    const int cells = h * w;                                   // <= 2^28
    const int W2 = 2 * w;
    const long plane = 4L * cells;
    for (int c = blockIdx.x * kThreads + threadIdx.x; c < cells; c += gridDim.x * kThreads) {
        const int i = c / w, j = c - i * w;
        double m[4][3];
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const f64x2 v = *reinterpret_cast<const f64x2*>(moments + q * plane + (2 * i + r) * W2 + 2 * j);
                m[2 * r][q] = v.x, m[2 * r + 1][q] = v.y;
            }
        double A[4][3];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int l = 0; l < 3; ++l)
                A[s][l] = (m[s][0] * k.rinv[l] + m[s][1] * k.rinv[3 + l]) + m[s][2] * k.rinv[6 + l];
        double Nm[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = a; b < 3; ++b)
                Nm[a][b] = Nm[b][a] = ((A[0][a] * A[0][b] + A[1][a] * A[1][b]) + A[2][a] * A[2][b]) + A[3][a] * A[3][b];
        double C[3][3];
        C[0][0] = Nm[1][1] * Nm[2][2] - Nm[1][2] * Nm[1][2];
        C[0][1] = Nm[0][2] * Nm[1][2] - Nm[0][1] * Nm[2][2];
        C[0][2] = Nm[0][1] * Nm[1][2] - Nm[0][2] * Nm[1][1];
        C[1][1] = Nm[0][0] * Nm[2][2] - Nm[0][2] * Nm[0][2];
        C[1][2] = Nm[0][1] * Nm[0][2] - Nm[0][0] * Nm[1][2];
        C[2][2] = Nm[0][0] * Nm[1][1] - Nm[0][1] * Nm[0][1];
        C[1][0] = C[0][1], C[2][0] = C[0][2], C[2][1] = C[1][2];
        const double det = (Nm[0][0] * C[0][0] + Nm[0][1] * C[0][1]) + Nm[0][2] * C[0][2];
        const double q = det / ((Nm[0][0] * Nm[1][1]) * Nm[2][2]);
        const bool good = q >= k.qmin;                         // false for NaN
        double V[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) V[a][b] = C[a][b] / det;
        double P[3][4];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int s = 0; s < 4; ++s) P[a][s] = (V[a][0] * A[s][0] + V[a][1] * A[s][1]) + V[a][2] * A[s][2];
        float* g = gain + 16L * c;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float o[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const double v = (k.a_nom[3 * t] * P[0][s] + k.a_nom[3 * t + 1] * P[1][s]) + k.a_nom[3 * t + 2] * P[2][s];
                o[s] = good ? (float)v : (s == t ? 1.0f : 0.0f);
            }
            store_floats<4>(g + 4 * t, o);
        }
        if (quality) quality[c] = good ? (float)q : 0.0f;
    }
}

// ---------------------------------------------------------------------------------------------------- apply, CELL
// A lane owns NC adjacent cells of one cell row: columns 2 NC cx .. 2 NC cx + 2 NC - 1 of rows 2i, 2i + 1.  NC = 2 needs
// W2 % 4 == 0 (every piece starts on a multiple of 4 elements), NC = 1 serves W2 % 4 == 2.
template <typename T, int NC>
__global__ __launch_bounds__(kThreads) void dofp_calibrate_cell_kernel(const T* __restrict__ mosaic, const float* __restrict__ dark,
                                                                       const float* __restrict__ gain, float* __restrict__ out,
                                                                       int B, int h, int w) {
    constexpr int K = 2 * NC;
    const int chunks = w / NC;
    const int items = h * chunks;                              // <= 2^28
    const int W2 = 2 * w;
    const long plane = 4L * h * w;
    for (int it = blockIdx.x * kThreads + threadIdx.x; it < items; it += gridDim.x * kThreads) {
        const int i = it / chunks, cx = it - i * chunks;
        const int off = (2 * i) * W2 + K * cx;                 // < H2 * W2 <= 2^30
        f32x4 G[NC][4];                                        // widened to fp64 where used (the compiler hoists it: ~112 VGPRs at NC = 2)
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int t = 0; t < 4; ++t) G[c][t] = *reinterpret_cast<const f32x4*>(gain + 16L * ((long)i * w + NC * cx + c) + 4 * t);
        double d[2][K];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
#pragma unroll
            for (int j = 0; j < K; ++j) d[r][j] = 0.0;
            if (dark) load_as_double<float, K>(dark + off + r * W2, d[r]);
        }
        for (int b = 0; b < B; ++b) {
            const T* src = mosaic + b * plane + off;
            double e[2][K];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                load_as_double<T, K>(src + r * W2, e[r]);
                if (dark) {
#pragma unroll
                    for (int j = 0; j < K; ++j) e[r][j] = e[r][j] - d[r][j];
                }
            }
            float* dst = out + b * plane + off;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                float o[K];
#pragma unroll
                for (int c = 0; c < NC; ++c)
#pragma unroll
                    for (int x = 0; x < 2; ++x) {
                        const f32x4 g = G[c][2 * r + x];
                        o[2 * c + x] = (float)((((double)g.x * e[0][2 * c] + (double)g.y * e[0][2 * c + 1]) +
                                                (double)g.z * e[1][2 * c]) + (double)g.w * e[1][2 * c + 1]);
                    }
                store_floats<K>(dst + r * W2, o);
            }
        }
    }
}

// --------------------------------------------------------------------------------------------------- apply, PIXEL
// out[b][i] = fp32((double)g[i] * ((double)m[b][i] - (double)dark[i])); a lane owns 4 consecutive pixels of the flat frame.
template <typename T>
__global__ __launch_bounds__(kThreads) void dofp_calibrate_pixel_kernel(const T* __restrict__ mosaic, const float* __restrict__ dark,
                                                                        const float* __restrict__ gain, float* __restrict__ out,
                                                                        int B, int groups) {
    const long plane = 4L * groups;
    for (int g = blockIdx.x * kThreads + threadIdx.x; g < groups; g += gridDim.x * kThreads) {
        const int i = 4 * g;                                   // < H2 * W2 <= 2^30
        double gn[4], d[4] = {0.0, 0.0, 0.0, 0.0};
        load_as_double<float, 4>(gain + i, gn);
        if (dark) load_as_double<float, 4>(dark + i, d);
        for (int b = 0; b < B; ++b) {
            double e[4];
            load_as_double<T, 4>(mosaic + b * plane + i, e);
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (float)(gn[j] * (dark ? e[j] - d[j] : e[j]));
            store_floats<4>(out + b * plane + i, o);
        }
    }
}

template <typename T>
void launch_moments(const void* frames, const void* dark, const double* weights, double* out, int N, int Q, int groups,
                    int accumulate, hipStream_t st) {
    const dim3 grid(grid_for(groups)), block(kThreads);
#define PD_MOMENTS(QQ) \
    hipLaunchKernelGGL((frame_moments_kernel<T, QQ>), grid, block, 0, st, (const T*)frames, (const float*)dark, weights, out, N, \
                       groups, accumulate)
    if (Q == 1) PD_MOMENTS(1);
    else if (Q == 2) PD_MOMENTS(2);
    else if (Q == 3) PD_MOMENTS(3);
    else PD_MOMENTS(4);
#undef PD_MOMENTS
}

template <typename T>
void launch_calibrate(const void* mosaic, const void* dark, const void* gain, int gain_kind, void* out, int B, int H2, int W2,
                      hipStream_t st) {
    const int h = H2 / 2, w = W2 / 2;
    const dim3 block(kThreads);
    if (gain_kind == PD_DOFP_CAL_PIXEL)
        hipLaunchKernelGGL((dofp_calibrate_pixel_kernel<T>), dim3(grid_for((long)h * w)), block, 0, st, (const T*)mosaic,
                           (const float*)dark, (const float*)gain, (float*)out, B, h * w);
    else if (w % 2 == 0)
        hipLaunchKernelGGL((dofp_calibrate_cell_kernel<T, 2>), dim3(grid_for((long)h * (w / 2))), block, 0, st, (const T*)mosaic,
                           (const float*)dark, (const float*)gain, (float*)out, B, h, w);
    else
        hipLaunchKernelGGL((dofp_calibrate_cell_kernel<T, 1>), dim3(grid_for((long)h * w)), block, 0, st, (const T*)mosaic,
                           (const float*)dark, (const float*)gain, (float*)out, B, h, w);
}

}  // namespace

#define PD_CAL_DTYPE(fn) \
    PD_REQUIRE(dtype == PD_POLAR_U8 || dtype == PD_POLAR_U16 || dtype == PD_POLAR_F32, \
               fn ": unknown dtype %d (PD_POLAR_U8 / _U16 / _F32)", dtype)
#define PD_CAL_SIDES(fn) \
    PD_REQUIRE(H2 >= 2 && W2 >= 2 && H2 % 2 == 0 && W2 % 2 == 0, fn ": the frame must have even sides >= 2, got %d x %d", H2, W2)

extern "C" int pd_frame_moments(const void* frames, int dtype, const void* dark, const double* weights, double* out, int N,
                                int Q, int H2, int W2, int accumulate, void* stream) {
    PD_CAL_DTYPE("pd_frame_moments");
    PD_REQUIRE(N >= 1, "pd_frame_moments: needs at least one frame (N = %d)", N);
    PD_REQUIRE(Q >= 1 && Q <= 4, "pd_frame_moments: Q = %d is outside 1..4", Q);
    PD_REQUIRE(frames && weights && out, "pd_frame_moments: frames, weights and out must not be null");
    PD_CAL_SIDES("pd_frame_moments");
    // in-frame offsets are 32-bit in the kernel, frame offsets 64-bit
    PD_REQUIRE((long)H2 * W2 <= (1L << 30) && (long)N * H2 * W2 <= (1L << 40),
               "pd_frame_moments: %d frames of %d x %d are too large for the kernel's index arithmetic", N, H2, W2);
    PD_REQUIRE(pd::aligned16(frames) && pd::aligned16(dark) && pd::aligned16(out),
               "pd_frame_moments: frames, dark and out must be 16-byte aligned");
    PD_REQUIRE(pd::aligned8(weights), "pd_frame_moments: weights must be 8-byte aligned");
    const int groups = (H2 / 2) * (W2 / 2);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == PD_POLAR_U8) launch_moments<uint8_t>(frames, dark, weights, out, N, Q, groups, accumulate != 0, st);
    else if (dtype == PD_POLAR_U16) launch_moments<uint16_t>(frames, dark, weights, out, N, Q, groups, accumulate != 0, st);
    else launch_moments<float>(frames, dark, weights, out, N, Q, groups, accumulate != 0, st);
    return pd::check_launch("pd_frame_moments");
}

extern "C" int pd_dofp_cal_solve(const double* moments, const double* rinv, const double* a_nom, double qmin, float* gain,
                                 float* quality, int H2, int W2, void* stream) {
    PD_REQUIRE(moments && rinv && a_nom && gain, "pd_dofp_cal_solve: moments, rinv, a_nom and gain must not be null");
    SolveArgs k;
    for (int i = 0; i < 9; ++i) {
        PD_REQUIRE(std::isfinite(rinv[i]), "pd_dofp_cal_solve: rinv[%d] = %g is not finite", i, rinv[i]);
        k.rinv[i] = rinv[i];
    }
    for (int i = 0; i < 12; ++i) {
        PD_REQUIRE(std::isfinite(a_nom[i]), "pd_dofp_cal_solve: a_nom[%d] = %g is not finite", i, a_nom[i]);
        k.a_nom[i] = a_nom[i];
    }
    PD_REQUIRE(std::isfinite(qmin), "pd_dofp_cal_solve: qmin = %g is not finite", qmin);
    k.qmin = qmin;
    PD_CAL_SIDES("pd_dofp_cal_solve");
    PD_REQUIRE((long)H2 * W2 <= (1L << 30), "pd_dofp_cal_solve: a frame of %d x %d is too large for the kernel's index arithmetic",
               H2, W2);
    PD_REQUIRE(pd::aligned16(moments) && pd::aligned16(gain) && pd::aligned4(quality),
               "pd_dofp_cal_solve: moments and gain must be 16-byte aligned (quality: 4-byte)");
    hipLaunchKernelGGL(dofp_cal_solve_kernel, dim3(grid_for((long)(H2 / 2) * (W2 / 2))), dim3(kThreads), 0, (hipStream_t)stream,
                       moments, gain, quality, k, H2 / 2, W2 / 2);
    return pd::check_launch("pd_dofp_cal_solve");
}

extern "C" int pd_dofp_calibrate(const void* mosaic, int dtype, const void* dark, const void* gain, int gain_kind, void* out,
                                 int B, int H2, int W2, void* stream) {
    if (B == 0) return PD_OK;
    PD_REQUIRE(B > 0, "pd_dofp_calibrate: bad shape (B = %d)", B);
    PD_CAL_DTYPE("pd_dofp_calibrate");
    PD_REQUIRE(gain_kind == PD_DOFP_CAL_CELL || gain_kind == PD_DOFP_CAL_PIXEL,
               "pd_dofp_calibrate: unknown gain_kind %d (PD_DOFP_CAL_CELL / PD_DOFP_CAL_PIXEL)", gain_kind);
    PD_REQUIRE(mosaic && gain && out, "pd_dofp_calibrate: mosaic, gain and out must not be null");
    PD_CAL_SIDES("pd_dofp_calibrate");
    PD_REQUIRE((long)H2 * W2 <= (1L << 30) && (long)B * H2 * W2 <= (1L << 40),
               "pd_dofp_calibrate: %d frames of %d x %d are too large for the kernel's index arithmetic", B, H2, W2);
    PD_REQUIRE(pd::aligned16(mosaic) && pd::aligned16(dark) && pd::aligned16(gain) && pd::aligned16(out),
               "pd_dofp_calibrate: mosaic, dark, gain and out must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == PD_POLAR_U8) launch_calibrate<uint8_t>(mosaic, dark, gain, gain_kind, out, B, H2, W2, st);
    else if (dtype == PD_POLAR_U16) launch_calibrate<uint16_t>(mosaic, dark, gain, gain_kind, out, B, H2, W2, st);
    else launch_calibrate<float>(mosaic, dark, gain, gain_kind, out, B, H2, W2, st);
    return pd::check_launch("pd_dofp_calibrate");
}
