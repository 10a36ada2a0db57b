// The cost-volume student's training step (the reference's --train_student branch): the consistency masks from the plane
// sweep's lowest-cost and confidence maps, the adaptive depth-bin tracker, and the masked reprojection / consistency loss.
//
// Reference restated (include/polardepth.h states every definition):
//   trainer.py:617-627     F.interpolate(mode="nearest") of lowest_cost / confidence_mask to full resolution
//   trainer.py:1112-1124   compute_matching_mask against the teacher's depth
//   trainer.py:650-664     update_adaptive_depth_bins;  resnet_encoder.py:406-420  compute_depth_bins
//   trainer.py:1202-1236   the is_multi branch of compute_losses
//
// All of these are streaming kernels bound by memory: a thread handles four pixels that are neighbours in x, so fp32 maps
// move as 16-byte and byte masks as 4-byte accesses, coalesced over the wavefront.  The four pixels of pd_student_masks
// share one quarter-resolution source (W = 4w).  No atomics, no host synchronisation; every launch can be captured.
// The file is built with -ffp-contract=off (csrc/Makefile): no product is fused into a sum.
#include "pd_common.h"
#include "frame_reduce.hpp"

namespace {

using pd_frames::FrameArgs;
using pd_frames::OverFrames;
using pd_wave::wave_max;
using pd_wave::wave_min;
using pd_wave::wave_or;
constexpr int RT = pd_frames::RT;

// ------------------------------------------------------------------ pd_student_masks
// minimum / maximum that ignore NaN (fminf / fmaxf) plus a flag: the pair becomes NaN at the end if the flag is set
struct MinMax {
    float mn = __builtin_inff(), mx = -__builtin_inff();
    int nan = 0;
    __device__ __forceinline__ void add(float v) {
        nan |= (v != v);
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    __device__ __forceinline__ void merge(float omn, float omx) {
        nan |= (omn != omn);
        mn = fminf(mn, omn);
        mx = fmaxf(mx, omx);
    }
    // over the workgroup (RT = 256: four wavefronts); the result is valid in thread 0.  sm: 12 floats of LDS
    __device__ __forceinline__ void block_reduce(float* sm) {
        mn = wave_min(mn);
        mx = wave_max(mx);
        nan = wave_or(nan);
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) { sm[wave * 3] = mn; sm[wave * 3 + 1] = mx; sm[wave * 3 + 2] = nan ? 1.f : 0.f; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int k = 1; k < RT / 64; ++k) {
                mn = fminf(mn, sm[k * 3]);
                mx = fmaxf(mx, sm[k * 3 + 1]);
                nan |= (sm[k * 3 + 2] != 0.f);
            }
        }
    }
    __device__ __forceinline__ void store(float* out) const {
        const float q = __builtin_nanf("");
        out[0] = nan ? q : mn;
        out[1] = nan ? q : mx;
    }
};

// blockIdx.y = item, thread = four pixels (4 qx .. 4 qx + 3) of row y: one source pixel (y >> 2, qx)
__global__ __launch_bounds__(RT) void masks_kernel(const float* __restrict__ lowest, const float* __restrict__ confidence,
                                                   const float* __restrict__ mono, const float* __restrict__ aug,
                                                   int motion_masking, unsigned char* __restrict__ rmask,
                                                   float* __restrict__ cmask, float* __restrict__ lowest_up,
                                                   float* __restrict__ partial, int h, int w) {
    __shared__ float sm[12];
    const long n = blockIdx.y;
    const int H = 4 * h;
    const int quads = H * w;                      // <= 2^28
    const bool augmented = aug && aug[n] != 0.f;
    const float* lo = lowest + n * (long)h * w;
    const float* cf = confidence + n * (long)h * w;
    const long base = n * (long)quads;            // in quads
    MinMax mm;
    for (int q = blockIdx.x * RT + threadIdx.x; q < quads; q += gridDim.x * RT) {
        const int y = q / w, qx = q - y * w;
        const int s = (y >> 2) * w + qx;
        const float l = lo[s];
        const bool conf = cf[s] != 0.f;
        const float4 t4 = reinterpret_cast<const float4*>(mono)[base + q];
        const float t[4] = {t4.x, t4.y, t4.z, t4.w};
        const float md = 1.0f / l;
        float c[4];
        unsigned char r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            mm.add(t[k]);
            const bool match = ((md - t[k]) / t[k] < 1.0f) && ((t[k] - md) / md < 1.0f);
            const bool cm = conf && (!motion_masking || match);
            c[k] = cm ? 1.f : 0.f;
            r[k] = ((!motion_masking || cm) && !augmented) ? 1 : 0;
        }
        reinterpret_cast<uchar4*>(rmask)[base + q] = make_uchar4(r[0], r[1], r[2], r[3]);
        if (cmask) reinterpret_cast<float4*>(cmask)[base + q] = make_float4(c[0], c[1], c[2], c[3]);
        if (lowest_up) reinterpret_cast<float4*>(lowest_up)[base + q] = make_float4(l, l, l, l);
    }
    mm.block_reduce(sm);
    if (threadIdx.x == 0) mm.store(partial + (n * gridDim.x + blockIdx.x) * 2);
}

// one workgroup per item over its `rows` partial pairs
__global__ __launch_bounds__(RT) void minmax_finalize_kernel(const float* __restrict__ partial, int rows,
                                                             float* __restrict__ minmax) {
    __shared__ float sm[12];
    const long n = blockIdx.x;
    MinMax mm;
    for (int r = threadIdx.x; r < rows; r += RT) mm.merge(partial[(n * rows + r) * 2], partial[(n * rows + r) * 2 + 1]);
    mm.block_reduce(sm);
    if (threadIdx.x == 0) mm.store(minmax + n * 2);
}


// ------------------------------------------------------------------ pd_depth_bins_update
__global__ __launch_bounds__(128) void bins_update_kernel(const float* __restrict__ minmax, int N, double* __restrict__ tracker,
                                                          double floor_depth, int D, int inverse, float* __restrict__ bins) {
    __shared__ double tr[2];
    if (threadIdx.x == 0) {
        float smn = 0.f, smx = 0.f;
        for (int n = 0; n < N; ++n) { smn += minmax[2 * n]; smx += minmax[2 * n + 1]; }
        const double mn = (double)(smn / (float)N), mx = (double)(smx / (float)N);
        const double lo = mn * 0.9;
        const double mn64 = lo > floor_depth ? lo : floor_depth;     // Python's max(floor, lo): floor unless lo is greater
        const double mx64 = mx * 1.1;
        const double tmin = tracker[0] * 0.99 + mn64 * 0.01;
        const double tmax = tracker[1] * 0.99 + mx64 * 0.01;
        tracker[0] = tmin;
        tracker[1] = tmax;
        tr[0] = tmin;
        tr[1] = tmax;
    }
    __syncthreads();
    const double start = inverse ? 1.0 / tr[1] : tr[0];
    const double stop = inverse ? 1.0 / tr[0] : tr[1];
    const double delta = stop - start;
    const int div = D - 1;
    const double step = div > 0 ? delta / (double)div : 0.0;
    for (int i = threadIdx.x; i < D; i += 128) {
        const int j = inverse ? D - 1 - i : i;       // element of the linspace
        double y;
        if (div <= 0) y = (double)j * delta;                          // numpy: one sample, y = arange * delta
        else if (step == 0.0) y = ((double)j / (double)div) * delta;  // numpy's denormal branch
        else y = (double)j * step;
        y = y + start;
        if (div > 0 && j == div) y = stop;
        bins[i] = (float)(inverse ? 1.0 / y : y);
    }
}

// ------------------------------------------------------------------ pd_student_combine_*
// thread = four pixels; quads never straddle two items (H * W is a multiple of 4)
__global__ __launch_bounds__(RT) void student_combine_fwd_kernel(const FrameArgs a, int F, const float* __restrict__ valid,
                                                                 const unsigned char* __restrict__ rmask,
                                                                 const float* __restrict__ multi, const float* __restrict__ mono,
                                                                 unsigned char* __restrict__ sel, double* __restrict__ partial,
                                                                 long quads, int qper, int avg) {
    __shared__ double sm[4 * 3];
    double acc[3] = {0.0, 0.0, 0.0};
    for (long q = blockIdx.x * (long)RT + threadIdx.x; q < quads; q += (long)gridDim.x * RT) {
        const long n = q / qper;
        const float* vrow = valid ? valid + n * F : nullptr;
        OverFrames o[4];
        for (int f = 0; f < F; ++f) {
            if (vrow && vrow[f] == 0.f) continue;
            const float4 r4 = reinterpret_cast<const float4*>(a.reproj[f])[q];
            o[0].add(r4.x, f, avg);
            o[1].add(r4.y, f, avg);
            o[2].add(r4.z, f, avg);
            o[3].add(r4.w, f, avg);
        }
        const uchar4 k4 = reinterpret_cast<const uchar4*>(rmask)[q];
        const float4 d4 = reinterpret_cast<const float4*>(multi)[q];
        const float4 t4 = reinterpret_cast<const float4*>(mono)[q];
        const unsigned char kk[4] = {k4.x, k4.y, k4.z, k4.w};
        const float dd[4] = {d4.x, d4.y, d4.z, d4.w}, tt[4] = {t4.x, t4.y, t4.z, t4.w};
        unsigned char s[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[k].finish(avg);
            const bool keep = o[k].nvalid > 0 && kk[k] != 0;
            const float r = keep ? 1.f : 0.f;
            s[k] = keep ? (unsigned char)o[k].arg : (unsigned char)255;
            acc[0] += (double)(o[k].m * r);
            acc[1] += (double)r;
            acc[2] += (double)(fabsf(dd[k] - tt[k]) * (1.f - r));
        }
        reinterpret_cast<uchar4*>(sel)[q] = make_uchar4(s[0], s[1], s[2], s[3]);
    }
    pd_frames::block_rows<3>(acc, sm, partial);
}

__global__ __launch_bounds__(256) void student_combine_finalize_kernel(const double* __restrict__ partial, int rows,
                                                                       double count, double* __restrict__ sums,
                                                                       float* __restrict__ loss) {
    __shared__ double sm[3 * 256];
    double s[3];
    pd_frames::finalize_rows<3>(partial, rows, sm, s);
    if (threadIdx.x == 0) {
        sums[0] = s[0];
        sums[1] = s[1];
        sums[2] = s[2];
        loss[0] = (float)(s[0] / (s[1] + 1e-7));
        loss[1] = (float)(s[2] / count);
    }
}

__global__ __launch_bounds__(RT) void student_combine_bwd_kernel(const FrameArgs a, int F, const float* __restrict__ gloss,
                                                                 const unsigned char* __restrict__ sel,
                                                                 const double* __restrict__ sums, const float* __restrict__ valid,
                                                                 const float* __restrict__ multi, const float* __restrict__ mono,
                                                                 float* __restrict__ gmulti, long quads, int qper, double count,
                                                                 int avg) {
    const float g = (float)((double)gloss[0] / (sums[1] + 1e-7));
    const float gc = (float)((double)gloss[1] / count);
    for (long q = blockIdx.x * (long)RT + threadIdx.x; q < quads; q += (long)gridDim.x * RT) {
        const uchar4 s4 = reinterpret_cast<const uchar4*>(sel)[q];
        const int s[4] = {s4.x, s4.y, s4.z, s4.w};
        const float* vrow = valid ? valid + (q / qper) * F : nullptr;
        int nv = 0;
        for (int f = 0; f < F; ++f) nv += !(vrow && vrow[f] == 0.f);
        for (int f = 0; f < F; ++f) {
            float o[4];
            const bool fvalid = !(vrow && vrow[f] == 0.f);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!avg) o[k] = (s[k] == f) ? g : 0.f;
                else o[k] = (fvalid && s[k] != 255 && nv) ? g / (float)nv : 0.f;
            }
            reinterpret_cast<float4*>(a.greproj[f])[q] = make_float4(o[0], o[1], o[2], o[3]);
        }
        const float4 d4 = reinterpret_cast<const float4*>(multi)[q];
        const float4 t4 = reinterpret_cast<const float4*>(mono)[q];
        const float dd[4] = {d4.x, d4.y, d4.z, d4.w}, tt[4] = {t4.x, t4.y, t4.z, t4.w};
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d = dd[k] - tt[k];
            const float sg = (float)(d > 0.f) - (float)(d < 0.f);       // sign(0) = sign(NaN) = 0, as torch.sign
            o[k] = (gc * sg) * (s[k] == 255 ? 1.f : 0.f);
        }
        reinterpret_cast<float4*>(gmulti)[q] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

using pd::aligned4;
using pd::aligned8;

}  // namespace

// ============================================================================ C ABI
// workgroups per item of masks_kernel: one thread per quad, 4 h w quads per item
extern "C" int pd_student_masks_rows(int N, int h, int w) { return h <= 0 || w <= 0 ? 1 : (int)pd::item_grid(N, 4L * h * w); }

extern "C" int pd_student_masks(const void* lowest, const void* confidence, const void* mono_depth, const void* aug,
                                int motion_masking, void* rmask, void* cmask, void* lowest_up, void* minmax, void* partial_ws,
                                int N, int h, int w, int H, int W, void* stream) {
    PD_REQUIRE(lowest && confidence && mono_depth && rmask && minmax && partial_ws,
               "pd_student_masks: lowest, confidence, mono_depth, rmask, minmax and partial_ws must not be null");
    PD_REQUIRE(N >= 0 && N <= 65535 && h > 0 && w > 0, "pd_student_masks: bad shape N=%d h=%d w=%d (0 <= N <= 65535)", N, h, w);
    PD_REQUIRE((long)h * w <= (1L << 26), "pd_student_masks: image too large (%d x %d at 1/4 resolution)", h, w);
    PD_REQUIRE(H == 4 * h && W == 4 * w, "pd_student_masks: H = 4h and W = 4w required, got %d x %d for %d x %d", H, W, h, w);
    PD_REQUIRE(motion_masking == 0 || motion_masking == 1, "pd_student_masks: motion_masking must be 0 or 1, got %d", motion_masking);
    PD_REQUIRE(pd::aligned16(mono_depth) && pd::aligned16(cmask) && pd::aligned16(lowest_up) && aligned4(rmask),
               "pd_student_masks: mono_depth, cmask and lowest_up must be 16-byte aligned, rmask 4-byte");
    if (N == 0) return PD_OK;
    const int rows = pd_student_masks_rows(N, h, w);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(masks_kernel, dim3(rows, N), dim3(RT), 0, st, (const float*)lowest, (const float*)confidence,
                       (const float*)mono_depth, (const float*)aug, motion_masking, (unsigned char*)rmask, (float*)cmask,
                       (float*)lowest_up, (float*)partial_ws, h, w);
    hipLaunchKernelGGL(minmax_finalize_kernel, dim3(N), dim3(RT), 0, st, (const float*)partial_ws, rows, (float*)minmax);
    return pd::check_launch("pd_student_masks");
}

extern "C" int pd_depth_bins_update(const void* minmax, int N, void* tracker, double floor_depth, int D, int binning,
                                    void* bins, void* stream) {
    PD_REQUIRE(minmax && tracker && bins, "pd_depth_bins_update: minmax, tracker and bins must not be null");
    PD_REQUIRE(N >= 1 && N <= 65535, "pd_depth_bins_update: 1 <= N <= 65535 items, got %d", N);
    PD_REQUIRE(D >= 1 && D <= 128, "pd_depth_bins_update: 1 <= D <= 128 depth bins, got %d", D);
    PD_REQUIRE(binning == PD_BINS_LINEAR || binning == PD_BINS_INVERSE, "pd_depth_bins_update: binning must be 0 (linear) or 1 (inverse), got %d", binning);
    PD_REQUIRE(aligned8(tracker), "pd_depth_bins_update: tracker must be 8-byte aligned");
    hipLaunchKernelGGL(bins_update_kernel, dim3(1), dim3(128), 0, (hipStream_t)stream, (const float*)minmax, N, (double*)tracker,
                       floor_depth, D, binning, (float*)bins);
    return pd::check_launch("pd_depth_bins_update");
}

extern "C" int pd_student_combine_rows(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 1;
    return (int)pd::flat_grid((long)N * H * W / 4);
}

// a thread handles a quad, four pixels that are neighbours in x
static const char* const kQuads = "%s: H and W must be multiples of 4 (the masks are 4x a quarter-resolution map), got %d x %d";

extern "C" int pd_student_combine_fwd(const void* const* reproj, int F, const void* valid, const void* rmask,
                                      const void* multi_depth, const void* mono_depth, void* sel, void* partial_ws, void* sums,
                                      void* loss, int N, int H, int W, int avg, void* stream) {
    if (int rc = pd_frames::combine_args("pd_student_combine_fwd", F, N, H, W, avg)) return rc;
    PD_REQUIRE(H % 4 == 0 && W % 4 == 0, kQuads, "pd_student_combine_fwd", H, W);
    PD_REQUIRE(reproj && rmask && multi_depth && mono_depth && sel && partial_ws && sums && loss,
               "pd_student_combine_fwd: reproj, rmask, multi_depth, mono_depth, sel, partial_ws, sums and loss must not be null");
    PD_REQUIRE(aligned8(partial_ws) && aligned8(sums), "pd_student_combine_fwd: partial_ws and sums must be 8-byte aligned");
    PD_REQUIRE(pd::aligned16(multi_depth) && pd::aligned16(mono_depth) && aligned4(rmask) && aligned4(sel),
               "pd_student_combine_fwd: multi_depth and mono_depth must be 16-byte aligned, rmask and sel 4-byte");
    FrameArgs a = {};
    for (int f = 0; f < F; ++f) {
        PD_REQUIRE(reproj[f] && pd::aligned16(reproj[f]), "pd_student_combine_fwd: map %d is null or not 16-byte aligned", f);
        a.reproj[f] = (const float*)reproj[f];
    }
    if (N == 0) return PD_OK;
    const int qper = H * W / 4;
    const long quads = (long)N * qper;
    const int grid = pd_student_combine_rows(N, H, W);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(student_combine_fwd_kernel, dim3(grid), dim3(RT), 0, st, a, F, (const float*)valid,
                       (const unsigned char*)rmask, (const float*)multi_depth, (const float*)mono_depth, (unsigned char*)sel,
                       (double*)partial_ws, quads, qper, avg);
    hipLaunchKernelGGL(student_combine_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)partial_ws, grid,
                       (double)N * (double)H * (double)W, (double*)sums, (float*)loss);
    return pd::check_launch("pd_student_combine_fwd");
}

extern "C" int pd_student_combine_bwd(const void* gloss, const void* sel, const void* sums, const void* valid,
                                      const void* multi_depth, const void* mono_depth, void* const* greproj, void* gmulti, int F,
                                      int N, int H, int W, int avg, void* stream) {
    if (int rc = pd_frames::combine_args("pd_student_combine_bwd", F, N, H, W, avg)) return rc;
    PD_REQUIRE(H % 4 == 0 && W % 4 == 0, kQuads, "pd_student_combine_bwd", H, W);
    PD_REQUIRE(gloss && sel && sums && multi_depth && mono_depth && greproj && gmulti,
               "pd_student_combine_bwd: gloss, sel, sums, multi_depth, mono_depth, greproj and gmulti must not be null");
    PD_REQUIRE(aligned8(sums), "pd_student_combine_bwd: sums must be 8-byte aligned");
    PD_REQUIRE(pd::aligned16(multi_depth) && pd::aligned16(mono_depth) && pd::aligned16(gmulti) && aligned4(sel),
               "pd_student_combine_bwd: multi_depth, mono_depth and gmulti must be 16-byte aligned, sel 4-byte");
    FrameArgs a = {};
    for (int f = 0; f < F; ++f) {
        PD_REQUIRE(greproj[f] && pd::aligned16(greproj[f]), "pd_student_combine_bwd: map %d is null or not 16-byte aligned", f);
        a.greproj[f] = (float*)greproj[f];
    }
    if (N == 0) return PD_OK;
    const int qper = H * W / 4;
    const long quads = (long)N * qper;
    hipLaunchKernelGGL(student_combine_bwd_kernel, dim3(pd::flat_grid(quads)), dim3(RT), 0, (hipStream_t)stream, a, F,
                       (const float*)gloss, (const unsigned char*)sel, (const double*)sums, (const float*)valid,
                       (const float*)multi_depth, (const float*)mono_depth, (float*)gmulti, quads, qper,
                       (double)N * (double)H * (double)W, avg);
    return pd::check_launch("pd_student_combine_bwd");
}
