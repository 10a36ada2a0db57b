// DoLP / AoLP statistics of an XOLP tensor on the device: moments, extrema, histograms and out-of-table counts in one read
// pass (what the reference's polarisation/xolp_mean_and_std_dev.py computes with NumPy for 46 HAMMER frames, plus what
// tells a wrong sensor description from a right one).  Definition and record layout: include/polardepth.h, pd_xolp_stats.
//
// A pure read stream of 8 B/px (9 with a mask).  Two launches:
//   xolp_stats_kernel           one work item = one quad (4 consecutive columns of one row, both channels: two 16-byte
//                               loads, one 4-byte mask load), grid-stride with the next item's loads issued before the
//                               current one is processed.  Per lane: fp64 running sums, integer counters, extrema.  Per
//                               workgroup: one LDS histogram (513 x uint32).  Everything a workgroup found leaves as ONE
//                               partial record in the workspace, written with plain stores: no global atomics.
//   xolp_stats_finalize_kernel  sums the partial records in index order (fp64 for the four sums), folds them into `stats`.
// The fp64 sums are bit-reproducible: the item -> lane assignment depends on the shape only, a lane adds its items in order,
// a wave its lanes by a fixed shuffle tree, a workgroup its waves in order, the finalize kernel the workgroups in order.
//
// Histogram scheme -- aggregate equal bins before the atomic.  Real DoLP / AoLP maps are smooth: the 256 pixels a wave
// holds fall into a handful of bins, and 64 lanes adding 1 to one LDS word serialise.  So a lane whose four pixels share a
// bin is "flat", consecutive flat lanes with one bin form a run (one packed shuffle of the previous lane's bins, one ballot
// per channel), and only the first lane of a run adds, 4 x the run length at once.  Lanes that are not flat (a bin edge,
// a masked or non-finite pixel, the partial last quad of a row) add their pixels one by one.  On i.i.d. data nearly every
// lane takes the second path and the adds spread over the banks; on smooth data a wave issues a few adds per channel.
#include "pd_common.h"

#include <cmath>

namespace {

constexpr int kThreads = 1024;            // 16 waves: one histogram per workgroup serves four waves per SIMD
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 256;           // one workgroup per CU; the finalize kernel reads at most 256 partial records
constexpr long kQuadsPerBlock = 4L * kThreads;   // below the cap a lane gets about four quads: the grid-stride loop always runs
constexpr int kBinsRho = 257, kBinsPhi = 256, kBins = kBinsRho + kBinsPhi;
constexpr size_t kPartialBytes = 4 * 8 + 4 * 8 + 4 * 4 + (size_t)kBins * 4;      // sums, counters, extrema, histogram
constexpr size_t kStatsHist = 80;         // byte offset of the histograms in the record (header)
constexpr int kHistBlocks = (kBins + 63) / 64;

constexpr double kPi = 3.14159265358979323846;
constexpr float kC1 = (float)(kPi / 2.0);
constexpr float kC2 = (float)(256.0 / kPi);

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Geo {
    unsigned total;       // quads of this launch
    unsigned Q, H, W, ld; // quads per row that hold data, rows, data columns, row pitch
    unsigned dq, dy, db;  // one grid stride as (frames, rows, quads)
};

struct Item {
    f32x4 r, p;
    uint32_t m;
};

__device__ __forceinline__ void load_item(Item& it, const float* __restrict__ xolp, const uint8_t* __restrict__ mask,
                                          const Geo& g, unsigned b, unsigned y, unsigned q) {
    const unsigned off = (2u * b * g.H + y) * g.ld + 4u * q;      // < 2^30: the host splits the batch
    it.r = *reinterpret_cast<const f32x4*>(xolp + off);
    it.p = *reinterpret_cast<const f32x4*>(xolp + off + g.H * g.ld);
    it.m = mask ? *reinterpret_cast<const uint32_t*>(mask + (b * g.H + y) * g.ld + 4u * q) : 0x01010101u;
}

__device__ __forceinline__ int bin_rho(float r) { return r < 0.0f ? 0 : (r >= 1.0f ? 256 : (int)(r * 256.0f)); }
__device__ __forceinline__ int bin_phi(float p) {
    const float t = (p + kC1) * kC2;
    return t < 0.0f ? 0 : (t >= 256.0f ? 255 : (int)t);
}

// one channel's four bins of a lane into the workgroup histogram (see the head of the file)
__device__ __forceinline__ void hist_add(unsigned* hist, const int (&k)[4], const bool (&v)[4], bool flat, bool head,
                                         int lane) {
    const unsigned long long heads = __ballot(head);
    if (flat) {
        if (head) {
            const unsigned long long rest = (heads >> lane) >> 1;      // the heads after this lane
            const int run = rest ? __ffsll((long long)rest) : 64 - lane;
            atomicAdd(&hist[k[0]], 4u * (unsigned)run);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (v[j]) atomicAdd(&hist[k[j]], 1u);
    }
}

__global__ __launch_bounds__(kThreads) void xolp_stats_kernel(const float* __restrict__ xolp, const uint8_t* __restrict__ mask,
                                                              unsigned char* __restrict__ ws, Geo g, float t0, float t1) {
    __shared__ unsigned hist[kBins];
    __shared__ double wsum[4][kWaves];
    __shared__ unsigned wcnt[4][kWaves];
    __shared__ float wext[4][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < kBins; i += kThreads) hist[i] = 0;
    __syncthreads();

    const unsigned step = gridDim.x * kThreads;
    unsigned item = blockIdx.x * kThreads + tid;
    unsigned wbase = item - lane;      // the wave's first item: the loop below is uniform over the wave (shuffle, ballot)
    unsigned b, y, q;
    {
        const unsigned row = item / g.Q;
        q = item - row * g.Q;
        b = row / g.H;
        y = row - b * g.H;
    }
    double s[4] = {0.0, 0.0, 0.0, 0.0};                    // sum rho, rho^2, phi, phi^2
    unsigned c[4] = {0, 0, 0, 0};                          // n, nonfinite, over[0], over[1]
    float e[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};      // min rho, max rho, min phi, max phi

    const Item none = {f32x4{0.0f, 0.0f, 0.0f, 0.0f}, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0u};      // what a lane without an item holds
    Item cur = none;
    bool act = item < g.total;
    if (act) load_item(cur, xolp, mask, g, b, y, q);
    while (wbase < g.total) {
        // the next item, one grid stride on: (b, y, q) advance with carries, no division in the loop
        unsigned nq = q + g.dq, ny = y + g.dy, nb = b + g.db;
        if (nq >= g.Q) { nq -= g.Q; ++ny; }
        if (ny >= g.H) { ny -= g.H; ++nb; }
        const unsigned nitem = item + step;
        const bool nact = nitem < g.total;
        Item nxt = none;
        if (nact) load_item(nxt, xolp, mask, g, nb, ny, nq);

        int kr[4], kp[4];
        bool v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float r = cur.r[j], p = cur.p[j];
            const bool pass = act && 4u * q + j < g.W && ((cur.m >> (8 * j)) & 0xffu) != 0;
            const bool fin = __builtin_isfinite(r) && __builtin_isfinite(p);
            v[j] = pass && fin;
            c[1] += pass && !fin;
            kr[j] = kp[j] = 0;
            if (v[j]) {                                    // finite values only: the float -> int conversions are defined
                kr[j] = bin_rho(r);
                kp[j] = bin_phi(p);
                const double dr = (double)r, dp = (double)p;
                s[0] += dr; s[1] += dr * dr;               // the square of a converted fp32 is exact in fp64
                s[2] += dp; s[3] += dp * dp;
                c[0] += 1; c[2] += r > t0; c[3] += r > t1;
                e[0] = fminf(e[0], r); e[1] = fmaxf(e[1], r);
                e[2] = fminf(e[2], p); e[3] = fmaxf(e[3], p);
            }
        }
        const bool all = v[0] && v[1] && v[2] && v[3];
        const bool flat_r = all && kr[0] == kr[1] && kr[1] == kr[2] && kr[2] == kr[3];
        const bool flat_p = all && kp[0] == kp[1] && kp[1] == kp[2] && kp[2] == kp[3];
        const int key = (flat_r ? kr[0] : 0x1ff) | ((flat_p ? kp[0] : 0x1ff) << 16);      // 0x1ff: no bin
        const int prev = __shfl_up(key, 1);
        hist_add(hist, kr, v, flat_r, !flat_r || lane == 0 || (prev & 0xffff) != kr[0], lane);
        hist_add(hist + kBinsRho, kp, v, flat_p, !flat_p || lane == 0 || (prev >> 16) != kp[0], lane);

        cur = nxt; act = nact; item = nitem; wbase += step;
        q = nq; y = ny; b = nb;
    }

    // lanes -> wave by a fixed tree, waves -> workgroup in order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s[k] += __shfl_down(s[k], off);
            c[k] += __shfl_down(c[k], off);
        }
        e[0] = fminf(e[0], __shfl_down(e[0], off)); e[1] = fmaxf(e[1], __shfl_down(e[1], off));
        e[2] = fminf(e[2], __shfl_down(e[2], off)); e[3] = fmaxf(e[3], __shfl_down(e[3], off));
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { wsum[k][wave] = s[k]; wcnt[k][wave] = c[k]; wext[k][wave] = e[k]; }
    }
    __syncthreads();

    // the workgroup's partial record: [4][G] fp64 sums | [4][G] int64 counters | [4][G] fp32 extrema | [G][513] uint32 bins
    const unsigned G = gridDim.x, blk = blockIdx.x;
    if (tid < 4) {
        double t = 0.0;
        for (int w = 0; w < kWaves; ++w) t += wsum[tid][w];
        reinterpret_cast<double*>(ws)[tid * G + blk] = t;
    } else if (tid < 8) {
        long long t = 0;
        for (int w = 0; w < kWaves; ++w) t += wcnt[tid - 4][w];
        reinterpret_cast<long long*>(ws + 32 * (size_t)G)[(tid - 4) * G + blk] = t;
    } else if (tid < 12) {
        const int k = tid - 8;
        float t = wext[k][0];
        for (int w = 1; w < kWaves; ++w) t = (k & 1) ? fmaxf(t, wext[k][w]) : fminf(t, wext[k][w]);
        reinterpret_cast<float*>(ws + 64 * (size_t)G)[k * G + blk] = t;
    }
    if (tid < kBins) reinterpret_cast<unsigned*>(ws + 80 * (size_t)G)[blk * kBins + tid] = hist[tid];
}

// blocks 0 .. kHistBlocks-1: 64 histogram bins each, 16 slices of the partial records per bin; block kHistBlocks: the scalars.
// G == 0 writes (or adds) the empty record.
__global__ __launch_bounds__(kThreads) void xolp_stats_finalize_kernel(const unsigned char* __restrict__ ws,
                                                                       unsigned char* __restrict__ stats, int G, int accumulate) {
    const int tid = threadIdx.x;
    if (blockIdx.x < kHistBlocks) {
        __shared__ unsigned long long red[kWaves][64];
        const unsigned* wh = reinterpret_cast<const unsigned*>(ws + 80 * (size_t)G);
        const int bin = blockIdx.x * 64 + (tid & 63), grp = tid >> 6;
        unsigned long long acc = 0;
        if (bin < kBins)
            for (int gi = grp; gi < G; gi += kWaves) acc += wh[gi * kBins + bin];
        red[grp][tid & 63] = acc;
        __syncthreads();
        if (tid < 64 && bin < kBins) {
            unsigned long long t = 0;
            for (int k = 0; k < kWaves; ++k) t += red[k][tid];
            unsigned long long* out = reinterpret_cast<unsigned long long*>(stats + kStatsHist) + bin;
            *out = accumulate ? *out + t : t;
        }
        return;
    }
    __shared__ double ds[4 * kMaxBlocks];
    __shared__ long long cs[4 * kMaxBlocks];
    __shared__ float es[4 * kMaxBlocks];
    const double* wd = reinterpret_cast<const double*>(ws);
    const long long* wc = reinterpret_cast<const long long*>(ws + 32 * (size_t)G);
    const float* we = reinterpret_cast<const float*>(ws + 64 * (size_t)G);
    for (int i = tid; i < 4 * G; i += kThreads) { ds[i] = wd[i]; cs[i] = wc[i]; es[i] = we[i]; }
    __syncthreads();
    if (tid < 4) {                                  // counters: n, nonfinite, over[0], over[1]
        long long t = 0;
        for (int gi = 0; gi < G; ++gi) t += cs[tid * G + gi];
        long long* out = reinterpret_cast<long long*>(stats) + tid;
        *out = accumulate ? *out + t : t;
    } else if (tid < 8) {                           // fp64 sums, workgroups in index order
        const int k = tid - 4;
        double t = 0.0;
        for (int gi = 0; gi < G; ++gi) t += ds[k * G + gi];
        double* out = reinterpret_cast<double*>(stats + 32) + k;
        *out = accumulate ? *out + t : t;
    } else if (tid < 12) {                          // extrema
        const int k = tid - 8;
        float t = (k & 1) ? -INFINITY : INFINITY;
        for (int gi = 0; gi < G; ++gi) t = (k & 1) ? fmaxf(t, es[k * G + gi]) : fminf(t, es[k * G + gi]);
        float* out = reinterpret_cast<float*>(stats + 64) + k;
        if (accumulate) t = (k & 1) ? fmaxf(t, *out) : fminf(t, *out);
        *out = t;
    }
}

static_assert(kStatsHist + (size_t)kBins * 8 == PD_XOLP_STATS_BYTES, "record layout");

inline int grid_for(long quads) {
    const long b = (quads + kQuadsPerBlock - 1) / kQuadsPerBlock;
    return (int)(b > kMaxBlocks ? kMaxBlocks : (b < 1 ? 1 : b));
}

// workgroups for B x H rows of ceil(W / 4) quads, without overflow for any int arguments
inline int grid_for_shape(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 1;
    const long rows = (long)B * H;
    if (rows >= kMaxBlocks * kQuadsPerBlock) return kMaxBlocks;
    return grid_for(rows * ((W + 3L) / 4));
}

}  // namespace

extern "C" size_t pd_xolp_stats_workspace(int B, int H, int W) {
    return (grid_for_shape(B, H, W) * kPartialBytes + 15) & ~(size_t)15;
}

extern "C" int pd_xolp_stats(const void* xolp, const void* mask, void* stats, void* workspace, size_t ws_bytes, int B, int H,
                             int W, int ld, const float thresholds[2], int accumulate, void* stream) {
    PD_REQUIRE(B >= 0 && H > 0 && W > 0 && ld > 0, "pd_xolp_stats: bad shape (B = %d, H = %d, W = %d, ld = %d)", B, H, W, ld);
    PD_REQUIRE((xolp || B == 0) && stats && workspace, "pd_xolp_stats: xolp, stats and workspace must not be null");
    PD_REQUIRE(thresholds && std::isfinite(thresholds[0]) && std::isfinite(thresholds[1]),
               "pd_xolp_stats: thresholds must be two finite numbers");
    PD_REQUIRE(W <= ld, "pd_xolp_stats: W = %d exceeds the row pitch ld = %d", W, ld);
    PD_REQUIRE(ld % 4 == 0, "pd_xolp_stats: the row pitch ld = %d must be a multiple of 4", ld);
    PD_REQUIRE(pd::aligned16(xolp) && pd::aligned16(mask) && pd::aligned16(stats) && pd::aligned16(workspace),
               "pd_xolp_stats: xolp, mask, stats and workspace must be 16-byte aligned");
    const size_t need = pd_xolp_stats_workspace(B, H, W);
    PD_REQUIRE(ws_bytes >= need, "pd_xolp_stats: workspace too small (%zu bytes, pd_xolp_stats_workspace asks for %zu)",
               ws_bytes, need);
    // element offsets are 32-bit in the kernel: a launch covers at most 2^30 elements, the batch is split by frames
    const long frame = 2L * H * ld;
    PD_REQUIRE(frame <= (1L << 30), "pd_xolp_stats: a frame of %d x %d (pitch %d) is too large for the kernel's index arithmetic",
               H, W, ld);
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) {
        if (!accumulate)
            hipLaunchKernelGGL(xolp_stats_finalize_kernel, dim3(kHistBlocks + 1), dim3(kThreads), 0, st,
                               (const unsigned char*)workspace, (unsigned char*)stats, 0, 0);
        return pd::check_launch("pd_xolp_stats");
    }
    const long max_b = (1L << 30) / frame;
    const unsigned Q = (unsigned)((W + 3) / 4);
    for (long b0 = 0; b0 < B; b0 += max_b) {
        const long nb = std::min<long>(max_b, B - b0);
        Geo g;
        g.total = (unsigned)(nb * H * Q);      // <= 2^30 / 8
        g.Q = Q; g.H = (unsigned)H; g.W = (unsigned)W; g.ld = (unsigned)ld;
        const int G = grid_for((long)g.total);
        const unsigned step = (unsigned)G * kThreads, drow = step / Q;
        g.dq = step % Q; g.dy = drow % (unsigned)H; g.db = drow / (unsigned)H;
        hipLaunchKernelGGL(xolp_stats_kernel, dim3(G), dim3(kThreads), 0, st, static_cast<const float*>(xolp) + b0 * frame,
                           mask ? static_cast<const uint8_t*>(mask) + b0 * (frame / 2) : nullptr, (unsigned char*)workspace, g,
                           thresholds[0], thresholds[1]);
        hipLaunchKernelGGL(xolp_stats_finalize_kernel, dim3(kHistBlocks + 1), dim3(kThreads), 0, st,
                           (const unsigned char*)workspace, (unsigned char*)stats, G, (accumulate || b0 > 0) ? 1 : 0);
    }
    return pd::check_launch("pd_xolp_stats");
}
