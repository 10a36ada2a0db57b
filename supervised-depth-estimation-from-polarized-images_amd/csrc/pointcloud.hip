// Point-cloud accuracy: back-projection of depth maps into tiled clouds, the exact nearest-neighbour distance between two
// clouds, and its per-image, per-class records (counts, fp64 sums, a 0.5 mm histogram).  Definition, cloud layout and
// record: include/polardepth.h, pd_backproject / pd_cloud_nn / pd_cloud_stats.
//
//   backproject_kernel   one workgroup of 256 lanes per 16x16 pixel tile, one lane per slot: the point, then the tile's
//                        box by a fixed shuffle tree and four wave partials in LDS.
//   cloud_nn_kernel      ONE WAVE per query tile, four queries per lane (slots lane, lane + 64, ...).  Target points are
//                        wave-uniform: they are read with uniform addresses (the scalar-load path) and used as scalar
//                        operands, so a target costs the vector unit nothing but the arithmetic of the four queries --
//                        no LDS, no barrier.  Target tiles are tested 64 at a time (one box per lane, one ballot); the
//                        ballot is re-taken against the current R after every scanned tile, R by a wave max reduction.
//                        Every branch is wave-uniform.
//   pcd_stat_kernel      the scheme of nstat_kernel (csrc/normals_stats.hip): LDS histogram [K][512], per-lane fp64 sums,
//                        partials through the workspace, pcd_finalize_kernel adds them in index order.
#include "pd_common.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kTile = PD_PCD_TILE;
constexpr int kBins = PD_PCD_BINS;
constexpr int kEdges = kBins - 1;
constexpr int kMaxK = PD_PCD_MAX_CLASSES;
constexpr int kRecWords = PD_PCD_RECORD_BYTES / 4;
constexpr int kHistWord = 12;                       // the histogram starts at byte 48
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxGroups = 64;                      // workgroups per image of the stats kernel
constexpr long kSlotsPerGroup = 4L * kThreads;
constexpr long kMaxBlocks = 1L << 30;               // per launch
constexpr long kMaxSlots = 1L << 30;                // per image: slot offsets inside a frame are 32-bit

static_assert(48 + 4 * kBins == PD_PCD_RECORD_BYTES && PD_PCD_RECORD_BYTES % 16 == 0, "record layout");
static_assert(kTile == 256, "a tile is 16 x 16 pixels, four slots per lane of a wave");

struct Box { float lo[3], hi[3]; int count, pad; };
static_assert(sizeof(Box) == 32, "box record");

struct Classes { int lo[kMaxK], hi[kMaxK]; };

__device__ __forceinline__ bool in_range(float d, float lo, float hi) { return d >= lo && d <= hi; }      // NaN fails

__global__ __launch_bounds__(kThreads) void backproject_kernel(const float* __restrict__ depth, const float* __restrict__ Kmat,
                                                               const float* __restrict__ gate, float4* __restrict__ points,
                                                               Box* __restrict__ boxes, unsigned H, unsigned W, unsigned TX,
                                                               unsigned T, float min_d, float max_d) {
    __shared__ float red[kWaves][6];
    __shared__ int cnt[kWaves];
    const unsigned img = blockIdx.x / T, tile = blockIdx.x - img * T;
    const unsigned ty = tile / TX, tx = tile - ty * TX;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned v = ty * 16u + ((unsigned)tid >> 4), u = tx * 16u + ((unsigned)tid & 15u);
    const float* Km = Kmat + (size_t)img * 16;
    const float fx = Km[0], cx = Km[2], fy = Km[5], cy = Km[6];
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    if (v < H && u < W) {
        const size_t pix = (size_t)img * H * W + (size_t)v * W + u;
        const float z = depth[pix];
        const float g = gate ? gate[pix] : z;
        if (in_range(g, min_d, max_d)) {
            if (__builtin_isfinite(z) && z > 0.f) {
                p.x = (((float)u - cx) / fx) * z;
                p.y = (((float)v - cy) / fy) * z;
                p.z = z;
                p.w = 1.f;
            } else {
                p.w = -1.f;
            }
        }
    }
    points[(size_t)blockIdx.x * kTile + tid] = p;
    const bool is = p.w == 1.f;
    float lo[3] = {is ? p.x : INFINITY, is ? p.y : INFINITY, is ? p.z : INFINITY};
    float hi[3] = {is ? p.x : -INFINITY, is ? p.y : -INFINITY, is ? p.z : -INFINITY};
    int c = is ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], off));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off));
        }
        c += __shfl_xor(c, off);
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            red[wave][a] = lo[a];
            red[wave][3 + a] = hi[a];
        }
        cnt[wave] = c;
    }
    __syncthreads();
    if (tid == 0) {
        Box b;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            b.lo[a] = fminf(fminf(red[0][a], red[1][a]), fminf(red[2][a], red[3][a]));
            b.hi[a] = fmaxf(fmaxf(red[0][3 + a], red[1][3 + a]), fmaxf(red[2][3 + a], red[3][3 + a]));
        }
        b.count = cnt[0] + cnt[1] + cnt[2] + cnt[3];
        b.pad = 0;
        boxes[blockIdx.x] = b;
    }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

// every w = 1 target of one tile against the four queries of each lane; tp is wave-uniform
__device__ __forceinline__ void scan_tile(const float4* __restrict__ tp, const float (&qx)[4], const float (&qy)[4],
                                          const float (&qz)[4], float (&best)[4]) {
#pragma unroll 8
    for (int j = 0; j < kTile; ++j) {
        const float4 t = tp[j];
        // a slot that is no point moves to infinity: its distance is +inf for every finite query (an integer compare and a
        // select on uniform values: scalar work)
        const float tx = __float_as_uint(t.w) == 0x3f800000u ? t.x : INFINITY;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float dx = qx[i] - tx, dy = qy[i] - t.y, dz = qz[i] - t.z;
            best[i] = fminf(best[i], (dx * dx + dy * dy) + dz * dz);
        }
    }
}

__global__ __launch_bounds__(64) void cloud_nn_kernel(const float4* __restrict__ qpts, const Box* __restrict__ qboxes,
                                                      const float4* __restrict__ tpts, const Box* __restrict__ tboxes,
                                                      float* __restrict__ d2, int* __restrict__ visited, unsigned Tq,
                                                      unsigned Tt, unsigned brute) {
    const unsigned img = blockIdx.x / Tq, tile = blockIdx.x - img * Tq;
    const int lane = threadIdx.x;
    const float4* qp = qpts + (size_t)blockIdx.x * kTile;
    const float4* tbase = tpts + (size_t)img * Tt * kTile;
    const Box* tb = tboxes + (size_t)img * Tt;
    float qx[4], qy[4], qz[4], best[4];
    bool isq[4];
    bool any = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 q = qp[i * 64 + lane];
        qx[i] = q.x; qy[i] = q.y; qz[i] = q.z;
        isq[i] = q.w == 1.f;
        any = any || isq[i];
        best[i] = INFINITY;
    }
    int seen = 0;
    if (brute) {
        for (unsigned t = 0; t < Tt; ++t) scan_tile(tbase + (size_t)t * kTile, qx, qy, qz, best);
        seen = (int)Tt;
    } else if (__builtin_amdgcn_ballot_w64(any) != 0ull) {
        float R = INFINITY;
        auto refresh = [&]() {
            float r = -INFINITY;
#pragma unroll
            for (int i = 0; i < 4; ++i) r = isq[i] ? fmaxf(r, best[i]) : r;
            R = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(wave_max(r))));      // the builtin moves 32 bits as an int
        };
        if (tile < Tt && tb[tile].count > 0) {
            scan_tile(tbase + (size_t)tile * kTile, qx, qy, qz, best);
            ++seen;
            refresh();
        }
        const Box qb = qboxes[blockIdx.x];
        for (unsigned t0 = 0; t0 < Tt; t0 += 64) {
            const unsigned t = t0 + (unsigned)lane;
            bool ok = t < Tt && t != tile;
            float bd = INFINITY;
            if (ok) {
                const Box b = tb[t];
                ok = b.count > 0;
                const float gx = fmaxf(fmaxf(0.f, b.lo[0] - qb.hi[0]), qb.lo[0] - b.hi[0]);
                const float gy = fmaxf(fmaxf(0.f, b.lo[1] - qb.hi[1]), qb.lo[1] - b.hi[1]);
                const float gz = fmaxf(fmaxf(0.f, b.lo[2] - qb.hi[2]), qb.lo[2] - b.hi[2]);
                bd = (gx * gx + gy * gy) + gz * gz;
            }
            unsigned long long rest = __builtin_amdgcn_ballot_w64(ok);
            while (true) {
                // R only falls: a tile that fails now fails for good
                rest &= __builtin_amdgcn_ballot_w64(bd <= R);
                if (rest == 0ull) break;
                const unsigned j = (unsigned)__builtin_ctzll(rest);
                rest &= rest - 1ull;
                scan_tile(tbase + (size_t)(t0 + j) * kTile, qx, qy, qz, best);
                ++seen;
                refresh();
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) d2[(size_t)blockIdx.x * kTile + i * 64 + lane] = isq[i] ? best[i] : __builtin_nanf("");
    if (visited && lane == 0) visited[blockIdx.x] = seen;
}

struct Geo {
    unsigned H, W, TX, slots;     // rows, columns, tiles per tile row, slots per image
    unsigned G;                   // workgroups per image
    int K;
};

__global__ __launch_bounds__(kThreads) void pcd_zero_kernel(uint4* __restrict__ stats, long n16) {
    for (long i = blockIdx.x * (long)kThreads + threadIdx.x; i < n16; i += (long)gridDim.x * kThreads)
        stats[i] = make_uint4(0u, 0u, 0u, 0u);
}

__global__ __launch_bounds__(kThreads) void pcd_stat_kernel(const float* __restrict__ d2, const float4* __restrict__ pts,
                                                            const int* __restrict__ mask, const float* __restrict__ edges2,
                                                            float* __restrict__ dist, unsigned* __restrict__ stats,
                                                            double* __restrict__ ws, Classes cls, Geo g) {
    extern __shared__ __align__(16) unsigned char smem[];
    double* wsum = reinterpret_cast<double*>(smem);                                   // [kWaves][kMaxK][2]
    float* edges = reinterpret_cast<float*>(wsum + kWaves * kMaxK * 2);               // [512], the last one is padding
    unsigned* bad = reinterpret_cast<unsigned*>(edges + kBins);                       // [kMaxK]
    unsigned* unm = bad + kMaxK;                                                      // [kMaxK]
    unsigned* hist = unm + kMaxK;                                                     // [K][512]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = g.K;
    for (int i = tid; i < kBins; i += kThreads) edges[i] = i < kEdges ? edges2[i] : INFINITY;
    if (tid < kMaxK) bad[tid] = unm[tid] = 0;
    for (int i = tid; i < K * kBins; i += kThreads) hist[i] = 0;
    __syncthreads();

    const unsigned img = blockIdx.x / g.G, grp = blockIdx.x - img * g.G;
    const size_t frame = (size_t)g.H * g.W, base = (size_t)img * frame, sbase = (size_t)img * g.slots;
    const int* mask_f = mask ? mask + base : nullptr;
    float* dist_f = dist ? dist + base : nullptr;

    double s[kMaxK][2];
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) s[k][0] = s[k][1] = 0.0;

    // slots of this image go round-robin over its G workgroups, a lane takes them in increasing order
    for (unsigned item = grp * kThreads + tid; item < g.slots; item += g.G * kThreads) {
        const unsigned tile = item >> 8, slot = item & 255u;
        const unsigned ty = tile / g.TX, tx = tile - ty * g.TX;
        const unsigned y = ty * 16u + (slot >> 4), x = tx * 16u + (slot & 15u);
        if (y >= g.H || x >= g.W) continue;
        const unsigned p = y * g.W + x;
        const float w = pts[sbase + item].w;
        const float v = d2[sbase + item];
        const bool point = w == 1.f, isbad = w == -1.f;
        const bool inf = point && v == INFINITY;
        const bool fin = point && __builtin_isfinite(v);
        const double vd = fin ? (double)v : 0.0;
        const double dd = sqrt(vd);
        if (dist_f) dist_f[p] = fin ? (float)dd : (inf ? INFINITY : __builtin_nanf(""));
        if (!(point || isbad)) continue;
        int lo = 0, hi = kEdges;
        if (fin) {
#pragma unroll 1
            for (int it = 0; it < 9; ++it) {              // 2^9 > 511
                const int mid = (lo + hi) >> 1;           // lo == hi: the padding entry or one already decided, harmless
                const bool le = lo < hi && edges[mid] <= v;
                const bool gtb = lo < hi && !le;
                lo = le ? mid + 1 : lo;
                hi = gtb ? mid : hi;
            }
        }
        const int m = mask_f ? mask_f[p] : 0;
#pragma unroll
        for (int k = 0; k < kMaxK; ++k) {
            if (k < K) {
                const bool in = cls.lo[k] > cls.hi[k] || (m >= cls.lo[k] && m <= cls.hi[k]);
                if (in) {
                    if (fin) {
                        atomicAdd(&hist[k * kBins + lo], 1u);
                        s[k][0] += dd;
                        s[k][1] += vd;
                    } else if (inf) {
                        atomicAdd(&unm[k], 1u);
                    } else if (isbad) {
                        atomicAdd(&bad[k], 1u);
                    }
                }
            }
        }
    }

    // lanes -> wave by a fixed tree, waves -> workgroup in order
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
        if (k < K) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                s[k][0] += __shfl_down(s[k][0], off);
                s[k][1] += __shfl_down(s[k][1], off);
            }
            if (lane == 0) {
                wsum[(wave * kMaxK + k) * 2] = s[k][0];
                wsum[(wave * kMaxK + k) * 2 + 1] = s[k][1];
            }
        }
    }
    __syncthreads();
    if (tid < 2 * K) {
        double t = 0.0;
        for (int w = 0; w < kWaves; ++w) t += wsum[w * kMaxK * 2 + tid];
        ws[((size_t)blockIdx.x * K) * 2 + tid] = t;      // [img][grp][k][2]
    }
    unsigned* rec = stats + (size_t)img * K * kRecWords;
    if (tid < K && bad[tid])
        atomicAdd(reinterpret_cast<unsigned long long*>(rec + (size_t)tid * kRecWords + 2), (unsigned long long)bad[tid]);
    if (tid < K && unm[tid])
        atomicAdd(reinterpret_cast<unsigned long long*>(rec + (size_t)tid * kRecWords + 4), (unsigned long long)unm[tid]);
    for (int i = tid; i < K * kBins; i += kThreads) {
        const unsigned v = hist[i];
        if (v) {
            const int k = i / kBins;
            atomicAdd(rec + (size_t)k * kRecWords + kHistWord + (i - k * kBins), v);
        }
    }
}

// one workgroup per record [img][k]
__global__ __launch_bounds__(kThreads) void pcd_finalize_kernel(unsigned* __restrict__ stats, const double* __restrict__ ws,
                                                                int K, int G) {
    __shared__ unsigned long long red[kThreads];
    const int tid = threadIdx.x;
    const unsigned img = blockIdx.x / K, k = blockIdx.x - img * K;
    unsigned* rec = stats + (size_t)blockIdx.x * kRecWords;
    unsigned long long acc = 0;
    for (int i = tid; i < kBins; i += kThreads) acc += rec[kHistWord + i];
    red[tid] = acc;
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    if (tid == 0) *reinterpret_cast<long long*>(rec) = (long long)red[0];
    if (tid == 64 || tid == 128) {                     // the two fp64 sums, workgroups in index order
        const int which = tid == 64 ? 0 : 1;
        double t = 0.0;
        for (int gi = 0; gi < G; ++gi) t += ws[(((size_t)img * G + gi) * K + k) * 2 + which];
        reinterpret_cast<double*>(rec)[3 + which] = t;
    }
}

inline long tiles_x(int W) { return (W + 15L) / 16; }
inline long tiles_of(int H, int W) { return ((H + 15L) / 16) * tiles_x(W); }

inline int groups_for(int H, int W) {
    if (H <= 0 || W <= 0) return 1;
    const long slots = tiles_of(H, W) * kTile;
    const long b = (slots + kSlotsPerGroup - 1) / kSlotsPerGroup;
    return (int)std::min<long>(kMaxGroups, std::max<long>(1, b));
}

inline size_t lds_bytes(int K) {
    return (size_t)kWaves * kMaxK * 2 * 8 + (size_t)kBins * 4 + (size_t)kMaxK * 8 + (size_t)K * kBins * 4;
}

}  // namespace

extern "C" int pd_backproject(const void* depth, const void* K, const void* gate, void* points, void* boxes, int N, int H,
                              int W, float min_depth, float max_depth, void* stream) {
    PD_REQUIRE(N >= 0 && H > 0 && W > 0, "pd_backproject: bad shape (N = %d, H = %d, W = %d)", N, H, W);
    PD_REQUIRE(depth && K && points && boxes, "pd_backproject: depth, K, points and boxes must not be null");
    PD_REQUIRE(pd::aligned16(points) && pd::aligned16(boxes), "pd_backproject: points and boxes must be 16-byte aligned");
    const long T = tiles_of(H, W);
    PD_REQUIRE(T * kTile <= kMaxSlots, "pd_backproject: a frame of %d x %d is too large for the kernel's index arithmetic", H, W);
    if (N == 0) return PD_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t frame = (size_t)H * W;
    const long per = std::max<long>(1, kMaxBlocks / T);
    for (long n0 = 0; n0 < N; n0 += per) {
        const long nb = std::min<long>(per, N - n0);
        hipLaunchKernelGGL(backproject_kernel, dim3((unsigned)(nb * T)), dim3(kThreads), 0, st,
                           static_cast<const float*>(depth) + (size_t)n0 * frame, static_cast<const float*>(K) + (size_t)n0 * 16,
                           gate ? static_cast<const float*>(gate) + (size_t)n0 * frame : nullptr,
                           static_cast<float4*>(points) + (size_t)n0 * T * kTile, static_cast<Box*>(boxes) + (size_t)n0 * T,
                           (unsigned)H, (unsigned)W, (unsigned)tiles_x(W), (unsigned)T, min_depth, max_depth);
    }
    return pd::check_launch("pd_backproject");
}

extern "C" int pd_cloud_nn(const void* q_points, const void* q_boxes, int Tq, const void* t_points, const void* t_boxes, int Tt,
                           void* d2, void* visited, unsigned flags, int N, void* stream) {
    PD_REQUIRE(N >= 0 && Tq > 0 && Tt > 0, "pd_cloud_nn: bad shape (N = %d, Tq = %d, Tt = %d)", N, Tq, Tt);
    PD_REQUIRE(q_points && q_boxes && t_points && t_boxes && d2,
               "pd_cloud_nn: q_points, q_boxes, t_points, t_boxes and d2 must not be null");
    PD_REQUIRE((flags & ~PD_PCD_BRUTE) == 0, "pd_cloud_nn: unknown flags 0x%x", flags);
    PD_REQUIRE(pd::aligned16(q_points) && pd::aligned16(q_boxes) && pd::aligned16(t_points) && pd::aligned16(t_boxes),
               "pd_cloud_nn: points and boxes must be 16-byte aligned");
    PD_REQUIRE((long)Tq * kTile <= kMaxSlots && (long)Tt * kTile <= kMaxSlots,
               "pd_cloud_nn: a cloud of %d / %d tiles is too large for the kernel's index arithmetic", Tq, Tt);
    if (N == 0) return PD_OK;
    hipStream_t st = (hipStream_t)stream;
    const long per = std::max<long>(1, kMaxBlocks / Tq);
    for (long n0 = 0; n0 < N; n0 += per) {
        const long nb = std::min<long>(per, N - n0);
        hipLaunchKernelGGL(cloud_nn_kernel, dim3((unsigned)(nb * Tq)), dim3(64), 0, st,
                           static_cast<const float4*>(q_points) + (size_t)n0 * Tq * kTile,
                           static_cast<const Box*>(q_boxes) + (size_t)n0 * Tq,
                           static_cast<const float4*>(t_points) + (size_t)n0 * Tt * kTile,
                           static_cast<const Box*>(t_boxes) + (size_t)n0 * Tt, static_cast<float*>(d2) + (size_t)n0 * Tq * kTile,
                           visited ? static_cast<int*>(visited) + (size_t)n0 * Tq : nullptr, (unsigned)Tq, (unsigned)Tt,
                           flags & PD_PCD_BRUTE);
    }
    return pd::check_launch("pd_cloud_nn");
}

extern "C" size_t pd_cloud_stats_workspace(int N, int H, int W, int K) {
    const size_t n = N > 0 ? (size_t)N : 1, k = (size_t)std::min(std::max(K, 1), kMaxK);
    return n * (size_t)groups_for(H, W) * k * 16;
}

extern "C" int pd_cloud_stats(const void* d2, const void* points, const void* mask, const int* classes, int K,
                              const void* edges2, void* dist, void* stats, void* workspace, size_t ws_bytes, int N, int H, int W,
                              void* stream) {
    PD_REQUIRE(N >= 0 && H > 0 && W > 0, "pd_cloud_stats: bad shape (N = %d, H = %d, W = %d)", N, H, W);
    PD_REQUIRE(d2 && points && classes && edges2 && stats && workspace,
               "pd_cloud_stats: d2, points, classes, edges2, stats and workspace must not be null");
    PD_REQUIRE(K >= 1 && K <= kMaxK, "pd_cloud_stats: K = %d classes, 1 .. %d are supported", K, kMaxK);
    Classes cls;
    for (int k = 0; k < kMaxK; ++k) {
        cls.lo[k] = k < K ? classes[2 * k] : 1;
        cls.hi[k] = k < K ? classes[2 * k + 1] : 0;
        PD_REQUIRE(k >= K || mask || cls.lo[k] > cls.hi[k],
                   "pd_cloud_stats: class %d is the range [%d, %d] of the mask value, but mask is null", k, cls.lo[k], cls.hi[k]);
    }
    PD_REQUIRE(pd::aligned16(points) && pd::aligned16(stats) && pd::aligned16(workspace),
               "pd_cloud_stats: points, stats and workspace must be 16-byte aligned");
    const long T = tiles_of(H, W);
    PD_REQUIRE(T * kTile <= kMaxSlots, "pd_cloud_stats: a frame of %d x %d is too large for the kernel's index arithmetic", H, W);
    const size_t need = pd_cloud_stats_workspace(N, H, W, K);
    PD_REQUIRE(ws_bytes >= need, "pd_cloud_stats: workspace too small (%zu bytes, pd_cloud_stats_workspace asks for %zu)",
               ws_bytes, need);
    if (N == 0) return PD_OK;
    hipStream_t st = (hipStream_t)stream;
    Geo g;
    g.H = (unsigned)H; g.W = (unsigned)W; g.TX = (unsigned)tiles_x(W); g.slots = (unsigned)(T * kTile);
    g.G = (unsigned)groups_for(H, W);
    g.K = K;
    const size_t frame = (size_t)H * W;
    const long per = 1L << 20;                           // keeps gridDim.x = images * groups below 2^31
    for (long n0 = 0; n0 < N; n0 += per) {
        const long nb = std::min<long>(per, N - n0);
        unsigned char* rec = static_cast<unsigned char*>(stats) + (size_t)n0 * K * PD_PCD_RECORD_BYTES;
        double* part = static_cast<double*>(workspace) + (size_t)n0 * g.G * K * 2;
        const long n16 = nb * K * (PD_PCD_RECORD_BYTES / 16);
        const int zgrid = (int)std::min<long>(1024, (n16 + kThreads - 1) / kThreads);
        hipLaunchKernelGGL(pcd_zero_kernel, dim3(zgrid), dim3(kThreads), 0, st, reinterpret_cast<uint4*>(rec), n16);
        hipLaunchKernelGGL(pcd_stat_kernel, dim3((unsigned)(nb * g.G)), dim3(kThreads), lds_bytes(K), st,
                           static_cast<const float*>(d2) + (size_t)n0 * g.slots,
                           static_cast<const float4*>(points) + (size_t)n0 * g.slots,
                           mask ? static_cast<const int*>(mask) + (size_t)n0 * frame : nullptr,
                           static_cast<const float*>(edges2), dist ? static_cast<float*>(dist) + (size_t)n0 * frame : nullptr,
                           reinterpret_cast<unsigned*>(rec), part, cls, g);
        hipLaunchKernelGGL(pcd_finalize_kernel, dim3((unsigned)(nb * K)), dim3(kThreads), 0, st,
                           reinterpret_cast<unsigned*>(rec), part, K, (int)g.G);
    }
    return pd::check_launch("pd_cloud_stats");
}
