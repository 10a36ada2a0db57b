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
//   pcd_stat_kernel      the per-class records of class_records.hpp (their three launches, and why the sums are
//                        bit-reproducible, are described there): one work item = one slot; the counters are `bad` and
//                        `unmatched`.  The bin of a distance is the number of table entries edges2[j] <= d2, by a nine-step
//                        binary search over a copy of the caller's 511 floats in LDS.
#include "class_records.hpp"
#include "wave_ops.hpp"

#include <cmath>

namespace {

using Rec = Layout<PD_PCD_BINS, 2, 12>;             // two counters (`bad`, `unmatched`), the histogram starts at byte 48
constexpr int kTile = PD_PCD_TILE;
constexpr int kBins = Rec::kBins;
constexpr int kEdges = kBins - 1;
constexpr long kMaxBlocks = 1L << 30;               // per launch
constexpr long kMaxSlots = 1L << 30;                // per image: slot offsets inside a frame are 32-bit

static_assert(48 + 4 * kBins == PD_PCD_RECORD_BYTES && Rec::kBytes == PD_PCD_RECORD_BYTES, "record layout");
static_assert(kMaxK == PD_PCD_MAX_CLASSES, "class limit");
static_assert(kTile == 256, "a tile is 16 x 16 pixels, four slots per lane of a wave");

struct Box { float lo[3], hi[3]; int count, pad; };
static_assert(sizeof(Box) == 32, "box record");

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

using pd_wave::wave_max;

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

__global__ __launch_bounds__(kThreads) void pcd_stat_kernel(const float* __restrict__ d2, const float4* __restrict__ pts,
                                                            const int* __restrict__ mask, const float* __restrict__ edges2,
                                                            float* __restrict__ dist, unsigned* __restrict__ stats,
                                                            double* __restrict__ ws, Classes cls, Geo g) {
    extern __shared__ __align__(16) unsigned char smem[];
    double* wsum = reinterpret_cast<double*>(smem);                                   // [kWaves][kMaxK][2]
    float* edges = reinterpret_cast<float*>(wsum + kWaves * kMaxK * 2);               // [512], the last one is padding
    unsigned* bad = reinterpret_cast<unsigned*>(edges + kBins);                       // [kMaxK]: the counters [2][kMaxK]
    unsigned* unm = bad + kMaxK;                                                      // [kMaxK]
    unsigned* hist = unm + kMaxK;                                                     // [K][512]
    const int tid = threadIdx.x;
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
                if (in_class(cls, k, m)) {
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

    flush_records<Rec>(s, wsum, bad, hist, stats, ws, img, K);
}

inline long tiles_x(int W) { return (W + 15L) / 16; }
inline long tiles_of(int H, int W) { return ((H + 15L) / 16) * tiles_x(W); }
inline int groups_of(int H, int W) { return groups_for(H > 0 && W > 0 ? tiles_of(H, W) * kTile : 0); }      // items: slots

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
    return records_workspace(N, K, groups_of(H, W));
}

extern "C" int pd_cloud_stats(const void* d2, const void* points, const void* mask, const int* classes, int K,
                              const void* edges2, void* dist, void* stats, void* workspace, size_t ws_bytes, int N, int H, int W,
                              void* stream) {
    PD_REQUIRE(N >= 0 && H > 0 && W > 0, "pd_cloud_stats: bad shape (N = %d, H = %d, W = %d)", N, H, W);
    PD_REQUIRE(d2 && points && classes && edges2 && stats && workspace,
               "pd_cloud_stats: d2, points, classes, edges2, stats and workspace must not be null");
    Classes cls;
    if (int e = parse_classes("pd_cloud_stats", classes, K, mask != nullptr, &cls)) return e;
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
    g.G = (unsigned)groups_of(H, W);
    g.K = K;
    const size_t frame = (size_t)H * W;
    run_records<Rec>(stats, workspace, N, K, (int)g.G, st, [&](long n0, long nb, unsigned* rec, double* part) {
        hipLaunchKernelGGL(pcd_stat_kernel, dim3((unsigned)(nb * g.G)), dim3(kThreads), lds_bytes(K), st,
                           static_cast<const float*>(d2) + (size_t)n0 * g.slots,
                           static_cast<const float4*>(points) + (size_t)n0 * g.slots,
                           mask ? static_cast<const int*>(mask) + (size_t)n0 * frame : nullptr,
                           static_cast<const float*>(edges2), dist ? static_cast<float*>(dist) + (size_t)n0 * frame : nullptr,
                           rec, part, cls, g);
    });
    return pd::check_launch("pd_cloud_stats");
}
