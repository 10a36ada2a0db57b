// Polarimetric depth refinement: the disambiguated polarisation normals integrated back into the depth prior, per item a
// screened Poisson problem in zeta = log z solved by Chebyshev semi-iteration on the Jacobi-preconditioned normal equations.
// Definition, operation order and the spectrum bound: include/polardepth.h; NumPy statement: tests/polar_refine_ref.py.
//
// Every kernel but the fused one (refine_steps_kernel, described where it stands): one lane per pixel, a workgroup is a
// 64 x 4 tile of ONE item (blockIdx.x = (item * tiles_y + ty) * tiles_x + tx), fp64, plain vector stores.  No atomics and no waiting between workgroups: the two maxima (S, the residual) leave as one
// partial per workgroup and a second launch with one workgroup per item reduces them; a maximum has no order.
//
// refine_setup_kernel: a pixel needs liveness, rho, p, q and zeta0 of itself and of its E, W, S, N neighbours.  They are
//   recomputed (pix_at, five evaluations per pixel, the neighbours' loads hit L2) instead of staged: setup runs once next to
//   `iters` steps, and the same function on the same inputs gives the same bits on both sides of an edge.
//   Its second instantiation (<Weight>, pd_polar_refine_setup_w) takes a per-pixel weight of the prior: lam_i = lam * clamp(w)
//   enters diag and rhs only, and the partial that leaves is the workgroup's MINIMUM of a_i = lam_i / (lam_i + s_i), the lower
//   end of the spectrum (refine_table_w_kernel reduces it per item).  The steps and finish read coefficient planes and do not
//   know of the weight.  refine_weights_kernel makes such a map from the decoder's stated uncertainty and, for a robust data
//   term, from the previous round's solution: a lane per pixel, streaming.
// refine_step_kernel: one step per launch.  Per pixel and step it reads wE, wS, rhs, idiag, zeta, d (48 B) and writes zeta, d
//   (16 B); wW, wN and the four neighbours' zeta are re-reads of lines the tile or its neighbour tile fetched.
#include "pd_common.h"
#include "depth_normals.hpp"

#include <cmath>
#include <type_traits>

namespace {

constexpr int TW = 64, TH = 4, RT = TW * TH;

struct Geo {
    int H, W, tx, ty;             // tiles per row / column of an item
    size_t P;                     // pixels per item
};

__device__ __forceinline__ bool locate(const Geo& g, long& n, int& x, int& y) {
    const unsigned b = blockIdx.x;
    const unsigned per = (unsigned)(g.tx * g.ty);
    n = (long)(b / per);
    const unsigned t = b - (unsigned)n * per;
    const int tyi = (int)(t / (unsigned)g.tx), txi = (int)(t - (unsigned)tyi * (unsigned)g.tx);
    x = txi * TW + (int)(threadIdx.x % TW);
    y = tyi * TH + (int)(threadIdx.x / TW);
    return x < g.W && y < g.H;
}

// the workgroup's maximum of v >= 0 (MIN: its minimum, +inf = nothing) into out[blockIdx.x]
template <bool MIN>
__device__ __forceinline__ void block_reduce(double v, double* __restrict__ out) {
    __shared__ double sm[RT];
    sm[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = RT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double o = sm[threadIdx.x + s];
            if (MIN ? o < sm[threadIdx.x] : o > sm[threadIdx.x]) sm[threadIdx.x] = o;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = sm[0];
}

__device__ __forceinline__ void block_max(double v, double* __restrict__ out) { block_reduce<false>(v, out); }

struct Pix { bool live; double rho, p, q, zeta; };

struct SetupArgs {
    const float* depth; const float* K; const float4* pn; const float* xolp; const unsigned char* valid;
    size_t ldp;
    double lam, edge_max, cos_inc;
};

__device__ __forceinline__ Pix pix_at(const SetupArgs& a, const Geo& g, pd_dn::Cam c, long n, int x, int y) {
    Pix o{false, 0.0, 0.0, 0.0, 0.0};
    if (x < 0 || y < 0 || x >= g.W || y >= g.H) return o;
    const size_t i = (size_t)n * g.P + (size_t)y * g.W + x;
    const float z = a.depth[i];
    const bool zok = __builtin_isfinite(z) && z > 0.f;
    o.zeta = zok ? log((double)z) : 0.0;
    const float4 nf = a.pn[i];
    const double rho = (double)a.xolp[((size_t)n * 2 * g.H + y) * a.ldp + x];
    const double nx = (double)nf.x, ny = (double)nf.y, nz = (double)nf.z;
    const double fx = (double)c.fx, fy = (double)c.fy;
    const double xt = ((double)x - (double)c.cx) / fx, yt = ((double)y - (double)c.cy) / fy;
    const double nr = (nx * xt + ny * yt) + nz;
    const double n2 = (nx * nx + ny * ny) + nz * nz, r2 = (xt * xt + yt * yt) + 1.0;
    const bool ok = zok && __builtin_isfinite(n2) && n2 > 0.0 && __builtin_isfinite(rho) && rho > 0.0 &&
                    (!a.valid || a.valid[i]) && fabs(nr) >= a.cos_inc * (sqrt(n2) * sqrt(r2));
    if (ok) {
        o.live = true;
        o.rho = rho;
        o.p = -nx / (fx * nr);
        o.q = -ny / (fy * nr);
    }
    return o;
}

// weight and gradient of the edge a -> b; gb selects p or q
__device__ __forceinline__ void edge(const Pix& a, const Pix& b, double ga, double gb, double edge_max, double& w, double& g) {
    w = 0.0; g = 0.0;
    if (a.live && b.live && fabs(b.zeta - a.zeta) <= edge_max) {
        w = sqrt(a.rho * b.rho);
        g = (ga + gb) * 0.5;
    }
}

// the per-pixel weight of the prior (pd_polar_refine_setup_w); NoWeight is the scalar lam
struct Weight { const float* map; double lo, hi; };
struct NoWeight {};

// lam_i of pixel i: lam * clamp(weight_i); a NaN takes the lower end
__device__ __forceinline__ double lam_at(double lam, const NoWeight&, size_t) { return lam; }
__device__ __forceinline__ double lam_at(double lam, const Weight& wt, size_t i) {
    const double w = (double)wt.map[i];
    return lam * (!(w >= wt.lo) ? wt.lo : w > wt.hi ? wt.hi : w);
}

// W = NoWeight: the partial is the workgroup's maximum of s.  W = Weight: lam_i = lam * clamp(weight) enters diag and rhs, and
// the partial is the workgroup's minimum of a_i = lam_i / (lam_i + s) over its touched pixels, +inf where it touches nothing.
template <class W>
__global__ __launch_bounds__(RT) void refine_setup_kernel(SetupArgs a, Geo g, double* __restrict__ zeta0, double* __restrict__ coef,
                                                          double* __restrict__ pq, double* __restrict__ partial, W wt) {
    constexpr bool WT = std::is_same<W, Weight>::value;
    long n; int x, y;
    const bool in = locate(g, n, x, y);
    double s = 0.0, ai = INFINITY;
    if (in) {
        const pd_dn::Cam c = pd_dn::load_cam(a.K, n);
        const Pix m = pix_at(a, g, c, n, x, y), e = pix_at(a, g, c, n, x + 1, y), w = pix_at(a, g, c, n, x - 1, y),
                  so = pix_at(a, g, c, n, x, y + 1), no = pix_at(a, g, c, n, x, y - 1);
        double wE, gE, wW, gW, wS, gS, wN, gN;
        edge(m, e, m.p, e.p, a.edge_max, wE, gE);
        edge(w, m, w.p, m.p, a.edge_max, wW, gW);
        edge(m, so, m.q, so.q, a.edge_max, wS, gS);
        edge(no, m, no.q, m.q, a.edge_max, wN, gN);
        s = ((wE + wW) + wS) + wN;
        const double lam = lam_at(a.lam, wt, (size_t)n * g.P + (size_t)y * g.W + x);
        const double diag = (((lam + wE) + wW) + wS) + wN;
        const double rhs = (((lam * m.zeta - wE * gE) + wW * gW) - wS * gS) + wN * gN;
        const size_t o = (size_t)y * g.W + x;
        zeta0[(size_t)n * g.P + o] = m.zeta;
        double* cf = coef + (size_t)n * 4 * g.P + o;
        cf[0] = wE; cf[g.P] = wS; cf[2 * g.P] = rhs; cf[3 * g.P] = 1.0 / diag;
        if (pq) {
            pq[(size_t)n * 2 * g.P + o] = m.p;
            pq[(size_t)n * 2 * g.P + g.P + o] = m.q;
        }
        if (WT && s > 0.0) ai = lam / (lam + s);
    }
    block_reduce<WT>(WT ? ai : s, partial);
}

// one workgroup per item: the maximum (MIN: the minimum, +inf = nothing) of its `per` partials; lane 0 goes on with fin(n, it)
template <bool MIN, class F>
__device__ __forceinline__ void item_reduce(const double* __restrict__ partial, int per, F fin) {
    __shared__ double sm[RT];
    const long n = blockIdx.x;
    double m = MIN ? (double)INFINITY : 0.0;
    for (int i = threadIdx.x; i < per; i += RT) {
        const double v = partial[n * per + i];
        if (MIN ? v < m : v > m) m = v;
    }
    sm[threadIdx.x] = m;
    __syncthreads();
#pragma unroll
    for (int s = RT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double o = sm[threadIdx.x + s];
            if (MIN ? o < sm[threadIdx.x] : o > sm[threadIdx.x]) sm[threadIdx.x] = o;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) fin(n, sm[0]);
}

template <class F>
__device__ __forceinline__ void item_max(const double* __restrict__ partial, int per, F fin) { item_reduce<false>(partial, per, fin); }

// the Chebyshev scalars of one item from the lower end a of its spectrum; zeros where there is none
__device__ __forceinline__ void write_table(double* __restrict__ t, int iters, bool any, double a) {
    if (!any) {
        for (int k = 0; k < 2 * iters; ++k) t[k] = 0.0;
        return;
    }
    const double delta = 1.0 - a, sigma = 1.0 / delta;
    double rho = 1.0 / sigma;
    t[0] = 0.0; t[1] = 1.0;
    for (int k = 1; k < iters; ++k) {
        const double rk = 1.0 / (2.0 * sigma - rho);
        t[2 * k] = rk * rho;
        t[2 * k + 1] = (2.0 * rk) / delta;
        rho = rk;
    }
}

__global__ __launch_bounds__(RT) void refine_table_kernel(const double* __restrict__ partial, int per, double lam, int iters,
                                                          double* __restrict__ S, double* __restrict__ table) {
    item_max(partial, per, [&](long n, double s) {
        S[n] = s;
        write_table(table + (size_t)n * iters * 2, iters, s > 0.0 && __builtin_isfinite(s), lam / (lam + s));
    });
}

// the weighted route: the partials are minima of a_i, +inf where a workgroup touches nothing
__global__ __launch_bounds__(RT) void refine_table_w_kernel(const double* __restrict__ partial, int per, int iters,
                                                            double* __restrict__ A, double* __restrict__ table) {
    item_reduce<true>(partial, per, [&](long n, double a) {
        const bool any = a > 0.0 && __builtin_isfinite(a);
        A[n] = any ? a : 0.0;
        write_table(table + (size_t)n * iters * 2, iters, any, a);
    });
}

__global__ __launch_bounds__(RT) void refine_max_kernel(const double* __restrict__ partial, int per, double* __restrict__ out) {
    item_max(partial, per, [&](long n, double m) { out[n] = m; });
}

// r of the definition at (x, y) of item n from zeta; touched = any live edge
__device__ __forceinline__ double residual_at(const double* __restrict__ cf, const double* __restrict__ z, const Geo& g, int x,
                                              int y, bool& touched) {
    const size_t o = (size_t)y * g.W + x;
    // setup leaves 0 on the edges that leave the image; a caller's own coef cannot make a lane read outside its item either
    const double wE = x + 1 < g.W ? cf[o] : 0.0, wS = y + 1 < g.H ? cf[g.P + o] : 0.0;
    const double wW = x > 0 ? cf[o - 1] : 0.0, wN = y > 0 ? cf[g.P + o - g.W] : 0.0;
    touched = ((wE + wW) + wS) + wN > 0.0;
    if (!touched) return 0.0;
    const double tE = wE > 0.0 ? wE * z[o + 1] : 0.0, tW = wW > 0.0 ? wW * z[o - 1] : 0.0;
    const double tS = wS > 0.0 ? wS * z[o + g.W] : 0.0, tN = wN > 0.0 ? wN * z[o - g.W] : 0.0;
    return (cf[2 * g.P + o] + (((tE + tW) + tS) + tN)) * cf[3 * g.P + o] - z[o];
}

__global__ __launch_bounds__(RT) void refine_step_kernel(const double* __restrict__ coef, const double* __restrict__ table, int iters,
                                                         int k, const double* __restrict__ zin, double* __restrict__ zout,
                                                         double* __restrict__ d, Geo g) {
    long n; int x, y;
    if (!locate(g, n, x, y)) return;
    const double* t = table + ((size_t)n * iters + k) * 2;
    const double alpha = t[0], beta = t[1];
    const double* z = zin + (size_t)n * g.P;
    bool touched;
    const double r = residual_at(coef + (size_t)n * 4 * g.P, z, g, x, y, touched);
    const size_t i = (size_t)n * g.P + (size_t)y * g.W + x;
    const double dk = k == 0 ? beta * r : alpha * d[i] + beta * r;
    d[i] = dk;
    zout[i] = z[(size_t)y * g.W + x] + dk;
}

__global__ __launch_bounds__(RT) void refine_finish_kernel(const float* __restrict__ depth, const double* __restrict__ coef,
                                                           const double* __restrict__ zeta, float* __restrict__ out,
                                                           unsigned char* __restrict__ touched_map, double* __restrict__ partial,
                                                           Geo g) {
    long n; int x, y;
    double ar = 0.0;
    if (locate(g, n, x, y)) {
        const double* z = zeta + (size_t)n * g.P;
        bool touched;
        const double r = residual_at(coef + (size_t)n * 4 * g.P, z, g, x, y, touched);
        const size_t o = (size_t)y * g.W + x, i = (size_t)n * g.P + o;
        out[i] = touched ? (float)exp(z[o]) : depth[i];
        touched_map[i] = touched ? 1 : 0;
        ar = fabs(r);
        if (!(ar >= 0.0)) ar = 0.0;               // a NaN is ignored
    }
    block_max(ar, partial);
}

// the raw weight of the prior, (float)(u * h), a lane per pixel over the whole batch (streaming: 4 to 28 bytes per pixel):
// u = ((unc_ref z) / b)^2 from the stated Laplace scale b, h = min(1, c / |zeta_prev - zeta0|) from the previous solution
__global__ __launch_bounds__(RT) void refine_weights_kernel(const float* __restrict__ depth, const float* __restrict__ b, double unc_ref,
                                                            const double* __restrict__ zeta_prev, const double* __restrict__ zeta0,
                                                            double c, float* __restrict__ weight, size_t total) {
    const size_t i = (size_t)blockIdx.x * RT + threadIdx.x;
    if (i >= total) return;
    double u = 1.0, h = 1.0;
    if (b) {
        const float z = depth[i], bi = b[i];
        const double t = (unc_ref * (double)z) / (double)bi;
        u = __builtin_isfinite(z) && z > 0.f && __builtin_isfinite(bi) && bi > 0.f ? t * t : (double)NAN;
    }
    if (zeta_prev) {
        const double r = fabs(zeta_prev[i] - zeta0[i]);
        if (r > c) h = c / r;
    }
    weight[i] = (float)(u * h);
}

// T consecutive steps k0 .. k0 + T - 1 in one launch (overlapped tiling): a workgroup owns FW x FH pixels of one item and holds
// the (FW + 2T) x (FH + 2T) region around them in LDS -- zeta, wE and wS, so that a neighbour's weight and value are LDS reads
// -- and rhs, idiag and d of its lanes' pixels in registers: the coefficients are read once per launch, not once per step.
// Step j of the launch is formed on the region less a rim of j + 1 pixels, which is where the values of step j - 1 are
// those of the one-step kernel; the rim that is lost per step is the redundant work, and after T steps the owned pixels are
// still inside.  The image's own border is no rim: the weights across it are 0 and nothing is read there.  Every value is
// formed by the one-step kernel's expression from the one-step kernel's operands: the same bits.  d has to ping-pong here
// (a rim pixel's d belongs to the neighbour workgroup, which may already have written its new one).  Workgroups do not wait
// for each other.  LDS at T = 8: 80 x 34 x 3 x 8 = 65,280 bytes, under the 64 KB a launch gets without an attribute call.
constexpr int FW = 64, FH = 18;

template <int T>
__global__ __launch_bounds__(RT) void refine_steps_kernel(const double* __restrict__ coef, const double* __restrict__ table, int iters,
                                                          int k0, const double* __restrict__ zin, double* __restrict__ zout,
                                                          const double* __restrict__ din, double* __restrict__ dout, Geo g) {
    constexpr int RW = FW + 2 * T, RH = FH + 2 * T, RP = RW * RH, SLOTS = (RP + RT - 1) / RT;
    static_assert(3 * RP * sizeof(double) <= 64 * 1024, "the launch needs no LDS attribute call");
    __shared__ double sz[RP], sE[RP], sS[RP];
    const unsigned per = (unsigned)(g.tx * g.ty);                 // here: the FW x FH tiles of an item
    const long n = (long)(blockIdx.x / per);
    const unsigned t = blockIdx.x - (unsigned)n * per;
    const int tyi = (int)(t / (unsigned)g.tx), txi = (int)(t - (unsigned)tyi * (unsigned)g.tx);
    const int gx0 = txi * FW - T, gy0 = tyi * FH - T;
    const double* cf = coef + (size_t)n * 4 * g.P;
    const double* z = zin + (size_t)n * g.P;
    const int tid = (int)threadIdx.x;

    double rhs[SLOTS], idg[SLOTS], d[SLOTS], zn[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int idx = s * RT + tid;
        rhs[s] = 0.0; idg[s] = 0.0; d[s] = 0.0; zn[s] = 0.0;
        if (idx < RP) {
            const int ly = idx / RW, lx = idx - ly * RW;
            const int gx = gx0 + lx, gy = gy0 + ly;
            double vz = 0.0, vE = 0.0, vS = 0.0;
            if (gx >= 0 && gy >= 0 && gx < g.W && gy < g.H) {
                const size_t o = (size_t)gy * g.W + gx;
                vz = z[o];
                vE = gx + 1 < g.W ? cf[o] : 0.0;
                vS = gy + 1 < g.H ? cf[g.P + o] : 0.0;
                rhs[s] = cf[2 * g.P + o];
                idg[s] = cf[3 * g.P + o];
                if (k0 > 0) d[s] = din[(size_t)n * g.P + o];
            }
            sz[idx] = vz; sE[idx] = vE; sS[idx] = vS;
        }
    }
    __syncthreads();

#pragma unroll 1
    for (int j = 0; j < T; ++j) {
        const double* tb = table + ((size_t)n * iters + (k0 + j)) * 2;
        const double alpha = tb[0], beta = tb[1];
        const bool first = k0 + j == 0;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const int idx = s * RT + tid;
            const int ly = idx / RW, lx = idx - ly * RW;
            const int gx = gx0 + lx, gy = gy0 + ly;
            // idx < RP follows from ly < RH - j - 1
            if (lx > j && lx < RW - j - 1 && ly > j && ly < RH - j - 1 && gx >= 0 && gy >= 0 && gx < g.W && gy < g.H) {
                const double wE = sE[idx], wS = sS[idx], wW = sE[idx - 1], wN = sS[idx - RW];
                const double zc = sz[idx];
                double r = 0.0;
                if (((wE + wW) + wS) + wN > 0.0) {
                    const double tE = wE > 0.0 ? wE * sz[idx + 1] : 0.0, tW = wW > 0.0 ? wW * sz[idx - 1] : 0.0;
                    const double tS = wS > 0.0 ? wS * sz[idx + RW] : 0.0, tN = wN > 0.0 ? wN * sz[idx - RW] : 0.0;
                    r = (rhs[s] + (((tE + tW) + tS) + tN)) * idg[s] - zc;
                }
                const double dk = first ? beta * r : alpha * d[s] + beta * r;
                d[s] = dk;
                zn[s] = zc + dk;
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const int idx = s * RT + tid;
            const int ly = idx / RW, lx = idx - ly * RW;
            const int gx = gx0 + lx, gy = gy0 + ly;
            if (lx > j && lx < RW - j - 1 && ly > j && ly < RH - j - 1 && gx >= 0 && gy >= 0 && gx < g.W && gy < g.H) sz[idx] = zn[s];
        }
        __syncthreads();
    }

#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int idx = s * RT + tid;
        const int ly = idx / RW, lx = idx - ly * RW;
        const int gx = gx0 + lx, gy = gy0 + ly;
        if (lx >= T && lx < T + FW && ly >= T && ly < T + FH && gx < g.W && gy < g.H) {       // owned: gx, gy >= 0
            const size_t i = (size_t)n * g.P + (size_t)gy * g.W + gx;
            zout[i] = sz[idx];
            dout[i] = d[s];
        }
    }
}

inline long ftiles_of(int H, int W) { return (long)((W + FW - 1) / FW) * ((H + FH - 1) / FH); }

inline long tiles_of(int H, int W) { return (long)((W + TW - 1) / TW) * ((H + TH - 1) / TH); }

inline int shape_args(const char* who, int N, int H, int W) {
    PD_REQUIRE(N >= 0 && H > 0 && W > 0, "%s: bad shape (N = %d, H = %d, W = %d)", who, N, H, W);
    PD_REQUIRE((long)H * W <= (1L << 30), "%s: a frame of %d x %d is too large for the kernel's index arithmetic", who, H, W);
    PD_REQUIRE((double)N * (double)tiles_of(H, W) < 2147483648.0, "%s: too many tiles (N = %d items of %ld workgroups)", who, N,
               tiles_of(H, W));
    return PD_OK;
}

inline int ws_args(const char* who, const void* workspace, size_t ws_bytes, int N, int H, int W) {
    PD_REQUIRE(workspace, "%s: workspace must not be null", who);
    PD_REQUIRE(pd::aligned16(workspace), "%s: workspace must be 16-byte aligned", who);
    const size_t need = pd_polar_refine_workspace(N, H, W);
    PD_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu bytes, pd_polar_refine_workspace asks for %zu)", who, ws_bytes, need);
    return PD_OK;
}

inline Geo geo_of(int H, int W) {
    Geo g;
    g.H = H; g.W = W; g.tx = (W + TW - 1) / TW; g.ty = (H + TH - 1) / TH; g.P = (size_t)H * W;
    return g;
}

}  // namespace

extern "C" size_t pd_polar_refine_workspace(int N, int H, int W) {
    const size_t rows = N > 0 && H > 0 && W > 0 ? (size_t)N * (size_t)tiles_of(H, W) : 0;
    return (rows * sizeof(double) + 16 + 15) / 16 * 16;
}

extern "C" int pd_polar_refine_setup(const void* depth, const void* K_intrinsics, const void* pol_normal, const void* xolp,
                                     long ldp, const void* valid, double lam, double edge_max, double cos_inc, void* zeta0,
                                     void* coef, void* pq, void* workspace, size_t ws_bytes, int N, int H, int W, void* stream) {
    const char* who = "pd_polar_refine_setup";
    if (int e = shape_args(who, N, H, W)) return e;
    PD_REQUIRE(depth && K_intrinsics && pol_normal && xolp && zeta0 && coef,
               "%s: depth, K, pol_normal, xolp, zeta0 and coef must not be null", who);
    PD_REQUIRE(ldp >= W, "%s: the row pitch ldp = %ld must be at least W = %d", who, ldp, W);
    PD_REQUIRE(std::isfinite(lam) && lam > 0.0, "%s: lam = %g must be finite and > 0", who, lam);
    PD_REQUIRE(std::isfinite(edge_max) && edge_max >= 0.0, "%s: edge_max = %g must be finite and >= 0", who, edge_max);
    PD_REQUIRE(cos_inc > 0.0 && cos_inc <= 1.0, "%s: cos_inc = %g must be in (0, 1]: the cosine of an incidence limit below 90 degrees",
               who, cos_inc);
    PD_REQUIRE(pd::aligned16(pol_normal) && pd::aligned8(zeta0) && pd::aligned8(coef) && pd::aligned8(pq) && pd::aligned4(depth) &&
               pd::aligned4(K_intrinsics) && pd::aligned4(xolp),
               "%s: pol_normal must be 16-byte aligned, zeta0, coef and pq 8-byte aligned, depth, K and xolp 4-byte aligned", who);
    if (int e = ws_args(who, workspace, ws_bytes, N, H, W)) return e;
    if (N == 0) return PD_OK;
    const Geo g = geo_of(H, W);
    SetupArgs a{static_cast<const float*>(depth), static_cast<const float*>(K_intrinsics), static_cast<const float4*>(pol_normal),
                static_cast<const float*>(xolp), static_cast<const unsigned char*>(valid), (size_t)ldp, lam, edge_max, cos_inc};
    hipLaunchKernelGGL(refine_setup_kernel<NoWeight>, dim3((unsigned)(N * tiles_of(H, W))), dim3(RT), 0, (hipStream_t)stream, a, g,
                       static_cast<double*>(zeta0), static_cast<double*>(coef), static_cast<double*>(pq),
                       static_cast<double*>(workspace), NoWeight{});
    return pd::check_launch(who);
}

extern "C" int pd_polar_refine_table(const void* workspace, size_t ws_bytes, double lam, int iters, void* S, void* table, int N,
                                     int H, int W, void* stream) {
    const char* who = "pd_polar_refine_table";
    if (int e = shape_args(who, N, H, W)) return e;
    PD_REQUIRE(S && table, "%s: S and table must not be null", who);
    PD_REQUIRE(std::isfinite(lam) && lam > 0.0, "%s: lam = %g must be finite and > 0", who, lam);
    PD_REQUIRE(iters >= 1, "%s: iters = %d must be at least 1", who, iters);
    PD_REQUIRE(pd::aligned8(S) && pd::aligned8(table), "%s: S and table must be 8-byte aligned", who);
    if (int e = ws_args(who, workspace, ws_bytes, N, H, W)) return e;
    if (N == 0) return PD_OK;
    hipLaunchKernelGGL(refine_table_kernel, dim3((unsigned)N), dim3(RT), 0, (hipStream_t)stream,
                       static_cast<const double*>(workspace), (int)tiles_of(H, W), lam, iters, static_cast<double*>(S),
                       static_cast<double*>(table));
    return pd::check_launch(who);
}

extern "C" int pd_polar_refine_setup_w(const void* depth, const void* K_intrinsics, const void* pol_normal, const void* xolp,
                                       long ldp, const void* valid, double lam, double edge_max, double cos_inc, const void* weight,
                                       double weight_min, double weight_max, void* zeta0, void* coef, void* pq, void* workspace,
                                       size_t ws_bytes, int N, int H, int W, void* stream) {
    const char* who = "pd_polar_refine_setup_w";
    if (int e = shape_args(who, N, H, W)) return e;
    PD_REQUIRE(depth && K_intrinsics && pol_normal && xolp && weight && zeta0 && coef,
               "%s: depth, K, pol_normal, xolp, weight, zeta0 and coef must not be null", who);
    PD_REQUIRE(ldp >= W, "%s: the row pitch ldp = %ld must be at least W = %d", who, ldp, W);
    PD_REQUIRE(std::isfinite(lam) && lam > 0.0, "%s: lam = %g must be finite and > 0", who, lam);
    PD_REQUIRE(std::isfinite(edge_max) && edge_max >= 0.0, "%s: edge_max = %g must be finite and >= 0", who, edge_max);
    PD_REQUIRE(cos_inc > 0.0 && cos_inc <= 1.0, "%s: cos_inc = %g must be in (0, 1]: the cosine of an incidence limit below 90 degrees",
               who, cos_inc);
    PD_REQUIRE(0.0 < weight_min && weight_min <= weight_max && std::isfinite(weight_max),
               "%s: the clamp must be 0 < weight_min <= weight_max < inf, got [%g, %g]", who, weight_min, weight_max);
    PD_REQUIRE(pd::aligned16(pol_normal) && pd::aligned8(zeta0) && pd::aligned8(coef) && pd::aligned8(pq) && pd::aligned4(depth) &&
               pd::aligned4(K_intrinsics) && pd::aligned4(xolp) && pd::aligned4(weight),
               "%s: pol_normal must be 16-byte aligned, zeta0, coef and pq 8-byte aligned, depth, K, xolp and weight 4-byte aligned", who);
    if (int e = ws_args(who, workspace, ws_bytes, N, H, W)) return e;
    if (N == 0) return PD_OK;
    const Geo g = geo_of(H, W);
    SetupArgs a{static_cast<const float*>(depth), static_cast<const float*>(K_intrinsics), static_cast<const float4*>(pol_normal),
                static_cast<const float*>(xolp), static_cast<const unsigned char*>(valid), (size_t)ldp, lam, edge_max, cos_inc};
    const Weight wt{static_cast<const float*>(weight), weight_min, weight_max};
    hipLaunchKernelGGL(refine_setup_kernel<Weight>, dim3((unsigned)(N * tiles_of(H, W))), dim3(RT), 0, (hipStream_t)stream, a, g,
                       static_cast<double*>(zeta0), static_cast<double*>(coef), static_cast<double*>(pq),
                       static_cast<double*>(workspace), wt);
    return pd::check_launch(who);
}

extern "C" int pd_polar_refine_table_w(const void* workspace, size_t ws_bytes, int iters, void* A, void* table, int N, int H, int W,
                                       void* stream) {
    const char* who = "pd_polar_refine_table_w";
    if (int e = shape_args(who, N, H, W)) return e;
    PD_REQUIRE(A && table, "%s: A and table must not be null", who);
    PD_REQUIRE(iters >= 1, "%s: iters = %d must be at least 1", who, iters);
    PD_REQUIRE(pd::aligned8(A) && pd::aligned8(table), "%s: A and table must be 8-byte aligned", who);
    if (int e = ws_args(who, workspace, ws_bytes, N, H, W)) return e;
    if (N == 0) return PD_OK;
    hipLaunchKernelGGL(refine_table_w_kernel, dim3((unsigned)N), dim3(RT), 0, (hipStream_t)stream,
                       static_cast<const double*>(workspace), (int)tiles_of(H, W), iters, static_cast<double*>(A),
                       static_cast<double*>(table));
    return pd::check_launch(who);
}

extern "C" int pd_polar_refine_weights(const void* depth, const void* b, double unc_ref, const void* zeta_prev, const void* zeta0,
                                       double c, void* weight, int N, int H, int W, void* stream) {
    const char* who = "pd_polar_refine_weights";
    if (int e = shape_args(who, N, H, W)) return e;
    PD_REQUIRE(depth && weight, "%s: depth and weight must not be null", who);
    PD_REQUIRE(!b || (std::isfinite(unc_ref) && unc_ref > 0.0), "%s: unc_ref = %g must be finite and > 0 when b is given", who, unc_ref);
    PD_REQUIRE(!zeta_prev == !zeta0, "%s: zeta_prev and zeta0 must both be given or both be null", who);
    PD_REQUIRE(!zeta_prev || (std::isfinite(c) && c > 0.0), "%s: c = %g must be finite and > 0 when zeta_prev is given", who, c);
    PD_REQUIRE(pd::aligned4(depth) && pd::aligned4(b) && pd::aligned4(weight) && pd::aligned8(zeta_prev) && pd::aligned8(zeta0),
               "%s: depth, b and weight must be 4-byte aligned, zeta_prev and zeta0 8-byte aligned", who);
    if (N == 0) return PD_OK;
    const size_t total = (size_t)N * H * W;
    hipLaunchKernelGGL(refine_weights_kernel, dim3((unsigned)((total + RT - 1) / RT)), dim3(RT), 0, (hipStream_t)stream,
                       static_cast<const float*>(depth), static_cast<const float*>(b), unc_ref, static_cast<const double*>(zeta_prev),
                       static_cast<const double*>(zeta0), c, static_cast<float*>(weight), total);
    return pd::check_launch(who);
}

extern "C" int pd_polar_refine_step(const void* coef, const void* table, int iters, int k, const void* zeta_in, void* zeta_out,
                                    void* d, int N, int H, int W, void* stream) {
    const char* who = "pd_polar_refine_step";
    if (int e = shape_args(who, N, H, W)) return e;
    PD_REQUIRE(coef && table && zeta_in && zeta_out && d, "%s: coef, table, zeta_in, zeta_out and d must not be null", who);
    PD_REQUIRE(iters >= 1, "%s: iters = %d must be at least 1", who, iters);
    PD_REQUIRE(k >= 0 && k < iters, "%s: the step k = %d must be in [0, iters = %d)", who, k, iters);
    PD_REQUIRE(zeta_in != zeta_out, "%s: zeta_in and zeta_out must be two buffers (a step reads its neighbours' zeta)", who);
    PD_REQUIRE(pd::aligned8(coef) && pd::aligned8(table) && pd::aligned8(zeta_in) && pd::aligned8(zeta_out) && pd::aligned8(d),
               "%s: coef, table, zeta_in, zeta_out and d must be 8-byte aligned", who);
    if (N == 0) return PD_OK;
    hipLaunchKernelGGL(refine_step_kernel, dim3((unsigned)(N * tiles_of(H, W))), dim3(RT), 0, (hipStream_t)stream,
                       static_cast<const double*>(coef), static_cast<const double*>(table), iters, k,
                       static_cast<const double*>(zeta_in), static_cast<double*>(zeta_out), static_cast<double*>(d), geo_of(H, W));
    return pd::check_launch(who);
}

extern "C" int pd_polar_refine_steps(const void* coef, const void* table, int iters, int k0, int T, const void* zeta_in,
                                     void* zeta_out, const void* d_in, void* d_out, int N, int H, int W, void* stream) {
    const char* who = "pd_polar_refine_steps";
    if (int e = shape_args(who, N, H, W)) return e;
    PD_REQUIRE(coef && table && zeta_in && zeta_out && d_out, "%s: coef, table, zeta_in, zeta_out and d_out must not be null", who);
    PD_REQUIRE(iters >= 1, "%s: iters = %d must be at least 1", who, iters);
    PD_REQUIRE(T >= 1 && T <= PD_POLAR_REFINE_MAX_T, "%s: T = %d must be in [1, %d]", who, T, PD_POLAR_REFINE_MAX_T);
    PD_REQUIRE(k0 >= 0 && k0 <= iters - T, "%s: the steps k0 = %d .. k0 + T - 1 = %d must lie in [0, iters = %d)", who, k0, k0 + T - 1,
               iters);
    PD_REQUIRE(k0 == 0 || d_in, "%s: d_in must not be null unless k0 = 0 (the first step does not read d)", who);
    PD_REQUIRE(zeta_in != zeta_out && d_in != d_out,
               "%s: zeta_in / zeta_out and d_in / d_out must be two buffers each (a workgroup reads its neighbours' pixels)", who);
    PD_REQUIRE(pd::aligned8(coef) && pd::aligned8(table) && pd::aligned8(zeta_in) && pd::aligned8(zeta_out) && pd::aligned8(d_in) &&
               pd::aligned8(d_out), "%s: coef, table, zeta_in, zeta_out, d_in and d_out must be 8-byte aligned", who);
    PD_REQUIRE((double)N * (double)ftiles_of(H, W) < 2147483648.0, "%s: too many tiles (N = %d items of %ld workgroups)", who, N,
               ftiles_of(H, W));
    if (N == 0) return PD_OK;
    Geo g = geo_of(H, W);
    g.tx = (W + FW - 1) / FW; g.ty = (H + FH - 1) / FH;
    const dim3 grid((unsigned)(N * ftiles_of(H, W)));
    const double* cf = static_cast<const double*>(coef);
    const double* tb = static_cast<const double*>(table);
    const double* zi = static_cast<const double*>(zeta_in);
    const double* di = static_cast<const double*>(d_in);
    double* zo = static_cast<double*>(zeta_out);
    double* dd = static_cast<double*>(d_out);
    hipStream_t st = (hipStream_t)stream;
    switch (T) {
#define PD_STEPS_CASE(t) case t: hipLaunchKernelGGL(refine_steps_kernel<t>, grid, dim3(RT), 0, st, cf, tb, iters, k0, zi, zo, di, dd, g); break;
        PD_STEPS_CASE(1) PD_STEPS_CASE(2) PD_STEPS_CASE(3) PD_STEPS_CASE(4)
        PD_STEPS_CASE(5) PD_STEPS_CASE(6) PD_STEPS_CASE(7) PD_STEPS_CASE(8)
#undef PD_STEPS_CASE
    }
    return pd::check_launch(who);
}

extern "C" int pd_polar_refine_finish(const void* depth, const void* coef, const void* zeta, void* depth_out, void* touched,
                                      void* residual, void* workspace, size_t ws_bytes, int N, int H, int W, void* stream) {
    const char* who = "pd_polar_refine_finish";
    if (int e = shape_args(who, N, H, W)) return e;
    PD_REQUIRE(depth && coef && zeta && depth_out && touched && residual,
               "%s: depth, coef, zeta, depth_out, touched and residual must not be null", who);
    PD_REQUIRE(pd::aligned8(coef) && pd::aligned8(zeta) && pd::aligned8(residual) && pd::aligned4(depth) && pd::aligned4(depth_out),
               "%s: coef, zeta and residual must be 8-byte aligned, depth and depth_out 4-byte aligned", who);
    if (int e = ws_args(who, workspace, ws_bytes, N, H, W)) return e;
    if (N == 0) return PD_OK;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(refine_finish_kernel, dim3((unsigned)(N * tiles_of(H, W))), dim3(RT), 0, st,
                       static_cast<const float*>(depth), static_cast<const double*>(coef), static_cast<const double*>(zeta),
                       static_cast<float*>(depth_out), static_cast<unsigned char*>(touched), static_cast<double*>(workspace),
                       geo_of(H, W));
    hipLaunchKernelGGL(refine_max_kernel, dim3((unsigned)N), dim3(RT), 0, st, static_cast<const double*>(workspace),
                       (int)tiles_of(H, W), static_cast<double*>(residual));
    return pd::check_launch(who);
}
