// Demosaic of COLOUR division-of-focal-plane frames on the device (Sony IMX250MYR class: a Bayer colour filter over the
// polarizer array, every 4x4 super-pixel a 2x2 Bayer cell of 2x2 polarizer cells) -> the four polarizer planes of
// ("pol", 0, 0), the uint8 RGB picture of ("color_raw", 0, 0) and, on request, the twelve per-colour polarizer images.
// Definition: include/polardepth.h, pd_cdofp_demosaic; fp64 statement: tests/cdofp_ref.py.
//
// One streaming kernel, bound by its stores and its fp64 arithmetic (1..4 bytes read, 19 or 67 written, about 200 fp64
// operations per mosaic pixel):
//   - a lane owns the four columns 4J .. 4J+3 of one output row and every output of them; each fp32 row segment is one
//     16-byte store (W4 % 4 == 0 aligns every row), each colour row segment one 4-byte store;
//   - capped grid, grid-stride loop over (frame, row, column chunk), as in dofp.hip;
//   - the stencil -- per lane 8 mosaic rows (two lattice rows of each of the four row offsets) x 12 columns (lattice columns
//     J-1, J, J+1) -- is read as 24 aligned 4-element loads through L1 / L2: neighbouring lanes and rows share them, no LDS.
// What is static and what is not: the loop over the 16 sub-lattices (ry, rx) is unrolled, so the column weights and the
// choice between lattice columns are compile-time and every value sits in a register of its own.  The Bayer order is a
// template parameter (four orders), which makes the colour of a sub-lattice static too.  The polarizer layout permutes whole
// planes, so it only moves store addresses; the one place where the order of the planes enters the arithmetic is the colour
// sum ((ch0 + ch1) + (ch2 + ch3)), which depends on the layout through nothing but the site that shares a pair with site 0
// (addition commutes): a uniform three-way choice.
// -ffp-contract=off (Makefile): every product and sum below rounds on its own, in the header's order.
#include "pd_common.h"

#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr long kMaxBlocks = 2048;      // 256 CUs x 8 workgroups; the rest of the work is grid-strided

inline unsigned grid_for(long items) {
    const long b = (items + kThreads - 1) / kThreads;
    return (unsigned)(b > kMaxBlocks ? kMaxBlocks : (b < 1 ? 1 : b));
}

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <typename T> struct chunk4;
template <> struct chunk4<uint8_t> { using type = uint32_t; };
template <> struct chunk4<uint16_t> { using type = u32x2; };
template <> struct chunk4<float> { using type = f32x4; };

struct Args {
    float* planes;          // [B][4][H4][W4] or null
    uint8_t* color;         // [B][3][H4][W4] or null
    float* rgb;             // [B][4][3][H4][W4] or null
    double gains[3];
    double scale;
    int plane_of_site[4];   // layout
    int partner;            // the site whose plane shares a pair of the colour sum with site 0's plane
    long total;             // B * H4 * (W4 / 4)
    int H4, W4;
};

// the Bayer orders as 2 bits per cell c = 2 by + bx
constexpr int kRGGB = 0 | (1 << 2) | (1 << 4) | (2 << 6);
constexpr int kBGGR = 2 | (1 << 2) | (1 << 4) | (0 << 6);
constexpr int kGRBG = 1 | (0 << 2) | (2 << 4) | (1 << 6);
constexpr int kGBRG = 1 | (2 << 2) | (0 << 4) | (1 << 6);

constexpr int colour_of(int order, int c) { return (order >> (2 * c)) & 3; }
// the n-th cell (reading order) of colour k: for green, n = 0 is the one in the upper Bayer row
constexpr int cell_of(int order, int k, int n) {
    for (int c = 0; c < 4; ++c)
        if (colour_of(order, c) == k && n-- == 0) return c;
    return -1;
}

__device__ __forceinline__ int clamp_index(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// four consecutive samples (one aligned access) as doubles
template <typename T>
__device__ __forceinline__ void load4(const T* __restrict__ p, double (&m)[4]) {
    union { typename chunk4<T>::type v; T e[4]; } c;
    c.v = *reinterpret_cast<const typename chunk4<T>::type*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = (double)c.e[j];
}

__device__ __forceinline__ uint32_t to_u8(double c) {
    double r = floor(c + 0.5);
    r = r >= 0.0 ? r : 0.0;          // NaN -> 0
    r = r > 255.0 ? 255.0 : r;
    return (uint32_t)(int)r;
}

template <typename T, int BAYER>
__global__ __launch_bounds__(kThreads) void cdofp_kernel(const T* __restrict__ mosaic, const Args a) {
    const int H4 = a.H4, W4 = a.W4;
    const int nx = W4 / 4, ny = H4 / 4;
    const long plane = (long)H4 * W4;
    for (long i = blockIdx.x * (long)kThreads + threadIdx.x; i < a.total; i += (long)gridDim.x * kThreads) {
        const int J = (int)(i % nx);
        const long t = i / nx;
        const int y = (int)(t % H4);
        const long b = t / H4;
        const T* frame = mosaic + b * plane;
        const int jc[3] = {4 * clamp_index(J - 1, nx), 4 * J, 4 * clamp_index(J + 1, nx)};
        // q[site][cell][column]: the interpolated sub-lattice of polarizer site 2 (ry & 1) + (rx & 1) and Bayer cell
        // 2 (ry >> 1) + (rx >> 1) at the lane's four columns
        double q[4][4][4];
#pragma unroll
        for (int ry = 0; ry < 4; ++ry) {
            const int d = y - ry;                      // >= -3: the shift and the mask below are floor and modulo
            const int ty = d & 3, i0 = d >> 2;
            const double wy0 = (double)(4 - ty), wy1 = (double)ty;
            const T* top = frame + (4 * clamp_index(i0, ny) + ry) * W4;      // row * W4 < H4 * W4 <= 2^30
            const T* bot = frame + (4 * clamp_index(i0 + 1, ny) + ry) * W4;
            double st[3][4], sb[3][4];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                load4<T>(top + jc[j], st[j]);
                load4<T>(bot + jc[j], sb[j]);
            }
#pragma unroll
            for (int rx = 0; rx < 4; ++rx) {
#pragma unroll
                for (int xx = 0; xx < 4; ++xx) {
                    const int j0 = xx < rx ? 0 : 1;                          // lattice column J - 1 or J
                    const double wx1 = (double)((xx - rx) & 3), wx0 = 4.0 - wx1;
                    q[2 * (ry & 1) + (rx & 1)][2 * (ry >> 1) + (rx >> 1)][xx] =
                        ((wy0 * ((wx0 * st[j0][rx]) + (wx1 * st[j0 + 1][rx]))) +
                         (wy1 * ((wx0 * sb[j0][rx]) + (wx1 * sb[j0 + 1][rx])))) * 0.0625;
                }
            }
        }
        constexpr int cR = cell_of(BAYER, 0, 0), cG0 = cell_of(BAYER, 1, 0), cG1 = cell_of(BAYER, 1, 1),
                      cB = cell_of(BAYER, 2, 0);
        double ch[4][3][4];      // [site][colour][column]
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int xx = 0; xx < 4; ++xx) {
                ch[s][0][xx] = q[s][cR][xx] * a.gains[0];
                ch[s][1][xx] = ((q[s][cG0][xx] + q[s][cG1][xx]) * 0.5) * a.gains[1];
                ch[s][2][xx] = q[s][cB][xx] * a.gains[2];
            }
        }
        const int off = y * W4 + 4 * J;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const long p = a.plane_of_site[s];
            if (a.planes) {
                float o[4];
#pragma unroll
                for (int xx = 0; xx < 4; ++xx)
                    o[xx] = (float)((((19595.0 * ch[s][0][xx]) + (38470.0 * ch[s][1][xx])) + (7471.0 * ch[s][2][xx])) *
                                    (1.0 / 65536.0));
                *reinterpret_cast<f32x4*>(a.planes + (b * 4 + p) * plane + off) = f32x4{o[0], o[1], o[2], o[3]};
            }
            if (a.rgb) {
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    *reinterpret_cast<f32x4*>(a.rgb + (b * 12 + p * 3 + k) * plane + off) =
                        f32x4{(float)ch[s][k][0], (float)ch[s][k][1], (float)ch[s][k][2], (float)ch[s][k][3]};
            }
        }
        if (a.color) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                uint32_t word = 0;
#pragma unroll
                for (int xx = 0; xx < 4; ++xx) {
                    const double c1 = ch[1][k][xx], c2 = ch[2][k][xx], c3 = ch[3][k][xx];
                    const double mate = a.partner == 1 ? c1 : (a.partner == 2 ? c2 : c3);
                    const double u = a.partner == 1 ? c2 : c1, v = a.partner == 3 ? c2 : c3;
                    const double c = (((ch[0][k][xx] + mate) + (u + v)) * 0.25) * a.scale;
                    word |= to_u8(c) << (8 * xx);
                }
                *reinterpret_cast<uint32_t*>(a.color + (b * 3 + k) * plane + off) = word;
            }
        }
    }
}

template <typename T>
void launch(const void* mosaic, const Args& a, int order, hipStream_t st) {
    const dim3 grid(grid_for(a.total)), block(kThreads);
    const T* m = (const T*)mosaic;
    switch (order) {
        case kRGGB: hipLaunchKernelGGL((cdofp_kernel<T, kRGGB>), grid, block, 0, st, m, a); break;
        case kBGGR: hipLaunchKernelGGL((cdofp_kernel<T, kBGGR>), grid, block, 0, st, m, a); break;
        case kGRBG: hipLaunchKernelGGL((cdofp_kernel<T, kGRBG>), grid, block, 0, st, m, a); break;
        default: hipLaunchKernelGGL((cdofp_kernel<T, kGBRG>), grid, block, 0, st, m, a); break;
    }
}

}  // namespace

extern "C" int pd_cdofp_demosaic(const void* mosaic, int dtype, const int* layout, const int* bayer, const double* gains,
                                 double color_scale, void* planes, void* color_u8, void* rgb_planes, int B, int H4, int W4,
                                 void* stream) {
    if (B == 0) return PD_OK;
    PD_REQUIRE(B > 0, "pd_cdofp_demosaic: bad shape (B = %d)", B);
    PD_REQUIRE(dtype == PD_POLAR_U8 || dtype == PD_POLAR_U16 || dtype == PD_POLAR_F32,
               "pd_cdofp_demosaic: unknown dtype %d (PD_POLAR_U8 / _U16 / _F32)", dtype);
    PD_REQUIRE(mosaic && layout && bayer, "pd_cdofp_demosaic: mosaic, layout and bayer must not be null");
    PD_REQUIRE(planes || color_u8 || rgb_planes,
               "pd_cdofp_demosaic: planes, color_u8 and rgb_planes must not all be null");
    Args a{};
    unsigned seen = 0;
    int site_of_plane[4] = {0, 0, 0, 0};
    for (int s = 0; s < 4; ++s) {
        const int p = layout[s];
        PD_REQUIRE(p >= 0 && p < 4 && !(seen & (1u << p)),
                   "pd_cdofp_demosaic: layout (%d,%d,%d,%d) is not a permutation of 0..3", layout[0], layout[1], layout[2],
                   layout[3]);
        seen |= 1u << p;
        a.plane_of_site[s] = p;
        site_of_plane[p] = s;
    }
    a.partner = site_of_plane[a.plane_of_site[0] ^ 1];      // planes pair up as (0, 1) and (2, 3)
    int order = 0;
    bool colours = true;
    for (int c = 0; c < 4; ++c) {
        colours = colours && bayer[c] >= 0 && bayer[c] <= 2;
        order |= (bayer[c] & 3) << (2 * c);
    }
    PD_REQUIRE(colours && (order == kRGGB || order == kBGGR || order == kGRBG || order == kGBRG),
               "pd_cdofp_demosaic: bayer (%d,%d,%d,%d) is not a Bayer order (0 = R, 1 = G, 2 = B: one R, one B, two G on a "
               "diagonal)", bayer[0], bayer[1], bayer[2], bayer[3]);
    for (int k = 0; k < 3; ++k) {
        a.gains[k] = gains ? gains[k] : 1.0;
        PD_REQUIRE(std::isfinite(a.gains[k]), "pd_cdofp_demosaic: gains must be finite, got (%g,%g,%g)", gains[0], gains[1],
                   gains[2]);
    }
    PD_REQUIRE(std::isfinite(color_scale) && color_scale > 0.0,
               "pd_cdofp_demosaic: color_scale must be finite and greater than 0, got %g", color_scale);
    a.scale = color_scale;
    PD_REQUIRE(H4 >= 4 && W4 >= 4 && H4 % 4 == 0 && W4 % 4 == 0,
               "pd_cdofp_demosaic: the mosaic's sides must be multiples of 4 and >= 4, got %d x %d", H4, W4);
    // in-frame offsets are 32-bit in the kernel, plane, frame and work counters 64-bit: the limits of pd_dofp_demosaic
    PD_REQUIRE((long)H4 * W4 <= (1L << 30) && (long)B * H4 * W4 <= (1L << 40),
               "pd_cdofp_demosaic: %d frames of %d x %d are too large for the kernel's index arithmetic", B, H4, W4);
    PD_REQUIRE(pd::aligned16(mosaic) && pd::aligned16(planes) && pd::aligned16(color_u8) && pd::aligned16(rgb_planes),
               "pd_cdofp_demosaic: mosaic, planes, color_u8 and rgb_planes must be 16-byte aligned");
    a.planes = (float*)planes;
    a.color = (uint8_t*)color_u8;
    a.rgb = (float*)rgb_planes;
    a.total = (long)B * H4 * (W4 / 4);
    a.H4 = H4;
    a.W4 = W4;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == PD_POLAR_U8) launch<uint8_t>(mosaic, a, order, st);
    else if (dtype == PD_POLAR_U16) launch<uint16_t>(mosaic, a, order, st);
    else launch<float>(mosaic, a, order, st);
    return pd::check_launch("pd_cdofp_demosaic");
}
