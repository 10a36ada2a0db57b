// Demosaic of division-of-focal-plane (DoFP) polarizer frames on the device: the interleaved 2x2 super-pixel mosaic a
// polarization sensor emits (Sony IMX250MZR: 90/45/135/0 degrees in reading order) -> the four planes of ("pol", 0, 0).
// Definition: include/polardepth.h, pd_dofp_demosaic; fp64 statement: tests/dofp_ref.py.
//
// Both modes are streaming kernels bound by their stores (bilinear writes 16 of its 17..20 bytes per mosaic pixel):
//   - a lane owns several consecutive output columns of one row and stores all four planes, 16 bytes per plane where the
//     rows are 16-byte aligned (only the base pointers are: W2 = 6 uint8 is legal), narrower where they are not;
//   - capped grid, grid-stride loop over (frame, row, column chunk);
//   - the bilinear neighbour rows are re-read through L1 / L2 (three rows of one chunk per lane; consecutive rows of a
//     frame are taken by consecutive chunks of work, i.e. by the same or a neighbouring workgroup at the same time): no LDS.
// Per mosaic pixel the bilinear mode forms four numbers in fp64 -- the sample itself, the mean of its left / right, of its
// upper / lower and of its four diagonal neighbours -- and each plane takes the one its site parity selects; the four
// planes of a pixel take four different ones.  -ffp-contract=off (Makefile); nothing here could contract anyway.
#include "pd_common.h"

namespace {

constexpr int kThreads = 256;
constexpr long kMaxBlocks = 2048;      // 256 CUs x 8 workgroups; the rest of the work is grid-strided

inline unsigned grid_for(long items) {
    const long b = (items + kThreads - 1) / kThreads;
    return (unsigned)(b > kMaxBlocks ? kMaxBlocks : (b < 1 ? 1 : b));
}

// plain vector types (no constructors: they sit in unions with their elements)
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int BYTES> struct vec_of;
template <> struct vec_of<1> { using type = uint8_t; };
template <> struct vec_of<2> { using type = uint16_t; };
template <> struct vec_of<4> { using type = uint32_t; };
template <> struct vec_of<8> { using type = u32x2; };
template <> struct vec_of<16> { using type = u32x4; };

// ---------------------------------------------------------------------------------------------------- super-pixel
// planes[b][p][y][x] = mosaic[b][2y + r_p][2x + c_p].  A lane reads 2 rows x 2K elements and writes K elements to each of
// the four planes, K * sizeof(T) = 16, 8, 4, 2 or 1 bytes: the host picks the largest K that divides the plane width, which
// makes every access of that width aligned.  sites: bits 2p, 2p+1 = 2 r_p + c_p.
template <typename T, int K>
__global__ __launch_bounds__(kThreads) void dofp_superpixel_kernel(const T* __restrict__ mosaic, T* __restrict__ planes,
                                                                   unsigned sites, long total, int h, int w) {
    using V = typename vec_of<K * (int)sizeof(T)>::type;
    const int chunks = w / K;
    const int W2 = 2 * w;
    const long plane = (long)h * w;
    for (long i = blockIdx.x * (long)kThreads + threadIdx.x; i < total; i += (long)gridDim.x * kThreads) {
        const int cx = (int)(i % chunks);
        const long t = i / chunks;
        const int y = (int)(t % h);
        const long b = t / h;
        const T* src = mosaic + b * 4 * plane + (2 * y) * W2 + 2 * K * cx;      // (2y) * W2 < H2 * W2 <= 2^30
        union { V v[2]; T e[2 * K]; } row[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            row[r].v[0] = *reinterpret_cast<const V*>(src + r * W2);
            row[r].v[1] = *reinterpret_cast<const V*>(src + r * W2 + K);
        }
        T* dst = planes + b * 4 * plane + y * w + K * cx;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const unsigned s = (sites >> (2 * p)) & 3u;
            union { V v; T e[K]; } out;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const T a = (s & 1u) ? row[0].e[2 * j + 1] : row[0].e[2 * j];
                const T c = (s & 1u) ? row[1].e[2 * j + 1] : row[1].e[2 * j];
                out.e[j] = (s & 2u) ? c : a;
            }
            *reinterpret_cast<V*>(dst + p * plane) = out.v;
        }
    }
}

// ------------------------------------------------------------------------------------------------------- bilinear
// index -1 reads 1, index n reads n - 2 (mirror about the edge sample: the site parity survives); anything further out --
// the columns past the end of a row's last, partial chunk, whose results are not stored -- is held inside the row
__device__ __forceinline__ int mirror(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i < 0 ? 0 : i;
}

template <typename T> struct chunk4;
template <> struct chunk4<uint8_t> { using type = uint32_t; };
template <> struct chunk4<uint16_t> { using type = u32x2; };
template <> struct chunk4<float> { using type = f32x4; };

// the six samples m[xs[0..5]] = columns x0-1 .. x0+4 of one row (mirrored by the caller) as doubles; ALIGNED: x0..x0+3 in
// one aligned access of 4 elements
template <typename T, bool ALIGNED>
__device__ __forceinline__ void load_row(const T* __restrict__ row, int x0, int xl, int xr, int W2, double (&m)[6]) {
    if constexpr (ALIGNED) {
        union { typename chunk4<T>::type v; T e[4]; } c;
        c.v = *reinterpret_cast<const typename chunk4<T>::type*>(row + x0);
        m[0] = (double)row[xl];
#pragma unroll
        for (int j = 0; j < 4; ++j) m[1 + j] = (double)c.e[j];
        m[5] = (double)row[xr];
    } else {
        m[0] = (double)row[xl];
#pragma unroll
        for (int j = 0; j < 4; ++j) m[1 + j] = (double)row[mirror(x0 + j, W2)];
        m[5] = (double)row[xr];
    }
}

// A lane owns columns x0 .. x0+3 (x0 % 4 == 0) of row y in all four planes.  ALIGNED (W2 % 4 == 0): every row of the input
// and of the output starts on a multiple of 4 elements, the chunk is one load and each plane one 16-byte store.  Otherwise
// (W2 % 4 == 2: rows start on multiples of 2 elements) element loads and 8-byte stores, the last chunk of a row holding
// two columns.
template <typename T, bool ALIGNED>
__global__ __launch_bounds__(kThreads) void dofp_bilinear_kernel(const T* __restrict__ mosaic, float* __restrict__ planes,
                                                                 unsigned sites, long total, int H2, int W2) {
    const int chunks = (W2 + 3) / 4;
    const long plane = (long)H2 * W2;
    for (long i = blockIdx.x * (long)kThreads + threadIdx.x; i < total; i += (long)gridDim.x * kThreads) {
        const int cx = (int)(i % chunks);
        const long t = i / chunks;
        const int y = (int)(t % H2);
        const long b = t / H2;
        const int x0 = 4 * cx;
        const int xl = mirror(x0 - 1, W2), xr = mirror(x0 + 4, W2);
        const T* frame = mosaic + b * plane;
        double up[6], mid[6], dn[6];
        load_row<T, ALIGNED>(frame + mirror(y - 1, H2) * W2, x0, xl, xr, W2, up);      // row * W2 < H2 * W2 <= 2^30
        load_row<T, ALIGNED>(frame + y * W2, x0, xl, xr, W2, mid);
        load_row<T, ALIGNED>(frame + mirror(y + 1, H2) * W2, x0, xl, xr, W2, dn);
        // v[k][j], k = 2 dy + dx: the value of column x0 + j for a plane whose site is dy rows and dx columns away (mod 2)
        float v[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[0][j] = (float)mid[1 + j];
            v[1][j] = (float)((mid[j] + mid[2 + j]) * 0.5);
            v[2][j] = (float)((up[1 + j] + dn[1 + j]) * 0.5);
            v[3][j] = (float)(((up[j] + up[2 + j]) + (dn[j] + dn[2 + j])) * 0.25);
        }
        float* dst = planes + b * 4 * plane + y * W2 + x0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const unsigned s = (sites >> (2 * p)) & 3u;
            const bool dy = (((unsigned)y ^ (s >> 1)) & 1u) != 0;
            const bool cp = (s & 1u) != 0;          // x0 is even: column x0 + j is dx = (j ^ c_p) & 1 away
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool dx = ((j & 1) != 0) != cp;
                o[j] = dy ? (dx ? v[3][j] : v[2][j]) : (dx ? v[1][j] : v[0][j]);
            }
            float* q = dst + p * plane;
            if constexpr (ALIGNED) {
                *reinterpret_cast<f32x4*>(q) = f32x4{o[0], o[1], o[2], o[3]};
            } else {
                *reinterpret_cast<f32x2*>(q) = f32x2{o[0], o[1]};
                if (x0 + 2 < W2) *reinterpret_cast<f32x2*>(q + 2) = f32x2{o[2], o[3]};
            }
        }
    }
}

template <typename T, int K>
void launch_superpixel_k(const void* mosaic, void* planes, unsigned sites, int B, int h, int w, hipStream_t st) {
    const long total = (long)B * h * (w / K);
    hipLaunchKernelGGL((dofp_superpixel_kernel<T, K>), dim3(grid_for(total)), dim3(kThreads), 0, st, (const T*)mosaic,
                       (T*)planes, sites, total, h, w);
}

// the widest access (at most 16 bytes) whose element count divides the plane width
template <typename T>
void launch_superpixel(const void* mosaic, void* planes, unsigned sites, int B, int h, int w, hipStream_t st) {
    if constexpr (sizeof(T) == 1)
        if (w % 16 == 0) return launch_superpixel_k<T, 16>(mosaic, planes, sites, B, h, w, st);
    if constexpr (sizeof(T) <= 2)
        if (w % 8 == 0) return launch_superpixel_k<T, 8>(mosaic, planes, sites, B, h, w, st);
    if (w % 4 == 0) return launch_superpixel_k<T, 4>(mosaic, planes, sites, B, h, w, st);
    if (w % 2 == 0) return launch_superpixel_k<T, 2>(mosaic, planes, sites, B, h, w, st);
    launch_superpixel_k<T, 1>(mosaic, planes, sites, B, h, w, st);
}

template <typename T>
void launch_bilinear(const void* mosaic, void* planes, unsigned sites, int B, int H2, int W2, hipStream_t st) {
    const long total = (long)B * H2 * ((W2 + 3) / 4);
    if (W2 % 4 == 0)
        hipLaunchKernelGGL((dofp_bilinear_kernel<T, true>), dim3(grid_for(total)), dim3(kThreads), 0, st, (const T*)mosaic,
                           (float*)planes, sites, total, H2, W2);
    else
        hipLaunchKernelGGL((dofp_bilinear_kernel<T, false>), dim3(grid_for(total)), dim3(kThreads), 0, st, (const T*)mosaic,
                           (float*)planes, sites, total, H2, W2);
}

}  // namespace

extern "C" int pd_dofp_demosaic(const void* mosaic, int dtype, void* planes, int mode, const int* layout, int B, int H2,
                                int W2, void* stream) {
    PD_REQUIRE(B >= 0, "pd_dofp_demosaic: bad shape (B = %d)", B);
    PD_REQUIRE(dtype == PD_POLAR_U8 || dtype == PD_POLAR_U16 || dtype == PD_POLAR_F32,
               "pd_dofp_demosaic: unknown dtype %d (PD_POLAR_U8 / _U16 / _F32)", dtype);
    PD_REQUIRE(mode == PD_DOFP_SUPERPIXEL || mode == PD_DOFP_BILINEAR,
               "pd_dofp_demosaic: unknown mode %d (PD_DOFP_SUPERPIXEL / PD_DOFP_BILINEAR)", mode);
    if (B == 0) return PD_OK;
    PD_REQUIRE(mosaic && planes && layout, "pd_dofp_demosaic: mosaic, planes and layout must not be null");
    unsigned seen = 0, sites = 0;
    for (int s = 0; s < 4; ++s) {
        const int p = layout[s];
        PD_REQUIRE(p >= 0 && p < 4 && !(seen & (1u << p)),
                   "pd_dofp_demosaic: layout (%d,%d,%d,%d) is not a permutation of 0..3", layout[0], layout[1], layout[2],
                   layout[3]);
        seen |= 1u << p;
        sites |= (unsigned)s << (2 * p);      // plane p is fed by the site s = 2 r + c
    }
    PD_REQUIRE(H2 >= 2 && W2 >= 2 && H2 % 2 == 0 && W2 % 2 == 0,
               "pd_dofp_demosaic: the mosaic must have even sides >= 2, got %d x %d", H2, W2);
    // in-frame offsets are 32-bit in the kernels (4 planes of a frame: 64-bit), frame and work counters 64-bit
    PD_REQUIRE((long)H2 * W2 <= (1L << 30) && (long)B * H2 * W2 <= (1L << 40),
               "pd_dofp_demosaic: %d frames of %d x %d are too large for the kernel's index arithmetic", B, H2, W2);
    PD_REQUIRE(pd::aligned16(mosaic) && pd::aligned16(planes), "pd_dofp_demosaic: mosaic and planes must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (mode == PD_DOFP_SUPERPIXEL) {
        if (dtype == PD_POLAR_U8) launch_superpixel<uint8_t>(mosaic, planes, sites, B, H2 / 2, W2 / 2, st);
        else if (dtype == PD_POLAR_U16) launch_superpixel<uint16_t>(mosaic, planes, sites, B, H2 / 2, W2 / 2, st);
        else launch_superpixel<uint32_t>(mosaic, planes, sites, B, H2 / 2, W2 / 2, st);      // a copy: floats move as bits
    } else {
        if (dtype == PD_POLAR_U8) launch_bilinear<uint8_t>(mosaic, planes, sites, B, H2, W2, st);
        else if (dtype == PD_POLAR_U16) launch_bilinear<uint16_t>(mosaic, planes, sites, B, H2, W2, st);
        else launch_bilinear<float>(mosaic, planes, sites, B, H2, W2, st);
    }
    return pd::check_launch("pd_dofp_demosaic");
}
