/*
 * polardepth.h -- C ABI of libpolardepth.so (MI355X / gfx950 hot path).
 *
 * Drop-in boundary for the polarimetric depth hot path.  The reference
 * (kkaytekin/Supervised-Depth-Estimation-from-Polarized-Images) is pure Python on
 * PyTorch and has no FFI of its own; the entry points below are what a ctypes
 * binding inside the reference's modules would call (INTEGRATION.md shows the
 * stubs).  Each entry point cites the reference code it replaces
 * (paths relative to the reference checkout).
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes only, no framework types;
 *   - device pointers come from the caller (e.g. tensor.data_ptr()); the caller
 *     owns every buffer including workspaces; nothing is allocated or freed here;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*); no entry point
 *     synchronises the device;
 *   - return 0 on success, a negative PD_E* code on failure; the message is
 *     available from pd_last_error() (thread-local);
 *   - re-entrant: no global mutable state (the only process-wide data are read-only lookup tables and idempotent
 *     hipFuncSetAttribute bookkeeping); the library reads NO environment variable -- every choice a caller can make
 *     (kernel family / arithmetic, measurement variants) is an argument of the entry point it concerns.
 */
#ifndef POLARDEPTH_H
#define POLARDEPTH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PD_OK 0
#define PD_EINVAL (-22)  /* bad argument (shape, alignment, null pointer) */
#define PD_ELAUNCH (-5)  /* HIP reported a launch error */

const char* pd_last_error(void);
int pd_version(void);

/* ------------------------------------------------------------------------- K1
 * Fused Stokes / DoLP / AoLP / physical-normals kernel.
 *
 * Replaces, in one pass over the four polarizer planes:
 *   polarisation/xolp.py:8-34            Iun_and_xolp   (mode PD_POLAR_LS)
 *   manydepth/datasets/indoor_dataset.py:430-442  IndoorDataset.get_xolp
 *   ppp_code/physical_normals_channels.py:15-36   PolarisationImage_channel (mode PD_POLAR_STOKES)
 *   manydepth/normals_vec.py:11-60       rho_diffuse / rho_spec / calc_normals
 *   manydepth/networks/pre_encoders.py:78-79,99-113  normalizeInput('XOLP') / get_normals
 *
 * Tables: a packed, position-independent blob (AoLP LUT over (I0-I90, I45-I135)
 * plus the three theta(rho) interpolation tables with scipy interp1d
 * 'linear'/'extrapolate' semantics).  Build it on the host with one of the two
 * functions below, copy it to the device once, and pass the device pointer.
 */
#define PD_POLAR_LS 0
#define PD_POLAR_STOKES 1
/* flags: default (0) = fp32 theta trig (two-float bin constants, |err| <= ~3e-7; cos/sin(phi) from a LUT,
 * cos/sin(phi+pi/2) by identity); PD_POLAR_PRECISE_NORMALS = fp64 sin/cos(theta) rounded once and
 * cos/sin(fl32(phi+pi/2)) like the reference (~1e-7, slower: ALU-bound).  DoLP / AoLP / index maps are
 * bit-exact in both. */
#define PD_POLAR_PRECISE_NORMALS 1
/* PD_POLAR_IEEE_RHO = evaluate the reference's fp64 sqrt/div sequence for every pixel instead of the
 * Newton-refined hardware seeds with a rounding test (same bits, ~1.3x the arithmetic); the exhaustive test
 * compares the two over all 2^32 uint8 quadruples. */
#define PD_POLAR_IEEE_RHO 2
/* measurement only (tools/bench_polar.py): force the nontemporal hint on / off the plane loads of the training step's
 * instantiation; by default launches of up to 32 frames' worth of 512x640 output carry it. */
#define PD_POLAR_NT_LOADS 4
#define PD_POLAR_PLAIN_LOADS 8

/* bytes needed for the table blob with n_d / n_s1 / n_s2 table nodes */
size_t pd_polar_tables_bytes(int n_d, int n_s1, int n_s2);
/* Pack caller-computed tables (x ascending, y), e.g. the NumPy ones of normals_vec.py:13-47. */
int pd_polar_tables_pack(const double* x_d, const double* y_d, int n_d,
                         const double* x_s1, const double* y_s1, int n_s1,
                         const double* x_s2, const double* y_s2, int n_s2,
                         void* host_blob, size_t blob_bytes);
/* Compute the tables with libm for refractive index n (1000 theta nodes, normals_vec.py:13,27)
 * and pack them.  *blob_bytes_out receives the size actually used. */
int pd_polar_tables_build(double n, void* host_blob, size_t blob_bytes, size_t* blob_bytes_used);

/*
 * pol        [B,4,H,W] uint8 device, planes in 0/45/90/135 degree order (pol00, pol01, pol10, pol11)
 * mask       [B,H,W] uint8 device or NULL (STOKES mode: outputs are 0 where mask == 0)
 * xolp       [B,2,H,W] fp32 or NULL   ch0 DoLP, ch1 AoLP      == inputs[("xolp",0,0)].float()
 * xolp_std   [B,2,H,W] fp32 or NULL   (xolp-0.08693199701957657)/0.44430732785457433
 * normals    [B,9,H,W] fp32 or NULL   cat(N_diff, N_spec1, N_spec2)   == get_normals(xolp).float()
 * ints       [B,5,H,W] int32 or NULL  exact by-products: d1, d2, idx_diffuse, idx_spec1, idx_spec2
 * tables     device copy of the blob
 * Wout    row pitch (in pixels) of every OUTPUT plane, Wout >= W (0 means W).  Wout > W writes the
 *         W real columns and zero-fills the Wout-W padding columns: the 512x612 HAMMER planes land
 *         directly in the 512x640 tensors the network needs (multiples of 32, trainer.py:107-108).
 * H*W must be a multiple of 4 (W and Wout multiples of 4 when they differ); pointers 16-byte aligned.
 */
int pd_polar_fwd(const void* pol, const void* mask, void* xolp, void* xolp_std, void* normals,
                 void* ints, const void* tables, size_t tables_bytes,
                 int B, int H, int W, int Wout, int mode, int flags, void* stream);

/* get_normals() on an existing fp32 XOLP tensor (pre_encoders.py:99-113, the path taken when a
 * data loader already produced inputs[("xolp",0,0)]): xolp [B,2,H,W] -> normals [B,9,H,W]. */
int pd_polar_normals_from_xolp(const void* xolp, void* normals, const void* tables, size_t tables_bytes,
                               int B, int H, int W, int flags, void* stream);

/* calc_normals (manydepth/normals_vec.py:53-60): out [B,3,P] = (cos(phi) sin(theta), sin(phi) sin(theta), cos(theta)) for
 * phi, theta [B,P].  Element types as torch promotes them there: *_f64 != 0 marks an fp64 operand; the output is fp64 when
 * either operand is (the reference's get_normals hands over an fp32 phi and an fp64 theta: cos(phi) is evaluated in fp32
 * and promoted, normals_vec.py:56-58), fp32 otherwise. */
int pd_polar_calc_normals(const void* phi, const void* theta, void* out, int B, long P, int phi_f64, int theta_f64,
                          void* stream);

/* rho_diffuse / rho_spec as functions of their own (manydepth/normals_vec.py:11-22, 25-50): rho fp32 [n] ->
 * theta_d, theta_s1, theta_s2 fp64 [n] (each may be NULL) = scipy interp1d(fill_value="extrapolate") of the three
 * tables, evaluated in scipy's operation order (slope * (rho - x_lo) + y_lo, fp64), so rho beyond a table extrapolates
 * exactly like the reference (theta_s1 up to +41 rad, theta_s2 down to -135 rad for DoLP ~ 2).  bins: optional int32
 * [3][n], the clip(searchsorted(x, rho, 'left'), 1, n-1) index of each table.  NaN rho sorts last like numpy. */
int pd_polar_theta(const void* rho, void* theta_d, void* theta_s1, void* theta_s2, void* bins,
                   const void* tables, size_t tables_bytes, long n, void* stream);

/* General polarizer angles and 8-bit / 16-bit / fp32 intensities (polarisation/xolp.py:8-34 for any four angles).
 *
 * pd_polar_fit_matrix (host only, no GPU): coef_out = row-major 3x4 coefficients P = (A^T A)^-1 A^T of the least-squares
 * fit I(theta) = x0 + x1 cos 2theta + x2 sin 2theta, A = [1, cos 2theta_j, sin 2theta_j] with |a| < 4 DBL_EPSILON snapped to 0
 * and |p| < 1e-12 max|p| snapped to 0 (0/45/90/135 degrees give exactly .25 .25 .25 .25 / .5 0 -.5 0 / 0 .5 0 -.5).
 * Non-finite angles and angle sets of rank < 3 (e.g. 0/90/180/270 degrees) return PD_EINVAL. */
int pd_polar_fit_matrix(const double angles_rad[4], double coef_out[12]);

#define PD_POLAR_U8 0
#define PD_POLAR_U16 1
#define PD_POLAR_F32 2
/*
 * pol        [B,4,H,W] device, element type `dtype` (PD_POLAR_U8 / _U16 / _F32), planes in the order of the angles
 *            given to pd_polar_fit_matrix
 * coef       HOST pointer to the 12 coefficients; read during the call and passed as kernel arguments (no allocation,
 *            copy or synchronisation: the call can be captured into a graph)
 * iun        [B,1,H,Wout] fp32 or NULL   (Imax + Imin) / 2
 * xolp / xolp_std / normals / tables / Wout   as for pd_polar_fwd; tables may be NULL unless normals are requested
 * Per pixel, in fp64 without contraction: x_k = ((P[k][0] I0 + P[k][1] I1) + P[k][2] I2) + P[k][3] I3,
 * r = sqrt(x1^2 + x2^2), Imax = x0 + r, Imin = x0 - r, Iun = (Imax + Imin) / 2, rho = (Imax - Imin) / (Imax + Imin) with
 * inf and NaN -> 0, phi = 0.5 atan2(x2, x1); each rounded once to fp32.  xolp_std and the normals derive from the fp32
 * rho, phi exactly as pd_polar_normals_from_xolp does.  flags: PD_POLAR_PRECISE_NORMALS only.  Shape, alignment and size
 * rules of pd_polar_fwd.
 */
int pd_polar_general_fwd(const void* pol, int dtype, const double* coef, void* iun, void* xolp, void* xolp_std,
                         void* normals, const void* tables, size_t tables_bytes,
                         int B, int H, int W, int Wout, int flags, void* stream);

/* XOLP statistics (csrc/xolp_stats.hip): the DoLP / AoLP distribution of the tensor the network sees, in one read pass on the
 * device.  Replaces polarisation/xolp_mean_and_std_dev.py:10-32 (np.mean / np.std over a stack of .npy frames, whose output
 * are the constants of normalizeInput('XOLP')) for any input K1 accepts, and counts what lies outside the zenith tables.
 *
 * xolp       fp32 [B,2,H,ld] device, ch0 = DoLP (rho), ch1 = AoLP (phi): what pd_polar_fwd / pd_polar_general_fwd write, or
 *            any other fp32 tensor.  The first W <= ld columns of a row are data; the ld - W padding columns are never read
 *            into a statistic (612 -> 640).  ld % 4 == 0; W is arbitrary.
 * mask       uint8 [B,H,ld] device or NULL; non-zero = the pixel counts
 * stats      the record below, on the device (PD_XOLP_STATS_BYTES)
 * workspace  caller-owned, >= pd_xolp_stats_workspace(B, H, W) bytes (monotone in each argument, never 0); scratch
 * thresholds two finite HOST floats, read during the call: over[i] counts rho > thresholds[i] (strictly greater)
 * accumulate 0: `stats` is overwritten; otherwise this call's finalised values are added to it (one fp64 add per sum,
 *            integer adds, min / max), so a whole data set accumulates on the device without a host read
 *
 * A pixel is INCLUDED when it is inside W, passes the mask and both its values are finite.  A pixel that fails only the
 * finiteness test adds 1 to `nonfinite` and to nothing else.  The record, byte offsets:
 *      0  int64   n             included pixels
 *      8  int64   nonfinite
 *     16  int64   over[2]       included pixels with rho > thresholds[0] / thresholds[1]
 *     32  double  sum_rho, sum_rho2, sum_phi, sum_phi2      over included pixels; every fp32 value is converted to fp64 first
 *                               (its square is then exact)
 *     64  float   min_rho, max_rho, min_phi, max_phi        +inf / -inf / +inf / -inf while n == 0
 *     80  uint64  hist_dolp[257]   k = rho < 0 ? 0 : (rho >= 1 ? 256 : (int)(rho * 256.0f)): 256 bins over [0,1), one for
 *                               rho >= 1; the product is exact in fp32 and -0.0 lands in bin 0
 *   2136  uint64  hist_aolp[256]   t = (phi + C1) * C2 in fp32, in that order, C1 = (float)(pi / 2), C2 = (float)(256 / pi);
 *                               k = t < 0 ? 0 : (t >= 256 ? 255 : (int)t)
 * The four sums are bit-reproducible from run to run: lanes, waves and workgroups add their partial sums in a fixed order
 * that depends on the shape only, the per-workgroup partials go through `workspace`, and a second small launch adds them in
 * index order in fp64 -- no floating-point atomics.  Any order of N exactly converted terms errs by at most
 * (N - 1) 2^-53 sum|x|.  The integer fields and the extrema do not depend on the order.
 * B == 0 returns PD_OK (accumulate == 0: writes the empty record).  Two launches per 2^30 tensor elements, no allocation,
 * copy or synchronisation: the call can be captured into a graph.  Element offsets are 32-bit in the kernel; a batch beyond
 * 2^30 elements is split by frames on the host, a single frame beyond that is refused ("too large").  Every refusal is
 * PD_EINVAL with a message, decided before the device is touched: null xolp / stats / workspace, ws_bytes too small,
 * W > ld, ld % 4 != 0, a pointer that is not 16-byte aligned, non-finite thresholds, bad shape. */
#define PD_XOLP_STATS_BYTES 4184
size_t pd_xolp_stats_workspace(int B, int H, int W);
int pd_xolp_stats(const void* xolp, const void* mask, void* stats, void* workspace, size_t ws_bytes,
                  int B, int H, int W, int ld, const float thresholds[2], int accumulate, void* stream);

/* ------------------------------------------------------------------------- K2
 * Implicit-GEMM convolution on the fp32 matrix cores (v_mfma_f32_32x32x2_f32).
 *
 * Replaces torch.nn.Conv2d (+ ReflectionPad2d) and its autograd on the hot path:
 *   manydepth/networks/pre_encoders.py:15-25       ConvBlock.conv (bias, zero padding, stride 1/2)
 *   manydepth/networks/resnet_encoder.py:813-818   torchvision resnet18 conv1 / layer1 / layer2
 *   manydepth/layers.py:364-380                    Conv3x3 = ReflectionPad2d(1) + Conv2d(3)  (decoder)
 *
 * Layouts: x is fp32 with explicit element strides (sN,sH,sW,sC) -- NHWC (sC == 1) takes the
 * 16-byte gather path, anything else (e.g. the NCHW 2/3/9-channel stem inputs) the scalar one;
 * w is [Cout][KH][KW][Cin] (torch channels_last storage of the [Cout,Cin,KH,KW] parameter);
 * y is NHWC with row stride ldy >= Cout (ldy > Cout writes into a channel slice of a wider buffer).
 * (Ho, Wo) may be smaller than the full output grid: only the leading Ho x Wo outputs are computed.
 *
 * mode  0 zero padding | 1 reflection padding | 2 transposed (data gradient: x is dY on the
 *       forward output grid [N,H,W,C=Cout_fwd], (Ho,Wo) is the forward INPUT grid, w is the
 *       transposed weight [Cin_fwd][KH][KW][Cout_fwd] from pd_weight_transpose)
 * act   0 none | 1 ReLU | 2 ELU(alpha=1) | 3 sigmoid      (applied after bias)
 * out_scale  NULL or fp32 [Cout]: y = act(conv * out_scale + bias) -- an inference-mode BatchNorm folded into the
 *       epilogue (scale = gamma / sqrt(var + eps), bias = beta - mean * scale + conv_bias * scale)
 * affine != 0: every in-bounds input tap is replaced by (x - sub) / div before the product
 *       (ShallowEncoder.normalizeInput pre_encoders.py:76-83, resnet_encoder.py:812), scalar path only.
 * stats  NULL or fp32 [pd_conv2d_stats_rows(M,Cout)][Cout][2]: per-workgroup column sums and sums
 *       of squares of (conv + bias) -- training-mode BatchNorm statistics (reduced by pd_bn_finalize).
 * flags  kernel family / arithmetic of the products, the same word for pd_conv2d, pd_conv2d_add, pd_conv2d_rect,
 *       pd_conv2d_wgrad and their query functions (a query answers for the flags it is given):
 *         PD_CONV_AUTO       the library's choice (bf16-split products where they are faster, fp32 MFMA elsewhere);
 *         PD_CONV_FP32_MFMA  every product on v_mfma_f32_32x32x2_f32 / 16x16x4 (the reference's own arithmetic:
 *                            plain fp32 nn.Conv2d, pre_encoders.py:8-34);
 *         PD_CONV_BF16X3     bf16-split products whenever the shape fits those kernels, whatever the tile count (tests);
 *         PD_CONV_WGRAD_SPLIT_IN_REGS  weight gradient: conv_wgrad_uni_kernel's in-register split instead of
 *                            conv_wgrad_x3c_kernel (kept for its test; slower than either);
 *         PD_CONV_GENERAL_KERNELS      the general gather kernels instead of the uniform-tap / scalar-pixel ones (tests);
 *         PD_CONV_BF16       opt-in bf16 arithmetic (training mode): on the layers the single-bf16 kernels take
 *                            (pd_conv2d_uses_bf16 / pd_conv2d_wgrad_uses_bf16 non-zero) both operands are rounded ONCE to
 *                            bf16, round-to-nearest-even (v_cvt_pk_bf16_f32: a NaN stays a NaN; FLT_MAX and everything
 *                            from 0x1.ff8p127 up round to +-infinity), and each product is ONE v_mfma_f32_32x32x16_bf16
 *                            with fp32 accumulation.  Storage stays fp32 (inputs, outputs, weights, gradients), and the
 *                            epilogue (bias, activation, addend, BatchNorm partial sums) stays fp32.  bf16 denormal
 *                            operands (fp32 inputs below 2^-126 in magnitude round to them) are KEPT, not flushed: the
 *                            conversion and the MFMA preserve them on gfx950 (measured: 2^-130 x 2^20 gives 2^-110;
 *                            tests/test_conv_bf16_gpu.py pins it).  Every other layer -- 1x1,
 *                            strided, the 16-channel tail, out_scale, shapes outside the kernels' tile grids -- keeps the
 *                            arithmetic it has without the flag: a per-layer fallback, not an error.
 *       PD_CONV_FP32_MFMA and PD_CONV_BF16X3 exclude each other, PD_CONV_BF16 excludes both; unknown bits are an error.
 */
#define PD_CONV_AUTO 0u
#define PD_CONV_FP32_MFMA 1u
#define PD_CONV_BF16X3 2u
#define PD_CONV_WGRAD_SPLIT_IN_REGS 4u
#define PD_CONV_GENERAL_KERNELS 8u
#define PD_CONV_X3_IM2COL 16u   /* bf16-split forward / data gradient through the per-tap gather kernel (conv_igemm_x3_kernel)
                                 * also where the halo-tile kernel (conv_halo_x3_kernel) fits: A/B measurement and tests */
#define PD_CONV_WGRAD_ROW_WORKGROUPS 32u /* bf16-split 3x3 weight gradient with one filter row per workgroup (conv_wgrad_halo_x3_kernel)
                                         * also where the rolling-row kernel (conv_wgrad_roll_x3_kernel) fits: A/B measurement and tests */
#define PD_CONV_BF16 128u      /* single-bf16 products (above); bit 64 is unassigned */
#define PD_CONV_FLAGS_ALL 191u
int pd_conv2d_tile_m(long M, int Cout);
long pd_conv2d_stats_rows(long M, int Cout);
/* Non-zero (3: the halo-tile kernel conv_halo_x3_kernel -- stride 1, the output grid Ho x Wo (0 x 0: unknown, never 3) a whole
 * number of 8 x 32, 16 x 16 or 32 x 8 tiles, at least 512 workgroups; 3x3 / 5x5 with zero padding, the stride-1 data gradient or
 * reflection padding, C % 16 == 0, Cout % 32 == 0 (64-column workgroups, or 32-column ones where those would be fewer than 512
 * or Cout % 64 == 32), or the 4x4 zero-padded space-to-depth stems (contiguous pixels, 4 C % 16 == 0, Cout % 64 == 0) in their
 * row-window form --; 2 | 1: the per-tap gather kernel with 256- | 128-row tiles) when pd_conv2d / pd_conv2d_add send this shape (16-byte aligned NHWC operands assumed) to the kernel that forms the fp32
 * products on the bf16 matrix cores (conv_igemm_x3_kernel: x = hi + mid + lo in bf16, six MFMAs per 32x32x16 block, fp32
 * accumulation; PD_CONV_FP32_MFMA in `flags` keeps every layer on the fp32 MFMA): zero padding, the stride-1 data gradient or 3x3 reflection padding (a same-size layer is assumed), C % 4 == 0 and >= 8 (16-channel groups, the last may be partly empty),
 * Cout % 64 == 0, at least 512 tiles of 256 x 64 (M % 256 == 0) or 320 of 128 x 64 (M % 128 == 0), no out_scale, activation none or ELU.
 * Who decides: route_conv (csrc/conv.hip) routes every launch, and this query, pd_conv2d_uses_bf16 and pd_conv2d_route read the
 * same function's answer for a dense NHWC tensor of that shape (x and y 16-byte aligned, ldy = Cout, no addend, no BatchNorm
 * statistics, the input grid taken to be the output grid; Ho = Wo = 0: a plane no halo tile divides) -- so for C % 4 != 0,
 * which the 16-byte path cannot read, they answer 0 / the general kernel like the launch, where earlier versions could name
 * a bf16-split kernel such a tensor never reached.  bench.py's roofline object uses it. */
int pd_conv2d_uses_x3(long M, int Cout, int C, int KH, int KW, int stride, int pad, int mode, int act, int has_out_scale,
                      int Ho, int Wo, unsigned flags);
/* 3 when pd_conv2d / pd_conv2d_add / pd_conv2d_rect run this shape on the single-bf16 form of the halo-tile kernel
 * (conv_halo_bf16_kernel: one v_mfma_f32_32x32x16_bf16 per 32x32x16 block, operands rounded once) -- i.e. PD_CONV_BF16 is
 * in `flags` and pd_conv2d_uses_x3 answers 3 for the same arguments without it; 0 otherwise (the layer keeps the arithmetic
 * of pd_conv2d_uses_x3's answer).  Pure host logic, the same arguments as pd_conv2d_uses_x3. */
int pd_conv2d_uses_bf16(long M, int Cout, int C, int KH, int KW, int stride, int pad, int mode, int act, int has_out_scale,
                        int Ho, int Wo, unsigned flags);
/* The kernel pd_conv2d / pd_conv2d_add launch for this shape (the arguments and the tensor of pd_conv2d_uses_x3), as
 * family | BN << 4 | BM << 12: family 0 conv_igemm_kernel (general gather) | 1 conv_igemm_uni_kernel (uniform-tap) |
 * 2 conv_igemm_x3_kernel (bf16-split, per-tap gather) | 3 conv_halo_x3_kernel (bf16-split, halo tile) | 4 conv_halo_bf16_kernel
 * (its single-bf16 form, PD_CONV_BF16); BM x BN the workgroup's tile of the output matrix, rows x columns (halo tile: 256
 * pixels x 64 | 32 channels).  A flags word pd_conv2d refuses is read without PD_CONV_BF16.  Pure host logic; the profiler label
 * of a launch (ops._igemm_label) is made of this answer alone. */
int pd_conv2d_route(long M, int Cout, int C, int KH, int KW, int stride, int pad, int mode, int act, int has_out_scale,
                    int Ho, int Wo, unsigned flags);
int pd_conv2d(const void* x, const void* w, const void* bias, const void* out_scale, void* y, void* stats,
              int N, int H, int W, int C, long sN, long sH, long sW, long sC,
              int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, int mode, int act,
              int affine, float sub, float div, long ldy, unsigned flags, void* stream);

/* The 16-channel decoder tail (depth_decoder.py upconv(0,0) 32->16, upconv(0,1) 16->16; layers.py:329-380): 3x3
 * convolutions with 16 output channels from an input halo tile staged once in LDS (the implicit GEMM above re-stages
 * the input per tap and is bound by that path at 16 output channels).
 *   mode 0: y = act(conv3x3(reflection_pad1(x), w) + bias), x NHWC [N,H,W,C] (C = 16 or 32, strides sN/sH/sW, channel
 *           stride 1), w [16][3][3][C], y NHWC [N,H,W,16] with row stride ldy, act 0 none | 2 ELU;
 *   mode 1: data gradient on the reflection-PADDED grid: x = dz [N,H,W,16], w = the transposed filter
 *           [Cout][3][3][16] (pd_weight_transpose), y [N,H+2,W+2,Cout] (Cout = 16 or 32), zero outside the image;
 *           pd_reflect_fold folds the border afterwards;
 *   mode 2: the zero-padding (pad 1) data gradient on the H x W grid (same operands as mode 1, y [N,H,W,Cout]) = the
 *           interior of mode 1's result; pd_reflect_dgrad_border adds the folded border strips. */
int pd_conv16(const void* x, const void* w, const void* bias, void* y, int N, int H, int W, int C,
              long sN, long sH, long sW, int Ho, int Wo, int Cout, long ldy, int mode, int act, void* stream);

/* Weight (+ bias) gradient of the mode-0 convolution above: dw [16][3][3][C] (+)= sum_p dz[p] (x) x[reflect(p+tap-1)],
 * dbias [16] (+)= sum_p dz[p] (or NULL).  Persistent workgroups, one deterministic partial per workgroup in
 * `workspace` (>= pd_conv16_wgrad_workspace(C) bytes), summed in a fixed order. */
size_t pd_conv16_wgrad_workspace(int C);
int pd_conv16_wgrad(const void* x, const void* dz, void* dw, void* dbias, void* workspace, size_t ws_bytes,
                    int N, int H, int W, int C, long sN, long sH, long sW, long ldd, int accumulate, void* stream);

/* Stride-2 data gradient by output parity (3x3 / stride 2 / pad 1, even input grid; resnet18 layer2.0.conv1,
 * resnet_encoder.py / torchvision BasicBlock): pd_dgrad_s2_filters turns the transposed filter wt [Cin][3][3][Cout] into
 * the four exact class filters, back to back in wsub (9*Cin*Cout floats): class c = 2*(ih%2) + iw%2 is
 * [Cin][1 + ih%2][1 + iw%2][Cout] at float offset Cin*Cout*{0,1,3,5}[c]; each class is pd_conv2d_rect(mode 2,
 * KH = 1 + ih%2, KW = 1 + iw%2, pad_h = ih%2, pad_w = iw%2) of dY onto the [N,Ho,Wo,Cin] sub-grid; pd_interleave4
 * scatters the four sub-grids [4][N][Ho][Wo][C] into dX [N][2Ho][2Wo][C].  9 tap-units instead of the 36 of the masked
 * transposed gather.
 * pd_conv2d_rect: stride-1 convolution (mode 0) / data gradient (mode 2) with a KH x KW filter and separate row /
 * column padding, no bias / activation; needs C % 32 == 0 and 16-byte aligned NHWC operands (uniform-tap kernel). */
int pd_dgrad_s2_filters(const void* wt, void* wsub, int Cin, int Cout, void* stream);
int pd_conv2d_rect(const void* x, const void* w, void* y, int N, int H, int W, int C, long sN, long sH, long sW, long sC,
                   int Ho, int Wo, int Cout, int KH, int KW, int pad_h, int pad_w, int mode, long ldy, unsigned flags,
                   void* stream);
int pd_interleave4(const void* sub, void* dx, int N, int Ho, int Wo, int C, void* stream);

/* y = conv(x, w) + addend: the same convolution (no bias / scale / activation / statistics) with an NHWC tensor of the
 * output's shape (row stride ld_add, may alias y) added in the epilogue.  Used for the data gradient of the first
 * convolution of a residual block, which autograd would otherwise sum with the gradient of the skip connection in a
 * separate pass (the reference: torch's `out += identity` backward, pre_encoders.py:46, torchvision BasicBlock). */
int pd_conv2d_add(const void* x, const void* w, const void* addend, long ld_add, void* y,
                  int N, int H, int W, int C, long sN, long sH, long sW, long sC,
                  int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, int mode, long ldy, unsigned flags,
                  void* stream);

/* Weight gradient dW[Cout][KH][KW][Cin] (+ optional dbias[Cout]) of the convolution above
 * (modes 0 and 1).  dy is NHWC on the output grid with row stride ldd.  Partial tiles go to
 * `workspace` (pd_conv2d_wgrad_workspace bytes) and are summed deterministically; accumulate != 0
 * adds to dw/dbias instead of overwriting.  Replaces autograd's conv weight/bias gradient.
 * The slice count of every kernel depends on the shape and `flags` only, never on ws_bytes:
 * pd_conv2d_wgrad_workspace(M, Cout, K, flags) bytes hold it, and a larger workspace gives the same bits. */
size_t pd_conv2d_wgrad_workspace(long M, int Cout, int K, unsigned flags);
int pd_conv2d_wgrad(const void* x, const void* dy, void* dw, void* dbias, void* workspace, size_t ws_bytes,
                    int N, int H, int W, int C, long sN, long sH, long sW, long sC,
                    int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, int mode,
                    int affine, float sub, float div, long ldd, int accumulate, unsigned flags, void* stream);
/* 3 (conv_wgrad_roll_x3_kernel: 3x3, stride 1, same-size output, C % 64 == 0, Cout % 64 == 0, Wo % 16 == 0, tile columns long and
 * many enough for >= 12 tile rows per slice on >= 384 workgroups: all three filter rows per workgroup, input rows rolling
 * through LDS; PD_CONV_WGRAD_ROW_WORKGROUPS in `flags` declines it),
 * 2 (conv_wgrad_halo_x3_kernel: 3x3 / 5x5, stride 1, zero or reflection padding, C % 64 == 0 and Cout % 64 == 0 -- or 3x3 with
 * Cout % 32 == 0, C % 32 == 0 on 1 x 32 tiles --, the output grid a whole number of 1 x 32, 2 x 16, 4 x 8 or (3x3) 8 x 4 pixel tiles: both
 * operands split once per tile and read through ds_read_b64_tr_b16) or
 * 1 when pd_conv2d_wgrad sends this shape (zero or reflection padding; 16-byte aligned NHWC operands assumed) to the kernel that forms the
 * fp32 products on the bf16 matrix cores, every element split once (conv_wgrad_x3c_kernel; PD_CONV_FP32_MFMA: fp32 MFMA) --
 * the profiler label of a launch and bench.py's roofline object use it.  Reflection padding other than ReflectionPad2d(1) in
 * front of a same-size 3x3 runs the general kernel (0).  Who decides: route_wgrad (csrc/conv.hip) routes every launch, and this
 * query, pd_conv2d_wgrad_uses_bf16 and pd_conv2d_wgrad_route read the same function's answer for dense, 16-byte aligned NHWC x and
 * dy (ldd = Cout); an empty output grid: 0. */
int pd_conv2d_wgrad_uses_x3(long M, int Cout, int C, int KH, int KW, int stride, int pad, int mode, int H, int W, int Ho, int Wo,
                            unsigned flags);
/* 3 (conv_wgrad_roll_bf16_kernel) or 2 (conv_wgrad_halo_bf16_kernel): pd_conv2d_wgrad runs this shape on the single-bf16 form
 * of the kernel pd_conv2d_wgrad_uses_x3 names with the same code (PD_CONV_BF16 in `flags`); 0: the layer keeps the arithmetic it
 * has without the flag.  Pure host logic. */
int pd_conv2d_wgrad_uses_bf16(long M, int Cout, int C, int KH, int KW, int stride, int pad, int mode, int H, int W, int Ho, int Wo,
                              unsigned flags);
/* The launch pd_conv2d_wgrad plans for this shape (the arguments and the tensors of pd_conv2d_wgrad_uses_x3), as
 * code | one << 2 | rows << 4: code = pd_conv2d_wgrad_uses_x3's answer, one = 1 for the single-bf16 form (pd_conv2d_wgrad_uses_bf16
 * non-zero), rows >= 1 the partial rows ([Cout][K] weights + [Cout] bias each) the kernel writes and the ordered reduction sums --
 * never more than pd_conv2d_wgrad_workspace(M, Cout, K, flags) pays for.  A flags word pd_conv2d_wgrad refuses is read without
 * PD_CONV_BF16.  Pure host logic; the profiler label of a launch (ops.conv2d_wgrad) is made of this answer alone. */
int pd_conv2d_wgrad_route(long M, int Cout, int C, int KH, int KW, int stride, int pad, int mode, int H, int W, int Ho, int Wo,
                          unsigned flags);

/* 7x7 / stride-2 / pad-3 stems (pre_encoders.py:54 ShallowEncoder.Conv1, torchvision resnet conv1) executed as a
 * 4x4 / stride-1 / pad-2 convolution over the space-to-depth input [N][H/2][W/2][4C] (4C is a multiple of 4 ->
 * 16-byte gather path): input transform (with the optional (x-sub)/div normalisation), weight regrouping
 * [Cout][7][7][C] -> [Cout][4][4][4C] and the inverse mapping of the weight gradient.  pd_conv2d /
 * pd_conv2d_wgrad are then called with KH=KW=4, stride 1, pad 2 and the (H/2, W/2) output grid. */
int pd_stem_s2d_input(const void* x, void* out, int N, int C, int H, int W, long sN, long sC, long sH, long sW,
                      int affine, float sub, float div, void* stream);
int pd_stem_s2d_weight(const void* w, void* w2, int Cout, int C, void* stream);
int pd_stem_s2d_weight_grad(const void* dw2, void* dw, int Cout, int C, int accumulate, void* stream);

/* w [Cout][T][Cin] -> wt [Cin][T][Cout], T = KH*KW: operand of the mode-2 (data gradient) GEMM. */
int pd_weight_transpose(const void* w, void* wt, int Cout, int T, int Cin, void* stream);
/* Every convolution weight of a flat parameter buffer in one launch (the data-gradient operands of a whole step):
 * entry e of `table` (device int32[n][4]) = {element offset in src and dst, Cout, T, Cin}; blk (device int32[n+1]) =
 * first workgroup of entry e at T * ceil(Cout/32) * ceil(Cin/32) workgroups per entry, blk[n] = nblocks.  Replaces one pd_weight_transpose per
 * layer and step (the reference keeps no such copy: cuDNN's backward-data reads the forward filter, trainer.py:430). */
int pd_weight_transpose_batched(const void* src, void* dst, const void* table, const void* blk, int n, int nblocks,
                                void* stream);

/* ------------------------------------------------------------------------- K3
 * Memory-bound kernels fused around the convolutions (NHWC fp32, 16 bytes per lane).
 *
 * pd_bn_fwd_finalize: BatchNorm2d statistics.  training != 0: reduces the conv epilogue partials
 *   [R][C][2] in fp64 (acc_ws: 2*C + 1 doubles -- the sums and an arrival ticket -- that must be ZERO on entry
 *   and are left zero by the call: a long-lived accumulator per stream saves a memset per layer; the workgroup
 *   that arrives last finalises, so the whole call is ONE launch; same contract in pd_bn_bwd_finalize),
 *   updates running_mean/var with torch semantics
 *   (momentum, unbiased variance) and emits scale = gamma*invstd, shift = beta - mean*scale plus
 *   the saved mean / invstd; training == 0: coefficients from the running statistics.
 *   Replaces nn.BatchNorm2d's statistics pass (pre_encoders.py:19,29; torchvision BasicBlock.bn*).
 * pd_chain_fwd: out = relu_post( dropout( pool2x2( relu_pre( x*scale + shift ) ) ) + res )
 *   i.e. the tail of pre_encoders.ConvBlock (:28-34) + the ResidualBlock add (:46), or the
 *   torchvision BasicBlock tail (bn -> +identity -> relu).  scale == NULL means identity.
 *   Dropout masks come from Philox4x32-10(seed, offset, element) and are regenerated in backward.
 * pd_chain_bwd_reduce / pd_bn_bwd_finalize / pd_chain_bwd_apply: the two-pass backward
 *   (per-channel sum g, sum g*xhat -> dgamma, dbeta -> dx of the raw conv output; optional dres
 *   = dy * (out > 0) for post-add ReLU blocks).
 */
int pd_bn_fwd_finalize(const void* partial, long R, int C, double count, const void* gamma, const void* beta,
                       void* running_mean, void* running_var, float momentum, float eps, void* acc_ws, long acc_len,
                       void* scale, void* shift, void* save_mean, void* save_invstd, int training, void* stream);
/* acc_len: doubles in acc_ws, checked against 2*C + 1 (the ticket word lives at acc_ws[2*C]). */
int pd_bn_bwd_finalize(const void* partial, long R, int C, double count, void* acc_ws, long acc_len, void* dgamma,
                       void* dbeta, void* coef, int accumulate, void* stream);
long pd_chain_bwd_rows(int N, int H, int W, int C);
int pd_chain_fwd(const void* x, const void* scale, const void* shift, const void* res, void* out,
                 int N, int H, int W, int C, long ld_res, long ld_out, int relu_pre, int pool,
                 float drop_p, uint64_t seed, uint64_t offset, const void* step_state, int relu_post, void* stream);
int pd_chain_bwd_reduce(const void* dy, long ld_dy, const void* x, const void* out, long ld_out,
                        const void* scale, const void* shift, const void* mean, const void* invstd,
                        void* partial, int N, int H, int W, int C, int relu_pre, int pool, float drop_p,
                        uint64_t seed, uint64_t offset, const void* step_state, int relu_post, void* stream);
int pd_chain_bwd_apply(const void* dy, long ld_dy, const void* x, const void* out, long ld_out,
                       const void* scale, const void* shift, const void* mean, const void* invstd,
                       const void* coef, void* dx, void* dres, int N, int H, int W, int C, int relu_pre,
                       int pool, float drop_p, uint64_t seed, uint64_t offset, const void* step_state, int relu_post,
                       void* stream);

/* nn.MaxPool2d(3, 2, 1) of the ResNet stem (resnet_encoder.py:814) and its gradient. */
/* idx (optional in fwd): uint8 [N,Ho,Wo,C] window position (dh*3+dw) of the first maximum, consumed by bwd. */
int pd_maxpool3s2_fwd(const void* x, void* y, void* idx, int N, int H, int W, int C, void* stream);
int pd_maxpool3s2_bwd(const void* idx, const void* dy, void* dx, int N, int H, int W, int C, void* stream);
/* ... + addend (optional, NHWC [N,H,W,C] with row stride ld_add): the gradient a second consumer of the pooled tensor
 * delivers (the decoder's skip connection, depth_decoder.py:65-66), summed in the same pass. */
int pd_maxpool3s2_bwd_add(const void* idx, const void* dy, const void* addend, long ld_add, void* dx, int N, int H, int W,
                          int C, void* stream);

/* Decoder glue: out[N,2H,2W,Ca+Cs] = cat(bilinear_x2(a), skip)  (layers.py:446-449 upsample,
 * depth_decoder.py:64-67 cat) and the gradient of the upsampled part (gather form). */
int pd_upcat_fwd(const void* a, const void* skip, long ld_skip, void* out, int N, int H, int W, int Ca, int Cs,
                 void* stream);
int pd_up_bwd(const void* dout, long ld_d, void* da, int N, int H, int W, int Ca, void* stream);
/* same with the ELU derivative folded in: a = elu_y [N,H,W,Ca] is the output of a ConvBlock (layers.py:329-342), da
 * leaves multiplied by (a > 0 ? 1 : a + 1), i.e. as the gradient of the convolution output. elu_y NULL = pd_up_bwd. */
int pd_up_bwd_elu(const void* dout, long ld_d, const void* elu_y, void* da, int N, int H, int W, int Ca, void* stream);

/* DPT decoder glue (reference manydepth/dpt/blocks.py; --train_dpt, trainer.py:147-171):
 * pd_up2x_ac_fwd / _bwd: nn.functional.interpolate(scale_factor=2, mode="bilinear", align_corners=True) of an NHWC
 *   tensor [N,H,W,C] -> [N,2H,2W,C] (blocks.py:138-172 Interpolate, :375-377 in FeatureFusionBlock_custom) and its
 *   gradient in gather form (deterministic);
 * pd_relu_add: out = (relu ? max(x, 0) : x) + (res ? res : 0) over n floats -- the activation in front of the first
 *   convolution and the skip sum of ResidualConvUnit_custom (blocks.py:289-307). */
int pd_up2x_ac_fwd(const void* a, void* out, int N, int H, int W, int C, void* stream);
int pd_up2x_ac_bwd(const void* dout, void* da, int N, int H, int W, int C, void* stream);
int pd_relu_add(const void* x, const void* res, void* out, long n, int relu, void* stream);

/* dz = dy * f'(.) through the activation OUTPUT y: act 1 ReLU, 2 ELU (layers.py:337), 3 sigmoid. */
int pd_act_bwd(const void* dy, const void* y, void* dz, long n, int act, void* stream);
/* Gradient of ReflectionPad2d(1): dxp [N,H+2,W+2,C] -> dx [N,H,W,C]  (layers.py:372). */
int pd_reflect_fold(const void* dxp, void* dx, int N, int H, int W, int C, void* stream);
/* ... of ReflectionPad2d(pad), 1 <= pad < min(H, W): dxp [N,H+2pad,W+2pad,C] -> dx [N,H,W,C]  (layers.py:352, Conv5x5). */
int pd_reflect_fold_pad(const void* dxp, void* dx, int N, int H, int W, int C, int pad, void* stream);
/* The same gradient without the padded intermediate: dx (in/out, NHWC [N,H,W,Cin]) already holds the zero-padding
 * (pad 1) data gradient -- the interior of the padded-grid gradient -- and receives the four folded border strips
 * (1x3 / 3x1 filter slices applied to the first / last row and column of dz [N,H,W,Cout], row stride ldd;
 * w [Cout][3][3][Cin], the forward filter).  Touches 2(H+W) pixels per image instead of two full-tensor passes. */
int pd_reflect_dgrad_border(const void* dz, long ldd, const void* w, void* dx, int N, int H, int W, int Cout, int Cin,
                            void* stream);
/* torch.optim.Adam step (trainer.py:238,442) over one flat fp32 buffer; grads are pre-multiplied
 * by grad_scale (1/world_size after the RCCL sum).  zero_grad != 0 also clears g in the same pass
 * (trainer.py:436 zero_grad of the NEXT iteration, without a separate 85 MB memset).
 * step_state (optional): the step words below; Adam's t is then read from step_state[1] and lr / grad_scale from
 * step_state[2] on the device instead of the `step`, `lr`, `grad_scale` arguments, so that a hipGraph of the training step
 * can be replayed with frozen arguments and still follow a learning-rate schedule (trainer.py:238-240,467 StepLR).  Bias
 * corrections use beta^t by repeated squaring in double on either side (identical bits). */
int pd_adam_step(void* p, void* g, void* m, void* v, long n, float lr, float beta1, float beta2, float eps,
                 float weight_decay, long step, const void* step_state, float grad_scale, int zero_grad, void* stream);
/* Step words in device memory, int64[4]: [0] training steps begun -- the dropout sites of pd_chain_* add
 * step_state[0] << 12 to their Philox offset (step_state NULL: the offset argument alone) --, [1] optimizer steps,
 * [2] the fp32 bit patterns of lr (low word) and grad_scale (high word).  pd_step_tick increments the selected counters
 * (one thread); pd_step_set_hyper writes word [2] (call it whenever the scheduler changed lr: it is NOT part of a captured
 * step).  The only per-step state of a captured training step. */
int pd_step_tick(void* step_state, int bump_dropout, int bump_adam, void* stream);
int pd_step_set_hyper(void* step_state, float lr, float grad_scale, void* stream);

/* ------------------------------------------------------------------------- K5
 * Multi-scale supervised loss (trainer.py:1126-1150,1241-1265,1298-1309; layers.py:62-71,452-465).
 * Per scale: pd_disp_to_depth (bilinear to H x W + disp_to_depth), pd_sup_loss_fwd (masked L1 and
 * the kornia depth_to_normals cosine term as wavefront-reduced partial sums), pd_smooth_fwd;
 * pd_loss_finalize turns the partials into vals = [loss, (loss/s, supervised_depth_loss/s,
 * normals_loss/s) per scale] on the device.  Backward: pd_loss_weights, pd_sup_loss_bwd,
 * pd_up_gather_bwd, pd_smooth_bwd.  No host synchronisation anywhere.
 */
int pd_loss_rows(long n);
int pd_disp_to_depth(const void* disp, void* depth, void* updisp, int N, int hs, int ws, int H, int W,
                     float min_depth, float max_depth, void* stream);
/* generic != 0: the any-ratio kernel instead of the one specialised for zooms 1 / 2 / 4 / 8 (tests compare the two); it
 * alone also takes a full size that is no integer multiple of the scale size (H >= hs, W >= ws), as pd_unc_loss_bwd's
 * callers need */
int pd_up_gather_bwd(const void* gup, void* gdisp, int N, int hs, int ws, int H, int W, int accumulate, int generic,
                     void* stream);
/* gt_normals (optional, NULL = recompute per call): [N,H,W,4] floats written by pd_gt_normals -- the unit normal of the
 * ground-truth depth at every in-range pixel (trainer.py:1298-1309 evaluates it once per scale; it does not depend on
 * the scale, so a step computes it once and its eight consumers read it back). */
int pd_gt_normals(const void* gt, const void* K, void* gt_normals, int N, int H, int W, float min_depth, float max_depth,
                  void* stream);
int pd_sup_loss_fwd(const void* pred, const void* gt, const void* K, const void* gt_normals, void* partial, int N, int H,
                    int W, float min_depth, float max_depth, int with_normals, void* stream);
/* Trainer.compute_supervised_normals_losses as a function of its own (trainer.py:1298-1309) with the CALLER's mask:
 * out[0] = sum((2 - cos(n_gt, n_pred)) * mask) / sum(mask), normals = kornia depth_to_normals of the two depth maps at
 * every pixel (no depth-range gate), mask fp32 [N,H,W] (any values: it multiplies).  partial_ws: pd_loss_rows(N*H*W) * 2
 * floats; the ratio is formed on the device from an ordered fp64 sum of the partials. */
int pd_normals_loss_masked(const void* pred, const void* gt, const void* K, const void* mask, void* partial_ws, void* out,
                           int N, int H, int W, void* stream);
/* Loss of PREDICTED normals -- the `arch1++_separate_normals_dec` variant (reference README.md:54: "the decoder directly
 * predicts normals; these normals are compared with normals calculated from ground truth"; its source is not in the reference
 * checkout, the formula is trainer.py:1298-1309 with the network's 3-channel output in place of depth_to_normals(pred)):
 * out[0] = sum((2 - cos(pred, n_gt)) m) / sum(m), out[1] = sum(m); pred pixel-major (NHWC) fp32 with pixel stride ld >= 3,
 * gt_normals from pd_gt_normals, m = gt depth inside [min_depth, max_depth].  partial_ws: pd_loss_rows(N*H*W) * 2 floats.
 * _bwd: dpred = gout[0] / out[1] * m * -(d cos / d pred), written for every pixel (zeros outside the mask). */
int pd_normals_pred_loss_fwd(const void* pred, long ld, const void* gt_normals, const void* gt, void* partial_ws, void* out,
                             int N, int H, int W, float min_depth, float max_depth, void* stream);
int pd_normals_pred_loss_bwd(const void* pred, long ld, const void* gt_normals, const void* gt, const void* gout,
                             const void* loss_count, void* dpred, long ld_dpred, int N, int H, int W, float min_depth,
                             float max_depth, void* stream);
/* The loop over scales of trainer.py:1134-1265 in one call: the per-scale kernels above dispatched by blockIdx.y = scale
 * with each scale's own grid (identical partial sums, hence identical bits), the supervised forward pass reading the
 * ground truth once for all scales: 4 launches forward, 4 + a memset backward, whatever S <= 8.
 * Arrays of S device pointers (host arrays): disps [N,1,hs,ws], colors [N,3,hs,ws], depths [N,1,H,W] (out), means [N] (out),
 * edge_ws [N,hs,ws,2] (out, entries may be NULL); sup_part [S][part_stride][3], sm_part [S][part_stride][2] floats with
 * part_stride >= pd_loss_rows(N*H*W); then pd_loss_finalize as before.
 * Backward: wts [S][3] (pd_loss_weights), sums [S][5]; workspaces gup_ws S*N*H*W floats, g_ws sum_s N*hs*ws floats,
 * gd_acc S*N doubles; gdisps [N,1,hs,ws] (out) = d loss / d disp_s. */
int pd_multiscale_loss_fwd(const void* const* disps, const void* const* colors, const int* hs, const int* ws, int S,
                           const void* gt, const void* K, const void* gt_normals, void* const* depths, void* const* means,
                           void* const* edge_ws, void* sup_part, void* sm_part, int part_stride, int N, int H, int W,
                           float min_depth, float max_depth, int with_normals, void* stream);
int pd_multiscale_loss_bwd(const void* const* disps, const void* const* colors, const void* const* depths,
                           const void* const* means, const void* const* edge_ws, const int* hs, const int* ws, int S,
                           const void* gt, const void* K, const void* gt_normals, const void* wts, const void* sums,
                           void* gup_ws, void* g_ws, void* gd_acc, void* const* gdisps, int N, int H, int W,
                           float min_depth, float max_depth, void* stream);
/* pd_sup_loss_bwd: ab_ws ([N,H,W,6] floats) is only read by the two-pass form (two_pass_form != 0, kept for its test);
 * by default one kernel evaluates the per-pixel normal gradients for the halo of an 8 x 64 tile into LDS and gathers
 * from there, so ab_ws may be NULL. */
int pd_sup_loss_bwd(const void* pred, const void* gt, const void* K, const void* gt_normals, const void* wts,
                    const void* sums, void* ab_ws, void* gout, int N, int H, int W, float min_depth, float max_depth,
                    int with_normals, int to_disp, int two_pass_form, void* stream);
/* Edge-aware smoothness (layers.py:452-465 get_smooth_loss) of the mean-normalised disparity of trainer.py:1256-1258:
 * partial[block][2] = (sum |dx (disp / (mean + 1e-7))| e^{-|dx I|}, same for y); the caller divides by the element
 * counts N h (w-1) and N (h-1) w.  mean [N] receives the per-image means; mean == NULL evaluates the term on disp as it
 * is -- layers.get_smooth_loss as a function of its own (the facade's manydepth.layers.get_smooth_loss).
 * edge_w (optional, NULL = recompute in the backward pass): [N,h,w,2] floats, the image-only edge weights
 * e^{-|dx I|}, e^{-|dy I|} written by the forward pass and read by the backward pass.
 * pd_smooth_bwd: wts[2] = d loss / d (smooth_x + smooth_y) (the two terms are averaged separately, as in the reference);
 * g_ws [N,h,w] floats, gd_acc N doubles. */
int pd_smooth_fwd(const void* disp, const void* img, void* mean, void* partial, void* edge_w, int N, int h, int w,
                  void* stream);
int pd_smooth_bwd(const void* disp, const void* img, const void* mean, const void* wts, const void* edge_w, void* g_ws,
                  void* gd_acc, void* gdisp, int N, int h, int w, int accumulate, void* stream);
int pd_loss_finalize(const void* sup_part, const int* sup_rows, const void* sm_part, const int* sm_rows,
                     const int* dims, const int* scale_ids, int S, int part_stride, float w_normals,
                     float w_smooth, void* sums, void* vals, void* stream);
/* vals from given sums [S][5] fp64 (sum|.|m, sum(2-cos)m, sum m, smooth_x, smooth_y): the division step of
 * pd_loss_finalize alone, for data-parallel runs that all-reduce the three masked sums per scale first
 * (trainer.py:1247,1308 normalise by the mask count of the whole batch). */
int pd_loss_from_sums(const void* sums, const int* dims, const int* scale_ids, int S, float w_normals,
                      float w_smooth, void* vals, void* stream);
int pd_loss_weights(const void* gvals, const int* scale_ids, int S, float w_normals, float w_smooth, void* wts,
                    void* stream);

/* SSIM map (mode 0, layers.py:468-499) or the photometric reprojection loss of trainer.py:1069-1081 (mode 1:
 * out [N,1,H,W] = 0.85 * mean_c SSIM + 0.15 * mean_c |y - x|, or the L1 part alone when no_ssim).  x, y planar
 * NCHW fp32.  Inactive under --depth_supervision_only; the photometric mode (below) runs mode 1 with its gradient.
 * A NaN or infinite pixel gives NaN on the windows that hold it (torch.clamp propagates NaN; so does the clamp here). */
int pd_ssim_fwd(const void* x, const void* y, void* out, int N, int C, int H, int W, int mode, int no_ssim,
                void* stream);
/* Gradient of pd_ssim_fwd w.r.t. both images: gout [N,C,H,W] (mode 0) or [N,1,H,W] (mode 1), gx / gy [N,C,H,W] (gy may be
 * NULL), coef_ws 5*N*C*H*W floats.  Two launches: per-pixel coefficients of the five window means (with the clamp mask), then
 * the gather over the (reflected) 3x3 windows that contain each pixel. */
int pd_ssim_bwd(const void* x, const void* y, const void* gout, void* coef_ws, void* gx, void* gy, int N, int C, int H, int W,
                int mode, int no_ssim, void* stream);

/* ------------------------------------------------------------------------- photometric multi-view term (csrc/reproj.hip)
 * Training with --depth_supervision True --pose_input True (without --depth_supervision_only): the neighbouring frames
 * are warped into the current view with the predicted depth and the ground-truth relative pose, and monodepth2's
 * reprojection loss (pd_ssim_fwd mode 1), reduced over the frames by minimum with automasking, joins the supervised terms
 * (trainer.py:479-530, 983-1067, 1069-1098, 1150-1236).
 *
 * pd_view_synth_fwd -- BackprojectDepth + Project3D + F.grid_sample(bilinear, padding_mode="border", align_corners=True)
 * (layers.py:383-443, trainer.py:1021-1044) for one source frame.
 *   depth  [N,1,H,W] fp32      src [N,C,H,W] planar fp32      K, inv_K, T [N,4,4] fp32 row-major
 *   warped [N,C,H,W] fp32 out  coords [N,H,W,2] fp32 out (8-byte aligned): (u, v) of every pixel, UNCLAMPED
 * Per pixel (x, y), evaluated in fp64 from the fp32 inputs, every sum left to right as written, no fused multiply-add:
 *   P[i][j] = K[i][0] T[0][j] + K[i][1] T[1][j] + K[i][2] T[2][j] + K[i][3] T[3][j]      (i < 3; once per batch item)
 *   r[i]    = inv_K[i][0] x + inv_K[i][1] y + inv_K[i][2]                                 (i < 3)
 *   p       = depth * r
 *   h[i]    = P[i][0] p[0] + P[i][1] p[1] + P[i][2] p[2] + P[i][3]
 *   u = h[0] / (h[2] + 1e-7),  v = h[1] / (h[2] + 1e-7)
 * rounded once to fp32 and stored in coords.  Under align_corners=True Project3D's division by W-1 / H-1, its (. - 0.5) * 2
 * and grid_sample's un-normalisation cancel, so (u, v) are source pixel coordinates.  Sampling, in fp32 from the stored
 * coordinate: uc = min(max(u, 0), W-1), vc likewise with H-1 (a non-finite coordinate becomes 0); x0 = floor(uc),
 * x1 = min(x0 + 1, W-1), wx1 = uc - x0, wx0 = 1 - wx1 (y likewise);
 *   warped = ((src[y0][x0] (wx0 wy0) + src[y0][x1] (wx1 wy0)) + src[y1][x0] (wx0 wy1)) + src[y1][x1] (wx1 wy1).
 *
 * pd_view_synth_bwd -- the gradient w.r.t. depth alone (the sources are data, and so is T under --pose_input; a PREDICTED
 * pose takes pd_view_synth_bwd_pose below): each output pixel depends on its own depth only, hence no scatter and no atomics.
 *   gdepth [N,1,H,W] (=, or += when accumulate != 0) = sum_c gwarped_c (d warped_c / du * du/ddepth + d warped_c / dv * dv/ddepth)
 * d warped / d(u, v) from the four taps with the weights of `coords`; it is exactly zero on an axis whose coordinate is
 * <= 0, >= size-1 or not finite (PyTorch's border rule).  With h = depth * q + b, q = P[:, :3] r:
 *   du/ddepth = (q[0] - u q[2]) / (h[2] + 1e-7), dv/ddepth = (q[1] - v q[2]) / (h[2] + 1e-7), in fp64 as above.
 * Limits of both: 0 <= N <= 65535 (N = 0 does nothing), C, H, W > 0, H * W <= 2^30.
 *
 * pd_view_synth_bwd_pose -- pd_view_synth_bwd and the gradient w.r.t. the pose T in one pass over the same taps (gwarped and
 * src are read once).  gdepth may be NULL (skipped); where given it holds the bits pd_view_synth_bwd writes.
 *   partial_ws  N * pd_view_synth_pose_rows(H, W) * 12 doubles, 8-byte aligned (pd_view_synth_pose_rows is a pure function
 *               of H and W: min(ceil(H W / 256), 512))
 *   gP          [N,12] doubles out, or NULL: the gradient w.r.t. P = (K T)[:3,:], row-major 3x4
 *   gT          [N,4,4] fp32 out, written with "="
 * Per pixel with gu = sum_c gwarped_c d warped_c / du, gv likewise (fp32, the expressions of pd_view_synth_bwd), and u, v,
 * hz = h[2] + 1e-7, p = depth * r in fp64 as in pd_view_synth_fwd; free_x / free_y = the axis is neither clamped nor
 * non-finite.  The rest in fp64, no fused multiply-add:
 *   a0 = free_x ? gu / hz : 0        a1 = free_y ? gv / hz : 0
 *   a2 = -((free_x ? a0 u : 0) + (free_y ? a1 v : 0))
 *   gP[i][j] += a_i * (p[0], p[1], p[2], 1)[j]        a row whose axis is not free receives no term (never 0 * inf), and a
 *                                                     pixel with neither axis free contributes nothing at all
 * The 12 sums per item are accumulated in the order of pd_reproj_combine_fwd: per thread over its grid-stride pixels, per
 * wavefront by shuffles, per workgroup, one row of partial_ws per workgroup; then one workgroup per item sums that item's
 * rows and forms, in fp64 rounded once,
 *   gT[k][j] = (K[0][k] gP[0][j] + K[1][k] gP[1][j]) + K[2][k] gP[2][j]        (k, j < 4).
 * Bit-reproducible, no atomics, no host synchronisation.  Limits as pd_view_synth_bwd.
 *
 * pd_depth_to_updisp_bwd -- gup[i] = -gdepth[i] * depth[i]^2 * (1/min_depth - 1/max_depth): the gradient of
 * depth = 1 / (min_disp + (max_disp - min_disp) * up) w.r.t. the upsampled disparity `up` (layers.py:62-71), n elements;
 * pd_up_gather_bwd carries it on to the disparity map.  gup may alias gdepth. */
#define PD_REPROJ_MAX_FRAMES 8
int pd_view_synth_fwd(const void* depth, const void* src, const void* K, const void* inv_K, const void* T, void* warped,
                      void* coords, int N, int C, int H, int W, void* stream);
int pd_view_synth_bwd(const void* gwarped, const void* src, const void* coords, const void* depth, const void* K,
                      const void* inv_K, const void* T, void* gdepth, int N, int C, int H, int W, int accumulate,
                      void* stream);
int pd_view_synth_pose_rows(int H, int W);
int pd_view_synth_bwd_pose(const void* gwarped, const void* src, const void* coords, const void* depth, const void* K,
                           const void* inv_K, const void* T, void* gdepth, void* partial_ws, void* gP, void* gT, int N, int C,
                           int H, int W, int accumulate, void* stream);
int pd_depth_to_updisp_bwd(const void* gdepth, const void* depth, void* gup, long n, float min_depth, float max_depth,
                           void* stream);
/* pd_reproj_combine_fwd -- trainer.py:1163-1215 over F <= PD_REPROJ_MAX_FRAMES neighbouring frames.
 *   reproj    host array of F device pointers, each an [N,1,H,W] fp32 map of compute_reprojection_loss(warped_f, target)
 *   identity  the same for the unwarped sources (automasking), or NULL: no automasking, the mask is all ones
 *   noise     [N,1,H,W] fp32 added to the identity value (trainer.py:1193-1194), or NULL; needs identity
 *   valid     [N,F] fp32, 0 = frame f of item n does not exist, or NULL: all valid
 * Per pixel: m = the minimum of the valid frames' reproj values (the first valid frame, a later one only when strictly
 * smaller), or with avg != 0 their mean (sum in frame order / number of valid frames); the same over the identity maps,
 * plus noise; mask = m <= identity + noise (argmin index 0: a tie goes to the reprojection).  An invalid frame never wins
 * a minimum, and a pixel of an item without a valid frame has mask 0.
 *   sel   [N,H,W] uint8 out: the winning frame (0 with avg), 255 where the mask is 0 -- what the backward pass needs
 *   sums  2 doubles out (8-byte aligned): sum(m * mask), sum(mask);   loss 1 float out = sums[0] / (sums[1] + 1e-7)
 * Both sums are accumulated in fp64 in a fixed order: per thread over its grid-stride pixels, per wavefront by shuffles,
 * per workgroup, one row of partial_ws (pd_reproj_combine_rows(N,H,W) * 2 doubles, 8-byte aligned) per workgroup, then
 * one workgroup sums the rows (a second launch, like pd_loss_finalize).  Bit-reproducible, no host synchronisation.
 * pd_reproj_combine_bwd -- greproj (F device pointers, [N,1,H,W] fp32 out): gloss[0] / (sums[1] + 1e-7) in the winning
 * frame's map and 0 elsewhere; with avg that value / (number of valid frames) in every valid frame's map of an unmasked
 * pixel.  gloss: 1 float on the device. */
int pd_reproj_combine_rows(int N, int H, int W);
int pd_reproj_combine_fwd(const void* const* reproj, const void* const* identity, int F, const void* noise,
                          const void* valid, void* sel, void* partial_ws, void* sums, void* loss, int N, int H, int W,
                          int avg, void* stream);
int pd_reproj_combine_bwd(const void* gloss, const void* sel, const void* sums, const void* valid, void* const* greproj,
                          int F, int N, int H, int W, int avg, void* stream);

/* ------------------------------------------------------------------------- pose network tail (csrc/pose.hip)
 * The monodepth2 / ManyDepth setting: a pose network predicts the relative pose of two frames, and the photometric term
 * trains depth and pose together (trainer.py:222-236, 669-707; networks/pose_decoder.py; layers.py:74-149).
 *
 * pd_pose_matrix_fwd -- transformation_from_parameters(axisangle [N,3], translation [N,3], invert) -> T [N,4,4], fp32 in
 * and out.  Evaluated in fp64 from the fp32 inputs in the reference's order, each entry rounded once:
 *   angle = sqrt((a0 a0 + a1 a1) + a2 a2);  (x, y, z) = a / (angle + 1e-7);  ca = cos angle, sa = sin angle, C = 1 - ca
 *   xs = x sa, ys, zs;  xC = x C, yC, zC;  xyC = x yC, yzC = y zC, zxC = z xC
 *   R = [x xC + ca, xyC - zs, zxC + ys;  xyC + zs, y yC + ca, yzC - xs;  zxC - ys, yzC + xs, z zC + ca]
 *   invert == 0:  T = Trans(t) R = [R | t]
 *   invert == 1:  T = R^T Trans(-t) = [R^T | c],  c[i] = (R[0][i] (-t0) + R[1][i] (-t1)) + R[2][i] (-t2)
 *   last row (0, 0, 0, 1).
 * pd_pose_matrix_bwd -- gaxisangle, gtranslation [N,3] fp32 out ("=") from gT [N,4,4] fp32 (its last row is ignored), in
 * fp64, rounded once.  At angle == 0 the derivative of the norm is taken as 0 (PyTorch's rule), and the axisangle gradient
 * is then exactly 0.  One thread per item; N >= 0 (N = 0 does nothing).
 *
 * pd_pose_head_fwd -- the tail of PoseDecoder.forward from the input of ("pose", 2) on, and the two matrices of slot 0.
 *   x [N,h,w,Cin] NHWC fp32      w [Co,Cin], b [Co] fp32: the 1x1 convolution, Co = 6 nf
 *   axisangle, translation [N,nf,1,3] fp32 out      T, T_inv [N,4,4] fp32 out      mean [N,Cin] doubles out (8-byte aligned)
 * Per item, one workgroup of 256 threads:
 *   mean[c] = (sum over the pixels, ascending, of x[p][c] in fp64) / (h w)        (the mean commutes with a 1x1 convolution)
 *   o[k]    = fp32(0.01 * (b[k] + dot_k)),  dot_k = sum_c w[k][c] mean[c] in fp64: lane l of a wavefront sums
 *             c = l, l + 64, ... ascending, the 64 lanes are added by xor shuffles (32, 16, ... 1)
 *   axisangle[f] = o[6f .. 6f+2], translation[f] = o[6f+3 .. 6f+5]
 *   T = pd_pose_matrix_fwd(axisangle[0], translation[0], invert), T_inv the same with invert flipped (cam_T_cam and
 *   cam_T_cam_inv of trainer.py:694-707).
 * pd_pose_head_bwd -- gT, gT_inv [N,4,4], gaxisangle, gtranslation [N,nf,1,3] fp32: any may be NULL (= zero).
 *   gx [N,h,w,Cin] fp32 out ("=")      gw [Co,Cin], gb [Co] fp32, "=" or, with accumulate != 0, "+="
 *   gpre_ws  N * Co doubles of workspace, 8-byte aligned
 * In fp64: go = (gaxisangle | gtranslation) + for slot 0 the two pd_pose_matrix_bwd results; gpre = 0.01 go;
 * gx[p][c] = (sum_k w[k][c] gpre[k], k ascending) / (h w); gw[k][c] = sum_n gpre[n][k] mean[n][c] and gb[k] = sum_n
 * gpre[n][k], items ascending, one thread per element (a second launch).  Rows of gw / gb for slots >= 1 receive exactly 0
 * unless gaxisangle / gtranslation are given.  No atomics, no host synchronisation.
 * Limits of both: 0 <= N <= 65535 (N = 0 does nothing), h, w > 0, h w <= 2^20, Cin a multiple of 64 and <= 1024, Co a
 * multiple of 6 and <= 384, invert 0 or 1.  Meant for the decoder's small plane (1/32 of the image: a few hundred pixels):
 * one thread per channel walks the pixels of its item serially, forward for the mean (the stated ascending order) and
 * backward for gx, so the time grows with h w on Cin threads per item; a large plane is legal but slow. */
int pd_pose_matrix_fwd(const void* axisangle, const void* translation, void* T, int N, int invert, void* stream);
int pd_pose_matrix_bwd(const void* gT, const void* axisangle, const void* translation, void* gaxisangle, void* gtranslation,
                       int N, int invert, void* stream);
int pd_pose_head_fwd(const void* x, const void* w, const void* b, void* axisangle, void* translation, void* T, void* T_inv,
                     void* mean, int N, int h, int wd, int Cin, int Co, int invert, void* stream);
int pd_pose_head_bwd(const void* gT, const void* gT_inv, const void* gaxisangle, const void* gtranslation,
                     const void* axisangle, const void* translation, const void* w, const void* mean, void* gx, void* gw,
                     void* gb, void* gpre_ws, int N, int h, int wd, int Cin, int Co, int invert, int accumulate, void* stream);

/* pd_pose_chain -- the matching-pose half of predict_poses (trainer.py:708-746): the poses 0 -> fi of a chain of L
 * consecutive frames in ONE launch, forward only (the reference runs it under no_grad).
 *   axisangle, translation  [L,N,3] fp32: link k is the pose network's slot-0 output for the pair (frame s (k+1), frame s k)
 *                           stacked in temporal order, s = direction (-1: the past frames -1, -2, ...; +1: the future ones)
 *   present                 [L,N] fp32, or NULL = all present: 0 means frame s (k+1) of item n does not exist
 *   init                    [N,4,4] fp32, or NULL: the pose 0 -> frame 0 of the chain to continue from (streaming use)
 *   rel, rel_inv            [L,N,4,4] fp32 out ("=")
 * Per item n, k ascending:
 *   M_k    = pd_pose_matrix_fwd(axisangle[k], translation[k], invert = (s < 0)), rounded to fp32 exactly as there
 *            (trainer.py:718-719, 731-732);  Minv_k the same with invert flipped (:720-721, 733-734)
 *   A_k    = M_k A_{k-1} (:725, 738), A_{-1} = init; without init A_0 = M_0.  Each entry is
 *            ((m_i0 a_0c + m_i1 a_1c) + m_i2 a_2c) + m_i3 a_3c in fp64 from the fp32 values of M_k and of the STORED A_{k-1}
 *            (what rel[k-1] holds, or init), no fused multiply-add, rounded once
 *   rel[k] = A_k where present[k][n] != 0, else sixteen 0.0f -- and the next link multiplies those zeros: the reference
 *            stores the zeroed pose and reads it back (:725, 741-745).  A zero therefore travels down the chain by
 *            arithmetic alone; a NaN pose stays NaN, in its own item only.
 *   rel_inv[k] = Minv_k: the link's OWN inverse, neither chained nor zeroed.  This is what the reference stores in
 *            ("relative_pose_inv", fi) (:720-721, 746) -- a quirk kept on purpose; it is not the inverse of rel[k] for k > 0.
 * One thread per item walks the links (64-thread groups); no atomics, no host synchronisation, capturable.
 * Limits: 1 <= L <= PD_POSE_CHAIN_MAX_LINKS, N >= 1, direction -1 or 1; anything else, or a NULL among axisangle,
 * translation, rel, rel_inv, is PD_EINVAL before any launch. */
#define PD_POSE_CHAIN_MAX_LINKS 8
int pd_pose_chain(const void* axisangle, const void* translation, const void* present, const void* init, void* rel,
                  void* rel_inv, int L, int N, int direction, void* stream);

/* Pose supervision and the records of the pose evaluator (csrc/pose_loss.hip): --supervise_pose of trainer.py:1267-1285, the
 * predicted cam_T_cam against the ground-truth relative pose, rotations compared as rotation vectors.
 *
 * rv(M) for a 3x3 block M -- roma.rotmat_to_rotvec, i.e. roma.rotmat_to_unitquat followed by roma.unitquat_to_rotvec, which
 * roma adapted from SciPy's Rotation.from_matrix / as_rotvec.  In fp64 from the fp32 values, every expression in its order, no
 * fused multiply-add:
 *   tr = (M00 + M11) + M22;  c = the index of the FIRST maximum of (M00, M11, M22, tr)
 *   c < 3, i = c, j = (i + 1) % 3, k = (j + 1) % 3:
 *     q[i] = (1 - tr) + 2 M[i][i];  q[j] = M[j][i] + M[i][j];  q[k] = M[k][i] + M[i][k];  q[3] = M[k][j] - M[j][k]
 *   c == 3:  q = (M21 - M12, M02 - M20, M10 - M01, 1 + tr)
 *   q = q / sqrt(((q0 q0 + q1 q1) + q2 q2) + q3 q3)   (four divisions);  q = -q where q3 < 0
 *   s = sqrt((q0 q0 + q1 q1) + q2 q2);  angle = 2 atan2(s, q3)
 *   scale = (2 + angle^2 / 12) + 7 (angle^2 angle^2) / 2880 where angle <= 1e-3, else angle / sin(angle / 2)
 *   rv = scale * (q0, q1, q2)
 * Near angle = pi the sign of rv is discontinuous (q3 changes sign, or the branch c changes); so it is in the reference, and
 * nothing here smooths it.  M need not be orthogonal; a non-finite entry propagates into rv.
 *
 * pd_pose_loss_fwd
 *   T_pred, T_gt   host arrays of F device pointers (1 <= F <= PD_REPROJ_MAX_FRAMES, as pd_reproj_combine_fwd), each [N,4,4] fp32
 *   frame_weight   F host floats
 *   valid          [N,F] fp32, 0 = item n has no frame f and does not count, or NULL: all count
 *   records        [F,N,10] doubles out (8-byte aligned) or NULL, written for invalid items too:
 *                  rv(R_pred) (3), rv(R_gt) (3), |rv(D)| with D[i][j] = (R_pred[0][i] R_gt[0][j] + R_pred[1][i] R_gt[1][j]) +
 *                  R_pred[2][i] R_gt[2][j] (the geodesic angle of R_pred^T R_gt, radians), |t_pred - t_gt|, |t_pred|, |t_gt|
 *                  (norms: sqrt((x x + y y) + z z); t = T[:3,3])
 *   vals           3 + 2 F floats out
 * Per frame f, in fp64: cnt_f = the number of items with valid != 0 (N without valid);
 *   e_r[n] = sum_k (rv(R_pred)[k] - rv(R_gt)[k])^2, e_t[n] = sum_k (t_pred[k] - t_gt[k])^2, k ascending
 *   r_f = 0.1 * ((sum of e_r over the valid n) / (3 cnt_f)),  t_f = (sum of e_t over the valid n) / (3 cnt_f);  both 0 when cnt_f == 0
 *   vals[0] = sum_f r_f, vals[1] = sum_f t_f, vals[2] = sum_f frame_weight[f] (r_f + t_f)  (f ascending),
 *   vals[3 + 2f] = r_f, vals[4 + 2f] = t_f, each rounded once to fp32.
 * One workgroup of 256 threads: thread t sums its items t, t + 256, ... ascending, the 64 lanes of a wavefront by xor shuffles
 * (32, 16, ... 1), the four wavefronts ((w0 + w1) + w2) + w3.  Bit-reproducible, no atomics, no host synchronisation.
 *
 * pd_pose_loss_bwd -- gvals: 3 floats ON THE DEVICE, the gradients of vals[0..2] (vals[3..] carry none); gT: host array of
 * F device pointers [N,4,4] fp32, written with "=".  One thread per (frame, item), in fp64, rounded once; with
 * a_r = gvals[0] + frame_weight[f] gvals[2], a_t = gvals[1] + frame_weight[f] gvals[2]:
 *   gT[:3,:3] = (a_r * 0.1 * 2 / (3 cnt_f)) * J^T (rv(R_pred) - rv(R_gt)),  gT[:3,3] = (a_t * 2 / (3 cnt_f)) * (t_pred - t_gt),
 *   last row 0; an invalid item receives 16 zeros; the ground truth receives no gradient.
 * J = d rv / d M of the expressions above as written: the branch c is fixed, the sign flip is a constant factor, the
 * small-angle polynomial is differentiated in its own branch (angle / 6 + 7 angle^3 / 720), and d sqrt(x) / dx is taken as 0 at
 * x == 0 (PyTorch's rule for norm, as in pd_pose_matrix_bwd), so that at the identity d rv / d M is (M21 - M12) / 2, ...
 * Limits of both: 0 <= N <= 65535; N == 0 writes zeros into vals (forward) and touches nothing else (the matrix pointers may
 * then be null).  Parity with roma itself is pinned through SciPy's identical algorithm (tests/test_pose_loss_ref.py). */
int pd_pose_loss_fwd(const void* const* T_pred, const void* const* T_gt, int F, const float* frame_weight, const void* valid,
                     void* records, void* vals, int N, void* stream);
int pd_pose_loss_bwd(const void* gvals, const void* const* T_pred, const void* const* T_gt, int F, const float* frame_weight,
                     const void* valid, void* const* gT, int N, void* stream);

/* ------------------------------------------------------------------------- multi-frame cost volume (csrc/matching.hip)
 * pd_cost_volume -- ManyDepth's plane sweep from known poses: ResnetEncoderMatching.match_features, compute_confidence_mask
 * and the lowest-cost map (resnet_encoder.py:430-511, 534-541, 620-630), forward only (the reference runs it under no_grad).
 *   cur     [B,h,w,C] fp32 NHWC, 16-byte aligned         features of the current frame (1/4 resolution)
 *   lookup  [B,F,h,w,C] fp32 NHWC, 16-byte aligned       features of the F lookup frames
 *   T       [B,F,4,4] fp32 row-major                     relative pose, current camera -> lookup camera
 *   K, inv_K [B,4,4] fp32                                intrinsics of the feature resolution
 *   bins    [D] fp32 ON THE DEVICE                       hypothesised depths, read by the kernel: new bins need no rebuild and
 *                                                        no host synchronisation
 *   valid   [B,F] fp32 or NULL                           0 = frame f of item b is skipped (NULL: none is)
 *   cost    [B,h,w,D] fp32 out, pixel stride ldc >= D floats: ldc > D writes into channels of a wider NHWC buffer (the
 *           input of reduce_conv, beside the 64 feature channels) and leaves its other channels alone
 *   missing [B,h,w,D] uint8 out or NULL      confidence [B,h,w] fp32 out (0 / 1)
 *   argmin  [B,h,w] int32 out                lowest [B,h,w] fp32 out = 1 / bins[argmin]
 * 1. Per item and frame, in fp64 from the fp32 inputs, sums left to right, no fused multiply-add (as pd_view_synth_fwd):
 *      P[i][j] = K[i][0] T[0][j] + K[i][1] T[1][j] + K[i][2] T[2][j] + K[i][3] T[3][j]      (i < 3)
 *    A frame with valid[b][f] == 0 is skipped entirely.  (polardepth.ops.cost_volume also clears valid where the 16
 *    elements of T[b][f] sum to 0, the reference's "missing frame" rule, :463.)
 * 2. Per pixel (x, y) and bin d, in fp64 likewise:
 *      r[i] = inv_K[i][0] x + inv_K[i][1] y + inv_K[i][2];   p = bins[d] * r;
 *      hh[i] = P[i][0] p[0] + P[i][1] p[1] + P[i][2] p[2] + P[i][3];
 *      u = hh[0] / (hh[2] + 1e-7),  v = hh[1] / (hh[2] + 1e-7), each rounded once to fp32.
 *    Project3D's normalisation and grid_sample's align_corners=True un-normalisation cancel: (u, v) are pixel coordinates
 *    of the lookup frame.  A point behind the lookup camera is NOT rejected (the reference does not reject it).
 * 3. Edge mask, decided on the fp32 coordinates (a NaN gives 0):
 *      m = (u >= 2) && (u <= w-2) && (v >= 2) && (v <= h-2) && (2 <= x < w-2) && (2 <= y < h-2).
 *    Where m = 1 all four bilinear taps lie inside the image, so the reference's padding_mode='zeros' never shows in a
 *    value that is used: the kernel samples ONLY where m = 1, needs no clamp, and reads nothing for the other entries.
 * 4. Where m = 1, in fp32 without fused multiply-add: x0 = floor(u), wx1 = u - x0, wx0 = 1 - wx1 (y likewise),
 *      warped_c = ((L[y0][x0][c] (wx0 wy0) + L[y0][x0+1][c] (wx1 wy0)) + L[y0+1][x0][c] (wx0 wy1)) + L[y0+1][x0+1][c] (wx1 wy1)
 *      diff = (sum_c |warped_c - cur_c|) / (float)C
 *    The order of the channel sum: 16 partial sums, partial l adding channels 4l, 4l+1, 4l+2, 4l+3, then 64 + 4l, ... in
 *    ascending order from 0 (a partial without channels is 0); then a binary tree: partials (0,1), (2,3), ... are added,
 *    then those pairs' sums pairwise, four levels in all.
 * 5. Over the valid frames in frame order, where m = 1:  s += diff;  n += (diff > 0).
 * 6. c = s / ((float)n + 1e-7f), in fp32 exactly as written (the reference's fp32 run: 1 + 1e-7 rounds up, 2 + 1e-7 not).
 * 7. Per pixel over its D bins: missing = (c == 0); mx = max_d c (NaN if any c is NaN); filled = missing ? mx : c;
 *    confidence = (number of bins with c > 0) == D; argmin = the FIRST index of the minimum of (filled == 0 ? 100 : filled),
 *    where a NaN counts as below every number (the first NaN wins, as numpy.argmin); lowest = 1 / bins[argmin];
 *    cost = filled, or filled * confidence when apply_confidence != 0 (resnet_encoder.py:630).
 * 8. Non-finite features and poses propagate through these expressions and no further: a NaN coordinate masks its entry,
 *    a NaN feature makes the sums it enters NaN; nothing of one batch item reaches another.
 * A pixel outside the interior, an item without a valid frame and F = 0 give cost 0, missing 1, confidence 0, argmin 0.
 * Limits: C % 4 == 0 (C >= 4), 1 <= D <= 128, 0 <= F <= PD_REPROJ_MAX_FRAMES, h, w >= 1, h * w <= 2^30, 0 <= B <= 65535
 * (B = 0 does nothing), ldc >= D.  One launch, no atomics, no workspace, no host synchronisation; bit-reproducible. */
int pd_cost_volume(const void* cur, const void* lookup, const void* T, const void* K, const void* inv_K, const void* bins,
                   const void* valid, void* cost, long ldc, void* missing, void* confidence, void* argmin, void* lowest,
                   int B, int F, int h, int w, int C, int D, int apply_confidence, void* stream);

/* ------------------------------------------------------------------------- cost-volume student's step (csrc/student.hip)
 * The reference's --train_student branch (trainer.py:567-664, 1112-1124, 1202-1236): the multi-frame network is trained
 * with the reprojection loss where the cost volume can be trusted and pulled towards the teacher's depth where it cannot.
 * Streaming kernels, four x-neighbouring pixels per thread (16-byte accesses); no atomics, no host synchronisation.
 *
 * pd_student_masks -- once per step, independent of the scale.
 *   lowest, confidence [N,h,w] fp32       as pd_cost_volume writes them (confidence 0 / 1)
 *   mono_depth [N,1,H,W] fp32             the teacher's scale-0 depth at full resolution, 16-byte aligned
 *   aug [N] fp32 or NULL                  != 0: the item was augmented (static frame / zero pose), NULL: none was
 *   motion_masking 0 / 1                  0 = --disable_motion_masking
 * H == 4h and W == 4w are required.  F.interpolate(mode="nearest") reads source index floor(dst * (in / out)) with the
 * scale in / out computed in fp32; for out = 4 * in that scale is exactly 0.25, dst * 0.25 is exact, and its floor is
 * dst >> 2: the nearest source of pixel (y, x) is (y >> 2, x >> 2), bit for bit what the reference reads.
 * Per pixel, all in fp32, every operation rounded once, a comparison with a NaN false:
 *   l = lowest[n][y>>2][x>>2];  md = 1.0f / l;  t = mono_depth[n][0][y][x]
 *   mm    = ((md - t) / t < 1) && ((t - md) / md < 1)                              compute_matching_mask
 *   cmask = (confidence[n][y>>2][x>>2] != 0) && (!motion_masking || mm)
 *   rmask = (!motion_masking || cmask) && !(aug && aug[n] != 0)
 *   rmask     [N,H,W] uint8 out, 4-byte aligned: where the reprojection loss applies
 *   cmask     [N,H,W] fp32 out (0 / 1) or NULL, 16-byte aligned: outputs["consistency_mask"]
 *   lowest_up [N,H,W] fp32 out (= l) or NULL, 16-byte aligned: outputs["lowest_cost"]
 *   minmax    [N,2] fp32 out: the minimum and the maximum of mono_depth over item n, both NaN if the item holds a NaN
 *   partial_ws  N * pd_student_masks_rows(N, h, w) * 2 floats: one (min, max) pair per workgroup; a second launch with one
 *               workgroup per item reduces them (minimum and maximum do not depend on the order).
 * Limits: 0 <= N <= 65535 (N = 0 does nothing), h, w >= 1, h * w <= 2^26.
 *
 * pd_depth_bins_update -- update_adaptive_depth_bins (trainer.py:650-664) and compute_depth_bins (resnet_encoder.py:
 * 406-420) in one workgroup, with no host round trip (the reference synchronises twice per step here).
 *   minmax [N,2] fp32 (N >= 1)    tracker: 2 doubles on the device, 8-byte aligned, in and out: (min, max)
 *   floor_depth = opt.min_depth   bins [D] fp32 out, 1 <= D <= 128   binning PD_BINS_LINEAR / PD_BINS_INVERSE
 *   mn = (fp32 sum of minmax[n][0], n ascending) / (float)N;   mx likewise over minmax[n][1]
 * then in fp64, every product and sum rounded on its own (no fused multiply-add):
 *   lo = mn * 0.9;  mn64 = lo > floor_depth ? lo : floor_depth  (Python's max(floor, lo): a NaN gives floor);  mx64 = mx * 1.1
 *   tracker[1] = tracker[1] * 0.99 + mx64 * 0.01;   tracker[0] = tracker[0] * 0.99 + mn64 * 0.01
 * bins = polardepth.matching.depth_bins(tracker[0], tracker[1], D, binning), bit for bit.  numpy.linspace(start, stop, D) in
 * fp64 is: delta = stop - start, step = delta / (D - 1), y[j] = j * step (or (j / (D - 1)) * delta when step == 0), then
 * y[j] + start, and y[D-1] = stop; with D == 1, y[0] = 0 * delta + start.  linear: start, stop = tracker[0], tracker[1] and
 * bins[i] = (float)y[i]; inverse: start, stop = 1 / tracker[1], 1 / tracker[0] and bins[i] = (float)(1 / y[D-1-i]).
 * The step's own plane sweep has already read the old bins: the update is enqueued after the losses.
 *
 * pd_student_combine_fwd -- the is_multi branch of compute_losses (trainer.py:1202-1236) for one scale.
 *   reproj    host array of F <= PD_REPROJ_MAX_FRAMES device pointers to [N,1,H,W] fp32 maps, valid [N,F] fp32 or NULL, avg:
 *             as pd_reproj_combine_fwd; m = the minimum (first valid frame, a later one only when strictly smaller) or the
 *             mean over the valid frames, 0 without one.  No identity maps: the reference overwrites its automask with ones.
 *   rmask [N,H,W] uint8 (pd_student_masks)      multi_depth, mono_depth [N,1,H,W] fp32
 *   r = (rmask != 0 && the item has a valid frame) ? 1.0f : 0.0f
 *   sel  [N,H,W] uint8 out: the winning frame (0 with avg), 255 where r = 0
 *   sums 3 doubles out: sum(m * r), sum(r), sum(|multi - mono| * (1 - r)); every term is formed in fp32 as written -- a
 *        real product, so a NaN under the mask propagates as in the reference -- and added in fp64 in the fixed order of
 *        pd_reproj_combine_fwd (the same two-stage reducer, csrc/frame_reduce.hpp; a thread adds its four pixels in x order)
 *   loss 2 floats out: sums[0] / (sums[1] + 1e-7) and sums[2] / (N * H * W)        (reproj_loss, consistency_loss)
 *   partial_ws pd_student_combine_rows(N,H,W) * 3 doubles, 8-byte aligned.
 * pd_student_combine_bwd -- gloss: 2 floats on the device.
 *   greproj (F device pointers, [N,1,H,W] fp32 out) as pd_reproj_combine_bwd defines it from sel, sums[1] and gloss[0]
 *   gmulti [N,1,H,W] fp32 out = ((float)(gloss[1] / (N * H * W)) * sign(multi - mono)) * (1 - r)
 *   sign(0) = 0 and sign(NaN) = 0: torch.sign returns 0 for a NaN on the CPU, and abs' backward is grad * sign.
 *   No gradient reaches mono_depth or the masks.
 * Both need H % 4 == 0 and W % 4 == 0 (what pd_student_masks produces), the fp32 maps 16-byte and the uint8 maps 4-byte
 * aligned, H * W <= 2^30; N = 0 does nothing.  Bit-reproducible. */
#define PD_BINS_LINEAR 0
#define PD_BINS_INVERSE 1
int pd_student_masks_rows(int N, int h, int w);
int pd_student_masks(const void* lowest, const void* confidence, const void* mono_depth, const void* aug, int motion_masking,
                     void* rmask, void* cmask, void* lowest_up, void* minmax, void* partial_ws, int N, int h, int w, int H,
                     int W, void* stream);
int pd_depth_bins_update(const void* minmax, int N, void* tracker, double floor_depth, int D, int binning, void* bins,
                         void* stream);
int pd_student_combine_rows(int N, int H, int W);
int pd_student_combine_fwd(const void* const* reproj, int F, const void* valid, const void* rmask, const void* multi_depth,
                           const void* mono_depth, void* sel, void* partial_ws, void* sums, void* loss, int N, int H, int W,
                           int avg, void* stream);
int pd_student_combine_bwd(const void* gloss, const void* sel, const void* sums, const void* valid, const void* multi_depth,
                           const void* mono_depth, void* const* greproj, void* gmulti, int F, int N, int H, int W, int avg,
                           void* stream);

/* compute_depth_errors (layers.py:539-557) per image on the device: metrics [N][8] = abs_rel, sq_rel, rmse,
 * rmse_log, a1, a2, a3, pixel count over min < gt < max (and mask == mask_value when mask != NULL, the
 * per-material selection of trainer.py:1385-1411); pred is clamped to [min, max] (trainer.py:1422-1423).
 * partial_ws: N * 64 * 8 floats. */
int pd_depth_metrics(const void* gt, const void* pred, const void* mask, int mask_value, void* partial_ws,
                     void* metrics, int N, long P, float min_depth, float max_depth, void* stream);

/* Surface-normal accuracy per pixel class (csrc/normals_stats.hip): the angular error of predicted normals against the
 * normals of the ground-truth depth, for K classes of the instance mask at once, in one read of the batch.  The reference
 * stops at depth (evaluation.py:120-288); this is the standard normals report (mean / median / RMS angle, share of pixels
 * within 11.25 / 22.5 / 30 degrees) as per-image, per-class records from which all of these follow.
 *
 * pred       fp32 device, pixel-major, pixel stride ld >= 3 floats (x, y, z first): ld = 3 is a channels-last [N,3,H,W]
 *            tensor, ld = 4 what pd_gt_normals writes.  Need not be unit length.
 * gtn        fp32 [N,H,W,4] from pd_gt_normals
 * gt         fp32 [N,H,W] ground-truth depth
 * mask       int32 [N,H,W] or NULL
 * classes    HOST int[K][2], read during the call and passed as kernel arguments; 1 <= K <= PD_NSTAT_MAX_CLASSES.  Class k
 *            holds the pixels with lo <= mask <= hi (evaluation.py:242-267: mask_gt >= thres1 & mask_gt <= thres2);
 *            lo > hi = every pixel.  A pixel may be in several classes.
 * cos_edges  DEVICE double[719], cos_edges[j-1] = cos(j * 0.25 degrees) for j = 1 .. 719, strictly decreasing.  The caller
 *            supplies it, so that whoever checks a histogram bins against the same 719 doubles whatever libm built them.
 * gate       0: the pixel's depth gt is inside [min_depth, max_depth] (>=, <=: the gate of pd_gt_normals).  1: all nine
 *            depths of the replicate-clamped 3x3 window are -- the Sobel normal of a pixel beside a hole of the depth map
 *            is an artefact of the hole.
 * err_deg    NULL, or fp32 [N,H,W]: the angle in degrees where the pixel passes the gate and is valid (below), NaN
 *            elsewhere, whatever its class
 * stats      [N][K] records on the device, written whole by every call; byte offsets:
 *      0  int64   n          valid pixels of the class
 *      8  int64   bad        pixels of the class that pass the gate but are not valid
 *     16  double  sum_deg    sum of the angle in degrees over the valid pixels
 *     24  double  sum_deg2   sum of its square
 *     32  uint32  hist[720]  0.25-degree bins over [0, 180]
 * workspace  caller-owned, >= pd_normals_stats_workspace(N, H, W, K) bytes (monotone in each argument, never 0, a multiple
 *            of 16); scratch
 *
 * Per pixel that passes the gate, every fp32 component converted to fp64 first (all products are then exact), in this order:
 *     d  = (px gx + py gy) + pz gz,   a2 = (px px + py py) + pz pz,   b2 = (gx gx + gy gy) + gz gz,
 *     c  = d / (sqrt(a2) sqrt(b2)).
 * The pixel is VALID when a2 > 0, b2 > 0 and c is finite; otherwise it adds 1 to `bad` of each of its classes and to nothing
 * else (a NaN or zero prediction is counted, not averaged).  For a valid pixel c is clamped to [-1, 1]; its bin is
 * #{ j : c <= cos_edges[j-1] }, found by binary search -- no acos takes part in a bin decision; exactly parallel normals
 * land in bin 0, exactly orthogonal ones in bin 360, antiparallel ones in bin 719.  theta = acos(c) * 57.29577951308232 is
 * added to sum_deg and theta * theta to sum_deg2 of each of its classes.
 * n, bad and hist are integer sums and do not depend on any order (LDS atomics, then one global add per non-empty bin per
 * workgroup).  The two fp64 sums are bit-reproducible from run to run: lanes, waves and workgroups add in an order fixed by
 * the shape, per-workgroup partials go through `workspace`, and a small last launch adds them in index order -- the scheme
 * of pd_xolp_stats; no floating-point atomics, no cross-workgroup ticket.  Any order of n exactly converted terms errs by at
 * most (n - 1) 2^-53 of the sum.
 * Three launches per 2^20 images, no allocation, copy or synchronisation: the call can be captured into a graph.  Offsets
 * inside a frame are 32-bit; a frame beyond 2^30 pixels is refused ("too large").  N == 0 returns PD_OK.  Every refusal is
 * PD_EINVAL with a message, decided before the device is touched: a null pred / gtn / gt / classes / cos_edges / stats /
 * workspace, ws_bytes too small, K outside 1 .. 16, a ranged class with mask == NULL, ld < 3, gate not 0 or 1, gtn / stats /
 * workspace not 16-byte aligned, bad shape. */
#define PD_NSTAT_BINS         720      /* 0.25 degree bins over [0, 180] */
#define PD_NSTAT_MAX_CLASSES  16
#define PD_NSTAT_RECORD_BYTES 2912     /* 32 + 4 * 720 */
size_t pd_normals_stats_workspace(int N, int H, int W, int K);
int pd_normals_stats(const void* pred, long ld, const void* gtn, const void* gt, const void* mask,
                     const int* classes, int K, const void* cos_edges, int gate, void* err_deg,
                     void* stats, void* workspace, size_t ws_bytes, int N, int H, int W,
                     float min_depth, float max_depth, void* stream);

/* Point-cloud accuracy (csrc/pointcloud.hip): the surface distance between the cloud of a predicted depth map and the cloud
 * of the ground truth -- accuracy, completeness, Chamfer distance, precision / recall / F-score at 5 / 10 / 20 mm -- per
 * image and pixel class.  The reference back-projects both depth maps through the camera matrix
 * (pointcloud/eval_pointcloud.py:256-291, :83-85) and shows them in a viewer; these three calls measure what that demo is
 * looked at for.  tests/pointcloud_ref.py states the definition in NumPy.
 *
 * TILED CLOUD.  The cloud of one image is T tiles of PD_PCD_TILE = 256 point slots:
 *   points  fp32 [N][T * 256][4] = (x, y, z, w), 16-byte aligned.  w = 1: a point.  w = 0: no point (outside the image, or
 *           gated out), x = y = z = 0.  w = -1: a "bad" point (inside the gate, but its depth is non-finite or <= 0),
 *           x = y = z = 0.
 *   boxes   [N][T] records of 32 bytes, 16-byte aligned:
 *              0  float lo[3]   min of x, y, z over the w = 1 slots of the tile (+inf each for an empty tile)
 *             12  float hi[3]   max of x, y, z (-inf each for an empty tile)
 *             24  int32 count   the number of w = 1 slots
 *             28  int32 0
 * pd_cloud_nn does not care what the tiles are: any partition of a cloud into 256-slot tiles with correct boxes gives the
 * same distances; compact tiles only make the boxes tight.
 *
 * pd_backproject: depth fp32 [N,H,W], K fp32 [N,4,4] (fx = K[0][0], fy = K[1][1], cx = K[0][2], cy = K[1][2]), gate fp32
 * [N,H,W] or NULL -> points and boxes with T = ceil(H/16) * ceil(W/16): the 16x16 pixel tiles in row-major tile order, slots
 * row-major inside the tile, slots outside the image w = 0.  A pixel is in the cloud iff the gate depth (gate == NULL: the
 * depth itself) is inside [min_depth, max_depth] (>=, <=, NaN fails: the gate of pd_gt_normals).  Inside the gate a depth
 * that is non-finite or <= 0 gives w = -1.  Otherwise z = depth (copied), x = ((u - cx) / fx) * z, y = ((v - cy) / fy) * z
 * with u, v the integer column and row, every operation rounded to fp32: the pinhole model of create_from_rgbd_image without
 * the reference's display flip.  One launch.
 *
 * pd_cloud_nn: d2 fp32 [N][Tq * 256].  For a w = 1 query, d2 = the minimum over the w = 1 targets of the same image of
 *     ((dx * dx + dy * dy) + dz * dz),   dx = qx - tx, dy = qy - ty, dz = qz - tz,
 * every operation rounded to fp32, nothing fused; +inf when the target cloud of that image has no point.  For a query with
 * w != 1: NaN.  A minimum does not depend on the order of its terms, so this is a bit-exact definition.
 * flags: 0 = pruned, PD_PCD_BRUTE = scan every target tile.  visited: NULL or int32 [N][Tq], the number of target tiles
 * scanned for that query tile.
 * Pruning (exact).  One wave owns a query tile and keeps R = the maximum over the tile's w = 1 queries of their best d2 so
 * far (+inf until each of them has a finite one).  It scans the target tile of the same index first (if there is one and it
 * holds a point) and any other target tile only if it holds a point and boxd2 <= R at that moment, where
 *     boxd2 = ((gx * gx + gy * gy) + gz * gz),   g = max(0, lo_t - hi_q, lo_q - hi_t) per axis,
 * in fp32 and in the operation order of the point distance.  fp32 rounding is monotone, so boxd2 is a lower bound of the
 * COMPUTED d2 of every pair of points from the two boxes, and a skipped tile cannot hold a smaller value for any query of
 * the tile.  R is refreshed after every scanned tile.  A query tile without a w = 1 slot writes its NaNs and leaves (visited
 * 0); under PD_PCD_BRUTE every query tile scans all Tt tiles (visited = Tt).
 *
 * pd_cloud_stats: one direction's records.  d2 and points are the query side of pd_cloud_nn with the tiling of
 * pd_backproject for H x W (the slot -> pixel map); mask int32 [N,H,W] or NULL; classes HOST int[K][2] as in
 * pd_normals_stats (lo > hi = every pixel; a ranged class needs a mask); edges2 DEVICE float[511], edges2[j-1] = the fp32
 * rounding of (j * 0.0005 m)^2 computed in fp64, supplied by the caller; dist NULL or fp32 [N,H,W].
 * stats: [N][K] records, written whole by every call; byte offsets:
 *      0  int64   n           slots of the class with w = 1 and a finite d2 (the sum of the bins)
 *      8  int64   bad         slots of the class with w = -1
 *     16  int64   unmatched   slots of the class with w = 1 and d2 = +inf
 *     24  double  sum_d       sum of sqrt((double)d2) in metres over the n slots
 *     32  double  sum_d2      sum of (double)d2
 *     40  8 bytes of zero
 *     48  uint32  hist[512]   bin = #{ j : edges2[j-1] <= d2 }: 0.5 mm bins, the last one open-ended; 5 / 10 / 20 mm are
 *                             bin edges (bins 0..9, 0..19, 0..39 lie below them).  No square root takes part in a bin.
 * dist: (float)sqrt((double)d2) where the pixel's slot has w = 1 (+inf where unmatched), NaN elsewhere.
 * The integer fields are exact; the two sums are bit-reproducible (fixed lane, wave and workgroup order, partials through
 * `workspace`, no floating-point atomics, no cross-workgroup ticket: the scheme of pd_normals_stats).
 * workspace: >= pd_cloud_stats_workspace(N, H, W, K) bytes (never 0, a multiple of 16, monotone), 16-byte aligned.
 *
 * No call synchronises, allocates or reads the environment.  N == 0 returns PD_OK after the checks.  Every refusal is
 * PD_EINVAL with a message, decided before the device is touched: null pointers, points / boxes / stats / workspace not
 * 16-byte aligned, K outside 1 .. 16, a ranged class with mask == NULL, non-positive shapes or tile counts, a frame whose
 * slot offsets exceed 32 bits ("too large"), unknown flag bits, a too-small workspace (naming the needed size). */
#define PD_PCD_TILE         256
#define PD_PCD_BINS         512       /* 0.5 mm bins, the last one open-ended */
#define PD_PCD_MAX_CLASSES  16
#define PD_PCD_RECORD_BYTES 2096      /* 48 + 4 * 512 */
#define PD_PCD_BRUTE        1u
int pd_backproject(const void* depth, const void* K, const void* gate, void* points, void* boxes, int N, int H, int W,
                   float min_depth, float max_depth, void* stream);
int pd_cloud_nn(const void* q_points, const void* q_boxes, int Tq, const void* t_points, const void* t_boxes, int Tt,
                void* d2, void* visited, unsigned flags, int N, void* stream);
size_t pd_cloud_stats_workspace(int N, int H, int W, int K);
int pd_cloud_stats(const void* d2, const void* points, const void* mask, const int* classes, int K, const void* edges2,
                   void* dist, void* stats, void* workspace, size_t ws_bytes, int N, int H, int W, void* stream);

/* Depth accuracy per pixel class (csrc/depth_stats.hip): the figures of compute_depth_errors (layers.py:539-577) -- abs_rel,
 * sq_rel, rmse, rmse_log, a1, a2, a3 -- and the distribution of the absolute error, for K classes of the instance mask at
 * once, in one read of the batch; and the exact per-class medians that median scaling needs (trainer.py:1344, :1416).
 * tests/depth_stats_ref.py states the definition in NumPy.
 *
 * gt, pred   fp32 [N,H,W] on the device; mask int32 [N,H,W] or NULL; classes HOST int[K][2] as in pd_normals_stats
 *            (lo > hi = every pixel; a ranged class needs a mask); 1 <= K <= PD_DSTAT_MAX_CLASSES.
 * PIXEL SET  S(n,k) = the pixels of image n with min_depth < gt < max_depth (strict, NaN fails: the gate of
 *            pd_depth_metrics and of the reference), in class k, with a finite pred.  A pixel that passes the gate and the
 *            class but whose pred is NaN or +-inf adds 1 to `bad` of that class and takes part in nothing else.
 *            p0 = fminf(fmaxf(pred, min_depth), max_depth).  min_depth > 0 and max_depth > min_depth are required;
 *            max_depth = +inf is allowed.
 *
 * pd_depth_medians: count int64 [N][K] = |S(n,k)|; med fp32 [N][K][4] = the order statistics of rank (n-1)/2 and n/2
 * (integer division) of gt, then of rank (n-1)/2 and n/2 of p0, over S(n,k): the very bit patterns a sort would put at those
 * ranks.  NaN where n = 0.  Every value is positive, so the unsigned order of the bit patterns is the order of the floats:
 * a radix selection, eight bits a pass from the top, four passes.  A pass is two launches: a histogram kernel (the image's
 * pixels round-robin over its workgroups; a workgroup counts, in LDS with integer atomics, the current digit of the values
 * that match the digits already chosen -- one 256-bin histogram per class, quantity and rank -- and adds its non-zero bins
 * to the global histogram with integer atomics), and a one-workgroup-per-(n,k) kernel that finds the bin holding the rank
 * and narrows the prefix.  The first pass yields n, from which the device derives the two ranks.  Nine launches per 2^20
 * images; no sort, no allocation, no synchronisation, no floating-point atomics, no cross-workgroup ticket: the call can be
 * captured into a graph.  workspace: >= pd_depth_medians_workspace(N, K) bytes, 16-byte aligned.
 *
 * pd_depth_stats: scale NULL or DEVICE fp32 [N][K]; edges DEVICE double[511], edges[j-1] = j * 0.0005 (metres), supplied by
 * the caller like the tables of the other two evaluators; err NULL or fp32 [N,H,W].
 * Per pixel of S(n,k):  p = p0 without a scale, else p = fminf(fmaxf(p0 * scale[n][k], min_depth), max_depth), every
 * operation in fp32 and in this order (trainer.py:1416-1419).  A non-finite scale[n][k] makes every pixel of the class that
 * passes the gate `bad` for that image.  With g = gt:
 *   a1, a2, a3   count fmaxf(g / p, p / g) < 1.25, 1.5625, 1.953125, decided in fp32 with IEEE division: the reference's own
 *                expression, so the counts are exact against it.
 *   the sums     g and p widened to fp64; d = g - p (exact); |d| / g, d * d / g, d * d and l * l with l = log1p(d / p), added
 *                per class.  log1p of the exact difference instead of log g - log p: the same quantity, log(g / p), without
 *                the cancellation between two logarithms that for g ~ p leaves an absolute error of an ulp of log g in a
 *                value many orders smaller.
 *   the bin      #{ j >= 1 : edges[j-1] <= |d| }, found by binary search: 0.5 mm bins, the last one open-ended; 5 / 10 /
 *                20 mm are bin edges.  No division takes part in a bin decision.
 * stats: [N][K] records, written whole by every call; byte offsets:
 *      0  int64   n            |S(n,k)| (the sum of the bins)
 *      8  int64   a1
 *     16  int64   a2
 *     24  int64   a3
 *     32  int64   bad
 *     40  double  sum_abs_rel  sum |d| / g
 *     48  double  sum_sq_rel   sum d * d / g
 *     56  double  sum_sq       sum d * d
 *     64  double  sum_log2     sum l * l
 *     72  8 bytes of zero
 *     80  uint32  hist[512]
 * err (only without a scale -- a scaled error is per class; err together with scale is refused): (float)|g - p0| in metres
 * where the pixel passes the gate and pred is finite, whatever its class; NaN elsewhere.
 * The integer fields are exact; the four sums are bit-reproducible (the scheme of pd_normals_stats: fixed lane, wave and
 * workgroup order, partials through `workspace`).  Three launches per 2^20 images; capturable.
 * workspace: >= pd_depth_stats_workspace(N, H, W, K) bytes (never 0, a multiple of 16, monotone), 16-byte aligned.
 *
 * Neither call synchronises, allocates or reads the environment.  N == 0 returns PD_OK after the checks.  Every refusal is
 * PD_EINVAL with a message, decided before the device is touched: null pointers, bad shape, K outside 1 .. 16, a ranged class
 * with mask == NULL, !(min_depth > 0) or !(max_depth > min_depth), stats / count / workspace not 16-byte aligned, a
 * too-small workspace (naming the needed size), a frame beyond 2^30 pixels ("too large"), err together with scale. */
#define PD_DSTAT_BINS         512      /* 0.5 mm bins over |gt - pred|, the last one open-ended */
#define PD_DSTAT_MAX_CLASSES  16
#define PD_DSTAT_COUNTERS     4        /* a1, a2, a3, bad */
#define PD_DSTAT_SUMS         4
#define PD_DSTAT_RECORD_BYTES 2128     /* 80 + 4 * 512 */
size_t pd_depth_medians_workspace(int N, int K);
int pd_depth_medians(const void* gt, const void* pred, const void* mask, const int* classes, int K, void* count, void* med,
                     void* workspace, size_t ws_bytes, int N, int H, int W, float min_depth, float max_depth, void* stream);
size_t pd_depth_stats_workspace(int N, int H, int W, int K);
int pd_depth_stats(const void* gt, const void* pred, const void* mask, const int* classes, int K, const void* scale,
                   const void* edges, void* err, void* stats, void* workspace, size_t ws_bytes, int N, int H, int W,
                   float min_depth, float max_depth, void* stream);

/* Multi-view depth consistency per pixel class (csrc/consistency.hip): do the depth maps of neighbouring frames describe
 * the same surface once the camera motion between them is taken into account?  The forward-backward reprojection check of
 * MVSNet's geometric filter (Yao et al., ECCV 2018, sec. 4.2), scored per class of the instance mask in one read of the batch.
 * It needs no ground-truth depth.  tests/consistency_ref.py states the definition in NumPy, in the order written here.
 *
 * depth0       fp32 [N,H,W]     depth of the current view
 * depths       fp32 [N,F,H,W]   depth of each source view, 1 <= F <= PD_REPROJ_MAX_FRAMES
 * T            fp32 [N,F,4,4]   rigid motion from view 0 to view f (a point X of camera 0 is R X + t in camera f)
 * K, inv_K     fp32 [N,4,4]
 * frame_valid  fp32 [N,F] or NULL (every view present)
 * visible      uint8 [N,F,H,W] or NULL: a 0 takes the (pixel, view) pair out of the comparison
 * mask         int32 [N,H,W] or NULL; classes HOST int[n_classes][2] as in pd_normals_stats (lo > hi = every pixel; a ranged
 *              class needs a mask); 1 <= n_classes <= PD_DSTAT_MAX_CLASSES
 * tau_px, tau_rel   HOST double[3], loose -> tight: positive, finite, non-increasing.  The defaults of the Python layer are
 *              (4, 0.04), (2, 0.02), (1, 0.01); the tightest pair is MVSNet's filter.
 * fuse_level   2, 3 or 4: the level a view must reach to enter n_cons and fused
 *
 * Every step is fp64 unless fp32 is stated; the file is built with -ffp-contract=off; the camera pieces are those of
 * csrc/view_geom.hpp (cam_P, cam_iK, ray, project_ray, axis_of, Bilinear), whose comments give their order of operations.
 * With in(d) = (d >= min_depth && d <= max_depth) in fp32 (NaN fails), pixel (x, y) of item n and view f get exactly ONE
 * outcome, tested in this order:
 *   1 invalid    !in(d0), d0 = depth0[n][y][x]
 *   2 absent     frame_valid[n][f] == 0
 *   3 filtered   visible given and visible[n][f][y][x] == 0
 *   4 outside    (forward leg)  P = cam_P(K_n, T_nf), r = ray(inv_K_n, x, y), project_ray(P, r, (double)d0) -> (u, v, hz);
 *                uf = (float)u, vf = (float)v, rounded ONCE.  Outside unless hz > 1e-3 && 0 <= uf <= W-1 && 0 <= vf <= H-1
 *                (the last four in fp32; NaN fails).
 *   5 hole       ax = axis_of(uf, W), ay = axis_of(vf, H); the taps v00 = D[ay.i0][ax.i0], v10 = D[ay.i0][ax.i1],
 *                v01 = D[ay.i1][ax.i0], v11 = D[ay.i1][ax.i1] of D = depths[n][f].  A hole unless in() holds for all four;
 *                otherwise d1 = Bilinear(ax.w1, ay.w1).blend(v00, v10, v01, v11) in fp32.
 *   6 outside    (return leg)  R = T[:3,:3], t = T[:3,3] widened to fp64; Ti = [R^T | -(R^T t)] with
 *                (R^T t)[i] = (R[0][i] t0 + R[1][i] t1) + R[2][i] t2 and the last row (0, 0, 0, 1);
 *                P'[i][j] = ((K[i][0] Ti[0][j] + K[i][1] Ti[1][j]) + K[i][2] Ti[2][j]) + K[i][3] Ti[3][j] (cam_P's order on
 *                doubles); r' = ray(inv_K_n, (double)uf, (double)vf): the ray of the FRACTIONAL pixel;
 *                project_ray(P', r', (double)d1) -> (u2, v2, hz2).  Outside unless hz2 > 1e-3.
 *   7 compared   du = u2 - x, dv = v2 - y; e2 = du du + dv dv; e_px = sqrt(e2); e_rel = |hz2 - d0| / d0.  hz2 carries
 *                project_ray's + 1e-7, as every depth that function returns.  Level j (0 loose, 1 mid, 2 tight) is met when
 *                e2 < tau_px[j] tau_px[j] && e_rel < tau_rel[j]; no square root takes part in a decision.
 *
 * stats: [N][n_classes] records pooled over the F views, written whole by every call; byte offsets:
 *      0  int64   n           the compared pairs (the sum of the bins)
 *      8  int64   loose       compared pairs that meet level 0  (the levels are nested: loose >= mid >= tight)
 *     16  int64   mid         ... level 1
 *     24  int64   tight       ... level 2
 *     32  int64   invalid
 *     40  int64   absent
 *     48  int64   filtered
 *     56  int64   outside     either leg
 *     64  int64   hole
 *     72  double  sum e_px
 *     80  double  sum e_rel
 *     88  double  sum e2      (e_px squared, before the root)
 *     96  double  sum e_rel e_rel
 *    104  8 bytes of zero
 *    112  uint32  hist[256]   bin = min((int)floor(e_rel * 1024), 255): width 1/1024, the last bin open
 * n + invalid + absent + filtered + outside + hole = (pixels of the class) * F.  The integer fields are exact.  The sums are
 * bit-reproducible: a lane adds the terms of one pixel over f ascending (from 0), adds that to the pixel's classes, and
 * takes its pixels in increasing order; lanes, waves and workgroups follow in the fixed order of csrc/class_records.hpp.
 *
 * Per-pixel outputs, each NULL or:
 *   level   uint8 [N,F,H,W]   0 = not compared; 1 = compared, no level met; 2, 3, 4 = the tightest level met (loose, mid, tight)
 *   n_cons  uint8 [N,H,W]     the number of views with level >= fuse_level
 *   fused   fp32  [N,H,W]     (float)((d0 + sum hz2_f) / (1 + n_cons)) over those views, summed in fp64 with f ascending
 *                             starting from d0, rounded once; on an invalid pixel n_cons = 0 and fused = 0
 * A work item is a pixel, its lane loops over the views: the outputs are written with plain stores by the lane that owns
 * the pixel.  A workgroup belongs to one image and holds P, P' and inv_K of its F views in LDS.  Three launches per 2^20
 * images; the call neither synchronises, allocates nor reads the environment and can be captured into a graph.
 * workspace: >= pd_depth_consistency_workspace(N, H, W, n_classes) bytes (never 0, a multiple of 16, monotone), 16-byte
 * aligned.  N == 0 returns PD_OK after the checks.  Every refusal is PD_EINVAL with a message, decided before the device is
 * touched: those of pd_depth_stats (null pointers, bad shape, n_classes outside 1 .. 16, a ranged class with mask == NULL,
 * !(min_depth > 0), !(max_depth > min_depth), stats / workspace not 16-byte aligned, a too-small workspace, a frame beyond
 * 2^30 pixels), F outside 1 .. PD_REPROJ_MAX_FRAMES, thresholds that are not positive and finite or not nested, fuse_level
 * outside 2 .. 4. */
#define PD_CONS_BINS         256      /* bins of e_rel, 1/1024 wide, the last one open-ended */
#define PD_CONS_COUNTERS     8        /* loose, mid, tight, invalid, absent, filtered, outside, hole */
#define PD_CONS_SUMS         4
#define PD_CONS_RECORD_BYTES 1136     /* 112 + 4 * 256 */
size_t pd_depth_consistency_workspace(int N, int H, int W, int K);
int pd_depth_consistency(const void* depth0, const void* depths, const void* T, const void* K, const void* inv_K,
                         const void* frame_valid, const void* visible, const void* mask, const int* classes, int n_classes,
                         float min_depth, float max_depth, const double* tau_px, const double* tau_rel, int fuse_level,
                         void* level, void* n_cons, void* fused, void* stats, void* workspace, size_t ws_bytes, int N, int F,
                         int H, int W, void* stream);

/* Polarimetric normals evaluation per pixel class (csrc/polar_normals_stats.hip): does a predicted surface agree with the
 * polarisation that was measured?  K1 turns every pixel's DoLP / AoLP into three physical normal candidates (N_diff, N_spec1,
 * N_spec2: manydepth/normals_vec.py:53-60); this call scores predicted normals against them, per class of the instance mask,
 * in one evaluator launch.  It needs one frame, no ground truth and no pose, so it reports on glass and metal, where the depth
 * sensors have holes; and a wrong polarizer layout, angle set or AoLP handedness turns its azimuth residual from a few
 * degrees into tens.  The prediction in turn resolves the pi ambiguity and the diffuse / specular ambiguity of the
 * polarisation normal: the chosen candidate per pixel is a disambiguated normal map.  tests/polar_normals_ref.py states the
 * definition in NumPy.
 * By default the residual uses the orthographic convention of calc_normals (the camera looks along -z at every pixel), whose
 * error grows towards the frame's edge; pd_polar_normals_stats_ray with ray_frame = 1 scores in the frame of each pixel's
 * viewing ray instead (THE RAY FRAME, below).  (The training loss on the same decisions is pd_polar_loss_fwd / _bwd, below.)
 *
 * pred         fp32 device, pixel-major, pixel stride ld >= 3 floats, as for pd_normals_stats (ld = 3: a channels-last
 *              [N,3,H,W] tensor read in place; ld = 4: what pd_gt_normals writes, read with 16-byte loads when aligned)
 * pol_normals  fp32 planar [N,9,H,ldp], what pd_polar_fwd / pd_polar_general_fwd / pd_polar_normals_from_xolp write:
 *              channels 0-2 N_diff, 3-5 N_spec1, 6-8 N_spec2
 * xolp         fp32 [N,2,H,ldp]; only channel 0 (DoLP, rho) is read
 * ldp          row pitch of both, ldp >= W; the padding columns are never read
 * mask         int32 [N,H,W] or NULL; classes HOST int[K][2] exactly as in pd_normals_stats (lo > hi = every pixel; a ranged
 *              class needs a mask; a pixel may be in several classes); 1 <= K <= PD_PNSTAT_MAX_CLASSES
 * valid        uint8 [N,H,W] or NULL; a 0 takes the pixel out altogether: it is in no counter and its maps read "not counted"
 * cos_edges    the same DEVICE double[719] table pd_normals_stats takes; the azimuth set uses its first 359 entries
 * rho_min, rho_max   the DoLP range in which a pixel is scored; tilt2_min = sin^2 of the smallest tilt of the prediction at
 *              which its azimuth is defined; aolp_sign = +1 or -1 multiplies the y component of every candidate
 *
 * Per pixel, every fp32 value converted to fp64 first (all products are then exact), no contraction, in this order.
 * GATES, in this order; a pixel that fails one adds 1 to that counter in each of its classes, in BOTH record sets, and to
 * nothing else:
 *   1 dolp_out   rho is not finite, or rho < rho_min, or rho > rho_max
 *   2 bad        a2 = (px px + py py) + pz pz is not finite or not > 0; or any of the nine candidate components is not finite;
 *                or no candidate has b2 > 0 (b2 below)
 * ORIENTATION: if pz < 0, p is negated (exact).  For every candidate cy' = aolp_sign * cy (exact).
 * NORMAL SET (PD_PNSTAT_NORMAL_BINS = 720 bins of 0.25 degrees over [0, 180]).  Six candidates in the fixed order (diff,+),
 * (diff,-), (spec1,+), (spec1,-), (spec2,+), (spec2,-); the "-" candidate is (-cx, -cy', cz), the pi flip of the azimuth.
 * With m = (px cx) + (py cy'), q = pz cz, b2 = (cx cx + cy' cy') + cz cz:
 *     c+ = (m + q) / (sqrt(a2) sqrt(b2)),   c- = (-m + q) / (sqrt(a2) sqrt(b2)).
 * The first strict maximum in that order wins; candidates with b2 == 0 or a non-finite c are skipped (after the gates no c
 * of fp32 inputs is non-finite; were all skipped, the pixel would count as `bad` in this set).  c is clamped to [-1, 1], its
 * bin is #{ j in 1..719 : c <= cos_edges[j-1] }, deg = acos(c) * 57.29577951308232.  `spec`: the winner is a specular
 * candidate; `flipped`: it is a "-" candidate.
 * AZIMUTH SET (PD_PNSTAT_AZIMUTH_BINS = 360 bins of 0.25 degrees over [0, 90]).  t2 = px px + py py.  Branch d uses the xy of
 * N_diff, branch s the xy of N_spec1 (N_spec2 shares its azimuth); u2 = cx cx + cy' cy'; a branch is usable when u2 > 0.  The
 * pixel adds to `frontal`, and to nothing else of this set, when t2 <= tilt2_min * a2 or no branch is usable.  Otherwise
 *     c_b = |(px cx) + (py cy')| / (sqrt(t2) sqrt(u2)) clamped to [0, 1]  (-1 for a branch that is not usable),
 * c = max(c_d, c_s), `spec` when c_s > c_d strictly, bin = #{ j in 1..359 : c <= cos_edges[j-1] } (exactly 90 degrees lands
 * in bin 359), deg = acos(c) * 57.29577951308232.
 * No trigonometric function takes part in any decision: bins and choices are made on cosines in fp64.
 * SUMS, in both sets, per class of a pixel that counts: deg, deg * deg, rho * deg, rho -- the last two give the
 * DoLP-weighted mean.  They are bit-reproducible from run to run (the fixed lane, wave and workgroup order of
 * csrc/class_records.hpp, partial sums through `workspace`); the integer fields are exact.
 *
 * Records, [N][K] each, written whole by every call; either pointer may be NULL, not both.  Byte offsets:
 *   stats_normal                               stats_azimuth
 *      0  int64   n  (the sum of the bins)        0  int64   n
 *      8  int64   bad                             8  int64   bad
 *     16  int64   dolp_out                       16  int64   dolp_out
 *     24  int64   spec                           24  int64   frontal
 *     32  int64   flipped                        32  int64   spec
 *     40  double  sum deg                        40  double  sum deg
 *     48  double  sum deg deg                    48  double  sum deg deg
 *     56  double  sum rho deg                    56  double  sum rho deg
 *     64  double  sum rho                        64  double  sum rho
 *     72  8 bytes of zero                        72  8 bytes of zero
 *     80  uint32  hist[720]                      80  uint32  hist[360]
 * Per class: n + bad + dolp_out = the pixels of the class with valid != 0 (normal set), n + bad + dolp_out + frontal =
 * the same (azimuth set).
 * Per-pixel maps, each NULL or:
 *   az_deg      fp32  [N,H,W]    the azimuth residual; NaN where the pixel does not count in the azimuth set, whatever its class
 *   n_deg       fp32  [N,H,W]    the angle to the winner; NaN where the pixel does not count in the normal set
 *   choice      uint8 [N,H,W]    0 = not counted in the normal set, else 1 + the winner's index in the order above
 *   pol_normal  fp32  [N,H,W,4]  the winning candidate (+-cx, +-cy', cz, 0), negated when p was negated so that it lies on
 *                                p's side; zeros where not counted
 * One evaluator launch between the zero and finalize launches of csrc/class_records.hpp (one of each per record set) per 2^20
 * images: blockIdx.y picks the record set a workgroup fills.  No allocation, copy or synchronisation: the call can be
 * captured into a graph.  workspace: >= pd_polar_normals_stats_workspace(N, H, W, K) bytes (monotone in each argument,
 * never 0, a multiple of 16).  N == 0 returns PD_OK after the checks.  Every refusal is PD_EINVAL with a message, decided
 * before the device is touched: a null pred / pol_normals / xolp / classes / cos_edges / workspace, both record sets NULL,
 * ws_bytes too small, K outside 1 .. 16, a ranged class with mask == NULL, ld < 3, ldp < W, aolp_sign not +-1, a non-finite
 * or inverted rho_min / rho_max, tilt2_min outside [0, 1), pol_normals / records / pol_normal / workspace not 16-byte
 * aligned, a frame beyond 2^30 pixels ("too large"), bad shape.
 *
 * THE RAY FRAME (pd_polar_normals_stats_ray, pd_polar_loss_fwd_ray / _bwd_ray with ray_frame = 1; csrc/ray_frame.hpp;
 * tests/polar_ray_ref.py states it in NumPy).  K1's candidates are physical quantities about the viewing ray of their pixel:
 * the zenith from DoLP is the angle between the normal and that ray, the azimuth from AoLP is measured around it.  The
 * prediction is formed in camera coordinates; the two agree only at the principal point, and at fx = 0.58 W the ray at the
 * frame's edge is tilted by about 40 degrees.  One rotation per pixel takes the prediction into the frame of its ray; every
 * rule after that is the one above applied to the rotated vector.  R(x, y) is the MINIMAL rotation that takes the unit ray
 * u = r / |r|, r = ((x - cx) / fx, (y - cy) / fy, 1), onto (0, 0, 1); (x, y) is the integer pixel position, as in the Sobel
 * chain of pd_gt_normals.  It is evaluated in fp64 from the fp32 p and the fp32 intrinsics K [N,4,4] of the pixel's batch item
 * (fx = K[0][0], fy = K[1][1], cx = K[0][2], cy = K[1][2]), in exactly this order, without contraction, + - x / sqrt only:
 *     xt = (double(x) - cx) / fx          yt = (double(y) - cy) / fy
 *     L  = sqrt((xt*xt + yt*yt) + 1.0)    ux = xt / L    uy = yt / L    uz = 1.0 / L
 *     d  = (px*ux + py*uy) + pz*uz        s  = (d + pz) / (1.0 + uz)
 *     p' = (px - s*ux,  py - s*uy,  d)
 * and its transpose, used for the pol_normal map and for the loss gradient:
 *     d = (gx*ux + gy*uy) + gz*uz     s = (d + gz) / (1.0 + uz)     t = 2.0*gz
 *     R^T g = ((gx - s*ux) + t*ux,  (gy - s*uy) + t*uy,  (gz - s*(uz + 1.0)) + t*uz)
 * On the axis (xt = yt = 0) R is the identity bit for bit (s = (pz + pz) / 2 = pz); 1 + uz > 1, so no denominator is at risk;
 * a zero or NaN fx / fy makes p' non-finite and the pixel `bad`, and no address depends on it.  p' replaces the fp64 p
 * everywhere from the `bad` gate on: a2, t2, m, q are formed from p'.  The orientation p'z >= 0 becomes the physical
 * visibility condition p.u >= 0, `frontal` becomes "too frontal to the ray".  choice, n_deg and az_deg are those of the ray
 * frame; pol_normal is R^T of the winning candidate on the prediction's side, formed in fp64 and rounded once: a camera-frame
 * normal map.
 * Why the minimal rotation: it gives the exact zenith (p'z = p.u) and keeps every angle between the prediction and the
 * candidates.  For the azimuth it is the middle of three models, with alpha the ray's tilt: an orthogonal projection of the
 * field onto the sensor plane shortens the component in the meridional plane by cos alpha; the published perspective
 * phase-angle model (the plane of incidence cut with the image plane) shortens the component across it by cos alpha; the minimal
 * rotation shortens neither, which is also how a rotationally symmetric lens carries the s and p components (s is kept, p
 * turns with the ray).  It differs from the phase-angle model by a mean of about 2.5 degrees and up to 8-10 degrees in the
 * extreme corner, against an orthographic error of up to 47 degrees.  THE REMAINING LIMIT: this is a convention, not a
 * measurement; a second azimuth model is not built.
 * pd_polar_normals_stats_ray takes K (fp32 [N,4,4], device) and ray_frame (0 or 1) after ld and is otherwise
 * pd_polar_normals_stats: same records, maps, workspace and launches, still capturable.  With ray_frame = 0 it writes the
 * bytes of pd_polar_normals_stats and ignores K, which may be NULL.  Two more refusals (PD_EINVAL, before the device is
 * touched): ray_frame not 0 or 1; ray_frame = 1 with K == NULL. */
#define PD_PNSTAT_NORMAL_BINS          720      /* 0.25 degree bins over [0, 180] */
#define PD_PNSTAT_AZIMUTH_BINS         360      /* 0.25 degree bins over [0, 90] */
#define PD_PNSTAT_MAX_CLASSES          16
#define PD_PNSTAT_COUNTERS             4        /* bad, dolp_out, then spec, flipped (normal) or frontal, spec (azimuth) */
#define PD_PNSTAT_SUMS                 4
#define PD_PNSTAT_NORMAL_RECORD_BYTES  2960     /* 80 + 4 * 720 */
#define PD_PNSTAT_AZIMUTH_RECORD_BYTES 1520     /* 80 + 4 * 360 */
size_t pd_polar_normals_stats_workspace(int N, int H, int W, int K);
int pd_polar_normals_stats(const void* pred, long ld, const void* pol_normals, const void* xolp, long ldp, const void* mask,
                           const int* classes, int K, const void* valid, const void* cos_edges, float rho_min, float rho_max,
                           double tilt2_min, int aolp_sign, void* stats_normal, void* stats_azimuth, void* az_deg,
                           void* n_deg, void* choice, void* pol_normal, void* workspace, size_t ws_bytes, int N, int H, int W,
                           void* stream);
int pd_polar_normals_stats_ray(const void* pred, long ld, const void* K, int ray_frame, const void* pol_normals,
                               const void* xolp, long ldp, const void* mask, const int* classes, int n_classes,
                               const void* valid, const void* cos_edges, float rho_min, float rho_max, double tilt2_min,
                               int aolp_sign, void* stats_normal, void* stats_azimuth, void* az_deg, void* n_deg, void* choice,
                               void* pol_normal, void* workspace, size_t ws_bytes, int N, int H, int W, void* stream);

/* The polarimetric normals loss (csrc/polar_loss.hip): the two figures of pd_polar_normals_stats as a training term on a depth
 * map, so that Evaluation.test_polar_normals reports what training minimises.  It needs one frame, no ground truth and no
 * pose.  Like the evaluator it keeps the orthographic convention of calc_normals by default; pd_polar_loss_fwd_ray / _bwd_ray
 * with ray_frame = 1 form both terms in the frame of each pixel's viewing ray (THE RAY FRAME, above, and the last paragraph).
 * tests/polar_loss_ref.py states the definition in NumPy.
 *
 * depth        fp32 [N,1,H,W]
 * K            fp32 [N,4,4] intrinsics
 * pol_normals, xolp, ldp, valid, rho_min, rho_max, tilt2_min, aolp_sign    exactly as in pd_polar_normals_stats: planar
 *              [N,9,H,ldp] and [N,2,H,ldp] read in place, the padding columns never read
 * dolp_weighted   1: the weight of a pixel is w = rho; 0: w = 1
 *
 * Per pixel p = the fp32 normal of the depth map, formed exactly as pd_gt_normals forms it without a depth range (min_depth =
 * -FLT_MAX, max_depth = FLT_MAX): Sobel/8 of the unprojected points with replicate padding, cross product, v / max(|v|, 1e-12),
 * fp32, no contraction -- bit for bit what the evaluator scores when it is handed the depth map.  From p on every fp32 value is
 * converted to fp64 first and every decision is the evaluator's, in its operation order:
 * GATES, in this order: valid == 0 (the pixel counts nowhere); dolp_out; bad.  ORIENTATION: p is negated when pz < 0;
 * cy' = aolp_sign * cy.
 * NORMAL TERM: the six cosines c+-, the first strict maximum c* wins, clamped to [-1, 1]:   l_n = 1 - c*   (1 - cos of n_deg).
 * AZIMUTH TERM: `frontal` when t2 <= tilt2_min * a2 or no branch is usable; otherwise branch d or s, s only when c_s > c_d
 * strictly (c_d, c_s as the evaluator forms them); with m = (px cx) + (py cy') and u2 of the chosen branch
 *     l_a = 1 - (m m) / (t2 u2)   clamped to [0, 1]   (sin^2 of az_deg; no square root, smooth at m = 0).
 * Only + - x / sqrt in fp64 take part.  VALUES: L_n = sum w l_n / sum w over the pixels with a winner, L_a = sum w l_a / sum w
 * over the pixels counted in the azimuth set, each rounded once to fp32; a term whose sum w is 0 has value 0 and a zero
 * gradient (an H = 1 or W = 1 frame: every normal is the zero vector, hence `bad`).  The sums are fp64 in the fixed lane /
 * wave / workgroup / finalize order of csrc/frame_reduce.hpp, no atomics: bit-reproducible.
 *
 * Outputs of pd_polar_loss_fwd:
 *   state   uint8 [N,H,W], the decisions of the pixel:
 *             bits 0-2  (PD_PLOSS_STATE_WINNER)   0 = no winner, else 1 + the winner's index: the evaluator's `choice`
 *             bit  3    (PD_PLOSS_STATE_NEGATED)  p was negated
 *             bits 4-5  (PD_PLOSS_STATE_BRANCH)   the azimuth branch: 0 = none (a gate, or frontal), 1 = d, 2 = s
 *             bits 6-7  (>> PD_PLOSS_STATE_GATE_SHIFT)  the gate that dropped the pixel: 0 = none, 1 = valid == 0,
 *                       2 = dolp_out, 3 = bad
 *   sums    PD_PLOSS_RECORD_BYTES = 96 bytes, 8-byte aligned:
 *              0  double  sum w l_n          32  int64  pixels with a winner        64  int64  frontal
 *              8  double  sum w  (normal)    40  int64  pixels in the azimuth set   72  int64  specular winners
 *             16  double  sum w l_a          48  int64  dolp_out                    80  int64  flipped winners
 *             24  double  sum w  (azimuth)   56  int64  bad                         88  8 bytes of zero
 *   values  fp32 [2] = (L_n, L_a)
 *   maps    NULL or fp32 [N,H,W,2] = (l_n, l_a) rounded to fp32, NaN where the pixel is not counted in that term
 * workspace: >= pd_polar_loss_rows(N, H, W) * 11 * 8 bytes, 16-byte aligned; pd_polar_loss_rows is monotone and never 0.
 *
 * pd_polar_loss_bwd: gdepth [N,1,H,W] = d (g[0] L_n + g[1] L_a) / d depth, written for every pixel, zeros included.  It reads
 * `state` instead of deciding again (the winner and the branch are data, as the minimum over frames in pd_reproj_combine),
 * gvalues = the DEVICE fp32 [2] upstream gradient, and `sums` of the forward call.  dL/dp is formed in fp64,
 *     normal term    -(g[0] w / sum w) (c^ - c* p^) / |p|          c^, p^ the unit candidate and the unit p
 *     azimuth term   -(g[1] w / sum w) 2 m / (t2 u2) ((cx, cy') - (m / t2) (px, py)),   z component 0
 * a clamped c* or l_a contributing nothing; the sign is restored for a negated p and the sum is rounded once to fp32.  From
 * there the path is the fp32 one of pd_sup_loss_bwd: through v / max(|v|, 1e-12) (its |v| <= 1e-12 branch included), dA = B x
 * wv, dB = wv x A, and the transposed replicate-padded Sobel gather.  One launch: per 8 x 64 tile the (dA, dB) of the 10 x 66
 * halo go to LDS and the gather runs from there; PD_PLOSS_BWD_TILES_PER_TRIP tiles per grid-stride trip.
 *
 * Neither call allocates, copies or synchronises: both can be captured into a graph.  N == 0 returns PD_OK after the checks
 * and touches nothing (the values of an empty batch are 0).  Every refusal is PD_EINVAL with a message, decided before the
 * device is touched: bad shape, a null depth / K / pol_normals / xolp / state / sums / values / workspace (/ gvalues /
 * gdepth), ldp < W, aolp_sign not +-1, dolp_weighted not 0 or 1, a non-finite or inverted rho_min / rho_max, tilt2_min outside
 * [0, 1), pol_normals or workspace not 16-byte aligned, sums or maps not 8-byte aligned, ws_bytes too small, a frame beyond
 * 2^30 pixels ("too large").
 *
 * pd_polar_loss_fwd_ray / pd_polar_loss_bwd_ray take ray_frame (0 or 1) after dolp_weighted and are otherwise the two calls
 * above: same outputs, workspace and launches, still capturable; with ray_frame = 0 they write the bytes of the old entries.
 * One more refusal: ray_frame not 0 or 1.  With ray_frame = 1 (THE RAY FRAME, above): forward, p' = R(x, y) p is formed right
 * after the conversion of p to fp64 and stands for p from the `bad` gate on; the NEGATED bit means p'z < 0, i.e. the surface is
 * seen from behind (p.u < 0), which a depth map's own normal is not under a sane camera.  Backward: the halo evaluation
 * rebuilds p' from p, dL/dp' is formed exactly as above with p' for p, then dL/dp = R^T dL/dp' in fp64, then the sign is
 * restored for a negated vector, then the sum is rounded once to fp32 and the fp32 chain above follows.  There is no gradient
 * with respect to K. */
#define PD_PLOSS_SUMS                4
#define PD_PLOSS_COUNTERS            7        /* n_normal, n_azimuth, dolp_out, bad, frontal, spec, flipped */
#define PD_PLOSS_RECORD_BYTES        96
#define PD_PLOSS_STATE_WINNER        7
#define PD_PLOSS_STATE_NEGATED       8
#define PD_PLOSS_STATE_BRANCH        48
#define PD_PLOSS_STATE_BRANCH_SHIFT  4
#define PD_PLOSS_STATE_GATE_SHIFT    6
#define PD_PLOSS_BWD_TILES_PER_TRIP  4096
int pd_polar_loss_rows(int N, int H, int W);
int pd_polar_loss_fwd(const void* depth, const void* K, const void* pol_normals, const void* xolp, long ldp, const void* valid,
                      float rho_min, float rho_max, double tilt2_min, int aolp_sign, int dolp_weighted, void* state, void* sums,
                      void* values, void* maps, void* workspace, size_t ws_bytes, int N, int H, int W, void* stream);
int pd_polar_loss_bwd(const void* depth, const void* K, const void* pol_normals, const void* xolp, long ldp, const void* state,
                      const void* gvalues, const void* sums, int aolp_sign, int dolp_weighted, void* gdepth, int N, int H, int W,
                      void* stream);
int pd_polar_loss_fwd_ray(const void* depth, const void* K, const void* pol_normals, const void* xolp, long ldp,
                          const void* valid, float rho_min, float rho_max, double tilt2_min, int aolp_sign, int dolp_weighted,
                          int ray_frame, void* state, void* sums, void* values, void* maps, void* workspace, size_t ws_bytes,
                          int N, int H, int W, void* stream);
int pd_polar_loss_bwd_ray(const void* depth, const void* K, const void* pol_normals, const void* xolp, long ldp,
                          const void* state, const void* gvalues, const void* sums, int aolp_sign, int dolp_weighted,
                          int ray_frame, void* gdepth, int N, int H, int W, void* stream);

/* Row softmax of the attention variant (BASELINE config 5; SURVEY A17 -- defined by this build, the reference
 * branch is absent): in place x[r][:] = softmax(scale * x[r][:]) and its backward
 * dp[r][:] <- scale * p * (dp - sum(dp * p)).  The score GEMMs (Q K^T, P V and their gradients) are pd_conv2d /
 * pd_conv2d_wgrad calls with 1x1 filters. */
int pd_softmax_rows_fwd(void* x, long R, long L, float scale, void* stream);
int pd_softmax_rows_bwd(const void* p, void* dp, long R, long L, float scale, void* stream);

/* ---- Pillow-compatible 8-bit LANCZOS resampling of uint8 planes (Image.resize(..., Image.ANTIALIAS),
 * indoor_dataset.py:335-349): one pass of ImagingResample's 8bpc branch.
 * src [P][Hs][Ws] uint8; vertical == 0: dst [P][Hs][out_size] (horizontal pass), else dst [P][out_size][Ws].
 * coeffs int32 [out_size][ksize] (22-bit fixed point), bounds int32 [out_size][2] = (first input index, count):
 * Pillow's precompute_coeffs + normalize_coeffs_8bpc, built by polardepth/resize.py on the host. */
int pd_resize_u8_pass(const void* src, void* dst, const void* coeffs, const void* bounds, int ksize, int P, int Hs,
                      int Ws, int out_size, int vertical, void* stream);

/* ---- the same pass for 16-bit and float planes, the other two element types K1's general kernel takes: Pillow's
 * ImagingResampleHorizontal_16bpc / ImagingResampleVertical_16bpc (mode I;16) and the IMAGING_TYPE_FLOAT32 case of
 * ImagingResampleHorizontal_32bpc / ImagingResampleVertical_32bpc (mode F), src/libImaging/Resample.c.
 * dtype   PD_POLAR_U16 or PD_POLAR_F32 (PD_POLAR_U8 is an error: pd_resize_u8_pass); src, dst: planes of that type, shapes
 *         as for pd_resize_u8_pass
 * coeffs  DOUBLE [out_size][ksize] = precompute_coeffs' w[x] / ww without the 8bpc normalisation; bounds as above
 *         (polardepth/resize.py lanczos_coeffs_f64).  A bounds row that points outside the input is cut to fit.
 * Per output: double ss = 0; ss += (double)in[first + x] * k[x] in tap order, multiply and add rounded separately.
 *   F:    out = (float)ss.  NaN and infinity follow IEEE: a non-finite input reaches every output whose window holds it,
 *         also through a zero coefficient.
 *   I;16: v = ss >= 0 ? (int)(ss + 0.5) : (int)(ss - 0.5), then Pillow's BYTEWISE store: low byte = clip8(v % 256) with
 *         C's remainder, high byte = clip8(v >> 8).  Undershoot (v < 0) gives 0.  Overshoot past 65535 does NOT saturate
 *         to 65535: the high byte clips to 255 and the low byte wraps (65836 -> 0xff2c).  Data in 12-bit range never gets
 *         there.  The image between the two passes has the planes' own type and the same rule. */
int pd_resize_wide_pass(const void* src, void* dst, int dtype, const void* coeffs, const void* bounds, int ksize, int P,
                        int Hs, int Ws, int out_size, int vertical, void* stream);

/* ---- demosaic of division-of-focal-plane (DoFP) polarizer frames (csrc/dofp.hip): the interleaved mosaic a polarization
 * sensor emits -- every 2x2 super-pixel carries the four filters -- -> the four planes of ("pol", 0, 0).  Not in the
 * reference, whose data arrive split into pol00 .. pol11 (polarisation/pol_split_and_save.py cuts QUADRANT frames).
 * mosaic  [B][H2][W2] device, contiguous, element type `dtype` (PD_POLAR_U8 / _U16 / _F32); H2, W2 even and >= 2; rows need
 *         no alignment (W2 = 6 uint8 is fine), the two base pointers must be 16-byte aligned
 * layout  four HOST ints, a permutation of 0..3, read during the call: layout[2 r + c] = the plane that the site at row
 *         parity r, column parity c feeds; r_p, c_p below are the site of plane p.  (2,1,3,0) is the Sony IMX250MZR
 *         (90/45/135/0 degrees in reading order) with the planes in the nominal 0/45/90/135 order.
 * PD_DOFP_SUPERPIXEL: planes [B][4][H2/2][W2/2] of the SAME dtype, planes[p][y][x] = mosaic[2y + r_p][2x + c_p]
 * PD_DOFP_BILINEAR:   planes [B][4][H2][W2] fp32; with dy = (y - r_p) & 1, dx = (x - c_p) & 1 and m = the frame:
 *           dy dx
 *           0  0   m[y][x]
 *           0  1   (m[y][x-1] + m[y][x+1]) * 0.5
 *           1  0   (m[y-1][x] + m[y+1][x]) * 0.5
 *           1  1   ((m[y-1][x-1] + m[y-1][x+1]) + (m[y+1][x-1] + m[y+1][x+1])) * 0.25
 *         index -1 reads index 1 and index n reads index n-2 (a mirror about the edge sample: the site parity survives).
 *         fp64 in exactly that order, rounded once to fp32: exact for the integer types, and for fp32 what makes the result
 *         defined (a frame of FLT_MAX returns FLT_MAX, not infinity).  NaN and infinity reach the outputs whose stencil
 *         holds them.
 * B == 0 returns 0.  No allocation, copy or synchronisation: the call can be captured into a graph.  Frames beyond 2^30
 * pixels (or 2^40 in the batch) are refused ("too large": in-frame offsets are 32-bit in the kernels). */
#define PD_DOFP_SUPERPIXEL 0
#define PD_DOFP_BILINEAR 1
int pd_dofp_demosaic(const void* mosaic, int dtype, void* planes, int mode, const int* layout, int B, int H2, int W2,
                     void* stream);

/* ---- demosaic of COLOUR division-of-focal-plane frames (csrc/cdofp.hip): the colour model of that sensor (Sony IMX250MYR
 * class) has a Bayer colour filter over the polarizer array, so every 4x4 super-pixel is a 2x2 Bayer cell of 2x2 polarizer
 * cells, and one raw frame holds the RGB picture and the four polarizer planes.  Not in the reference beyond the `L` weights
 * and the shape of its 12-channel input (indoor_dataset.py:220-250).
 * mosaic  [B][H4][W4] device, contiguous, element type `dtype` (PD_POLAR_U8 / _U16 / _F32); H4, W4 multiples of 4 and >= 4;
 *         rows need no alignment beyond what that gives, every base pointer must be 16-byte aligned
 * layout  four HOST ints, read during the call, as for pd_dofp_demosaic: a permutation of 0..3, layout[2 (y & 1) + (x & 1)]
 *         = the polarizer plane the site feeds
 * bayer   four HOST ints, read during the call: bayer[2 ((y >> 1) & 1) + ((x >> 1) & 1)] = the colour of the site, 0 = R,
 *         1 = G, 2 = B; one of the four Bayer orders (one R, one B, two G on a diagonal); (0,1,1,2) is RGGB
 * gains   three HOST doubles, finite: per-colour multipliers (white balance); NULL = (1,1,1)
 * Definition -- every step fp64, in exactly this order.  The frame m is 16 sub-lattices (ry, rx) in {0..3}^2,
 * L[i][j] = m[4i + ry][4j + rx], ny = H4 / 4, nx = W4 / 4.  For the output pixel (y, x): i0 = floor((y - ry) / 4),
 * ty = (y - ry) mod 4, j0 = floor((x - rx) / 4), tx = (x - rx) mod 4; a, b, c, d = L[i0][j0], L[i0][j0+1], L[i0+1][j0],
 * L[i0+1][j0+1] with every lattice index clamped to [0, n-1];
 *     v = ((4 - ty) * ((4 - tx) * a + tx * b) + ty * ((4 - tx) * c + tx * d)) * 0.0625
 * A zero weight still multiplies: a non-finite sample reaches every output whose lattice cell holds it.  For polarizer plane
 * p and colour k, R and B come from one sub-lattice each and G from two, (v_first + v_second) * 0.5 with first the one in the
 * upper Bayer row; then ch[p][k] = v * gains[k].
 * Outputs (each may be NULL, not all three):
 * planes      [B][4][H4][W4] fp32 = ((19595 R + 38470 G) + 7471 B) * (1 / 65536) of ch[p] (Pillow's `L` weights, which the
 *             loader applies to the pol* files), rounded once to fp32
 * color_u8    [B][3][H4][W4] uint8: c = ((ch[0][k] + ch[1][k]) + (ch[2][k] + ch[3][k])) * 0.25 * color_scale, stored as
 *             clamp(floor(c + 0.5), 0, 255), NaN -> 0.  color_scale must be finite and > 0: 1 for 8-bit frames, 255 / 4095
 *             for 12-bit ones
 * rgb_planes  [B][4][3][H4][W4] fp32: ch rounded once (the per-colour polarizer images)
 * B == 0 returns 0 before anything is looked at.  Every refusal is PD_EINVAL with a message, decided before any launch: null
 * pointers, unknown dtype, bad layout, bad bayer, non-finite gains or scale, sides that are no multiples of 4, misalignment,
 * frames beyond 2^30 pixels (or 2^40 in the batch: "too large", in-frame offsets are 32-bit in the kernel).  No allocation,
 * copy or synchronisation: the call can be captured into a graph. */
int pd_cdofp_demosaic(const void* mosaic, int dtype, const int* layout, const int* bayer, const double* gains,
                      double color_scale, void* planes, void* color_u8, void* rgb_planes, int B, int H4, int W4,
                      void* stream);

/* ---- super-pixel calibration of DoFP frames (csrc/dofp_cal.hip; Powell & Gruev, "Calibration methods for division-of-focal-
 * plane polarimeters", Opt. Express 2013): a dark frame plus one 4x4 matrix per 2x2 polarizer cell that maps the four measured
 * samples to what an ideal cell would have measured.  Not in the reference, which assumes an ideal sensor.  Three calls: the
 * moments of a stack of frames, the matrices from the moments of a flat-field series behind a rotating linear polarizer, and
 * dark + matrix applied to incoming frames before pd_dofp_demosaic / pd_cdofp_demosaic (both take float32).
 * Site of a pixel: s = 2 (y & 1) + (x & 1); cell (i, j) holds rows 2i, 2i+1 and columns 2j, 2j+1.  In a colour frame every
 * such cell lies under one Bayer colour, so one definition serves both sensors; the matrices are in SITE order, independent
 * of any layout.  All arithmetic is fp64 in exactly the stated order (no contraction, division as division), rounded once
 * where a narrower type is stored; tests/dofp_cal_ref.py restates it in NumPy and the results agree bit for bit.
 * Common: H2, W2 even and >= 2; every base pointer 16-byte aligned (rows need no alignment: W2 = 6 uint8 is fine); frames
 * beyond 2^30 pixels (or 2^40 in the stack / batch) are refused ("too large": in-frame offsets are 32-bit in the kernels);
 * every refusal is PD_EINVAL with a message, decided before any launch.  No allocation, copy or synchronisation: all three
 * calls can be captured into a graph.
 *
 * pd_frame_moments
 * frames   [N][H2][W2] device, contiguous, element type `dtype` (PD_POLAR_U8 / _U16 / _F32), N >= 1
 * dark     fp32 [H2][W2] device, or NULL (then e = (double)f)
 * weights  fp64 [N][Q], a DEVICE pointer, Q in 1..4
 * out      fp64 [Q][H2][W2] device
 *   out[q][y][x] = (accumulate ? out[q][y][x] : 0) + sum_n w[n][q] * ((double)f[n][y][x] - (double)dark[y][x]),
 * n ascending, each term formed as e = f - d; t = w * e; acc = acc + t.  A thread owns its pixels and loops over n: there is
 * no reduction across threads, the result is deterministic by construction.  Q = 1, w = 1 / N, no dark: the mean frame.
 *
 * pd_dofp_cal_solve
 * moments  fp64 [3][H2][W2] device: pd_frame_moments of the flat-field series with w[n] = (1, p cos 2a_n, p sin 2a_n) times
 *          the relative intensity of frame n (a_n: the polarizer's angle, p: its degree of polarization)
 * rinv     nine HOST doubles, row-major, finite: the inverse of R1 = sum_n w[n] w[n]^T, divided by the radiometric level
 * a_nom    twelve HOST doubles [4 sites][3], finite: row s = 1/2 (1, cos 2 theta_s, sin 2 theta_s), theta_s the nominal angle
 *          of site s
 * qmin     HOST double, finite
 * gain     fp32 [H2/2][W2/2][4][4] device; quality fp32 [H2/2][W2/2] device or NULL
 * Per cell, with m[s][k] = moments[k][2i + (s >> 1)][2j + (s & 1)]:
 *   A[s][l]  = (m[s][0] rinv[0][l] + m[s][1] rinv[1][l]) + m[s][2] rinv[2][l]              (the cell's analyzer vectors)
 *   N[k][l]  = ((A[0][k] A[0][l] + A[1][k] A[1][l]) + A[2][k] A[2][l]) + A[3][k] A[3][l]   for k <= l, mirrored
 *   C00 = N11 N22 - N12 N12   C01 = N02 N12 - N01 N22   C02 = N01 N12 - N02 N11
 *   C11 = N00 N22 - N02 N02   C12 = N01 N02 - N00 N12   C22 = N00 N11 - N01 N01            (C symmetric)
 *   det = (N00 C00 + N01 C01) + N02 C02;   V[k][l] = C[k][l] / det
 *   P[k][s]  = (V[k][0] A[s][0] + V[k][1] A[s][1]) + V[k][2] A[s][2]                       (the pseudo-inverse of A)
 *   G[t][s]  = (a_nom[t][0] P[0][s] + a_nom[t][1] P[1][s]) + a_nom[t][2] P[2][s], stored as fp32
 *   q        = det / ((N00 * N11) * N22)      (Hadamard's ratio: 1 for the nominal cell, 0 or NaN for a cell that cannot see
 *              three Stokes components, such as one with two dead sites)
 * If !(q >= qmin) the cell's G is the 4x4 identity and its quality 0; otherwise quality is (float)q.  G has rank 3 by design
 * (a_nom . pinv(A)): a cell with ONE dead site still gets a valid G that rebuilds the dead sample from the other three.
 *
 * pd_dofp_calibrate
 * mosaic   [B][H2][W2] device, contiguous, element type `dtype`;  dark fp32 [H2][W2] device or NULL (then e = (double)m)
 * gain     PD_DOFP_CAL_CELL: fp32 [H2/2][W2/2][4][4] as above; PD_DOFP_CAL_PIXEL: fp32 [H2][W2], the classical flat-field
 *          gain (the diagonal case)
 * out      fp32 [B][H2][W2] device
 * With e_s = (double)m - (double)dark at site s of the cell:
 *   CELL:  the sample at site t becomes fp32(((G[t][0] e_0 + G[t][1] e_1) + G[t][2] e_2) + G[t][3] e_3)
 *   PIXEL: fp32((double)g * e)
 * No clamping (a dark-subtracted sample may be negative); NaN and infinity reach exactly the outputs whose sum holds them; a
 * zero matrix entry still multiplies.  B == 0 returns 0 before anything is looked at. */
#define PD_DOFP_CAL_CELL 0
#define PD_DOFP_CAL_PIXEL 1
int pd_frame_moments(const void* frames, int dtype, const void* dark, const double* weights, double* out, int N, int Q,
                     int H2, int W2, int accumulate, void* stream);
int pd_dofp_cal_solve(const double* moments, const double* rinv, const double* a_nom, double qmin, float* gain,
                      float* quality, int H2, int W2, void* stream);
int pd_dofp_calibrate(const void* mosaic, int dtype, const void* dark, const void* gain, int gain_kind, void* out, int B,
                      int H2, int W2, void* stream);

/* ---- torchvision 0.8.2's PIL ColorJitter on uint8 planar RGB, Pillow-exact, fused with the loader's uint8 -> fp32 / 255
 * (indoor_dataset.py:92-106, 192-233, 404-407; csrc/color.hip, arithmetic in csrc/color_math.hpp).
 * src [B][3][H][W] uint8 (what pd_resize_u8_pass leaves for a [B,3,.,.] input), any H, W >= 1.
 * dst_u8 [B][3][H][W] uint8 and dst_f32 [B][3][H][W] fp32 = (float)u / 255.0f: either may be NULL, not both.
 * params: device double [B][8] = (code, value) x 4, applied in that order; code 0 none, 1 brightness, 2 contrast,
 *   3 saturation, 4 hue, anything else 0.  The codes are read on the device (a captured step replays with new rows).
 *   A row holds each operation at most once, as ColorJitter's do: a second contrast in a row behaves as code 0.
 *   NULL = identity for every sample (the plain conversion): one launch, sum_ws is not read.
 * sum_ws: 16 bytes per sample, 8-byte aligned, caller-owned: {uint64 sum of L, uint32 arrival ticket, int32 mean}.
 *   The sum and ticket words must be ZERO on entry and are left zero by the call (a buffer zeroed once serves every
 *   later call on the same stream, like acc_ws of pd_bn_fwd_finalize); the mean word is scratch.  The contrast
 *   degenerate int(sum L / (H W) + 0.5) comes from integer partials and integer atomics: exact, independent of order.
 * At most two launches (reduce, apply), no allocation, no host synchronisation. */
int pd_color_jitter_u8(const void* src, const void* params, void* dst_u8, void* dst_f32, void* sum_ws, int B, int H,
                       int W, void* stream);

/* ---- fused attention (flash-attention recurrence on the fp32 matrix cores).
 * q, k, v, o, do, dq, dk, dv: [N][T][128] fp32 (token-major = NHWC), lse / delta: [N][T] fp32; T % 32 == 0.
 * pd_attn_fwd:  o = softmax(q k^T * scale) v,  lse = log sum exp of the scaled scores (saved for the backward). */
int pd_attn_fwd(const void* q, const void* k, const void* v, void* o, void* lse, int N, int T, int C, float scale,
                void* stream);
/* pd_attn_bwd: dq, dk, dv from do (recomputing the scores block by block); delta [N][T] is scratch (sum_c do*o). */
int pd_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o, const void* lse,
                void* delta, void* dq, void* dk, void* dv, int N, int T, int C, float scale, void* stream);

/* The same attention on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16; BASELINE configs[4] "bf16, MFMA attention
 * path"): identical tensors and semantics (fp32 [N][T][128] in and out), operands rounded to bf16 when staged,
 * softmax statistics / exp2 / accumulators in fp32.  Selected by PD_ATTENTION_BF16=1 / bench.py --attention --bf16.
 * workspace (caller-owned, pd_attn_bf16_workspace bytes, 16-byte aligned): the operands every workgroup re-reads are packed
 * once per call into bf16 images of the kernels' LDS tiles (forward: K rows + V^T; backward: K rows, K^T, V rows, Q rows,
 * Q^T, dO rows, dO^T), so that staging a block is a verbatim 16-byte copy. */
size_t pd_attn_bf16_workspace(int N, int T, int C, int backward);
int pd_attn_bf16_fwd(const void* q, const void* k, const void* v, void* o, void* lse, void* workspace, size_t ws_bytes,
                     int N, int T, int C, float scale, void* stream);
int pd_attn_bf16_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o, const void* lse,
                     void* delta, void* dq, void* dk, void* dv, void* workspace, size_t ws_bytes, int N, int T, int C,
                     float scale, void* stream);
/* The same in parts (1 = delta + operand packing, 2 = dK / dV, 4 = dQ; 7 = pd_attn_bf16_bwd): the two gradient kernels are
 * independent, so a caller may enqueue parts 2 and 4 on two streams behind part 1 -- the workgroups of one kernel then fill
 * the last, partly empty round of the other. */
int pd_attn_bf16_bwd_parts(const void* q, const void* k, const void* v, const void* o, const void* d_o, const void* lse,
                           void* delta, void* dq, void* dk, void* dv, void* workspace, size_t ws_bytes, int N, int T, int C,
                           float scale, int parts, void* stream);

/* ---- disparity heads: sigmoid(Conv3x3(x)) with one output channel
 * (manydepth/networks/depth_decoder.py:52-53,69-71; layers.py:364-380 Conv3x3 = ReflectionPad2d(1) + Conv2d(C,1,3)).
 * Direct memory-bound kernels instead of a 32-wide MFMA tile with one useful column.
 *   x  [N,H,W,C] NHWC fp32, C in {16,32,64,128};  w [3][3][C] (= channels_last storage of the [1,C,3,3] weight);
 *   y / dy [N,H,W] (= [N,1,H,W]);  bias [1] or NULL.
 * pd_disphead_fwd:        y = sigmoid(bias + conv)
 * pd_disphead_bwd_data:   dx [N,H,W,C] = gradient w.r.t. x given dy (gradient w.r.t. y) and y; the fold of the
 *                         reflection padding is built in
 * pd_disphead_bwd_weight: dw [3][3][C] (+)= , dbias [1] (+)= (NULL to skip); workspace >= pd_disphead_workspace(C)
 *                         bytes, 16-byte aligned; deterministic two-stage summation
 * pd_disphead_bwd:        both gradients in one pass over x (dx may be NULL): what the training step calls.
 *                         add [N,H,W,C] or NULL is summed into dx (the gradient x receives from its other consumer,
 *                         depth_decoder.py:64 reads the same x); elu != 0: x is the ELU output of a ConvBlock
 *                         (layers.py:329-342) and dx leaves multiplied by ELU'(.) = (x > 0 ? 1 : x + 1) */
int pd_disphead_fwd(const void* x, const void* w, const void* bias, void* y, int N, int H, int W, int C, void* stream);
int pd_disphead_bwd_data(const void* dy, const void* y, const void* w, void* dx, int N, int H, int W, int C,
                         void* stream);
size_t pd_disphead_workspace(int C);
int pd_disphead_bwd_weight(const void* dy, const void* y, const void* x, void* dw, void* dbias, void* workspace,
                           size_t ws_bytes, int N, int H, int W, int C, int accumulate, void* stream);
int pd_disphead_bwd(const void* dy, const void* y, const void* x, const void* w, const void* add, int elu, void* dx,
                    void* dw, void* dbias, void* workspace, size_t ws_bytes, int N, int H, int W, int C, int accumulate,
                    void* stream);

/* ---- Depth uncertainty (csrc/unc_loss.hip, csrc/unc_stats.hip): the decoder's sigmoid uncertainty heads
 * (depth_decoder.py:46-73, "unc_conv") trained and scored as the scale of a Laplace error model of the predicted depth.
 * tests/unc_loss_ref.py and tests/unc_stats_ref.py state the definitions in NumPy.
 *
 * THE SCALE of a pixel.  u in [0, 1] is the head's output; with (b_lo, b_hi) in metres, 0 < b_lo < b_hi < inf,
 *     log b = fma((double)u, log(b_hi / b_lo), log b_lo)        in fp64, the two logarithms taken on the host;
 *     b = exp(log b)                                             in metres;    log 2b = log b + M_LN2.
 * (b_lo, b_hi) is a convention of the caller (the Python layer's default is 0.5 mm .. 0.5 m), not a measurement.
 *
 * THE LOSS (pd_unc_loss_fwd / _bwd).  depth fp32 [N,H,W] contiguous (what pd_disp_to_depth wrote); gt fp32 [N,H,W] with
 * row pitch ldg >= W elements (image pitch H * ldg); unc fp32 [N,hs,ws] contiguous with hs <= H, ws <= W, sampled at every
 * pixel of the frame by the align_corners=False bilinear rule of pd_disp_to_depth in fp32 (csrc/up_index.hpp), any ratio;
 * valid uint8 [N,H,W] or NULL.
 *     m   = min_depth <= gt <= max_depth (inclusive, NaN fails: the mask of the supervised term) and valid != 0 and the
 *           sampled u finite (a non-finite u takes the pixel out, as it makes a pixel `bad` in the evaluator)
 *     L   = sum m (|gt - depth| / b + log 2b) / sum m,   every term in fp64 from the fp32 inputs, the difference exact;
 *           0 where sum m = 0.  A non-finite depth UNDER the mask makes the value non-finite, as in the supervised term;
 *           outside the mask nothing is read into a sum.
 *   sums    double[PD_ULOSS_SUMS = 4], 8-byte aligned: sum |gt - depth| / b, sum log 2b, sum m, sum b -- added per lane over
 *           its grid-stride items, then lane -> wave -> workgroup -> one finalize workgroup in a fixed order: bit-reproducible.
 *   value   fp32 [1] = (float)((sums[0] + sums[1]) / sums[2]), rounded once
 *   maps    NULL or fp32 [N,H,W,2] = (the pixel's term, b), NaN where m = 0; 8-byte aligned
 *   workspace: >= pd_unc_loss_rows(N, H, W) * 4 * 8 bytes, 16-byte aligned; pd_unc_loss_rows is monotone and never 0.
 * pd_unc_loss_bwd: with c = gvalue[0] / sums[2] (0 where sums[2] = 0) and sums as the forward call left them,
 *   gdepth  fp32 [N,H,W] = c sign(depth - gt) / b under the mask (0 at depth == gt), 0 elsewhere; NULL = the detached mode:
 *           the gradient is neither formed nor written
 *   gup     fp32 [N,H,W] = c (1 - |gt - depth| / b) log(b_hi / b_lo) under the mask, 0 elsewhere: the gradient with respect
 *           to the SAMPLED u; pd_up_gather_bwd(gup, gunc, N, hs, ws, H, W, 0, generic, stream) folds it to [N,hs,ws]
 *           (generic != 0 where H / hs or W / ws is no integer).
 * Two launches forward, one backward; where W and ldg are multiples of 4 and the pointers 16-byte aligned a work item is
 * four pixels with 16-byte accesses.  No atomics, no allocation, no synchronisation, no environment variable: capturable.
 * N == 0 returns PD_OK after the checks.  Refusals (PD_EINVAL, before the device is touched): null pointers, bad shapes,
 * ldg < W, !(0 < min_depth < max_depth), !(0 < b_lo < b_hi < inf), misaligned pointers, a too-small workspace (naming the
 * needed size), a frame beyond 2^30 pixels.
 *
 * THE EVALUATOR (pd_unc_stats): calibration and sparsification per pixel class in one read of the batch, the sixth evaluator
 * on csrc/class_records.hpp.  gt, pred, unc fp32 [N,H,W] (unc at full resolution); mask, classes, edges, min_depth as
 * pd_depth_stats takes them; max_depth finite and <= PD_USTAT_MAX_DEPTH.
 * PIXEL SET  S(n,k) and p0: those of pd_depth_stats (strict gate, finite pred), and additionally 0 <= u <= 1 (a NaN u fails).
 *            A pixel that passes the gate and the class but not the rest adds 1 to `bad` and takes part in nothing else.
 * Per pixel of S(n,k), in fp64:  e = |gt - p0| (exact);  b, log 2b as above;  e_um = (uint64) rint(e * 1e6), the error in
 *            whole micrometres (<= 1e9);  ub = min(511, (int)(u * 512.f)) (exact in fp32);  eb = the 0.5 mm bin of
 *            pd_depth_stats, #{ j >= 1 : edges[j-1] <= e }, by the same binary search.
 * stats: [N][K] records of PD_USTAT_RECORD_BYTES, written whole by every call; byte offsets:
 *      0  int64   n          |S(n,k)| (the sum of the bins)
 *      8  int64   bad
 *     16  int64   cover50    e <= b * M_LN2    (the central 50 % of a Laplace density of scale b), decided in fp64
 *     24  int64   cover90    e <= b * M_LN10   (the central 90 %)
 *     32  double  sum_nll    sum (e / b + log 2b)
 *     40  double  sum_b      sum b
 *     48  double  sum_e      sum e
 *     56  8 bytes of zero
 *     64  uint32  hist[512]  the count per ub
 * tables: uint64 [N][K][PD_USTAT_TABLE_ROWS = 3][512], written whole by every call: row 0 = sum e_um by ub, row 1 = the
 * count by eb (= pd_depth_stats' hist), row 2 = sum e_um by eb.  From hist and row 0 the host draws the sparsification curve
 * of the stated uncertainty, from rows 1 and 2 the oracle's (polardepth/uncertainty_eval.py).  Two limits of the binning:
 * pixels that share a 1/512 step of u are tied, and the oracle's last error bin (>= 255.5 mm) is open-ended.
 * The integer fields and the tables are integer sums: exact, no order can change them.  The three fp64 sums are
 * bit-reproducible (the scheme of pd_normals_stats).  A class's histogram and tables take 14 KiB of LDS, so a workgroup serves
 * four classes at a time and goes over its pixels once per four classes.  Four launches per 2^20 images; capturable.
 * workspace: >= pd_unc_stats_workspace(N, H, W, K) bytes (never 0, a multiple of 16, monotone), 16-byte aligned.
 * Refusals: those of pd_depth_stats, max_depth above PD_USTAT_MAX_DEPTH or not finite, !(0 < b_lo < b_hi < inf), stats /
 * tables / workspace not 16-byte aligned. */
#define PD_ULOSS_SUMS          4
#define PD_USTAT_BINS          512
#define PD_USTAT_COUNTERS      3        /* bad, cover50, cover90 */
#define PD_USTAT_SUMS          3        /* nll, b, e */
#define PD_USTAT_TABLE_ROWS    3
#define PD_USTAT_RECORD_BYTES  2112     /* 64 + 4 * 512 */
#define PD_USTAT_MAX_DEPTH     1000
int pd_unc_loss_rows(int N, int H, int W);
int pd_unc_loss_fwd(const void* depth, const void* gt, long ldg, const void* unc, int hs, int ws, const void* valid,
                    float min_depth, float max_depth, double b_lo, double b_hi, void* sums, void* value, void* maps,
                    void* workspace, size_t ws_bytes, int N, int H, int W, void* stream);
int pd_unc_loss_bwd(const void* depth, const void* gt, long ldg, const void* unc, int hs, int ws, const void* valid,
                    float min_depth, float max_depth, double b_lo, double b_hi, const void* gvalue, const void* sums,
                    void* gdepth, void* gup, int N, int H, int W, void* stream);
size_t pd_unc_stats_workspace(int N, int H, int W, int K);
int pd_unc_stats(const void* gt, const void* pred, const void* unc, const void* mask, const int* classes, int K,
                 const void* edges, double b_lo, double b_hi, void* stats, void* tables, void* workspace, size_t ws_bytes,
                 int N, int H, int W, float min_depth, float max_depth, void* stream);

/* ---- Polarimetric depth refinement (csrc/polar_refine.hip): the disambiguated polarisation normals (`pol_normal` of
 * pd_polar_normals_stats) integrated back into the depth that disambiguated them.  The coarse depth keeps the low
 * frequencies, the normals supply the relief.  The reference has no counterpart: the definition is this comment, and
 * tests/polar_refine_ref.py states it in NumPy.  fp64 throughout, only + - x / sqrt in the order written here (the library is
 * built without contraction), plus one log per pixel on the way in and one exp on the way out.
 *
 * Inputs.  depth fp32 [N,H,W] contiguous, the prior z; K fp32 [N,4,4] (fx = K[0][0], fy = K[1][1], cx = K[0][2],
 * cy = K[1][2]); pol_normal fp32 [N,H,W,4], 16-byte aligned (the fourth float is not read); xolp fp32 [N,2,H,ldp], only
 * channel 0 (the DoLP rho) is read, with the row pitch ldp >= W in elements (image pitch 2 * H * ldp); valid uint8 [N,H,W] or
 * NULL.
 *
 * A PIXEL (x, y), all in fp64 from the fp32 inputs:
 *     xt = ((double)x - cx) / fx,  yt = ((double)y - cy) / fy            the viewing ray r = (xt, yt, 1)
 *     nr = (nx*xt + ny*yt) + nz,   n2 = (nx*nx + ny*ny) + nz*nz,   r2 = (xt*xt + yt*yt) + 1.0
 *     zeta0 = log((double)z) where z is finite and > 0, else 0.0
 *     live  = z finite and > 0,  n2 finite and > 0,  rho finite and > 0,  valid != 0,  and
 *             fabs(nr) >= cos_inc * (sqrt(n2) * sqrt(r2))                (a NaN fails)
 *     p = -nx / (fx * nr),  q = -ny / (fy * nr)                          d zeta/dx, d zeta/dy of the surface n . dP = 0, P = z r;
 *                                                                        unchanged under n -> -n
 * AN EDGE between a = (x, y) and b = (x+1, y) (E of a, W of b) or b = (x, y+1) (S of a, N of b) is live when both pixels are
 * live and fabs(zeta0_b - zeta0_a) <= edge_max; then  w = sqrt(rho_a * rho_b),  g = (p_a + p_b) * 0.5  (q for S).  A dead edge,
 * and every edge that leaves the image, has w = 0 and g = 0.
 * THE SYSTEM per item: E = sum lam (zeta - zeta0)^2 + sum w (zeta_b - zeta_a - g)^2, whose normal equations have
 *     s    = ((wE + wW) + wS) + wN                                       wW = wE of the left, wN = wS of the upper pixel
 *     diag = (((lam + wE) + wW) + wS) + wN,      idiag = 1.0 / diag
 *     rhs  = (((lam*zeta0 - wE*gE) + wW*gW) - wS*gS) + wN*gN
 * pd_polar_refine_setup writes zeta0 double [N][H][W], coef double [N][4][H][W] = the planes wE, wS, rhs, idiag, and, where pq
 * is not NULL, pq double [N][2][H][W] = (p, q), 0 where the pixel is not live.  A pixel is TOUCHED when s > 0.
 * S[n] = max over the item of s: an exact maximum (partials per workgroup in the workspace, no atomics).
 *
 * THE SOLVER: Chebyshev semi-iteration on D^-1 A, whose spectrum lies in [a, 2 - a], a = lam / (lam + S) (Gershgorin's
 * circles, and the grid is bipartite so the spectrum is symmetric about 1).  No inner products, hence no ordered sums.
 * pd_polar_refine_table writes S and table double [N][iters][2] = (alpha_k, beta_k):
 *     a = lam / (lam + S),  delta = 1.0 - a,  sigma = 1.0 / delta,  rho_0 = 1.0 / sigma
 *     (alpha_0, beta_0) = (0, 1);   rho_k = 1.0 / (2.0*sigma - rho_{k-1}),  alpha_k = rho_k * rho_{k-1},
 *     beta_k = (2.0*rho_k) / delta;   S == 0 (or not finite): every entry of the item is 0 and the item stays at its prior.
 * pd_polar_refine_step, step k, a lane per pixel, zeta ping-pong (zeta_in != zeta_out), d in place:
 *     r = touched ? (rhs + (((wE*zE + wW*zW) + wS*zS) + wN*zN)) * idiag - zeta : 0.0      (a zero weight's neighbour is not read)
 *     d = k == 0 ? beta_0 * r : alpha_k * d + beta_k * r            (k == 0 does not read d)
 *     zeta_out = zeta + d
 * The start is zeta_0 = zeta0.  k must be in [0, iters).
 *
 * pd_polar_refine_finish: depth_out fp32 [N,H,W] = (float)exp(zeta) where touched, else the prior's bits (dead pixels,
 * non-finite and non-positive priors included); touched uint8 [N,H,W]; residual double [N] = max over touched pixels of
 * fabs(r) with r formed from zeta as above (0 where nothing is touched; a NaN is ignored).
 *
 * workspace: >= pd_polar_refine_workspace(N, H, W) bytes (never 0, a multiple of 16, monotone), 16-byte aligned; setup
 * leaves the partial maxima there for table, finish uses it for the residual's.  One launch per call, two for finish
 * (the map, then the maximum): plain vector stores, no atomics, no allocation, no synchronisation, no waiting between workgroups; capturable.
 * N == 0 returns PD_OK after the checks.  Refusals (PD_EINVAL before any launch): null pointers, bad shapes, ldp < W, !(lam > 0),
 * lam / edge_max not finite, edge_max < 0, cos_inc outside (0, 1], iters < 1, k outside [0, iters), zeta_in == zeta_out,
 * misaligned pointers, a too-small workspace, a frame beyond 2^30 pixels or a batch beyond 2^31 workgroups.
 * lam, iters, edge_max and the incidence limit are conventions of the caller, not measurements (polardepth/refine.py). */
size_t pd_polar_refine_workspace(int N, int H, int W);
int pd_polar_refine_setup(const void* depth, const void* K_intrinsics, const void* pol_normal, const void* xolp, long ldp,
                          const void* valid, double lam, double edge_max, double cos_inc, void* zeta0, void* coef, void* pq,
                          void* workspace, size_t ws_bytes, int N, int H, int W, void* stream);
int pd_polar_refine_table(const void* workspace, size_t ws_bytes, double lam, int iters, void* S, void* table, int N, int H,
                          int W, void* stream);
int pd_polar_refine_step(const void* coef, const void* table, int iters, int k, const void* zeta_in, void* zeta_out, void* d,
                         int N, int H, int W, void* stream);
/* pd_polar_refine_steps: the steps k0 .. k0 + T - 1, 1 <= T <= PD_POLAR_REFINE_MAX_T, in ONE launch: a workgroup holds its
 * 64 x 18 pixels and a rim of T around them in LDS and reads the coefficients once (overlapped tiling, the rim is redundant
 * work; workgroups do not wait for each other).  The result equals T calls of pd_polar_refine_step bit for bit.  Here d
 * ping-pongs too: d_in (not read when k0 == 0, may then be NULL) != d_out.  Refusals: those of the step, T outside its range,
 * k0 < 0 or k0 + T > iters, d_in == d_out. */
#define PD_POLAR_REFINE_MAX_T 8
int pd_polar_refine_steps(const void* coef, const void* table, int iters, int k0, int T, const void* zeta_in, void* zeta_out,
                          const void* d_in, void* d_out, int N, int H, int W, void* stream);
int pd_polar_refine_finish(const void* depth, const void* coef, const void* zeta, void* depth_out, void* touched,
                           void* residual, void* workspace, size_t ws_bytes, int N, int H, int W, void* stream);

/* ---- A PER-PIXEL WEIGHT OF THE PRIOR (csrc/polar_refine.hip; NumPy statement: tests/polar_refine_w_ref.py).  The scalar lam
 * trusts the prior equally everywhere.  Here  E = sum lam_i (zeta - zeta0)^2 + sum w (zeta_b - zeta_a - g)^2  with
 *     lam_i = lam * w_i,    w_i = weight_min where !(weight >= weight_min)   (a NaN, a zero, a negative),
 *                                 weight_max where weight > weight_max         (+inf),       else (double)weight
 * from weight fp32 [N,H,W] (any values), the comparisons in fp64.  Liveness and the edges do not depend on the weight:
 *     diag = (((lam_i + wE) + wW) + wS) + wN,    rhs = (((lam_i*zeta0 - wE*gE) + wW*gW) - wS*gS) + wN*gN
 * and everything else is as written above.  THE SPECTRUM: row i of D^-1 A has Gershgorin radius s_i / diag_i and the grid is
 * still bipartite, so the spectrum lies in [a, 2 - a] with
 *     a = min over the touched pixels (s_i > 0) of  a_i = lam_i / (lam_i + s_i)
 * an exact minimum, hence without an order.  With weight == 1 everywhere a equals lam / (lam + S) bit for bit (fp addition and
 * division are monotone), and so does everything that follows.  a >= lam*weight_min / (lam*weight_min + 4*rho_max): a smaller
 * weight_min needs more steps for the same residual.
 * pd_polar_refine_setup_w: pd_polar_refine_setup with the weight; the same zeta0 / coef / pq planes; the workspace (the same
 *     size) receives per workgroup the minimum of a_i, +inf where the workgroup touches nothing.
 * pd_polar_refine_table_w: A double [N] = a of the item, 0 where nothing is touched, and table [N][iters][2] by the recurrence
 *     above started from that a (delta = 1.0 - a, ...); all zero where A is 0, and the item stays at its prior.
 * pd_polar_refine_step, _steps and _finish take the coefficient planes of either setup.
 * pd_polar_refine_weights writes a raw map  weight = (float)(u * h),  a lane per pixel, only + - x / :
 *     u = t*t,  t = (unc_ref * (double)z) / (double)b     from b fp32 [N,H,W], the Laplace scale in metres that the decoder
 *                 states for its depth z (`depth`); NaN where z or b is not finite or not positive; 1.0 where b is NULL.
 *                 unc_ref is the relative scale b / z at which the prior has the weight 1.  A Laplace density has the
 *                 variance 2 b^2: the factor is absorbed in unc_ref.
 *     h = c / r where r = fabs(zeta_prev - zeta0) > c, else 1.0       a Huber data term solved by iteratively reweighted least
 *                 squares: zeta_prev double [N,H,W] is the previous round's solution; 1.0 where zeta_prev is NULL (zeta_prev and
 *                 zeta0 are both given or both NULL).
 * One launch each; plain vector stores, no atomics, no allocation, no synchronisation; capturable.  N == 0 returns PD_OK after the
 * checks.  Refusals (PD_EINVAL before any launch): those of setup / table; a null weight; !(0 < weight_min <= weight_max < inf);
 * !(unc_ref > 0) or not finite when b is given; !(c > 0) or not finite when zeta_prev is given; zeta_prev without zeta0 or the
 * other way round; misaligned pointers.  unc_ref, weight_min and c are conventions of the caller, not measurements. */
int pd_polar_refine_setup_w(const void* depth, const void* K_intrinsics, const void* pol_normal, const void* xolp, long ldp,
                            const void* valid, double lam, double edge_max, double cos_inc, const void* weight,
                            double weight_min, double weight_max, void* zeta0, void* coef, void* pq, void* workspace,
                            size_t ws_bytes, int N, int H, int W, void* stream);
int pd_polar_refine_table_w(const void* workspace, size_t ws_bytes, int iters, void* A, void* table, int N, int H, int W,
                            void* stream);
int pd_polar_refine_weights(const void* depth, const void* b, double unc_ref, const void* zeta_prev, const void* zeta0,
                            double c, void* weight, int N, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* POLARDEPTH_H */
