// Shared by csrc/polar_normals_stats.hip and csrc/polar_loss.hip: the frame of a pixel's viewing ray.  K1's candidates are
// quantities about that ray (the zenith from DoLP is the angle to it, the azimuth from AoLP is measured around it), the
// predicted normal is formed in camera coordinates; the two agree only at the principal point.  R(x, y) is the MINIMAL
// rotation that takes the unit ray u = r / |r|, r = ((x - cx) / fx, (y - cy) / fy, 1), onto (0, 0, 1): it gives the exact
// zenith (p'z = p.u), keeps every angle, and carries the component across the meridional plane unchanged while the one in
// it turns with the ray.  fp64 from the fp32 intrinsics and the integer pixel position, only + - x / sqrt, in the operation
// order of include/polardepth.h; both translation units are built without contraction, so tests/polar_ray_ref.py reproduces
// every bit.  1 + uz > 1: no division hazard.  A zero or NaN focal length gives a non-finite frame, hence a non-finite p'
// (the pixel is `bad`); no address depends on the frame.
#pragma once
#include "depth_normals.hpp"

namespace pd_ray {

struct Frame { double ux, uy, uz; };

__device__ __forceinline__ Frame make(pd_dn::Cam c, int x, int y) {
    const double xt = ((double)x - (double)c.cx) / (double)c.fx, yt = ((double)y - (double)c.cy) / (double)c.fy;
    const double L = sqrt((xt * xt + yt * yt) + 1.0);
    return Frame{xt / L, yt / L, 1.0 / L};
}

// p <- R p.  On the axis (ux = uy = 0, uz = 1) s = (pz + pz) / 2 = pz and p is unchanged
__device__ __forceinline__ void rotate(const Frame& f, double& px, double& py, double& pz) {
    const double d = (px * f.ux + py * f.uy) + pz * f.uz;
    const double s = (d + pz) / (1.0 + f.uz);
    px = px - s * f.ux; py = py - s * f.uy; pz = d;
}

// g <- R^T g: <R v, w> = <v, R^T w>
__device__ __forceinline__ void rotate_t(const Frame& f, double& gx, double& gy, double& gz) {
    const double d = (gx * f.ux + gy * f.uy) + gz * f.uz;
    const double s = (d + gz) / (1.0 + f.uz);
    const double t = 2.0 * gz;
    gx = (gx - s * f.ux) + t * f.ux; gy = (gy - s * f.uy) + t * f.uy; gz = (gz - s * (f.uz + 1.0)) + t * f.uz;
}

}  // namespace pd_ray
