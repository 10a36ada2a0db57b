// The source index of torch's upsample_bilinear2d with align_corners=False: shared by csrc/loss.hip (pd_disp_to_depth,
// pd_up_gather_bwd) and csrc/unc_loss.hip, so that a map sampled in one and folded back in the other uses the same weights
// bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace pd_up {

__device__ __forceinline__ void src_index(int dst, float scale, int in_size, int& i0, int& i1, float& l1) {
    const float s = fmaxf(scale * (dst + 0.5f) - 0.5f, 0.f);
    i0 = (int)s;
    if (i0 > in_size - 1) i0 = in_size - 1;
    i1 = i0 + (i0 < in_size - 1);
    l1 = s - i0;
}

// map [hs][ws] of one image sampled at pixel (x, y) of the H x W frame (sh = hs / H, sw = ws / W), in fp32 in the operation
// order of pd_disp_to_depth
__device__ __forceinline__ float sample(const float* __restrict__ m, int hs, int ws, float sh, float sw, int x, int y) {
    int y0, y1, x0, x1; float ly1, lx1;
    src_index(y, sh, hs, y0, y1, ly1);
    src_index(x, sw, ws, x0, x1, lx1);
    const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
    return ly0 * (lx0 * m[y0 * ws + x0] + lx1 * m[y0 * ws + x1]) + ly1 * (lx0 * m[y1 * ws + x0] + lx1 * m[y1 * ws + x1]);
}

}  // namespace pd_up
