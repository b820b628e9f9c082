// pcl_pano_pixel.h — make_pano's centre pixel of a camera-frame point, for the kernels that render or project outside the loss kernel
// (pcl_hist.hip: splat, bin and fix-up; pcl_score.hip: the block a point votes with).  Moved here from pcl_hist.hip word for word, so that
// both translation units run the same instructions on the same inputs.
#pragma once
#include "pcl_device.h"

// ||p|| with ONE rounding sequence at every call site (splat, bin, fix-up): the depth decides which point owns a pixel
__device__ __forceinline__ float pcl_point_depth(float px, float py, float pz)
{
#pragma clang fp contract(off)
    return sqrtf(px * px + py * py + pz * pz);
}

__device__ inline void pcl_pano_pixel_ref(float px, float py, float pz, int H, int W, int& row, int& col)
{
#pragma clang fp contract(off)
    // make_pano's pixel (utils.py:158-165) with the reference's operation order (same as pcl_ops.hip)
    float gx, gy;
    pcl_cloud2idx_point(px, py, pz, gx, gy);
    float cx = (gx + 1.0f) / 2.0f * (float)(W - 1);
    float cy = (gy + 1.0f) / 2.0f * (float)(H - 1);
    col = min(max((int)cx, 0), W - 1);
    row = min(max((int)cy, 0), H - 1);
}

// The fractional pixel coordinates from the loss kernel's fast atan2 (octant reduction + degree-8 polynomial, v_rcp / v_rsq: ~45
// instructions against ~170 for the two library atan2f of pcl_pano_pixel_ref): within a few fp32 ulps of the reference formula's (angle
// error <= 6e-7 rad against the library's, the affine chain's roundings: <= 1e-6 W pixels in all).
__device__ __forceinline__ void pcl_pano_coord_fast(float px, float py, float pz, int H, int W, float& cx, float& cy)
{
    const float pi = 3.14159265358979323846f, inv_two_pi = 0.15915494309189532f, inv_pi = 0.31830988618379067154f;
    const float rho2 = fmaf(px, px, py * py);
    const float rho = rho2 * __builtin_amdgcn_rsqf(rho2 + 1e-37f);
    const float theta = pcl_atan2_ypos(rho, pz + 1e-6f);
    const float phi = pcl_atan2(py, px + 1e-6f) + pi;
    const float gx = 2.0f * (1.0f - phi * inv_two_pi) - 1.0f, gy = 2.0f * (theta * inv_pi) - 1.0f;
    cx = (gx + 1.0f) * 0.5f * (float)(W - 1); cy = (gy + 1.0f) * 0.5f * (float)(H - 1);
}

// The pixel from the same coordinates, with a CERTIFICATE: whenever both coordinates are farther than `margin` from an integer — and
// inside the image — truncation gives the reference's pixel.  Returns false otherwise (0.5-1.5 % of the points): those are recomputed with
// the reference formula (pcl_bin_kernel's fix-up queue).  The bit-identity of the whole stage against the z-buffer splat path, which only
// knows the reference formula, is what tests/test_hip_harness.py::test_hist_trim_tile_binned_equals_the_zbuffer_path checks on every scene
// it runs.
__device__ __forceinline__ bool pcl_pano_pixel_fast(float px, float py, float pz, int H, int W, float margin_x, float margin_y, int& row, int& col)
{
    // (pcl_pano_coord_fast's lines once more, not a call: through the call pcl_bin_kernel compiled to another instruction stream)
    const float pi = 3.14159265358979323846f, inv_two_pi = 0.15915494309189532f, inv_pi = 0.31830988618379067154f;
    const float rho2 = fmaf(px, px, py * py);
    const float rho = rho2 * __builtin_amdgcn_rsqf(rho2 + 1e-37f);
    const float theta = pcl_atan2_ypos(rho, pz + 1e-6f);
    const float phi = pcl_atan2(py, px + 1e-6f) + pi;
    const float gx = 2.0f * (1.0f - phi * inv_two_pi) - 1.0f, gy = 2.0f * (theta * inv_pi) - 1.0f;
    const float cx = (gx + 1.0f) * 0.5f * (float)(W - 1), cy = (gy + 1.0f) * 0.5f * (float)(H - 1);
    const float fx = cx - floorf(cx), fy = cy - floorf(cy);
    col = (int)cx; row = (int)cy;
    // (a NaN coordinate fails every compare: not certain)
    return fx > margin_x && fx < 1.0f - margin_x && fy > margin_y && fy < 1.0f - margin_y && cx > margin_x && cx < (float)(W - 1) - margin_x &&
           cy > margin_y && cy < (float)(H - 1) - margin_y;
}
