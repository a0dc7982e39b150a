// Shared pieces of the LiDAR detection sources: the ground-truth slot count and the rotated footprint corner of detect_targets.hip and
// bev_labels.hip, and the parameter check of the per-pixel (PIXOR) maps that bev_labels.hip and detect_post.hip's bev mode both make.
#pragma once
#include "common.hpp"

namespace cobevt {

constexpr int kTgtMaxGt = 128;

// footprint corner k = 0 .. 3 of boxes_to_corners_3d: half sizes (sx, sy) along the box axes, the template [1,-1] [1,1] [-1,1] [-1,-1] / 2,
// rotate_points_along_z: [x y] [[cos, sin], [-sin, cos]], then the centre - every product and sum a separately rounded fp32 operation.
// The caller gives cos / sin of the yaw (tgt_standup_kernel: cosf / sinf; bev_labels.hip: the fp64 functions rounded to fp32).
__device__ __forceinline__ void box_footprint_corner(int k, float cx, float cy, float sx, float sy, float cs, float sn, float& X,
                                                     float& Y) {
#pragma clang fp contract(off)
    const float x = k < 2 ? sx : -sx, y = (k == 1 || k == 2) ? sy : -sy;
    X = (x * cs + y * -sn) + cx;
    Y = (x * sn + y * cs) + cy;
}

// params: [L1, W1, res, downsample_rate, target_mean (6), target_std_dev (6)]
inline bool bev_params_ok(const double* q) {
    for (int k = 0; k < 16; ++k)
        if (!(q[k] == q[k]) || q[k] - q[k] != 0.0) return false;                    // finite
    if (!(q[2] > 0.0) || !(q[3] > 0.0)) return false;
    for (int k = 10; k < 16; ++k)
        if (q[k] == 0.0) return false;
    return true;
}

}  // namespace cobevt
