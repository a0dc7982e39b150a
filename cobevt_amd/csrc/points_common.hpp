// Shared device helpers of the LiDAR point operators (voxelize.hip, bev_points.hip, cloud_prep.hip): the offsets convention of a
// stacked cloud - points (M, 4) fp32 of N agents, rows offsets[a] .. offsets[a + 1] of agent a, device int32 - and the two point masks.
#pragma once
#include "common.hpp"

namespace cobevt {

__device__ __forceinline__ long clamp_offset(int o, long M) { return o < 0 ? 0 : (o > M ? M : (long)o); }

// the agent that owns row i (-1: none): rows offsets[a] .. offsets[a + 1], offsets clamped to [0, M]
__device__ __forceinline__ int point_agent(const int* __restrict__ offsets, int N, long i, long M) {
    int agent = -1;
    for (int k = 0; k < N; ++k)
        if (agent < 0 && i >= clamp_offset(offsets[k], M) && i < clamp_offset(offsets[k + 1], M)) agent = k;
    return agent;
}

// pcd_utils.mask_points_by_range (:54-58, strict inequalities) and mask_ego_points (:79-80), each when its flag is set
__device__ __forceinline__ bool point_masks_keep(const float4 p, const float* lo, const float* hi, int range_mask, int ego_mask) {
    bool keep = true;
    if (range_mask) keep = keep && p.x > lo[0] && p.x < hi[0] && p.y > lo[1] && p.y < hi[1] && p.z > lo[2] && p.z < hi[2];
    if (ego_mask) keep = keep && !(p.x >= -1.95f && p.x <= 2.95f && p.y >= -1.1f && p.y <= 1.1f);
    return keep;
}

}  // namespace cobevt
