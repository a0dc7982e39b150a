// LiDAR points -> PIXOR's `bev_input` (gfx950): OpenCOOD's BevPreprocessor.preprocess for N agents.
// points (M, 4) fp32 [x, y, z, intensity] (rows offsets[a] .. offsets[a + 1] of agent a, device int32) -> bev (N, C, nx, ny) fp32, or
// (N, nx, ny, C) with channels_last: channels 0 .. C - 2 are the binary occupancy of the height slices, channel C - 1 the mean
// intensity of the cell's points.  The point masks and the offsets convention are voxelize.hip's: the device functions of
// points_common.hpp are the ones its classify launch calls.
//
// Semantics (bev_preprocessor.py :29-47, per agent):
//   index     trunc(((double)p - origin) / res) per axis: fp64 arithmetic on the fp32 point, as numpy promotes `pcd_raw[:, :3] -
//             bev_origin`, and `.astype(int)` truncates toward zero - it is NOT floor: a point in (origin - res, origin) lands in cell 0
//   dropped   a point with a non-finite coordinate or intensity, removed by a mask, with |intensity| >= 2^8 (see below), or whose
//             truncated index is outside [0, nx) x [0, ny) x [0, C - 1).  The last rule is a DELIBERATE DEVIATION: the reference
//             lets a negative index wrap to the far side of the map, raises on an index past the end, and writes a height hit with
//             iz = C - 1 into the intensity channel; none of that is meant.
//   kept      bev[ix, iy, iz] = 1; the intensity channel is the mean intensity of the cell's kept points, 0 for a cell without one.
//
// Deterministic parallel form.  The reference's fp32 running sum depends on the order of the points (the dataset shuffles them);
// here nothing depends on the order of the points, of the workgroups or of the atomics:
//   1 (memset)  bev <- 0, the workspace <- 0
//   2 points    one thread per point: the occupancy store (every writer stores the same 1.0f) and two INTEGER atomics per kept
//               point: count[cell] += 1 (32 bits) and sum[cell] += rint(intensity * 2^32) (64 bits, two's complement)
//   3 finalise  one thread per cell: mean = ((double)sum * 2^-32) / count, rounded to fp32 once
// Fixed point: the quantum is 2^-32.  An intensity with 2^-9 <= |i| < 2^8 is a multiple of the quantum and is summed EXACTLY; below
// 2^-9 the per-point quantisation error is at most 2^-33; |i| >= 2^8 is outside the domain and the point is dropped like a
// non-finite one (not summed wrongly).  With |i| < 2^8 a cell holds 2^23 points before the 64-bit sum can overflow.  The result
// therefore satisfies |mean_out - mean| <= 2^-33 + 2^-24 |mean| (1 + 2^-20) against the exact mean of the kept intensities, and is
// bitwise identical under any permutation of the points and from run to run.
// The two words of a cell live in separate arrays (voxelize.hip measured a cell's atomics' words in one record at 166 us against
// 97 us); this kernel itself has not been timed.
// No floating-point atomics, no host read-back, no allocation: the workspace comes from the caller (cobevt_bev_points_scratch).
#include "points_common.hpp"

namespace cobevt {

struct BevPointArgs {
    long M;
    int N, nx, ny, C, range_mask, ego_mask, channels_last;
    float lo[3], hi[3];                              // cav_lidar_range, for the range mask
    double origin[3], res;                           // L1, W1, H1 and the cell size
};

constexpr double kBevFixed = 4294967296.0;           // 2^32: the fixed-point scale of the intensity sum
constexpr float kBevMaxIntensity = 256.f;            // 2^8: |intensity| at and past this is outside the summed domain

// the workspace: sum (cells 64-bit words) first, for its alignment, then count (cells ints)
static long bev_points_ws_ints(const BevPointArgs& a) { return 3L * a.N * a.nx * a.ny; }

__global__ __launch_bounds__(256) void bev_points_kernel(const float4* __restrict__ points, const int* __restrict__ offsets,
                                                         float* __restrict__ bev, unsigned long long* __restrict__ sum,
                                                         int* __restrict__ count, BevPointArgs a) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.M) return;
    const int agent = point_agent(offsets, a.N, i, a.M);
    if (agent < 0) return;
    const float4 p = points[i];
    bool keep = isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(p.w) && fabsf(p.w) < kBevMaxIntensity;
    keep = keep && point_masks_keep(p, a.lo, a.hi, a.range_mask, a.ego_mask);
    // trunc, compared as doubles: a quotient past the int range drops the point; -0.0 (a point just below the origin) is cell 0
    const double tx = trunc(((double)p.x - a.origin[0]) / a.res);
    const double ty = trunc(((double)p.y - a.origin[1]) / a.res);
    const double tz = trunc(((double)p.z - a.origin[2]) / a.res);
    keep = keep && tx >= 0.0 && tx < (double)a.nx && ty >= 0.0 && ty < (double)a.ny && tz >= 0.0 && tz < (double)(a.C - 1);
    if (!keep) return;
    const int ix = (int)tx, iy = (int)ty, iz = (int)tz;
    const long cell = ((long)agent * a.nx + ix) * a.ny + iy;
    const long at = a.channels_last ? cell * a.C + iz : (((long)agent * a.C + iz) * a.nx + ix) * a.ny + iy;
    bev[at] = 1.f;
    atomicAdd(&count[cell], 1);
    atomicAdd(&sum[cell], (unsigned long long)(long long)rint((double)p.w * kBevFixed));
}

__global__ __launch_bounds__(256) void bev_points_finalise_kernel(float* __restrict__ bev, const unsigned long long* __restrict__ sum,
                                                                  const int* __restrict__ count, BevPointArgs a) {
    const long cells = (long)a.N * a.nx * a.ny;
    const long cell = (long)blockIdx.x * 256 + threadIdx.x;
    if (cell >= cells) return;
    const int n = count[cell];
    if (n <= 0) return;                              // the memset left the cell's intensity at 0
    const double mean = ((double)(long long)sum[cell] * (1.0 / kBevFixed)) / (double)n;
    const long per = (long)a.nx * a.ny;
    const long agent = cell / per, r = cell - agent * per;
    const long at = a.channels_last ? cell * a.C + (a.C - 1) : (agent * a.C + (a.C - 1)) * per + r;
    bev[at] = (float)mean;
}

// dims: [M, N, nx, ny, C, range_mask, ego_mask, channels_last] ; geom: [x0, y0, z0, x1, y1, z1, L1, W1, H1, res] (doubles)
static int bev_points_args(const long* dims, const double* geom, BevPointArgs& a) {
    if (!dims) return COBEVT_ERR_ARG;
    const long M = dims[0], N = dims[1], nx = dims[2], ny = dims[3], C = dims[4];
    if (M < 0 || M > 0x7fffffffL - 256 || N < 1 || N > 65535 || nx < 1 || ny < 1 || C < 2 || C > 65535) return COBEVT_ERR_SHAPE;
    if (nx > 0x7fffffffL / ny || nx * ny > 0x7fffffffL / N || nx * ny * N > (0x7fffffffL / 4) / C) return COBEVT_ERR_SHAPE;
    a.M = M; a.N = (int)N; a.nx = (int)nx; a.ny = (int)ny; a.C = (int)C;
    a.range_mask = dims[5] != 0; a.ego_mask = dims[6] != 0; a.channels_last = dims[7] != 0;
    if (geom) {
        for (int j = 0; j < 3; ++j) { a.lo[j] = (float)geom[j]; a.hi[j] = (float)geom[3 + j]; a.origin[j] = geom[6 + j]; }
        a.res = geom[9];
    }
    return COBEVT_OK;
}

}  // namespace cobevt

using namespace cobevt;

extern "C" int cobevt_bev_points_scratch(const long* dims, long* workspace_ints) {
    BevPointArgs a;
    if (!workspace_ints) return COBEVT_ERR_ARG;
    const int rc = bev_points_args(dims, nullptr, a);
    if (rc != COBEVT_OK) return rc;
    *workspace_ints = bev_points_ws_ints(a);
    return COBEVT_OK;
}

extern "C" int cobevt_bev_points(const float* points, const int* point_offsets, float* bev, int* workspace, const long* dims,
                                 const double* geom, hipStream_t stream) {
    if (!dims || !geom || !point_offsets || !bev || !workspace) return COBEVT_ERR_ARG;
    BevPointArgs a;
    const int rc = bev_points_args(dims, geom, a);
    if (rc != COBEVT_OK) return rc;
    if (a.M > 0 && !points) return COBEVT_ERR_ARG;
    if (((uintptr_t)points & 15) || ((uintptr_t)workspace & 7) || ((uintptr_t)bev & 3)) return COBEVT_ERR_SHAPE;
    if (!(a.res > 0.0) || a.res - a.res != 0.0) return COBEVT_ERR_SHAPE;              // positive and finite
    for (int j = 0; j < 3; ++j)
        if (a.origin[j] - a.origin[j] != 0.0) return COBEVT_ERR_SHAPE;
    const long cells = (long)a.N * a.nx * a.ny;
    unsigned long long* sum = (unsigned long long*)workspace;
    int* count = workspace + 2 * cells;
    if (hipMemsetAsync(bev, 0, 4 * (size_t)cells * a.C, stream) != hipSuccess) return COBEVT_ERR_LAUNCH;
    if (hipMemsetAsync(workspace, 0, 12 * (size_t)cells, stream) != hipSuccess) return COBEVT_ERR_LAUNCH;
    const unsigned pb = (unsigned)((a.M + 255) / 256);         // one thread per point
    if (pb)
        hipLaunchKernelGGL(bev_points_kernel, dim3(pb), dim3(256), 0, stream, (const float4*)points, point_offsets, bev, sum, count, a);
    hipLaunchKernelGGL(bev_points_finalise_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, bev,
                       (const unsigned long long*)sum, (const int*)count, a);
    return cobevt::launch_status();
}
