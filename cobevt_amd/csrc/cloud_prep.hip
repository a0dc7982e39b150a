// Assembly of LiDAR clouds (gfx950): what OpenCOOD's datasets do on the host in front of the
// pre-processors - pcd_utils.mask_ego_points, lidar_project, DataAugmentor's world flip / rotation / scaling, mask_points_by_range and
// the vstack of the agents' clouds - as one operator in front of cobevt_voxelize_points / cobevt_bev_points.
// points (M, 4) fp32 [x, y, z, intensity] of N agents in their SENSOR frames (rows offsets[a] .. offsets[a + 1] of agent a, device
// int32, the offsets convention of voxelize.hip) and T (N, 4, 4) fp64 -> out: the kept points, dense, in the ego frame, and
// out_offsets (N + 1): each agent's start in out.
//
// Semantics (sequential, per agent, in input order - or, with `order`, in the order points[order[i]], i the row; an order entry
// outside [0, M) drops the row):
//   1 ego mask    (optional) point_masks_keep's ego rule on the sensor-frame fp32 point
//   2 projection  (optional) rows r = 0 .. 2 of T[a]: ((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3] in fp64, this association, no
//                 contraction (pcd_utils.lidar_project; its np.dot is BLAS-ordered, so agreement is to the fp32 rounding).  Without
//                 matrices the stage is skipped, not replaced by an identity
//   3 augment     (optional) in the order flip along x (y <- -y), flip along y (x <- -x), rotation, scaling.  Rotation is the
//                 reference's fp32 chain: x, y, z are rounded to fp32, then x' = x c - y s and y' = x s + y c are formed in fp64 from
//                 fp32 values (exact products, one add) and rounded to fp32; c, s are fp32 from the host.  Scaling is
//                 fl32(v * fl32(scale)), NumPy's in-place `*=` of an fp32 array by a Python float.  Intensity is copied bitwise.
//                 DELIBERATE DEVIATION: that is the reference bit for bit where its points are fp32 at this step - raw clouds, and
//                 anything after a rotation.  After a projection WITHOUT a rotation the reference's array is still fp64 and `*=`
//                 multiplies by the fp64 scale; here v (fp64) is multiplied by fl32(scale) all the same and rounded to fp32 once,
//                 which can differ from the reference's value rounded to fp32 by one fp32 ulp on a fair share of the points
//   4 round       the point to fp32
//   5 range mask  (optional) point_masks_keep's range rule (strict inequalities, fp32 limits) on the fp32 OUTPUT point: the
//                 early-fusion order (augment, then crop).  DELIBERATE DEVIATION: where the reference still holds fp64 points at
//                 this step it compares in fp64, so a point within half an fp32 ulp of a limit can differ - 140.7999999 against
//                 140.8 is kept by the fp64 compare and dropped here
//   6 compaction  stable: kept points densely in out, in input (or `order`) order; rows of out at or past out_offsets[N] are NOT
//                 written.  out must not overlap points
// No rule for non-finite values, IEEE comparisons decide: a NaN survives the ego mask and is removed by the range mask.
//
// Boxes (optional, G <= 128 rows of 7, fp32 or fp64, in place, one extra workgroup of the scan launch): rows with mask == 1 get
// stage 3 as augment_utils applies it to boxes, in fp64: flip along x negates y and the heading; flip along y negates x, heading
// <- -(h + pi); rotation rounds x, y, z to fp32, rotates as the points and stores back (so z is rounded to fp32, as the reference's
// slice assignment does), heading += angle; scaling multiplies columns 0 .. 5 by the (fp64) scale; one rounding to the tensor's
// dtype at the end.  Other rows are untouched.  fp64 boxes - what the reference's datasets hold - follow the reference step by step;
// for fp32 boxes NumPy would round after every step (and add fl32(pi), multiply by fl32(scale)), here the chain runs in fp64 and is
// rounded once: a deviation of an fp32 ulp or so per step, on a dtype the reference does not use.
//
// Deterministic parallel form - no workgroup waits on another, no atomics at all:
//   1 classify  256 threads per 1024 points, kScanItems rounds of one point per thread: agent, stages 1 - 5; every wave stores its
//               ballot as the 64-bit flag word of its 64 points, the workgroup its kept count
//   2 scan      ONE workgroup: exclusive scan of the counts, serial over chunks of 1024 (the total at entry `nb`); then
//               out_offsets[a] = scanned count of the 1024-block of row clamp_offset(offsets[a]) + the flag bits before that row
//   3 scatter   per 1024 points: the flag words again, rank in the wave by mbcnt, waves' and rounds' counts through LDS; kept
//               points are computed again and written with one 16-byte store
// The flag that is counted is STORED (a bit per point, 1/128 of the traffic) and read by launches 2 and 3: the ranks and out_offsets
// then agree with the counts by construction, whatever the compiler makes of the arithmetic in two kernels, so no store can leave
// out.  The coordinates come from the same contraction-free function in launches 1 and 3.
// No host read, no allocation (workspace: cobevt_prepare_points_scratch), bitwise reproducible.  M = 0: the scan launch only.
#include "points_common.hpp"

namespace cobevt {

constexpr int kCloudItems = 4;                       // points per thread (kScanItems of voxelize.hip)
constexpr int kCloudBlock = 256 * kCloudItems;       // points per workgroup
constexpr int kCloudMaxBoxes = 128;

struct CloudArgs {
    long M;
    int N, G, ego_mask, range_mask, project, ordered, flip_x, flip_y, rotate, scale_on, box_f64;
    float lo[3], hi[3], c, s, scale;
    double angle, scale_d;
};

__host__ __device__ inline long cloud_blocks(long M) { return (M + kCloudBlock - 1) / kCloudBlock; }
// the workspace, in ints: the flag words (64-bit, first for their alignment), then the block counts and their total
static long cloud_ws_ints(long M) { return 2 * ((M + 63) / 64) + cloud_blocks(M) + 1; }

// the reference's rotation about z on fp32 values: exact fp64 products, one fp64 add, rounded to fp32
__device__ __forceinline__ void cloud_rotate(double& x, double& y, double& z, float c, float s) {
#pragma clang fp contract(off)
    const double xf = (double)(float)x, yf = (double)(float)y;
    const double xc = xf * (double)c, ys = yf * (double)s, xs = xf * (double)s, yc = yf * (double)c;
    x = (double)(float)(xc - ys);
    y = (double)(float)(xs + yc);
    z = (double)(float)z;
}

// stages 1 - 5 of row i (the agent's matrix at T): the fp32 output point and whether it is kept
__device__ __forceinline__ bool cloud_point(const float4 p, const double* __restrict__ T, const CloudArgs& a, float4& q) {
#pragma clang fp contract(off)
    bool keep = point_masks_keep(p, a.lo, a.hi, 0, a.ego_mask);
    double x = (double)p.x, y = (double)p.y, z = (double)p.z;
    if (a.project) {
        const double px = x, py = y, pz = z;
        x = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
        y = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
        z = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
    }
    if (a.flip_x) y = -y;
    if (a.flip_y) x = -x;
    if (a.rotate) cloud_rotate(x, y, z, a.c, a.s);
    if (a.scale_on) {
        const double sc = (double)a.scale;
        x = x * sc; y = y * sc; z = z * sc;
    }
    q.x = (float)x; q.y = (float)y; q.z = (float)z; q.w = p.w;
    return keep && point_masks_keep(q, a.lo, a.hi, a.range_mask, 0);
}

// row i of the (optionally reordered) input, its agent's stages applied; false without an agent or with an order entry outside [0, M)
__device__ __forceinline__ bool cloud_row(const float4* __restrict__ points, const int* __restrict__ offsets,
                                          const double* __restrict__ transforms, const int* __restrict__ order, long i,
                                          const CloudArgs& a, float4& q) {
    if (i >= a.M) return false;
    const int agent = point_agent(offsets, a.N, i, a.M);
    if (agent < 0) return false;
    long src = i;
    if (a.ordered) {
        src = order[i];
        if (src < 0 || src >= a.M) return false;
    }
    return cloud_point(points[src], a.project ? transforms + 16 * (long)agent : nullptr, a, q);
}

__global__ __launch_bounds__(256) void cloud_classify_kernel(const float4* __restrict__ points, const int* __restrict__ offsets,
                                                             const double* __restrict__ transforms, const int* __restrict__ order,
                                                             unsigned long long* __restrict__ flags, int* __restrict__ part, CloudArgs a) {
    __shared__ int lds[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long i0 = (long)blockIdx.x * kCloudBlock + threadIdx.x;
    int kept = 0;                                    // of this wave's points, over the rounds (the same in every lane)
#pragma unroll
    for (int k = 0; k < kCloudItems; ++k) {
        const long i = i0 + k * 256;                 // the wave's 64 rows start at a multiple of 64: they are one flag word
        float4 q;
        const bool keep = cloud_row(points, offsets, transforms, order, i, a, q);
        const unsigned long long bal = __ballot(keep);
        if (lane == 0 && i < a.M) flags[i >> 6] = bal;
        kept += __popcll(bal);
    }
    if (lane == 0) lds[w] = kept;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = lds[0] + lds[1] + lds[2] + lds[3];
}

// the flag bits of rows [o / 1024 * 1024, o)
__device__ __forceinline__ int cloud_flags_before(const unsigned long long* __restrict__ flags, long o) {
    int n = 0;
    for (long wd = (o / kCloudBlock * kCloudBlock) >> 6; wd < (o >> 6); ++wd) n += __popcll(flags[wd]);
    if (o & 63) n += __popcll(flags[o >> 6] & ((1ull << (o & 63)) - 1ull));
    return n;
}

template <typename BT>
__device__ __forceinline__ void cloud_box(BT* __restrict__ boxes, const BT* __restrict__ mask, int g, const CloudArgs& a) {
#pragma clang fp contract(off)
    if (!(mask[g] == (BT)1)) return;
    BT* b = boxes + 7 * g;
    double v[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) v[j] = (double)b[j];
    if (a.flip_x) { v[1] = -v[1]; v[6] = -v[6]; }
    if (a.flip_y) { v[0] = -v[0]; v[6] = -(v[6] + 3.141592653589793); }
    if (a.rotate) { cloud_rotate(v[0], v[1], v[2], a.c, a.s); v[6] = v[6] + a.angle; }
    if (a.scale_on)
#pragma unroll
        for (int j = 0; j < 6; ++j) v[j] = v[j] * a.scale_d;
#pragma unroll
    for (int j = 0; j < 7; ++j) b[j] = (BT)v[j];
}

// workgroup 0: the block counts -> their exclusive prefixes, in place, the total at entry `nb`; then out_offsets.  Workgroup 1 (only
// with boxes): the boxes, one thread per row.
__global__ __launch_bounds__(1024) void cloud_scan_kernel(const int* __restrict__ offsets, const unsigned long long* __restrict__ flags,
                                                          int* __restrict__ part, int* __restrict__ out_offsets, void* __restrict__ boxes,
                                                          const void* __restrict__ box_mask, long nb, CloudArgs a) {
    __shared__ int lds[32];
    if (blockIdx.x == 1) {
        const int g = threadIdx.x;
        if (g < a.G) {
            if (a.box_f64) cloud_box<double>((double*)boxes, (const double*)box_mask, g, a);
            else cloud_box<float>((float*)boxes, (const float*)box_mask, g, a);
        }
        return;
    }
    int carry = 0;
    for (long b0 = 0; b0 < nb; b0 += 1024) {
        const long b = b0 + threadIdx.x;
        const int v = b < nb ? part[b] : 0;
        // inclusive scan over the wave, the waves' totals through LDS
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int x = __shfl_up(inc, o, 64);
            if (lane >= o) inc += x;
        }
        if (lane == 63) lds[w] = inc;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int x = lds[k];
            if (k < w) before += x;
            total += x;
        }
        __syncthreads();
        if (b < nb) part[b] = carry + before + inc - v;
        carry += total;
    }
    if (threadIdx.x == 0) part[nb] = carry;
    __syncthreads();                                 // part is read back below by other threads of this workgroup
    for (int k = threadIdx.x; k <= a.N; k += 1024) {
        const long o = clamp_offset(offsets[k], a.M);
        out_offsets[k] = part[o / kCloudBlock] + cloud_flags_before(flags, o);
    }
}

__global__ __launch_bounds__(256) void cloud_scatter_kernel(const float4* __restrict__ points, const int* __restrict__ offsets,
                                                            const double* __restrict__ transforms, const int* __restrict__ order,
                                                            const unsigned long long* __restrict__ flags, const int* __restrict__ part,
                                                            float4* __restrict__ out, CloudArgs a) {
    __shared__ int lds[4 * kCloudItems];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long i0 = (long)blockIdx.x * kCloudBlock + threadIdx.x;
    unsigned long long bal[kCloudItems];
#pragma unroll
    for (int k = 0; k < kCloudItems; ++k) {
        const long i = i0 + k * 256;
        bal[k] = (i - lane) < a.M ? flags[(i - lane) >> 6] : 0ull;          // uniform over the wave
        if (lane == 0) lds[k * 4 + w] = __popcll(bal[k]);
    }
    __syncthreads();
    const long base = part[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kCloudItems; ++k) {
        if (!((bal[k] >> lane) & 1ull)) continue;
        int before = 0;                              // kept rows of this workgroup in front of the wave's 64 of round k
        for (int j = 0; j < k * 4 + w; ++j) before += lds[j];
        const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(bal[k] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal[k], 0));
        const long i = i0 + k * 256;
        float4 q;
        cloud_row(points, offsets, transforms, order, i, a, q);
        const long at = base + before + rank;
        if (at < a.M) out[at] = q;                   // always true: the counts are the stored flags'
    }
}

// dims: [M, N, G, ego_mask, range_mask, flip_x, flip_y, rotate, scale, boxes are fp64] ;
// geom: [x0, y0, z0, x1, y1, z1 (range mask), cos, sin (fp32 values), angle, scale] (doubles)
static int cloud_args(const long* dims, const double* geom, CloudArgs& a) {
    if (!dims) return COBEVT_ERR_ARG;
    const long M = dims[0], N = dims[1], G = dims[2];
    if (M < 0 || M > 0x7fffffffL - kCloudBlock || N < 1 || N > 65535 || G < 0 || G > kCloudMaxBoxes) return COBEVT_ERR_SHAPE;
    a.M = M; a.N = (int)N; a.G = (int)G;
    a.ego_mask = dims[3] != 0; a.range_mask = dims[4] != 0; a.flip_x = dims[5] != 0; a.flip_y = dims[6] != 0;
    a.rotate = dims[7] != 0; a.scale_on = dims[8] != 0; a.box_f64 = dims[9] != 0;
    a.project = 0; a.ordered = 0;
    for (int j = 0; j < 3; ++j) { a.lo[j] = 0.f; a.hi[j] = 0.f; }
    a.c = 1.f; a.s = 0.f; a.scale = 1.f; a.angle = 0.0; a.scale_d = 1.0;
    if (geom) {
        for (int j = 0; j < 3; ++j) { a.lo[j] = (float)geom[j]; a.hi[j] = (float)geom[3 + j]; }
        a.c = (float)geom[6]; a.s = (float)geom[7]; a.angle = geom[8]; a.scale_d = geom[9]; a.scale = (float)geom[9];
    }
    return COBEVT_OK;
}

}  // namespace cobevt

using namespace cobevt;

extern "C" int cobevt_prepare_points_scratch(const long* dims, long* workspace_ints) {
    CloudArgs a;
    if (!workspace_ints) return COBEVT_ERR_ARG;
    const int rc = cloud_args(dims, nullptr, a);
    if (rc != COBEVT_OK) return rc;
    *workspace_ints = cloud_ws_ints(a.M);
    return COBEVT_OK;
}

extern "C" int cobevt_prepare_points(const float* points, const int* point_offsets, const double* transforms, const int* order, float* out,
                                     int* out_offsets, void* boxes, const void* box_mask, int* workspace, const long* dims,
                                     const double* geom, hipStream_t stream) {
    if (!dims || !geom || !point_offsets || !out_offsets || !workspace) return COBEVT_ERR_ARG;
    CloudArgs a;
    const int rc = cloud_args(dims, geom, a);
    if (rc != COBEVT_OK) return rc;
    if (a.M > 0 && (!points || !out)) return COBEVT_ERR_ARG;
    if (a.G > 0 && (!boxes || !box_mask)) return COBEVT_ERR_ARG;
    if ((((uintptr_t)points | (uintptr_t)out) & 15) || (((uintptr_t)workspace | (uintptr_t)transforms | (uintptr_t)boxes | (uintptr_t)box_mask) & 7))
        return COBEVT_ERR_SHAPE;
    if (((uintptr_t)order | (uintptr_t)point_offsets | (uintptr_t)out_offsets) & 3) return COBEVT_ERR_SHAPE;
    a.project = transforms != nullptr;
    a.ordered = order != nullptr;
    const long nb = cloud_blocks(a.M);
    unsigned long long* flags = (unsigned long long*)workspace;
    int* part = workspace + 2 * ((a.M + 63) / 64);
    if (nb)
        hipLaunchKernelGGL(cloud_classify_kernel, dim3((unsigned)nb), dim3(256), 0, stream, (const float4*)points, point_offsets, transforms,
                           order, flags, part, a);
    hipLaunchKernelGGL(cloud_scan_kernel, dim3(a.G > 0 ? 2u : 1u), dim3(1024), 0, stream, point_offsets, (const unsigned long long*)flags,
                       part, out_offsets, boxes, box_mask, nb, a);
    if (nb)
        hipLaunchKernelGGL(cloud_scatter_kernel, dim3((unsigned)nb), dim3(256), 0, stream, (const float4*)points, point_offsets, transforms,
                           order, (const unsigned long long*)flags, (const int*)part, (float4*)out, a);
    return cobevt::launch_status();
}
