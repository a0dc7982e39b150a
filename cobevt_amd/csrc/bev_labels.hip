// PIXOR-style per-pixel detection label maps (gfx950): OpenCOOD's LidarBevPostprocessor.generate_label for a batch.  The other
// direction, its post_process, is the bev mode of detect_post.hip (cobevt_bev_post).
//
// Labels (lidar_bev_postprocessor.py generate_label / update_label_map / normalize_targets, box_utils.get_points_in_rotated_box),
// per sample b: gt (G, 7) fp32 [x, y, z, dx, dy, dz, yaw] in 'lwh' order, G <= 128 slots of which the ones with mask == 1 are valid,
// compacted in slot order as `gt_box_center[mask == 1]` does.
//   corners     0 .. 3 of boxes_to_corners_3d(order = 'lwh') in separately rounded fp32, as the reference's torch fp32 chain makes
//               them (box_footprint_corner of detect_common.hpp, the function cobevt_boxes_standup uses); cos / sin of the yaw are
//               the fp64 functions rounded to fp32: the correctly rounded values, which is what a good host cosf returns
//   after that  fp64 in the reference's operation order: corner_dist = (corner - origin) / res / downsample_rate; integer pixel
//               (i, j) belongs to a box when l = (p_rel . edge) / (edge . edge) lies in [0, 1] INCLUSIVE for the edges c1 - c0 and
//               c3 - c0; the pixel's continuous position is ((i, j) + origin / res / rate) * res * rate; targets [cos yaw, sin yaw,
//               x - px, y - py, log dx, log dy] from the fp32 box widened to fp64
//   overlap     the reference's loop lets the LAST valid box win: the kernel walks the boxes from last to first and stops at the hit
//   normalise   (v - target_mean) / target_std_dev on channels 1 .. 6 of EVERY pixel, background included; one cast to fp32
//   skipped     a box with an edge of squared norm <= 1e-6 (or not comparable: NaN) - the reference asserts there - marks no pixel;
//               its corners are still written
// One launch, one thread per label pixel, no atomics: the first G threads of each workgroup build the per-box constants (c0, the two
// edges, their squared norms, the six targets) once into LDS; workgroup 0 of a sample also writes bev_corners (valid boxes
// compacted to the front, zero rows behind them) and num_valid.
#include "detect_common.hpp"           // kTgtMaxGt and box_footprint_corner (detect_targets.hip), bev_params_ok (detect_post.hip)

namespace cobevt {

struct BevLabelArgs {
    int B, G, lx, ly;
    double x0, y0, res, rate, mean[6], std[6];
};
constexpr int kBevBoxDoubles = 14;                   // c0 (2), edge 1 (2), edge 2 (2), their squared norms (2), the targets (6)

// grid (ceil(lx ly / 256), B)
__global__ __launch_bounds__(256) void bev_labels_kernel(const float* __restrict__ gt, const float* __restrict__ mask,
                                                         float* __restrict__ label_map, float* __restrict__ bev_corners,
                                                         int* __restrict__ num_valid, BevLabelArgs a) {
#pragma clang fp contract(off)
    __shared__ double s_box[kTgtMaxGt][kBevBoxDoubles];
    __shared__ int s_valid[kTgtMaxGt];
    const int t = threadIdx.x, b = blockIdx.y, G = a.G;
    if (t < kTgtMaxGt) s_valid[t] = (t < G && mask[(long)b * G + t] == 1.f) ? 1 : 0;
    __syncthreads();
    int n = 0, rank = 0;
    for (int j = 0; j < G; ++j) {
        const int v = s_valid[j];
        n += v;
        if (j < t) rank += v;
    }
    if (t < G && s_valid[t]) {
        const float* q = gt + ((long)b * G + t) * 7;
        const float sx = q[3] * 0.5f, sy = q[4] * 0.5f;          // 'lwh': the size columns as they stand
        const double yaw = (double)q[6];
        const float cs = (float)cos(yaw), sn = (float)sin(yaw);
        double X[4], Y[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float fx, fy;
            box_footprint_corner(k, q[0], q[1], sx, sy, cs, sn, fx, fy);
            if (blockIdx.x == 0) {
                bev_corners[(((long)b * G + rank) * 4 + k) * 2] = fx;
                bev_corners[(((long)b * G + rank) * 4 + k) * 2 + 1] = fy;
            }
            X[k] = (((double)fx - a.x0) / a.res) / a.rate;
            Y[k] = (((double)fy - a.y0) / a.res) / a.rate;
        }
        double* o = s_box[rank];
        const double e1x = X[1] - X[0], e1y = Y[1] - Y[0], e2x = X[3] - X[0], e2y = Y[3] - Y[0];
        const double n1 = e1x * e1x + e1y * e1y, n2 = e2x * e2x + e2y * e2y;
        o[0] = X[0]; o[1] = Y[0]; o[2] = e1x; o[3] = e1y; o[4] = e2x; o[5] = e2y;
        o[6] = (n1 > 1e-6 && n2 > 1e-6) ? n1 : -1.0;             // -1: the reference asserts on this box; it marks no pixel
        o[7] = n2;
        o[8] = cos(yaw); o[9] = sin(yaw); o[10] = (double)q[0]; o[11] = (double)q[1];
        o[12] = log((double)q[3]); o[13] = log((double)q[4]);
    }
    if (blockIdx.x == 0) {
        if (t < G && t >= n) {
#pragma unroll
            for (int k = 0; k < 8; ++k) bev_corners[((long)b * G + t) * 8 + k] = 0.f;
        }
        if (t == 0) num_valid[b] = n;
    }
    __syncthreads();
    const int plane = a.lx * a.ly;
    const int p = blockIdx.x * 256 + t;
    if (p >= plane) return;
    const int i = p / a.ly, j = p - i * a.ly;
    double out[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) out[k] = 0.0;
    for (int k = n - 1; k >= 0; --k) {
        const double* o = s_box[k];
        if (o[6] < 0.0) continue;
        const double prx = (double)i - o[0], pry = (double)j - o[1];
        const double l1 = (prx * o[2] + pry * o[3]) / o[6];
        const double l2 = (prx * o[4] + pry * o[5]) / o[7];
        if (l1 >= 0.0 && l1 <= 1.0 && l2 >= 0.0 && l2 <= 1.0) {
            // transformation_utils.dist_to_continuous
            const double px = (((double)i + (a.x0 / a.res) / a.rate) * a.res) * a.rate;
            const double py = (((double)j + (a.y0 / a.res) / a.rate) * a.res) * a.rate;
            out[0] = 1.0; out[1] = o[8]; out[2] = o[9]; out[3] = o[10] - px; out[4] = o[11] - py; out[5] = o[12]; out[6] = o[13];
            break;
        }
    }
    float* dst = label_map + (long)b * 7 * plane + p;
    dst[0] = (float)out[0];
#pragma unroll
    for (int k = 1; k < 7; ++k) dst[(long)k * plane] = (float)((out[k] - a.mean[k - 1]) / a.std[k - 1]);
}

}  // namespace cobevt

using namespace cobevt;

extern "C" int cobevt_bev_labels(const float* gt_boxes, const float* mask, float* label_map, float* bev_corners, int* num_valid,
                                 const int* dims, const double* params, hipStream_t stream) {
    if (!dims || !params || !label_map || !num_valid) return COBEVT_ERR_ARG;
    const long B = dims[0], G = dims[1], lx = dims[2], ly = dims[3];
    if (G < 0 || G > kTgtMaxGt) return COBEVT_ERR_SHAPE;
    if (G > 0 && (!gt_boxes || !mask || !bev_corners)) return COBEVT_ERR_ARG;
    if (B < 1 || B > 65535 || lx < 1 || ly < 1 || lx > 0x7fffffffL / ly || lx * ly > (0x7fffffffL / 8) / B) return COBEVT_ERR_SHAPE;
    if (!bev_params_ok(params)) return COBEVT_ERR_SHAPE;
    BevLabelArgs a;
    a.B = (int)B; a.G = (int)G; a.lx = (int)lx; a.ly = (int)ly;
    a.x0 = params[0]; a.y0 = params[1]; a.res = params[2]; a.rate = params[3];
    for (int k = 0; k < 6; ++k) { a.mean[k] = params[4 + k]; a.std[k] = params[10 + k]; }
    hipLaunchKernelGGL(bev_labels_kernel, dim3((unsigned)((lx * ly + 255) / 256), (unsigned)B), dim3(256), 0, stream, gt_boxes, mask,
                       label_map, bev_corners, num_valid, a);
    return cobevt::launch_status();
}
