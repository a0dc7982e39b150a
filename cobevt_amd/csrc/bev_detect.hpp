// PIXOR-style per-pixel detection maps (gfx950), included by detect_post.hip only (after DetSrc / DetWs and the rounded fp32 helpers):
// OpenCOOD's LidarBevPostprocessor.generate_label for a batch, and the decode launch of its post_process.  The selection of the 1000
// best, the fp64 quad clip and the greedy NMS behind the decode are detect_post.hip's own launches - nothing of them is copied here.
//
// Labels (lidar_bev_postprocessor.py generate_label / update_label_map / normalize_targets, box_utils.get_points_in_rotated_box),
// per sample b: gt (G, 7) fp32 [x, y, z, dx, dy, dz, yaw] in 'lwh' order, G <= 128 slots of which the ones with mask == 1 are valid,
// compacted in slot order as `gt_box_center[mask == 1]` does.
//   corners     0 .. 3 of boxes_to_corners_3d(order = 'lwh') in separately rounded fp32, as the reference's torch fp32 chain makes
//               them (box_footprint_corner of detect_targets.hpp, the function cobevt_boxes_standup uses); cos / sin of the yaw are
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
//
// Decode (post_process / reg_map_to_bbx_corners / boxes2d_to_corners2d / project_points_by_matrix_torch), one thread per pixel of
// every cav: prob = sigmoid(cls) in fp32; a pixel is a candidate when prob > score_threshold and all its decoded values are finite.
//   fp64        reg * std + mean (the reference multiplies an fp32 map by float64 arrays: promoted), atan2, exp, the centre
//               (float)(L1 + i * res * rate) + x (torch.arange(dtype = float32) rounds the grid to fp32), the template times the sizes
//   fp32        rotate_points_along_z_2d casts points and rotation matrix to fp32: the half sizes and the fp64 cos / sin are
//               rounded to fp32 and the rotation is separately rounded fp32 products and sums; `corners2d += centre` adds the fp64
//               centre to the fp32 tensor in place: one fp64 add rounded to fp32; the projection by the cav's matrix is the fp32
//               chain of det_corners with z = 0
//   kept fp64   nothing beyond the reference: cos / sin are evaluated in fp64 and rounded, exactly where the reference's `.float()` is
// The candidate key is detect_post.hip's: (ordered score bits << 32) | ~global pixel index, cav 0's pixels in (i, j) order first.
#pragma once
#include "common.hpp"

namespace cobevt {

// ---------------------------------------------------------------------------------------------- decode
// corners of global pixel g -> co[k * 3 + {0, 1, 2}] for k = 0 .. 3 (z = 0), zeros for k = 4 .. 7; false when a value is not finite
__device__ __forceinline__ bool bev_decode(const DetSrc& s, int g, float* co) {
#pragma clang fp contract(off)
    const int c = det_cav_of(s, g), p = g - s.start[c];
    const int ly = s.W[c];
    const int i = p / ly, j = p - i * ly;
    const long plane = (long)s.H[c] * ly;
    const float* __restrict__ r = s.rm[c] + p;
    double v[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = (double)r[k * plane] * s.bev_std[k] + s.bev_mean[k];
    const double yaw = atan2(v[1], v[0]);
    const double dx = exp(v[4]), dy = exp(v[5]);
    const double cell = s.bev_res * s.bev_rate;
    const double cx = (double)(float)(s.bev_x0 + (double)i * cell) + v[2];
    const double cy = (double)(float)(s.bev_y0 + (double)j * cell) + v[3];
    const float sx = (float)(dx * 0.5), sy = (float)(dy * 0.5);
    const float cs = (float)cos(yaw), sn = (float)sin(yaw);
    const float* __restrict__ T = s.matrices + 16 * c;
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float x = k < 2 ? sx : -sx, y = (k == 1 || k == 2) ? sy : -sy;
        const float rx = add(mul(x, cs), mul(y, -sn)), ry = add(mul(x, sn), mul(y, cs));
        const float X = (float)((double)rx + cx), Y = (float)((double)ry + cy);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const float o = add(add(add(mul(T[4 * q], X), mul(T[4 * q + 1], Y)), mul(T[4 * q + 2], 0.f)), T[4 * q + 3]);
            finite = finite && isfinite(o);
            co[k * 3 + q] = o;
        }
        co[k * 3 + 2] = 0.f;
    }
#pragma unroll
    for (int q = 12; q < 24; ++q) co[q] = 0.f;
    return finite;
}

__global__ __launch_bounds__(256) void bev_decode_kernel(DetSrc s, DetWs ws, int total) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int c = det_cav_of(s, g);
    const float logit = s.psm[c][g - s.start[c]];
    const float score = __fdiv_rn(1.f, add(1.f, expf(-logit)));
    bool keep = score > s.score_threshold;           // false for a NaN score
    if (keep) {
        float co[24];
        keep = bev_decode(s, g, co);
    }
    if (keep) {
        const unsigned long long key = ((unsigned long long)ordered_bits(score) << 32) | (unsigned)~(unsigned)g;
        const int slot = atomicAdd(&ws.counters[0], 1);
        if (slot < total) ws.cand[slot] = key;       // slot < total always: one append per pixel at most
    }
}

// ---------------------------------------------------------------------------------------------- labels
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

// params: [L1, W1, res, downsample_rate, target_mean (6), target_std_dev (6)]
static bool bev_params_ok(const double* q) {
    for (int k = 0; k < 16; ++k)
        if (!(q[k] == q[k]) || q[k] - q[k] != 0.0) return false;                    // finite
    if (!(q[2] > 0.0) || !(q[3] > 0.0)) return false;
    for (int k = 10; k < 16; ++k)
        if (q[k] == 0.0) return false;
    return true;
}

}  // namespace cobevt
