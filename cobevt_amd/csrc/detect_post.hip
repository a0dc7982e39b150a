// LiDAR detection output (gfx950): OpenCOOD's VoxelPostprocessor.post_process behind a PointPillar head - box decode, the box filters,
// the cut at the 1000 best-scored candidates, rotated NMS and the range mask - plus delta_to_boxes3d and a pairwise rotated IoU.
// psm (1, A, H, W) / rm (1, 7A, H, W) NCHW fp32 and anchors (H, W, A, 7) of up to 16 agents ("cavs"), one 4 x 4 matrix each ->
// boxes (1000, 8, 3), scores (1000), index (1000) int32 (the global anchor index: cav c's anchors start at the sum of the earlier
// cavs' H W A, inside a cav in (h, w, a) order) and count (1), in pick order; rows at and past count are zero.
//
// Semantics (voxel_postprocessor.py post_process, box_utils.py):
//   score = sigmoid(psm); box = delta_to_boxes3d; the 8 corners as boxes_to_corners_3d builds them, projected by the cav's matrix;
//   a candidate survives when score > score_threshold, x extent <= 6, y extent <= 6, y extent != 0 (remove_large_pred_bbx computes its
//   z_len from the y column and uses it as a truth value: mirrored), min z >= -3 and max z <= 1; of the survivors of all cavs the 1000
//   with the highest scores enter NMS (equal scores: lower global index first - OUR rule, numpy's argsort leaves ties unspecified);
//   greedy NMS on the rotated IoU of corners 0..3 in xy, `iou > nms_thresh` compared in fp32 as the reference's float32 array does;
//   the picked boxes whose 8 corners all have x in [-140, 140] and y in [-40, 40] (GT_RANGE) are written - after suppression, so an
//   out-of-range box still suppresses.
//
// Deterministic parallel form - fp32 and integer data, fp64 only inside the clip; nothing depends on the order in which workgroups or
// atomics complete:
//   1 (memset)   the candidate counter <- 0
//   2 decode     one thread per anchor: the filters; a survivor appends its 64-bit key - (order-preserving score bits << 32) |
//                ~global index, so keys are unique - to the candidate list at atomicAdd(counter, 1): the ORDER of the list is
//                arbitrary, its content is a set, and there is no cap on it (the list holds one slot per anchor)
//   3 select     one workgroup: an 8 x 8-bit radix select over the list finds the 1000th largest key (LDS integer histogram), the
//                keys at or above it are gathered (again a set) and sorted descending by a bitonic network in LDS; thread t then
//                re-decodes the corners of its candidate (same device function, explicitly rounded operations: same bits)
//   4 mask       one pair (i, j) per lane, quad against quad in fp64 (Sutherland-Hodgman, at most 8 vertices, fixed storage, every
//                loop of the clip with a compile-time bound); the wave's 64-bit ballot is word j / 64 of row i: iou > thresh, j > i
//   5 greedy     one workgroup of 16 waves: wave c holds rows 64 c .. 64 c + 63 of the mask in registers (one row per lane); the waves
//                take turns: a wave walks its rows against word c of the removed set with wave-uniform reads, then ORs the other
//                words of its picked rows into the set in LDS by a butterfly over the lanes; then the range mask, a scan over the
//                picked flags and the ordered write, zeros past count
// No floating-point atomics, no workgroup waits on another, no host read-back, no allocation: the workspace comes from the caller
// (cobevt_detect_scratch).  The same select / mask / greedy launches serve cobevt_nms_rotated (boxes and scores given, no filters)
// and cobevt_bev_post (bev mode: per-pixel cls / reg maps, its own decode launch, (1000, 4, 2) quads out).
#include "common.hpp"
#include "detect_common.hpp"           // bev_params_ok, shared with bev_labels.hip

namespace cobevt {

constexpr int kDetTop = 1000;                       // box_utils.nms_rotated's `top`
constexpr int kDetWords = 16;                       // 64-bit words of a mask row: 1024 bits
constexpr int kDetMaxCav = 16;

struct DetSrc {
    // cav mode (boxes == nullptr)
    const float* psm[kDetMaxCav];
    const float* rm[kDetMaxCav];
    const float* anchors[kDetMaxCav];
    int H[kDetMaxCav], W[kDetMaxCav], A[kDetMaxCav];
    int start[kDetMaxCav + 1];                       // first global anchor index of each cav; start[ncav] = all anchors
    const float* matrices;                           // (ncav, 4, 4) on the device
    int ncav, hwl;
    float score_threshold;
    // box mode: boxes (N, box_floats / dim, dim) with dim = 3 (8 corners) or 2 (4 corners), scores (N)
    const float* boxes;
    const float* scores;
    int box_floats, n_boxes;
    // bev mode (bev != 0, cobevt_bev_post): psm = cls (1, 1, H, W), rm = reg (1, 6, H, W), A = 1; the map geometry and the
    // regression statistics of LidarBevPostprocessor
    int bev;
    double bev_x0, bev_y0, bev_res, bev_rate, bev_mean[6], bev_std[6];
};

// the workspace: the candidate keys (one slot per anchor), the sorted top candidates' corners / scores / indices, the mask, and two
// counters (candidates appended, candidates that enter NMS)
struct DetWs {
    unsigned long long* cand;
    unsigned long long* mask;
    float* sbox;
    float* sscore;
    int* sidx;
    int* counters;
};
static long det_ws_bytes(long total) {
    return 8 * total + 8L * kDetTop * kDetWords + 4L * kDetTop * 24 + 4L * kDetTop + 4L * kDetTop + 16;
}
static DetWs det_ws(void* w, long total) {
    DetWs s;
    s.cand = (unsigned long long*)w;
    s.mask = s.cand + total;
    s.sbox = (float*)(s.mask + (long)kDetTop * kDetWords);
    s.sscore = s.sbox + (long)kDetTop * 24;
    s.sidx = (int*)(s.sscore + kDetTop);
    s.counters = s.sidx + kDetTop;
    return s;
}

// float bits -> unsigned that orders like the float (positive floats already do; the flip covers a caller's negative scores)
__device__ __forceinline__ unsigned ordered_bits(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_float(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// every product and sum below is a separately rounded fp32 operation, as the reference's chain of torch ops is: no contraction into
// fused multiply-adds, so the two places that decode a box (launches 2 and 3) produce the same bits
__device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }

// delta_to_boxes3d for anchor i (in (h, w, a) order) of one sample: rm = that sample's (7A, H, W) planes
__device__ __forceinline__ void det_box(const float* __restrict__ rm, const float* __restrict__ anchors, int H, int W, int A, int i,
                                        float* b) {
    const int a = i % A, hw = i / A;
    const long plane = (long)H * W;
    const float* d = rm + (long)a * 7 * plane + hw;
    const float* an = anchors + (long)i * 7;
    const float diag = __fsqrt_rn(add(mul(an[4], an[4]), mul(an[5], an[5])));
    b[0] = add(mul(d[0], diag), an[0]);
    b[1] = add(mul(d[plane], diag), an[1]);
    b[2] = add(mul(d[2 * plane], an[3]), an[2]);
    b[3] = mul(expf(d[3 * plane]), an[3]);
    b[4] = mul(expf(d[4 * plane]), an[4]);
    b[5] = mul(expf(d[5 * plane]), an[5]);
    b[6] = add(d[6 * plane], an[6]);
}

// boxes_to_corners_3d + project_box3d: c[k * 3 + {0, 1, 2}], k = 0 .. 7 in the reference's corner order
__device__ __forceinline__ void det_corners(const float* b, int hwl, const float* __restrict__ T, float* c) {
    // 'hwl' reads the size columns as [5, 4, 3]; any other order as they stand
    const float sx = mul(hwl ? b[5] : b[3], 0.5f), sy = mul(b[4], 0.5f), sz = mul(hwl ? b[3] : b[5], 0.5f);
    const float cs = cosf(b[6]), sn = sinf(b[6]);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        // the template [1,-1,-1] [1,1,-1] [-1,1,-1] [-1,-1,-1] [1,-1,1] [1,1,1] [-1,1,1] [-1,-1,1] / 2
        const float x = (k & 3) < 2 ? sx : -sx, y = ((k & 3) == 1 || (k & 3) == 2) ? sy : -sy, z = k < 4 ? -sz : sz;
        // rotate_points_along_z: [x y z] [[cos, sin, 0], [-sin, cos, 0], [0, 0, 1]], then the centre
        const float X = add(add(mul(x, cs), mul(y, -sn)), b[0]);
        const float Y = add(add(mul(x, sn), mul(y, cs)), b[1]);
        const float Z = add(z, b[2]);
#pragma unroll
        for (int r = 0; r < 3; ++r)
            c[k * 3 + r] = add(add(add(mul(T[4 * r], X), mul(T[4 * r + 1], Y)), mul(T[4 * r + 2], Z)), T[4 * r + 3]);
    }
}

__device__ __forceinline__ int det_cav_of(const DetSrc& s, int g) {
    int c = 0;
#pragma unroll
    for (int k = 1; k < kDetMaxCav; ++k)
        if (k < s.ncav && g >= s.start[k]) c = k;
    return c;
}

// ---------------------------------------------------------------------------------------------- bev mode: the decode
// PIXOR-style per-pixel maps (LidarBevPostprocessor.post_process / reg_map_to_bbx_corners / boxes2d_to_corners2d /
// project_points_by_matrix_torch; the labels of the same maps are bev_labels.hip), one thread per pixel of every cav: prob =
// sigmoid(cls) in fp32; a pixel is a candidate when prob > score_threshold and all its decoded values are finite.
//   fp64        reg * std + mean (the reference multiplies an fp32 map by float64 arrays: promoted), atan2, exp, the centre
//               (float)(L1 + i * res * rate) + x (torch.arange(dtype = float32) rounds the grid to fp32), the template times the sizes
//   fp32        rotate_points_along_z_2d casts points and rotation matrix to fp32: the half sizes and the fp64 cos / sin are
//               rounded to fp32 and the rotation is separately rounded fp32 products and sums; `corners2d += centre` adds the fp64
//               centre to the fp32 tensor in place: one fp64 add rounded to fp32; the projection by the cav's matrix is the fp32
//               chain of det_corners with z = 0
//   kept fp64   nothing beyond the reference: cos / sin are evaluated in fp64 and rounded, exactly where the reference's `.float()` is
// The candidate key is the cav mode's: (ordered score bits << 32) | ~global pixel index, cav 0's pixels in (i, j) order first.
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

// ---------------------------------------------------------------------------------------------- decode, select
__device__ __forceinline__ void det_decode(const DetSrc& s, int g, float* corners) {
    if (s.bev) {                                     // uniform: the same bits as the bev decode launch (same function)
        bev_decode(s, g, corners);
        return;
    }
    const int c = det_cav_of(s, g);
    float b[7];
    det_box(s.rm[c], s.anchors[c], s.H[c], s.W[c], s.A[c], g - s.start[c], b);
    det_corners(b, s.hwl, s.matrices + 16 * c, corners);
}

__global__ __launch_bounds__(256) void det_decode_kernel(DetSrc s, DetWs ws, int total) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    float score;
    bool keep;
    if (s.boxes) {                                   // box mode: every box is a candidate
        score = s.scores[g];
        keep = true;
    } else {
        const int c = det_cav_of(s, g), i = g - s.start[c];
        const int a = i % s.A[c], hw = i / s.A[c];
        const float logit = s.psm[c][(long)a * s.H[c] * s.W[c] + hw];
        score = __fdiv_rn(1.f, add(1.f, expf(-logit)));
        keep = score > s.score_threshold;
        if (keep) {
            float co[24];
            det_decode(s, g, co);
            float lo[3], hi[3];
            bool finite = true;
#pragma unroll
            for (int r = 0; r < 3; ++r) { lo[r] = co[r]; hi[r] = co[r]; }
#pragma unroll
            for (int k = 0; k < 8; ++k)
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const float v = co[k * 3 + r];
                    finite = finite && isfinite(v);          // torch.max / min carry a NaN into a false comparison: dropped
                    lo[r] = fminf(lo[r], v); hi[r] = fmaxf(hi[r], v);
                }
            const float x_len = __fsub_rn(hi[0], lo[0]), y_len = __fsub_rn(hi[1], lo[1]);
            // remove_large_pred_bbx: its z_len is (max - min) of the Y column, used as a truth value - so "y extent != 0"
            const float z_len = y_len;
            keep = finite && x_len <= 6.f && y_len <= 6.f && z_len != 0.f && lo[2] >= -3.f && hi[2] <= 1.f;
        }
    }
    if (keep) {
        const unsigned long long key = ((unsigned long long)ordered_bits(score) << 32) | (unsigned)~(unsigned)g;
        const int slot = atomicAdd(&ws.counters[0], 1);
        if (slot < total) ws.cand[slot] = key;       // slot < total always: one append per anchor at most
    }
}

__global__ __launch_bounds__(1024) void det_select_kernel(DetSrc s, DetWs ws, int total) {
    __shared__ unsigned long long skey[1024];
    __shared__ int hist[256];
    __shared__ int s_digit, s_need, s_fill, wpart[4];
    const int t = threadIdx.x;
    int S = ws.counters[0];
    S = S < 0 ? 0 : (S > total ? total : S);
    unsigned long long thr = 0;                      // candidates at or above `thr` enter NMS
    if (S > kDetTop) {
        unsigned long long prefix = 0;
        int need = kDetTop;
#pragma unroll 1
        for (int shift = 56; shift >= 0; shift -= 8) {
            if (t < 256) hist[t] = 0;
            __syncthreads();
            const unsigned long long high = shift == 56 ? 0ull : (~0ull << (shift + 8));
            for (int i = t; i < S; i += 1024) {
                const unsigned long long k = ws.cand[i];
                if ((k & high) == prefix) atomicAdd(&hist[(int)(k >> shift) & 255], 1);
            }
            __syncthreads();
            // thread t < 256 takes digit 255 - t: the inclusive scan over t counts the keys whose digit is at least that one
            const int v = t < 256 ? hist[255 - t] : 0;
            int inc = v;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int x = __shfl_up(inc, o, 64);
                if ((t & 63) >= o) inc += x;
            }
            if (t < 256 && (t & 63) == 63) wpart[t >> 6] = inc;
            __syncthreads();
            if (t < 256) {
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (k < (t >> 6)) inc += wpart[k];
                if (inc - v < need && need <= inc) { s_digit = 255 - t; s_need = need - (inc - v); }
            }
            __syncthreads();
            prefix |= (unsigned long long)s_digit << shift;
            need = s_need;
        }
        thr = prefix;                                // keys are unique: exactly 1000 of them are >= the 1000th largest
    }
    if (t == 0) s_fill = 0;
    skey[t] = 0;
    __syncthreads();
    for (int i = t; i < S; i += 1024) {
        const unsigned long long k = ws.cand[i];
        if (k >= thr) {
            const int p = atomicAdd(&s_fill, 1);
            if (p < 1024) skey[p] = k;
        }
    }
    // descending bitonic sort of the 1024 slots (empty slots are 0, below every key)
    for (int k = 2; k <= 1024; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            const int o = t ^ j;
            if (o > t) {
                const unsigned long long a = skey[t], b = skey[o];
                if (((t & k) == 0) ? a < b : a > b) { skey[t] = b; skey[o] = a; }
            }
        }
    __syncthreads();
    const int K = S < kDetTop ? S : kDetTop;
    if (t == 0) ws.counters[1] = K;
    if (t >= K) return;
    const unsigned long long key = skey[t];
    const int g = (int)~(unsigned)key;
    float co[24];
    if (s.boxes) {
        const float* b = s.boxes + (long)g * s.box_floats;
        if (s.box_floats == 24) {
#pragma unroll
            for (int q = 0; q < 24; ++q) co[q] = b[q];
        } else {                                     // (N, 4, 2): corners 0 .. 3 in xy
#pragma unroll
            for (int q = 0; q < 24; ++q) co[q] = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) { co[k * 3] = b[2 * k]; co[k * 3 + 1] = b[2 * k + 1]; }
        }
    } else {
        det_decode(s, g, co);
    }
#pragma unroll
    for (int q = 0; q < 24; ++q) ws.sbox[t * 24 + q] = co[q];
    ws.sscore[t] = ordered_float((unsigned)(key >> 32));
    ws.sidx[t] = g;
}

// ---------------------------------------------------------------------------------------------- rotated IoU
// signed shoelace area of a quad
__device__ __forceinline__ double quad_signed_area(const double* x, const double* y) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) s += x[k] * y[(k + 1) & 3] - x[(k + 1) & 3] * y[k];
    return 0.5 * s;
}
__device__ __forceinline__ void put8(double* qx, double* qy, int m, double x, double y) {
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (k == m) { qx[k] = x; qy[k] = y; }
}

// IoU of two convex quads given as fp32 corners (stride floats apart, x then y), computed in fp64: Sutherland-Hodgman of a against
// the four edges of b, both wound counter-clockwise first (a projection may flip the winding).  Degenerate (zero union) -> 0.
__device__ double quad_iou(const float* __restrict__ a, int sa, const float* __restrict__ b, int sb) {
    double ax[4], ay[4], bx[4], by[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { ax[k] = a[k * sa]; ay[k] = a[k * sa + 1]; bx[k] = b[k * sb]; by[k] = b[k * sb + 1]; }
    double area_a = quad_signed_area(ax, ay), area_b = quad_signed_area(bx, by);
    if (area_a < 0.0) { double t = ax[1]; ax[1] = ax[3]; ax[3] = t; t = ay[1]; ay[1] = ay[3]; ay[3] = t; area_a = -area_a; }
    if (area_b < 0.0) { double t = bx[1]; bx[1] = bx[3]; bx[3] = t; t = by[1]; by[1] = by[3]; by[3] = t; area_b = -area_b; }
    double inter = 0.0;
    const double axl = fmin(fmin(ax[0], ax[1]), fmin(ax[2], ax[3])), axh = fmax(fmax(ax[0], ax[1]), fmax(ax[2], ax[3]));
    const double ayl = fmin(fmin(ay[0], ay[1]), fmin(ay[2], ay[3])), ayh = fmax(fmax(ay[0], ay[1]), fmax(ay[2], ay[3]));
    const double bxl = fmin(fmin(bx[0], bx[1]), fmin(bx[2], bx[3])), bxh = fmax(fmax(bx[0], bx[1]), fmax(bx[2], bx[3]));
    const double byl = fmin(fmin(by[0], by[1]), fmin(by[2], by[3])), byh = fmax(fmax(by[0], by[1]), fmax(by[2], by[3]));
    if (axl < bxh && bxl < axh && ayl < byh && byl < ayh) {            // bounding boxes overlap: clip
        double px[8], py[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { px[k] = k < 4 ? ax[k] : 0.0; py[k] = k < 4 ? ay[k] : 0.0; }
        int n = 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double ex = bx[e], ey = by[e], fx = bx[(e + 1) & 3] - ex, fy = by[(e + 1) & 3] - ey;
            double qx[8], qy[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) { qx[k] = 0.0; qy[k] = 0.0; }
            // start from the last vertex; side > = 0: inside (left of the edge)
            double prx = px[0], pry = py[0];
#pragma unroll
            for (int k = 1; k < 8; ++k)
                if (k == n - 1) { prx = px[k]; pry = py[k]; }
            double dp = fx * (pry - ey) - fy * (prx - ex);
            int m = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k < n) {
                    const double cx = px[k], cy = py[k];
                    const double dc = fx * (cy - ey) - fy * (cx - ex);
                    if ((dc >= 0.0) != (dp >= 0.0)) {
                        const double u = dp / (dp - dc);
                        put8(qx, qy, m, prx + u * (cx - prx), pry + u * (cy - pry));
                        ++m;
                    }
                    if (dc >= 0.0) { put8(qx, qy, m, cx, cy); ++m; }
                    prx = cx; pry = cy; dp = dc;
                }
            }
            n = m < 8 ? m : 8;                       // a convex polygon gains at most one vertex per edge: 4 + 4
#pragma unroll
            for (int k = 0; k < 8; ++k) { px[k] = qx[k]; py[k] = qy[k]; }
        }
        // shoelace over the n vertices
        double s2 = 0.0, prx = px[0], pry = py[0];
#pragma unroll
        for (int k = 1; k < 8; ++k)
            if (k == n - 1) { prx = px[k]; pry = py[k]; }
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < n) { s2 += prx * py[k] - px[k] * pry; prx = px[k]; pry = py[k]; }
        inter = n >= 3 ? fabs(0.5 * s2) : 0.0;
    }
    const double uni = area_a + area_b - inter;
    return uni > 0.0 ? inter / uni : 0.0;
}

// block = 4 waves = 4 rows; blockIdx.x = the word of the row
__global__ __launch_bounds__(256) void det_mask_kernel(DetWs ws, float thresh) {
    const int lane = threadIdx.x & 63, w = blockIdx.x;
    const int i = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int K = __builtin_amdgcn_readfirstlane(ws.counters[1]);
    if (i >= K) return;                              // uniform over the wave
    const int j = 64 * w + lane;
    bool over = false;
    if (64 * w + 63 > i) {                           // uniform: the word has columns past i
        if (j > i && j < K) {
            // compute_iou returns a float32 array and `iou > threshold` compares in float32
            over = (float)quad_iou(ws.sbox + i * 24, 3, ws.sbox + j * 24, 3) > thresh;
        }
    }
    const unsigned long long word = __ballot(over);
    if (lane == 0) ws.mask[(long)i * kDetWords + w] = word;
}

// 1024 threads; thread t owns sorted candidate t for the load and for the write
__global__ __launch_bounds__(1024) void det_greedy_kernel(DetWs ws, float* __restrict__ boxes, float* __restrict__ scores,
                                                          int* __restrict__ index, int* __restrict__ count, int apply_range,
                                                          int quad) {
    __shared__ unsigned long long removed[kDetWords];
    __shared__ unsigned long long picked[kDetWords];
    __shared__ int wsum[16];
    const int t = threadIdx.x, lane = t & 63, c = __builtin_amdgcn_readfirstlane(t >> 6);
    const int K = __builtin_amdgcn_readfirstlane(ws.counters[1]);
    // one mask row per lane, in registers (rows at and past K: zero)
    unsigned lo[kDetWords], hi[kDetWords];
#pragma unroll
    for (int w = 0; w < kDetWords; ++w) {
        const unsigned long long v = t < K ? ws.mask[(long)t * kDetWords + w] : 0ull;
        lo[w] = (unsigned)v; hi[w] = (unsigned)(v >> 32);
    }
    if (t < kDetWords) { removed[t] = 0ull; picked[t] = 0ull; }
    __syncthreads();
#pragma unroll 1
    for (int turn = 0; turn < 16; ++turn) {
        if (c == turn && 64 * c < K) {               // uniform over the wave
            // only word c of a row decides inside this wave's 64 rows: the walk keeps that word of the removed set in scalar
            // registers and reads word c of a picked row from its lane; the other words are ORed in once, after the walk
            const unsigned long long mine0 = removed[c];
            unsigned mlo = __builtin_amdgcn_readfirstlane((unsigned)mine0), mhi = __builtin_amdgcn_readfirstlane((unsigned)(mine0 >> 32));
            unsigned mylo = lo[0], myhi = hi[0];
#pragma unroll
            for (int w = 1; w < kDetWords; ++w)
                if (w == c) { mylo = lo[w]; myhi = hi[w]; }
            unsigned long long pick = 0ull;
            const int rows = K - 64 * c < 64 ? K - 64 * c : 64;
#pragma unroll 1
            for (int l = 0; l < rows; ++l) {
                const unsigned long long mine = ((unsigned long long)mhi << 32) | mlo;
                if (!((mine >> l) & 1ull)) {         // uniform: `mine` only holds wave-uniform values
                    pick |= 1ull << l;
                    mlo |= (unsigned)__builtin_amdgcn_readlane((int)mylo, l);
                    mhi |= (unsigned)__builtin_amdgcn_readlane((int)myhi, l);
                }
            }
            const bool me = (pick >> lane) & 1ull;
#pragma unroll
            for (int w = 0; w < kDetWords; ++w) {
                if (w < c) continue;                 // uniform; a row has no bits at or before its own column
                unsigned a = me ? lo[w] : 0u, b = me ? hi[w] : 0u;
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) { a |= __shfl_xor(a, o, 64); b |= __shfl_xor(b, o, 64); }
                if (lane == 0) removed[w] |= ((unsigned long long)b << 32) | a;
            }
            if (lane == 0) picked[c] = pick;
        }
        __syncthreads();
    }
    // the range mask (get_mask_for_boxes_within_range_torch, GT_RANGE) on the picked boxes, then the ordered write
    float co[24];
    bool keep = false;
    if (t < K) {
#pragma unroll
        for (int q = 0; q < 24; ++q) co[q] = ws.sbox[t * 24 + q];
        keep = (picked[c] >> lane) & 1ull;
        if (keep && apply_range) {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                keep = keep && co[k * 3] >= -140.f && co[k * 3] <= 140.f && co[k * 3 + 1] >= -40.f && co[k * 3 + 1] <= 40.f;
        }
    }
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) wsum[c] = __popcll(bal);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int v = wsum[k];
        if (k < c) before += v;
        all += v;
    }
    const int pos = before + __popcll(bal & ((1ull << lane) - 1ull));
    // quad (uniform): boxes is (1000, 4, 2), corners 0 .. 3 in xy; otherwise (1000, 8, 3)
    if (keep) {
        if (quad) {
#pragma unroll
            for (int k = 0; k < 4; ++k) { boxes[pos * 8 + 2 * k] = co[k * 3]; boxes[pos * 8 + 2 * k + 1] = co[k * 3 + 1]; }
        } else {
#pragma unroll
            for (int q = 0; q < 24; ++q) boxes[pos * 24 + q] = co[q];
        }
        scores[pos] = ws.sscore[t];
        index[pos] = ws.sidx[t];
    }
    if (t >= all && t < kDetTop) {                   // rows at and past count: zero
        if (quad) {
#pragma unroll
            for (int q = 0; q < 8; ++q) boxes[t * 8 + q] = 0.f;
        } else {
#pragma unroll
            for (int q = 0; q < 24; ++q) boxes[t * 24 + q] = 0.f;
        }
        scores[t] = 0.f;
        index[t] = 0;
    }
    if (t == 0) count[0] = all;
}

// ---------------------------------------------------------------------------------------------- the two public maps
__global__ __launch_bounds__(256) void det_boxes3d_kernel(const float* __restrict__ rm, const float* __restrict__ anchors,
                                                          float* __restrict__ out, int N, int H, int W, int A) {
    const long per = (long)H * W * A;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= per * N) return;
    const int n = (int)(i / per);
    float b[7];
    det_box(rm + (long)n * 7 * per, anchors, H, W, A, (int)(i - n * per), b);
#pragma unroll
    for (int q = 0; q < 7; ++q) out[i * 7 + q] = b[q];
}

__global__ __launch_bounds__(256) void det_pair_iou_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           double* __restrict__ out, int N, int M) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)N * M) return;
    out[i] = quad_iou(a + (i / M) * 8, 2, b + (i % M) * 8, 2);
}

static int det_launch_nms(const DetSrc& s, const DetWs& ws, int total, float nms_thresh, float* boxes, float* scores, int* index,
                          int* count, int apply_range, int quad, hipStream_t stream) {
    if (hipMemsetAsync(ws.counters, 0, 8, stream) != hipSuccess) return COBEVT_ERR_LAUNCH;
    if (total > 0 && s.bev)
        hipLaunchKernelGGL(bev_decode_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, s, ws, total);
    else if (total > 0)
        hipLaunchKernelGGL(det_decode_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, s, ws, total);
    hipLaunchKernelGGL(det_select_kernel, dim3(1), dim3(1024), 0, stream, s, ws, total);
    hipLaunchKernelGGL(det_mask_kernel, dim3(kDetWords, (kDetTop + 3) / 4), dim3(256), 0, stream, ws, nms_thresh);
    hipLaunchKernelGGL(det_greedy_kernel, dim3(1), dim3(1024), 0, stream, ws, boxes, scores, index, count, apply_range,
                       quad);
    return cobevt::launch_status();
}

}  // namespace cobevt

using namespace cobevt;

extern "C" int cobevt_detect_scratch(long total_anchors, long* workspace_bytes) {
    if (!workspace_bytes) return COBEVT_ERR_ARG;
    if (total_anchors < 0 || total_anchors > 0x7fffffffL - 1024) return COBEVT_ERR_SHAPE;
    *workspace_bytes = det_ws_bytes(total_anchors);
    return COBEVT_OK;
}

extern "C" int cobevt_detect_post(const float* const* psm, const float* const* rm, const float* const* anchors,
                                  const float* matrices, const int* cav_dims, int ncav, int hwl, float score_threshold,
                                  float nms_thresh, float* boxes, float* scores, int* index, int* count, void* workspace,
                                  hipStream_t stream) {
    if (!psm || !rm || !anchors || !matrices || !cav_dims || !boxes || !scores || !index || !count || !workspace) return COBEVT_ERR_ARG;
    if (ncav < 1 || ncav > kDetMaxCav) return COBEVT_ERR_SHAPE;
    if ((uintptr_t)workspace & 7) return COBEVT_ERR_SHAPE;
    DetSrc s = {};
    long total = 0;
    for (int c = 0; c < ncav; ++c) {
        const long H = cav_dims[3 * c], W = cav_dims[3 * c + 1], A = cav_dims[3 * c + 2];
        if (!psm[c] || !rm[c] || !anchors[c]) return COBEVT_ERR_ARG;
        if (H < 1 || W < 1 || A < 1 || H > 0x7fffffffL / W || H * W > (0x7fffffffL / 8) / A) return COBEVT_ERR_SHAPE;
        s.psm[c] = psm[c]; s.rm[c] = rm[c]; s.anchors[c] = anchors[c];
        s.H[c] = (int)H; s.W[c] = (int)W; s.A[c] = (int)A;
        s.start[c] = (int)total;
        total += H * W * A;
        if (total > 0x7fffffffL / 8) return COBEVT_ERR_SHAPE;
    }
    for (int c = ncav; c <= kDetMaxCav; ++c) s.start[c] = (int)total;
    s.matrices = matrices; s.ncav = ncav; s.hwl = hwl != 0; s.score_threshold = score_threshold;
    return det_launch_nms(s, det_ws(workspace, total), (int)total, nms_thresh, boxes, scores, index, count, 1, 0, stream);
}

extern "C" int cobevt_nms_rotated(const float* box_corners, const float* box_scores, long N, int corner_floats, float nms_thresh,
                                  float* boxes, float* scores, int* index, int* count, void* workspace, hipStream_t stream) {
    if (!boxes || !scores || !index || !count || !workspace) return COBEVT_ERR_ARG;
    if (N < 0 || N > 0x7fffffffL / 32 || (corner_floats != 24 && corner_floats != 8)) return COBEVT_ERR_SHAPE;
    if (N > 0 && (!box_corners || !box_scores)) return COBEVT_ERR_ARG;
    if ((uintptr_t)workspace & 7) return COBEVT_ERR_SHAPE;
    DetSrc s = {};
    // N = 0: the decode launch is skipped and nothing reads the pointer; it only has to select box mode
    s.boxes = box_corners ? box_corners : (const float*)workspace;
    s.scores = box_scores; s.box_floats = corner_floats; s.n_boxes = (int)N;
    return det_launch_nms(s, det_ws(workspace, N), (int)N, nms_thresh, boxes, scores, index, count, 0, 0, stream);
}

extern "C" int cobevt_delta_to_boxes3d(const float* rm, const float* anchors, float* boxes3d, int N, int H, int W, int A,
                                       hipStream_t stream) {
    if (!rm || !anchors || !boxes3d) return COBEVT_ERR_ARG;
    if (N < 1 || H < 1 || W < 1 || A < 1 || (long)H > 0x7fffffffL / W || (long)H * W > (0x7fffffffL / 8) / A
        || (long)H * W * A > (0x7fffffffL / 8) / N)
        return COBEVT_ERR_SHAPE;
    const long n = (long)N * H * W * A;
    hipLaunchKernelGGL(det_boxes3d_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, rm, anchors, boxes3d, N, H, W, A);
    return cobevt::launch_status();
}

extern "C" int cobevt_rotated_iou(const float* a, const float* b, double* iou, long N, long M, hipStream_t stream) {
    if (N < 0 || M < 0 || (N > 0 && M > 0x7fffffffL / N)) return COBEVT_ERR_SHAPE;
    if (N == 0 || M == 0) return COBEVT_OK;
    if (!a || !b || !iou) return COBEVT_ERR_ARG;
    hipLaunchKernelGGL(det_pair_iou_kernel, dim3((unsigned)((N * M + 255) / 256)), dim3(256), 0, stream, a, b, iou, (int)N, (int)M);
    return cobevt::launch_status();
}

extern "C" int cobevt_bev_post(const float* const* cls, const float* const* reg, const float* matrices, const int* cav_dims, int ncav,
                               const double* params, float score_threshold, float nms_thresh, float* boxes, float* scores, int* index,
                               int* count, void* workspace, hipStream_t stream) {
    if (!cls || !reg || !matrices || !cav_dims || !params || !boxes || !scores || !index || !count || !workspace) return COBEVT_ERR_ARG;
    if (ncav < 1 || ncav > kDetMaxCav) return COBEVT_ERR_SHAPE;
    if ((uintptr_t)workspace & 7) return COBEVT_ERR_SHAPE;
    if (!bev_params_ok(params)) return COBEVT_ERR_SHAPE;
    DetSrc s = {};
    long total = 0;
    for (int c = 0; c < ncav; ++c) {
        const long H = cav_dims[2 * c], W = cav_dims[2 * c + 1];
        if (!cls[c] || !reg[c]) return COBEVT_ERR_ARG;
        if (H < 1 || W < 1 || H > 0x7fffffffL / W || H * W > 0x7fffffffL / 8) return COBEVT_ERR_SHAPE;
        s.psm[c] = cls[c]; s.rm[c] = reg[c];
        s.H[c] = (int)H; s.W[c] = (int)W; s.A[c] = 1;
        s.start[c] = (int)total;
        total += H * W;
        if (total > 0x7fffffffL / 8) return COBEVT_ERR_SHAPE;
    }
    for (int c = ncav; c <= kDetMaxCav; ++c) s.start[c] = (int)total;
    s.matrices = matrices; s.ncav = ncav; s.score_threshold = score_threshold;
    s.bev = 1; s.bev_x0 = params[0]; s.bev_y0 = params[1]; s.bev_res = params[2]; s.bev_rate = params[3];
    for (int k = 0; k < 6; ++k) { s.bev_mean[k] = params[4 + k]; s.bev_std[k] = params[10 + k]; }
    return det_launch_nms(s, det_ws(workspace, total), (int)total, nms_thresh, boxes, scores, index, count, 1, 1, stream);
}
