// LiDAR detection TARGETS and LOSS (gfx950), the training side of detect_post.hip: OpenCOOD's VoxelPostprocessor.generate_label - the
// anchor-to-ground-truth assignment with the `bbox_overlaps` it needs - and the PointPillar detection loss with its gradient.
//
// Targets (voxel_postprocessor.py generate_label, box_utils.py, box_overlaps.pyx), per sample b of a batch, M = H W A anchors in
// (h, w, a) order, G <= 128 ground-truth slots of which the ones with mask == 1 are valid; column k below is the k-th VALID box:
//   standup box  the axis-aligned hull [x1, y1, x2, y2] of the four rotated footprint corners (length = column 5, width = column 4)
//   iou          bbox_overlaps on the fp32 standup boxes with the `+1` convention, in the arithmetic of the compiled reference (float
//                differences, the `+ 1.0` sums, areas and union in double, see tgt_iou): one IEEE operation per written operation,
//                no contraction into fused multiply-adds, correctly rounded division - the same bits
//   highest      per valid gt the lowest anchor index among those of maximal iou (np.argmax), kept only when that iou is > 0
//   positive     any iou > pos_threshold, or a kept highest anchor; its matched gt is the lowest k with iou > pos_threshold when
//                there is one, otherwise the lowest k it is the kept highest of (np.where / concatenate / np.unique(return_index))
//   negative     every iou < neg_threshold (all anchors without a valid gt), cleared for kept highest anchors
//   targets      for positives (gx - ax) / d, (gy - ay) / d with d = sqrt(a4^2 + a5^2), (gz - az) / a3, log(g3 / a3), log(g4 / a4),
//                log(g5 / a5), g6 - a6; zero elsewhere
// Deterministic parallel form: two launches behind two memset nodes.  `best` finds the per-gt maximum across all workgroups with
// integer atomics only - atomicMax on the 64-bit key (iou bits << 32) | ~anchor index; iou > 0, so its bit pattern orders like the
// value, and the inverted index makes the lowest anchor win a tie.  `label` recomputes the same iou (same function, same bits),
// reads the finished keys and writes every element of the three maps; num_pos is an integer atomicAdd per wave.
//
// Loss (upstream OpenCOOD's PointPillarLoss), p_b = max(1, positives of sample b), t = pos_equal_one:
//   conf_loss = cls_weight / B * sum [0.25 t + 0.75 (1 - t)] pt^2 bce / p_b,  bce = max(x, 0) - x t + log1p(exp(-|x|)),
//               pt = t (1 - sigmoid(x)) + (1 - t) sigmoid(x)
//   reg_loss  = reg / B * sum over positives of smooth_l1(d_k) / p_b, beta = 1 / 9, d_k = rm_k - tgt_k (k < 6),
//               d_6 = sin(rm_6) cos(tgt_6) - cos(rm_6) sin(tgt_6); a NaN target counts as d = 0
// Per-element arithmetic fp32; sums fp64 in a fixed order (a wave butterfly, the four waves of a workgroup in order, one partial
// pair per workgroup, then one finishing workgroup over the partials): no floating-point atomics, bitwise reproducible.
#include "detect_common.hpp"           // kTgtMaxGt and box_footprint_corner, shared with bev_labels.hip

namespace cobevt {

// ---------------------------------------------------------------------------------------------- standup boxes
__global__ __launch_bounds__(256) void tgt_standup_kernel(const float* __restrict__ boxes, float* __restrict__ out, long n) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* b = boxes + i * 7;
    // boxes_to_corners_3d with order 'hwl': the size columns read as [5, 4, 3]
    const float sx = b[5] * 0.5f, sy = b[4] * 0.5f;
    const float cs = cosf(b[6]), sn = sinf(b[6]);
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float X, Y;
        box_footprint_corner(k, b[0], b[1], sx, sy, cs, sn, X, Y);
        x1 = k ? fminf(x1, X) : X; x2 = k ? fmaxf(x2, X) : X;
        y1 = k ? fminf(y1, Y) : Y; y2 = k ? fmaxf(y2, Y) : Y;
    }
    *(float4*)(out + i * 4) = make_float4(x1, y1, x2, y2);
}

// ---------------------------------------------------------------------------------------------- targets
// box_overlaps.bbox_overlaps for one pair, with the bits of the C that Cython generates from the reference's .pyx: a = the anchor's
// standup box, q = the gt's.  A difference of two coordinates is a float operation; the `+ 1` is emitted as `+ 1.0`, a double, so
// iw and ih are (float)((double)difference + 1.0), box_area is the double product of two such sums rounded to float, and the union
// is formed in double from the anchor's sums, the float box_area and the float iw * ih, then rounded to float once; the quotient
// is a float division.  One IEEE operation per written operation: no contraction, correctly rounded division.
__device__ __forceinline__ float tgt_iou(const float4 a, const float4 q) {
#pragma clang fp contract(off)
    const float iw = (float)((double)(fminf(a.z, q.z) - fmaxf(a.x, q.x)) + 1.0);
    if (!(iw > 0.f)) return 0.f;
    const float ih = (float)((double)(fminf(a.w, q.w) - fmaxf(a.y, q.y)) + 1.0);
    if (!(ih > 0.f)) return 0.f;
    const float box_area = (float)(((double)(q.z - q.x) + 1.0) * ((double)(q.w - q.y) + 1.0));
    const float inter = iw * ih;
    const float ua = (float)((((double)(a.z - a.x) + 1.0) * ((double)(a.w - a.y) + 1.0) + (double)box_area) - (double)inter);
    return __fdiv_rn(inter, ua);
}

// the valid boxes of sample b, compacted in slot order into LDS by the first G threads of the workgroup -> their number.
// s_valid: kTgtMaxGt ints; s_st: the standup boxes; s_slot: the slot each valid box came from.  Ends with a barrier.
__device__ __forceinline__ int tgt_stage(const float* __restrict__ gstand, const float* __restrict__ mask, int b, int G,
                                         int* s_valid, float4* s_st, int* s_slot) {
    const int t = threadIdx.x;
    if (t < kTgtMaxGt) s_valid[t] = (t < G && mask[(long)b * G + t] == 1.f) ? 1 : 0;
    __syncthreads();
    int n = 0, rank = 0;
    for (int j = 0; j < G; ++j) {
        const int v = s_valid[j];
        n += v;
        if (j < t) rank += v;
    }
    if (t < G && s_valid[t]) {
        s_st[rank] = *(const float4*)(gstand + ((long)b * G + t) * 4);
        s_slot[rank] = t;
    }
    __syncthreads();
    return n;
}

// grid (ceil(M / 256), B).  best (B, G) 64-bit keys, zero on entry: key k of a sample belongs to its k-th valid box
__global__ __launch_bounds__(256) void tgt_best_kernel(const float* __restrict__ astand, const float* __restrict__ gstand,
                                                       const float* __restrict__ mask, unsigned long long* __restrict__ best, int M,
                                                       int G) {
    __shared__ float4 s_st[kTgtMaxGt];
    __shared__ unsigned long long s_key[kTgtMaxGt];
    __shared__ int s_valid[kTgtMaxGt], s_slot[kTgtMaxGt];
    const int t = threadIdx.x, b = blockIdx.y;
    const long i = (long)blockIdx.x * 256 + t;
    if (t < kTgtMaxGt) s_key[t] = 0ull;
    const int n = tgt_stage(gstand, mask, b, G, s_valid, s_st, s_slot);
    if (i < M) {
        const float4 a = *(const float4*)(astand + i * 4);
        for (int k = 0; k < n; ++k) {
            const float iou = tgt_iou(a, s_st[k]);
            if (iou > 0.f) atomicMax(&s_key[k], ((unsigned long long)__float_as_uint(iou) << 32) | (unsigned)~(unsigned)i);
        }
    }
    __syncthreads();
    if (t < n && s_key[t] != 0ull) atomicMax(&best[(long)b * G + t], s_key[t]);
}

// grid (ceil(M / 256), B).  Writes every element of pos / neg (B, M) and targets (B, M, 7); num_pos (B) is zero on entry
__global__ __launch_bounds__(256) void tgt_label_kernel(const float* __restrict__ anchors, const float* __restrict__ astand,
                                                        const float* __restrict__ gt, const float* __restrict__ gstand,
                                                        const float* __restrict__ mask, const unsigned long long* __restrict__ best,
                                                        float* __restrict__ pos, float* __restrict__ neg, float* __restrict__ targets,
                                                        int* __restrict__ num_pos, int M, int G, float pos_thr, float neg_thr) {
    __shared__ float4 s_st[kTgtMaxGt];
    __shared__ int s_hi[kTgtMaxGt];
    __shared__ int s_valid[kTgtMaxGt], s_slot[kTgtMaxGt];
    const int t = threadIdx.x, b = blockIdx.y;
    const long i = (long)blockIdx.x * 256 + t;
    const int n = tgt_stage(gstand, mask, b, G, s_valid, s_st, s_slot);
    if (t < n) {
        const unsigned long long key = best[(long)b * G + t];
        s_hi[t] = key != 0ull ? (int)~(unsigned)key : -1;          // the kept highest anchor of valid box t, or none
    }
    __syncthreads();
    bool positive = false;
    if (i < M) {
        const float4 a = *(const float4*)(astand + i * 4);
        int pos_k = -1, high_k = -1;
        bool all_neg = true;
        for (int k = 0; k < n; ++k) {
            const float iou = tgt_iou(a, s_st[k]);
            if (pos_k < 0 && iou > pos_thr) pos_k = k;
            if (high_k < 0 && s_hi[k] == (int)i) high_k = k;
            all_neg = all_neg && iou < neg_thr;
        }
        positive = pos_k >= 0 || high_k >= 0;
        const long o = (long)b * M + i;
        pos[o] = positive ? 1.f : 0.f;
        neg[o] = (all_neg && high_k < 0) ? 1.f : 0.f;
        float tg[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (positive) {
            const float* g = gt + ((long)b * G + s_slot[pos_k >= 0 ? pos_k : high_k]) * 7;
            const float* an = anchors + i * 7;
            const float d = sqrtf(an[4] * an[4] + an[5] * an[5]);
            tg[0] = (g[0] - an[0]) / d;
            tg[1] = (g[1] - an[1]) / d;
            tg[2] = (g[2] - an[2]) / an[3];
            tg[3] = logf(g[3] / an[3]);
            tg[4] = logf(g[4] / an[4]);
            tg[5] = logf(g[5] / an[5]);
            tg[6] = g[6] - an[6];
        }
#pragma unroll
        for (int q = 0; q < 7; ++q) targets[o * 7 + q] = tg[q];
    }
    const unsigned long long bal = __ballot(positive);
    if ((t & 63) == 0 && bal != 0ull) atomicAdd(&num_pos[b], (int)__popcll(bal));
}

// ---------------------------------------------------------------------------------------------- loss
// sum over the 256 threads in a fixed order -> valid in thread 0: a butterfly inside each wave, then the four waves in order
__device__ __forceinline__ double ppl_block_sum(double v, double* s4) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s4[0] + s4[1]) + s4[2]) + s4[3];
}

// grid (ceil(M / 256), B): positives (pos_equal_one > 0) per sample; counts (B) zero on entry
__global__ __launch_bounds__(256) void ppl_count_kernel(const float* __restrict__ pos, int* __restrict__ counts, int M) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const bool p = i < M && pos[(long)blockIdx.y * M + i] > 0.f;
    const unsigned long long bal = __ballot(p);
    if ((threadIdx.x & 63) == 0 && bal != 0ull) atomicAdd(&counts[blockIdx.y], (int)__popcll(bal));
}

// grid (ceil(H W / 256), A, B); thread = one anchor, hw fastest (the NCHW maps are read and their gradients written coalesced).
// partial: [conf, reg] per workgroup in fp64.  dpsm / drm: both or neither; every element is written.
__global__ __launch_bounds__(256) void ppl_main_kernel(const float* __restrict__ psm, const float* __restrict__ rm,
                                                       const float* __restrict__ pos, const float* __restrict__ tgt,
                                                       const int* __restrict__ num_pos, double* __restrict__ partial,
                                                       float* __restrict__ dpsm, float* __restrict__ drm, int HW, int A,
                                                       float cls_scale, float reg_scale) {
    __shared__ double s4[4];
    const int a = blockIdx.y, b = blockIdx.z;
    const long hw = (long)blockIdx.x * 256 + threadIdx.x;
    float conf = 0.f, reg = 0.f;
    if (hw < HW) {
        const int np = num_pos[b];
        const float pb = (float)(np > 1 ? np : 1);
        const long ip = ((long)b * A + a) * HW + hw;              // psm (B, A, H, W)
        const long il = ((long)b * HW + hw) * A + a;              // labels (B, H, W, A)
        const float x = psm[ip], t = pos[il];
        const float e = expf(-fabsf(x));
        const float bce = fmaxf(x, 0.f) - x * t + log1pf(e);
        const float sig = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        const float pt = t * (1.f - sig) + (1.f - t) * sig;
        const float aw = 0.25f * t + 0.75f * (1.f - t);
        conf = aw * pt * pt * bce / pb;
        if (dpsm) {
            const float dpt = (1.f - 2.f * t) * sig * (1.f - sig);
            dpsm[ip] = aw * (2.f * pt * dpt * bce + pt * pt * (sig - t)) / pb * cls_scale;
        }
        const bool positive = t > 0.f;
        const float beta = 1.f / 9.f;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const long ir = (((long)b * A + a) * 7 + k) * HW + hw;  // rm (B, 7A, H, W), channel a * 7 + k
            float g = 0.f;
            if (positive) {
                const float p = rm[ir], q = tgt[il * 7 + k];
                float d, dd;
                if (k < 6) {
                    d = isnan(q) ? 0.f : p - q;
                    dd = isnan(q) ? 0.f : 1.f;
                } else {
                    const float sp = sinf(p), cp = cosf(p), sq = sinf(q), cq = cosf(q);
                    const bool bad = isnan(cp * sq);                // the encoded target cos(rm) sin(tgt) is what the loss tests
                    d = bad ? 0.f : sp * cq - cp * sq;
                    dd = bad ? 0.f : cp * cq + sp * sq;
                }
                const float ad = fabsf(d);
                reg += (ad < beta ? 0.5f * d * d / beta : ad - 0.5f * beta) / pb;
                g = (ad < beta ? d / beta : (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f))) * dd / pb * reg_scale;
            }
            if (drm) drm[ir] = g;
        }
    }
    const double c = ppl_block_sum((double)conf, s4);
    const double r = ppl_block_sum((double)reg, s4);
    if (threadIdx.x == 0) {
        const long blk = ((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[2 * blk] = c;
        partial[2 * blk + 1] = r;
    }
}

// one workgroup: thread t adds partials t, t + 256, ... in order, then the fixed block sum.  loss = [total, conf_loss, reg_loss]
__global__ __launch_bounds__(256) void ppl_finish_kernel(const double* __restrict__ partial, long nblk, float* __restrict__ loss,
                                                         double cls_scale, double reg_scale) {
    __shared__ double s4[4];
    double c = 0.0, r = 0.0;
    for (long i = threadIdx.x; i < nblk; i += 256) { c += partial[2 * i]; r += partial[2 * i + 1]; }
    c = ppl_block_sum(c, s4);
    r = ppl_block_sum(r, s4);
    if (threadIdx.x == 0) {
        const double conf = cls_scale * c, reg = reg_scale * r;
        loss[0] = (float)(conf + reg);
        loss[1] = (float)conf;
        loss[2] = (float)reg;
    }
}

static long ppl_blocks(long B, long HW, long A) { return ((HW + 255) / 256) * A * B; }

}  // namespace cobevt

using namespace cobevt;

extern "C" int cobevt_boxes_standup(const float* boxes, float* standup, long n, hipStream_t stream) {
    if (n < 0 || n > 0x7fffffffL / 8) return COBEVT_ERR_SHAPE;
    if (n == 0) return COBEVT_OK;
    if (!boxes || !standup) return COBEVT_ERR_ARG;
    if ((uintptr_t)standup & 15) return COBEVT_ERR_SHAPE;
    hipLaunchKernelGGL(tgt_standup_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, boxes, standup, n);
    return cobevt::launch_status();
}

extern "C" int cobevt_detect_targets(const float* anchors, const float* anchor_standup, const float* gt_boxes, const float* gt_standup,
                                     const float* mask, float pos_threshold, float neg_threshold, float* pos_equal_one,
                                     float* neg_equal_one, float* targets, int* num_pos, void* workspace, int B, int H, int W, int A,
                                     int G, hipStream_t stream) {
    if (!anchors || !anchor_standup || !pos_equal_one || !neg_equal_one || !targets || !num_pos || !workspace) return COBEVT_ERR_ARG;
    if (G < 0 || G > kTgtMaxGt) return COBEVT_ERR_SHAPE;
    if (G > 0 && (!gt_boxes || !gt_standup || !mask)) return COBEVT_ERR_ARG;
    if (B < 1 || B > 65535 || H < 1 || W < 1 || A < 1 || (long)H > 0x7fffffffL / W || (long)H * W > (0x7fffffffL / 8) / A
        || (long)H * W * A > (0x7fffffffL / 8) / B)
        return COBEVT_ERR_SHAPE;
    if (((uintptr_t)anchor_standup & 15) || ((uintptr_t)gt_standup & 15) || ((uintptr_t)workspace & 7)) return COBEVT_ERR_SHAPE;
    const int M = H * W * A;
    unsigned long long* best = (unsigned long long*)workspace;           // (B, max(G, 1)) keys
    if (hipMemsetAsync(best, 0, 8 * (size_t)B * (G > 0 ? G : 1), stream) != hipSuccess) return COBEVT_ERR_LAUNCH;
    if (hipMemsetAsync(num_pos, 0, 4 * (size_t)B, stream) != hipSuccess) return COBEVT_ERR_LAUNCH;
    const dim3 grid((unsigned)((M + 255) / 256), (unsigned)B);
    if (G > 0) hipLaunchKernelGGL(tgt_best_kernel, grid, dim3(256), 0, stream, anchor_standup, gt_standup, mask, best, M, G);
    hipLaunchKernelGGL(tgt_label_kernel, grid, dim3(256), 0, stream, anchors, anchor_standup, gt_boxes, gt_standup, mask, best,
                       pos_equal_one, neg_equal_one, targets, num_pos, M, G, pos_threshold, neg_threshold);
    return cobevt::launch_status();
}

extern "C" int cobevt_pointpillar_loss(const float* psm, const float* rm, const float* pos_equal_one, const float* targets,
                                       const int* num_pos, float* loss, float* dpsm, float* drm, void* workspace, int B, int H, int W,
                                       int A, float cls_weight, float reg, hipStream_t stream) {
    if (!psm || !rm || !pos_equal_one || !targets || !loss || !workspace || ((dpsm == nullptr) != (drm == nullptr))) return COBEVT_ERR_ARG;
    if (B < 1 || B > 65535 || A < 1 || A > 65535 || H < 1 || W < 1 || (long)H > 0x7fffffffL / W || (long)H * W > (0x7fffffffL / 8) / A
        || (long)H * W * A > (0x7fffffffL / 8) / B)
        return COBEVT_ERR_SHAPE;
    if ((uintptr_t)workspace & 7) return COBEVT_ERR_SHAPE;
    const int HW = H * W, M = HW * A;
    const long nblk = ppl_blocks(B, HW, A);
    double* partial = (double*)workspace;                                // 2 nblk doubles, then B ints
    int* counts = (int*)(partial + 2 * nblk);
    if (!num_pos) {
        if (hipMemsetAsync(counts, 0, 4 * (size_t)B, stream) != hipSuccess) return COBEVT_ERR_LAUNCH;
        hipLaunchKernelGGL(ppl_count_kernel, dim3((unsigned)((M + 255) / 256), (unsigned)B), dim3(256), 0, stream, pos_equal_one, counts, M);
        num_pos = counts;
    }
    hipLaunchKernelGGL(ppl_main_kernel, dim3((unsigned)((HW + 255) / 256), (unsigned)A, (unsigned)B), dim3(256), 0, stream, psm, rm,
                       pos_equal_one, targets, num_pos, partial, dpsm, drm, HW, A, cls_weight / (float)B, reg / (float)B);
    hipLaunchKernelGGL(ppl_finish_kernel, dim3(1), dim3(256), 0, stream, (const double*)partial, nblk, loss,
                       (double)cls_weight / B, (double)reg / B);
    return cobevt::launch_status();
}
