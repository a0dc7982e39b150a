// AttFusion (fusion_modules/self_attn.py:36-57) on channels-last maps: per pixel, scaled-dot-product attention over the agents of a
// sample, of which the reference keeps row 0 (the ego's).  sample_rows / group_ok / 8 channels per lane are warp_common.hpp's, shared
// with pairwise_fusion.hip; no matrix product, so the one shared object serves all three libraries.
//
//   x (N, HW, C), out (B, HW, C);  sample b owns agent rows off .. off + n - 1 (off = sum record_len[:b]):
//   s_j = <x[off, p], x[off + j, p]> * scale,  w = softmax_j(s),  out[b, p] = sum_j w_j x[off + j, p]
//
// A group of G = C / 8 lanes owns one pixel (64 / G pixels per wave); G is a power of two <= 64, so a group never straddles a wave
// and the xor butterfly below stays inside it.  The ego row stays in registers, every agent row is loaded once (16-byte loads, the
// next one in flight while this one is folded in), the softmax is online with a running maximum, all arithmetic is fp32 with the
// accurate expf, and the result is rounded once to the storage type.  The op is memory-bound: n C in, C out per pixel.
#include "warp_common.hpp"

namespace cobevt {
namespace {

template <typename T>
__global__ __launch_bounds__(256) void att_fuse_kernel(const T* x, const int* record_len, T* out, int N, long HW, int C, float scale) {
    const int G = C >> 3;
    const int b = blockIdx.y;
    int off, n;
    sample_rows(record_len, b, off, n);
    // a wrong record_len reads nothing outside x: n is clamped to [0, N - off]
    if (off < 0 || off >= N) n = 0;
    else if (n > N - off) n = N - off;
    const long gid = ((long)blockIdx.x * 256 + threadIdx.x) / G;
    const int gl = threadIdx.x & (G - 1);
    // groups past the last pixel follow along on the last pixel (whole groups: no lane of a live group is missing from the butterfly)
    // and store nothing
    const bool live = gid < HW;
    const size_t p = (size_t)(live ? gid : HW - 1);
    const size_t stride = (size_t)HW * C;                       // one agent's map
    T* dst = out + ((size_t)b * HW + p) * C + gl * 8;
    float acc[8];
    if (n <= 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = 0.f;
        if (live) store8<T>(dst, acc);
        return;
    }
    const T* src = x + ((size_t)off * HW + p) * C + gl * 8;
    float e[8], t[8];
    load8<T>(src, e);
    if (n > 1) load8<T>(src + stride, t);
    // agent 0 is the ego itself: weight exp(0) = 1, so a sample of one agent returns its map bit for bit
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) { dot += e[k] * e[k]; acc[k] = e[k]; }
    for (int m = G >> 1; m >= 1; m >>= 1) dot += __shfl_xor(dot, m);
    float mx = dot * scale, den = 1.f;
    for (int j = 1; j < n; ++j) {
        float u[8];
        if (j + 1 < n) load8<T>(src + (size_t)(j + 1) * stride, u);
        dot = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) dot += e[k] * t[k];
        for (int m = G >> 1; m >= 1; m >>= 1) dot += __shfl_xor(dot, m);         // a + b == b + a: every lane of the group gets the same bits
        const float s = dot * scale;
        const float mn = fmaxf(mx, s);
        const float a = expf(mx - mn), w = expf(s - mn);
        den = den * a + w;
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = acc[k] * a + w * t[k];
        mx = mn;
        if (j + 1 < n) {
#pragma unroll
            for (int k = 0; k < 8; ++k) t[k] = u[k];
        }
    }
    const float inv = 1.f / den;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] *= inv;
    if (live) store8<T>(dst, acc);
}

// The backward of att_fuse_kernel<float> with respect to x: nothing is saved by the forward, the statistics are recomputed.  With
// g = dout[b, p], t_j = <g, x_j> and P as above:  ds_j = P_j (t_j - sum_k P_k t_k),  dx_j = P_j g + scale ds_j x_0, and the ego's row
// additionally gets scale sum_j ds_j x_j (x_0 is the query of every score and the key of its own).  Two passes over the agents: the
// first keeps the running maximum, the denominator and sum_k w_k t_k, the second recomputes s_j / t_j with the same instructions (the
// same bits), writes the rows of the agents 1 .. n - 1 and accumulates the ego's, which is stored last.  The same groups, grid and
// clamping as the forward; every row of dx is written once: the rows of a sample by its own workgroups, the rows behind the last
// sample's (agents that belong to no sample) get zeros from the workgroups of sample B - 1.  n = 1: P_0 = 1, ds_0 = 0, dx_0 = g.
// one lane's share of a dot product as a fixed chain of fused multiply-adds: both passes of the backward get the same bits
__device__ __forceinline__ float dot8(const float* a, const float* b) {
    float d = __fmul_rn(a[0], b[0]);
#pragma unroll
    for (int k = 1; k < 8; ++k) d = __fmaf_rn(a[k], b[k], d);
    return d;
}

__global__ __launch_bounds__(256) void att_fuse_bwd_kernel(const float* x, const int* record_len, const float* dout, float* dx, int B, int N, long HW,
                                                           int C, float scale) {
    // no contraction in this body: the second pass recomputes s_j and t_j, and exp(s_0 - max) = 1, ds_0 = 0 for a sample of one agent
    // hold only if both passes round the same products (a product fused into the subtraction that follows it is not rounded)
#pragma clang fp contract(off)
    const int G = C >> 3;
    const int b = blockIdx.y;
    int off, n;
    sample_rows(record_len, b, off, n);
    if (off < 0 || off >= N) n = 0;
    else if (n > N - off) n = N - off;
    if (n < 0) n = 0;
    const long gid = ((long)blockIdx.x * 256 + threadIdx.x) / G;
    const int gl = threadIdx.x & (G - 1);
    const bool live = gid < HW;
    const size_t p = (size_t)(live ? gid : HW - 1);
    const size_t stride = (size_t)HW * C;
    const size_t col = p * C + gl * 8;
    if (b == B - 1 && live) {
        // the rows no sample owns: from the end of this (the last) sample's agents to N
        long z0 = (long)off + n;
        if (z0 < 0) z0 = 0;
        float z[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) z[k] = 0.f;
        for (long r = z0; r < N; ++r) store8<float>(dx + (size_t)r * stride + col, z);
    }
    if (n <= 0) return;
    const float* src = x + (size_t)off * stride + col;
    float* dst = dx + (size_t)off * stride + col;
    float e[8], g[8], t[8];
    load8<float>(src, e);
    load8<float>(dout + (size_t)b * stride + col, g);
    // pass 1: the softmax statistics and U = sum_k w_k t_k, online
    float mx = 0.f, den = 0.f, U = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = e[k];
    for (int j = 0; j < n; ++j) {
        float u[8];
        if (j + 1 < n) load8<float>(src + (size_t)(j + 1) * stride, u);
        float dot = dot8(e, t), tj = dot8(g, t);
        for (int m = G >> 1; m >= 1; m >>= 1) { dot += __shfl_xor(dot, m); tj += __shfl_xor(tj, m); }
        const float s = dot * scale;
        if (j == 0) { mx = s; den = 1.f; U = tj; }
        else {
            const float mn = fmaxf(mx, s);
            const float a = expf(mx - mn), w = expf(s - mn);
            den = den * a + w;
            U = U * a + w * tj;
            mx = mn;
        }
        if (j + 1 < n) {
#pragma unroll
            for (int k = 0; k < 8; ++k) t[k] = u[k];
        }
    }
    const float inv = 1.f / den;
    const float tbar = U * inv;
    // pass 2: the rows
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { acc[k] = 0.f; t[k] = e[k]; }
    float p0 = 0.f, ds0 = 0.f;
    for (int j = 0; j < n; ++j) {
        float u[8];
        if (j + 1 < n) load8<float>(src + (size_t)(j + 1) * stride, u);
        float dot = dot8(e, t), tj = dot8(g, t);
        for (int m = G >> 1; m >= 1; m >>= 1) { dot += __shfl_xor(dot, m); tj += __shfl_xor(tj, m); }
        const float P = expf(dot * scale - mx) * inv;
        const float ds = P * (tj - tbar);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += ds * t[k];
        if (j == 0) { p0 = P; ds0 = ds; }
        else {
            float o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = P * g[k] + scale * ds * e[k];
            if (live) store8<float>(dst + (size_t)j * stride, o);
        }
        if (j + 1 < n) {
#pragma unroll
            for (int k = 0; k < 8; ++k) t[k] = u[k];
        }
    }
    float o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = p0 * g[k] + scale * ds0 * e[k] + scale * acc[k];
    if (live) store8<float>(dst, o);
}

}  // namespace
}  // namespace cobevt

using namespace cobevt;

extern "C" int cobevt_att_fuse_nhwc(const void* x, const int* record_len, void* out, int dtype, int B, int N, long HW, int C, float scale,
                                    hipStream_t stream) {
    if (!x || !record_len || !out) return COBEVT_ERR_ARG;
    if (dtype != 0 && dtype != 1) return COBEVT_ERR_ARG;
    if (!group_ok(C) || B < 1 || B > 65535 || N < 1 || HW < 1) return COBEVT_ERR_SHAPE;
    const long blocks = (HW * (C >> 3) + 255) / 256;
    if (blocks > 0x7fffffffL) return COBEVT_ERR_SHAPE;
    const dim3 grid((unsigned)blocks, (unsigned)B);
    if (dtype == 0) hipLaunchKernelGGL(att_fuse_kernel<bf16_t>, grid, dim3(256), 0, stream, (const bf16_t*)x, record_len, (bf16_t*)out, N, HW, C, scale);
    else hipLaunchKernelGGL(att_fuse_kernel<float>, grid, dim3(256), 0, stream, (const float*)x, record_len, (float*)out, N, HW, C, scale);
    return cobevt::launch_status();
}

extern "C" int cobevt_att_fuse_bwd_nhwc(const float* x, const int* record_len, const float* dout, float* dx, int B, int N, long HW, int C, float scale,
                                        hipStream_t stream) {
    if (!x || !record_len || !dout || !dx) return COBEVT_ERR_ARG;
    if (!group_ok(C) || B < 1 || B > 65535 || N < 1 || HW < 1) return COBEVT_ERR_SHAPE;
    const long blocks = (HW * (C >> 3) + 255) / 256;
    if (blocks > 0x7fffffffL) return COBEVT_ERR_SHAPE;
    hipLaunchKernelGGL(att_fuse_bwd_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, stream, x, record_len, dout, dx, B, N, HW, C, scale);
    return cobevt::launch_status();
}
