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
