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


// ---------------------------------------------------------------------------------------------- typed agent attention (HGTCavAttention)
// cobevt_typed_linear:  y[row] = W[t] n(x[row]) + bias[t] (+ residual[row]),  t = clamp(types[g], 0, T - 1) for the rows of group g
// (G groups of R consecutive rows: one agent's H W pixels).  One workgroup of four waves owns a tile of 32 rows of ONE group (a tail
// tile follows along on the group's last row and stores nothing outside the group) and all N columns.  Phase 1: eight lanes per row
// copy the row into LDS in the storage type, 16 bytes at a time; with ln they take  mu = sum x / K,  q = sum (x - mu)^2,
// r = rsqrtf(q / K + eps)  on the way and write (x - mu) r, rounded once to the storage type (the LayerNorm's affine is folded into W
// and bias by the host).  Every lane re-reads only the chunks it wrote itself, so the phase needs no barrier before its end.
// Phase 2: D = W X^T per 32 x 32 tile, two column tiles per wave and pass: the W fragment of a lane is 16 bytes of row n of W[t] as
// it lies (nn.Linear layout, no lowering), the X fragment 16 bytes of LDS row (lane & 31); bf16 storage on v_mfma_f32_32x32x16_bf16,
// fp32 storage on four exact v_mfma_f32_32x32x2_f32 per 16-byte piece - in every library: this source is compiled once.  Epilogue:
// a lane holds four consecutive columns of its row per accumulator quad: + bias (+ residual) in fp32, one rounding, 8 / 16-byte stores.
struct TypedLinearArgs {
    const void* x; const void* w; const float* bias; const int* types; const void* residual; void* out;
    int R, K, N, T, ln;
    float eps;
};

template <typename T> __device__ __forceinline__ void typed_mfma(const uint4& a, const uint4& b, f32x16& acc) {
    if constexpr (Elem<T>::kIsBf16) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
    } else {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void typed_linear_kernel(TypedLinearArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char typed_lds[];
    constexpr int EB = Elem<T>::kBytes, CH = Elem<T>::kChunk;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, half = lane >> 5;
    const int g = blockIdx.y;
    int t = a.types[g];
    t = t < 0 ? 0 : (t >= a.T ? a.T - 1 : t);                       // any types value reads inside W and bias
    const int K = a.K, N = a.N;
    const int rowbytes = K * EB, stride = rowbytes + 16;
    const long r0 = (long)blockIdx.x * 32;
    {   // phase 1
        const int row = tid >> 3, j = tid & 7;
        long r = r0 + row;
        if (r >= a.R) r = a.R - 1;
        const T* src = (const T*)a.x + ((size_t)g * a.R + (size_t)r) * K;
        unsigned char* dst = typed_lds + row * stride;
        const int nch = K / CH;
        float sum = 0.f;
        for (int c = j; c < nch; c += 8) {
            const uint4 v = *(const uint4*)(src + c * CH);
            *(uint4*)(dst + c * 16) = v;
            if (a.ln) {
                float f[8];
                chunk_to_f32<T>(v, f);
#pragma unroll
                for (int k = 0; k < CH; ++k) sum += f[k];
            }
        }
        if (a.ln) {
            sum += __shfl_xor(sum, 1); sum += __shfl_xor(sum, 2); sum += __shfl_xor(sum, 4);
            const float mu = sum / (float)K;
            float q = 0.f;
            for (int c = j; c < nch; c += 8) {
                float f[8];
                chunk_to_f32<T>(*(const uint4*)(dst + c * 16), f);
#pragma unroll
                for (int k = 0; k < CH; ++k) { const float d = f[k] - mu; q += d * d; }
            }
            q += __shfl_xor(q, 1); q += __shfl_xor(q, 2); q += __shfl_xor(q, 4);
            const float rs = rsqrtf(q / (float)K + a.eps);
            for (int c = j; c < nch; c += 8) {
                float f[8];
                chunk_to_f32<T>(*(const uint4*)(dst + c * 16), f);
#pragma unroll
                for (int k = 0; k < CH; ++k) f[k] = (f[k] - mu) * rs;
                *(uint4*)(dst + c * 16) = f32_to_chunk<T>(f);
            }
        }
    }
    __syncthreads();
    // phase 2
    const int ntiles = N >> 5, kgroups = rowbytes >> 5;
    const unsigned char* wt = (const unsigned char*)a.w + (size_t)t * N * rowbytes;
    const float* bt = a.bias + (size_t)t * N;
    const unsigned char* xrow = typed_lds + l32 * stride + 16 * half;
    const long r = r0 + l32;
    const bool live = r < a.R;
    const size_t orow = ((size_t)g * a.R + (size_t)(live ? r : a.R - 1)) * N;
    for (int ct = wave * 2; ct < ntiles; ct += 8) {
        const bool two = ct + 1 < ntiles;                            // an odd tile count: the second tile repeats the first, unstored
        const unsigned char* w0 = wt + (size_t)(ct * 32 + l32) * rowbytes + 16 * half;
        const unsigned char* w1 = wt + (size_t)((two ? ct + 1 : ct) * 32 + l32) * rowbytes + 16 * half;
        f32x16 acc0, acc1;
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
#pragma unroll 4
        for (int kg = 0; kg < kgroups; ++kg) {
            const uint4 xb = *(const uint4*)(xrow + kg * 32);
            const uint4 wa0 = *(const uint4*)(w0 + kg * 32);
            const uint4 wa1 = *(const uint4*)(w1 + kg * 32);
            typed_mfma<T>(wa0, xb, acc0);
            typed_mfma<T>(wa1, xb, acc1);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (s == 1 && !two) break;
            const f32x16& acc = s ? acc1 : acc0;
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                const int n = (ct + s) * 32 + 8 * qd + 4 * half;
                const float4 b4 = *(const float4*)(bt + n);
                float4 v = make_float4(acc[4 * qd] + b4.x, acc[4 * qd + 1] + b4.y, acc[4 * qd + 2] + b4.z, acc[4 * qd + 3] + b4.w);
                if (a.residual) {
                    const float4 rv = ld4q(a.residual, orow + n, Elem<T>::kIsBf16);
                    v.x += rv.x; v.y += rv.y; v.z += rv.z; v.w += rv.w;
                }
                if (live) st4q(a.out, orow + n, Elem<T>::kIsBf16, v);
            }
        }
    }
}

// cobevt_hgt_attention_nhwc: per pixel p, head m and query agent i of sample b, with a = clamp(types[b L + i], 0, T - 1):
//   s_j = scale <q_i, k'_(j, a)>  over the unmasked keys j,  out_i = sum_j softmax_j(s) v'_(j, a)
// proj (B, L, HW, (1 + 2 T) inner) = [q | k'_0 .. k'_(T-1) | v'_0 .. v'_(T-1)] per row, out (B, L, HW, inner), mask (B, HW, L) or null.
// Four lanes own one (pixel, head) of one query agent (8 of the head's 32 channels each, 16-byte accesses); a workgroup's rows all
// belong to one (b, i), so the variant is uniform in it.  Every lane runs every key (the butterfly needs whole groups) and folds in
// only the unmasked ones: fp32, running maximum, accurate expf, one rounding.  No key left: zeros.
template <typename T>
__global__ __launch_bounds__(256) void hgt_attention_kernel(const T* proj, const int* types, const float* mask, T* out, int L, long HW, int inner,
                                                            int Tn, float scale) {
    const int bi = blockIdx.y;                                      // b L + i
    const int b = bi / L;
    int ty = types[bi];
    ty = ty < 0 ? 0 : (ty >= Tn ? Tn - 1 : ty);
    const int G = inner >> 3;                                       // lanes per row: 4 per head
    // pixel and channel slot both from the GLOBAL lane index: G = 4 heads need not divide 256, so a row's lanes may straddle two
    // workgroups; 256 and G are multiples of 4, so the four lanes of a head stay together in one wave
    const long lane_id = (long)blockIdx.x * 256 + threadIdx.x;
    const long gid = lane_id / G;
    const int gl = (int)(lane_id % G);
    const bool live = gid < HW;
    const size_t p = (size_t)(live ? gid : HW - 1);
    const size_t ld = (size_t)(1 + 2 * Tn) * inner;
    const size_t agent = (size_t)HW * ld;
    const T* base = proj + ((size_t)b * L * HW + p) * ld + gl * 8;  // agent 0's row of this pixel
    const T* kp = base + (size_t)(1 + ty) * inner;
    const T* vp = base + (size_t)(1 + Tn + ty) * inner;
    const float* mp = mask ? mask + ((size_t)b * HW + p) * L : nullptr;
    float q[8], acc[8];
    load8<T>(base + (size_t)(bi - b * L) * agent, q);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.f;
    float mx = 0.f, den = 0.f;
    bool any = false;
    for (int j = 0; j < L; ++j) {
        float kk[8], vv[8];
        load8<T>(kp + (size_t)j * agent, kk);
        load8<T>(vp + (size_t)j * agent, vv);
        const bool on = mp ? mp[j] != 0.f : true;
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) dot += q[k] * kk[k];
        dot += __shfl_xor(dot, 1);
        dot += __shfl_xor(dot, 2);                                  // a + b == b + a: the four lanes of a head get the same bits
        const float s = dot * scale;
        if (on) {
            if (!any) {
                any = true; mx = s; den = 1.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[k] = vv[k];
            } else {
                const float mn = fmaxf(mx, s);
                const float ea = expf(mx - mn), w = expf(s - mn);
                den = den * ea + w;
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[k] = acc[k] * ea + w * vv[k];
                mx = mn;
            }
        }
    }
    const float inv = any ? 1.f / den : 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] *= inv;
    if (live) store8<T>(out + ((size_t)bi * HW + p) * inner + gl * 8, acc);
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

extern "C" int cobevt_typed_linear(const void* x, const void* w, const float* bias, const int* types, const void* residual, void* out,
                                   const long* dims, float ln_eps, hipStream_t stream) {
    // dims: [dtype, G, R, K, N, T, ln]
    if (!x || !w || !bias || !types || !out || !dims) return COBEVT_ERR_ARG;
    const long dtype = dims[0], G = dims[1], R = dims[2], K = dims[3], N = dims[4], Tn = dims[5], ln = dims[6];
    if ((dtype != 0 && dtype != 1) || (ln != 0 && ln != 1) || !(ln_eps >= 0.f)) return COBEVT_ERR_ARG;
    if (G < 1 || R < 1 || Tn < 1 || K < 32 || K % 32 || N < 32 || N % 32) return COBEVT_ERR_SHAPE;
    if (G > 65535 || Tn > 65535 || N > (1L << 20) || R > 0x7fffffffL) return COBEVT_ERR_SHAPE;        // R, K, N, T travel as int
    if (K > (ln ? 512 : 1024)) return COBEVT_ERR_UNSUPPORTED;
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)residual | (uintptr_t)out) & 15) return COBEVT_ERR_SHAPE;
    if ((uintptr_t)types & 3) return COBEVT_ERR_SHAPE;
    TypedLinearArgs a{x, w, bias, types, residual, out, (int)R, (int)K, (int)N, (int)Tn, (int)ln, ln_eps};
    const dim3 grid((unsigned)((R + 31) / 32), (unsigned)G);
    const int lds = 32 * ((int)K * (dtype == 0 ? 2 : 4) + 16);
    if (dtype == 0) {
        allow_dynamic_lds<typed_linear_kernel<bf16_t>>(160 * 1024);
        hipLaunchKernelGGL(typed_linear_kernel<bf16_t>, grid, dim3(256), lds, stream, a);
    } else {
        allow_dynamic_lds<typed_linear_kernel<float>>(160 * 1024);
        hipLaunchKernelGGL(typed_linear_kernel<float>, grid, dim3(256), lds, stream, a);
    }
    return cobevt::launch_status();
}

extern "C" int cobevt_hgt_attention_nhwc(const void* proj, const int* types, const float* mask, void* out, int dtype, int B, int L, long HW,
                                         int heads, int T, float scale, hipStream_t stream) {
    if (!proj || !types || !out) return COBEVT_ERR_ARG;
    if (dtype != 0 && dtype != 1) return COBEVT_ERR_ARG;
    if (B < 1 || L < 1 || HW < 1 || heads < 1 || T < 1) return COBEVT_ERR_SHAPE;
    if (L > 8 || heads > 64 || T > 64) return COBEVT_ERR_UNSUPPORTED;
    if ((long)B * L > 65535) return COBEVT_ERR_SHAPE;
    if (((uintptr_t)proj | (uintptr_t)out) & 15 || ((uintptr_t)types | (uintptr_t)mask) & 3) return COBEVT_ERR_SHAPE;
    const int inner = heads * 32;
    const long blocks = (HW * (inner >> 3) + 255) / 256;
    if (blocks > 0x7fffffffL) return COBEVT_ERR_SHAPE;
    const dim3 grid((unsigned)blocks, (unsigned)(B * L));
    if (dtype == 0) hipLaunchKernelGGL(hgt_attention_kernel<bf16_t>, grid, dim3(256), 0, stream, (const bf16_t*)proj, types, mask, (bf16_t*)out, L, HW, inner, T, scale);
    else hipLaunchKernelGGL(hgt_attention_kernel<float>, grid, dim3(256), 0, stream, (const float*)proj, types, mask, (float*)out, L, HW, inner, T, scale);
    return cobevt::launch_status();
}
