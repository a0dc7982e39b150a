// Wave-level device helpers shared by the cobevt_amd HIP kernels (gfx950 / CDNA4 only, wave64): cross-lane reductions, the
// half-wave exchanges behind the "rows in registers" kernels, and the small packing helpers that go with them.  One definition
// each - a new kernel includes this header instead of copying from a sibling.  Everything is __forceinline__.
#pragma once
#include "common.hpp"

namespace cobevt {

// ---- sums over xor-butterflies of lanes

// sum over the `width` lanes that differ in the low log2(width) lane bits (xor width/2 .. 1): 64 = the whole wave
__device__ __forceinline__ float wave_sum_xor(float v, int width) {
    for (int o = width >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// sum inside each 32-lane half of the wave (xor 16 .. 1): a row per half-wave
__device__ __forceinline__ float half_wave_sum(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// sum over 8 adjacent lanes in the order xor 1, 2, 4: a row held by 8 lanes (the LayerNorm sums of the 32-row dense-row kernels)
__device__ __forceinline__ float lane8_sum(float v) {
    v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
    return v;
}

// ---- the two half-waves (lane, lane ^ 32) without LDS: v_permlane32_swap exchanges the upper half of the first operand with the
// lower half of the second, so {r0, r1} = {own, partner} in one order or the other on every lane

__device__ __forceinline__ float xhalf_sum(float v) {          // v + the value of lane ^ 32
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float xhalf_max(float v) {          // max(v, the value of lane ^ 32)
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
// D = W . X^T hands a lane, of its own row, the columns {32 t + 8 k + 4 h + j} (h = lane >> 5): accumulator order.
// {lo, hi} (16 bytes at natural channel order, channels 16 m + 8 h .. + 7) <-> the two 4-channel runs this lane holds in
// accumulator order (run 2 m: channels 16 m + 4 h .. + 3; run 2 m + 1: channels 16 m + 8 + 4 h .. + 3).  The same exchange in
// both directions: it swaps the upper half-wave's `a` with the lower half-wave's `b`.
__device__ __forceinline__ void half_swap(uint2& a, uint2& b) {
    auto r = __builtin_amdgcn_permlane32_swap(a.x, b.x, false, false);
    a.x = r[0]; b.x = r[1];
    r = __builtin_amdgcn_permlane32_swap(a.y, b.y, false, false);
    a.y = r[0]; b.y = r[1];
}

// swap bits 2 and 3: key order inside a 16-key MFMA k-block (the order the score registers hold the keys in)
__device__ __forceinline__ int perm16(int k) { return (k & ~12) | ((k & 4) << 1) | ((k & 8) >> 1); }

// ---- packing

// 8 consecutive fp32 values (accumulator registers [8 u, 8 u + 8) of a tile) -> one bf16 MFMA operand
__device__ __forceinline__ uint4 pack8(const float* v) {
    return make_uint4(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7]));
}
__device__ __forceinline__ float rbf(float x) { return bf2f(f2bf(x)); }          // the value a bf16 store would keep

// normalise one 128-channel row held by 8 lanes (16 channels each)
__device__ __forceinline__ void normalise128(float (&v)[16], float eps) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) s += v[e];
    const float mean = lane8_sum(s) * (1.0f / 128.0f);
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) { const float d = v[e] - mean; q += d * d; }
    const float rstd = rsqrtf(lane8_sum(q) * (1.0f / 128.0f) + eps);
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = (v[e] - mean) * rstd;
}

// ---- LDS transpose read (ds_read_b64_tr_b16) of [row][bf16 channel] data: lane i of a 16-lane group supplies the address of row i / 4,
// channels 4 (i % 4) .. + 3, and receives channel i of the group's four rows - 4 consecutive rows of the lane's column in one read
// (attn_common.hpp read_vt16 spells the lane mapping out and pairs two of these reads into one MFMA operand)
__device__ __forceinline__ uint2 tr_read(const unsigned char* lds) {
    typedef short v4s __attribute__((ext_vector_type(4)));
    const v4s r = __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s __attribute__((address_space(3)))*)lds);
    return __builtin_bit_cast(uint2, r);
}

}  // namespace cobevt
