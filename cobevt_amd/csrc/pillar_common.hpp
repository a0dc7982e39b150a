// Device helpers shared by the LiDAR pillar kernels (pillar_vfe.hip: inference; train_pillar.hip: statistics and backward of the
// train-mode layer): the operator's arguments, the half-wave exchanges, the destination row of a pillar and the point decoration.
// The training kernels decorate, skip and place a pillar exactly as the inference operator does; pillar_vfe_kernel keeps the
// decoration, the layer and the maximum written out in place (see the note there), everything else has its one definition here.
#pragma once
#include "warp_common.hpp"

namespace cobevt {

constexpr int kPillarC = 64;          // channels of the one PFN layer

struct PillarArgs {
    long P;
    int T, rows;                      // rows != 0: dense rows (P, 64), destination row = p
    int N, B, max_cav, ny, nx;
    float vx, vy, vz, xoff, yoff, zoff;
};

constexpr int pillar_k(bool use_abs, bool dist) { return (use_abs ? 4 : 1) + 6 + (dist ? 1 : 0); }

// value of lane (lane ^ X) of the same 32-lane group (ds_swizzle bit mode: and 0x1f, or 0, xor X)
template <int X> __device__ __forceinline__ float swz_xor(float v) {
    return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), (X << 10) | 0x1f));
}
__device__ __forceinline__ float half_wave_sum_swz(float v) {
    v += swz_xor<16>(v);
    v += swz_xor<8>(v);
    v += swz_xor<4>(v);
    v += swz_xor<2>(v);
    v += swz_xor<1>(v);
    return v;
}

// Destination row of a pillar on the canvas, or -1 when the pillar is skipped (never written): batch index negative, >= N or in a
// regrouped slot >= max_cav; y or x outside the grid (or z + y nx + x outside the map).  The caller skips n_p <= 0.
__device__ __forceinline__ long canvas_row(const int4& c, const int* __restrict__ record_len, int N, int B, int max_cav, int ny, int nx) {
    const int n = c.x;
    if (n < 0 || n >= N) return -1;
    int slot = -1;
    if (record_len) {
        int off = 0;
        for (int bb = 0; bb < B; ++bb) {
            const int r = max(record_len[bb], 0);
            if (slot < 0 && n >= off && n < off + r && n - off < max_cav) slot = bb * max_cav + (n - off);
            off += r;
        }
    } else {
        slot = n;
    }
    if (slot < 0 || c.z < 0 || c.z >= ny || c.w < 0 || c.w >= nx) return -1;
    const long cell = (long)c.y + (long)c.z * nx + c.w;           // z + y * nx + x (point_pillar_scatter.py:30-32); y is the row
    if (cell < 0 || cell >= (long)ny * nx) return -1;
    return (long)slot * ny * nx + cell;
}

// The K decorated features of point `pt` = row min(t, T - 1) of a pillar whose T rows sit on the 32 lanes of a half-wave
// (pillar_vfe.py:105-143).  Every lane of the half-wave must call it (cross-lane sums).  Rows >= n_p come out as zeros.
template <bool kAbs, bool kDist>
__device__ __forceinline__ void pillar_decorate(const float4& pt, int t, int n_p, const int4& c, const PillarArgs& a,
                                                float (&f)[pillar_k(kAbs, kDist)]) {
    constexpr int K = pillar_k(kAbs, kDist);
    const int tr = min(t, a.T - 1);
    const bool inrow = t < a.T;
    // the mean sums all T rows (pillar_vfe.py:110-112), whatever the rows >= n_p hold
    const float fn = (float)n_p;
    const float mx = half_wave_sum_swz(inrow ? pt.x : 0.f) / fn, my = half_wave_sum_swz(inrow ? pt.y : 0.f) / fn,
                mz = half_wave_sum_swz(inrow ? pt.z : 0.f) / fn;
    // voxel centre as the reference forms it: coord * voxel rounded, then + offset rounded (no contraction: at +-140 m an fma moves the
    // centre by an ulp of 1.5e-5 m, which is not small against the +-0.2 m offsets it is subtracted from)
    const float cx = __fadd_rn(__fmul_rn((float)c.w, a.vx), a.xoff);
    const float cy = __fadd_rn(__fmul_rn((float)c.z, a.vy), a.yoff);
    const float cz = __fadd_rn(__fmul_rn((float)c.y, a.vz), a.zoff);
    int k = 0;
    if constexpr (kAbs) { f[0] = pt.x; f[1] = pt.y; f[2] = pt.z; f[3] = pt.w; k = 4; }
    else { f[0] = pt.w; k = 1; }
    f[k + 0] = pt.x - mx; f[k + 1] = pt.y - my; f[k + 2] = pt.z - mz;
    f[k + 3] = pt.x - cx; f[k + 4] = pt.y - cy; f[k + 5] = pt.z - cz;
    if constexpr (kDist) f[k + 6] = sqrtf(pt.x * pt.x + pt.y * pt.y + pt.z * pt.z);
    // rows t >= n_p are multiplied by 0 and STILL go through the layer: they contribute relu(s[c]) to the maximum (:137-143)
    const bool on = tr < n_p;
#pragma unroll
    for (int i = 0; i < K; ++i) f[i] = on ? f[i] : 0.f;
}

// The layer's 64 responses of one row: acc[ch] = S[ch] + sum_i f[i] W[i][ch], W (K, 64) and S (64) wave-uniform (scalar loads).
// One row of W (64 scalar registers) per trip of a rolled loop: unrolled, all K rows' loads are hoisted to the top and 400 - 700
// scalar registers spill.  The trip's feature is picked by wave-uniform selects (K - 1 against 64 fused multiply-adds).
template <int K>
__device__ __forceinline__ void pillar_responses(const float (&f)[K], const float* __restrict__ W, const float* __restrict__ S,
                                                 float (&acc)[kPillarC]) {
#pragma unroll
    for (int ch = 0; ch < kPillarC; ++ch) acc[ch] = S[ch];
#pragma unroll 1
    for (int i = 0; i < K; ++i) {
        float fi = f[0];
#pragma unroll
        for (int j = 1; j < K; ++j) fi = i == j ? f[j] : fi;
        const float* __restrict__ wr = W + i * kPillarC;
#pragma unroll
        for (int ch = 0; ch < kPillarC; ++ch) acc[ch] = fmaf(fi, wr[ch], acc[ch]);
    }
}

// Maximum of the 64 responses over the 32 lanes of the half-wave, transposing: after the xor-16 step a lane keeps channels
// [32 b4, +32), then [.. + 16 b3, +16), [.. + 8 b2, +8); the xor-2 / 1 steps are plain butterflies.  Lane group g = (t >> 2) & 7 ends up
// with channels 8 g .. 8 g + 7 in r (the same in its four lanes).
__device__ __forceinline__ void pillar_row_max(const float (&acc)[kPillarC], int t, float (&r)[8]) {
    const bool b4 = (t & 16) != 0, b3 = (t & 8) != 0, b2 = (t & 4) != 0;
    float u[32], v[16];
#pragma unroll
    for (int ch = 0; ch < 32; ++ch) {
        const float keep = b4 ? acc[32 + ch] : acc[ch], send = b4 ? acc[ch] : acc[32 + ch];
        u[ch] = fmaxf(keep, swz_xor<16>(send));
    }
#pragma unroll
    for (int ch = 0; ch < 16; ++ch) {
        const float keep = b3 ? u[16 + ch] : u[ch], send = b3 ? u[ch] : u[16 + ch];
        v[ch] = fmaxf(keep, swz_xor<8>(send));
    }
#pragma unroll
    for (int ch = 0; ch < 8; ++ch) {
        const float keep = b2 ? v[8 + ch] : v[ch], send = b2 ? v[ch] : v[8 + ch];
        r[ch] = fmaxf(keep, swz_xor<4>(send));
    }
#pragma unroll
    for (int ch = 0; ch < 8; ++ch) {
        r[ch] = fmaxf(r[ch], swz_xor<2>(r[ch]));
        r[ch] = fmaxf(r[ch], swz_xor<1>(r[ch]));
    }
}

}  // namespace cobevt
