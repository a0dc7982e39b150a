// LiDAR pillar front end (gfx950): PillarVFE with one PFN layer of 64 channels + PointPillarScatter + regroup as one operator, from the
// reference's voxel dict straight to FuseBEVT's channels-last canvas (B, max_cav, ny, nx, 64).
// reference: opv2v/opencood/models/sub_modules/pillar_vfe.py:10-53 (PFNLayer), :105-146 (PillarVFE.forward),
//            point_pillar_scatter.py:14-47, fuse_utils.py:8-61 (regroup).
//
// Arithmetic: fp32 on the VALU in every compute mode and in all three libraries (absolute coordinates reach +-140 m: no bf16 / fp16
// operand, no MFMA, nothing that differs between the three libraries); only the final store converts to the storage dtype.
//
// Layout: a pillar's T <= 32 points sit on the 32 lanes of one half-wave (one 16-byte load per point), so the coordinate mean and the
// 64 channel maxima are cross-lane reductions inside the half-wave; the folded weight W (K, 64) and shift s (64) are wave-uniform
// (scalar loads).  The maxima are reduced "transposing": the xor-16 / 8 / 4 steps each halve the channels a lane keeps (64 -> 32 -> 16
// -> 8, 56 swizzles instead of 192), the xor-2 / 1 steps are plain butterflies over 8 channels, and lane group g = (lane >> 2) & 7 ends
// up with channels 8g .. 8g + 7 of the row: eight (bf16) or sixteen (fp32) 16-byte stores per row.
//
// Canvas: the operator's first launch writes every 16-byte chunk of the canvas with zeros (and the agent mask), its second writes the
// rows of the pillars that land on it - plain stores in stream order, no atomics, bitwise reproducible.
#include "pillar_common.hpp"

namespace cobevt {

template <typename T, bool kAbs, bool kDist>
__global__ __launch_bounds__(256) void pillar_vfe_kernel(const float4* __restrict__ vf, const int* __restrict__ npts,
                                                         const int4* __restrict__ coords, const float* __restrict__ W,
                                                         const float* __restrict__ S, const int* __restrict__ record_len,
                                                         T* __restrict__ out, PillarArgs a) {
    constexpr int K = pillar_k(kAbs, kDist);
    const int t = threadIdx.x & 31;
    const long p = (long)blockIdx.x * 8 + (threadIdx.x >> 5);
    int n_p = 0;
    int4 c = make_int4(-1, 0, 0, 0);
    long dst = -1;
    if (p < a.P) {
        n_p = npts[p];
        c = coords[p];
        if (a.rows) dst = p;
        else if (n_p > 0) dst = canvas_row(c, record_len, a.N, a.B, a.max_cav, a.ny, a.nx);
    }
    if (dst < 0) return;                         // uniform over the half-wave; every cross-lane step below stays inside it

    // The decoration, the layer and the transposing maximum below are pillar_decorate / pillar_responses / pillar_row_max of
    // pillar_common.hpp written out in place: routed through those functions the compiler allocates and schedules this kernel
    // differently (72 instead of 78 - 82 VGPRs) and the row pass of the 60 000-pillar probe measured 60.5 us against 49.4 us on record.
    // The training kernels (train_pillar.hip) use the functions; tests/test_point_pillar_train_gpu.py holds the two to the same results.
    // lanes past T hold a copy of row T - 1: a duplicate row changes no maximum (and is kept out of the sums), so the 64 channels need
    // no per-lane select before the reduction
    const int tr = min(t, a.T - 1);
    const float4 pt = vf[p * a.T + tr];
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
    float f[K];
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

    float acc[kPillarC];
#pragma unroll
    for (int ch = 0; ch < kPillarC; ++ch) acc[ch] = S[ch];
    // one row of W (64 scalar registers) per trip of a rolled loop: unrolled, all K rows' loads are hoisted to the top and 400 - 700
    // scalar registers spill.  The trip's feature is picked by wave-uniform selects (K - 1 against 64 fused multiply-adds).
#pragma unroll 1
    for (int i = 0; i < K; ++i) {
        float fi = f[0];
#pragma unroll
        for (int j = 1; j < K; ++j) fi = i == j ? f[j] : fi;
        const float* __restrict__ wr = W + i * kPillarC;
#pragma unroll
        for (int ch = 0; ch < kPillarC; ++ch) acc[ch] = fmaf(fi, wr[ch], acc[ch]);
    }
    // maximum over the 32 lanes, transposing: after the xor-16 step a lane keeps channels [32 b4, +32), then [.. + 16 b3, +16), [.. + 8 b2, +8)
    const bool b4 = (t & 16) != 0, b3 = (t & 8) != 0, b2 = (t & 4) != 0;
    float u[32], v[16], r[8];
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
    // ReLU after the maximum (they commute; 8 values per lane instead of 64).  A dense row of a pillar with n_p <= 0 (mean = x / 0 in
    // the reference) is written as zeros.
#pragma unroll
    for (int ch = 0; ch < 8; ++ch) r[ch] = n_p > 0 ? fmaxf(r[ch], 0.f) : 0.f;
    // the four lanes of a group hold the same 8 channels 8g .. 8g + 7
    T* dstp = out + dst * kPillarC + 8 * ((t >> 2) & 7);
    const int q = t & 3;
    if constexpr (Elem<T>::kIsBf16) {
        if (q == 0) *(uint4*)dstp = f32_to_chunk<T>(r);
    } else {
        float h[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) h[e] = q ? r[4 + e] : r[e];
        if (q < 2) *(uint4*)(dstp + 4 * q) = f32_to_chunk<T>(h);
    }
}

// Every 16-byte chunk of the canvas <- 0, and the agent mask of regroup (fuse_utils.py:38: slot l of sample b is present when
// l < record_len[b]) when the canvas is a regrouped one.
__global__ __launch_bounds__(256) void canvas_clear_kernel(uint4* __restrict__ out, long chunks, const int* __restrict__ record_len,
                                                           float* __restrict__ mask, int B, int max_cav) {
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long stride = (long)gridDim.x * 256;
    if (mask && i < (long)B * max_cav) {
        const int b = (int)(i / max_cav), l = (int)(i - (long)b * max_cav);
        mask[i] = l < record_len[b] ? 1.f : 0.f;
    }
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (; i < chunks; i += stride) out[i] = z;
}

// PointPillarScatter on given rows: 16-byte chunk j of row p -> chunk j of cell (n, y, x); skipped rows as canvas_row says.
__global__ __launch_bounds__(256) void scatter_rows_kernel(const uint4* __restrict__ rows, const int4* __restrict__ coords,
                                                           uint4* __restrict__ out, long P, int cpr, int N, int ny, int nx) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long p = i / cpr;
    if (p >= P) return;
    const int j = (int)(i - p * cpr);
    const long dst = canvas_row(coords[p], nullptr, N, 0, 0, ny, nx);
    if (dst < 0) return;
    out[dst * cpr + j] = rows[i];
}

static int clear_canvas(void* out, long bytes, const int* record_len, float* mask, int B, int max_cav, hipStream_t stream) {
    const long chunks = bytes / 16;
    long blocks = (chunks + 255) / 256;
    const long mask_blocks = mask ? ((long)B * max_cav + 255) / 256 : 0;
    if (blocks > 4096) blocks = 4096;                          // grid-stride past 16 workgroups per CU
    if (blocks < mask_blocks) blocks = mask_blocks;
    if (blocks < 1 || blocks > 0x7fffffffL) return COBEVT_ERR_SHAPE;
    hipLaunchKernelGGL(canvas_clear_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (uint4*)out, chunks, record_len, mask, B, max_cav);
    return cobevt::launch_status();
}

template <typename T, bool kAbs, bool kDist>
static int launch_pillar(const float* vf, const int* npts, const int* coords, const float* w, const float* shift, const int* record_len,
                         void* out, const PillarArgs& a, hipStream_t stream) {
    const long blocks = (a.P + 7) / 8;
    if (blocks > 0x7fffffffL) return COBEVT_ERR_SHAPE;
    hipLaunchKernelGGL((pillar_vfe_kernel<T, kAbs, kDist>), dim3((unsigned)blocks), dim3(256), 0, stream, (const float4*)vf, npts,
                       (const int4*)coords, w, shift, record_len, (T*)out, a);
    return cobevt::launch_status();
}

}  // namespace cobevt

using namespace cobevt;

// dims: [P, T, F, K, use_absolute_xyz, with_distance, dtype, rows, N, B, max_cav, ny, nx] ; geom: [voxel x, y, z, offset x, y, z]
extern "C" int cobevt_pillar_vfe(const float* voxel_features, const int* voxel_num_points, const int* voxel_coords, const float* w,
                                 const float* shift, const int* record_len, void* out, float* cav_mask, const int* dims,
                                 const float* geom, hipStream_t stream) {
    if (!dims || !geom || !out || !w || !shift) return COBEVT_ERR_ARG;
    PillarArgs a;
    a.P = dims[0]; a.T = dims[1];
    const int F = dims[2], K = dims[3], use_abs = dims[4], dist = dims[5], dtype = dims[6];
    a.rows = dims[7]; a.N = dims[8]; a.B = dims[9]; a.max_cav = dims[10]; a.ny = dims[11]; a.nx = dims[12];
    a.vx = geom[0]; a.vy = geom[1]; a.vz = geom[2]; a.xoff = geom[3]; a.yoff = geom[4]; a.zoff = geom[5];
    if (dtype != 0 && dtype != 1) return COBEVT_ERR_ARG;
    if (a.P < 0 || a.T < 1 || a.T > 32 || F != 4 || K != (use_abs ? 4 : 1) + 6 + (dist ? 1 : 0)) return COBEVT_ERR_SHAPE;
    if (a.P > 0 && (!voxel_features || !voxel_num_points || !voxel_coords)) return COBEVT_ERR_ARG;
    if (((uintptr_t)voxel_features | (uintptr_t)voxel_coords | (uintptr_t)out) & 15) return COBEVT_ERR_SHAPE;
    if (!a.rows) {
        if (a.N < 1 || a.ny < 1 || a.nx < 1) return COBEVT_ERR_SHAPE;
        long slots = a.N;
        if (record_len) {
            if (!cav_mask) return COBEVT_ERR_ARG;
            if (a.B < 1 || a.max_cav < 1) return COBEVT_ERR_SHAPE;
            slots = (long)a.B * a.max_cav;
        } else {
            a.B = 0; a.max_cav = 0;
        }
        const long bytes = slots * a.ny * a.nx * kPillarC * (dtype == 0 ? 2 : 4);
        const int rc = clear_canvas(out, bytes, record_len, record_len ? cav_mask : nullptr, a.B, a.max_cav, stream);
        if (rc != COBEVT_OK) return rc;
    }
    if (a.P == 0) return COBEVT_OK;
    const int which = (dtype << 2) | ((use_abs ? 1 : 0) << 1) | (dist ? 1 : 0);
    switch (which) {
        case 0: return launch_pillar<bf16_t, false, false>(voxel_features, voxel_num_points, voxel_coords, w, shift, record_len, out, a, stream);
        case 1: return launch_pillar<bf16_t, false, true>(voxel_features, voxel_num_points, voxel_coords, w, shift, record_len, out, a, stream);
        case 2: return launch_pillar<bf16_t, true, false>(voxel_features, voxel_num_points, voxel_coords, w, shift, record_len, out, a, stream);
        case 3: return launch_pillar<bf16_t, true, true>(voxel_features, voxel_num_points, voxel_coords, w, shift, record_len, out, a, stream);
        case 4: return launch_pillar<float, false, false>(voxel_features, voxel_num_points, voxel_coords, w, shift, record_len, out, a, stream);
        case 5: return launch_pillar<float, false, true>(voxel_features, voxel_num_points, voxel_coords, w, shift, record_len, out, a, stream);
        case 6: return launch_pillar<float, true, false>(voxel_features, voxel_num_points, voxel_coords, w, shift, record_len, out, a, stream);
        default: return launch_pillar<float, true, true>(voxel_features, voxel_num_points, voxel_coords, w, shift, record_len, out, a, stream);
    }
}

extern "C" int cobevt_scatter_rows(const void* rows, const int* voxel_coords, void* out, int dtype, long P, int C, int N, int ny, int nx,
                                   hipStream_t stream) {
    if (!out) return COBEVT_ERR_ARG;
    if (dtype != 0 && dtype != 1) return COBEVT_ERR_ARG;
    const int eb = dtype == 0 ? 2 : 4;
    if (P < 0 || C < 1 || (C * eb) % 16 || N < 1 || ny < 1 || nx < 1) return COBEVT_ERR_SHAPE;
    if (P > 0 && (!rows || !voxel_coords)) return COBEVT_ERR_ARG;
    if (((uintptr_t)rows | (uintptr_t)voxel_coords | (uintptr_t)out) & 15) return COBEVT_ERR_SHAPE;
    const int cpr = C * eb / 16;
    const int rc = clear_canvas(out, (long)N * ny * nx * C * eb, nullptr, nullptr, 0, 0, stream);
    if (rc != COBEVT_OK || P == 0) return rc;
    const long blocks = (P * cpr + 255) / 256;
    if (blocks > 0x7fffffffL) return COBEVT_ERR_SHAPE;
    hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const uint4*)rows, (const int4*)voxel_coords,
                       (uint4*)out, P, cpr, N, ny, nx);
    return cobevt::launch_status();
}
