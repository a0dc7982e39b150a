// Launch side of the row-local kernels: csrc/rows_select.hpp decides, the kernel files map its RowsLaunch to an instantiation and hand
// it to launch_rows.  Also what gemm_rows3.hip shares with the files it dispatches to: its parameter block and their launchers.
#pragma once
#include "common.hpp"
#include "rows_select.hpp"

namespace cobevt {

// max_lds: the dynamic-LDS limit the kernel is opted into (0: it never asks for more than the default 64 KB)
template <auto Kernel, class... Args> int launch_rows(const RowsLaunch& l, size_t max_lds, hipStream_t stream, Args... args) {
    if (max_lds) allow_dynamic_lds<Kernel>((int)max_lds);
    hipLaunchKernelGGL(Kernel, dim3(l.grid), dim3(l.block), l.lds, stream, args...);
    return launch_status();
}

struct Gr3Params {
    const bf16_t* in;       // [M][lda]
    const uint4* wfrag;     // fragment-ordered [N_p/32][8][64 lanes][16 B]
    const float* bias;      // [N] or null
    const bf16_t* residual; // [M][N] or null
    const float* pre_scale; // [K] or null (with pre_shift)
    const float* pre_shift;
    bf16_t* out;            // [M][N]
    int M, N, K, Kp;        // Kp = K rounded up to 128 (<= 512): the fragment array has Kp / 16 k-groups per 32-column tile
    long lda;
    int pre_relu, act, ln;
    float ln_eps;
    int in_stride, src_H, src_W, in_H, in_W;   // in_stride > 1: row m = (n, oy, ox) of an (src_H, src_W) map reads input pixel
                                               // (oy * in_stride, ox * in_stride) of an (in_H, in_W) map (1x1 / stride-2 conv)
    // EMB: the A rows are the BEV query  x[b][pix] + L2norm_c(w_bev . world[pix] + b_bev - w_cam . E_inv[b, cam][:, 3])
    // (fax_modules.py:370-375,387-388) of row m = ((b * n + cam) * hw + pix), produced while staging; `in` is x (B | 1, hw, K)
    const float* emb_E; const float* emb_world; const float* emb_wbev; const float* emb_bbev; const float* emb_wcam;
    int emb_n, emb_hw, emb_xbcast;
    // navg > 1: A row m = (b, r) is the MEAN of the navg rows in[b * avg_batch_stride + j * avg_stride + r * lda], j < navg
    // (SwapFusionEncoder.mlp_head: Reduce('b m d h w -> b d h w', 'mean') -> LayerNorm -> Linear, swap_fusion_modules.py:275-281)
    int navg, avg_rows_per_batch;
    long avg_stride, avg_batch_stride;
};

// gemm_rows3_f32.hip: cobevt_linear_rows_small_k for fp32 storage (p's pointers are fp32 tensors; Kp = K rounded up to 64)
int launch_linear_rows_f32(const Gr3Params& p, const RowsLaunch& l, hipStream_t stream);
// ln_linear64.hip: LayerNorm + Linear on 64-channel rows of a big map as independent waves
int launch_ln_linear64(const Gr3Params& p, const RowsLaunch& l, hipStream_t stream);

}  // namespace cobevt
