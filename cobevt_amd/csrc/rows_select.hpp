// Row-local routing: which kernel the row chain after an attention, the FAX projection chain and the small-K dense-row GEMMs
// launch, on which grid, decided by plain integer arithmetic on the launch parameters.  This header owns that decision and has no
// HIP dependency (standard library + the public header's status codes), so tests/test_rows_select.py pins it on the CPU against
// tests/golden/rows_select/.
//   chain_parse / proj_parse / small_k_parse / bev_embed_parse / mean_parse
//                  dims + null-ness of the pointers -> ChainShape / RowsGemmShape, or the entry point's error code
//   chain_select / proj_select / small_k_select / bev_embed_select / mean_select
//                  shape (+ RowsGates) -> RowsLaunch (kernel instantiation, grid, block, LDS, block count of the persistent kernels)
// row_chain.hip, row_chain64.hip, row_chain_f32.hip, proj_chain128.hip, gemm_rows3.hip, gemm_rows3_f32.hip, ln_linear64.hip and
// bev_query.hip only map a RowsLaunch to its instantiation and launch it.
#pragma once
#include <stddef.h>
#include <stdlib.h>
#include "../../include/cobevt_hip.h"

namespace cobevt {

// The A/B switches of the wave-level kernels, read from the environment once per process (rows_gates):
//   COBEVT_RC64_PREFETCH  row_chain64_kernel: 1 (default) = the next block's a / skip rows requested under the current block's chain,
//                         four waves per workgroup; 2 = the same prefetch with six waves; anything else (0) = six waves, no prefetch
//   COBEVT_LN_LINEAR64=0  LayerNorm + Linear on big 64-channel maps through the generic dense-row kernel instead of ln_linear64_kernel
//   COBEVT_LN64_BLOCKS=n  caps ln_linear64_kernel's persistent grid (n > 0; default 1536 = six workgroups per CU)
struct RowsGates { int rc64_prefetch; bool ln_linear64; int ln64_blocks; };

inline const RowsGates& rows_gates() {
    static const RowsGates g = [] {
        const char* pf = getenv("COBEVT_RC64_PREFETCH");
        const char* on = getenv("COBEVT_LN_LINEAR64");
        const char* cap = getenv("COBEVT_LN64_BLOCKS");
        return RowsGates{pf ? atoi(pf) : 1, !(on && on[0] == '0'), cap && atoi(cap) > 0 ? atoi(cap) : 1536};
    }();
    return g;
}

enum RowsFamily { ROWS_CHAIN, ROWS_CHAIN64, ROWS_CHAIN_F32, ROWS_PROJ128, ROWS_LN_LINEAR64, ROWS_GEMM3, ROWS_GEMM3_F32, ROWS_BEV_QUERY };

// One kernel launch.  Template tuple by family (fields of the other families stay 0):
//   CHAIN         row_chain_kernel<NPASS, ROWS, FULL, MLP>      CHAIN64      row_chain64_kernel<NNT, NW, PF>
//   CHAIN_F32     row_chain_f32_kernel                          PROJ128      proj_chain128_kernel<NNT, NW>
//   LN_LINEAR64   ln_linear64_kernel<NNT, NW>                   GEMM3        gemm_rows3_kernel<EMB, ROWS>
//   GEMM3_F32     gemm_rows3_f32_kernel                         BEV_QUERY    bev_query_kernel<NW>
struct RowsLaunch {
    int status;               // COBEVT_OK, or the entry point's error code (nothing is launched)
    RowsFamily family;
    int NPASS, ROWS, NNT, NW;
    bool FULL, MLP, PF, EMB;
    unsigned grid;
    int block;
    size_t lds;
    int nblk;                 // 32-row blocks the persistent kernels walk (their trailing argument), else 0
};

// ---- constants the kernels share with the selection (each kernel file ties its device-side LDS struct to these with a static_assert)
constexpr int kRcBnMax = 768;                       // row_chain.hip: floats of the bias table behind the next projection's bias
constexpr int kRcF32BnMax = 768;                    // row_chain_f32.hip: the same
constexpr int kPcMaxNnt = 8;                        // proj_chain128.hip: 32-column tiles of Wn that fit its LDS
constexpr int kBqMaxCams = 32;                      // bev_query.hip: B * n cameras whose offsets fit the LDS table
constexpr int kG3Row = 256 + 16;                    // gemm_rows3.hip: staged output row, 128 bf16 + pad
constexpr int kG3Rows = 32;
constexpr int kG3fRows = 32;                        // gemm_rows3_f32.hip
constexpr int kG3fYRow = 512 + 16;                  // ... staged output row, 128 fp32 + pad
constexpr size_t rc_lds(int rows) { return (size_t)rows * 1072 + 6144; }     // RcLds<ROWS>::BYTES: 40,448 (four workgroups per CU) / 74,752
constexpr size_t kRcF32Lds = 73216, kRc64Lds = 67840, kPc128Lds = 100864, kBqLds = 51712;
// gemm_rows3_kernel: A rows [rows][Kp * 2 + 16] | output tile [rows][272] | N_p floats of bias (| the embed form's 2 KB operand table)
constexpr size_t g3_lds(int rows, int Kp, int N, size_t extra = 0) {
    return (size_t)rows * (Kp * 2 + 16) + (size_t)rows * kG3Row + (size_t)((N + 127) / 128) * 128 * 4 + extra;
}
constexpr size_t g3f_lds(int Kp, int N) { return (size_t)kG3fRows * (Kp * 4 + 16) + (size_t)kG3fRows * kG3fYRow + (size_t)((N + 127) / 128) * 128 * 4; }

inline RowsLaunch rows_fail(int code) { RowsLaunch l = {}; l.status = code; return l; }
inline RowsLaunch rows_launch(RowsFamily family, long work, int per_block, int block, size_t lds) {
    RowsLaunch l = {};
    l.status = COBEVT_OK; l.family = family;
    l.grid = (unsigned)((work + per_block - 1) / per_block); l.block = block; l.lds = lds;
    return l;
}
// persistent wave-level kernels: NW waves per workgroup walk nblk 32-row blocks, at most `cap` workgroups
inline RowsLaunch rows_persistent(RowsFamily family, int nblk, int NNT, int NW, int cap, size_t lds) {
    const int blocks = (nblk + NW - 1) / NW;
    RowsLaunch l = rows_launch(family, blocks > cap ? cap : blocks, 1, NW * 64, lds);
    l.NNT = NNT; l.NW = NW; l.nblk = nblk;
    return l;
}

// ---------------------------------------------------------------- cobevt_attn_mlp_chain / cobevt_proj_chain
struct ChainShape {
    int dtype, M, C, Hd, Hdp, Nn, next_ln, next_act, skip_rows, pre_relu;
    int variant;              // attn_mlp_chain: rows per workgroup (0 = automatic; 32 / 64 pin the generic kernel); proj_chain: 0 =
                              // automatic, 1 = the barrier-phased kernel
    bool has_skip, has_next;
};

// dims: [dtype, M, C, Hd, Hdp, Nn, next_ln, next_act, rows_per_workgroup, skip_rows]; required = a, out, wp, w1, b1, w2, b2 all given
inline int chain_parse(const int* dims, bool required, bool has_skip, bool has_post_g, bool has_post_b, bool has_wnext, bool has_out_next,
                       ChainShape& s) {
    s = ChainShape{};
    if (!required || !dims) return COBEVT_ERR_ARG;
    if (dims[0] != 0 && dims[0] != 1) return COBEVT_ERR_ARG;
    s.dtype = dims[0]; s.M = dims[1]; s.C = dims[2]; s.Hd = dims[3]; s.Hdp = dims[4];
    s.Nn = dims[5]; s.next_ln = dims[6]; s.next_act = dims[7]; s.variant = dims[8];
    s.skip_rows = dims[9] > 0 ? dims[9] : s.M;                 // dims[9]: rows of `skip` (0 = M), M % skip_rows == 0
    s.has_skip = has_skip; s.has_next = has_wnext;
    const bool xor_ptrs = has_post_g != has_post_b || has_wnext != has_out_next;
    if (s.dtype == 1) {       // fp32 storage: widths are chain_select's business (other widths run the GEMMs separately: UNSUPPORTED)
        if (xor_ptrs) return COBEVT_ERR_ARG;
        if (s.M < 1 || s.skip_rows > s.M || s.M % s.skip_rows || (has_wnext && (s.next_act < 0 || s.next_act > 2))) return COBEVT_ERR_SHAPE;
        return COBEVT_OK;
    }
    if (s.M < 1 || s.C < 8 || s.C > 128 || s.C % 8 || s.Hd < 8 || s.Hd > 256 || s.Hd % 8) return COBEVT_ERR_SHAPE;
    if (s.Hdp % 128 || s.Hdp < s.Hd || s.Hdp > 256) return COBEVT_ERR_SHAPE;
    if (s.skip_rows > s.M || s.M % s.skip_rows) return COBEVT_ERR_SHAPE;
    if (xor_ptrs) return COBEVT_ERR_ARG;
    if (has_wnext && (s.Nn < 8 || s.Nn % 8 || s.Nn > kRcBnMax || s.next_act < 0 || s.next_act > 2)) return COBEVT_ERR_SHAPE;
    return COBEVT_OK;
}

inline RowsLaunch chain_generic(const ChainShape& s, int rows, bool mlp) {
    RowsLaunch l = rows_launch(ROWS_CHAIN, s.M, rows, rows * 8, rc_lds(rows));
    l.NPASS = s.Hd > 128 ? 2 : 1; l.ROWS = rows; l.FULL = s.C == 128; l.MLP = mlp;
    return l;
}

inline RowsLaunch chain_select(const ChainShape& s, const RowsGates& gates) {
    if (s.dtype == 1) {       // the C = 128 / hidden 256 chain (row_chain_f32.hip)
        if (s.C != 128 || s.Hd != 256 || s.Hdp != 256) return rows_fail(COBEVT_ERR_UNSUPPORTED);
        if (s.has_next && (s.Nn < 4 || s.Nn % 4 || s.Nn > kRcF32BnMax)) return rows_fail(COBEVT_ERR_UNSUPPORTED);
        return rows_launch(ROWS_CHAIN_F32, s.M, 32, 256, kRcF32Lds);
    }
    // automatic: 64-channel chains with a 128-wide hidden layer and a full skip on big maps take the persistent form (row_chain64.hip;
    // small maps: the generic kernel's finer workgroups fill the chip better), two workgroups per CU walking the 32-row blocks.
    // Same-job A/B on the LiDAR FuseBEVT workload (profiles/r06_rc64_prefetch_ab.txt): the next block's rows prefetched under the
    // current block's chain, 2 x 4 waves per CU at 192 VGPRs - 102 -> 87 us per launch (370 MB: 3.6 -> 4.25 TB/s), 525 -> 538 frames/s;
    // the same prefetch with six waves per workgroup (one workgroup per CU fits) 103 us; without it 2 x 6 waves per CU = 3 per SIMD.
    const int nnt = s.has_next ? s.Nn / 32 : 0;
    if (s.variant == 0 && s.C == 64 && s.Hd == 128 && s.Hdp == 128 && s.has_skip && s.skip_rows == s.M && s.M >= 16384 &&
        (!s.has_next || (s.Nn % 32 == 0 && s.Nn <= 192)) && (nnt == 0 || nnt == 2 || nnt == 4 || nnt == 6)) {
        const bool pf = gates.rc64_prefetch == 1 || gates.rc64_prefetch == 2;
        RowsLaunch l = rows_persistent(ROWS_CHAIN64, (s.M + 31) / 32, nnt, gates.rc64_prefetch == 1 ? 4 : 6, 512, kRc64Lds);
        l.PF = pf;
        return l;
    }
    return chain_generic(s, s.variant == 64 ? 64 : 32, true);
}

// dims: [dtype, M, C (= 128), Nn, next_ln, next_act, skip_rows, pre_relu, variant]; required = a, wp, wnext, bnext, out_next all given
inline int proj_parse(const int* dims, bool required, bool has_pre_scale, bool has_pre_shift, bool has_skip, ChainShape& s) {
    s = ChainShape{};
    if (!required || !dims) return COBEVT_ERR_ARG;
    if (has_pre_scale != has_pre_shift) return COBEVT_ERR_ARG;
    if (dims[0] != 0) return COBEVT_ERR_UNSUPPORTED;
    s.M = dims[1]; s.C = dims[2]; s.Hd = 8; s.Hdp = 128;
    s.Nn = dims[3]; s.next_ln = dims[4]; s.next_act = dims[5];
    s.skip_rows = dims[6] > 0 ? dims[6] : s.M;
    s.pre_relu = dims[7]; s.variant = dims[8];
    s.has_skip = has_skip; s.has_next = true;
    if (s.M < 1 || s.C != 128) return COBEVT_ERR_SHAPE;               // K = C = 128 (the level-0 feature / embedding width)
    if (s.Nn < 8 || s.Nn % 8 || s.Nn > kRcBnMax || s.next_act < 0 || s.next_act > 2) return COBEVT_ERR_SHAPE;
    if (s.skip_rows > s.M || s.M % s.skip_rows) return COBEVT_ERR_SHAPE;
    return COBEVT_OK;
}

inline RowsLaunch proj_select(const ChainShape& s) {
    // big maps: rows in registers, weights in LDS (proj_chain128.hip), one persistent workgroup of eight waves per CU; smaller maps:
    // the 32-row workgroups of the generic kernel fill the chip better
    if (s.variant == 0 && s.next_act == 0 && s.M >= 32768 && (s.Nn == 128 || s.Nn == 32 * kPcMaxNnt))
        return rows_persistent(ROWS_PROJ128, (s.M + 31) / 32, s.Nn / 32, 8, 256, kPc128Lds);
    return chain_generic(s, 32, false);
}

// ---------------------------------------------------------------- cobevt_*linear_rows_small_k
// The integer half of gemm_rows3.hip's Gr3Params (same meaning field by field); rows_gemm_neutral sets what an entry point does not use.
struct RowsGemmShape {
    int dtype, M, N, K, Kp;
    long lda;
    int pre_relu, act, ln, in_stride, src_H, src_W, in_H, in_W;
    int emb_B, emb_n, emb_hw, emb_xbcast;
    int navg, avg_rows_per_batch;
    long avg_stride, avg_batch_stride;
    int rows_hint;            // linear_rows_small_k: rows per workgroup (64; anything else = 32)
    bool plain_ln;            // LayerNorm + Linear and nothing else: no residual, affine, ReLU or row gather in front
    bool query128;            // bev_embed: the FAX level-0 shape (D = N = 128 behind a LayerNorm, whole 32-row blocks per camera)
};

inline RowsGemmShape rows_gemm_neutral() {
    RowsGemmShape s = {};
    s.Kp = 128;
    s.in_stride = s.src_H = s.src_W = s.in_H = s.in_W = 1;
    s.emb_B = s.emb_n = s.emb_hw = 1;
    s.navg = s.avg_rows_per_batch = 1;
    return s;
}

inline RowsLaunch gemm3_launch(const RowsGemmShape& s, bool emb, int rows) {
    RowsLaunch l = rows_launch(ROWS_GEMM3, s.M, rows, rows * 8, g3_lds(rows, s.Kp, s.N, emb ? 128 * 16 : 0));
    l.EMB = emb; l.ROWS = rows;
    return l;
}

// dims: [dtype, M, N, K, lda, pre_relu, act, ln, in_stride, src_H, src_W, in_H, in_W, rows_per_workgroup]; required = in, wfrag, out.
// fp32 storage (gemm_rows3_f32.hip) checks the same things in units of 4 elements, and reports every failure as UNSUPPORTED.
inline int small_k_parse(const long* dims, bool required, bool has_residual, bool has_pre_scale, bool has_pre_shift, RowsGemmShape& s) {
    s = rows_gemm_neutral();
    if (!required || !dims) return COBEVT_ERR_ARG;
    if (dims[0] != 0 && dims[0] != 1) return COBEVT_ERR_UNSUPPORTED;
    s.dtype = (int)dims[0];
    s.M = (int)dims[1]; s.N = (int)dims[2]; s.K = (int)dims[3]; s.lda = dims[4];
    s.pre_relu = (int)dims[5]; s.act = (int)dims[6]; s.ln = (int)dims[7];
    s.in_stride = (int)dims[8]; s.src_H = (int)dims[9]; s.src_W = (int)dims[10]; s.in_H = (int)dims[11]; s.in_W = (int)dims[12];
    s.rows_hint = (int)dims[13];
    const bool f32 = s.dtype == 1;
    const int ch = f32 ? 4 : 8;
    const int shape = f32 ? COBEVT_ERR_UNSUPPORTED : COBEVT_ERR_SHAPE, arg = f32 ? COBEVT_ERR_UNSUPPORTED : COBEVT_ERR_ARG;
    s.Kp = f32 ? (s.K + 63) / 64 * 64 : (s.K + 127) / 128 * 128;
    if (s.M < 1 || s.N < ch || s.N % ch || s.N > 4096 || s.K < ch || s.K > 512 || s.K % ch || s.lda < s.K || s.lda % ch) return shape;
    // LayerNorm fusion: bf16 needs the row in one 128-channel tile; fp32 has the 128-channel one of the FAX / fusion blocks only
    if (s.ln && (f32 ? s.K != 128 : s.K > 128)) return COBEVT_ERR_UNSUPPORTED;
    if (s.in_stride < 1 || (s.in_stride > 1 && (s.src_H < 1 || s.src_W < 1 || s.in_H < 1 || s.in_W < 1 || s.M % (s.src_H * s.src_W)))) return shape;
    if (s.in_stride > 1 && has_residual) return COBEVT_ERR_UNSUPPORTED;
    if (has_pre_scale != has_pre_shift) return arg;
    if (s.ln && has_pre_scale) return COBEVT_ERR_UNSUPPORTED;
    if (s.act < 0 || s.act > 4) return arg;
    s.plain_ln = s.ln && !has_residual && !has_pre_scale && !s.pre_relu && s.in_stride == 1;
    return COBEVT_OK;
}

inline RowsLaunch small_k_select(const RowsGemmShape& s, const RowsGates& gates) {
    if (s.dtype == 1) return rows_launch(ROWS_GEMM3_F32, s.M, kG3fRows, 256, g3f_lds(s.Kp, s.N));
    // LayerNorm + Linear of a big 64-channel map: independent waves (ln_linear64.hip).  Persistent: SIX co-resident workgroups per CU
    // (24.8 KB of LDS and 72 VGPRs each) walk the 32-row blocks.  Measured on the LiDAR shape (M = 524,288, N = 192): 512 workgroups
    // 90.8 us, 1024 84.2, 1536 64.8 (4.1 TB/s), 2048 (not co-resident: a tail) 79.8.
    if (s.plain_ln && gates.ln_linear64 && s.K == 64 && s.lda == 64 && s.N >= 32 && s.N <= 192 && s.N % 32 == 0 && s.M >= 65536) {
        const int nnt = s.N / 32;
        return rows_persistent(ROWS_LN_LINEAR64, (s.M + 31) / 32, nnt, 4, gates.ln64_blocks, (size_t)nnt * (4 * 1024 + 32 * 4));
    }
    return gemm3_launch(s, false, s.rows_hint == 64 ? 64 : 32);
}

// dims: [dtype(0), B, n, hw, D (= K <= 128), N, ln, x_bcast]; required = every pointer but the bias given
inline int bev_embed_parse(const long* dims, bool required, RowsGemmShape& s) {
    s = rows_gemm_neutral();
    if (!required || !dims) return COBEVT_ERR_ARG;
    if (dims[0] != 0) return COBEVT_ERR_UNSUPPORTED;
    const long B = dims[1], n = dims[2], hw = dims[3], rows = B * n * hw;
    s.K = (int)dims[4]; s.N = (int)dims[5]; s.ln = (int)dims[6];
    s.lda = s.K;
    s.emb_B = (int)B; s.emb_n = (int)n; s.emb_hw = (int)hw; s.emb_xbcast = (int)dims[7];
    // the wave-level kernel (bev_query.hip) is offered the call BEFORE the shape checks below, as it always was: hw = 0 reaches it
    // with an empty grid (a launch error, not a shape error)
    s.query128 = dims[4] == 128 && dims[5] == 128 && dims[6] && hw % 32 == 0 && B >= 1 && n >= 1 && rows <= 0x7fffffffL &&
                 (long)s.emb_B * s.emb_n <= kBqMaxCams && s.emb_B >= 1 && s.emb_n >= 1;
    if (s.query128) return COBEVT_OK;
    if (B < 1 || n < 1 || hw < 1 || hw % kG3Rows != 0 || rows > 0x7fffffffL) return COBEVT_ERR_SHAPE;    // one camera per workgroup
    if (s.N < 8 || s.N % 8 || s.N > 4096 || s.K < 8 || s.K > 128 || s.K % 8) return COBEVT_ERR_SHAPE;
    s.M = (int)rows;
    return COBEVT_OK;
}

inline RowsLaunch bev_embed_select(const RowsGemmShape& s) {
    // the FAX level-0 shape: rows never leave the registers, weights in LDS; persistent, three workgroups (12 waves) per CU
    if (s.query128) return rows_persistent(ROWS_BEV_QUERY, s.emb_B * (s.emb_hw >> 5) * s.emb_n, 0, 4, 256 * 3, kBqLds);
    return gemm3_launch(s, true, kG3Rows);
}

// dims: [dtype(0), B, L, R, K, N, ln, act]; required = in, wfrag, out given
inline int mean_parse(const long* dims, bool required, RowsGemmShape& s) {
    s = rows_gemm_neutral();
    if (!required || !dims) return COBEVT_ERR_ARG;
    if (dims[0] != 0) return COBEVT_ERR_UNSUPPORTED;
    const long B = dims[1], Lr = dims[2], R = dims[3];
    s.K = (int)dims[4]; s.N = (int)dims[5]; s.ln = (int)dims[6]; s.act = (int)dims[7];
    s.lda = s.K;
    if (B < 1 || Lr < 1 || Lr > 64 || R < 1 || B * R > 0x7fffffffL) return COBEVT_ERR_SHAPE;
    if (s.N < 8 || s.N % 8 || s.N > 4096 || s.K < 8 || s.K > 128 || s.K % 8 || s.act < 0 || s.act > 4) return COBEVT_ERR_SHAPE;
    s.M = (int)(B * R);
    s.navg = (int)Lr; s.avg_rows_per_batch = (int)R; s.avg_stride = R * s.K; s.avg_batch_stride = Lr * R * s.K;
    return COBEVT_OK;
}

inline RowsLaunch mean_select(const RowsGemmShape& s) { return gemm3_launch(s, false, kG3Rows); }

}  // namespace cobevt
