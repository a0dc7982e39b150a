// Dense-row GEMM for K <= 512, the row chain's way (gfx950, bf16):
//   out[m][n] = act( f(A[m][:]) . W[n][:] + bias[n] + residual[m][n] ),   f = LayerNorm | per-channel affine (+ReLU) | id
// reference: the same Linear / 1x1-conv sites as gemm_rows.hip (to_q / to_k / to_v / to_qkv behind a LayerNorm, feature_proj /
// feature_linear behind BN + ReLU, the Bottleneck 1x1 convs; fax_modules.py:193-203,283-300,472, swap_fusion_modules.py:93).
//
// gemm_rows.hip stages a 128 x 128 weight tile through LDS per workgroup and runs load -> LDS -> MFMA -> staging -> store as
// serial phases of two co-resident 8-wave workgroups; its s_memtime trace is dominated by the per-CU load / store pipes and
// the phases do not overlap.  The fused row chain (row_chain.hip) moves the same kind of GEMM 2-3x faster per phase with
// 32-row workgroups of 4 waves whose weights arrive as MFMA fragments straight from L2 (one coalesced 1-KB load per wave and
// k-group, host-side re-layout, no weight LDS) and whose many small workgroups per CU overlap each other's phases.  This
// kernel is that structure for a single GEMM: 32 rows per workgroup (8 threads per row stage + normalise the A rows into
// LDS), wave w owns columns [32w, 32w+32) of every 128-column pass with the next pass's fragments in flight (two register
// sets), D = W.X^T so a lane owns one row and runs of four consecutive columns (bias / residual / activation in registers),
// results leave through a bf16 LDS tile as 16-byte coalesced stores.
#include "bev_query.hpp"
#include "wave_ops.hpp"

namespace cobevt {

// Gr3Params: rows_launch.hpp.  LDS: A rows [32][Kp * 2 + 16] | output tile [32][272] | N_p floats of bias (rows_select.hpp: g3_lds)

// ROWS = 32 (4 waves) or 64 (8 waves = 2 row halves x 4 column tiles: every weight fragment serves twice the rows)
template <bool EMB, int ROWS = 32>
__global__ __launch_bounds__(ROWS * 8, 4) void gemm_rows3_kernel(Gr3Params p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int arow = p.Kp * 2 + 16;
    unsigned char* As = smem;
    unsigned char* Ys = smem + ROWS * arow;
    float* sb = (float*)(Ys + ROWS * kG3Row);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wn = wave & 3, wm = wave >> 2;
    const int h = lane >> 5, ql = lane & 31;
    const int m0 = blockIdx.x * ROWS;
    const int row = wm * 32 + ql;
    const bool row_ok = m0 + row < p.M;
    const int npn = (p.N + 127) / 128, nkt = p.Kp >> 7, nkg = p.Kp >> 4;
    const int nsteps = npn * nkt;
    const int cbase = wn * 32 + 4 * h;

    // step s = (pass, k-tile): the eight fragments of columns [128 pass + 32 wn, +32) x k-groups [8 kt, +8)
    auto load_frags = [&](uint4 (&b)[8], int step) {
        const int pass = step / nkt, kt = step - pass * nkt;
        const uint4* src = p.wfrag + ((size_t)(pass * 4 + wn) * nkg + kt * 8) * 64 + lane;
#pragma unroll
        for (int g = 0; g < 8; ++g) b[g] = src[g * 64];
        __builtin_amdgcn_sched_barrier(0);
    };
    uint4 fa[8], fb[8];
    load_frags(fa, 0);

    // bias of all passes into LDS (zero padded), unconditional clamped loads
    for (int i = tid; i < npn * 128; i += ROWS * 8) {
        const float b = p.bias ? p.bias[i < p.N ? i : 0] : 0.f;
        sb[i] = i < p.N ? b : 0.f;
    }
    // EMB: per-channel (w_bev0, w_bev1, b_bev - w_cam . c) of this workgroup's camera (hw % 32 == 0: one camera per workgroup)
    float4* coef = (float4*)(sb + npn * 128);
    if (EMB) {
        const int bn = m0 / p.emb_hw;
        if (tid < 128) {
            float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
            const int k = tid < p.K ? tid : 0;
            const float* E = p.emb_E + (size_t)bn * 16;
            const float4 wc = *(const float4*)(p.emb_wcam + k * 4);
            c.x = p.emb_wbev[k * 2];
            c.y = p.emb_wbev[k * 2 + 1];
            c.z = p.emb_bbev[k] - (wc.x * E[3] + wc.y * E[7] + wc.z * E[11] + wc.w * E[15]);
            coef[tid] = tid < p.K ? c : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();
    }
    // ---- stage the 32 A rows: 8 threads per row, 16 channels per 128-channel tile each; LayerNorm (single tile) or the
    // per-channel pre-activation in flight
    {
        const int r = tid >> 3, sub = tid & 7;
        const bool ok = m0 + r < p.M;
        size_t arow_idx = ok ? m0 + r : 0;
        if (p.in_stride > 1) {
            const int hw = p.src_H * p.src_W;
            const int n = (int)(arow_idx / hw), rem = (int)(arow_idx - (size_t)n * hw);
            const int oy = rem / p.src_W, ox = rem - oy * p.src_W;
            arow_idx = ((size_t)n * p.in_H + (size_t)oy * p.in_stride) * p.in_W + (size_t)ox * p.in_stride;
        }
        float wx = 0.f, wy = 0.f;
        if (EMB) {                                            // x row of (b, pix); world coordinates of pix
            const int m = (int)arow_idx, bn = m / p.emb_hw, pix = m - bn * p.emb_hw;
            wx = p.emb_world[pix];
            wy = p.emb_world[p.emb_hw + pix];
            arow_idx = (size_t)(p.emb_xbcast ? 0 : bn / p.emb_n) * p.emb_hw + pix;
        }
        const bf16_t* src = p.in + arow_idx * p.lda;
        if (p.navg > 1) {
            const long bb = (long)arow_idx / p.avg_rows_per_batch, rr = (long)arow_idx - bb * p.avg_rows_per_batch;
            src = p.in + bb * p.avg_batch_stride + rr * p.lda;
        }
        for (int kt = 0; kt < nkt; ++kt) {
            const int kb = kt * 128 + sub * 16;
            uint4 raw[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) raw[j] = *(const uint4*)(src + (kb + j * 8 < p.K ? kb + j * 8 : 0));
            float v[16];
            chunk_to_f32<bf16_t>(raw[0], v);
            chunk_to_f32<bf16_t>(raw[1], v + 8);
            if (p.navg > 1) {
                for (int a = 1; a < p.navg; ++a) {
                    float u[16];
                    const bf16_t* sa = src + a * p.avg_stride;
                    chunk_to_f32<bf16_t>(*(const uint4*)(sa + (kb < p.K ? kb : 0)), u);
                    chunk_to_f32<bf16_t>(*(const uint4*)(sa + (kb + 8 < p.K ? kb + 8 : 0)), u + 8);
#pragma unroll
                    for (int e = 0; e < 16; ++e) v[e] += u[e];
                }
                const float inv = 1.0f / (float)p.navg;
#pragma unroll
                for (int e = 0; e < 16; ++e) v[e] *= inv;
            }
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (!ok || kb + e >= p.K) v[e] = 0.f;
            if (EMB) {                                        // single tile (K <= 128): v holds x, add the normalised embedding
                float em[16], ss = 0.f;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float4 c = coef[kb + e];
                    em[e] = (kb + e) < p.K ? (c.x * wx + c.y * wy + c.z) : 0.f;
                    ss += em[e] * em[e];
                }
                ss = lane8_sum(ss);
                const float inv = 1.0f / (sqrtf(ss) + 1e-7f);
#pragma unroll
                for (int e = 0; e < 16; ++e) v[e] = ok ? em[e] * inv + v[e] : 0.f;
                // rounded exactly as cobevt_fax_bev_embed would have stored the query, then normalised
                chunk_to_f32<bf16_t>(f32_to_chunk<bf16_t>(v), v);
                chunk_to_f32<bf16_t>(f32_to_chunk<bf16_t>(v + 8), v + 8);
            }
            if (p.ln) {                                   // Kp == 128 (checked by the entry point): the row is here
                // (the 8-lane sums stay written out here: through lane8_sum the compiler schedules this kernel differently)
                float s = 0.f;
#pragma unroll
                for (int e = 0; e < 16; ++e) s += v[e];
                s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 4, 64);
                const float mean = s / (float)p.K;
                float q = 0.f;
#pragma unroll
                for (int e = 0; e < 16; ++e) { const float d = (kb + e) < p.K ? v[e] - mean : 0.f; q += d * d; }
                q += __shfl_xor(q, 1, 64); q += __shfl_xor(q, 2, 64); q += __shfl_xor(q, 4, 64);
                const float rstd = rsqrtf(q / (float)p.K + p.ln_eps);
#pragma unroll
                for (int e = 0; e < 16; ++e) v[e] = (kb + e) < p.K ? (v[e] - mean) * rstd : 0.f;
            } else if (p.pre_scale) {
#pragma unroll
                for (int e = 0; e < 16; e += 4) {
                    const int k = kb + e;
                    const float4 sc = *(const float4*)(p.pre_scale + (k < p.K ? k : 0)), sh = *(const float4*)(p.pre_shift + (k < p.K ? k : 0));
                    const float x0 = v[e] * sc.x + sh.x, x1 = v[e + 1] * sc.y + sh.y, x2 = v[e + 2] * sc.z + sh.z, x3 = v[e + 3] * sc.w + sh.w;
                    const bool in = ok && k < p.K;                  // K % 8 == 0: a run of four is inside or outside
                    v[e] = in ? (p.pre_relu ? fmaxf(x0, 0.f) : x0) : 0.f;
                    v[e + 1] = in ? (p.pre_relu ? fmaxf(x1, 0.f) : x1) : 0.f;
                    v[e + 2] = in ? (p.pre_relu ? fmaxf(x2, 0.f) : x2) : 0.f;
                    v[e + 3] = in ? (p.pre_relu ? fmaxf(x3, 0.f) : x3) : 0.f;
                }
            }
            *(uint4*)(As + r * arow + kb * 2) = f32_to_chunk<bf16_t>(v);
            *(uint4*)(As + r * arow + kb * 2 + 16) = f32_to_chunk<bf16_t>(v + 8);
        }
    }
    __syncthreads();

    const int abase = row * arow + h * 16;
    f32x16 acc;
    uint2 rs[4];
    auto step_body = [&](int step, const uint4 (&cur)[8], uint4 (&nxt)[8]) {
        const int pass = step / nkt, kt = step - pass * nkt;
        if (step + 1 < nsteps) load_frags(nxt, step + 1);
        if (kt == 0) {
            // residual pieces of this lane's (row, column runs): in flight under the MFMAs
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int col0 = pass * 128 + cbase + 8 * k;
                const bool ok = p.residual && row_ok && col0 < p.N;
                rs[k] = make_uint2(0, 0);
                if (p.residual) rs[k] = *(const uint2*)(p.residual + (ok ? (size_t)(m0 + row) * p.N + col0 : 0));
                if (!ok) rs[k] = make_uint2(0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        }
        const int kleft = p.K - kt * 128;
        const int ng = kleft >= 128 ? 8 : (kleft * 2 + 31) / 32;
#pragma unroll
        for (int g = 0; g < 8; ++g)
            if (g < ng) {
                const uint4 af = *(const uint4*)(As + abase + (kt * 8 + g) * 32);
                mfma_kgroup<bf16_t>(cur[g], af, acc);
            }
        if (kt + 1 < nkt) return;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int col0 = pass * 128 + cbase + 8 * k;
            const float4 b = *(const float4*)(sb + col0);
            float v0 = acc[4 * k] + b.x + bf2f(rs[k].x & 0xffff), v1 = acc[4 * k + 1] + b.y + bf2f(rs[k].x >> 16);
            float v2 = acc[4 * k + 2] + b.z + bf2f(rs[k].y & 0xffff), v3 = acc[4 * k + 3] + b.w + bf2f(rs[k].y >> 16);
            if (p.act) { v0 = apply_act<bf16_t>(v0, p.act); v1 = apply_act<bf16_t>(v1, p.act); v2 = apply_act<bf16_t>(v2, p.act); v3 = apply_act<bf16_t>(v3, p.act); }
            *(uint2*)(Ys + row * kG3Row + (cbase + 8 * k) * 2) = make_uint2(pack_bf2(v0, v1), pack_bf2(v2, v3));
        }
        __syncthreads();                              // ROWS x 128 result staged in Ys
        {
            const int r = tid >> 3, sub = tid & 7;
            if (m0 + r < p.M) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int c0 = pass * 128 + sub * 16 + j * 8;
                    if (c0 < p.N) *(uint4*)(p.out + (size_t)(m0 + r) * p.N + c0) = *(const uint4*)(Ys + r * kG3Row + sub * 32 + j * 16);
                }
            }
        }
        if (pass + 1 < npn) __syncthreads();          // Ys is rewritten by the next pass
    };
    for (int step = 0; step < nsteps; step += 2) {
        step_body(step, fa, fb);
        if (step + 1 < nsteps) step_body(step + 1, fb, fa);
    }
}

// the kernel's parameter block of a parsed call; the pointers are the caller's
static Gr3Params gr3_params(const RowsGemmShape& s, const void* in, const void* wfrag, const float* bias, void* out, float ln_eps) {
    Gr3Params p = {};
    p.in = (const bf16_t*)in; p.wfrag = (const uint4*)wfrag; p.bias = bias; p.out = (bf16_t*)out;
    p.M = s.M; p.N = s.N; p.K = s.K; p.Kp = s.Kp; p.lda = s.lda;
    p.pre_relu = s.pre_relu; p.act = s.act; p.ln = s.ln; p.ln_eps = ln_eps;
    p.in_stride = s.in_stride; p.src_H = s.src_H; p.src_W = s.src_W; p.in_H = s.in_H; p.in_W = s.in_W;
    p.emb_n = s.emb_n; p.emb_hw = s.emb_hw; p.emb_xbcast = s.emb_xbcast;
    p.navg = s.navg; p.avg_rows_per_batch = s.avg_rows_per_batch; p.avg_stride = s.avg_stride; p.avg_batch_stride = s.avg_batch_stride;
    return p;
}

static int launch_gr3(const Gr3Params& p, const RowsLaunch& l, hipStream_t stream) {
    switch (l.family) {
        case ROWS_GEMM3_F32: return launch_linear_rows_f32(p, l, stream);
        case ROWS_LN_LINEAR64: return launch_ln_linear64(p, l, stream);
        default:
            if (l.ROWS == 64) return launch_rows<gemm_rows3_kernel<false, 64>>(l, g3_lds(64, 512, 4096), stream, p);
            if (!l.EMB) return launch_rows<gemm_rows3_kernel<false, 32>>(l, 0, stream, p);
            return launch_rows<gemm_rows3_kernel<true, 32>>(l, 0, stream, p);
    }
}

}  // namespace cobevt

using namespace cobevt;

// C-ABI entry point, see include/cobevt_hip.h.  fp32 storage: the tensor pointers travel in the same block (gemm_rows3_f32.hip casts them back)
extern "C" int cobevt_linear_rows_small_k(const void* in, const void* wfrag, const float* bias, const void* residual,
                                          const float* pre_scale, const float* pre_shift, void* out, const long* dims, float ln_eps,
                                          hipStream_t stream) {
    RowsGemmShape s;
    const int rc = small_k_parse(dims, in && wfrag && out, residual != nullptr, pre_scale != nullptr, pre_shift != nullptr, s);
    if (rc != COBEVT_OK) return rc;
    Gr3Params p = gr3_params(s, in, wfrag, bias, out, ln_eps);
    p.residual = (const bf16_t*)residual; p.pre_scale = pre_scale; p.pre_shift = pre_shift;
    return launch_gr3(p, small_k_select(s, rows_gates()), stream);
}

// C-ABI entry point, see include/cobevt_hip.h
extern "C" int cobevt_bev_embed_linear_rows_small_k(const float* E_inv, const float* world, const float* w_bev, const float* b_bev,
                                                    const float* w_cam, const void* x, const void* wfrag, const float* bias, void* out,
                                                    const long* dims, float ln_eps, hipStream_t stream) {
    RowsGemmShape s;
    const int rc = bev_embed_parse(dims, E_inv && world && w_bev && b_bev && w_cam && x && wfrag && out, s);
    if (rc != COBEVT_OK) return rc;
    const RowsLaunch l = bev_embed_select(s);
    if (l.family == ROWS_BEV_QUERY) {
        BevQueryParams q;
        q.E_inv = E_inv; q.world = world; q.w_bev = w_bev; q.b_bev = b_bev; q.w_cam = w_cam; q.x = (const bf16_t*)x;
        q.wfrag = (const uint4*)wfrag; q.bias = bias; q.out = (bf16_t*)out;
        q.B = s.emb_B; q.n = s.emb_n; q.hw = s.emb_hw; q.x_bcast = s.emb_xbcast; q.ln_eps = ln_eps;
        return launch_bev_query(q, l, stream);
    }
    Gr3Params p = gr3_params(s, x, wfrag, bias, out, ln_eps);
    p.emb_E = E_inv; p.emb_world = world; p.emb_wbev = w_bev; p.emb_bbev = b_bev; p.emb_wcam = w_cam;
    return launch_gr3(p, l, stream);
}

// C-ABI entry point, see include/cobevt_hip.h: out (B * R, N) = act(LayerNorm?(mean_j in[b][j][r][:]) . W^T + bias), in (B, L, R, K)
extern "C" int cobevt_mean_linear_rows_small_k(const void* in, const void* wfrag, const float* bias, void* out, const long* dims,
                                               float ln_eps, hipStream_t stream) {
    RowsGemmShape s;
    const int rc = mean_parse(dims, in && wfrag && out, s);
    if (rc != COBEVT_OK) return rc;
    return launch_gr3(gr3_params(s, in, wfrag, bias, out, ln_eps), mean_select(s), stream);
}
