// Train mode of the LiDAR pillar front end (gfx950): Linear -> BatchNorm1d (batch statistics over all valid pillars x T rows, the
// masked all-zero rows included) -> ReLU -> max over T (pillar_vfe.py:31-53 in train()), without a (P, T, 64) activation tensor.
//
// The pre-norm activation z = f W^T is linear in the K <= 11 decorated features, so with M = valid pillars x T rows
//     mean = W sum(f) / M,      E[z^2] = diag(W G W^T) / M,      G = F^T F  (K x K),
// and the batch statistics need K + K (K + 1) / 2 sums over the points.  Once they are known the forward is the inference operator
// (pillar_vfe.hip) on the folded operands W' = W gamma rstd, s' = beta - mean gamma rstd; the backward recomputes a pillar's rows, finds
// the winning row of every channel (lowest row index on ties: masked rows are identical and have f = 0, a zero maximum carries no
// gradient, so no tie can change a parameter gradient) and accumulates, with g = d out[p, c] where the maximum is positive,
//     A[c, k] = sum g f[winner, k],   Sdy[c] = sum g,   Sdz[c] = sum g zhat[winner],
//     dW[c, :] = rstd gamma (A[c, :] - Sdy sum(f) / M - Sdz rstd (W_c G - mean_c sum(f)) / M),   dgamma = Sdz,   dbeta = Sdy
// (the two / M terms vanish with frozen statistics; without a norm dW = A and d bias = Sdy).
//
// Launches (no host read anywhere, M comes from the device count, so a padded batch replays from a captured graph):
//   1 pillar_compact_kernel   one workgroup: rank of every valid pillar (a stable compaction), its destination row, the valid count
//   2 pillar_stats_kernel     per-lane fp64 sums of f and f f^T over the pillars of a workgroup -> one fp64 partial per workgroup
//   3 pillar_finish_kernel    partials in fixed order (fp64) -> mean, biased variance, rstd, (W', s'), running-statistics update
//   4 pillar_bwd_kernel       phase 1: a half-wave recomputes one pillar, leaves f (32 x K) and the 64 winners / maxima in LDS;
//                             phase 2: lane c of the same wave adds g f[winner] into K + 2 private registers, pillars in rank order
//   5 pillar_bwd_finish_kernel  partials in fixed order (fp64), then the dW formula above
// Work is shared out by RANK among valid pillars, not by pillar index: where the skipped rows of a padded batch sit changes no
// summation order, and no floating-point atomic is used - the statistics and the gradients are bitwise reproducible and bitwise equal
// to those of the same batch without its skipped rows.
#include "pillar_common.hpp"
#include "wave_ops.hpp"

namespace cobevt {

constexpr int kStatRanks = 256;       // valid pillars per workgroup of the statistics pass (32 per half-wave)
constexpr int kBwdRanks = 64;         // ... of the backward pass (8 rounds of 8 half-waves)
constexpr int kStatDoubles = 512;     // the saved statistics block, see stat_layout below

// fp64 block the finishing launch leaves for the backward: [0] M, [1] valid pillars, [2 .. 2 + K) sum(f), then G (K x K, full),
// then mean (64), rstd (64), biased variance (64)
__host__ __device__ constexpr int stat_sf() { return 2; }
__host__ __device__ constexpr int stat_g(int K) { return 2 + K; }
__host__ __device__ constexpr int stat_mean(int K) { return 2 + K + K * K; }
__host__ __device__ constexpr int stat_rstd(int K) { return stat_mean(K) + kPillarC; }
__host__ __device__ constexpr int stat_var(int K) { return stat_mean(K) + 2 * kPillarC; }
static_assert(stat_var(11) + kPillarC <= kStatDoubles, "statistics block");

// One workgroup of 1024 threads: thread i owns the pillars [i chunk, (i + 1) chunk); a pillar is valid when the inference operator
// writes it (rows form: n_p > 0; canvas form: n_p > 0 and canvas_row >= 0).  order[r] = pillar of rank r, dst[r] = its destination row.
__global__ __launch_bounds__(1024) void pillar_compact_kernel(const int* __restrict__ npts, const int4* __restrict__ coords,
                                                              const int* __restrict__ record_len, int* __restrict__ order,
                                                              long* __restrict__ dst, int* __restrict__ count, PillarArgs a) {
    __shared__ int part[1024];
    const int tid = threadIdx.x;
    const long chunk = (a.P + 1023) / 1024;
    const long lo = min((long)tid * chunk, a.P), hi = min(lo + chunk, a.P);
    auto row_of = [&](long p) -> long {
        if (npts[p] <= 0) return -1;
        return a.rows ? p : canvas_row(coords[p], record_len, a.N, a.B, a.max_cav, a.ny, a.nx);
    };
    int n = 0;
    for (long p = lo; p < hi; ++p) n += row_of(p) >= 0 ? 1 : 0;
    part[tid] = n;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                       // inclusive scan
        const int v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int r = part[tid] - n;
    for (long p = lo; p < hi; ++p) {
        const long d = row_of(p);
        if (d >= 0) { order[r] = (int)p; dst[r] = d; ++r; }
    }
    if (tid == 1023) count[0] = part[1023];
}

// Sums of f and of the upper triangle of f f^T in fp64 (at +-140 m x^2 reaches 2e4 and E[z^2] - mean^2 cancels).  Half-wave h of
// workgroup b takes the ranks b * 256 + h + 8 i; the partial of a workgroup is reduced over its lanes by a fixed butterfly.
template <bool kAbs, bool kDist>
__global__ __launch_bounds__(256) void pillar_stats_kernel(const float4* __restrict__ vf, const int* __restrict__ npts,
                                                           const int4* __restrict__ coords, const int* __restrict__ order,
                                                           const int* __restrict__ count, double* __restrict__ partial, PillarArgs a) {
    constexpr int K = pillar_k(kAbs, kDist);
    constexpr int NS = K + K * (K + 1) / 2;
    __shared__ double red[4][NS];
    const int cnt = count[0];
    const long base = (long)blockIdx.x * kStatRanks;
    if (base >= cnt) return;                                    // uniform over the workgroup
    const int t = threadIdx.x & 31, hw = threadIdx.x >> 5;
    double acc[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) acc[i] = 0.0;
    for (long r = base + hw; r < min(base + kStatRanks, (long)cnt); r += 8) {      // uniform over the half-wave
        const long p = order[r];
        const int n_p = npts[p];
        const int4 c = coords[p];
        const float4 pt = vf[p * a.T + min(t, a.T - 1)];
        float f[K];
        pillar_decorate<kAbs, kDist>(pt, t, n_p, c, a, f);
        // the lanes past T hold a copy of row T - 1: kept out of the sums
        double d[K];
#pragma unroll
        for (int i = 0; i < K; ++i) d[i] = t < a.T ? (double)f[i] : 0.0;
        int s = K;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            acc[i] += d[i];
#pragma unroll
            for (int j = i; j < K; ++j) { acc[s] = fma(d[i], d[j], acc[s]); ++s; }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        double v = acc[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < NS) {
        const int i = threadIdx.x;
        partial[(long)blockIdx.x * NS + i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
    }
}

// mode 0: batch statistics (reduces the partials, updates the running statistics); 1: frozen running statistics; 2: no norm
// (W' = W^T, s' = bias).  One workgroup of 1024 threads.  w (64, K), wf (K, 64), sf (64).  With zero valid pillars nothing is updated
// and (W', s') = (0, beta): the forward then writes no row and the backward reads none.
template <int K>
__global__ __launch_bounds__(1024) void pillar_finish_kernel(const double* __restrict__ partial, const int* __restrict__ count,
                                                             const float* __restrict__ w, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float* __restrict__ running_mean,
                                                             float* __restrict__ running_var, long* __restrict__ num_batches,
                                                             float* __restrict__ wf, float* __restrict__ sf, double* __restrict__ stat,
                                                             int T, int mode, float eps, float momentum) {
    constexpr int NS = K + K * (K + 1) / 2;
    __shared__ double red[8][128];
    __shared__ double S[128];
    const int tid = threadIdx.x;
    const int cnt = count ? count[0] : 0;
    const double M = (double)cnt * (double)T;
    if (mode == 0) {
        const int nb = (cnt + kStatRanks - 1) / kStatRanks;
        const int i = tid & 127, j = tid >> 7;
        double v = 0.0;
        if (i < NS)
            for (int b = j; b < nb; b += 8) v += partial[(long)b * NS + i];
        red[j][i] = v;
        __syncthreads();
        if (tid < 128) {
            double s = red[0][tid];
#pragma unroll
            for (int q = 1; q < 8; ++q) s += red[q][tid];
            S[tid] = s;
        }
        __syncthreads();
        if (tid == 0) { stat[0] = M; stat[1] = (double)cnt; }
        if (tid < K) stat[stat_sf() + tid] = S[tid];
        if (tid < K * K) {
            const int r = tid / K, c = tid - r * K, lo = min(r, c), hi = max(r, c);
            stat[stat_g(K) + tid] = S[K + lo * K - lo * (lo - 1) / 2 + (hi - lo)];      // upper triangle, row-major
        }
    } else if (tid == 0) {
        stat[0] = M; stat[1] = (double)cnt;
    }
    if (tid >= kPillarC) return;
    const int c = tid;
    double wr[K];
#pragma unroll
    for (int i = 0; i < K; ++i) wr[i] = (double)w[c * K + i];
    double scale = 1.0, shift = 0.0;
    if (mode == 2) {
        shift = beta ? (double)beta[c] : 0.0;                   // the Linear's bias
    } else {
        double mean = 0.0, var = 0.0, rstd = 0.0;
        if (mode == 1) {
            mean = (double)running_mean[c];
            var = (double)running_var[c];
            rstd = 1.0 / sqrt(var + (double)eps);
        } else if (cnt > 0) {
            double ez2 = 0.0;
            int s = K;
#pragma unroll
            for (int i = 0; i < K; ++i) {
                mean += wr[i] * S[i];
#pragma unroll
                for (int j = i; j < K; ++j) { ez2 += (i == j ? 1.0 : 2.0) * wr[i] * wr[j] * S[s]; ++s; }
            }
            mean /= M;
            var = fmax(ez2 / M - mean * mean, 0.0);
            rstd = 1.0 / sqrt(var + (double)eps);
            if (running_mean && running_var) {
                const double unbiased = M > 1.0 ? var * (M / (M - 1.0)) : var;
                running_mean[c] = (float)((1.0 - (double)momentum) * (double)running_mean[c] + (double)momentum * mean);
                running_var[c] = (float)((1.0 - (double)momentum) * (double)running_var[c] + (double)momentum * unbiased);
            }
            if (c == 0 && num_batches) num_batches[0] += 1;
        }
        stat[stat_mean(K) + c] = mean;
        stat[stat_rstd(K) + c] = rstd;
        stat[stat_var(K) + c] = var;
        const double g = gamma ? (double)gamma[c] : 1.0, b = beta ? (double)beta[c] : 0.0;
        scale = g * rstd;
        shift = b - mean * scale;
    }
#pragma unroll
    for (int i = 0; i < K; ++i) wf[i * kPillarC + c] = (float)(wr[i] * scale);
    sf[c] = (float)shift;
}

// Backward.  LDS per half-wave slot: f (32 x K), the 64 winners and the 64 maxima of one pillar.  Workgroup b takes the ranks
// [64 b, 64 b + 64): round i puts rank 64 b + 8 i + h on half-wave h; wave v then walks the two pillars of its own half-waves in rank
// order.  Only rows t < T may win (the lanes past T hold a copy of row T - 1).  g is read straight from the gradient of the canvas
// (or of the dense rows) at the pillar's destination row: scatter and regroup backward are this read.
template <bool kAbs, bool kDist>
__global__ __launch_bounds__(256) void pillar_bwd_kernel(const float4* __restrict__ vf, const int* __restrict__ npts,
                                                         const int4* __restrict__ coords, const int* __restrict__ order,
                                                         const long* __restrict__ dst, const int* __restrict__ count,
                                                         const float* __restrict__ Wf, const float* __restrict__ Sf,
                                                         const float* __restrict__ w, const double* __restrict__ stat,
                                                         const float* __restrict__ dout, float* __restrict__ partial, int mode,
                                                         PillarArgs a) {
    constexpr int K = pillar_k(kAbs, kDist);
    constexpr int NV = K + 2;
    constexpr int KS = K | 1;             // odd row stride: the 32 rows of a pillar fall on different LDS banks
    __shared__ float lf[8][32 * KS];
    __shared__ float lmax[8][kPillarC];
    __shared__ int lwin[8][kPillarC];
    __shared__ float lred[4][NV][kPillarC];
    const int cnt = count[0];
    const long base = (long)blockIdx.x * kBwdRanks;
    if (base >= cnt) return;                                    // uniform over the workgroup
    const int t = threadIdx.x & 31, hw = threadIdx.x >> 5;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // phase-2 operands of channel c = lane: the raw weight row, mean and rstd (zhat = rstd (W_c f - mean))
    float wr[K];
#pragma unroll
    for (int i = 0; i < K; ++i) wr[i] = w[lane * K + i];
    const float mean = mode == 2 ? 0.f : (float)stat[stat_mean(K) + lane], rstd = mode == 2 ? 1.f : (float)stat[stat_rstd(K) + lane];
    float acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.f;

#pragma unroll 1
    for (int round = 0; round < kBwdRanks / 8; ++round) {
        const long r = base + round * 8 + hw;
        const bool live = r < cnt;                              // uniform over the half-wave
        float y[kPillarC];
        if (live) {
            const long p = order[r];
            const int n_p = npts[p];
            const int4 c = coords[p];
            const float4 pt = vf[p * a.T + min(t, a.T - 1)];
            float f[K];
            pillar_decorate<kAbs, kDist>(pt, t, n_p, c, a, f);
            pillar_responses<K>(f, Wf, Sf, y);
            float m8[8];
            pillar_row_max(y, t, m8);
            // lane group g = (t >> 2) & 7 holds the maxima of channels 8 g .. 8 g + 7
            if ((t & 3) == 0) {
#pragma unroll
                for (int e = 0; e < 8; ++e) lmax[hw][8 * (t >> 2) + e] = m8[e];
            }
#pragma unroll
            for (int i = 0; i < K; ++i) lf[hw][t * KS + i] = f[i];
        }
        __syncthreads();
        if (live) {
            // winner of a channel: the lowest row t < T whose response equals the maximum (one compare per channel; the vote is a
            // scalar mask per wave, its two halves are the wave's two pillars)
            int w0 = -1, w1 = -1;
#pragma unroll
            for (int ch = 0; ch < kPillarC; ++ch) {
                const bool hit = t < a.T && y[ch] == lmax[hw][ch];
                const unsigned long long vote = __ballot(hit);
                const unsigned half = (unsigned)(lane < 32 ? vote : vote >> 32);
                const int win = half ? __ffs((int)half) - 1 : -1;
                if (ch < 32) w0 = (t == ch) ? win : w0;
                else w1 = (t == ch - 32) ? win : w1;
            }
            lwin[hw][t] = w0;
            lwin[hw][t + 32] = w1;
        }
        __syncthreads();
        // phase 2: lane c of wave v, pillars of half-waves 2 v and 2 v + 1 in rank order
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int slot = 2 * wave + q;
            const long rr = base + round * 8 + slot;
            if (rr < cnt) {                                     // uniform over the wave
                const float mx = lmax[slot][lane];
                const int win = lwin[slot][lane];
                const float g = (mx > 0.f && win >= 0) ? dout[dst[rr] * kPillarC + lane] : 0.f;
                const int wi = max(win, 0);
                float z = 0.f;
#pragma unroll
                for (int i = 0; i < K; ++i) {
                    const float fi = lf[slot][wi * KS + i];
                    acc[i] = fmaf(g, fi, acc[i]);
                    z = fmaf(wr[i], fi, z);
                }
                acc[K] += g;
                acc[K + 1] = fmaf(g, (z - mean) * rstd, acc[K + 1]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) lred[wave][i][lane] = acc[i];
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i)
            partial[((long)blockIdx.x * NV + i) * kPillarC + lane] = ((lred[0][i][lane] + lred[1][i][lane]) + lred[2][i][lane]) + lred[3][i][lane];
    }
}

// One workgroup of 1024 threads: group j of 64 lanes sums the partials j, j + 16, .. in fp64, the groups are added in order, then the
// first wave applies the dW formula.  dw (64, K), dgamma / dbeta (64) fp32 (dbeta = d bias in mode 2, dgamma unused there).
template <int K>
__global__ __launch_bounds__(1024) void pillar_bwd_finish_kernel(const float* __restrict__ partial, const int* __restrict__ count,
                                                                 const float* __restrict__ w, const float* __restrict__ gamma,
                                                                 const double* __restrict__ stat, float* __restrict__ dw,
                                                                 float* __restrict__ dgamma, float* __restrict__ dbeta, int mode) {
    constexpr int NV = K + 2;
    __shared__ double red[16][kPillarC];
    __shared__ double tot[NV][kPillarC];
    const int c = threadIdx.x & 63, j = threadIdx.x >> 6;
    const int cnt = count[0];
    const int nb = (cnt + kBwdRanks - 1) / kBwdRanks;
#pragma unroll 1
    for (int i = 0; i < NV; ++i) {
        double v = 0.0;
        for (int b = j; b < nb; b += 16) v += (double)partial[((long)b * NV + i) * kPillarC + c];
        red[j][c] = v;
        __syncthreads();
        if (j == 0) {
            double s = red[0][c];
#pragma unroll
            for (int q = 1; q < 16; ++q) s += red[q][c];
            tot[i][c] = s;
        }
        __syncthreads();
    }
    if (j != 0) return;
    const double sdy = tot[K][c], sdz = tot[K + 1][c];
    if (mode == 2) {
#pragma unroll 1
        for (int i = 0; i < K; ++i) dw[c * K + i] = (float)tot[i][c];
        if (dbeta) dbeta[c] = (float)sdy;
        return;
    }
    const double g = gamma ? (double)gamma[c] : 1.0;
    const double mean = stat[stat_mean(K) + c], rstd = stat[stat_rstd(K) + c], M = stat[0];
    const bool batch = mode == 0 && M > 0.0;
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        double v = tot[k][c];
        if (batch) {
            double wg = 0.0;
#pragma unroll 1
            for (int i = 0; i < K; ++i) wg += (double)w[c * K + i] * stat[stat_g(K) + i * K + k];
            const double sfk = stat[stat_sf() + k];
            v -= sdy * sfk / M + sdz * rstd * (wg - mean * sfk) / M;
        }
        dw[c * K + k] = (float)(rstd * g * v);
    }
    if (dgamma) dgamma[c] = (float)sdz;
    if (dbeta) dbeta[c] = (float)sdy;
}

// backward of scatter_rows_kernel: 16-byte chunk j of row p <- chunk j of cell (n, y, x) of the canvas gradient, zero for skipped rows
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint4* __restrict__ canvas, const int4* __restrict__ coords,
                                                          uint4* __restrict__ rows, long P, int cpr, int N, int ny, int nx) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long p = i / cpr;
    if (p >= P) return;
    const int j = (int)(i - p * cpr);
    const long src = canvas_row(coords[p], nullptr, N, 0, 0, ny, nx);
    rows[i] = src < 0 ? make_uint4(0, 0, 0, 0) : canvas[src * cpr + j];
}

static int parse_args(const int* dims, const float* geom, PillarArgs& a, int& K, int& which) {
    a.P = dims[0]; a.T = dims[1];
    const int F = dims[2], use_abs = dims[4], dist = dims[5];
    K = dims[3];
    a.rows = dims[7]; a.N = dims[8]; a.B = dims[9]; a.max_cav = dims[10]; a.ny = dims[11]; a.nx = dims[12];
    a.vx = geom[0]; a.vy = geom[1]; a.vz = geom[2]; a.xoff = geom[3]; a.yoff = geom[4]; a.zoff = geom[5];
    if (a.P < 0 || a.P > 0x7fffffffL || a.T < 1 || a.T > 32 || F != 4 || K != pillar_k(use_abs != 0, dist != 0)) return COBEVT_ERR_SHAPE;
    if (!a.rows && (a.N < 1 || a.ny < 1 || a.nx < 1)) return COBEVT_ERR_SHAPE;
    which = ((use_abs ? 1 : 0) << 1) | (dist ? 1 : 0);
    return COBEVT_OK;
}

template <int K>
static int launch_finish(const double* partial, const int* count, const float* w, const float* gamma, const float* beta, float* rm,
                         float* rv, long* nbt, float* wf, float* sf, double* stat, int T, int mode, float eps, float momentum,
                         hipStream_t stream) {
    hipLaunchKernelGGL((pillar_finish_kernel<K>), dim3(1), dim3(1024), 0, stream, partial, count, w, gamma, beta, rm, rv, nbt, wf, sf, stat,
                       T, mode, eps, momentum);
    return cobevt::launch_status();
}

template <int K>
static int launch_bwd_finish(const float* partial, const int* count, const float* w, const float* gamma, const double* stat, float* dw,
                             float* dgamma, float* dbeta, int mode, hipStream_t stream) {
    hipLaunchKernelGGL((pillar_bwd_finish_kernel<K>), dim3(1), dim3(1024), 0, stream, partial, count, w, gamma, stat, dw, dgamma, dbeta, mode);
    return cobevt::launch_status();
}

}  // namespace cobevt

using namespace cobevt;

extern "C" int cobevt_pillar_train_scratch(long P, long* stats_doubles, long* bwd_floats) {
    if (P < 0 || !stats_doubles || !bwd_floats) return COBEVT_ERR_ARG;
    const long sb = (P + kStatRanks - 1) / kStatRanks, bb = (P + kBwdRanks - 1) / kBwdRanks;
    *stats_doubles = (sb > 0 ? sb : 1) * (11 + 66);
    *bwd_floats = (bb > 0 ? bb : 1) * 13 * kPillarC;
    return COBEVT_OK;
}

extern "C" int cobevt_pillar_train_stats(const float* voxel_features, const int* voxel_num_points, const int* voxel_coords,
                                         const int* record_len, const float* w, const float* gamma, const float* beta,
                                         float* running_mean, float* running_var, long* num_batches_tracked, int* order, long* dst,
                                         int* count, double* partial, float* w_folded, float* shift_folded, double* stat,
                                         const int* dims, const float* geom, int mode, float eps, float momentum, hipStream_t stream) {
    if (!dims || !geom || !w || !order || !dst || !count || !w_folded || !shift_folded || !stat) return COBEVT_ERR_ARG;
    if (mode < 0 || mode > 2) return COBEVT_ERR_ARG;
    PillarArgs a;
    int K, which;
    const int rc = parse_args(dims, geom, a, K, which);
    if (rc != COBEVT_OK) return rc;
    if (a.P > 0 && (!voxel_features || !voxel_num_points || !voxel_coords)) return COBEVT_ERR_ARG;
    if (mode == 0 && !partial) return COBEVT_ERR_ARG;
    if (mode == 1 && (!running_mean || !running_var)) return COBEVT_ERR_ARG;
    if (((uintptr_t)voxel_features | (uintptr_t)voxel_coords) & 15) return COBEVT_ERR_SHAPE;
    if (!a.rows && !record_len) { a.B = 0; a.max_cav = 0; }
    if (!a.rows && record_len && (a.B < 1 || a.max_cav < 1)) return COBEVT_ERR_SHAPE;
    hipLaunchKernelGGL(pillar_compact_kernel, dim3(1), dim3(1024), 0, stream, voxel_num_points, (const int4*)voxel_coords, record_len, order,
                       dst, count, a);
    int st = cobevt::launch_status();
    if (st != COBEVT_OK) return st;
    if (mode == 0 && a.P > 0) {
        const unsigned blocks = (unsigned)((a.P + kStatRanks - 1) / kStatRanks);
        const float4* vf = (const float4*)voxel_features;
        const int4* co = (const int4*)voxel_coords;
        switch (which) {
            case 0: hipLaunchKernelGGL((pillar_stats_kernel<false, false>), dim3(blocks), dim3(256), 0, stream, vf, voxel_num_points, co, order, count, partial, a); break;
            case 1: hipLaunchKernelGGL((pillar_stats_kernel<false, true>), dim3(blocks), dim3(256), 0, stream, vf, voxel_num_points, co, order, count, partial, a); break;
            case 2: hipLaunchKernelGGL((pillar_stats_kernel<true, false>), dim3(blocks), dim3(256), 0, stream, vf, voxel_num_points, co, order, count, partial, a); break;
            default: hipLaunchKernelGGL((pillar_stats_kernel<true, true>), dim3(blocks), dim3(256), 0, stream, vf, voxel_num_points, co, order, count, partial, a); break;
        }
        st = cobevt::launch_status();
        if (st != COBEVT_OK) return st;
    }
    switch (K) {
        case 7: return launch_finish<7>(partial, count, w, gamma, beta, running_mean, running_var, num_batches_tracked, w_folded, shift_folded, stat, a.T, mode, eps, momentum, stream);
        case 8: return launch_finish<8>(partial, count, w, gamma, beta, running_mean, running_var, num_batches_tracked, w_folded, shift_folded, stat, a.T, mode, eps, momentum, stream);
        case 10: return launch_finish<10>(partial, count, w, gamma, beta, running_mean, running_var, num_batches_tracked, w_folded, shift_folded, stat, a.T, mode, eps, momentum, stream);
        default: return launch_finish<11>(partial, count, w, gamma, beta, running_mean, running_var, num_batches_tracked, w_folded, shift_folded, stat, a.T, mode, eps, momentum, stream);
    }
}

extern "C" int cobevt_pillar_train_bwd(const float* voxel_features, const int* voxel_num_points, const int* voxel_coords, const int* order,
                                       const long* dst, const int* count, const float* w_folded, const float* shift_folded, const float* w,
                                       const float* gamma, const double* stat, const float* dout, float* partial, float* dw,
                                       float* dgamma, float* dbeta, const int* dims, const float* geom, int mode, hipStream_t stream) {
    if (!dims || !geom || !order || !dst || !count || !w_folded || !shift_folded || !w || !stat || !dout || !partial || !dw) return COBEVT_ERR_ARG;
    if (mode < 0 || mode > 2) return COBEVT_ERR_ARG;
    PillarArgs a;
    int K, which;
    const int rc = parse_args(dims, geom, a, K, which);
    if (rc != COBEVT_OK) return rc;
    if (a.P > 0 && (!voxel_features || !voxel_num_points || !voxel_coords)) return COBEVT_ERR_ARG;
    if (((uintptr_t)voxel_features | (uintptr_t)voxel_coords) & 15) return COBEVT_ERR_SHAPE;
    if (a.P > 0) {
        const unsigned blocks = (unsigned)((a.P + kBwdRanks - 1) / kBwdRanks);
        const float4* vf = (const float4*)voxel_features;
        const int4* co = (const int4*)voxel_coords;
        switch (which) {
            case 0: hipLaunchKernelGGL((pillar_bwd_kernel<false, false>), dim3(blocks), dim3(256), 0, stream, vf, voxel_num_points, co, order, dst, count, w_folded, shift_folded, w, stat, dout, partial, mode, a); break;
            case 1: hipLaunchKernelGGL((pillar_bwd_kernel<false, true>), dim3(blocks), dim3(256), 0, stream, vf, voxel_num_points, co, order, dst, count, w_folded, shift_folded, w, stat, dout, partial, mode, a); break;
            case 2: hipLaunchKernelGGL((pillar_bwd_kernel<true, false>), dim3(blocks), dim3(256), 0, stream, vf, voxel_num_points, co, order, dst, count, w_folded, shift_folded, w, stat, dout, partial, mode, a); break;
            default: hipLaunchKernelGGL((pillar_bwd_kernel<true, true>), dim3(blocks), dim3(256), 0, stream, vf, voxel_num_points, co, order, dst, count, w_folded, shift_folded, w, stat, dout, partial, mode, a); break;
        }
        const int st = cobevt::launch_status();
        if (st != COBEVT_OK) return st;
    }
    switch (K) {
        case 7: return launch_bwd_finish<7>(partial, count, w, gamma, stat, dw, dgamma, dbeta, mode, stream);
        case 8: return launch_bwd_finish<8>(partial, count, w, gamma, stat, dw, dgamma, dbeta, mode, stream);
        case 10: return launch_bwd_finish<10>(partial, count, w, gamma, stat, dw, dgamma, dbeta, mode, stream);
        default: return launch_bwd_finish<11>(partial, count, w, gamma, stat, dw, dgamma, dbeta, mode, stream);
    }
}

extern "C" int cobevt_gather_rows(const void* canvas, const int* voxel_coords, void* rows, int dtype, long P, int C, int N, int ny, int nx,
                                  hipStream_t stream) {
    if (dtype != 0 && dtype != 1) return COBEVT_ERR_ARG;
    const int eb = dtype == 0 ? 2 : 4;
    if (P < 0 || C < 1 || (C * eb) % 16 || N < 1 || ny < 1 || nx < 1) return COBEVT_ERR_SHAPE;
    if (P == 0) return COBEVT_OK;
    if (!canvas || !voxel_coords || !rows) return COBEVT_ERR_ARG;
    if (((uintptr_t)rows | (uintptr_t)voxel_coords | (uintptr_t)canvas) & 15) return COBEVT_ERR_SHAPE;
    const int cpr = C * eb / 16;
    const long blocks = (P * cpr + 255) / 256;
    if (blocks > 0x7fffffffL) return COBEVT_ERR_SHAPE;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const uint4*)canvas, (const int4*)voxel_coords,
                       (uint4*)rows, P, cpr, N, ny, nx);
    return cobevt::launch_status();
}
