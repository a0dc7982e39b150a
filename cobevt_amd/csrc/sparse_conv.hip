// Sparse 3-D convolutions over an active-voxel set (gfx950): what OpenCOOD's SECOND-style encoder
// (mean_vfe.py, sparse_backbone_3d.py, height_compression.py) delegates to spconv - SubMConv3d, SparseConv3d, SparseConvTensor.dense -
// and MeanVFE in front of them.  Library-independent: the fp32-storage kernel is the exact v_mfma_f32_32x32x2_f32 one in all three
// libraries (this source does not reach the fp32 matrix-path header), bf16 storage runs v_mfma_f32_32x32x16_bf16 with fp32 accumulation.
//
// A LEVEL is a sparse shape (N, D, H, W) with an active set.  Its index, in one int32 workspace of cobevt_sparse_scratch(dims) ints:
//   bits    one bit per cell, cell = ((b D + z) H + y) W + x, 32 cells per word (padded to whole 1024-word blocks)
//   prefix  per word, the number of active cells in all words before it
//   part    per 1024-word block, the same (the scan's partials; the total at entry `blocks`)
// so that row(cell) = prefix[cell >> 5] + popcount(bits[cell >> 5] & ((1 << (cell & 31)) - 1)): rows are ordered by cell index, and a
// neighbour lookup is two loads.  Next to it, caller-owned: indices (cap, 4) int32 [b, z, y, x] by row, and num (2) int32 =
// [live rows = min(active cells, cap), dropped = active cells - live rows].  Rows at or past the capacity are dropped from the HIGH end
// of the cell order: they are not written anywhere and every lookup treats them as inactive.  Nothing reads num on the host: every
// launch is sized by the capacity and reads the live count itself, so a captured graph replays on clouds of any size.
//
// Building an index - no host read, integer atomics only, and only such whose FINAL value does not depend on arrival order:
//   1 clear   the bits, by a kernel
//   2 mark    level 0: one thread per row of voxel_coords, atomicOr of its cell's bit; rows with b < 0 (the padding convention) or a
//             coordinate outside the shape are ignored.  A strided SparseConv3d(k, s, p): one thread per live input row, atomicOr of
//             the bit of every output o with s o - p + k' = i for a k' in [0, k) per axis - at most 8 for 3 / 2 / 1, 2 for (3, 1, 1) / (2, 1, 1)
//   3 count   popcount per 1024 words
//   4 scan    ONE workgroup: exclusive scan of the block counts, serial over chunks of 1024; writes num
//   5 emit    per 1024 words: prefix per word, and indices of the rows below the capacity (level 0: source[row] <- INT_MAX too)
//   6 source  (level 0 only) atomicMin(source[row(cell)], input row): of duplicate cells the lowest input row wins, and the first
//             convolution reads its input rows THROUGH source, so the features are never permuted in memory
//
// The convolution - one kernel for SubMConv3d and SparseConv3d, output-stationary: no floating-point atomics, bitwise reproducible.
// A workgroup owns 128 consecutive output rows (neighbours along x, by the cell order), one 32-row MFMA tile per wave.  It resolves
// its rows x taps neighbour table into LDS once (input cell = s o - p + k; for SubM s = 1, p = 1, the output set IS the input set).
// A wave then walks the taps: one ballot decides whether any of its 32 rows has that tap, absent taps cost nothing; for a present
// tap every lane gathers its row's 16-byte pieces straight from global memory (absent rows: zeros) and multiplies by the tap's
// [Cout][Cin] weight slice (read through L1 / L2: at most 442 KB per layer, shared by every wave).  The weights are the FIRST MFMA
// operand, so a lane holds 4 consecutive channels of ONE row per accumulator quad: the epilogue adds the folded BatchNorm shift,
// applies ReLU and stores 8 / 16 bytes per quad in the storage dtype.  Feature rows at or past the live count are NOT written.
// Channels: input rows are kgroups x 32 bytes (Cin <= 8 is padded to one k-group with zero weights behind it), Cout is padded to a
// multiple of 32 in the weight table only.
//
// Training (fp32 rows) is in this file too: the same kernel with a plain-store epilogue (z = conv(x)) and with the
// transposed neighbour rule (the input gradient), BatchNorm statistics / apply / backward over the live rows, the weight gradient with
// the rows as the MFMA's k dimension, and the densify step's adjoint.
#include "common.hpp"

namespace cobevt {

constexpr int kSpScanWords = 1024;                 // words per workgroup of the count / emit launches: 256 threads x one uint4
constexpr int kSpBlockRows = 128;                  // output rows per workgroup of the convolution: four waves x one 32-row tile
constexpr int kSpMaxTaps = 27;
constexpr long kSpMaxCells = 0x7fffffffL - 32L * kSpScanWords;      // a cell index, and its padded word range, fit an int

struct SpShape { int N, D, H, W; };
struct SpGeom { int k[3], s[3], p[3]; };

static long sp_cells(const SpShape& s) { return (long)s.N * s.D * s.H * s.W; }
// 1024-word blocks of a level, and the words padded to whole blocks
static long sp_blocks(const SpShape& s) { const long b = ((sp_cells(s) + 31) / 32 + kSpScanWords - 1) / kSpScanWords; return b > 0 ? b : 1; }
static long sp_words(const SpShape& s) { return sp_blocks(s) * kSpScanWords; }
static long sp_index_ints(const SpShape& s) { return 2 * sp_words(s) + sp_blocks(s) + 1; }

struct SpIndex {                                   // the three tables of a level's workspace
    unsigned* bits;
    int* prefix;
    int* part;
};
static SpIndex sp_index(int* ws, const SpShape& s) {
    SpIndex ix;
    ix.bits = (unsigned*)ws; ix.prefix = ws + sp_words(s); ix.part = ws + 2 * sp_words(s);
    return ix;
}

static int sp_shape_args(const long* d, SpShape& s) {
    for (int j = 0; j < 4; ++j)
        if (d[j] < 1 || d[j] > 0x7fffffffL) return COBEVT_ERR_SHAPE;
    if (d[0] > 65535) return COBEVT_ERR_SHAPE;
    long cells = d[0];
    for (int j = 1; j < 4; ++j) {
        if (cells > kSpMaxCells / d[j]) return COBEVT_ERR_SHAPE;
        cells *= d[j];
    }
    s.N = (int)d[0]; s.D = (int)d[1]; s.H = (int)d[2]; s.W = (int)d[3];
    return COBEVT_OK;
}

// kernel, stride, pad per axis (z, y, x) from nine longs: 3 x 3 x 3 or (3, 1, 1); 1, 2 or (2, 1, 1); 1, (0, 1, 1) or 0
static int sp_geom_args(const long* d, SpGeom& g) {
    const bool k333 = d[0] == 3 && d[1] == 3 && d[2] == 3, k311 = d[0] == 3 && d[1] == 1 && d[2] == 1;
    const bool s111 = d[3] == 1 && d[4] == 1 && d[5] == 1, s222 = d[3] == 2 && d[4] == 2 && d[5] == 2, s211 = d[3] == 2 && d[4] == 1 && d[5] == 1;
    const bool p111 = d[6] == 1 && d[7] == 1 && d[8] == 1, p011 = d[6] == 0 && d[7] == 1 && d[8] == 1, p000 = d[6] == 0 && d[7] == 0 && d[8] == 0;
    if (!(k333 || k311) || !(s111 || s222 || s211) || !(p111 || p011 || p000)) return COBEVT_ERR_SHAPE;
    if (k311 && !p000) return COBEVT_ERR_SHAPE;                       // a pad as wide as the kernel: outputs without any input
    for (int j = 0; j < 3; ++j) { g.k[j] = (int)d[j]; g.s[j] = (int)d[3 + j]; g.p[j] = (int)d[6 + j]; }
    return COBEVT_OK;
}

// the output shape of SparseConv3d: floor((n + 2 p - k) / s) + 1 per axis
static int sp_out_shape(const SpShape& si, const SpGeom& g, SpShape& so) {
    const int n[3] = {si.D, si.H, si.W};
    int o[3];
    for (int j = 0; j < 3; ++j) {
        const int span = n[j] + 2 * g.p[j] - g.k[j];
        if (span < 0) return COBEVT_ERR_SHAPE;
        o[j] = span / g.s[j] + 1;
    }
    so.N = si.N; so.D = o[0]; so.H = o[1]; so.W = o[2];
    return COBEVT_OK;
}

// [b, z, y, x] -> cell, or -1 for a padding row (b < 0) or a coordinate outside the shape
__device__ __forceinline__ int sp_cell(const int4 c, const SpShape& s) {
    if (c.x < 0 || c.x >= s.N || c.y < 0 || c.y >= s.D || c.z < 0 || c.z >= s.H || c.w < 0 || c.w >= s.W) return -1;
    return ((c.x * s.D + c.y) * s.H + c.z) * s.W + c.w;
}

// row of an active cell below the live count, else -1
__device__ __forceinline__ int sp_lookup(const unsigned* __restrict__ bits, const int* __restrict__ prefix, int cell, int live) {
    const unsigned w = bits[cell >> 5], m = 1u << (cell & 31);
    if (!(w & m)) return -1;
    const int row = prefix[cell >> 5] + __popc(w & (m - 1u));
    return row < live ? row : -1;
}

// p[0 .. bytes) <- 0, 16-byte stores and a byte tail; p 16-byte aligned.  A kernel, not a memset node: the index is rebuilt on every
// replay of a captured forward, and the bitmaps cleared by hipMemsetAsync nodes came back non-zero from the second replay on
// (DESIGN.md 3r), while a kernel node is replayed like every other launch here
__global__ __launch_bounds__(256) void sp_clear_kernel(uint4* __restrict__ p, size_t bytes) {
    const size_t n16 = bytes / 16, stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += stride) p[i] = make_uint4(0, 0, 0, 0);
    if (blockIdx.x == 0 && threadIdx.x < (bytes & 15)) ((unsigned char*)p)[n16 * 16 + threadIdx.x] = 0;
}
static void sp_clear(void* p, size_t bytes, hipStream_t stream) {
    size_t blocks = (bytes / 16 + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);          // grid-stride past 16 workgroups per CU
    hipLaunchKernelGGL(sp_clear_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (uint4*)p, bytes);
}

__global__ __launch_bounds__(256) void sp_mark_rows_kernel(const int4* __restrict__ coords, long P, SpShape s, unsigned* __restrict__ bits) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const int cell = sp_cell(coords[i], s);
    if (cell >= 0) atomicOr(&bits[cell >> 5], 1u << (cell & 31));
}

__global__ __launch_bounds__(256) void sp_mark_down_kernel(const int4* __restrict__ in_idx, const int* __restrict__ in_num, long in_cap,
                                                           SpShape si, SpGeom g, SpShape so, unsigned* __restrict__ bits) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= in_cap || i >= in_num[0]) return;
    const int4 c = in_idx[i];
    if (sp_cell(c, si) < 0) return;
    for (int kz = 0; kz < g.k[0]; ++kz) {
        const int nz = c.y + g.p[0] - kz;
        if (nz < 0 || nz % g.s[0] || nz / g.s[0] >= so.D) continue;
        for (int ky = 0; ky < g.k[1]; ++ky) {
            const int ny = c.z + g.p[1] - ky;
            if (ny < 0 || ny % g.s[1] || ny / g.s[1] >= so.H) continue;
            for (int kx = 0; kx < g.k[2]; ++kx) {
                const int nx = c.w + g.p[2] - kx;
                if (nx < 0 || nx % g.s[2] || nx / g.s[2] >= so.W) continue;
                const int cell = ((c.x * so.D + nz / g.s[0]) * so.H + ny / g.s[1]) * so.W + nx / g.s[2];
                atomicOr(&bits[cell >> 5], 1u << (cell & 31));
            }
        }
    }
}

__device__ __forceinline__ int sp_popc4(const uint4& v) { return __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w); }

__global__ __launch_bounds__(256) void sp_count_kernel(const uint4* __restrict__ bits, int* __restrict__ part) {
    __shared__ int lds[4];
    int n = sp_popc4(bits[(long)blockIdx.x * 256 + threadIdx.x]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = lds[0] + lds[1] + lds[2] + lds[3];
}

// the block counts -> their exclusive prefixes, in place, the total at entry `nb`; num = [min(total, cap), total - that]
__global__ __launch_bounds__(1024) void sp_scan_kernel(int* __restrict__ part, long nb, long cap, int* __restrict__ num) {
    __shared__ int lds[16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int carry = 0;
    for (long b0 = 0; b0 < nb; b0 += 1024) {
        const long b = b0 + threadIdx.x;
        const int v = b < nb ? part[b] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int x = __shfl_up(inc, o, 64);
            if (lane >= o) inc += x;
        }
        if (lane == 63) lds[w] = inc;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int x = lds[k];
            if (k < w) before += x;
            total += x;
        }
        __syncthreads();
        if (b < nb) part[b] = carry + before + inc - v;
        carry += total;
    }
    if (threadIdx.x == 0) {
        part[nb] = carry;
        const int live = carry < cap ? carry : (int)cap;
        num[0] = live;
        num[1] = carry - live;
    }
}

__global__ __launch_bounds__(256) void sp_emit_kernel(const uint4* __restrict__ bits, const int* __restrict__ part, int4* __restrict__ prefix,
                                                      int4* __restrict__ indices, int* __restrict__ source, long cap, SpShape s) {
    __shared__ int lds[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;             // this thread's four words
    const uint4 v = bits[q];
    const int n = sp_popc4(v);
    int inc = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int x = __shfl_up(inc, o, 64);
        if (lane >= o) inc += x;
    }
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    int base = part[blockIdx.x] + inc - n;
    for (int k = 0; k < w; ++k) base += lds[k];
    const unsigned word[4] = {v.x, v.y, v.z, v.w};
    int pre[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { pre[j] = base; base += __popc(word[j]); }
    prefix[q] = make_int4(pre[0], pre[1], pre[2], pre[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned m = word[j];
        int r = pre[j];
        while (m) {
            const int bit = __ffs(m) - 1;
            m &= m - 1u;
            if (r < cap) {
                int cell = (int)((q * 4 + j) * 32 + bit);            // below the shape's cell count: only valid cells are ever marked
                const int x = cell % s.W; cell /= s.W;
                const int y = cell % s.H; cell /= s.H;
                indices[r] = make_int4(cell / s.D, cell % s.D, y, x);
                if (source) source[r] = 0x7fffffff;                  // level 0: above every input row, for the source launch's atomicMin
            }
            ++r;
        }
    }
}

__global__ __launch_bounds__(256) void sp_source_kernel(const int4* __restrict__ coords, long P, SpShape s, const unsigned* __restrict__ bits,
                                                        const int* __restrict__ prefix, const int* __restrict__ num, int* __restrict__ source) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const int cell = sp_cell(coords[i], s);
    if (cell < 0) return;
    const int row = sp_lookup(bits, prefix, cell, num[0]);
    if (row >= 0) atomicMin(&source[row], (int)i);
}

// count, scan, emit of a level whose bits are marked
static void sp_rank(const SpIndex& ix, const SpShape& s, int4* indices, int* num, int* source, long cap, hipStream_t stream) {
    const long nb = sp_blocks(s);
    hipLaunchKernelGGL(sp_count_kernel, dim3((unsigned)nb), dim3(256), 0, stream, (const uint4*)ix.bits, ix.part);
    hipLaunchKernelGGL(sp_scan_kernel, dim3(1), dim3(1024), 0, stream, ix.part, nb, cap, num);
    hipLaunchKernelGGL(sp_emit_kernel, dim3((unsigned)nb), dim3(256), 0, stream, (const uint4*)ix.bits, (const int*)ix.part, (int4*)ix.prefix,
                       indices, source, cap, s);
}

// ---------------------------------------------------------------------------------------------- the convolution
struct SpConvArgs {
    const void* in;                                // (in_rows, kgroups x 32 bytes)
    const unsigned* in_bits;
    const int* in_prefix;
    const int* in_num;
    const int* row_map;                            // level 0: index row -> input row, else null
    const int4* out_idx;
    const int* out_num;
    const void* wgt;                               // [taps][NB x 32][kgroups x 32 bytes], the BatchNorm scale folded in
    const float* bias;                             // [NB x 32]
    void* out;                                     // (out_cap, cout)
    SpShape si;
    SpGeom g;
    long in_rows, out_cap;
    int taps, cout;
};

// one 32-byte k-group of a 32 x 32 tile: D[channel][row] += W[channel][k] X[row][k]; `w` / `x` are the 16-byte pieces this lane read
// from row (lane & 31) of either operand at byte 16 (lane >> 5) of the k-group (the fp32 form contracts the piece's four floats in
// four steps, the same permutation of k on both sides)
template <typename T> __device__ __forceinline__ void sp_mfma(const uint4& w, const uint4& x, f32x16& acc) {
    if constexpr (Elem<T>::kIsBf16) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w), __builtin_bit_cast(bf16x8, x), acc, 0, 0, 0);
    } else {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(w.x), __uint_as_float(x.x), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(w.y), __uint_as_float(x.y), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(w.z), __uint_as_float(x.z), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(w.w), __uint_as_float(x.w), acc, 0, 0, 0);
    }
}

// the epilogue / neighbour rule of sparse_conv_kernel.  kSpFused is the inference kernel; the two training forms (fp32 only) store the
// accumulators as they are and write zeros to the rows in [live, capacity)
constexpr int kSpFused = 0;                        // relu(acc + shift): folded weights
constexpr int kSpRaw = 1;                          // z = conv(x): unfolded weights, the forward neighbour rule
constexpr int kSpRawT = 2;                         // the input gradient: the "output" rows are the convolution's INPUT level, the rows read are
                                                   // d z of its output level, neighbour o = (i + p - k) / s where the division is exact

// zeros into this lane's share of one row (the lane pair l, l + 32 covers a row's channels in 16-byte pieces)
__device__ __forceinline__ void sp_zero_row(float* out, long row, long cap, int cout, int half) {
    if (row >= cap) return;
    for (int ch = 4 * half; ch < cout; ch += 8) *(float4*)(out + (size_t)row * cout + ch) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// KG: 32-byte k-groups of an input row; NB: 32-channel blocks of the (padded) output
template <typename T, int KG, int NB, int MODE = kSpFused>
__global__ __launch_bounds__(256) void sparse_conv_kernel(SpConvArgs a) {
    constexpr int ES = Elem<T>::kBytes;
    constexpr int ROWB = KG * 32;
    __shared__ int tab[kSpMaxTaps * kSpBlockRows];                   // [tap][row of the workgroup]: the input row, or -1
    const int live = a.out_num[0] < a.out_cap ? a.out_num[0] : (int)a.out_cap;       // (num[0] <= capacity by construction)
    const long r0 = (long)blockIdx.x * kSpBlockRows;
    if (r0 >= live) {                                                // uniform over the workgroup
        if constexpr (MODE != kSpFused) sp_zero_row((float*)a.out, r0 + (threadIdx.x >> 6) * 32 + (threadIdx.x & 31), a.out_cap, a.cout, (threadIdx.x & 63) >> 5);
        return;
    }
    const int in_live = a.in_num[0];
    const int kyx = a.g.k[1] * a.g.k[2];
    for (int e = threadIdx.x; e < a.taps * kSpBlockRows; e += 256) {
        const int t = e / kSpBlockRows, r = e % kSpBlockRows;
        int v = -1;
        if (r0 + r < live) {
            const int4 c = a.out_idx[r0 + r];
            const int kz = t / kyx, rem = t - kz * kyx, ky = rem / a.g.k[2], kx = rem - ky * a.g.k[2];
            int cell;
            if constexpr (MODE == kSpRawT) {
                const int nz = c.y + a.g.p[0] - kz, ny = c.z + a.g.p[1] - ky, nx = c.w + a.g.p[2] - kx;
                cell = -1;
                if (nz >= 0 && ny >= 0 && nx >= 0 && nz % a.g.s[0] == 0 && ny % a.g.s[1] == 0 && nx % a.g.s[2] == 0)
                    cell = sp_cell(make_int4(c.x, nz / a.g.s[0], ny / a.g.s[1], nx / a.g.s[2]), a.si);
            } else {
                cell = sp_cell(make_int4(c.x, c.y * a.g.s[0] - a.g.p[0] + kz, c.z * a.g.s[1] - a.g.p[1] + ky,
                                         c.w * a.g.s[2] - a.g.p[2] + kx), a.si);
            }
            if (cell >= 0) {
                v = sp_lookup(a.in_bits, a.in_prefix, cell, in_live);
                if (v >= 0 && a.row_map) v = a.row_map[v];
                if (v >= a.in_rows) v = -1;                          // never taken by an index this file built: no read past the features
            }
        }
        tab[e] = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
    const int rl = wave * 32 + (lane & 31);
    if (r0 + wave * 32 >= live) {                                    // uniform over the wave; no barrier follows
        if constexpr (MODE != kSpFused) sp_zero_row((float*)a.out, r0 + rl, a.out_cap, a.cout, half);
        return;
    }
    f32x16 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
    const unsigned char* wlane = (const unsigned char*)a.wgt + (size_t)(lane & 31) * ROWB + half * 16;
    for (int t = 0; t < a.taps; ++t) {
        const int mine = tab[t * kSpBlockRows + rl];
        if (__ballot(mine >= 0) == 0ull) continue;                   // no row of this tile has the tap
        const unsigned char* xp = (const unsigned char*)a.in + (size_t)(mine >= 0 ? mine : 0) * ROWB + half * 16;
        const unsigned char* wp = wlane + (size_t)t * (NB * 32 * ROWB);
#pragma unroll
        for (int g = 0; g < KG; ++g) {
            const uint4 x = mine >= 0 ? *(const uint4*)(xp + g * 32) : make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int b = 0; b < NB; ++b) sp_mfma<T>(*(const uint4*)(wp + (size_t)b * 32 * ROWB + g * 32), x, acc[b]);
        }
    }
    const long row = r0 + rl;
    if (row >= live) {
        if constexpr (MODE != kSpFused) sp_zero_row((float*)a.out, row, a.out_cap, a.cout, half);
        return;
    }
    unsigned char* o = (unsigned char*)a.out + (size_t)row * a.cout * ES;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ch = b * 32 + 8 * q + 4 * half;                // the lane's accumulator quad q: four consecutive channels of its row
            if (ch >= a.cout) continue;
            if constexpr (MODE != kSpFused) {
                *(float4*)(o + ch * ES) = make_float4(acc[b][4 * q + 0], acc[b][4 * q + 1], acc[b][4 * q + 2], acc[b][4 * q + 3]);
                continue;
            }
            const float4 sh = *(const float4*)(a.bias + ch);
            const float v0 = fmaxf(acc[b][4 * q + 0] + sh.x, 0.f), v1 = fmaxf(acc[b][4 * q + 1] + sh.y, 0.f);
            const float v2 = fmaxf(acc[b][4 * q + 2] + sh.z, 0.f), v3 = fmaxf(acc[b][4 * q + 3] + sh.w, 0.f);
            if constexpr (Elem<T>::kIsBf16) *(uint2*)(o + ch * ES) = make_uint2(pack_bf2(v0, v1), pack_bf2(v2, v3));
            else *(float4*)(o + ch * ES) = make_float4(v0, v1, v2, v3);
        }
}

template <typename T, int KG, int NB>
static void sp_conv_launch(const SpConvArgs& a, long out_cap, hipStream_t stream) {
    hipLaunchKernelGGL((sparse_conv_kernel<T, KG, NB>), dim3((unsigned)((out_cap + kSpBlockRows - 1) / kSpBlockRows)), dim3(256), 0, stream, a);
}

// the channel pairs of VoxelBackBone8x: (input row in channels of the storage dtype, Cout) -> the instantiation; false: unsupported
template <typename T>
static bool sp_conv_dispatch(int cin_pad, const SpConvArgs& a, long out_cap, hipStream_t stream, bool launch) {
    constexpr int G = 32 / Elem<T>::kBytes;                          // channels per k-group
    const int kg = cin_pad / G, co = a.cout;
    if (cin_pad % G) return false;
#define COBEVT_SP_CASE(KGV, NBV) do { if (launch) sp_conv_launch<T, KGV, NBV>(a, out_cap, stream); return true; } while (0)
    if (kg == 1 && (co == 16 || co == 32)) COBEVT_SP_CASE(1, 1);     // <= 8 -> 16 (padded), and bf16 16 -> 16 / 32
    if (cin_pad == 16 && (co == 16 || co == 32)) COBEVT_SP_CASE(16 / G, 1);
    if (cin_pad == 32 && co == 32) COBEVT_SP_CASE(32 / G, 1);
    if (cin_pad == 32 && co == 64) COBEVT_SP_CASE(32 / G, 2);
    if (cin_pad == 64 && co == 64) COBEVT_SP_CASE(64 / G, 2);
    if (cin_pad == 64 && co == 128) COBEVT_SP_CASE(64 / G, 4);
#undef COBEVT_SP_CASE
    return false;
}

// ---------------------------------------------------------------------------------------------- training (fp32 rows only)
// The training forward of a layer is z = conv(x) (kSpRaw), the BatchNorm statistics of z over the live rows, y = relu(z scale + shift);
// its backward is the BatchNorm + ReLU backward (d y -> d z), the input gradient (kSpRawT) and the weight gradient.  Every row count
// is the level's device word num[0]; no floating-point atomics anywhere: reductions over rows are cut into a FIXED number of row
// chunks whose length comes from num[0] (not from the capacity), one partial per chunk, and a finishing launch adds the partials in
// chunk order in fp64 - the bits depend on the live rows alone.
constexpr int kSpStatBlocks = 64;                  // row chunks of the statistics / BatchNorm-backward sums
constexpr int kSpWgradChunks = 64;                 // row chunks of the weight gradient
constexpr int kSpMaxChannels = 128;

template <int MODE>
static bool sp_train_dispatch(int kg, int cout, const SpConvArgs& a, long out_cap, hipStream_t stream, bool launch) {
    const unsigned blocks = (unsigned)((out_cap + kSpBlockRows - 1) / kSpBlockRows);
#define COBEVT_SP_CASE(KGV, NBV) do { if (launch) hipLaunchKernelGGL((sparse_conv_kernel<float, KGV, NBV, MODE>), dim3(blocks), dim3(256), 0, stream, a); \
                                      return true; } while (0)
    if constexpr (MODE == kSpRaw) {                                  // (input row in 8-channel groups, Cout): the backbone's pairs
        if (kg == 1 && cout == 16) COBEVT_SP_CASE(1, 1);
        if (kg == 2 && (cout == 16 || cout == 32)) COBEVT_SP_CASE(2, 1);
        if (kg == 4 && cout == 32) COBEVT_SP_CASE(4, 1);
        if (kg == 4 && cout == 64) COBEVT_SP_CASE(4, 2);
        if (kg == 8 && cout == 64) COBEVT_SP_CASE(8, 2);
        if (kg == 8 && cout == 128) COBEVT_SP_CASE(8, 4);
    } else {                                                         // (d z row in 8-channel groups, Cin): the reversed pairs
        if (kg == 2 && cout == 16) COBEVT_SP_CASE(2, 1);
        if (kg == 4 && (cout == 16 || cout == 32)) COBEVT_SP_CASE(4, 1);
        if (kg == 8 && cout == 32) COBEVT_SP_CASE(8, 1);
        if (kg == 8 && cout == 64) COBEVT_SP_CASE(8, 2);
        if (kg == 16 && cout == 64) COBEVT_SP_CASE(16, 2);
    }
#undef COBEVT_SP_CASE
    return false;
}

// the live rows n cut into `chunks` chunks of whole 32-row tiles: the chunk length
__device__ __forceinline__ int sp_chunk_rows(int n, int chunks) { return ((n + chunks - 1) / chunks + 31) / 32 * 32; }

// per-chunk fp64 sums over the live rows of z (cap, C) about the pivot z[0]: partial[chunk][0][c] = sum (z - pivot), [1] = sum (z - pivot)^2.
// A thread owns channel tid % C and every (256 / C)-th row of its chunk; the 256 / C row lanes are added in lane order
__global__ __launch_bounds__(256) void sp_stat_partial_kernel(const float* __restrict__ z, const int* __restrict__ num, long cap, int C,
                                                              double* __restrict__ partial) {
    __shared__ double lds[2][256];
    const int n = num[0] < cap ? num[0] : (int)cap;
    const int L = sp_chunk_rows(n, kSpStatBlocks);
    const int c = threadIdx.x % C, rl = threadIdx.x / C, R = 256 / C;
    const long lo = (long)blockIdx.x * L, hi = lo + L < n ? lo + L : n;
    double s1 = 0.0, s2 = 0.0;
    if (lo < hi) {
        const double pivot = (double)z[c];
        for (long r = lo + rl; r < hi; r += R) {
            const double d = (double)z[(size_t)r * C + c] - pivot;
            s1 += d; s2 += d * d;
        }
    }
    lds[0][threadIdx.x] = s1; lds[1][threadIdx.x] = s2;
    __syncthreads();
    if (threadIdx.x < C) {
        double t1 = 0.0, t2 = 0.0;
        for (int j = 0; j < R; ++j) { t1 += lds[0][j * C + c]; t2 += lds[1][j * C + c]; }
        partial[((size_t)blockIdx.x * 2 + 0) * C + c] = t1;
        partial[((size_t)blockIdx.x * 2 + 1) * C + c] = t2;
    }
}

// one workgroup: the partials in chunk order -> stat (4, C) fp32 = [mean, rstd, scale = gamma rstd, shift = beta - mean scale] and the
// running statistics.  mode 0: batch statistics (biased variance); n == 0 leaves mean 0 / variance 0 and updates nothing, n == 1 has
// variance 0 and updates nothing (no unbiased variance exists).  mode 1: the frozen running statistics, no update
__global__ __launch_bounds__(kSpMaxChannels) void sp_stat_finish_kernel(const float* __restrict__ z, const int* __restrict__ num, long cap, int C, int mode,
                                                                        const double* __restrict__ partial, const float* __restrict__ gamma,
                                                                        const float* __restrict__ beta, float* __restrict__ rmean, float* __restrict__ rvar,
                                                                        long* __restrict__ nbt, float* __restrict__ stat, float eps, float momentum) {
    const int c = threadIdx.x;
    if (c >= C) return;
    const int n = num[0] < cap ? num[0] : (int)cap;
    double mean = 0.0, var = 0.0;
    if (mode == 1) {
        mean = (double)rmean[c]; var = (double)rvar[c];
    } else if (n > 0) {
        double s1 = 0.0, s2 = 0.0;
        for (int b = 0; b < kSpStatBlocks; ++b) { s1 += partial[((size_t)b * 2 + 0) * C + c]; s2 += partial[((size_t)b * 2 + 1) * C + c]; }
        const double m = s1 / n;
        var = s2 / n - m * m;
        var = var > 0.0 ? var : 0.0;
        mean = (double)z[c] + m;
        if (n > 1 && rmean && rvar) {
            rmean[c] = (float)((1.0 - (double)momentum) * (double)rmean[c] + (double)momentum * mean);
            rvar[c] = (float)((1.0 - (double)momentum) * (double)rvar[c] + (double)momentum * (var * n / (n - 1)));
            if (c == 0 && nbt) nbt[0] += 1;
        }
    }
    const double rstd = 1.0 / sqrt(var + (double)eps), scale = (double)gamma[c] * rstd;
    stat[c] = (float)mean;
    stat[C + c] = (float)rstd;
    stat[2 * C + c] = (float)scale;
    stat[3 * C + c] = (float)((double)beta[c] - mean * scale);
}

// y = relu(z scale + shift) on the live rows, 0 behind them; one thread per four channels
__global__ __launch_bounds__(256) void sp_bn_apply_kernel(const float4* __restrict__ z, const int* __restrict__ num, long cap, int C,
                                                          const float* __restrict__ stat, float4* __restrict__ y) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= cap * (C / 4)) return;
    const long row = e / (C / 4);
    const int ch = (int)(e - row * (C / 4)) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < num[0]) {
        const float4 x = z[e], sc = *(const float4*)(stat + 2 * C + ch), sh = *(const float4*)(stat + 3 * C + ch);
        v = make_float4(fmaxf(fmaf(x.x, sc.x, sh.x), 0.f), fmaxf(fmaf(x.y, sc.y, sh.y), 0.f), fmaxf(fmaf(x.z, sc.z, sh.z), 0.f),
                        fmaxf(fmaf(x.w, sc.w, sh.w), 0.f));
    }
    y[e] = v;
}

// the BatchNorm + ReLU backward's sums, per chunk in fp64: with g = d y [y > 0] and xhat = (z - mean) rstd,
// partial[chunk][0][c] = sum g, [1] = sum g xhat.  Rows at or past num[0] are not read
__global__ __launch_bounds__(256) void sp_bnb_partial_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ z,
                                                             const int* __restrict__ num, long cap, int C, const float* __restrict__ stat,
                                                             double* __restrict__ partial) {
    __shared__ double lds[2][256];
    const int n = num[0] < cap ? num[0] : (int)cap;
    const int L = sp_chunk_rows(n, kSpStatBlocks);
    const int c = threadIdx.x % C, rl = threadIdx.x / C, R = 256 / C;
    const long lo = (long)blockIdx.x * L, hi = lo + L < n ? lo + L : n;
    const double mean = (double)stat[c], rstd = (double)stat[C + c];
    double s1 = 0.0, s2 = 0.0;
    for (long r = lo + rl; r < hi; r += R) {
        const size_t i = (size_t)r * C + c;
        if (y[i] > 0.f) {
            const double g = (double)dy[i];
            s1 += g; s2 += g * (((double)z[i] - mean) * rstd);
        }
    }
    lds[0][threadIdx.x] = s1; lds[1][threadIdx.x] = s2;
    __syncthreads();
    if (threadIdx.x < C) {
        double t1 = 0.0, t2 = 0.0;
        for (int j = 0; j < R; ++j) { t1 += lds[0][j * C + c]; t2 += lds[1][j * C + c]; }
        partial[((size_t)blockIdx.x * 2 + 0) * C + c] = t1;
        partial[((size_t)blockIdx.x * 2 + 1) * C + c] = t2;
    }
}

// d gamma = sum g xhat, d beta = sum g, and coef (3, C) = [k = gamma rstd, A = k rstd d gamma / n, B = k d beta / n] (A = B = 0 with frozen
// statistics or without rows), formed in fp64 and rounded once
__global__ __launch_bounds__(kSpMaxChannels) void sp_bnb_finish_kernel(const int* __restrict__ num, long cap, int C, int mode, const double* __restrict__ partial,
                                                                       const float* __restrict__ gamma, const float* __restrict__ stat,
                                                                       float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ coef) {
    const int c = threadIdx.x;
    if (c >= C) return;
    const int n = num[0] < cap ? num[0] : (int)cap;
    double s1 = 0.0, s2 = 0.0;
    if (n > 0)
        for (int b = 0; b < kSpStatBlocks; ++b) { s1 += partial[((size_t)b * 2 + 0) * C + c]; s2 += partial[((size_t)b * 2 + 1) * C + c]; }
    const double rstd = (double)stat[C + c], k = (double)gamma[c] * rstd;
    dgamma[c] = (float)s2;
    dbeta[c] = (float)s1;
    coef[c] = (float)k;
    coef[C + c] = (mode == 0 && n > 0) ? (float)(k * rstd * s2 / n) : 0.f;
    coef[2 * C + c] = (mode == 0 && n > 0) ? (float)(k * s1 / n) : 0.f;
}

// d z = k g - (B + (z - mean) A) on the live rows, 0 behind them (d y there is not read)
__global__ __launch_bounds__(256) void sp_bnb_apply_kernel(const float4* __restrict__ dy, const float4* __restrict__ y, const float4* __restrict__ z,
                                                           const int* __restrict__ num, long cap, int C, const float* __restrict__ stat,
                                                           const float* __restrict__ coef, float4* __restrict__ dz) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= cap * (C / 4)) return;
    const long row = e / (C / 4);
    const int ch = (int)(e - row * (C / 4)) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < num[0]) {
        const float4 g = dy[e], yy = y[e], x = z[e], mu = *(const float4*)(stat + ch);
        const float4 k = *(const float4*)(coef + ch), A = *(const float4*)(coef + C + ch), B = *(const float4*)(coef + 2 * C + ch);
        v.x = fmaf(k.x, yy.x > 0.f ? g.x : 0.f, -fmaf(x.x - mu.x, A.x, B.x));
        v.y = fmaf(k.y, yy.y > 0.f ? g.y : 0.f, -fmaf(x.y - mu.y, A.y, B.y));
        v.z = fmaf(k.z, yy.z > 0.f ? g.z : 0.f, -fmaf(x.z - mu.z, A.z, B.z));
        v.w = fmaf(k.w, yy.w > 0.f ? g.w : 0.f, -fmaf(x.w - mu.w, A.w, B.w));
    }
    dz[e] = v;
}

// The weight gradient dW[t][co][ci] = sum over the live output rows o of d z[o][co] x[nbr(o, t)][ci] on v_mfma_f32_32x32x2_f32 with the
// ROWS as the k dimension: lanes 0 .. 31 supply row 2 j, lanes 32 .. 63 row 2 j + 1, each lane one channel, so both operands are
// 128-byte loads per half-wave and nothing is transposed.  One wave per workgroup: (row chunk, tap); a 32-row tile in which no row
// has the tap is skipped by one ballot.  -> partial [chunk][tap][Cout pad 32][Cin pad] fp32; chunks past the live rows write nothing
struct SpWgradArgs {
    const float* x;                                // (in_rows, cin_pad)
    const unsigned* in_bits;
    const int* in_prefix;
    const int* in_num;
    const int* row_map;
    const int4* out_idx;
    const int* out_num;
    const float* dz;                               // (out_cap, cout)
    float* partial;
    SpShape si;
    SpGeom g;
    long in_rows, out_cap;
    int taps, cout, cin_pad;
};

// CB / IB: 32-channel blocks of Cout / of the input row (a row of 8 or 16 channels is one block whose upper lanes supply zeros)
template <int CB, int IB>
__global__ __launch_bounds__(64) void sparse_wgrad_kernel(SpWgradArgs a) {
    const int n = a.out_num[0] < a.out_cap ? a.out_num[0] : (int)a.out_cap;
    const int L = sp_chunk_rows(n, kSpWgradChunks);
    const int chunk = blockIdx.x, t = blockIdx.y;
    const long lo = (long)chunk * L;
    if (lo >= n) return;
    const long hi = lo + L < n ? lo + L : n;
    const int lane = threadIdx.x, half = lane >> 5, l32 = lane & 31;
    const int in_live = a.in_num[0];
    const int kyx = a.g.k[1] * a.g.k[2];
    const int kz = t / kyx, rem = t - kz * kyx, ky = rem / a.g.k[2], kx = rem - ky * a.g.k[2];
    f32x16 acc[CB][IB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int ib = 0; ib < IB; ++ib)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[cb][ib][r] = 0.f;
    for (long tile = lo; tile < hi; tile += 32) {
        int nb = -1;
        if (tile + l32 < hi) {
            const int4 c = a.out_idx[tile + l32];
            const int cell = sp_cell(make_int4(c.x, c.y * a.g.s[0] - a.g.p[0] + kz, c.z * a.g.s[1] - a.g.p[1] + ky, c.w * a.g.s[2] - a.g.p[2] + kx), a.si);
            if (cell >= 0) {
                nb = sp_lookup(a.in_bits, a.in_prefix, cell, in_live);
                if (nb >= 0 && a.row_map) nb = a.row_map[nb];
                if (nb >= a.in_rows) nb = -1;
            }
        }
        if (__ballot(nb >= 0) == 0ull) continue;
        for (int j = 0; j < 16; ++j) {
            const int r = 2 * j + half;
            const int src = __shfl(nb, r, 64);
            float av[CB], bv[IB];
#pragma unroll
            for (int cb = 0; cb < CB; ++cb)
                av[cb] = (src >= 0 && cb * 32 + l32 < a.cout) ? a.dz[(size_t)(tile + r) * a.cout + cb * 32 + l32] : 0.f;
#pragma unroll
            for (int ib = 0; ib < IB; ++ib)
                bv[ib] = (src >= 0 && ib * 32 + l32 < a.cin_pad) ? a.x[(size_t)src * a.cin_pad + ib * 32 + l32] : 0.f;
#pragma unroll
            for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                for (int ib = 0; ib < IB; ++ib) acc[cb][ib] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb], bv[ib], acc[cb][ib], 0, 0, 0);
        }
    }
    float* p = a.partial + ((size_t)chunk * a.taps + t) * (CB * 32) * a.cin_pad;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int ib = 0; ib < IB; ++ib) {
            const int ci = ib * 32 + l32;
            if (ci >= a.cin_pad) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = cb * 32 + 8 * (r >> 2) + 4 * half + (r & 3);          // accumulator register r of this lane: row co, column ci
                p[(size_t)co * a.cin_pad + ci] = acc[cb][ib][r];
            }
        }
}

// the chunks in order, in fp64, rounded once -> dW (Cout, kz, ky, kx, Cin), the module's layout, real channels only
__global__ __launch_bounds__(256) void sp_wgrad_reduce_kernel(const float* __restrict__ partial, const int* __restrict__ out_num, long out_cap, int taps,
                                                              int cout, int cout_pad, int cin, int cin_pad, float* __restrict__ dw) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= cout * taps * cin) return;
    const int co = e / (taps * cin), rem = e - co * taps * cin, t = rem / cin, ci = rem - t * cin;
    const int n = out_num[0] < out_cap ? out_num[0] : (int)out_cap;
    double s = 0.0;
    if (n > 0) {
        const int chunks = (n + sp_chunk_rows(n, kSpWgradChunks) - 1) / sp_chunk_rows(n, kSpWgradChunks);
        for (int c = 0; c < chunks; ++c) s += (double)partial[(((size_t)c * taps + t) * cout_pad + co) * cin_pad + ci];
    }
    dw[e] = (float)s;
}

// the adjoint of sparse_dense_kernel: d features[row][c] = d canvas[b][y][x][c D + z] on the live rows, 0 behind them
__global__ __launch_bounds__(256) void sparse_dense_bwd_kernel(const float* __restrict__ dcanvas, const int4* __restrict__ idx, const int* __restrict__ num,
                                                               float* __restrict__ dfeat, SpShape s, int C, long total) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long row = e / C;
    float v = 0.f;
    if (row < num[0]) {
        const int c = (int)(e - row * C);
        const int4 ix = idx[row];
        if (sp_cell(ix, s) >= 0) v = dcanvas[(((size_t)ix.x * s.H + ix.z) * s.W + ix.w) * ((size_t)C * s.D) + (size_t)c * s.D + ix.y];
    }
    dfeat[e] = v;
}

// ---------------------------------------------------------------------------------------------- MeanVFE, densify
// out[p][c] = (sum of the first n = voxel_num_points[p] point slots, in slot order) / max(n, 1) for c < C, 0 for the pad channels and
// for padding rows (coords given and b < 0)
template <typename T>
__global__ __launch_bounds__(256) void mean_vfe_kernel(const float* __restrict__ vf, const int* __restrict__ npts, const int4* __restrict__ coords,
                                                       T* __restrict__ out, long P, int Tn, int C, int Cpad) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= P * Cpad) return;
    const long p = e / Cpad;
    const int c = (int)(e - p * Cpad);
    float v = 0.f;
    if (c < C && (!coords || coords[p].x >= 0)) {
        const int n = npts[p], m = n < 0 ? 0 : (n > Tn ? Tn : n);
        float s = 0.f;
        for (int t = 0; t < m; ++t) s += vf[(p * Tn + t) * C + c];
        v = __fdiv_rn(s, (float)(n > 1 ? n : 1));
    }
    store_elem<T>(out, (size_t)e, v);
}

// rows -> the zero-filled NHWC canvas (N, H, W, C D) with channel index c D + d: HeightCompression's view(N, C D, H, W) of dense()
template <typename T>
__global__ __launch_bounds__(256) void sparse_dense_kernel(const T* __restrict__ feat, const int4* __restrict__ idx, const int* __restrict__ num,
                                                           T* __restrict__ out, SpShape s, int C, long total) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long row = e / C;
    if (row >= num[0]) return;
    const int c = (int)(e - row * C);
    const int4 ix = idx[row];
    if (sp_cell(ix, s) < 0) return;
    out[(((size_t)ix.x * s.H + ix.z) * s.W + ix.w) * ((size_t)C * s.D) + (size_t)c * s.D + ix.y] = feat[e];
}

}  // namespace cobevt

using namespace cobevt;

// dims: [dtype, P, T, C, Cpad]
extern "C" int cobevt_mean_vfe(const float* voxel_features, const int* voxel_num_points, const int* voxel_coords, void* out, const long* dims,
                               hipStream_t stream) {
    if (!dims) return COBEVT_ERR_ARG;
    const long dt = dims[0], P = dims[1], T = dims[2], C = dims[3], Cpad = dims[4];
    if ((dt != 0 && dt != 1) || P < 0 || T < 1 || T > 0x7fffffffL || C < 1 || Cpad < C || Cpad > 64) return COBEVT_ERR_SHAPE;
    if (P > (0x7fffffffL - 256) / Cpad * 256 || P > 0x7fffffffffffL / (T * C)) return COBEVT_ERR_SHAPE;
    if (P == 0) return COBEVT_OK;
    if (!voxel_features || !voxel_num_points || !out) return COBEVT_ERR_ARG;
    if (((uintptr_t)voxel_features | (uintptr_t)voxel_num_points | (uintptr_t)out) & 3 || ((uintptr_t)voxel_coords & 15)) return COBEVT_ERR_SHAPE;
    const unsigned blocks = (unsigned)((P * Cpad + 255) / 256);
    if (dt == 0)
        hipLaunchKernelGGL(mean_vfe_kernel<bf16_t>, dim3(blocks), dim3(256), 0, stream, voxel_features, voxel_num_points, (const int4*)voxel_coords,
                           (bf16_t*)out, P, (int)T, (int)C, (int)Cpad);
    else
        hipLaunchKernelGGL(mean_vfe_kernel<float>, dim3(blocks), dim3(256), 0, stream, voxel_features, voxel_num_points, (const int4*)voxel_coords,
                           (float*)out, P, (int)T, (int)C, (int)Cpad);
    return cobevt::launch_status();
}

// dims: [N, D, H, W]
extern "C" int cobevt_sparse_scratch(const long* dims, long* workspace_ints) {
    if (!dims || !workspace_ints) return COBEVT_ERR_ARG;
    SpShape s;
    const int rc = sp_shape_args(dims, s);
    if (rc != COBEVT_OK) return rc;
    *workspace_ints = sp_index_ints(s);
    return COBEVT_OK;
}

static bool sp_rows_ok(long n, long lo) { return n >= lo && n <= 0x7fffffffL - 256; }

// dims: [N, D, H, W, P, capacity]
extern "C" int cobevt_sparse_index(const int* voxel_coords, int* workspace, int* indices, int* num, int* source, const long* dims,
                                   hipStream_t stream) {
    if (!dims || !workspace || !indices || !num || !source) return COBEVT_ERR_ARG;
    SpShape s;
    const int rc = sp_shape_args(dims, s);
    if (rc != COBEVT_OK) return rc;
    const long P = dims[4], cap = dims[5];
    if (!sp_rows_ok(P, 0) || !sp_rows_ok(cap, 1)) return COBEVT_ERR_SHAPE;
    if (P > 0 && !voxel_coords) return COBEVT_ERR_ARG;
    if (((uintptr_t)voxel_coords | (uintptr_t)workspace | (uintptr_t)indices) & 15) return COBEVT_ERR_SHAPE;
    if (((uintptr_t)num | (uintptr_t)source) & 3) return COBEVT_ERR_SHAPE;
    const SpIndex ix = sp_index(workspace, s);
    sp_clear(ix.bits, 4 * (size_t)sp_words(s), stream);
    const unsigned pb = (unsigned)((P + 255) / 256);
    if (pb) hipLaunchKernelGGL(sp_mark_rows_kernel, dim3(pb), dim3(256), 0, stream, (const int4*)voxel_coords, P, s, ix.bits);
    sp_rank(ix, s, (int4*)indices, num, source, cap, stream);
    if (pb)
        hipLaunchKernelGGL(sp_source_kernel, dim3(pb), dim3(256), 0, stream, (const int4*)voxel_coords, P, s, (const unsigned*)ix.bits,
                           (const int*)ix.prefix, (const int*)num, source);
    return cobevt::launch_status();
}

// dims: [N, D, H, W (the INPUT level), input capacity, output capacity, kernel z y x, stride z y x, pad z y x]
extern "C" int cobevt_sparse_downsample(const int* in_indices, const int* in_num, int* workspace, int* indices, int* num, const long* dims,
                                        hipStream_t stream) {
    if (!dims || !in_indices || !in_num || !workspace || !indices || !num) return COBEVT_ERR_ARG;
    SpShape si, so;
    SpGeom g;
    int rc = sp_shape_args(dims, si);
    if (rc == COBEVT_OK) rc = sp_geom_args(dims + 6, g);
    if (rc == COBEVT_OK) rc = sp_out_shape(si, g, so);
    if (rc != COBEVT_OK) return rc;
    const long in_cap = dims[4], cap = dims[5];
    if (!sp_rows_ok(in_cap, 1) || !sp_rows_ok(cap, 1)) return COBEVT_ERR_SHAPE;
    if (((uintptr_t)in_indices | (uintptr_t)workspace | (uintptr_t)indices) & 15) return COBEVT_ERR_SHAPE;
    if (((uintptr_t)num | (uintptr_t)in_num) & 3) return COBEVT_ERR_SHAPE;
    const SpIndex ix = sp_index(workspace, so);
    sp_clear(ix.bits, 4 * (size_t)sp_words(so), stream);
    hipLaunchKernelGGL(sp_mark_down_kernel, dim3((unsigned)((in_cap + 255) / 256)), dim3(256), 0, stream, (const int4*)in_indices, in_num, in_cap,
                       si, g, so, ix.bits);
    sp_rank(ix, so, (int4*)indices, num, nullptr, cap, stream);
    return cobevt::launch_status();
}

// dims: [dtype, N, D, H, W (the INPUT level), input feature rows, output capacity, input row in channels, Cout, kernel z y x, stride z y x,
// pad z y x]
extern "C" int cobevt_sparse_conv(const void* in, const int* in_workspace, const int* in_num, const int* row_map, const int* out_indices,
                                  const int* out_num, const void* weight, const float* bias, void* out, const long* dims, hipStream_t stream) {
    if (!dims || !in || !in_workspace || !in_num || !out_indices || !out_num || !weight || !bias || !out) return COBEVT_ERR_ARG;
    SpConvArgs a;
    int rc = sp_shape_args(dims + 1, a.si);
    if (rc == COBEVT_OK) rc = sp_geom_args(dims + 9, a.g);
    if (rc != COBEVT_OK) return rc;
    const long dt = dims[0], in_rows = dims[5], out_cap = dims[6], cin_pad = dims[7], cout = dims[8];
    if ((dt != 0 && dt != 1) || !sp_rows_ok(in_rows, 1) || !sp_rows_ok(out_cap, 1) || cin_pad < 1 || cin_pad > 64 || cout < 16 || cout > 128)
        return COBEVT_ERR_SHAPE;
    if (((uintptr_t)in | (uintptr_t)in_workspace | (uintptr_t)out_indices | (uintptr_t)weight | (uintptr_t)bias | (uintptr_t)out) & 15)
        return COBEVT_ERR_SHAPE;
    if (((uintptr_t)in_num | (uintptr_t)out_num | (uintptr_t)row_map) & 3) return COBEVT_ERR_SHAPE;
    const SpIndex ix = sp_index((int*)in_workspace, a.si);
    a.in = in; a.in_bits = ix.bits; a.in_prefix = ix.prefix; a.in_num = in_num; a.row_map = row_map;
    a.out_idx = (const int4*)out_indices; a.out_num = out_num; a.wgt = weight; a.bias = bias; a.out = out;
    a.in_rows = in_rows; a.out_cap = out_cap; a.taps = a.g.k[0] * a.g.k[1] * a.g.k[2]; a.cout = (int)cout;
    if (!(dt == 0 ? sp_conv_dispatch<bf16_t>((int)cin_pad, a, out_cap, stream, false) : sp_conv_dispatch<float>((int)cin_pad, a, out_cap, stream, false)))
        return COBEVT_ERR_SHAPE;
    if (dt == 0) sp_conv_dispatch<bf16_t>((int)cin_pad, a, out_cap, stream, true);
    else sp_conv_dispatch<float>((int)cin_pad, a, out_cap, stream, true);
    return cobevt::launch_status();
}

// dims: [dtype, N, D, H, W, capacity, C]
extern "C" int cobevt_sparse_dense(const void* features, const int* indices, const int* num, void* out, const long* dims, hipStream_t stream) {
    if (!dims || !features || !indices || !num || !out) return COBEVT_ERR_ARG;
    SpShape s;
    const int rc = sp_shape_args(dims + 1, s);
    if (rc != COBEVT_OK) return rc;
    const long dt = dims[0], cap = dims[5], C = dims[6];
    if ((dt != 0 && dt != 1) || !sp_rows_ok(cap, 1) || C < 1 || C > 4096 || cap > (0x7fffffffL - 256) / C * 256) return COBEVT_ERR_SHAPE;
    if ((((uintptr_t)features | (uintptr_t)num) & 3) || (((uintptr_t)indices | (uintptr_t)out) & 15)) return COBEVT_ERR_SHAPE;
    const size_t es = dt == 0 ? 2 : 4;
    sp_clear(out, (size_t)sp_cells(s) * (size_t)C * es, stream);
    const long total = cap * C;
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (dt == 0)
        hipLaunchKernelGGL(sparse_dense_kernel<bf16_t>, dim3(blocks), dim3(256), 0, stream, (const bf16_t*)features, (const int4*)indices, num,
                           (bf16_t*)out, s, (int)C, total);
    else
        hipLaunchKernelGGL(sparse_dense_kernel<float>, dim3(blocks), dim3(256), 0, stream, (const float*)features, (const int4*)indices, num,
                           (float*)out, s, (int)C, total);
    return cobevt::launch_status();
}

// ---------------------------------------------------------------------------------------------- training entry points (fp32 rows)
static bool sp_train_channels(long c) { return c == 16 || c == 32 || c == 64 || c == 128; }
// (input row in channels, Cout) of the backbone: <= 8 -> 16 as the 8-channel row, and SparseConvPlan.PAIRS
static bool sp_train_pair(long cin_pad, long cout) {
    return (cin_pad == 8 && cout == 16) || (cin_pad == 16 && (cout == 16 || cout == 32)) || (cin_pad == 32 && (cout == 32 || cout == 64)) ||
           (cin_pad == 64 && (cout == 64 || cout == 128));
}
static long sp_wgrad_floats(long cin_pad, long cout, long taps) { return (long)kSpWgradChunks * taps * ((cout + 31) / 32 * 32) * cin_pad; }
static long sp_stat_doubles() { return (long)kSpStatBlocks * 2 * kSpMaxChannels; }

// dims: [input row in channels, Cout, taps] -> sizes[0] = floats of cobevt_sparse_conv_wgrad's scratch (row chunks x taps x Cout padded to
// 32 x input row), sizes[1] = doubles of the scratch of cobevt_sparse_bn_relu / cobevt_sparse_bn_relu_bwd; neither depends on a capacity
extern "C" int cobevt_sparse_train_scratch(const long* dims, long* sizes) {
    if (!dims || !sizes) return COBEVT_ERR_ARG;
    if (!sp_train_pair(dims[0], dims[1]) || (dims[2] != 27 && dims[2] != 3)) return COBEVT_ERR_SHAPE;
    sizes[0] = sp_wgrad_floats(dims[0], dims[1], dims[2]);
    sizes[1] = sp_stat_doubles();
    return COBEVT_OK;
}

// dims: [N, D, H, W (the INPUT level), input feature rows, output capacity, input row in channels, Cout, kernel z y x, stride z y x, pad z y x]
extern "C" int cobevt_sparse_conv_raw(const float* in, const int* in_workspace, const int* in_num, const int* row_map, const int* out_indices,
                                      const int* out_num, const float* weight, float* out, const long* dims, hipStream_t stream) {
    if (!dims || !in || !in_workspace || !in_num || !out_indices || !out_num || !weight || !out) return COBEVT_ERR_ARG;
    SpConvArgs a;
    int rc = sp_shape_args(dims, a.si);
    if (rc == COBEVT_OK) rc = sp_geom_args(dims + 8, a.g);
    if (rc != COBEVT_OK) return rc;
    const long in_rows = dims[4], out_cap = dims[5], cin_pad = dims[6], cout = dims[7];
    if (!sp_rows_ok(in_rows, 1) || !sp_rows_ok(out_cap, 1) || !sp_train_pair(cin_pad, cout)) return COBEVT_ERR_SHAPE;
    if (((uintptr_t)in | (uintptr_t)in_workspace | (uintptr_t)out_indices | (uintptr_t)weight | (uintptr_t)out) & 15) return COBEVT_ERR_SHAPE;
    if (((uintptr_t)in_num | (uintptr_t)out_num | (uintptr_t)row_map) & 3) return COBEVT_ERR_SHAPE;
    const SpIndex ix = sp_index((int*)in_workspace, a.si);
    a.in = in; a.in_bits = ix.bits; a.in_prefix = ix.prefix; a.in_num = in_num; a.row_map = row_map;
    a.out_idx = (const int4*)out_indices; a.out_num = out_num; a.wgt = weight; a.bias = nullptr; a.out = out;
    a.in_rows = in_rows; a.out_cap = out_cap; a.taps = a.g.k[0] * a.g.k[1] * a.g.k[2]; a.cout = (int)cout;
    if (!sp_train_dispatch<kSpRaw>((int)cin_pad / 8, (int)cout, a, out_cap, stream, false)) return COBEVT_ERR_SHAPE;
    sp_train_dispatch<kSpRaw>((int)cin_pad / 8, (int)cout, a, out_cap, stream, true);
    return cobevt::launch_status();
}

// dims: [N, D, H, W (the convolution's INPUT level), input capacity, output capacity, Cin (16 / 32 / 64), Cout, kernel, stride, pad].
// dz (output capacity, Cout) by the OUTPUT level's rows (out_workspace / out_num), weight_t [taps][Cin padded to 32][Cout] ->
// dx (input capacity, Cin) by the input level's rows (in_indices / in_num); rows at or past in_num[0] are written as 0
extern "C" int cobevt_sparse_conv_dgrad(const float* dz, const int* out_workspace, const int* out_num, const int* in_indices, const int* in_num,
                                        const float* weight_t, float* dx, const long* dims, hipStream_t stream) {
    if (!dims || !dz || !out_workspace || !out_num || !in_indices || !in_num || !weight_t || !dx) return COBEVT_ERR_ARG;
    SpConvArgs a;
    SpShape si;
    int rc = sp_shape_args(dims, si);
    if (rc == COBEVT_OK) rc = sp_geom_args(dims + 8, a.g);
    if (rc == COBEVT_OK) rc = sp_out_shape(si, a.g, a.si);           // the level that is looked up is the convolution's output
    if (rc != COBEVT_OK) return rc;
    const long in_cap = dims[4], out_cap = dims[5], cin = dims[6], cout = dims[7];
    if (!sp_rows_ok(in_cap, 1) || !sp_rows_ok(out_cap, 1) || cin < 16 || !sp_train_pair(cin, cout)) return COBEVT_ERR_SHAPE;
    if (((uintptr_t)dz | (uintptr_t)out_workspace | (uintptr_t)in_indices | (uintptr_t)weight_t | (uintptr_t)dx) & 15) return COBEVT_ERR_SHAPE;
    if (((uintptr_t)in_num | (uintptr_t)out_num) & 3) return COBEVT_ERR_SHAPE;
    const SpIndex ix = sp_index((int*)out_workspace, a.si);
    a.in = dz; a.in_bits = ix.bits; a.in_prefix = ix.prefix; a.in_num = out_num; a.row_map = nullptr;
    a.out_idx = (const int4*)in_indices; a.out_num = in_num; a.wgt = weight_t; a.bias = nullptr; a.out = dx;
    a.in_rows = out_cap; a.out_cap = in_cap; a.taps = a.g.k[0] * a.g.k[1] * a.g.k[2]; a.cout = (int)cin;
    if (!sp_train_dispatch<kSpRawT>((int)cout / 8, (int)cin, a, in_cap, stream, false)) return COBEVT_ERR_SHAPE;
    sp_train_dispatch<kSpRawT>((int)cout / 8, (int)cin, a, in_cap, stream, true);
    return cobevt::launch_status();
}

static bool sp_bn_dims(const long* dims) {
    return sp_rows_ok(dims[0], 1) && sp_train_channels(dims[1]) && (dims[2] == 0 || dims[2] == 1) && dims[3] >= sp_stat_doubles() &&
           dims[0] <= (0x7fffffffL - 256) / (dims[1] / 4);
}

// dims: [capacity, C (16 / 32 / 64 / 128), mode (0 batch statistics, 1 frozen running statistics), doubles of `partial`].
// z (capacity, C) -> stat (4, C) fp32 [mean, rstd, scale, shift]; mode 0 updates running_mean / running_var (fp32) and
// num_batches_tracked (int64) in place when all three are given and num[0] > 1; y (capacity, C) = relu(z scale + shift), 0 at and past
// num[0], or null for the statistics alone
extern "C" int cobevt_sparse_bn_relu(const float* z, const int* num, const float* gamma, const float* beta, float* running_mean, float* running_var,
                                     long* num_batches_tracked, float* stat, double* partial, float* y, const long* dims, float eps, float momentum,
                                     hipStream_t stream) {
    if (!dims || !z || !num || !gamma || !beta || !stat || !partial) return COBEVT_ERR_ARG;
    if (dims[2] == 1 && (!running_mean || !running_var)) return COBEVT_ERR_ARG;
    if (!sp_bn_dims(dims) || !(eps > 0.f) || !(momentum >= 0.f && momentum <= 1.f)) return COBEVT_ERR_SHAPE;
    if (((uintptr_t)z | (uintptr_t)stat | (uintptr_t)y) & 15) return COBEVT_ERR_SHAPE;
    if (((uintptr_t)num | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)running_mean | (uintptr_t)running_var) & 3) return COBEVT_ERR_SHAPE;
    if (((uintptr_t)partial | (uintptr_t)num_batches_tracked) & 7) return COBEVT_ERR_SHAPE;
    const long cap = dims[0];
    const int C = (int)dims[1], mode = (int)dims[2];
    if (mode == 0) hipLaunchKernelGGL(sp_stat_partial_kernel, dim3(kSpStatBlocks), dim3(256), 0, stream, z, num, cap, C, partial);
    const bool track = mode == 0 && running_mean && running_var;
    hipLaunchKernelGGL(sp_stat_finish_kernel, dim3(1), dim3(kSpMaxChannels), 0, stream, z, num, cap, C, mode, (const double*)partial, gamma, beta,
                       (track || mode == 1) ? running_mean : nullptr, (track || mode == 1) ? running_var : nullptr, track ? num_batches_tracked : nullptr,
                       stat, eps, momentum);
    if (y)
        hipLaunchKernelGGL(sp_bn_apply_kernel, dim3((unsigned)((cap * (C / 4) + 255) / 256)), dim3(256), 0, stream, (const float4*)z, num, cap, C,
                           (const float*)stat, (float4*)y);
    return cobevt::launch_status();
}

// dims as cobevt_sparse_bn_relu.  dy, y, z (capacity, C), stat of the forward -> dgamma (C), dbeta (C), coef (3, C) [k, A, B] and
// dz (capacity, C) = k g - (B + (z - mean) A), g = dy [y > 0]; 0 at and past num[0], where dy is not read
extern "C" int cobevt_sparse_bn_relu_bwd(const float* dy, const float* y, const float* z, const int* num, const float* gamma, const float* stat,
                                         double* partial, float* dgamma, float* dbeta, float* coef, float* dz, const long* dims, hipStream_t stream) {
    if (!dims || !dy || !y || !z || !num || !gamma || !stat || !partial || !dgamma || !dbeta || !coef || !dz) return COBEVT_ERR_ARG;
    if (!sp_bn_dims(dims)) return COBEVT_ERR_SHAPE;
    if (((uintptr_t)dy | (uintptr_t)y | (uintptr_t)z | (uintptr_t)stat | (uintptr_t)coef | (uintptr_t)dz) & 15) return COBEVT_ERR_SHAPE;
    if (((uintptr_t)num | (uintptr_t)gamma | (uintptr_t)dgamma | (uintptr_t)dbeta) & 3 || ((uintptr_t)partial & 7)) return COBEVT_ERR_SHAPE;
    const long cap = dims[0];
    const int C = (int)dims[1], mode = (int)dims[2];
    hipLaunchKernelGGL(sp_bnb_partial_kernel, dim3(kSpStatBlocks), dim3(256), 0, stream, dy, y, z, num, cap, C, stat, partial);
    hipLaunchKernelGGL(sp_bnb_finish_kernel, dim3(1), dim3(kSpMaxChannels), 0, stream, num, cap, C, mode, (const double*)partial, gamma, stat, dgamma,
                       dbeta, coef);
    hipLaunchKernelGGL(sp_bnb_apply_kernel, dim3((unsigned)((cap * (C / 4) + 255) / 256)), dim3(256), 0, stream, (const float4*)dy, (const float4*)y,
                       (const float4*)z, num, cap, C, stat, (const float*)coef, (float4*)dz);
    return cobevt::launch_status();
}

// dims: [N, D, H, W (the INPUT level), input feature rows, output capacity, Cin, input row in channels, Cout, kernel, stride, pad, floats of
// `partial`].  x as cobevt_sparse_conv_raw's `in` (row_map honoured), dz (output capacity, Cout) -> dw (Cout, kz, ky, kx, Cin) fp32
extern "C" int cobevt_sparse_conv_wgrad(const float* x, const int* in_workspace, const int* in_num, const int* row_map, const int* out_indices,
                                        const int* out_num, const float* dz, float* partial, float* dw, const long* dims, hipStream_t stream) {
    if (!dims || !x || !in_workspace || !in_num || !out_indices || !out_num || !dz || !partial || !dw) return COBEVT_ERR_ARG;
    SpWgradArgs a;
    int rc = sp_shape_args(dims, a.si);
    if (rc == COBEVT_OK) rc = sp_geom_args(dims + 9, a.g);
    if (rc != COBEVT_OK) return rc;
    const long in_rows = dims[4], out_cap = dims[5], cin = dims[6], cin_pad = dims[7], cout = dims[8], taps = (long)a.g.k[0] * a.g.k[1] * a.g.k[2];
    if (!sp_rows_ok(in_rows, 1) || !sp_rows_ok(out_cap, 1) || !sp_train_pair(cin_pad, cout) || cin < 1 || cin > cin_pad || (cin_pad > 8 && cin != cin_pad))
        return COBEVT_ERR_SHAPE;
    if (dims[18] < sp_wgrad_floats(cin_pad, cout, taps)) return COBEVT_ERR_SHAPE;
    if (((uintptr_t)x | (uintptr_t)in_workspace | (uintptr_t)out_indices | (uintptr_t)dz | (uintptr_t)partial | (uintptr_t)dw) & 15) return COBEVT_ERR_SHAPE;
    if (((uintptr_t)in_num | (uintptr_t)out_num | (uintptr_t)row_map) & 3) return COBEVT_ERR_SHAPE;
    const SpIndex ix = sp_index((int*)in_workspace, a.si);
    a.x = x; a.in_bits = ix.bits; a.in_prefix = ix.prefix; a.in_num = in_num; a.row_map = row_map; a.out_idx = (const int4*)out_indices;
    a.out_num = out_num; a.dz = dz; a.partial = partial; a.in_rows = in_rows; a.out_cap = out_cap; a.taps = (int)taps; a.cout = (int)cout;
    a.cin_pad = (int)cin_pad;
    const dim3 grid(kSpWgradChunks, (unsigned)taps);
    const int cb = (int)(cout + 31) / 32, ib = (int)(cin_pad + 31) / 32;
    if (cb == 1 && ib == 1) hipLaunchKernelGGL((sparse_wgrad_kernel<1, 1>), grid, dim3(64), 0, stream, a);
    else if (cb == 2 && ib == 1) hipLaunchKernelGGL((sparse_wgrad_kernel<2, 1>), grid, dim3(64), 0, stream, a);
    else if (cb == 2 && ib == 2) hipLaunchKernelGGL((sparse_wgrad_kernel<2, 2>), grid, dim3(64), 0, stream, a);
    else hipLaunchKernelGGL((sparse_wgrad_kernel<4, 2>), grid, dim3(64), 0, stream, a);
    const long total = cout * taps * cin;
    hipLaunchKernelGGL(sp_wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const float*)partial, out_num, out_cap, (int)taps,
                       (int)cout, cb * 32, (int)cin, (int)cin_pad, dw);
    return cobevt::launch_status();
}

// dims: [N, D, H, W, capacity, C].  dcanvas (N, H, W, C D) fp32 -> dfeatures (capacity, C): the adjoint of cobevt_sparse_dense
extern "C" int cobevt_sparse_dense_bwd(const float* dcanvas, const int* indices, const int* num, float* dfeatures, const long* dims, hipStream_t stream) {
    if (!dims || !dcanvas || !indices || !num || !dfeatures) return COBEVT_ERR_ARG;
    SpShape s;
    const int rc = sp_shape_args(dims, s);
    if (rc != COBEVT_OK) return rc;
    const long cap = dims[4], C = dims[5];
    if (!sp_rows_ok(cap, 1) || C < 1 || C > 4096 || cap > (0x7fffffffL - 256) / C * 256) return COBEVT_ERR_SHAPE;
    if ((((uintptr_t)dcanvas | (uintptr_t)dfeatures | (uintptr_t)num) & 3) || ((uintptr_t)indices & 15)) return COBEVT_ERR_SHAPE;
    const long total = cap * C;
    hipLaunchKernelGGL(sparse_dense_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, dcanvas, (const int4*)indices, num, dfeatures, s,
                       (int)C, total);
    return cobevt::launch_status();
}
