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

// KG: 32-byte k-groups of an input row; NB: 32-channel blocks of the (padded) output
template <typename T, int KG, int NB>
__global__ __launch_bounds__(256) void sparse_conv_kernel(SpConvArgs a) {
    constexpr int ES = Elem<T>::kBytes;
    constexpr int ROWB = KG * 32;
    __shared__ int tab[kSpMaxTaps * kSpBlockRows];                   // [tap][row of the workgroup]: the input row, or -1
    const int live = a.out_num[0] < a.out_cap ? a.out_num[0] : (int)a.out_cap;       // (num[0] <= capacity by construction)
    const long r0 = (long)blockIdx.x * kSpBlockRows;
    if (r0 >= live) return;                                          // uniform over the workgroup
    const int in_live = a.in_num[0];
    const int kyx = a.g.k[1] * a.g.k[2];
    for (int e = threadIdx.x; e < a.taps * kSpBlockRows; e += 256) {
        const int t = e / kSpBlockRows, r = e % kSpBlockRows;
        int v = -1;
        if (r0 + r < live) {
            const int4 c = a.out_idx[r0 + r];
            const int kz = t / kyx, rem = t - kz * kyx, ky = rem / a.g.k[2], kx = rem - ky * a.g.k[2];
            const int cell = sp_cell(make_int4(c.x, c.y * a.g.s[0] - a.g.p[0] + kz, c.z * a.g.s[1] - a.g.p[1] + ky,
                                               c.w * a.g.s[2] - a.g.p[2] + kx), a.si);
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
    if (r0 + wave * 32 >= live) return;                              // uniform over the wave; no barrier follows
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
    if (row >= live) return;
    unsigned char* o = (unsigned char*)a.out + (size_t)row * a.cout * ES;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ch = b * 32 + 8 * q + 4 * half;                // the lane's accumulator quad q: four consecutive channels of its row
            if (ch >= a.cout) continue;
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
