// Voxelisation of raw LiDAR points (gfx950): spconv's points_to_voxel with OpenCOOD's collate, in front of pillar_vfe.hip.
// points (M, 4) fp32 [x, y, z, intensity] of N agents (rows offsets[a] .. offsets[a + 1] of agent a, device int32) -> the voxel dict
// the pillar front end reads: voxel_features (N max_voxels, T, 4), voxel_coords [a, 0, y, x], voxel_num_points, and num_voxels (N).
//
// Semantics (sequential, per agent, in input order): a point is dropped when a coordinate is not finite, when an optional mask
// (pcd_utils.mask_points_by_range :54-58, mask_ego_points :79-80) removes it or when floor((p - lo) / v) falls outside the grid; the
// first kept point of a cell opens a voxel (numbered in order of first appearance, at most max_voxels per agent; cells past the cap
// are dropped with all their points); a voxel keeps the first T points of its cell.  fp32 / int32 only and identical in all three
// libraries; subtract and divide are the correctly rounded ones (a reciprocal multiply moves points that sit on a cell edge).
//
// Deterministic parallel form - nothing depends on the order in which workgroups or atomics complete:
//   1 clear      first <- INT_MAX, count <- 0, fill <- 0 per (agent, y, x); voxel -> cell map <- -1
//   2 classify   one thread per point: cell index (or -1); atomicMin(first[cell], i), atomicAdd(count[cell], 1) - integer atomics
//                whose FINAL values do not depend on arrival order
//   3 reduce     the pair (leader, leader ? count[cell] : 0), leader = (first[cell] == i), summed per 1024 points
//   4 scan       one workgroup scans the partials (serial over chunks of 1024: no workgroup waits on another); N + 1 more workgroups
//                count the leaders between an agent's offset and the start of its 1024-block, which restarts the numbering per agent
//   5 apply      leaders get their voxel row (row >= max_voxels: the cell is dropped) and the start of the cell's bucket
//   6 fill       every kept point appends its index to its cell's bucket: the ORDER in a bucket is arbitrary, its content is a set
//   7 select     one half-wave per voxel row: the T smallest indices of the bucket, ascending, by a bitonic sort of each 32-index
//                chunk and a keep-lower-half merge against the running set, all in ds_swizzle exchanges; then one 16-byte load and
//                one 16-byte store per kept point.  Rows without a voxel get coords [-1, 0, 0, 0] / 0 points; their features are
//                NOT written.
// No floating-point atomics, no host read-back, no allocation: the workspace comes from the caller (cobevt_voxelize_scratch).
//
// The 3-D form (cobevt_voxelize3d_points: cells (z, y, x), voxel_coords [a, z, y, x], in front of sparse_conv.hip's MeanVFE /
// VoxelBackBone8x) is the same seven launches with ONE thing replaced: the tables are not indexed by the cell - one entry per (agent,
// z, y, x) is 1.48 GB per agent on the backbone's (41, 1600, 1408) grid - but by the SLOT the cell's 64-bit key
// agent * (nx ny nz) + (z ny + y) nx + x occupies in an open-addressed hash table of `slots` > M entries (a power of two, by default
// the smallest >= 2 M).  classify inserts the key by a 64-bit atomicCAS on the key word under linear probing - bounded by `slots`
// iterations and waiting on no other thread - and from there the slot plays the part of the dense cell index in every step; apply
// and select decode the agent and (z, y, x) from key[slot].  WHICH slot a key lands in depends on arrival order; that is internal
// state: every output depends on the slot only through first / count / start of the key that owns it.  The cost follows M, slots and
// N max_voxels, never the grid.
#include "points_common.hpp"           // the offsets / mask device functions, shared with bev_points.hip and cloud_prep.hip

namespace cobevt {

constexpr int kScanItems = 4;                       // points per thread of the reduce / apply launches
constexpr int kScanBlock = 256 * kScanItems;        // points per workgroup there
constexpr int kIntMax = 0x7fffffff;

constexpr unsigned long long kEmptyKey = ~0ull;    // no cell has it: keys are below 2^62

// tables: entries of the four per-cell tables - N ny nx cells (dense, nz = 1) or the hash table's slots (3-D)
struct VoxelArgs {
    long M, Pcap, tables;
    int N, T, max_voxels, nx, ny, nz, range_mask, ego_mask;
    float lo[3], hi[3], v[3];
};

// the workspace, in ints: in the 3-D form the 64-bit key of every slot (in front: 8-byte aligned when the workspace is), then four
// tables of one entry per (agent, y, x) or per slot - separate arrays: with the four words of a cell in one 16-byte
// record the two atomics of a point fall into one cache line and the classify launch measured 166 us against 97 us -,
// the voxel -> cell map, per-point cell and bucket arrays, the scan partials (pairs, one more than there are blocks: the totals) and
// the per-agent leader counts
struct VoxelWs {
    unsigned long long* key;
    int *first, *count, *fill, *start, *vox_cell, *cellof, *bucket, *part, *agent_part;
};
__host__ __device__ inline long scan_blocks(long M) { const long b = (M + kScanBlock - 1) / kScanBlock; return b > 0 ? b : 1; }
template <bool HASH> static long voxel_ws_ints(const VoxelArgs& a) {
    return (HASH ? 6 : 4) * a.tables + a.Pcap + 2 * a.M + 2 * (scan_blocks(a.M) + 1) + (a.N + 1);
}
template <bool HASH> static VoxelWs voxel_ws(int* w, const VoxelArgs& a) {
    const long cells = a.tables;
    VoxelWs s;
    s.key = HASH ? (unsigned long long*)w : nullptr;
    s.first = HASH ? w + 2 * cells : w; s.count = s.first + cells; s.fill = s.count + cells; s.start = s.fill + cells;
    s.vox_cell = s.start + cells; s.cellof = s.vox_cell + a.Pcap; s.bucket = s.cellof + a.M;
    s.part = s.bucket + a.M; s.agent_part = s.part + 2 * (scan_blocks(a.M) + 1);
    return s;
}

// value of lane (lane ^ X) of the same 32-lane group (ds_swizzle bit mode: and 0x1f, or 0, xor X)
template <int X> __device__ __forceinline__ int swz_xor_i(int v) { return __builtin_amdgcn_ds_swizzle(v, (X << 10) | 0x1f); }
template <int J> __device__ __forceinline__ int cmp_exchange(int v, bool keep_min) {
    const int o = swz_xor_i<J>(v);
    return keep_min ? min(v, o) : max(v, o);
}
// ascending bitonic merge of a bitonic sequence held one value per lane of a half-wave
__device__ __forceinline__ int bitonic_merge32(int v, int t) {
    v = cmp_exchange<16>(v, (t & 16) == 0);
    v = cmp_exchange<8>(v, (t & 8) == 0);
    v = cmp_exchange<4>(v, (t & 4) == 0);
    v = cmp_exchange<2>(v, (t & 2) == 0);
    v = cmp_exchange<1>(v, (t & 1) == 0);
    return v;
}
// ascending bitonic sort over the 32 lanes of a half-wave: stage K sorts runs of K lanes, alternately ascending and descending
template <int K, int J> __device__ __forceinline__ int sort_step(int v, int t) {
    return cmp_exchange<J>(v, ((t & J) == 0) == ((t & K) == 0));
}
__device__ __forceinline__ int bitonic_sort32(int v, int t) {
    v = sort_step<2, 1>(v, t);
    v = sort_step<4, 2>(v, t); v = sort_step<4, 1>(v, t);
    v = sort_step<8, 4>(v, t); v = sort_step<8, 2>(v, t); v = sort_step<8, 1>(v, t);
    v = sort_step<16, 8>(v, t); v = sort_step<16, 4>(v, t); v = sort_step<16, 2>(v, t); v = sort_step<16, 1>(v, t);
    return bitonic_merge32(v, t);
}

// exclusive scan of a pair over the NT threads of the workgroup (e*), and its totals (t*); lds: 2 * NT / 64 ints
template <int NT>
__device__ __forceinline__ void block_scan2(int va, int vb, int* lds, int& ea, int& eb, int& ta, int& tb) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int ia = va, ib = vb;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int xa = __shfl_up(ia, o, 64), xb = __shfl_up(ib, o, 64);
        if (lane >= o) { ia += xa; ib += xb; }
    }
    if (lane == 63) { lds[2 * w] = ia; lds[2 * w + 1] = ib; }
    __syncthreads();
    int ba = 0, bb = 0;
    ta = 0; tb = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) {
        const int xa = lds[2 * k], xb = lds[2 * k + 1];
        if (k < w) { ba += xa; bb += xb; }
        ta += xa; tb += xb;
    }
    __syncthreads();
    ea = ba + ia - va; eb = bb + ib - vb;
}

// the cell's 64-bit key and its place in the table.  splitmix64's finaliser spreads the keys of neighbouring cells over the table
__device__ __forceinline__ unsigned long long mix_key(unsigned long long k) {
    k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27; k *= 0x94d049bb133111ebull;
    return k ^ (k >> 31);
}
// the slot that holds `key`, claiming the first empty one on its probe sequence: whoever of the threads with one key gets there first
// writes it, all of them leave with the same slot.  At most `slots` probes, none of which waits for another thread; slots > M keeps
// an empty slot in the table, so the -1 (the point is dropped) after a full round cannot happen.
__device__ __forceinline__ int hash_slot(unsigned long long* __restrict__ keys, long slots, unsigned long long key) {
    const unsigned long long mask = (unsigned long long)slots - 1;
    unsigned long long h = mix_key(key) & mask;
    for (long it = 0; it < slots; ++it) {
        const unsigned long long seen = atomicCAS(&keys[h], kEmptyKey, key);
        if (seen == kEmptyKey || seen == key) return (int)h;
        h = (h + 1) & mask;
    }
    return -1;
}
// the cell of a table entry -> agent and (z, y, x)
template <bool HASH> __device__ __forceinline__ int cell_agent(const VoxelWs& s, const VoxelArgs& a, int cell) {
    if constexpr (HASH) return (int)(s.key[cell] / ((unsigned long long)a.nz * a.ny * a.nx));
    else return cell / (a.ny * a.nx);
}
template <bool HASH> __device__ __forceinline__ int4 cell_coords(const VoxelWs& s, const VoxelArgs& a, int cell) {
    if constexpr (HASH) {
        const unsigned long long per_agent = (unsigned long long)a.nz * a.ny * a.nx, k = s.key[cell];
        const unsigned long long agent = k / per_agent, r = k - agent * per_agent, zy = r / a.nx;
        return make_int4((int)agent, (int)(zy / a.ny), (int)(zy % a.ny), (int)(r - zy * a.nx));
    } else {
        const int per_agent = a.ny * a.nx;
        const int agent = cell / per_agent, r = cell - agent * per_agent;
        return make_int4(agent, 0, r / a.nx, r % a.nx);
    }
}

template <bool HASH> __global__ __launch_bounds__(256) void voxel_clear_kernel(VoxelWs s, long cells, long Pcap) {
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < cells; i += stride) {
        if constexpr (HASH) s.key[i] = kEmptyKey;
        s.first[i] = kIntMax; s.count[i] = 0; s.fill[i] = 0;
    }
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < Pcap; i += stride) s.vox_cell[i] = -1;
}

template <bool HASH>
__global__ __launch_bounds__(256) void voxel_classify_kernel(const float4* __restrict__ points, const int* __restrict__ offsets, VoxelWs s,
                                                             VoxelArgs a) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.M) return;
    const int agent = point_agent(offsets, a.N, i, a.M);
    int cell = -1;
    if (agent >= 0) {
        const float4 p = points[i];
        bool keep = isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && point_masks_keep(p, a.lo, a.hi, a.range_mask, a.ego_mask);
        // floor((p - lo) / v) with the rounded subtract and divide, compared as floats (a quotient past the int range drops the point)
        const float cx = floorf(__fdiv_rn(__fsub_rn(p.x, a.lo[0]), a.v[0]));
        const float cy = floorf(__fdiv_rn(__fsub_rn(p.y, a.lo[1]), a.v[1]));
        const float cz = floorf(__fdiv_rn(__fsub_rn(p.z, a.lo[2]), a.v[2]));
        keep = keep && cx >= 0.f && cx < (float)a.nx && cy >= 0.f && cy < (float)a.ny && cz >= 0.f && cz < (float)a.nz;
        if (keep) {
            if constexpr (HASH)
                cell = hash_slot(s.key, a.tables, (((unsigned long long)agent * a.nz + (int)cz) * a.ny + (int)cy) * a.nx + (int)cx);
            else
                cell = (agent * a.ny + (int)cy) * a.nx + (int)cx;
        }
        if (cell >= 0) {
            atomicMin(&s.first[cell], (int)i);
            atomicAdd(&s.count[cell], 1);
        }
    }
    s.cellof[i] = cell;
}

// the scanned pair of point i: (1, count of its cell) for the first point of a cell, (0, 0) otherwise
__device__ __forceinline__ void leader_pair(const VoxelWs& s, long i, long M, int& lead, int& cnt) {
    lead = 0; cnt = 0;
    if (i < M) {
        const int c = s.cellof[i];
        if (c >= 0 && s.first[c] == (int)i) { lead = 1; cnt = s.count[c]; }
    }
}

__global__ __launch_bounds__(256) void voxel_reduce_kernel(VoxelWs s, long M) {
    __shared__ int lds[8];
    const long i0 = (long)blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    int la = 0, ca = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        int l, c;
        leader_pair(s, i0 + k, M, l, c);
        la += l; ca += c;
    }
    int ea, eb, ta, tb;
    block_scan2<256>(la, ca, lds, ea, eb, ta, tb);
    if (threadIdx.x == 0) { s.part[2 * (long)blockIdx.x] = ta; s.part[2 * (long)blockIdx.x + 1] = tb; }
}

// workgroup 0: the partials -> their exclusive prefixes, in place, the totals at entry `nb`.  Workgroup 1 + a, a = 0 .. N: the leaders
// between the start of the 1024-block that holds offsets[a] and offsets[a].
__global__ __launch_bounds__(1024) void voxel_scan_kernel(const int* __restrict__ offsets, VoxelWs s, long M, long nb) {
    __shared__ int lds[32];
    int ea, eb, ta, tb;
    if (blockIdx.x == 0) {
        int ca = 0, cb = 0;
        for (long b0 = 0; b0 < nb; b0 += 1024) {
            const long b = b0 + threadIdx.x;
            const int va = b < nb ? s.part[2 * b] : 0, vb = b < nb ? s.part[2 * b + 1] : 0;
            block_scan2<1024>(va, vb, lds, ea, eb, ta, tb);
            if (b < nb) { s.part[2 * b] = ca + ea; s.part[2 * b + 1] = cb + eb; }
            ca += ta; cb += tb;
        }
        if (threadIdx.x == 0) { s.part[2 * nb] = ca; s.part[2 * nb + 1] = cb; }
        return;
    }
    const int a = blockIdx.x - 1;
    const long o = clamp_offset(offsets[a], M);
    const long j = o / kScanBlock * kScanBlock + threadIdx.x;
    int l = 0, c = 0;
    if (j < o) leader_pair(s, j, M, l, c);
    block_scan2<1024>(l, 0, lds, ea, eb, ta, tb);
    if (threadIdx.x == 0) s.agent_part[a] = ta;
}

// leaders before offsets[a], over all agents' points
__device__ __forceinline__ int leaders_before(const int* __restrict__ offsets, const VoxelWs& s, int a, long M) {
    return s.part[2 * (clamp_offset(offsets[a], M) / kScanBlock)] + s.agent_part[a];
}

template <bool HASH>
__global__ __launch_bounds__(256) void voxel_apply_kernel(const int* __restrict__ offsets, VoxelWs s, int* __restrict__ num_voxels,
                                                          VoxelArgs a) {
    __shared__ int lds[8];
    if (blockIdx.x == 0)
        for (int k = threadIdx.x; k < a.N; k += 256) {
            const int n = leaders_before(offsets, s, k + 1, a.M) - leaders_before(offsets, s, k, a.M);
            num_voxels[k] = n < 0 ? 0 : (n > a.max_voxels ? a.max_voxels : n);
        }
    const long i0 = (long)blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    int l[kScanItems], c[kScanItems], la = 0, ca = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        leader_pair(s, i0 + k, a.M, l[k], c[k]);
        la += l[k]; ca += c[k];
    }
    int ea, eb, ta, tb;
    block_scan2<256>(la, ca, lds, ea, eb, ta, tb);
    ea += s.part[2 * (long)blockIdx.x];
    eb += s.part[2 * (long)blockIdx.x + 1];
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        if (l[k]) {
            const int cell = s.cellof[i0 + k];
            const int agent = cell_agent<HASH>(s, a, cell);
            const int row = ea - leaders_before(offsets, s, agent, a.M);
            if (row >= 0 && row < a.max_voxels) {
                s.start[cell] = eb;
                s.vox_cell[(long)agent * a.max_voxels + row] = cell;
            } else {
                s.start[cell] = -1;                  // past the cap: the cell is dropped with all its points
            }
        }
        ea += l[k]; eb += c[k];
    }
}

__global__ __launch_bounds__(256) void voxel_fill_kernel(VoxelWs s, long M) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const int c = s.cellof[i];
    if (c < 0) return;
    const int st = s.start[c];
    if (st < 0) return;
    s.bucket[st + atomicAdd(&s.fill[c], 1)] = (int)i;
}

template <bool HASH>
__global__ __launch_bounds__(256) void voxel_select_kernel(const uint4* __restrict__ points, VoxelWs s, uint4* __restrict__ vf,
                                                           int4* __restrict__ coords, int* __restrict__ npts, VoxelArgs a) {
    const int t = threadIdx.x & 31;
    const long p = (long)blockIdx.x * 8 + (threadIdx.x >> 5);
    if (p >= a.Pcap) return;                         // uniform over the half-wave, as every branch and trip count below
    const int cell = s.vox_cell[p];
    if (cell < 0) {
        if (t == 0) { coords[p] = make_int4(-1, 0, 0, 0); npts[p] = 0; }
        return;
    }
    const int cnt = s.count[cell];
    const int* __restrict__ b = s.bucket + s.start[cell];
    // the 32 smallest indices seen so far, ascending over the lanes (INT_MAX where there are fewer)
    int best = kIntMax;
    for (int k0 = 0; k0 < cnt; k0 += 32) {
        int v = k0 + t < cnt ? b[k0 + t] : kIntMax;
        v = bitonic_sort32(v, t);
        // ascending `best` against the chunk reversed: the lane-wise minimum holds the 32 smallest of both as a bitonic sequence
        best = bitonic_merge32(min(best, swz_xor_i<31>(v)), t);
    }
    const int n_p = min(cnt, a.T);
    if (t < a.T) vf[p * a.T + t] = t < n_p ? points[best] : make_uint4(0, 0, 0, 0);
    if (t == 0) { coords[p] = cell_coords<HASH>(s, a, cell); npts[p] = n_p; }
}

constexpr long kMaxSlots = 1L << 31;                // a slot index is an int
constexpr long kMaxAxis = 1L << 24;                 // 3-D: every cell index is exact in fp32, so `c < (float)n` is `c < n`
constexpr long kMinSlots = 64;                      // of the default table only

// dims: [M, N, T, max_voxels, nx, ny, nz, range_mask, ego_mask] (+ [slots], 0 = the default, HASH) ; geom: [x0, y0, z0, x1, y1, z1,
// voxel x, y, z]
template <bool HASH> static int voxel_args(const long* dims, const float* geom, VoxelArgs& a) {
    if (!dims) return COBEVT_ERR_ARG;
    const long M = dims[0], N = dims[1], T = dims[2], mv = dims[3], nx = dims[4], ny = dims[5], nz = dims[6];
    if (T < 1 || T > 32 || (HASH ? nz < 1 : nz != 1)) return COBEVT_ERR_SHAPE;
    if (M < 0 || M > 0x7fffffffL - kScanBlock || N < 1 || N > 65535 || mv < 1 || nx < 1 || ny < 1) return COBEVT_ERR_SHAPE;
    if (mv > 0x7fffffffL / N) return COBEVT_ERR_SHAPE;
    if (HASH) {
        if (nx > kMaxAxis || ny > kMaxAxis || nz > kMaxAxis) return COBEVT_ERR_SHAPE;
        if (nx * ny > (1L << 62) / nz || nx * ny * nz > (1L << 62) / N) return COBEVT_ERR_SHAPE;       // the key: N nx ny nz <= 2^62
        long slots = dims[9];
        if (slots == 0) {
            slots = kMinSlots;
            while (slots < 2 * M) slots <<= 1;
            if (slots > kMaxSlots) slots = kMaxSlots;
        }
        if (slots < 1 || slots > kMaxSlots || (slots & (slots - 1)) != 0 || slots <= M) return COBEVT_ERR_SHAPE;
        a.tables = slots;
    } else {
        if (nx > 0x7fffffffL / ny || nx * ny > 0x7fffffffL / N) return COBEVT_ERR_SHAPE;
        a.tables = N * ny * nx;
    }
    a.M = M; a.N = (int)N; a.T = (int)T; a.max_voxels = (int)mv; a.nx = (int)nx; a.ny = (int)ny; a.nz = (int)nz; a.Pcap = N * mv;
    a.range_mask = dims[7] != 0; a.ego_mask = dims[8] != 0;
    if (geom)
        for (int j = 0; j < 3; ++j) { a.lo[j] = geom[j]; a.hi[j] = geom[3 + j]; a.v[j] = geom[6 + j]; }
    return COBEVT_OK;
}

template <bool HASH> static int voxel_scratch(const long* dims, long* workspace_ints) {
    VoxelArgs a;
    if (!workspace_ints) return COBEVT_ERR_ARG;
    const int rc = voxel_args<HASH>(dims, nullptr, a);
    if (rc != COBEVT_OK) return rc;
    *workspace_ints = voxel_ws_ints<HASH>(a);
    return COBEVT_OK;
}

template <bool HASH>
static int voxel_points(const float* points, const int* point_offsets, float* voxel_features, int* voxel_coords, int* voxel_num_points,
                        int* num_voxels, int* workspace, const long* dims, const float* geom, hipStream_t stream) {
    if (!dims || !geom || !point_offsets || !voxel_features || !voxel_coords || !voxel_num_points || !num_voxels || !workspace)
        return COBEVT_ERR_ARG;
    VoxelArgs a;
    const int rc = voxel_args<HASH>(dims, geom, a);
    if (rc != COBEVT_OK) return rc;
    if (a.M > 0 && !points) return COBEVT_ERR_ARG;
    if (((uintptr_t)points | (uintptr_t)voxel_features | (uintptr_t)voxel_coords) & 15) return COBEVT_ERR_SHAPE;
    if ((uintptr_t)workspace & (HASH ? 7 : 3)) return COBEVT_ERR_SHAPE;          // the 64-bit keys lead the 3-D workspace
    for (int j = 0; j < 3; ++j)
        if (!(a.v[j] > 0.f)) return COBEVT_ERR_SHAPE;
    const VoxelWs s = voxel_ws<HASH>(workspace, a);
    const long cells = a.tables, nb = scan_blocks(a.M);
    const long most = cells > a.Pcap ? cells : a.Pcap;
    long cb = (most + 255) / 256;
    if (cb > 4096) cb = 4096;                                  // grid-stride past 16 workgroups per CU
    const unsigned pb = (unsigned)((a.M + 255) / 256);         // one thread per point
    hipLaunchKernelGGL(voxel_clear_kernel<HASH>, dim3((unsigned)cb), dim3(256), 0, stream, s, cells, a.Pcap);
    if (pb)
        hipLaunchKernelGGL(voxel_classify_kernel<HASH>, dim3(pb), dim3(256), 0, stream, (const float4*)points, point_offsets, s, a);
    hipLaunchKernelGGL(voxel_reduce_kernel, dim3((unsigned)nb), dim3(256), 0, stream, s, a.M);
    hipLaunchKernelGGL(voxel_scan_kernel, dim3((unsigned)(a.N + 2)), dim3(1024), 0, stream, point_offsets, s, a.M, nb);
    hipLaunchKernelGGL(voxel_apply_kernel<HASH>, dim3((unsigned)nb), dim3(256), 0, stream, point_offsets, s, num_voxels, a);
    if (pb) hipLaunchKernelGGL(voxel_fill_kernel, dim3(pb), dim3(256), 0, stream, s, a.M);
    hipLaunchKernelGGL(voxel_select_kernel<HASH>, dim3((unsigned)((a.Pcap + 7) / 8)), dim3(256), 0, stream, (const uint4*)points, s,
                       (uint4*)voxel_features, (int4*)voxel_coords, voxel_num_points, a);
    return cobevt::launch_status();
}

}  // namespace cobevt

using namespace cobevt;

extern "C" int cobevt_voxelize_scratch(const long* dims, long* workspace_ints) { return voxel_scratch<false>(dims, workspace_ints); }

extern "C" int cobevt_voxelize_points(const float* points, const int* point_offsets, float* voxel_features, int* voxel_coords,
                                      int* voxel_num_points, int* num_voxels, int* workspace, const long* dims, const float* geom,
                                      hipStream_t stream) {
    return voxel_points<false>(points, point_offsets, voxel_features, voxel_coords, voxel_num_points, num_voxels, workspace, dims, geom,
                               stream);
}

extern "C" int cobevt_voxelize3d_scratch(const long* dims, long* workspace_ints) { return voxel_scratch<true>(dims, workspace_ints); }

extern "C" int cobevt_voxelize3d_points(const float* points, const int* point_offsets, float* voxel_features, int* voxel_coords,
                                        int* voxel_num_points, int* num_voxels, int* workspace, const long* dims, const float* geom,
                                        hipStream_t stream) {
    return voxel_points<true>(points, point_offsets, voxel_features, voxel_coords, voxel_num_points, num_voxels, workspace, dims, geom,
                              stream);
}

