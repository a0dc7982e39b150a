// Attention routing: which gathered-attention kernel a cobevt_window_attention* call launches, on which grid, decided by plain
// integer arithmetic on the launch parameters.  This header owns that decision and has no HIP dependency (standard library +
// the public header's status codes), so tests/test_attn_select.py pins it on the CPU against tests/golden/attn_select/.
//   attn_parse   dims + null-ness of the optional pointers -> AttnParams / AttnHints, or the entry point's error code
//   attn_select  AttnParams / AttnHints + CU count + the two environment gates -> AttnLaunch (kernel instantiation, grid, LDS)
// attention.hip / attention_resident.hip only map an AttnLaunch to its instantiation and launch it.
#pragma once
#include <stddef.h>
#include "../../include/cobevt_hip.h"

namespace cobevt {

struct TokMap {
    int mode;  // 0 window partition, 1 grid partition, 2 rows already stored window-partitioned
    int ncam;  // cameras / agents concatenated inside a window
    int HH, WW;
    int w1, w2;
    int X, Y;  // windows along H and W (HH == X*w1, WW == Y*w2)
};

struct AttnParams {
    const void* q; const void* k; const void* v; void* out;
    int ldq, ldk, ldv, ldo;
    int qoff, koff, voff, ooff;
    TokMap qmap, kmap, omap;
    int B, L, heads, Nq, Nk;
    float scale;
    int bias_mode;            // 0 none, 1 relative-position table lookup
    const float* bias_table;  // [rows][heads]
    int bias_rows;
    int bias_L;               // agent extent of the 3-D table (1 => 2-D table)
    const float* mask;        // key mask fp32, 0 => key masked out; (B,HH,WW,ncam), or (B,L,w1,w2,ncam) for mode 2; may be null
    int mean_q;               // 0: every query token on its own; 1: per-camera query copies, outputs averaged over the cameras
                              // (fax_modules.py:243); 2: per-camera query copies, camera c's query scores camera c's keys only,
                              // ONE softmax over all cameras' keys (CVT CrossAttention, cvt_modules.py:142-153)
    float* lse;               // training forward: base-2 log-sum-exp of every query's logits, [B][L][heads][Nq] (nullable)
    int klinear;              // streaming kernel: key token tk of the (single) window is row b * Nk + tk - no key table in LDS
    // training only: nn.Dropout on the attention probabilities (FAX global attention, fax_modules.py:114,161): element (query,
    // key) of a (batch, window, head) is kept with probability 1 - drop_p and scaled by 1 / (1 - drop_p); the keep decision is a
    // counter-based hash of (drop_seed, element index), so the backward kernels regenerate the forward's mask
    float drop_p;
    unsigned drop_seed;
    // nullable device word ADDED to drop_seed: a captured training step (tools/train_graph_probe.py) bumps it inside the graph, so every
    // replay draws a new mask although the kernel arguments are frozen in the graph's nodes
    const unsigned* drop_seed_dev;
    // key split (streaming kernel, inference): the keys of a window are shared out over `ksplit` workgroups per query tile; each
    // writes its normalised partial output rows to part_out[split] (same row indexing as `out`, row stride heads * 32) and the
    // base-2 log-sum-exp of its keys to part_lse[split][row][head]; attn_ksplit_merge_kernel combines them into `out`.
    // For the launches whose grid leaves the chip idle AND whose per-query key walk is long (level-2 / global FAX attention:
    // 1024 keys, 160 workgroups) - the tile loop is one dependent round trip per iteration.
    int ksplit;
    void* part_out;
    float* part_lse;
    long part_rows;           // rows of `out` (stride between the splits' partial buffers)
};

static inline bool map_ok(const TokMap& m) {
    if (m.mode < 0 || m.mode > 2 || m.ncam < 1 || m.w1 < 1 || m.w2 < 1 || m.X < 1 || m.Y < 1) return false;
    if (m.mode != 2 && (m.HH != m.X * m.w1 || m.WW != m.Y * m.w2)) return false;
    return m.w1 < 256 && m.w2 < 256 && m.ncam < 32768;
}

static inline TokMap read_map(const int* d) {
    TokMap m;
    m.mode = d[0]; m.ncam = d[1]; m.HH = d[2]; m.WW = d[3]; m.w1 = d[4]; m.w2 = d[5]; m.X = d[6]; m.Y = d[7];
    return m;
}

// What a call says beyond the kernels' parameter block.  dims[0] = dtype | variant << 8 | query split << 16:
//   dtype    0 bf16, 1 fp32 storage
//   variant  0 = automatic (K/V-resident kernel where it applies), 1 = force the streaming kernel (A/B runs, parity tests of both
//            paths), 2 = ... with 64-key tiles only
//   qsplit   query split of the resident kernel, 0 = automatic
struct AttnHints {
    int dtype, variant, qsplit;
    bool has_mask, has_lse;
};

// The two A/B switches of the resident kernel, read from the environment once per process by the entry point; both default ON:
//   COBEVT_ATTN_BIG=0      keeps plain windows of 513 .. 1024 keys on the streaming kernel
//   COBEVT_ATTN_PERSIST=0  keeps one (window, head) item per workgroup on every shape
struct AttnGates { bool big_resident, persist; };

enum AttnFamily { ATTN_RESIDENT, ATTN_RESIDENT_BIG, ATTN_STREAM, ATTN_STREAM_DROP };

// One kernel launch (+ the key-split merge launch).  Template tuple: attn_resident_kernel<NT, NW, MEAN, BIAS, MASK, RAGGED, W8,
// PERSIST> (RESIDENT; RESIDENT_BIG = the plain four-wave form of 513 .. 1024 keys: NT 10 .. 16, RAGGED only), or
// attn_gather_kernel<dtype, BIAS, MASK, KT> (STREAM; STREAM_DROP = its fp32 dropout form).  Fields of the other family stay 0.
struct AttnLaunch {
    int status;               // COBEVT_OK, or the entry point's error code (nothing is launched)
    AttnFamily family;
    int NT, NW;
    bool MEAN, BIAS, MASK, RAGGED, W8, PERSIST;
    int dtype, KT;
    unsigned grid[3];
    int block;
    size_t lds;
    int qsplit;               // resident kernels' second argument
    unsigned merge_grid;      // attn_ksplit_merge_kernel<dtype> workgroups of 256 threads, 0 = no merge launch
};

// AttnLds<T, KT>::kFixed of the streaming kernel's three tile shapes (attention.hip pins each with a static_assert)
constexpr size_t kAttnStreamLdsBf16Kt64 = 19456, kAttnStreamLdsBf16Kt128 = 38400, kAttnStreamLdsF32Kt64 = 36352;

// Everything a cobevt_window_attention* call checks before it chooses a kernel.  Fills every non-pointer field of `p` (pointers:
// null; the caller stores them afterwards, part_out / part_lse only when p.ksplit > 1).  part_rows: `out_rows` of the key-split call.
inline int attn_parse(const int* dims, bool has_bias_table, bool has_mask, bool has_lse, float drop_p, int ksplit, bool has_parts,
                      long part_rows, AttnParams& p, AttnHints& h) {
    // dims: [dtype | variant << 8 | qsplit << 16, B, L, heads, ldq, ldk, ldv, ldo, qoff, koff, voff, ooff, bias_mode, bias_rows, bias_L,
    //        mean_q, qmap[8], kmap[8], omap[8]]
    p = AttnParams{};
    h.dtype = dims[0] & 0xff; h.variant = (dims[0] >> 8) & 0xff; h.qsplit = (dims[0] >> 16) & 0xff;
    h.has_mask = has_mask; h.has_lse = has_lse;
    p.B = dims[1]; p.L = dims[2]; p.heads = dims[3];
    p.ldq = dims[4]; p.ldk = dims[5]; p.ldv = dims[6]; p.ldo = dims[7];
    p.qoff = dims[8]; p.koff = dims[9]; p.voff = dims[10]; p.ooff = dims[11];
    p.bias_mode = dims[12]; p.bias_rows = dims[13]; p.bias_L = dims[14];
    p.mean_q = dims[15];
    p.qmap = read_map(dims + 16); p.kmap = read_map(dims + 24); p.omap = read_map(dims + 32);
    p.drop_p = drop_p;
    p.ksplit = 1;
    if (drop_p < 0.f || drop_p >= 1.f || (drop_p > 0.f && (!has_lse || h.dtype != 1))) return COBEVT_ERR_ARG;   // dropout: training forward only
    if (h.dtype != 0 && h.dtype != 1) return COBEVT_ERR_ARG;
    if (!map_ok(p.qmap) || !map_ok(p.kmap) || !map_ok(p.omap)) return COBEVT_ERR_SHAPE;
    if (p.B < 1 || p.heads < 1 || p.L != p.qmap.X * p.qmap.Y || p.L != p.kmap.X * p.kmap.Y) return COBEVT_ERR_SHAPE;
    if (p.bias_mode && (!has_bias_table || p.bias_rows < 1 || p.bias_L < 1)) return COBEVT_ERR_ARG;
    const int ch = h.dtype == 0 ? 8 : 4;
    if ((p.ldq | p.ldk | p.ldv | p.ldo | p.qoff | p.koff | p.voff | p.ooff) % ch) return COBEVT_ERR_SHAPE;
    p.Nq = p.qmap.ncam * p.qmap.w1 * p.qmap.w2;
    p.Nk = p.kmap.ncam * p.kmap.w1 * p.kmap.w2;
    if (p.mean_q < 0 || p.mean_q > 2) return COBEVT_ERR_ARG;
    if (p.mean_q && p.qmap.ncam == 1) p.mean_q = 0;
    if (p.mean_q == 1 && (p.qmap.ncam > 8 || p.omap.ncam != 1)) return COBEVT_ERR_UNSUPPORTED;
    if (p.mean_q == 2) {     // camera-paired queries: cameras on both sides, whole tiles per camera, no bias / mask
        if (p.omap.ncam != 1 || p.qmap.ncam != p.kmap.ncam || p.bias_mode || has_mask) return COBEVT_ERR_UNSUPPORTED;
    }
    // keys of a single window that covers the whole map are rows b * Nk + tk: no table (CVT attends to 4 x 64 x 64 keys)
    p.klinear = (p.kmap.mode != 2 && p.kmap.X == 1 && p.kmap.Y == 1 && !p.bias_mode && !has_mask) ? 1 : 0;
    if (has_lse && p.mean_q) return COBEVT_ERR_UNSUPPORTED;     // (the training path averages cameras outside the kernel)
    // key split: streaming kernel only, plain inference attention - every query of a window on its own, or camera-paired (mean_q = 2:
    // partial rows and the merge follow the output map, one row per BEV position; a split may start or end inside a camera, the key
    // loop reloads the query copy whenever a tile's camera differs from the one it holds)
    if (ksplit > 1) {
        if (ksplit > 16 || !has_parts || part_rows < 1 || has_lse || p.mean_q == 1 || drop_p > 0.f) return COBEVT_ERR_ARG;
        if (p.mean_q != 2 && p.omap.ncam != p.qmap.ncam) return COBEVT_ERR_UNSUPPORTED;
        p.ksplit = ksplit; p.part_rows = part_rows;
    }
    return COBEVT_OK;
}

// The K/V-resident kernel (attention_resident.hip) for this problem, or false when it does not apply.
inline bool attn_select_resident(const AttnParams& p, const AttnHints& h, int cus, AttnGates gates, AttnLaunch& a) {
    if (h.dtype != 0 || h.variant != 0 || p.mean_q == 2 || h.has_lse || p.ksplit != 1) return false;
    const bool hb = p.bias_mode != 0, hm = h.has_mask, mean = p.mean_q != 0, info = hb || hm;
    // <= 64 keys: one streaming tile is already optimal; > 512: LDS - except the plain variant (no bias / mask / camera mean), whose K / V
    // of up to 1024 keys (the FAX level-2 and global attentions: one whole-map window per agent) fit as 128 KB + tables: four-wave
    // workgroups, one per CU, one 32-query tile per wave instead of the streaming kernel's key split + merge launch
    const bool big = p.Nk > 512;
    if (p.Nk < 65 || p.Nk > 1024 || (big && (info || mean || !gates.big_resident))) return false;
    if (mean && info) return false;                    // the camera mean only occurs in the plain cross attention
    const int nt = ((p.Nk + 127) / 128) * 2;           // 64-key tiles, even
    const int P = p.qmap.w1 * p.qmap.w2;
    if (p.omap.ncam != (mean ? 1 : p.qmap.ncam)) return false;
    const int NQ = mean ? P : p.Nq;
    size_t lds = (size_t)nt * 64 * 128 + (size_t)nt * 64 * 4 * (1 + (info ? 2 : 0) + (hb ? 1 : 0)) + (size_t)NQ * 4 * (hb ? 3 : 2);
    if (hb) {
        // four shifted copies of the reversed, row-padded table column (see the kernel): key quads must share (agent, window row)
        if (p.kmap.w2 % 4 != 0 || p.bias_rows != (2 * p.bias_L - 1) * (2 * p.kmap.w1 - 1) * (2 * p.kmap.w2 - 1)) return false;
        const size_t rp = (size_t)(2 * p.bias_L - 1) * (2 * p.kmap.w1 - 1) * (2 * p.kmap.w2);
        lds = ((lds + 15) & ~(size_t)15) + 4 * (rp + 4) * 4;
    }
    lds = (lds + 15) & ~(size_t)15;
    if (lds > 160 * 1024) return false;
    if ((long)p.B * p.qmap.ncam * (p.qmap.mode == 2 ? (long)p.L * P : (long)p.qmap.HH * p.qmap.WW) >= 0x7fffffffL) return false;
    const int ntiles = (NQ + 31) / 32;
    // waves per workgroup: 8 when the LDS footprint leaves room for one or two workgroups per CU only and the window has the
    // query tiles to feed them (LiDAR FuseBEVT: 512 tokens per window)
    // (16 waves = 4 per SIMD at one workgroup per CU was measured 2x slower for the 512-key bias + mask windows: 128 VGPRs spill)
    const int nw = big ? 4 : (lds > 40 * 1024 && ntiles >= 16) ? 8 : 4;
    // query split: enough workgroups to fill 256 CUs x (4 | 2 | 1 resident workgroups), every wave keeping >= 1 tile
    const long base = (long)p.B * p.L * p.heads;
    int qsplit = h.qsplit;
    if (qsplit <= 0 && big) {                           // one query tile per wave where the window has them
        qsplit = 1;
        while (qsplit * 2 * nw <= ntiles) qsplit *= 2;
    } else if (qsplit <= 0) {
        const int resident = lds > 80 * 1024 ? 1 : (lds > 40 * 1024 ? 2 : 4);
        qsplit = 1;
        while (base * qsplit < 256L * resident && ntiles >= 2 * qsplit * nw) qsplit *= 2;
        if (base * qsplit < 256L && ntiles >= 2 * qsplit * nw - nw) qsplit *= 2;     // fewer workgroups than CUs: one tile per wave
        // bias / mask windows on a grid that still does not reach the CU count (the 5-agent fusion: 64 (window, head) pairs of 10 query
        // tiles): keep splitting while a workgroup keeps two tiles - 13.2 us against the streaming kernel's 14.9 us in-graph
        if (info) while (base * qsplit < 256L && ntiles >= 4 * qsplit) qsplit *= 2;
    }
    if (qsplit > ntiles) qsplit = ntiles;
    if (qsplit < 1) qsplit = 1;
    // fewer workgroups than CUs (nuScenes: 100 windows x 1 head; the 5-agent fusion: 16 windows x 4 heads): the streaming kernel's
    // finer query split fills the chip better than one staging per (window, head) can (measured: 31 vs 52 us, 25 vs 29 us)
    if (h.qsplit <= 0 && !big && base * qsplit < 256) return false;
    unsigned gx = (unsigned)(p.L * p.heads * qsplit);
    if ((unsigned)p.B > 65535) return false;
    // one workgroup per CU (> 80 KB of LDS) and several items per CU: persistent workgroups, a whole number of (8 windows x heads)
    // groups of them so that a workgroup keeps its head (and its bias copies) across its items
    bool persist = false;
    if (gates.persist && nw == 8 && lds > 80 * 1024 && !mean) {
        const int per = 8 * p.heads;
        const int pgx = cus >= per && (p.L & 7) == 0 ? (cus / per) * per : cus;
        if ((long)pgx * 2 <= (long)gx) {                // at least two items per workgroup, else the plain form
            gx = (unsigned)pgx;
            persist = true;
        }
    }
    const bool padded = p.Nk != nt * 64;
    a.family = big ? ATTN_RESIDENT_BIG : ATTN_RESIDENT;
    a.NT = nt; a.NW = nw;
    a.W8 = hb && !padded && p.kmap.w1 == 8 && p.kmap.w2 == 8;
    a.MEAN = mean; a.BIAS = hb; a.MASK = hm; a.RAGGED = padded && !info; a.PERSIST = persist;
    a.grid[0] = gx; a.grid[1] = (unsigned)p.B; a.grid[2] = 1;
    a.block = nw * 64; a.lds = lds; a.qsplit = qsplit;
    return true;
}

// The whole decision for a parsed call: cus = compute units of the device (256 when the query fails).
inline AttnLaunch attn_select(const AttnParams& p, const AttnHints& h, int cus, AttnGates gates) {
    AttnLaunch a = {};
    a.status = COBEVT_OK;
    if (attn_select_resident(p, h, cus, gates, a)) return a;
    auto fail = [&a](int code) { a.status = code; return a; };
    const int P = p.qmap.w1 * p.qmap.w2;
    if (p.mean_q == 1) { a.block = 64 * (p.qmap.ncam < 4 ? 4 : p.qmap.ncam); a.grid[1] = (unsigned)((P + 31) / 32); }
    else { a.block = 256; a.grid[1] = (unsigned)(((p.mean_q == 2 ? P : p.Nq) + 127) / 128 * p.ksplit); }
    a.grid[0] = (unsigned)(p.L * p.heads); a.grid[2] = (unsigned)p.B;
    if (a.grid[1] > 65535 || a.grid[2] > 65535) return fail(COBEVT_ERR_SHAPE);
    // 128-key tiles: bf16, enough keys, not the camera-paired mode (its tiles never mix cameras)
    // ... and a grid that does not fill the chip anyway (there the iteration count sets the time; on a full grid the wider tile's
    // registers cost occupancy: 512-token LiDAR windows, bias + mask, 8192 workgroups: 357 us against 266 us with 64-key tiles)
    const bool wide = h.dtype == 0 && p.mean_q != 2 && p.Nk >= 256 && h.variant != 2 &&      // variant 2: 64-key tiles (A/B)
                      (long)a.grid[0] * a.grid[1] * a.grid[2] <= 1024;
    // >= 1 key tile per split (camera-paired: 64-key tiles that never mix cameras, as the kernel counts them)
    const int key_tiles = p.mean_q == 2 ? p.kmap.ncam * ((p.kmap.w1 * p.kmap.w2 + 63) / 64) : (p.Nk + (wide ? 127 : 63)) / (wide ? 128 : 64);
    if (p.ksplit > 1 && key_tiles < p.ksplit) return fail(COBEVT_ERR_SHAPE);
    size_t lds = h.dtype == 0 ? (wide ? kAttnStreamLdsBf16Kt128 : kAttnStreamLdsBf16Kt64) : kAttnStreamLdsF32Kt64;
    if (p.bias_mode) lds += ((size_t)p.bias_rows * 4 + 15) & ~(size_t)15;
    if (!p.klinear) lds += (size_t)p.Nk * 8;        // per-key row / coordinate table
    if ((long)p.B * p.kmap.ncam * (p.kmap.mode == 2 ? (long)p.L * p.kmap.w1 * p.kmap.w2 : (long)p.kmap.HH * p.kmap.WW) >= 0x7fffffffL)
        return fail(COBEVT_ERR_UNSUPPORTED);        // the table holds 32-bit row indices
    if (p.mean_q == 1) { const size_t need = (size_t)p.qmap.ncam * 16 * 64 * 4; if (need > lds) lds = need; }
    if (lds > 64 * 1024) return fail(COBEVT_ERR_UNSUPPORTED);
    a.family = p.drop_p > 0.f ? ATTN_STREAM_DROP : ATTN_STREAM;     // dropout: fp32 training forward, checked by attn_parse
    a.dtype = h.dtype; a.KT = wide ? 128 : 64;
    a.BIAS = p.bias_mode != 0; a.MASK = h.has_mask;
    a.lds = lds;
    if (p.ksplit > 1) a.merge_grid = (unsigned)((p.part_rows * p.heads * 4 + 255) / 256);
    return a;
}

}  // namespace cobevt
