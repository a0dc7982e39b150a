// nuScenes camera ingest (gfx950): what LoadDataTransform (nuscenes/cross_view_transformer/data/transforms.py:118-177) does to a sample
// before the model sees it, on decoded uint8 frames in device memory.
//   resize_pil_kernel : Image.resize(.., resample=BILINEAR) of Pillow's 8-bit path + the top crop + ToTensor's byte -> fp32 table.
//                       Pillow resamples in two passes of 22-bit fixed point, horizontal first, and rounds the horizontal result to a BYTE
//                       before the vertical pass reads it; an axis that keeps its size is skipped.  The tap tables (first source index,
//                       tap count, integer coefficients per output index) are made on the host from Pillow's own float64 statements
//                       (ops.pil_resize_taps) and passed in, so the kernel is integer arithmetic and one table lookup: bit-exact.
//                       One workgroup = one image, a band of `band` output rows and a tile of at most kIngestTile output columns.
//                       The source rows the band needs come in chunks of kIngestChunk rows: 16-byte loads of the tile's byte span (a
//                       row of W * 3 bytes starts on no particular boundary: the up to 15 bytes before the first and after the last
//                       aligned 16 are loaded one by one) into one of two LDS buffers - the loads of chunk i + 1 are in flight in
//                       registers while the horizontal pass (an output pixel of a source row per item, its tap bytes read as aligned
//                       dwords) turns chunk i into the band's uint8 rows in LDS - then the vertical pass
//                       (a row at a time, so its taps are wave-uniform scalar loads), the table and the stores.  Rows the crop drops
//                       are never computed.
//   decode_bev_kernel : common.py:69-78 decode -> * 255 -> uint8 -> ToTensor of the bit-packed BEV label: (x >> c) & 1 as 0.0 / 1.0.
#include "common.hpp"

namespace cobevt {

constexpr int kIngestRows = 8;          // output rows per workgroup (halved by the launcher until the LDS fits)
constexpr int kIngestTile = 128;        // output columns per workgroup, at most
constexpr int kIngestChunk = 8;         // source rows staged per round (G below; 4 where two buffers of 8 rows do not fit the LDS):
                                        // half the barriers of 4 rows and twice the bytes in flight per workgroup
constexpr int kIngestEdge = 30;         // single-byte items per source row: up to 15 before and 15 after the aligned pieces
constexpr int kIngestSlack = 32;        // bytes of a staged source row beyond its span: the 16-byte phase, and the reads of zero-weighted taps
constexpr int kIngestMaxTaps = 17;      // a down-scale of 8: 2 * ceil(8) + 1
constexpr int kIngestBits = 22;         // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int kIngestMaxClasses = 16;

struct IngestArgs {
    int H, W;                           // source
    int hr, wr, top;                    // resized size, rows cut from its top
    int band, tw;                       // output rows / columns per workgroup
    int rows_cap, raw_stride;           // band rows / bytes per staged source row the LDS holds
    int ksx, ksy;                       // row length of the coefficient tables
    int out_u8;
};

// taps per output index of one axis as Pillow sizes them: 2 * ceil(max(n_in / n_out, 1)) + 1
inline int ingest_ksize(int n_in, int n_out) {
    const double scale = (double)n_in / (double)n_out;
    const double support = 1.0 * (scale < 1.0 ? 1.0 : scale);
    return 2 * (int)ceil(support) + 1;
}

// source indices a run of `count` consecutive outputs can touch: its taps lie within support of centres (count - 1) * scale apart
inline int ingest_span(int n_in, int n_out, int count) {
    const double scale = (double)n_in / (double)n_out;
    const double support = scale < 1.0 ? 1.0 : scale;
    const double span = floor((count - 1) * scale + 2.0 * support) + 2.0;
    return span < (double)n_in ? (int)span : n_in;
}

// coefficient row length in the LDS: a multiple of four, read 16 bytes at a time
__host__ __device__ inline int ingest_kpad(int ks) { return (ks + 3) & ~3; }

// bytes of LDS: the byte table, the tile's horizontal tables, two chunk buffers, the band's rows
inline size_t ingest_lds(const IngestArgs& a, int chunk) {
    const size_t tables = ((size_t)a.tw * (2 + ingest_kpad(a.ksx)) * 4 + 15) & ~(size_t)15;
    return 1024 + tables + 2 * (size_t)chunk * a.raw_stride + (size_t)a.rows_cap * a.tw * 3;
}

__device__ inline int ingest_clip8(int acc) {
    const int v = (acc + (1 << (kIngestBits - 1))) >> kIngestBits;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// bytes sh .. sh + 3 of the eight bytes lo, hi (little endian): an unaligned dword from two aligned ones
__device__ inline unsigned ingest_shift(unsigned hi, unsigned lo, int sh) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, (unsigned)sh);
#else
    return (unsigned)((((unsigned long long)hi << 32) | lo) >> (8 * sh));
#endif
}

// byte * coefficient: the coefficients are 22-bit fixed point (at most 2^22), so the full-rate 24-bit multiply is exact; the 32-bit
// one runs at a quarter of its rate, and the kernel is bound by the instructions it issues
__device__ inline int ingest_mul(unsigned byte, int k) { return __mul24((int)byte, k); }

// staging item k of a source row of nb bytes at gp: k < nvmax a 16-byte piece, then 15 single bytes in front of the first aligned piece
// and 15 behind the last.  -> its byte offset in the row, whether it is a 16-byte piece; false when the row has no such item
__device__ inline bool ingest_item(const unsigned char* gp, int nb, int nvmax, int k, int& off, bool& vec) {
    const int mis = (int)((uintptr_t)gp & 15);
    const int head = min(nb, (16 - mis) & 15), nvec = (nb - head) >> 4;
    vec = k < nvmax;
    if (vec) { off = head + 16 * k; return k < nvec; }
    const int b = k - nvmax;
    if (b < 15) { off = b; return b < head; }
    off = head + 16 * nvec + (b - 15);
    return off < nb;
}

// sum_t p[t * stride] * kk[t] over cnt >= 1 taps, four loads in flight
template <typename K>
__device__ inline int ingest_taps(const unsigned char* p, int stride, const K* kk, int cnt) {
    int acc = 0;
    for (int t = 0; t < cnt; t += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int tt = min(t + u, cnt - 1);
            const int k = t + u < cnt ? kk[tt] : 0;
            acc += ingest_mul(p[tt * stride], k);
        }
    }
    return acc;
}

// G source rows per round; a thread holds G staging items (16 bytes or 1 byte each) in registers per round
template <int G>
__global__ __launch_bounds__(256) void resize_pil_kernel(const unsigned char* __restrict__ src, void* __restrict__ out,
                                                         const int* __restrict__ hb, const int* __restrict__ hc,
                                                         const int* __restrict__ vb, const int* __restrict__ vc,
                                                         const float* __restrict__ lut, IngestArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int ksp = ingest_kpad(a.ksx);
    float* slut = (float*)smem;                                              // 256 floats
    int* shc = (int*)(smem + 1024);                                          // the tile's coefficient rows, zero from the tap count to ksp
    int* shb = shc + ksp * a.tw;                                             // ... and [byte offset of the first tap in the staged row, tap count]
    unsigned char* raw = smem + 1024 + (((size_t)a.tw * (2 + ksp) * 4 + 15) & ~(size_t)15);   // 2 x G source rows, each at its own 16-byte phase
    unsigned char* stg = raw + 2 * G * a.raw_stride;              // rows_cap rows of the horizontally resampled tile, uint8
    const int tid = threadIdx.x, n = blockIdx.z;
    const int x0 = blockIdx.x * a.tw, tw = min(a.tw, a.wr - x0), tw3 = tw * 3, stg_stride = a.tw * 3;
    const int oy0 = a.top + blockIdx.y * a.band, nr = min(a.band, a.hr - oy0);
    if (!a.out_u8) slut[tid] = lut[tid];

    // the source window of this band and tile.  The tables are the caller's: every index taken from them is clamped to the window, so
    // that a wrong table gives wrong pixels and no access outside the image or the LDS.
    int y0 = oy0, y1 = oy0 + nr, sx0 = x0, sx1 = x0 + tw;
    if (vb) { y0 = vb[2 * oy0]; y1 = vb[2 * (oy0 + nr - 1)] + vb[2 * (oy0 + nr - 1) + 1]; }
    if (hb) { sx0 = hb[2 * x0]; sx1 = hb[2 * (x0 + tw - 1)] + hb[2 * (x0 + tw - 1) + 1]; }
    y1 = max(1, min(y1, a.H)); y0 = max(0, min(y0, y1 - 1));
    sx1 = max(1, min(sx1, a.W)); sx0 = max(0, min(sx0, sx1 - 1));
    sx1 = min(sx1, sx0 + (a.raw_stride - kIngestSlack) / 3);
    const int nrows = min(y1 - y0, a.rows_cap);
    const int nb = (sx1 - sx0) * 3;                                          // bytes of a source row this tile reads
    const int nvmax = nb >> 4, ipr = nvmax + kIngestEdge;                    // items per row; the launcher keeps ipr <= 256, so G slots a thread hold a chunk
    const unsigned char* base = src + (((size_t)n * a.H + y0) * a.W + sx0) * 3;
    const size_t row_bytes = (size_t)a.W * 3;
    if (hb) {
        // per output column: where its first tap lies in a staged row and how many taps, clamped to the window; coefficients past the
        // count are ZERO up to a multiple of four, so the pass below reads four taps at a time without a test (what lies behind a
        // row's last byte in the LDS is multiplied by zero; kIngestSlack keeps those reads inside the buffer)
        for (int i = tid; i < tw * ksp; i += 256) {
            const int x = i / ksp, t = i - x * ksp;
            const int xmin = min(max(hb[2 * (x0 + x)], sx0), sx1 - 1);
            const int cnt = max(0, min(min(hb[2 * (x0 + x) + 1], a.ksx), sx1 - xmin));
            shc[i] = t < cnt ? hc[(size_t)(x0 + x) * a.ksx + t] : 0;
            if (t == 0) { shb[2 * x] = (xmin - sx0) * 3; shb[2 * x + 1] = cnt; }
        }
    }

    uint4 slot[G];
    int sg[G], sk[G];                                  // the row within a chunk and the item within the row of each slot
#pragma unroll
    for (int u = 0; u < G; ++u) { sg[u] = (tid + u * 256) / ipr; sk[u] = tid + u * 256 - sg[u] * ipr; }
    auto fetch = [&](int c0) __attribute__((always_inline)) {                // chunk c0's bytes -> registers
        const int ng = min(G, nrows - c0);
#pragma unroll
        for (int u = 0; u < G; ++u) {
            if (sg[u] < ng) {
                const unsigned char* gp = base + (size_t)(c0 + sg[u]) * row_bytes;
                int off; bool vec;
                if (ingest_item(gp, nb, nvmax, sk[u], off, vec)) {
                    if (vec) slot[u] = *(const uint4*)(gp + off);
                    else slot[u] = make_uint4(gp[off], 0, 0, 0);
                }
            }
        }
    };
    auto commit = [&](int c0, unsigned char* buf) __attribute__((always_inline)) {      // registers -> the chunk buffer, each row at its global phase
        const int ng = min(G, nrows - c0);
#pragma unroll
        for (int u = 0; u < G; ++u) {
            if (sg[u] < ng) {
                const unsigned char* gp = base + (size_t)(c0 + sg[u]) * row_bytes;
                int off; bool vec;
                if (ingest_item(gp, nb, nvmax, sk[u], off, vec)) {
                    unsigned char* lp = buf + sg[u] * a.raw_stride + (int)((uintptr_t)gp & 15) + off;
                    if (vec) *(uint4*)lp = slot[u];
                    else *lp = (unsigned char)slot[u].x;
                }
            }
        }
    };

    fetch(0);
    commit(0, raw);
    __syncthreads();
    for (int c0 = 0, cur = 0; c0 < nrows; c0 += G, cur ^= 1) {
        const int ng = min(G, nrows - c0);
        const bool more = c0 + G < nrows;
        if (more) fetch(c0 + G);
        const unsigned char* buf = raw + cur * G * a.raw_stride;
        // where row g of the chunk starts in its buffer: at the 16-byte phase of its global address (the low bits suffice)
        const unsigned base_lo = (unsigned)(uintptr_t)base, row_lo = (unsigned)row_bytes;
        if (hb) {
            // one item = one output pixel of one source row: its taps are 3 * cnt consecutive bytes, read as ALIGNED dwords (four taps =
            // 12 bytes = three dwords once shifted to the pixel's byte phase) - a third of the LDS reads of a byte at a time, which at
            // one to three waves per SIMD is what the pass waits for
            for (int i = tid; i < ng * tw; i += 256) {
                const int g = i / tw, x = i - g * tw;
                const int cnt = shb[2 * x + 1];
                const int* kk = shc + x * ksp;
                const int start = g * a.raw_stride + (int)((base_lo + (unsigned)(c0 + g) * row_lo) & 15) + shb[2 * x];
                const unsigned* wp = (const unsigned*)(buf + (start & ~3));
                const int sh = start & 3;
                int acc0 = 0, acc1 = 0, acc2 = 0;
                for (int t = 0; t < cnt; t += 4, wp += 3) {
                    const int4 k = *(const int4*)(kk + t);
                    const unsigned w0 = wp[0], w1 = wp[1], w2 = wp[2], w3 = wp[3];
                    const unsigned d0 = ingest_shift(w1, w0, sh), d1 = ingest_shift(w2, w1, sh), d2 = ingest_shift(w3, w2, sh);
                    acc0 += ingest_mul((d0 & 255), k.x) + ingest_mul((d0 >> 24), k.y) + ingest_mul(((d1 >> 16) & 255), k.z) + ingest_mul(((d2 >> 8) & 255), k.w);
                    acc1 += ingest_mul(((d0 >> 8) & 255), k.x) + ingest_mul((d1 & 255), k.y) + ingest_mul((d1 >> 24), k.z) + ingest_mul(((d2 >> 16) & 255), k.w);
                    acc2 += ingest_mul(((d0 >> 16) & 255), k.x) + ingest_mul(((d1 >> 8) & 255), k.y) + ingest_mul((d2 & 255), k.z) + ingest_mul((d2 >> 24), k.w);
                }
                unsigned char* sp = stg + (c0 + g) * stg_stride + 3 * x;
                sp[0] = (unsigned char)ingest_clip8(acc0);                   // rounded to a byte HERE, as Pillow does
                sp[1] = (unsigned char)ingest_clip8(acc1);
                sp[2] = (unsigned char)ingest_clip8(acc2);
            }
        } else {
            for (int i = tid; i < ng * tw3; i += 256) {
                const int g = i / tw3, j = i - g * tw3;
                stg[(c0 + g) * stg_stride + j] = buf[g * a.raw_stride + (int)((base_lo + (unsigned)(c0 + g) * row_lo) & 15) + j];
            }
        }
        if (more) commit(c0 + G, raw + (cur ^ 1) * G * a.raw_stride);
        __syncthreads();
    }

    const int ho = a.hr - a.top;
    for (int r = 0; r < nr; ++r) {                                           // a row at a time: its taps are the same for every lane
        const int oy = oy0 + r;
        int ymin = min(r, nrows - 1), cnt = 1;
        const int* kk = nullptr;
        if (vb) {
            ymin = min(max(vb[2 * oy] - y0, 0), nrows - 1);
            cnt = min(min(vb[2 * oy + 1], a.ksy), nrows - ymin);
            kk = vc + (size_t)oy * a.ksy;
        }
        for (int j = tid; j < tw3; j += 256) {
            int x, c;
            if (a.out_u8) { x = j / 3; c = j - 3 * x; }                      // bytes of a pixel are neighbours in the output
            else { c = (j >= tw) + (j >= 2 * tw); x = j - c * tw; }          // planes: x runs along the lanes
            const unsigned char* sp = stg + ymin * stg_stride + x * 3 + c;
            const int v = vb ? ingest_clip8(ingest_taps(sp, stg_stride, kk, cnt)) : (int)sp[0];
            if (a.out_u8) ((unsigned char*)out)[(((size_t)n * ho + (oy - a.top)) * a.wr + x0 + x) * 3 + c] = (unsigned char)v;
            else ((float*)out)[(((size_t)n * 3 + c) * ho + (oy - a.top)) * a.wr + x0 + x] = slut[v];
        }
    }
}

__global__ __launch_bounds__(256) void decode_bev_kernel(const int* __restrict__ labels, float* __restrict__ out, int hw, int C) {
    const int n = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= hw) return;
    const int v = labels[(size_t)n * hw + pix];
    for (int c = 0; c < C; ++c) out[((size_t)n * C + c) * hw + pix] = (float)((v >> c) & 1);
}

// dims = [n, H, W, channels, h_resize, w_resize, top_crop, out is uint8]
static int launch_resize_pil(const unsigned char* src, void* out, const int* hb, const int* hc, const int* vb, const int* vc,
                             const float* lut, const int* dims, hipStream_t stream) {
    if (!src || !out || !dims) return COBEVT_ERR_ARG;
    const int n = dims[0], H = dims[1], W = dims[2], C = dims[3], hr = dims[4], wr = dims[5], top = dims[6], out_u8 = dims[7];
    if (C != 3 || n < 1 || n > 65535 || H < 1 || W < 1 || hr < 1 || wr < 1 || top < 0 || top >= hr) return COBEVT_ERR_SHAPE;
    const int ksx = ingest_ksize(W, wr), ksy = ingest_ksize(H, hr);
    if (ksx > kIngestMaxTaps || ksy > kIngestMaxTaps) return COBEVT_ERR_SHAPE;
    const bool hpass = W != wr, vpass = H != hr;
    if ((hpass && (!hb || !hc)) || (vpass && (!vb || !vc)) || (!out_u8 && !lut)) return COBEVT_ERR_ARG;
    if ((((uintptr_t)hb | (uintptr_t)hc | (uintptr_t)vb | (uintptr_t)vc | (uintptr_t)lut) & 3) || (!out_u8 && ((uintptr_t)out & 3)))
        return COBEVT_ERR_SHAPE;
    IngestArgs a;
    a.H = H; a.W = W; a.hr = hr; a.wr = wr; a.top = top; a.ksx = ksx; a.ksy = ksy; a.out_u8 = out_u8 ? 1 : 0;
    const int ntx = (wr + kIngestTile - 1) / kIngestTile;
    a.tw = (wr + ntx - 1) / ntx;
    const int span = hpass ? ingest_span(W, wr, a.tw) : a.tw;
    a.raw_stride = ((span * 3 + 15) & ~15) + kIngestSlack;
    if (a.raw_stride / 16 + kIngestEdge > 256) return COBEVT_ERR_UNSUPPORTED;       // items per row <= 256, one per thread (never with a scale <= 8)
    int chunk = kIngestChunk;
    for (a.band = kIngestRows;; a.band >>= 1) {
        a.rows_cap = vpass ? ingest_span(H, hr, a.band) : a.band;
        chunk = ingest_lds(a, kIngestChunk) <= 64 * 1024 ? kIngestChunk : kIngestChunk / 2;
        if (ingest_lds(a, chunk) <= 64 * 1024) break;
        if (a.band == 1) return COBEVT_ERR_UNSUPPORTED;
    }
    const int bands = (hr - top + a.band - 1) / a.band;
    if (bands > 65535) return COBEVT_ERR_UNSUPPORTED;
    const dim3 grid(ntx, bands, n);
    if (chunk == kIngestChunk)
        hipLaunchKernelGGL((resize_pil_kernel<kIngestChunk>), grid, dim3(256), ingest_lds(a, chunk), stream, src, out, hpass ? hb : nullptr,
                           hc, vpass ? vb : nullptr, vc, lut, a);
    else
        hipLaunchKernelGGL((resize_pil_kernel<kIngestChunk / 2>), grid, dim3(256), ingest_lds(a, chunk), stream, src, out,
                           hpass ? hb : nullptr, hc, vpass ? vb : nullptr, vc, lut, a);
    return launch_status();
}

static int launch_decode_bev(const int* labels, float* out, int n, int hw, int C, hipStream_t stream) {
    if (!labels || !out) return COBEVT_ERR_ARG;
    if (n < 1 || n > 65535 || hw < 1 || C < 1 || C > kIngestMaxClasses) return COBEVT_ERR_SHAPE;
    hipLaunchKernelGGL(decode_bev_kernel, dim3((hw + 255) / 256, n), dim3(256), 0, stream, labels, out, hw, C);
    return launch_status();
}

}  // namespace cobevt

using namespace cobevt;

extern "C" int cobevt_resize_pil_u8(const unsigned char* src, void* out, const int* hbounds, const int* hcoeffs, const int* vbounds,
                                    const int* vcoeffs, const float* lut, const int* dims, hipStream_t stream) {
    return launch_resize_pil(src, out, hbounds, hcoeffs, vbounds, vcoeffs, lut, dims, stream);
}

extern "C" int cobevt_decode_bev(const int* labels, float* out, int N, int hw, int num_classes, hipStream_t stream) {
    return launch_decode_bev(labels, out, N, hw, num_classes, stream);
}
