// Transposed convolution with kernel = stride = s (no overlapping taps) + folded BatchNorm + activation, written pixel-shuffled into a
// channel slice of a wider NHWC map: the "deblocks" of BaseBEVBackbone             reference: opencood/models/backbones/base_bev_backbone.py
//
//   out[n, s*y + dy, s*x + dx, c_off + co] = act(shift[co] + sum_ci in[n, y, x, ci] * W'[(dy*s + dx)*Cout + co][ci])
//
// An fp32-storage matrix kernel: it includes f32_matrix.hpp, so it is built once per library, like igemm.hip.
//
// GEMM view: M = N*H*W input pixels (the NHWC input IS the [M][Cin] matrix), K = Cin, columns = s*s*Cout ordered tap-major, weights
// [s*s*Cout][Kpad] with the BatchNorm scale folded in.  Cout % 32 == 0, so a 32-column MFMA tile is 32 consecutive output channels of
// ONE tap (dy, dx): for every input pixel of the tile it lands on one destination pixel as 64 (bf16) / 128 (fp32) contiguous bytes.
//
// Workgroup = 4 waves on a 64-pixel x 128-column tile (waves 2 x 2, each 32 pixels x 2 x 32 columns), the K loop of the implicit GEMM:
// global -> register -> LDS with two buffers, one barrier per 64-byte K-tile.  The weights are the FIRST MFMA operand, so a lane of
// the C/D fragment holds, for pixel lane & 31, the channels 4*(lane >> 5) + 8*q + 0..3 (q = 0..3).
//
// Store scheme: the op is bound by the output write (K = 64..256 against s*s*Cout columns), so the epilogue does not store from the
// fragment (8 / 16 bytes per lane, four instructions per 64-byte run).  Each wave adds the shift, applies the activation, rounds to the
// storage type and writes its 32 x 32 tile into its own LDS region (the K loop's buffers, free after the last barrier), rows padded
// by 16 bytes; it then reads it back as 16-byte pieces in pixel-major order, so that 4 (bf16) / 8 (fp32) consecutive lanes store one
// destination pixel's whole 64 / 128-byte run with global_store_dwordx4.  Every destination element of the slice is written exactly
// once (no atomics, no zero-fill), nothing outside [c_off, c_off + Cout) is touched.
#include "common.hpp"
#include "f32_matrix.hpp"

namespace cobevt {

// this kernel's K-tile in LDS (the layout igemm.hip's loop uses too; the two files need not agree)
constexpr int kDeconvRowBytes = 80;  // 64 data + 16 pad
constexpr int kDeconvTileBytes = 64;

struct DeconvParams {
    const void* in;
    const void* wgt;
    const float* shift;
    void* out;
    int M, H, W, Cin;
    int Cout, NC, Kpad;
    int s, c_off, ldc, act;
};

constexpr int kDeconvBM = 64, kDeconvBN = 128;

template <typename T>
__global__ __launch_bounds__(256) void deconv_kernel(DeconvParams p) {
    constexpr int BM = kDeconvBM, BN = kDeconvBN;
    constexpr int ES = Elem<T>::kBytes;
    constexpr int BKE = kDeconvTileBytes / ES;
    constexpr int CH = Elem<T>::kChunk;
    constexpr int CPP = 32 * ES / 16;          // 16-byte pieces of one pixel's 32-channel run
    constexpr int ST_IT = 32 * CPP / 64;       // store instructions per 32 x 32 tile
    constexpr int ROWB = 32 * ES + 16;         // epilogue staging row: 32 channels + 16 bytes of padding
    static_assert(4 * 32 * ROWB <= 2 * (BM + BN) * kDeconvRowBytes, "the epilogue staging fits the K loop's buffers");

    __shared__ __attribute__((aligned(16))) unsigned char smem[2][(BM + BN) * kDeconvRowBytes];

    // consecutive workgroups: all column tiles of one pixel tile, then the next pixel tile (the pixel panel is re-read from L2)
    const int ntn = (p.NC + BN - 1) / BN;
    const int m0 = (blockIdx.x / ntn) * BM;
    const int n0 = (blockIdx.x % ntn) * BN;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int j = tid & 3;         // 16-byte chunk within the K-tile row
    const int rowp = tid >> 2;     // 0..63

    const T* in = (const T*)p.in;
    const T* wg = (const T*)p.wgt;
    const bool a_ok = m0 + rowp < p.M;
    const T* a_ptr = in + (size_t)(a_ok ? m0 + rowp : 0) * p.Cin + j * CH;
    const int nk = p.Kpad / BKE;
    uint4 a_reg, b_reg[2];

    auto load_tile = [&](int kt) {
        const int k = kt * BKE + j * CH;
        a_reg = make_uint4(0, 0, 0, 0);
        if (a_ok && k < p.Cin) a_reg = *(const uint4*)(a_ptr + kt * BKE);
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int col = n0 + rowp + 64 * it;
            b_reg[it] = make_uint4(0, 0, 0, 0);
            if (col < p.NC) b_reg[it] = *(const uint4*)(wg + ((size_t)col * p.Kpad + k));
        }
    };
    auto store_tile = [&](int buf) {
        unsigned char* As = smem[buf];
        unsigned char* Bs = smem[buf] + BM * kDeconvRowBytes;
        *(uint4*)(As + rowp * kDeconvRowBytes + j * 16) = stage_x_piece<T>(a_reg);
#pragma unroll
        for (int it = 0; it < 2; ++it) *(uint4*)(Bs + (rowp + 64 * it) * kDeconvRowBytes + j * 16) = stage_w_piece<T>(b_reg[it]);
    };

    f32x16 acc[2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;

    const int wm = wave >> 1, wn = wave & 1;
    const int frag_off = (lane & 31) * kDeconvRowBytes + (lane >> 5) * 16;

    load_tile(0);
    store_tile(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load_tile(kt + 1);
        const unsigned char* As = smem[buf] + wm * 32 * kDeconvRowBytes + frag_off;
        const unsigned char* Bs = smem[buf] + (BM + wn * 64) * kDeconvRowBytes + frag_off;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const uint4 xs = *(const uint4*)(As + g * 32);
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const uint4 ws = *(const uint4*)(Bs + b * 32 * kDeconvRowBytes + g * 32);
                mfma_kgroup_staged<T>(ws, xs, acc[b]);       // weights first: D row = channel, D column = pixel (f32_matrix.hpp)
            }
        }
        if (kt + 1 < nk) store_tile(buf ^ 1);
        __syncthreads();
    }

    // ---- epilogue (see the head of this file); the last barrier of the loop has released both K-tile buffers
    unsigned char* stg = &smem[0][0] + wave * (32 * ROWB);
    const int px = lane & 31, half = lane >> 5;
    const int sW = p.s * p.W;
    size_t dst_pix[ST_IT];         // destination pixel of tap (0, 0) for the piece this lane stores in round `it`
    bool dst_ok[ST_IT];
#pragma unroll
    for (int it = 0; it < ST_IT; ++it) {
        const int m = m0 + wm * 32 + (it * 64 + lane) / CPP;
        dst_ok[it] = m < p.M;
        const int mm = dst_ok[it] ? m : 0;
        const int hw = p.H * p.W;
        const int n = mm / hw, rem = mm - n * hw;
        const int y = rem / p.W, x = rem - y * p.W;
        dst_pix[it] = ((size_t)n * p.H + y) * p.s * sW + (size_t)x * p.s;
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int col0 = n0 + wn * 64 + b * 32;          // wave-uniform: 32 channels of one tap
        const bool tile_ok = col0 < p.NC;
        const int tap = tile_ok ? col0 / p.Cout : 0;
        const int co0 = tile_ok ? col0 - tap * p.Cout : 0;
        const int dy = tap / p.s, dx = tap - dy * p.s;
        if (tile_ok) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ch = 4 * half + 8 * q;
                const float4 sh = *(const float4*)(p.shift + co0 + ch);
                const float v0 = apply_act<T>(acc[b][4 * q + 0] + sh.x, p.act), v1 = apply_act<T>(acc[b][4 * q + 1] + sh.y, p.act);
                const float v2 = apply_act<T>(acc[b][4 * q + 2] + sh.z, p.act), v3 = apply_act<T>(acc[b][4 * q + 3] + sh.w, p.act);
                unsigned char* w = stg + px * ROWB + ch * ES;
                if constexpr (Elem<T>::kIsBf16) *(uint2*)w = make_uint2(pack_bf2(v0, v1), pack_bf2(v2, v3));
                else *(float4*)w = make_float4(v0, v1, v2, v3);
            }
        }
        __syncthreads();
        if (tile_ok) {
            unsigned char* out = (unsigned char*)p.out;
#pragma unroll
            for (int it = 0; it < ST_IT; ++it) {
                const int idx = it * 64 + lane;
                const int pp = idx / CPP, c = idx - pp * CPP;
                const uint4 v = *(const uint4*)(stg + pp * ROWB + c * 16);
                if (dst_ok[it]) {
                    const size_t elem = (dst_pix[it] + (size_t)dy * sW + dx) * p.ldc + p.c_off + co0;
                    *(uint4*)(out + elem * ES + c * 16) = v;
                }
            }
        }
        __syncthreads();
    }
}

template <typename T>
static int launch_deconv(const DeconvParams& p, hipStream_t stream) {
    const long long blocks = (long long)((p.M + kDeconvBM - 1) / kDeconvBM) * ((p.NC + kDeconvBN - 1) / kDeconvBN);
    if (blocks > 0x7fffffffLL) return COBEVT_ERR_SHAPE;
    hipLaunchKernelGGL((deconv_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, stream, p);
    return cobevt::launch_status();
}

}  // namespace cobevt

using namespace cobevt;

// C-ABI entry point, see include/cobevt_hip.h
extern "C" int cobevt_deconv_nhwc(const void* in, const void* wgt, const float* shift, void* out, const int* dims, hipStream_t stream) {
    // dims: [dtype, N, H, W, Cin, Cout, Kpad, s, c_off, ldc, act]
    if (!in || !wgt || !shift || !out || !dims) return COBEVT_ERR_ARG;
    const int dtype = dims[0], N = dims[1];
    if (dtype != 0 && dtype != 1) return COBEVT_ERR_ARG;
    DeconvParams p;
    p.in = in; p.wgt = wgt; p.shift = shift; p.out = out;
    p.H = dims[2]; p.W = dims[3]; p.Cin = dims[4]; p.Cout = dims[5]; p.Kpad = dims[6];
    p.s = dims[7]; p.c_off = dims[8]; p.ldc = dims[9]; p.act = dims[10];
    if (p.act < 0 || p.act > 4) return COBEVT_ERR_ARG;
    if (N <= 0 || p.H <= 0 || p.W <= 0 || p.Cin <= 0 || p.Cout <= 0) return COBEVT_ERR_SHAPE;
    if (p.s < 1 || p.s > 8) return COBEVT_ERR_SHAPE;
    const int bke = dtype == 0 ? 32 : 16, ch = dtype == 0 ? 8 : 4;
    if (p.Cin % ch != 0 || p.Cout % 32 != 0) return COBEVT_ERR_SHAPE;
    if (p.Kpad % bke != 0 || p.Kpad < p.Cin) return COBEVT_ERR_SHAPE;
    // 16-byte stores: the slice starts on an 8-channel boundary of a row whose length is a multiple of 8 channels
    if (p.c_off < 0 || p.c_off % 8 != 0 || p.ldc % 8 != 0 || (long long)p.c_off + p.Cout > p.ldc) return COBEVT_ERR_SHAPE;
    const long long M = (long long)N * p.H * p.W;
    if (M > 0x7fffffffLL - kDeconvBM || M * p.s * p.s > 0x7fffffffLL) return COBEVT_ERR_SHAPE;     // pixel indices are ints
    p.M = (int)M;
    p.NC = p.s * p.s * p.Cout;
    return dtype == 0 ? launch_deconv<bf16_t>(p, stream) : launch_deconv<float>(p, stream);
}
