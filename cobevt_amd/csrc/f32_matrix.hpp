// The fp32-storage matrix path: everything in the csrc tree whose meaning depends on which of the package's three libraries is being
// built.  This is the ONLY file that reads COBEVT_F32_SPLIT, and a source is compiled once per library exactly when it includes
// this header (cobevt_amd/build.py derives that from the include graph); every other source is compiled once and its object is
// linked into all three libraries.  So: include it directly from a .hip file whose fp32-storage kernels issue matrix products, and
// never from a shared header (attn_common.hpp, wave_ops.hpp, warp_common.hpp, row_chain.hpp, ...) - that would make every source
// behind that header a per-library one.  common.hpp only DECLARES mfma_kgroup_f32: a source that instantiates mfma_kgroup<float>
// without this header does not build.
//
//   COBEVT_F32_SPLIT  library                  one 16-byte piece of fp32 operands goes through
//   0 (default)       libcobevt_hip.so         four v_mfma_f32_32x32x2_f32: exact fp32
//   1                 libcobevt_hip_f32s.so    two v_mfma_f32_32x32x16_bf16 over (hi, lo) bf16 halves: ~1e-5 end to end
//   2                 libcobevt_hip_f32h.so    one v_mfma_f32_32x32x16_f16, the weight side as a single fp16 term
// All three export the same C ABI; bf16 storage (T = bf16_t) is the same code in all of them.
#pragma once
#include "common.hpp"

#ifndef COBEVT_F32_SPLIT
#define COBEVT_F32_SPLIT 0
#endif

namespace cobevt {

// COBEVT_F32_SPLIT = 1 builds the SECOND library of the package (cobevt_amd/build.py: libcobevt_hip_f32s.so): every fp32-storage
// kernel of the inference path then takes its matrix products through the split-bf16 form below instead of
// v_mfma_f32_32x32x2_f32 - the strict-parity mode that is not 16x off the bf16 matrix rate.

// (x, y) -> packed bf16 pairs (hi(x), hi(y)) and (lo(x), lo(y)): hi = round-to-nearest-even bf16, lo = bf16(x - hi) (x - hi is exact)
__device__ __forceinline__ void split_bf16_pair(float x, float y, uint32_t& hi, uint32_t& lo) {
    hi = pack_bf2(x, y);
    lo = pack_bf2(x - __uint_as_float(hi << 16), y - __uint_as_float(hi & 0xffff0000u));
}

// COBEVT_F32_SPLIT = 2 builds the THIRD library (libcobevt_hip_f32h.so; round 6): fp32 storage, ONE
// v_mfma_f32_32x32x16_f16 per 16-byte piece.  The activation-side piece x[0..3] goes in as an fp16 pair per value -
// hi = fp16(x), lo = fp16((x - hi) * 2^kF16LoShift): 22 significand bits - and the weight-side piece w[0..3] as ONE fp16 term, once
// at full scale against the hi slots and once scaled by 2^-kF16LoShift against the lo slots: sum_k (x_hi + x_lo) w_hi, i.e. the
// weights are rounded to 11 bits and nothing else is.  Half the matrix time of the split-bf16 form; only the ResNet encoder's
// convolutions are routed through this library (host/resnet_ms.py under set_compute_dtype("fp32_fast")): measured with the CPU
// oracle (tools/precision_emul.py, mode fp16_we) that costs 2.7-2.8e-4 max-rel / 1.0-1.5e-4 rms-rel on the 5-agent frame's logits,
// where fp16 weights in EVERY product cost 0.8-1.0e-3 and fp16 operands on both sides 1.6e-3 (the north-star's gate is 1e-3).
// The shift keeps the lo slots out of fp16's subnormal range for |x| >= 4e-3 (lo ~ 2^-12 |x|) whether or not the matrix pipe
// flushes subnormals; the scaled weight copy is normal for |w| >= 4e-3 and below that the lo term it would carry is < 2^-12 * 4e-3 |x|.
// Range: |x|, |w| <= 65504 (fp16) - the same precondition as the reference's own fp16 autocast (train_camera.py:157-160).
using f16x2 = __attribute__((ext_vector_type(2))) _Float16;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
constexpr float kF16LoScale = 64.0f;             // 2^6
__device__ __forceinline__ uint32_t pack_h2(float lo, float hi) {
    const f32x2 v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2));
}
// activation-side piece -> {hi(x0,x1), hi(x2,x3), lo(x0,x1), lo(x2,x3)}
__device__ __forceinline__ uint4 split_f16_piece(const uint4& x) {
    const float x0 = __uint_as_float(x.x), x1 = __uint_as_float(x.y), x2 = __uint_as_float(x.z), x3 = __uint_as_float(x.w);
    const uint32_t h01 = pack_h2(x0, x1), h23 = pack_h2(x2, x3);
    const f16x2 a = __builtin_bit_cast(f16x2, h01), b = __builtin_bit_cast(f16x2, h23);
    const uint32_t l01 = pack_h2((x0 - (float)a[0]) * kF16LoScale, (x1 - (float)a[1]) * kF16LoScale);
    const uint32_t l23 = pack_h2((x2 - (float)b[0]) * kF16LoScale, (x3 - (float)b[1]) * kF16LoScale);
    return make_uint4(h01, h23, l01, l23);
}
// weight-side piece -> {w01, w23, w01 / 2^s, w23 / 2^s} as fp16
__device__ __forceinline__ uint4 dup_f16_piece(const uint4& w) {
    const uint32_t h01 = pack_h2(__uint_as_float(w.x), __uint_as_float(w.y)), h23 = pack_h2(__uint_as_float(w.z), __uint_as_float(w.w));
    const f16x2 inv = {(_Float16)(1.0f / kF16LoScale), (_Float16)(1.0f / kF16LoScale)};
    const f16x2 s01 = __builtin_bit_cast(f16x2, h01) * inv, s23 = __builtin_bit_cast(f16x2, h23) * inv;
    return make_uint4(h01, h23, __builtin_bit_cast(uint32_t, s01), __builtin_bit_cast(uint32_t, s23));
}

// The fp32-storage branch of mfma_kgroup<T, kWeightsFirst> (common.hpp, which documents the operands and the C/D layout).
template <bool kWeightsFirst>
__device__ __forceinline__ void mfma_kgroup_f32(const uint4& a, const uint4& b, f32x16& acc) {
#if COBEVT_F32_SPLIT == 2
    const uint4 av = kWeightsFirst ? dup_f16_piece(a) : split_f16_piece(a);
    const uint4 bv = kWeightsFirst ? split_f16_piece(b) : dup_f16_piece(b);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, av), __builtin_bit_cast(f16x8, bv), acc, 0, 0, 0);
#elif COBEVT_F32_SPLIT
    // fp32 storage, split-bf16 matrix path (libcobevt_hip_f32s.so): x = hi + lo with hi = bf16(x), lo = bf16(x - hi),
    // |x - hi - lo| <= 2^-17 |x|.  The bf16 instruction contracts 8 element pairs per lane half where the piece holds 4
    // values, so A carries {hi[0..3], lo[0..3]} and B {hi[0..3], hi[0..3]} / {lo[0..3], lo[0..3]}: two
    // v_mfma_f32_32x32x16_bf16 (64 matrix-pipe cycles) add all FOUR cross terms (hi+lo)(hi+lo) of the 8 products that the
    // four v_mfma_f32_32x32x2_f32 (256 cycles) form exactly; bf16 x bf16 products are exact in the fp32 accumulator.
    uint32_t ah[2], al[2], bh[2], bl[2];
    split_bf16_pair(__uint_as_float(a.x), __uint_as_float(a.y), ah[0], al[0]);
    split_bf16_pair(__uint_as_float(a.z), __uint_as_float(a.w), ah[1], al[1]);
    split_bf16_pair(__uint_as_float(b.x), __uint_as_float(b.y), bh[0], bl[0]);
    split_bf16_pair(__uint_as_float(b.z), __uint_as_float(b.w), bh[1], bl[1]);
    const uint4 av = make_uint4(ah[0], ah[1], al[0], al[1]);
    const uint4 bhv = make_uint4(bh[0], bh[1], bh[0], bh[1]);
    const uint4 blv = make_uint4(bl[0], bl[1], bl[0], bl[1]);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, bhv), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, blv), acc, 0, 0, 0);
#else
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
#endif
}

// Activation pieces split ONCE, when a kernel stages them into an LDS patch that only feeds MFMA operand reads (fp32 storage in the
// second and third library): the in-loop forms above spend 12-14 VALU instructions per MFMA on the split, in a dependent chain between
// the LDS read and the MFMA (third library, 256 -> 256 on 20 x 32 x 32: 77 us in-loop, 54.7 us staged), while a patch piece is read by
// 9 taps x every cout tile of the workgroup.  Staged form of a piece {x0..x3}: {hi(x0,x1), hi(x2,x3), lo(x0,x1), lo(x2,x3)} - bf16 halves
// in the second library (x = hi + lo to 2^-17), fp16 halves with the scaled lo in the third.  stage_x_piece is the identity in the native
// library and for bf16 storage, and mfma_kgroup_xs is mfma_kgroup<T> (weights first) there.
template <typename T> constexpr bool kXSplit = (COBEVT_F32_SPLIT != 0) && !Elem<T>::kIsBf16;
template <typename T> constexpr bool kXSplit16 = (COBEVT_F32_SPLIT == 2) && !Elem<T>::kIsBf16;      // ... and the halves are fp16 (third library)
__device__ __forceinline__ void split_pair_staged(float x, float y, uint32_t& hi, uint32_t& lo) {
#if COBEVT_F32_SPLIT == 2
    hi = pack_h2(x, y);
    const f16x2 hv = __builtin_bit_cast(f16x2, hi);
    lo = pack_h2((x - (float)hv[0]) * kF16LoScale, (y - (float)hv[1]) * kF16LoScale);
#else
    split_bf16_pair(x, y, hi, lo);
#endif
}
template <typename T> __device__ __forceinline__ uint4 stage_x_piece(const uint4& x) {
    if constexpr (kXSplit<T>) {
        uint32_t h01, h23, l01, l23;
        split_pair_staged(__uint_as_float(x.x), __uint_as_float(x.y), h01, l01);
        split_pair_staged(__uint_as_float(x.z), __uint_as_float(x.w), h23, l23);
        return make_uint4(h01, h23, l01, l23);
    } else {
        return x;
    }
}
// w = the raw fp32 weight piece (a register fragment shared by the MT strips / pixel tiles of the wave: its split is amortised), xs = staged
template <typename T> __device__ __forceinline__ void mfma_kgroup_xs(const uint4& w, const uint4& xs, f32x16& acc) {
    if constexpr (kXSplit<T>) {
#if COBEVT_F32_SPLIT == 2
        const uint4 wv = dup_f16_piece(w);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wv), __builtin_bit_cast(f16x8, xs), acc, 0, 0, 0);
#else
        // (w_hi, w_hi) . (x_hi, x_lo) + (w_lo, w_lo) . (x_hi, x_lo): the same four cross terms as mfma_kgroup's split form
        uint32_t h01, h23, l01, l23;
        split_bf16_pair(__uint_as_float(w.x), __uint_as_float(w.y), h01, l01);
        split_bf16_pair(__uint_as_float(w.z), __uint_as_float(w.w), h23, l23);
        const uint4 wh = make_uint4(h01, h23, h01, h23), wl = make_uint4(l01, l23, l01, l23);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wh), __builtin_bit_cast(bf16x8, xs), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wl), __builtin_bit_cast(bf16x8, xs), acc, 0, 0, 0);
#endif
    } else {
        mfma_kgroup<T>(w, xs, acc);
    }
}

// Both operands staged: a kernel that also keeps its WEIGHTS in LDS converts them once with stage_w_piece - the duplicated form in the
// third library, the (hi, lo) form in the second, whose second product takes the weight piece with its halves swapped.  Two consumers,
// which differ only in operand order: mfma_kgroup_staged (weights first: the stem) and mfma_kgroup_ss (activations first, below).
template <typename T> __device__ __forceinline__ uint4 stage_w_piece(const uint4& w) {
    if constexpr (kXSplit<T>) {
#if COBEVT_F32_SPLIT == 2
        return dup_f16_piece(w);
#else
        return stage_x_piece<T>(w);          // {hi01, hi23, lo01, lo23}: the second product of mfma_kgroup_staged / _ss takes it with the halves swapped
#endif
    } else {
        return w;
    }
}
template <typename T> __device__ __forceinline__ void mfma_kgroup_staged(const uint4& ws, const uint4& xs, f32x16& acc) {
    if constexpr (kXSplit<T>) {
#if COBEVT_F32_SPLIT == 2
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, ws), __builtin_bit_cast(f16x8, xs), acc, 0, 0, 0);
#else
        const uint4 wsw = make_uint4(ws.z, ws.w, ws.x, ws.y);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ws), __builtin_bit_cast(bf16x8, xs), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wsw), __builtin_bit_cast(bf16x8, xs), acc, 0, 0, 0);
#endif
    } else {
        mfma_kgroup<T>(ws, xs, acc);
    }
}

// BOTH operands staged through LDS (the LDS-staged 3x3 kernel, the 128 x 128 dense-row kernel, the implicit GEMM): activations first.
// Second library: both tiles hold the {hi01, hi23, lo01, lo23} form; x . w = (x_hi, x_lo) . (w_hi, w_lo) + (x_hi, x_lo) . (w_lo, w_hi) -
// the second product takes the weight piece with its halves swapped (four register moves), so the loop has no conversion at all where the
// in-loop split spent 36 VALU instructions per two MFMA pairs.  Third library: x staged, w in the duplicated form, one fp16 MFMA.
template <typename T> __device__ __forceinline__ void mfma_kgroup_ss(const uint4& xs, const uint4& ws, f32x16& acc) {
    if constexpr (kXSplit<T>) {
#if COBEVT_F32_SPLIT == 2
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, xs), __builtin_bit_cast(f16x8, ws), acc, 0, 0, 0);
#else
        const uint4 wsw = make_uint4(ws.z, ws.w, ws.x, ws.y);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, xs), __builtin_bit_cast(bf16x8, ws), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, xs), __builtin_bit_cast(bf16x8, wsw), acc, 0, 0, 0);
#endif
    } else {
        mfma_kgroup<T, false>(xs, ws, acc);
    }
}

// PACKED fp16 form (third library, round 6 second step): tests/precision_emul.py mode fp16_e2 - BOTH operands of the ResNet encoder's
// convolutions rounded to fp16 - measures the same 2.7-2.8e-4 on the 5-agent frame as fp16 weights alone (the weights' rounding is what is
// seen; post-ReLU activations add nothing measurable), so the (hi, lo) pair of the activations buys nothing there and its four MFMA slots can
// carry a second k-group instead: a staged patch keeps ONE fp16 per activation, the 16-byte operand of lane half h is
// {k-group 2q: channels 4h .. 4h + 3, k-group 2q + 1: channels 4h .. 4h + 3}, and a pair of weight fragments is packed the same way -
// one v_mfma_f32_32x32x16_f16 per TWO k-groups, the bf16 kernels' matrix time on fp32 storage.  Kernels whose wave owns an even number of
// k-groups per tap use it (kXPack); the others keep the (hi, lo) form above.
template <typename T, int KGW> constexpr bool kXPack = (COBEVT_F32_SPLIT == 2) && !Elem<T>::kIsBf16 && (KGW % 2 == 0);
__device__ __forceinline__ uint2 pack_f16_hi(const uint4& x) {
    return make_uint2(pack_h2(__uint_as_float(x.x), __uint_as_float(x.y)), pack_h2(__uint_as_float(x.z), __uint_as_float(x.w)));
}
__device__ __forceinline__ uint4 pack_f16_pair(const uint4& w0, const uint4& w1) {
    const uint2 a = pack_f16_hi(w0), b = pack_f16_hi(w1);
    return make_uint4(a.x, a.y, b.x, b.y);
}
// byte offset of 16-byte piece j = 2 * kgroup + half of a 128-byte channel chunk inside the packed image of that chunk (its 8 bytes)
__device__ __forceinline__ constexpr int packed_piece_offset(int j) { return (j >> 2) * 32 + (j & 1) * 16 + ((j >> 1) & 1) * 8; }
__device__ __forceinline__ void mfma_f16_packed(const uint4& w, const uint4& x, f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, w), __builtin_bit_cast(f16x8, x), acc, 0, 0, 0);
}

// THREE-TERM form on k-group pairs (second library): where a wave owns an even number of k-groups per tap, the staged
// patch keeps the hi halves and the lo halves of a PAIR of k-groups as two separate 16-byte operands per lane half - {hi(2q): 4 values,
// hi(2q + 1): 4 values} and the same for lo - and a pair of weight fragments is split the same way: w_hi . x_hi + w_hi . x_lo + w_lo . x_hi,
// THREE v_mfma_f32_32x32x16_bf16 per two k-groups instead of four.  The dropped w_lo . x_lo term is 2^-16 of a product, the same order as
// the operands' own 2^-17 residuals: ~2e-5 end to end instead of 1e-5.
template <typename T, int KGW> constexpr bool kXPack3 = (COBEVT_F32_SPLIT == 1) && !Elem<T>::kIsBf16 && (KGW % 2 == 0);
// byte offset of the hi half (8 bytes; the lo half sits 16 bytes further) of piece j = 2 * kgroup + half inside the image of a 128-byte chunk
__device__ __forceinline__ constexpr int packed3_piece_offset(int j) { return (j >> 2) * 64 + (j & 1) * 32 + ((j >> 1) & 1) * 8; }
__device__ __forceinline__ void store_piece_packed3(unsigned char* dst, const uint4& x, bool zero) {
    uint32_t h01, h23, l01, l23;
    split_bf16_pair(__uint_as_float(x.x), __uint_as_float(x.y), h01, l01);
    split_bf16_pair(__uint_as_float(x.z), __uint_as_float(x.w), h23, l23);
    *(uint2*)dst = zero ? make_uint2(0, 0) : make_uint2(h01, h23);
    *(uint2*)(dst + 16) = zero ? make_uint2(0, 0) : make_uint2(l01, l23);
}
__device__ __forceinline__ void split_w_pair(const uint4& w0, const uint4& w1, uint4& wh, uint4& wl) {
    uint32_t h[4], l[4];
    split_bf16_pair(__uint_as_float(w0.x), __uint_as_float(w0.y), h[0], l[0]);
    split_bf16_pair(__uint_as_float(w0.z), __uint_as_float(w0.w), h[1], l[1]);
    split_bf16_pair(__uint_as_float(w1.x), __uint_as_float(w1.y), h[2], l[2]);
    split_bf16_pair(__uint_as_float(w1.z), __uint_as_float(w1.w), h[3], l[3]);
    wh = make_uint4(h[0], h[1], h[2], h[3]);
    wl = make_uint4(l[0], l[1], l[2], l[3]);
}
__device__ __forceinline__ void mfma_3term(const uint4& wh, const uint4& wl, const uint4& xh, const uint4& xl, f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wh), __builtin_bit_cast(bf16x8, xh), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wh), __builtin_bit_cast(bf16x8, xl), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wl), __builtin_bit_cast(bf16x8, xh), acc, 0, 0, 0);
}

}  // namespace cobevt
