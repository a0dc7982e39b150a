// Shared device helpers for the cobevt_amd HIP kernels (gfx950 / CDNA4 only).
//
// Two arithmetic modes share every kernel through one template parameter:
//   T = bf16_t : activations/weights stored bf16, v_mfma_f32_32x32x16_bf16, fp32 accumulate (perf mode)
//   T = float  : activations/weights stored fp32, v_mfma_f32_32x32x2_f32, exact fp32    (parity mode)
// Both modes address LDS tiles at byte level the same way: a "k-group" is 32 bytes per row
// (16 bf16 or 8 fp32); lane-half h = lane>>5 owns bytes [16h, 16h+16) of every k-group.  For fp32 the
// four floats of that 16-byte piece feed four 32x32x2 MFMAs, i.e. the contraction index is permuted
// identically on the A and B side, which leaves the sum unchanged.
//
// Nothing in this file depends on which of the package's three libraries is being built, and every source includes it.  What the
// T = float matrix products become in the second and third library - and every helper that goes with that - is f32_matrix.hpp,
// which only the sources with fp32-storage matrix kernels include; those are the sources the build compiles once per library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// error codes shared with include/cobevt_hip.h
#define COBEVT_OK 0
#define COBEVT_ERR_ARG 1
#define COBEVT_ERR_SHAPE 2
#define COBEVT_ERR_LAUNCH 3
#define COBEVT_ERR_UNSUPPORTED 4

namespace cobevt {

struct bf16_t { uint16_t bits; };

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

__device__ __forceinline__ float bf2f(uint16_t b) { return __uint_as_float(((uint32_t)b) << 16); }

using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using f32x2 = __attribute__((ext_vector_type(2))) float;

// fp32 pair -> packed bf16 pair with the hardware converter (v_cvt_pk_bf16_f32: round-to-nearest-even, the same
// rounding as torch.float32 -> torch.bfloat16); `lo` lands in bits 15:0.
__device__ __forceinline__ uint32_t pack_bf2(float lo, float hi) {
    const f32x2 v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

__device__ __forceinline__ uint16_t f2bf(float f) { return (uint16_t)(pack_bf2(f, 0.f) & 0xffffu); }

template <typename T> struct Elem;
template <> struct Elem<bf16_t> {
    static constexpr int kBytes = 2;
    static constexpr int kChunk = 8;   // elements per 16-byte chunk
    static constexpr bool kIsBf16 = true;
};
template <> struct Elem<float> {
    static constexpr int kBytes = 4;
    static constexpr int kChunk = 4;
    static constexpr bool kIsBf16 = false;
};

// A 16-byte chunk unpacked to fp32 lanes (8 values for bf16, 4 for fp32; unused tail left untouched).
template <typename T> __device__ __forceinline__ void chunk_to_f32(const uint4& c, float* v) {
    if constexpr (Elem<T>::kIsBf16) {
        v[0] = bf2f(c.x & 0xffff); v[1] = bf2f(c.x >> 16);
        v[2] = bf2f(c.y & 0xffff); v[3] = bf2f(c.y >> 16);
        v[4] = bf2f(c.z & 0xffff); v[5] = bf2f(c.z >> 16);
        v[6] = bf2f(c.w & 0xffff); v[7] = bf2f(c.w >> 16);
    } else {
        v[0] = __uint_as_float(c.x); v[1] = __uint_as_float(c.y);
        v[2] = __uint_as_float(c.z); v[3] = __uint_as_float(c.w);
    }
}
template <typename T> __device__ __forceinline__ uint4 f32_to_chunk(const float* v) {
    uint4 c;
    if constexpr (Elem<T>::kIsBf16) {
        c.x = pack_bf2(v[0], v[1]); c.y = pack_bf2(v[2], v[3]);
        c.z = pack_bf2(v[4], v[5]); c.w = pack_bf2(v[6], v[7]);
    } else {
        c.x = __float_as_uint(v[0]); c.y = __float_as_uint(v[1]);
        c.z = __float_as_uint(v[2]); c.w = __float_as_uint(v[3]);
    }
    return c;
}

template <typename T> __device__ __forceinline__ float load_elem(const T* p, size_t i);
template <> __device__ __forceinline__ float load_elem<bf16_t>(const bf16_t* p, size_t i) { return bf2f(p[i].bits); }
template <> __device__ __forceinline__ float load_elem<float>(const float* p, size_t i) { return p[i]; }
template <typename T> __device__ __forceinline__ void store_elem(T* p, size_t i, float v);
template <> __device__ __forceinline__ void store_elem<bf16_t>(bf16_t* p, size_t i, float v) { p[i].bits = f2bf(v); }
template <> __device__ __forceinline__ void store_elem<float>(float* p, size_t i, float v) { p[i] = v; }

// four consecutive elements at element offset `off` of an fp32 (sb = 0) or bf16 (sb = 1) tensor, as fp32 (the training kernels
// take either storage behind one pointer)
__device__ __forceinline__ float4 ld4q(const void* base, size_t off, int sb) {
    if (sb) {
        const uint2 u = *(const uint2*)((const uint16_t*)base + off);
        return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
    }
    return *(const float4*)((const float*)base + off);
}
__device__ __forceinline__ void st4q(void* base, size_t off, int sb, const float4& v) {
    if (sb) *(uint2*)((uint16_t*)base + off) = make_uint2(pack_bf2(v.x, v.y), pack_bf2(v.z, v.w));
    else *(float4*)((float*)base + off) = v;
}

// One 32-byte k-group of a 32x32 MFMA tile.  `a` and `b` are the 16-byte pieces this lane read from
// row (lane&31) of the A tile and the B tile at byte offset 16*(lane>>5) of the k-group.
// C/D layout (both dtypes): col = lane&31 (B row), row = (r&3) + 8*(r>>2) + 4*(lane>>5) (A row).
// kWeightsFirst: which operand is the weight-like one (D = W . X^T kernels pass the weights as `a`) - only the fp16 form of the
// third library distinguishes the two sides.
// The fp32-storage branch is the one thing here that differs between the package's libraries, so it is only declared: f32_matrix.hpp
// defines it, and a source whose kernels take it includes that header itself (and is then built once per library).
template <bool kWeightsFirst> __device__ __forceinline__ void mfma_kgroup_f32(const uint4& a, const uint4& b, f32x16& acc);
template <typename T, bool kWeightsFirst = true>
__device__ __forceinline__ void mfma_kgroup(const uint4& a, const uint4& b, f32x16& acc) {
    if constexpr (Elem<T>::kIsBf16) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a),
                                                      __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
    } else {
        mfma_kgroup_f32<kWeightsFirst>(a, b, acc);
    }
}

// accumulator register r of the 32x32 C/D fragment -> row within the tile
__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// erf by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7, below fp32 epilogue noise): one v_exp + one v_rcp + a degree-5
// polynomial instead of libm's multi-range erff (~40 instructions), which dominated the GELU epilogues.
__device__ __forceinline__ float erf_as(float x) {
    const float ax = fabsf(x);
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.0f));
    float poly = fmaf(1.061405429f, t, -1.453152027f);
    poly = fmaf(poly, t, 1.421413741f);
    poly = fmaf(poly, t, -0.284496736f);
    poly = fmaf(poly, t, 0.254829592f);
    const float e = __builtin_amdgcn_exp2f(-ax * ax * 1.4426950408889634f);
    const float y = fmaf(-poly * t, e, 1.0f);
    return copysignf(y, x);
}

// exact (erf) GELU of the reference: nn.GELU() default
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erf_as(x * 0.70710678118654752440f)); }

// GELU of the bf16 kernels (fax_modules.py:309-313, base_transformer.py:108): x Phi(x) as x * sigmoid(x (p0 + p1 x^2 + p2 x^4))
// with (p0, p1, p2) = (1.59433946, 0.0745210325, -7.69554552e-4) fitted to the exact x Phi(x) (the tanh form's 0.044715 cubic
// plus a quintic term): |error| <= 6.2e-5 for x >= -8 (below that the result is x * 7e-12 instead of a value tending to -0: < 1e-9 in magnitude down to x = -100) and <= 0.38 of the bf16 rounding error 2^-9 max(|gelu(x)|, 0.01) the result
// meets next - it is stored as bf16 in every kernel that calls this.  Seven VALU instructions (one v_exp_f32, one v_rcp_f32)
// against ~25 for the A&S erf form, which was 3.2k of the 5.5k VALU instructions of a 32-row block of the level-0 row chain.
// The polynomial turns over beyond |x| ~ 8.2, so its argument is clamped to [-8, 8] (sigmoid there: 1 - 7e-12 / 7e-12);
// the coefficients below carry the factor -log2(e) of exp(-z) = exp2(-z log2 e).  fp32 mode keeps gelu_erf.
__device__ __forceinline__ float gelu_bf16(float x) {
    const float xc = __builtin_amdgcn_fmed3f(x, -8.0f, 8.0f);
    const float u = xc * xc;
    float w = fmaf(u, 0.0011102325515821576f, -0.10751112550497055f);
    w = fmaf(w, u, -2.3001456260681152f);
    const float e = __builtin_amdgcn_exp2f(xc * w);
    return x * __builtin_amdgcn_rcpf(1.0f + e);
}
#ifdef COBEVT_GELU_EXACT          // A/B builds only (tools/build_variant.py): the erf form in the bf16 kernels too.  In front of gelu_t,
#define gelu_bf16 gelu_erf        // so that apply_act<T> (conv3x3, gemm_rows, gemm_rows3, igemm epilogues) switches with the direct callers
#endif
template <typename T> __device__ __forceinline__ float gelu_t(float x) {
    if constexpr (sizeof(T) == 2) return gelu_bf16(x);
    else return gelu_erf(x);
}

// epilogue activations by code: 0 none, 1 ReLU, 2 exact GELU, 3 swish x * sigmoid(x) (EfficientNet MBConv), 4 sigmoid
__device__ __forceinline__ float sigmoid_f(float x) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x)); }
template <typename T = float> __device__ __forceinline__ float apply_act(float x, int act) {
    if (act == 1) return fmaxf(x, 0.f);
    if (act == 2) return gelu_t<T>(x);
    if (act == 3) return x * sigmoid_f(x);
    if (act == 4) return sigmoid_f(x);
    return x;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a PER-DEVICE attribute: the limit is raised once per device the process
// launches on, not once per process.  Launch sites do not use this directly: they call allow_dynamic_lds below.
struct PerDeviceOnce {
    unsigned long long done = 0;
    bool first() {
        int d = 0;
        if (hipGetDevice(&d) != hipSuccess || d < 0 || d > 63) return true;
        const unsigned long long bit = 1ull << d;
        if (done & bit) return false;
        done |= bit;
        return true;
    }
};

// Opt `Kernel` into `bytes` of dynamic LDS (more than the default 64 KB) on the current device; called in front of every launch
// of such a kernel, it sets the attribute the first time the kernel is launched on a device.
template <auto Kernel> inline void allow_dynamic_lds(int bytes) {
    static PerDeviceOnce once;
    if (once.first()) (void)hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

// what an entry point returns after its launches
inline int launch_status() { return hipGetLastError() == hipSuccess ? COBEVT_OK : COBEVT_ERR_LAUNCH; }

}  // namespace cobevt
