// The device-only part of what the relative-attention kernels share (rel_attention.h is the part the host plan reads too):
// the vector types, the constants of the kernels' inner loops and the 16-bit operand trait of the two 16-bit forward files.
#pragma once
#include "device_prims.h"
#include "rel_attention.h"
#include "split_bf16.h"

namespace isi {

// constants of all the attention kernels; LD and the operand trait Prec are the 16-bit forward kernels'
// (rel_attention_fwd2.hip, rel_attention_fwd3.hip)
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

constexpr unsigned OOB = 0xFFFFFFF0u;   // a buffer offset beyond every descriptor: the load returns zeros
constexpr float NEG = -1e30f;
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
constexpr int LD = 68;     // floats per query row of the skew buffer (64 band rows + 4)

// the 16-bit operand type of a mode: conversions (round to nearest even) and the matrix instruction
template <bool F16> struct Prec;
template <> struct Prec<false> {
  static __device__ __forceinline__ unsigned pack2(const float a, const float b) {
    const f32x2_t v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
  }
  static __device__ __forceinline__ void split2(const float a, const float b, unsigned &hi, unsigned &lo) { isi::split2(a, b, hi, lo); }
  static __device__ __forceinline__ f32x16 mfma(const s16x8_t a, const s16x8_t b, const f32x16 c) { return ISI_MFB(a, b, c); }
};
template <> struct Prec<true> {
  static __device__ __forceinline__ unsigned pack2(const float a, const float b) {
    const f32x2_t v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2_t));
  }
  static __device__ __forceinline__ void split2(const float a, const float b, unsigned &hi, unsigned &lo) {
    const f32x2_t v = {a, b};
    const f16x2_t h = __builtin_convertvector(v, f16x2_t);
    const f16x2_t l = __builtin_convertvector(v - __builtin_convertvector(h, f32x2_t), f16x2_t);
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, l);
  }
  static __device__ __forceinline__ f32x16 mfma(const s16x8_t a, const s16x8_t b, const f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
  }
};

}  // namespace isi
