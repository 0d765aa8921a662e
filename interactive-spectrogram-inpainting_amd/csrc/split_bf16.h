// Split-bf16 helpers shared by the attention, convolution and GEMM kernels: an fp32 value is carried as hi + lo in bf16
// (hi = rne(x), lo = rne(x - hi)); a product a*b is evaluated as a_lo*b_hi + a_hi*b_lo + a_hi*b_hi on
// the bf16 matrix pipe with fp32 accumulation (the dropped lo*lo term is ~2^-18 of the product).
#pragma once
#include <hip/hip_runtime.h>

namespace isi {
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef short s16x8_t __attribute__((ext_vector_type(8)));

// (a, b) -> packed bf16 pairs: hi and lo parts (v_cvt_pk_bf16_f32)
__device__ __forceinline__ void split2(const float a, const float b, unsigned &hi, unsigned &lo) {
  const f32x2_t v = {a, b};
  const bf16x2_t h = __builtin_convertvector(v, bf16x2_t);
  const bf16x2_t l = __builtin_convertvector(v - __builtin_convertvector(h, f32x2_t), bf16x2_t);
  hi = __builtin_bit_cast(unsigned, h);
  lo = __builtin_bit_cast(unsigned, l);
}
__device__ __forceinline__ void split_f4(const float4 v, uint2 &hi, uint2 &lo) {
  split2(v.x, v.y, hi.x, lo.x);
  split2(v.z, v.w, hi.y, lo.y);
}
// the same pieces, as the convolution and residual-block kernels compute them ("bf16x3", ISI_CONV_BF16X3; ~10 VALU per
// float4): both lo pieces after both hi pieces.  Not written as a call of split_f4: with its order of statements the
// machine code of three resblock_f32_kernel instances comes out different (profiles/shared_device_helpers_isa.txt)
__device__ __forceinline__ void split_bf16x4(const float4 v, uint2 &hi, uint2 &lo) {
  const f32x2_t a = {v.x, v.y}, b = {v.z, v.w};
  const bf16x2_t ha = __builtin_convertvector(a, bf16x2_t), hb = __builtin_convertvector(b, bf16x2_t);
  const bf16x2_t la = __builtin_convertvector(a - __builtin_convertvector(ha, f32x2_t), bf16x2_t);
  const bf16x2_t lb = __builtin_convertvector(b - __builtin_convertvector(hb, f32x2_t), bf16x2_t);
  hi = make_uint2(__builtin_bit_cast(unsigned, ha), __builtin_bit_cast(unsigned, hb));
  lo = make_uint2(__builtin_bit_cast(unsigned, la), __builtin_bit_cast(unsigned, lb));
}
// x = hi + mid + lo exactly (3 x 8 significand bits): the six products hi.hi, hi.mid, mid.hi, hi.lo, lo.hi,
// mid.mid carry every term above 2^-24 of the result ("bf16x6", ISI_CONV_BF16X6: fp32-grade products at 6/16 of the
// fp32 pipe's time)
__device__ __forceinline__ void split3_bf16x4(const float4 v, uint2 &hi, uint2 &mid, uint2 &lo) {
  const f32x2_t a = {v.x, v.y}, b = {v.z, v.w};
  const bf16x2_t ha = __builtin_convertvector(a, bf16x2_t), hb = __builtin_convertvector(b, bf16x2_t);
  const f32x2_t ra = a - __builtin_convertvector(ha, f32x2_t), rb = b - __builtin_convertvector(hb, f32x2_t);
  const bf16x2_t ma = __builtin_convertvector(ra, bf16x2_t), mb = __builtin_convertvector(rb, bf16x2_t);
  const bf16x2_t la = __builtin_convertvector(ra - __builtin_convertvector(ma, f32x2_t), bf16x2_t);
  const bf16x2_t lb = __builtin_convertvector(rb - __builtin_convertvector(mb, f32x2_t), bf16x2_t);
  hi = make_uint2(__builtin_bit_cast(unsigned, ha), __builtin_bit_cast(unsigned, hb));
  mid = make_uint2(__builtin_bit_cast(unsigned, ma), __builtin_bit_cast(unsigned, mb));
  lo = make_uint2(__builtin_bit_cast(unsigned, la), __builtin_bit_cast(unsigned, lb));
}
// 16 accumulator registers of a 32x32 tile -> the two 16-deep k-blocks of an MFMA B operand (hi and lo):
// k-slot (half h, e) of block t is accumulator row 16 t + 8 (e >> 2) + 4 h + (e & 3) = register 8 t + e
__device__ __forceinline__ void split_acc16(const float *v, s16x8_t *hi, s16x8_t *lo) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    unsigned hh[4], ll[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) split2(v[8 * t + 2 * e], v[8 * t + 2 * e + 1], hh[e], ll[e]);
    hi[t] = __builtin_bit_cast(s16x8_t, make_uint4(hh[0], hh[1], hh[2], hh[3]));
    lo[t] = __builtin_bit_cast(s16x8_t, make_uint4(ll[0], ll[1], ll[2], ll[3]));
  }
}
}  // namespace isi

#define ISI_MFB(a, b, c) \
  __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0)
