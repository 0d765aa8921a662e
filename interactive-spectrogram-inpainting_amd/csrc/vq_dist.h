// The exact-fp32 distance stage the codebook searches share (vq_nearest.hip: one nearest code; vq_topm.hip: the M
// nearest among a palette), each piece defined ONCE and __forceinline__, in the manner of device_prims.h: a kernel's
// machine code does not depend on where the pieces are written down.
//
//   d[n,k] = (|z_n|^2 - 2 z_n.e_k) + |e_k|^2          (fp32, the reference's association, bottleneck.py:54-58)
//
// The codebook lies in LDS as [Kp][D + 4] fp32 rows (Kp = K rounded up to the 32-code MFMA tile; padding rows are
// zeros whose |e|^2 is +inf).  A wave handles 32 vectors per pass: z.e_k runs on the exact-fp32 matrix pipe with the
// operands swapped (codes = MFMA rows, vectors = MFMA columns), so the 16 accumulators of a lane all belong to ONE
// vector -- lane l and lane l + 32 hold interleaved code rows (mfma_row) of the same vector, and interleaved quads of
// its components: quad 2 j + half in zq[j].
#pragma once
#include "device_prims.h"

namespace isi {

#ifndef ISI_VQ_WAVES
#define ISI_VQ_WAVES 8
#endif
constexpr int VQ_BLOCK = 64 * ISI_VQ_WAVES;
constexpr int VQ_VEC_PER_BLOCK_ITER = 32 * ISI_VQ_WAVES;  // each wave owns 32 vectors per pass

// bytes of LDS the exact search keeps: codebook rows, |e|^2, per-wave sums, histogram (vq_nearest_kernel's layout)
template <int D>
constexpr size_t vq_exact_lds_bytes(int Kp) { return ((size_t)Kp * (D + 4) + 2 * Kp + ISI_VQ_WAVES) * sizeof(float); }
constexpr size_t kVqLdsBudget = 150 * 1024;

// codebook -> LDS (once per persistent workgroup): [Kp][D + 4], rows >= K zero
template <int D>
__device__ __forceinline__ void vq_fill_rows_f32(float *cb, const float *__restrict__ codes, int K, int Kp, int tid) {
  constexpr int LDD = D + 4;  // padded row: conflict-free b128 fragment reads
  for (int i = tid; i < Kp * (D / 4); i += VQ_BLOCK) {
    const int k = i / (D / 4), qd = i - k * (D / 4);
    *reinterpret_cast<float4 *>(cb + (size_t)k * LDD + qd * 4) =
        k < K ? *reinterpret_cast<const float4 *>(codes + (size_t)k * D + qd * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// The signatures below are the ones under which vq_nearest_kernel's instruction stream is the same, instruction for
// instruction, as with the text written out in the kernel (scalars by value, the accumulator by reference: a float4 by
// value or an array filled through a reference reorders the caller's IR and with it the schedule).

// quad `quad` of z_n (zeros for a lane beyond N).  A lane holds quad 2 j + half in zq[j]
__device__ __forceinline__ float4 vq_load_quad_f32(const float *__restrict__ z, int64_t n, bool valid, int quad, int D) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (valid) v = *reinterpret_cast<const float4 *>(z + n * D + quad * 4);
  return v;
}
// a quad's term of |z|^2.  x2 = (sum over the lane's quads, j ascending, starting from 0) + the partner's sum
// (__shfl_xor(.., 32)): that order is part of the distance's definition
__device__ __forceinline__ float vq_quad_norm2_f32(float x, float y, float z, float w) { return x * x + y * y + z * z + w * w; }

// acc += z.e_k of a tile's 32 codes: register r is code kt + mfma_row(r, half) of this lane's vector;
// arow = cb + (kt + col) * (D + 4) + half * 4, the lane's code row and its half of each k-pair of quads
template <int D>
__device__ __forceinline__ void vq_tile_dots_f32(f32x16 &acc, const float *arow, const float4 (&zq)[D / 8]) {
#pragma unroll
  for (int j = 0; j < D / 8; ++j) {
    const float4 a = *reinterpret_cast<const float4 *>(arow + j * 8);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, zq[j].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, zq[j].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, zq[j].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, zq[j].w, acc, 0, 0, 0);
  }
}

// the distance from its three terms, in the reference's association
__device__ __forceinline__ float vq_distance_f32(float x2, float dot, float e2k) { return (x2 - 2.f * dot) + e2k; }

}  // namespace isi
