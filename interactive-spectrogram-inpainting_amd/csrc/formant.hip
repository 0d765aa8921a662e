// Formant correction of STFT frames by the true envelope (gfx950): the step that lets `transpose` and `bend` move a sound's
// pitch and leave its resonances where they were.  Both move the pitch by reading the sound faster or slower, so a
// component at f in the stretched sound ends at rho f; it should carry the spectral envelope's value there.  Every frame
// is multiplied, bin by bin, by exp(V(rho k) - V(k)), V the frame's true envelope (Roebel & Rodet 2005: cepstral smoothing
// iterated on max(log spectrum, previous envelope), so that the envelope rests on the partials' peaks instead of running
// through the valleys between them).  Specification: tests/formant_spec.py; DESIGN.md section 6j.
//
// Per frame (b, t) of Y [B,T,2F] (real block | imaginary block, bin j = DFT bin k = j + 1 of n_fft = 2F):
//   P_j = fl(fl(re re) + fl(im im)) (no FMA), Pmax = max_j P_j, NaN if any P_j is;  rho = ratio clamped to [1/4, 4]
//   the frame is copied bit for bit unless 0 < Pmax < +inf, and when the ratio is NaN or rho == 1
//   L_j = max(1/2 ln P_j, 1/2 ln Pmax - depth);  Lx_0 = L_0, Lx_k = L_{k-1} on k = 0 .. F
//   S(A):  c_q = (1 / 2F) [A_0 + (-1)^q A_F + 2 sum_{0<k<F} A_k cos(pi q k / F)], q < n;  w_q = (1 + cos(pi q / n)) / 2
//          V_k = w_0 c_0 + 2 sum_{0<q<n} w_q c_q cos(pi q k / F)
//   A = Lx;  I times: V = S(A), A = max(Lx, V)
//   x = min(fl(rho k), F), i = min(floor x, F - 1), f = x - i, V_x = (1 - f) V_i + f V_{i+1}
//   out_j = exp(clamp(V_x - V_k, -max_gain, +max_gain)) (re_j, im_j)
//
// Form.  One workgroup of 512 lanes per frame; Lx, A, V, the 2F cosines and the n liftered coefficients stay in LDS for all
// I iterations (43.6 KB at F = 2048), nothing goes to HBM between them.  cos(pi q k / F) = table[(q k) mod 2F]: the index
// advances by a constant step mod 2F, no multiplication or division in the loops.
//   forward:  a wave owns q, its lanes stride over k (64 apart) with one fma chain each, then a butterfly sum over the lanes;
//             d_q = (m_q w_q / 2F) sum, m_0 = 1, m_q = 2 (the factor is made in double, rounded once)
//   inverse:  a lane owns k and runs q = 0 .. n - 1 in one fma chain; d_q is a broadcast read
// Both walk the table at a lane stride of q.  Unskewed, an odd q visits all 32 banks of a 32-lane group and an even q with
// 2^s | q only 32 / 2^s of them (q = 32: every lane on bank 0 with its own address).  The table is stored skewed, entry i at
// i + (i >> 5): a stride of 32 becomes 33 and no stride is worse than two-way, at the price of two-way conflicts on some
// banks for the odd strides that were free.  Measured: 37 - 39 % of the LDS cycles are conflict cycles; what was tried
// against it, and why the loops are not bound by LDS in the first place, is in DESIGN.md section 6j.
#include <cmath>

#include "isi_common.h"
#include "isi_internal.h"

namespace isi {

namespace {

constexpr int kMaxF = ISI_STFT_STRETCH_MAX_F;
constexpr int kMaxOrder = ISI_FORMANT_MAX_ORDER;
constexpr int kBlock = 512;
constexpr int kWaves = kBlock / 64;
constexpr int kTable = 2 * kMaxF + 2 * kMaxF / 32;      // the skewed table

__device__ __forceinline__ int skew(int i) { return i + (i >> 5); }

__global__ __launch_bounds__(kBlock) void formant_kernel(const float *__restrict__ Y, const float *__restrict__ ratio,
                                                         const int64_t ratio_bstride, const float *__restrict__ cos_table,
                                                         float *__restrict__ out, float *__restrict__ env, const int T,
                                                         const int F, const int order, const int iterations,
                                                         const float depth, const float max_gain) {
  __shared__ float sLx[kMaxF + 1], sA[kMaxF + 1], sV[kMaxF + 1];
  __shared__ float sCos[kTable];
  __shared__ float sD[kMaxOrder], sW[kMaxOrder];
  __shared__ float sMax[kWaves];
  __shared__ int sBad[kWaves];
  const int64_t frame = blockIdx.x;
  const int b = (int)(frame / T), t = (int)(frame % T);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n2 = 2 * F;
  const float *__restrict__ y = Y + frame * n2;
  float *__restrict__ o = out + frame * n2;
  float *__restrict__ e = env ? env + frame * (F + 1) : nullptr;

  const float r = ratio[(int64_t)b * ratio_bstride + t];
  const float rho = fminf(fmaxf(r, 0.25f), 4.f);
  const bool unit = !(r == r) || rho == 1.f;            // a NaN counts as 1

  // power, its maximum (NaN if any bin's is)
  float pm = 0.f;
  int bad = 0;
  for (int j = tid; j < F; j += kBlock) {
    const float re = y[j], im = y[F + j];
    const float P = __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im));
    sLx[j + 1] = P;
    bad |= !(P == P);
    pm = fmaxf(pm, P);
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    pm = fmaxf(pm, __shfl_xor(pm, s));
    bad |= __shfl_xor(bad, s);
  }
  if (lane == 0) {
    sMax[wave] = pm;
    sBad[wave] = bad;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    pm = fmaxf(pm, sMax[w]);
    bad |= sBad[w];
  }
  const bool ok = !bad && pm > 0.f && pm < INFINITY;

  if (!ok || unit) {                                    // uniform over the workgroup
    for (int j = tid; j < n2; j += kBlock) o[j] = y[j];
    if (!ok) {
      if (e)
        for (int k = tid; k <= F; k += kBlock) e[k] = 0.f;
      return;
    }
    if (!e) return;
  }

  const float floor_l = 0.5f * logf(pm) - depth;
  for (int j = tid; j < F; j += kBlock) {               // the lane that wrote P_j
    const float l = fmaxf(0.5f * logf(sLx[j + 1]), floor_l);
    sLx[j + 1] = l;
    sA[j + 1] = l;
    if (j == 0) {
      sLx[0] = l;
      sA[0] = l;
    }
  }
  for (int i = tid; i < n2; i += kBlock) sCos[skew(i)] = cos_table[i];
  for (int q = tid; q < order; q += kBlock) {
    const double w = 0.5 + 0.5 * cos(3.14159265358979323846 * (double)q / (double)order);
    sW[q] = (float)((q == 0 ? 1.0 : 2.0) * w / (double)n2);
  }

  for (int it = 0; it < iterations; ++it) {
    __syncthreads();
    for (int q = wave; q < order; q += kWaves) {
      const int step = (64 * q) % n2;
      int idx = (q * lane) % n2;
      float acc = 0.f;
      for (int k = lane; k <= F; k += 64) {
        float a = sA[k];
        if (k != 0 && k != F) a += a;
        acc = fmaf(a, sCos[skew(idx)], acc);
        idx += step;
        if (idx >= n2) idx -= n2;
      }
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor(acc, s);
      if (lane == 0) sD[q] = acc * sW[q];
    }
    __syncthreads();
    const bool last = it + 1 == iterations;
    for (int k = tid; k <= F; k += kBlock) {
      float v = 0.f;
      int idx = 0;
      for (int q = 0; q < order; ++q) {
        v = fmaf(sD[q], sCos[skew(idx)], v);
        idx += k;
        if (idx >= n2) idx -= n2;
      }
      sV[k] = v;
      if (!last) sA[k] = fmaxf(sLx[k], v);
    }
  }
  __syncthreads();

  if (e)
    for (int k = tid; k <= F; k += kBlock) e[k] = sV[k];
  if (unit) return;
  const float top = (float)F;
  for (int j = tid; j < F; j += kBlock) {
    const int k = j + 1;
    const float x = fminf(__fmul_rn(rho, (float)k), top);       // >= 1/4: truncation is the floor
    const int i = min((int)x, F - 1);
    const float f = x - (float)i;                               // exact
    const float vx = fmaf(f, sV[i + 1], __fmul_rn(1.f - f, sV[i]));
    const float d = fminf(fmaxf(vx - sV[k], -max_gain), max_gain);
    const float g = expf(d);
    o[j] = g * y[j];
    o[F + j] = g * y[F + j];
  }
}

bool overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + nb && pb < pa + na;
}

}  // namespace

int formant_shift_f32(const float *Y, const float *ratio, int ratio_batch, const float *cos_table, float *out, float *env, int B,
                      int T, int F, int order, int iterations, float depth, float max_gain, hipStream_t st) {
  if (!Y || !ratio || !cos_table || !out) return invalid("formant_shift: null pointer");
  if ((reinterpret_cast<uintptr_t>(Y) | reinterpret_cast<uintptr_t>(ratio) | reinterpret_cast<uintptr_t>(cos_table) |
       reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(env)) & 3)
    return invalid("formant_shift: pointers must be aligned to a float");
  if (B < 1 || T < 1 || F < 1) return invalid("formant_shift: B, T and F must be at least 1");
  if (F < 2) return invalid("formant_shift: F must be at least 2 (an envelope needs two coefficients)");
  if (ratio_batch != 1 && ratio_batch != B) return invalid("formant_shift: ratio_batch must be 1 or B");
  if (iterations < 1 || iterations > ISI_FORMANT_MAX_ITERATIONS)
    return invalid("formant_shift: iterations must lie in 1 .. ISI_FORMANT_MAX_ITERATIONS");
  if (!(depth >= 0.f) || !(max_gain >= 0.f) || std::isinf(depth) || std::isinf(max_gain))
    return invalid("formant_shift: depth and max_gain must be finite and not negative");
  if (F > kMaxF) return unsupported("formant_shift: F above ISI_STFT_STRETCH_MAX_F");
  if (order < 2 || order > (F < kMaxOrder ? F : kMaxOrder))
    return invalid("formant_shift: order must lie in 2 .. min(F, ISI_FORMANT_MAX_ORDER)");
  const __int128 lim = ((__int128)1 << 30) - 4;
  if ((__int128)B * T * 2 * F > lim || (__int128)B * T * (F + 1) > lim)
    return unsupported("formant_shift: every array must stay below 2^30 - 4 elements");
  const size_t n = (size_t)B * T * 2 * F * sizeof(float), n_env = (size_t)B * T * (F + 1) * sizeof(float);
  if (overlap(Y, n, out, n) || (env && (overlap(Y, n, env, n_env) || overlap(out, n, env, n_env))))
    return invalid("formant_shift: inputs and outputs must not overlap (out == Y is not supported)");
  hipLaunchKernelGGL(formant_kernel, dim3((unsigned)((int64_t)B * T)), dim3(kBlock), 0, st, Y, ratio,
                     (int64_t)(ratio_batch == 1 ? 0 : T), cos_table, out, env, T, F, order, iterations, depth, max_gain);
  return check_launch("formant_shift");
}

}  // namespace isi
