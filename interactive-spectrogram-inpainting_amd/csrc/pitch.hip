// Pitch of an uploaded sound (gfx950): the difference function of YIN (de Cheveigne & Kawahara 2002) per analysis frame
// in direct form, and the per-frame choice of the period.  Specification: tests/pitch_spec.py.
//
//   T = (L - W - tau_max) / hop + 1 frames, frame t starts at s = t hop
//   d[t][tau] = sum_{j < W} (x[s + j] - x[s + j + tau])^2,  tau = 0 .. tau_max          e[t] = sum_{j < W} x[s + j]^2
//   cs(tau) = sum_{k = 1 .. tau} d(k),  d'(0) = 1,  d'(tau) = d(tau) tau / cs(tau)  (1 where cs = 0)
//   tau* = the first tau in [tau_min, tau_max) with d'(tau) < threshold, then tau -> tau + 1 while tau + 1 < tau_max and
//          d'(tau + 1) < d'(tau); with no lag under the threshold the argmin of d' over [tau_min, tau_max), lowest on ties
//   period = tau* + (a - c) / (2 (a - 2 b + c)) on the raw a, b, c = d(tau* - 1), d(tau*), d(tau* + 1) when a - 2 b + c > 0
//
// WHY THE DIRECT FORM: E_a + E_tau - 2 corr on the matrix pipe loses 2^-24 E / d relative accuracy in the subtraction, and
// at the dip -- the only place the choice looks at -- d is orders of magnitude below the frame energy E.  The direct sum
// has non-negative terms only: relatively accurate at every lag.  Each term is one subtraction (rounded to fp32) and one
// fp32 fma into the lag's accumulator, j ascending: the bits of d[t][tau] depend on the frame's samples alone.
//
// DIFFERENCE KERNEL.  A workgroup of 256 threads owns 1024 consecutive lags of one frame and stages the frame's
// W + tau_max samples in LDS (20 KB at W = 3072, tau_max = 1920; float4 loads over the 16-byte aligned interior of the
// row, scalar loads at its ends).  A thread owns FOUR consecutive lags tau0 .. tau0 + 3 (tau0 = 4 * thread) and walks j in
// steps of four: the 16 terms of a step need x[j .. j + 3] (one ds_read_b128, the same address in every lane: a
// broadcast) and x[j + tau0 .. j + tau0 + 6], of which four were read in the step before and the new four are ONE
// ds_read_b128 at 16 bytes per lane, lane stride 16 bytes: conflict-free.  Two 16-byte LDS reads feed 16 subtract + fma
// pairs; the resampler's kernel spends one 4-byte read per fma.  At the defaults a frame is two workgroups (lags 0..1023
// and 1024..1920: 94 % of the lanes carry a lag).  The first of them also sums the frame energy: thread i adds its
// ceil(W / 256) consecutive squares in order, the 256 partial sums are added in a fixed tree.
//
// PICK KERNEL.  One workgroup per frame: d'(tau) through a prefix sum (a thread sums its ceil(n / 256) consecutive lags in
// order, the partial sums go through a 256-wide scan in LDS), a min-reduction on the index for the first lag under the
// threshold and one on (value, index) for the fallback, then one thread walks the descent and evaluates the vertex.
#include <cmath>

#include "isi_common.h"
#include "isi_internal.h"

namespace isi {

namespace {
constexpr int PT_THREADS = 256;
constexpr int PT_LAGS = 4;                                // consecutive lags of one thread
constexpr int PT_CHUNK = PT_THREADS * PT_LAGS;            // lags of one workgroup
constexpr int PT_MAX_STAGE = 15360;                       // W + tau_max floats of one frame: 60 KB of LDS
}  // namespace

__global__ __launch_bounds__(PT_THREADS) void pitch_difference_kernel(const float *__restrict__ x, int64_t x_stride,
                                                                      float *__restrict__ d, float *__restrict__ energy,
                                                                      int T, int W, int hop, int tau_max, int chunks) {
  extern __shared__ __attribute__((aligned(16))) float stage[];   // [round4(W + tau_max) + 4], zeros past W + tau_max
  const int chunk = (int)(blockIdx.x % (unsigned)chunks);
  const int64_t frame = (int64_t)(blockIdx.x / (unsigned)chunks);   // b * T + t
  const int t = (int)(frame % T);
  const int64_t b = frame / T;
  const int tid = (int)threadIdx.x;
  const float *__restrict__ xr = x + b * x_stride + (int64_t)t * hop;   // stage[i] = xr[i]
  const int n = W + tau_max;
  const int n_alloc = ((n + 3) & ~3) + 4;
  // 16-byte aligned interior [va, vb) of [0, n): the row base and the frame start are arbitrary, so the ends go scalar
  const int mis = (int)((reinterpret_cast<uintptr_t>(xr) >> 2) & 3);
  int va = (4 - mis) & 3;
  if (va > n) va = n;
  const int vb = va + ((n - va) & ~3);
  for (int i = tid; i < n_alloc; i += PT_THREADS) {
    if (i >= va && i < vb) continue;
    stage[i] = i < n ? xr[i] : 0.f;
  }
  for (int i = va + 4 * tid; i < vb; i += 4 * PT_THREADS) {
    const float4 v = *reinterpret_cast<const float4 *>(xr + i);
    float *dst = stage + i;                                 // not 16-byte aligned in general: four dword writes
    dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
  }
  __syncthreads();

  const int tau0 = chunk * PT_CHUNK + PT_LAGS * tid;
  if (tau0 <= tau_max) {
    const float4 *__restrict__ s4 = reinterpret_cast<const float4 *>(stage);
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
    float4 w = s4[tau0 >> 2];                               // x[j + tau0 .. j + tau0 + 3]
    const int W4 = W & ~3;
#define PT_TERM(a, v, acc) { const float df = (a) - (v); acc = fmaf(df, df, acc); }
#pragma unroll 4
    for (int j = 0; j < W4; j += 4) {
      const float4 a = s4[j >> 2];
      const float4 nx = s4[((j + tau0) >> 2) + 1];          // x[j + tau0 + 4 .. j + tau0 + 7]; reaches < n_alloc
      PT_TERM(a.x, w.x, acc0) PT_TERM(a.x, w.y, acc1) PT_TERM(a.x, w.z, acc2) PT_TERM(a.x, w.w, acc3)
      PT_TERM(a.y, w.y, acc0) PT_TERM(a.y, w.z, acc1) PT_TERM(a.y, w.w, acc2) PT_TERM(a.y, nx.x, acc3)
      PT_TERM(a.z, w.z, acc0) PT_TERM(a.z, w.w, acc1) PT_TERM(a.z, nx.x, acc2) PT_TERM(a.z, nx.y, acc3)
      PT_TERM(a.w, w.w, acc0) PT_TERM(a.w, nx.x, acc1) PT_TERM(a.w, nx.y, acc2) PT_TERM(a.w, nx.z, acc3)
      w = nx;
    }
    for (int j = W4; j < W; ++j) {                          // W % 4 last samples
      const float a = stage[j];
      const float *v = stage + j + tau0;                    // v[3] <= stage[W - 1 + tau_max + 3] < n_alloc
      PT_TERM(a, v[0], acc0) PT_TERM(a, v[1], acc1) PT_TERM(a, v[2], acc2) PT_TERM(a, v[3], acc3)
    }
#undef PT_TERM
    float *__restrict__ dr = d + frame * ((int64_t)tau_max + 1) + tau0;
    dr[0] = acc0;
    if (tau0 + 1 <= tau_max) dr[1] = acc1;
    if (tau0 + 2 <= tau_max) dr[2] = acc2;
    if (tau0 + 3 <= tau_max) dr[3] = acc3;
  }

  if (chunk == 0) {                                         // the frame energy: consecutive runs in order, then a fixed tree
    const int per = (W + PT_THREADS - 1) / PT_THREADS;
    const int j0 = tid * per, j1 = j0 + per < W ? j0 + per : W;
    float e = 0.f;
    for (int j = j0; j < j1; ++j) e = fmaf(stage[j], stage[j], e);
    __syncthreads();                                        // every thread of the workgroup is done reading the samples
    stage[tid] = e;                                         // n_alloc >= 256 is not given: see the launcher's LDS size
    __syncthreads();
    for (int step = PT_THREADS / 2; step > 0; step >>= 1) {
      if (tid < step) stage[tid] += stage[tid + step];
      __syncthreads();
    }
    if (tid == 0) energy[frame] = stage[0];
  }
}

__global__ __launch_bounds__(PT_THREADS) void pitch_pick_kernel(const float *__restrict__ d, int tau_min, int tau_max,
                                                                float threshold, float *__restrict__ period,
                                                                float *__restrict__ aperiodicity) {
  extern __shared__ __attribute__((aligned(16))) float dp[];    // [n]: d, then d' in place
  __shared__ float part[2][PT_THREADS];
  __shared__ float best_v[PT_THREADS];
  __shared__ int best_i[PT_THREADS], first_i[PT_THREADS];
  const int n = tau_max + 1, tid = (int)threadIdx.x;
  const float *__restrict__ dr = d + (int64_t)blockIdx.x * n;
  for (int i = tid; i < n; i += PT_THREADS) dp[i] = dr[i];
  __syncthreads();
  const int per = (n + PT_THREADS - 1) / PT_THREADS;
  const int k0 = tid * per < n ? tid * per : n, k1 = k0 + per < n ? k0 + per : n;
  float s = 0.f;
  for (int k = k0 > 1 ? k0 : 1; k < k1; ++k) s += dp[k];          // d(0) is no part of the cumulative sum
  part[0][tid] = s;
  __syncthreads();
  int cur = 0;
  for (int step = 1; step < PT_THREADS; step <<= 1) {             // inclusive scan of the 256 partial sums
    part[cur ^ 1][tid] = tid >= step ? part[cur][tid - step] + part[cur][tid] : part[cur][tid];
    cur ^= 1;
    __syncthreads();
  }
  float cs = tid ? part[cur][tid - 1] : 0.f;
  int first = 0x7fffffff, arg = 0x7fffffff;
  float low = INFINITY;
  for (int k = k0; k < k1; ++k) {
    float v = 1.f;
    if (k >= 1) {
      cs += dp[k];
      if (cs > 0.f) v = dp[k] * (float)k / cs;
    }
    dp[k] = v;
    if (k >= tau_min && k < tau_max) {
      if (v < threshold && first == 0x7fffffff) first = k;
      if (v < low) { low = v; arg = k; }                          // k ascends: the lowest tau on ties
    }
  }
  first_i[tid] = first;
  best_v[tid] = low;
  best_i[tid] = arg;
  __syncthreads();
  for (int step = PT_THREADS / 2; step > 0; step >>= 1) {
    if (tid < step) {
      const int f2 = first_i[tid + step];
      if (f2 < first_i[tid]) first_i[tid] = f2;
      const float v2 = best_v[tid + step];
      const int i2 = best_i[tid + step];
      if (v2 < best_v[tid] || (v2 == best_v[tid] && i2 < best_i[tid])) { best_v[tid] = v2; best_i[tid] = i2; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    int tau = first_i[0];
    if (tau == 0x7fffffff) {
      tau = best_i[0] == 0x7fffffff ? tau_min : best_i[0];        // (every d' a NaN: no lag compared below +inf)
    } else {
      while (tau + 1 < tau_max && dp[tau + 1] < dp[tau]) ++tau;
    }
    const float a = dr[tau - 1], bq = dr[tau], c = dr[tau + 1];   // tau_min >= 1 and tau < tau_max: inside the row
    const float v = (a - 2.f * bq) + c;
    float p = (float)tau;
    if (v > 0.f) p += (a - c) / (2.f * v);
    period[blockIdx.x] = p;
    aperiodicity[blockIdx.x] = dp[tau];
  }
}

int64_t pitch_frames(int64_t L, int W, int hop, int tau_max) {
  if (W <= 0 || hop <= 0 || tau_max < 0 || L < (int64_t)W + tau_max) return ISI_E_INVALID;
  return (L - W - tau_max) / hop + 1;
}

int pitch_difference_f32(const float *x, int64_t x_stride, float *d, float *energy, int B, int64_t L, int W, int hop,
                         int tau_max, hipStream_t st) {
  if (!x || !d || !energy) return invalid("pitch_difference: null pointer");
  if (B <= 0 || L <= 0 || W <= 0 || hop <= 0) return invalid("pitch_difference: non-positive size");
  if (tau_max < 3) return invalid("pitch_difference: tau_max below 3 (tau_min + 2 at the least tau_min, 1)");
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(energy)) & 3)
    return invalid("pitch_difference: pointers must be aligned to a float");
  if ((int64_t)W + tau_max > PT_MAX_STAGE)
    return unsupported("pitch_difference: W + tau_max beyond the 15360 floats of one frame's LDS stage");
  if (L < (int64_t)W + tau_max) return invalid("pitch_difference: L shorter than one frame, W + tau_max samples");
  if (x_stride < L) return invalid("pitch_difference: a row stride shorter than the row");
  if (L >= ((int64_t)1 << 31)) return unsupported("pitch_difference: rows of 2^31 samples or more");
  const int64_t T = pitch_frames(L, W, hop, tau_max);
  const int chunks = (tau_max + PT_CHUNK) / PT_CHUNK;       // ceil((tau_max + 1) / 1024)
  if (T * B * chunks >= ((int64_t)1 << 31)) return unsupported("pitch_difference: more than 2^31 workgroups");
  int n_alloc = ((W + tau_max + 3) & ~3) + 4;
  if (n_alloc < PT_THREADS) n_alloc = PT_THREADS;           // the energy tree reuses the stage
  hipLaunchKernelGGL(pitch_difference_kernel, dim3((unsigned)(T * B * chunks)), dim3(PT_THREADS),
                     (size_t)n_alloc * sizeof(float), st, x, x_stride, d, energy, (int)T, W, hop, tau_max, chunks);
  return check_launch("pitch_difference");
}

int pitch_pick_f32(const float *d, int64_t n_frames, int tau_min, int tau_max, float threshold, float *period,
                   float *aperiodicity, hipStream_t st) {
  if (!d || !period || !aperiodicity) return invalid("pitch_pick: null pointer");
  if (n_frames <= 0) return invalid("pitch_pick: non-positive number of frames");
  if (tau_min < 1) return invalid("pitch_pick: tau_min below 1");
  if ((int64_t)tau_max < (int64_t)tau_min + 2) return invalid("pitch_pick: tau_max below tau_min + 2");
  if (!(threshold > 0.f && threshold <= 1.f)) return invalid("pitch_pick: threshold is NaN or outside (0, 1]");
  if ((reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(period) | reinterpret_cast<uintptr_t>(aperiodicity)) & 3)
    return invalid("pitch_pick: pointers must be aligned to a float");
  if (tau_max >= PT_MAX_STAGE) return unsupported("pitch_pick: tau_max beyond the 15360 floats of one frame's LDS stage");
  if (n_frames >= ((int64_t)1 << 31)) return unsupported("pitch_pick: 2^31 frames or more");
  hipLaunchKernelGGL(pitch_pick_kernel, dim3((unsigned)n_frames), dim3(PT_THREADS), (size_t)(tau_max + 1) * sizeof(float),
                     st, d, tau_min, tau_max, threshold, period, aperiodicity);
  return check_launch("pitch_pick");
}

}  // namespace isi
