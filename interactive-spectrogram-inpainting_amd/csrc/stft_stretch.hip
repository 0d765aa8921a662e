// Re-timing of an STFT along a list of source positions with identity phase locking (gfx950): the step between
// isi_spec_to_stft_f32 / the analysis STFT and the inverse that turns them into a time stretch or, with the resampler, a
// transposition.  A phase vocoder that advances every bin on its own loses the phase relations across the bins of a
// partial (an attack smears, partials cancel); here every bin follows the nearest spectral peak of its source frame and
// keeps the source's phase difference to it.
//
// Source, per (b, t, j), j = DFT bin j + 1 of n_fft = 2F:  P = fl(fl(re re) + fl(im im)) (no FMA: the peak decisions are
// exact properties of the float32 data), A = sqrt(P), phi = atan2(im, re), Omega_j = 2 pi ((j + 1) hop mod n_fft) / n_fft,
// dev[t] = wrap(phi[t+1] - phi[t] - Omega_j) for t <= T - 2, wrap = principal value in (-pi, pi].
//   peak:  P > 0, and for d = 1, 2: P[j] > P[j-d] and P[j] >= P[j+d] (neighbours outside [0, F) do not object)
//   near[t, j] = the peak nearest to j, the lower one on a tie; j itself in a frame without a peak
// Output frame u at p = pos[u] clamped to [0, T-1] (NaN: 0), t = min(floor p, T - 2), f = p - t, ta = f < 0.5 ? t : t + 1:
//   M[j] = (1 - f) A[t,j] + f A[t+1,j]       D[j] = Omega_j + ((1 - f) dev[max(t-1,0), j] + f dev[t, j])
//   u == 0:  Phi[j] = phi[t,j] + f (Omegafull_j + dev[t,j]), Omegafull_j = 2 pi (j + 1) hop / n_fft
//   u > 0:   n = near[ta, j];  Phi[j] = wrap((Phi'[n] + D[n]) + (phi[ta,j] - phi[ta,n])), Phi' = the frame before
//   out = M (cos Phi | sin Phi)
// The leading copy run: c = the largest count with pos[0] an integer in [0, T-1] and pos[u] == pos[0] + u <= T - 1 for
// every u < c; those frames are the source's two floats bit for bit and Phi of frame c - 1 is that frame's phi.
//
// Form.  stretch_prepare_kernel, one workgroup per source frame, writes A, phi, dev and near to the workspace: every
// source frame is used by 1 / rate output frames, the arc tangents and the peak search are paid once, and nothing in it
// depends on another frame.  `near` is two scans over the frame's peak flags in LDS (last peak at or below j, first peak
// at or above j), log2 F steps each.  stretch_kernel is the recursion: Phi of a whole frame is needed before any bin of
// the next one (peaks drift across bins, so a bin's chain visits other bins), hence one workgroup per batch item with a
// barrier per output frame.  A lane owns bin j (and j + 1024 above F = 1024) and keeps its Phi in a register; per frame it
// leaves Phi' + D and phi[ta] in LDS, waits, and gathers both at its peak.  The LDS rows are double-buffered, so one
// barrier per frame suffices (a lane can be at most one frame ahead of the slowest).  What a frame reads from the
// workspace does not depend on the chain: its position and its six values are loaded two frames ahead (two dependent reads).
#include <climits>
#include <cmath>

#include "isi_common.h"
#include "isi_internal.h"

namespace isi {

namespace {

constexpr float PI_F = 3.14159265358979323846f;
constexpr float TWO_PI_F = 6.28318530717958647692f;
constexpr int kMaxF = ISI_STFT_STRETCH_MAX_F;
constexpr int kPrepBlock = 256;
constexpr int kPrepPer = kMaxF / kPrepBlock;     // bins per lane of the preparation pass
constexpr int kBlock = 1024;
constexpr int kPer = kMaxF / kBlock;             // bins per lane of the recursion
constexpr int kNoPeak = INT_MAX / 2;

static_assert(kMaxF % kBlock == 0 && kMaxF % kPrepBlock == 0, "the bin loops assume whole strides");

// principal value in (-pi, pi]
__device__ __forceinline__ float wrap_pi(float d) { return d - TWO_PI_F * ceilf((d - PI_F) / TWO_PI_F); }

// 2 pi m / n_fft, m an integer below 2^24 n_fft
__device__ __forceinline__ float turn_fraction(int64_t m, int n_fft) { return TWO_PI_F * ((float)m / (float)n_fft); }

__device__ __forceinline__ float omega_of(int j, int hop, int n_fft) {
  return turn_fraction(((int64_t)(j + 1) * hop) % n_fft, n_fft);
}

__global__ __launch_bounds__(kPrepBlock) void stretch_prepare_kernel(const float *__restrict__ X, float *__restrict__ A,
                                                                     float *__restrict__ PHI, float *__restrict__ DEV,
                                                                     int *__restrict__ NEAR, const int T, const int F,
                                                                     const int hop) {
  __shared__ float sP[kMaxF];
  __shared__ int sLo[kMaxF], sHi[kMaxF];
  const int64_t frame = blockIdx.x;
  const int t = (int)(frame % T), tid = threadIdx.x, n_fft = 2 * F;
  const bool has_next = t + 1 < T;
  const float *x0 = X + frame * 2 * F, *x1 = x0 + (has_next ? 2 * (int64_t)F : 0);
  float *a = A + frame * F, *phi = PHI + frame * F, *dev = DEV + frame * F;
  int *near = NEAR + frame * F;

  for (int j = tid; j < F; j += kPrepBlock) {
    const float re = x0[j], im = x0[F + j], re1 = x1[j], im1 = x1[F + j];
    const float P = __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im));
    const float ph = atan2f(im, re);
    sP[j] = P;
    a[j] = sqrtf(P);
    phi[j] = ph;
    dev[j] = has_next ? wrap_pi((atan2f(im1, re1) - ph) - omega_of(j, hop, n_fft)) : 0.f;
  }
  __syncthreads();
  for (int j = tid; j < F; j += kPrepBlock) {
    const float P = sP[j];
    bool peak = P > 0.f;
#pragma unroll
    for (int d = 1; d <= 2; ++d) {
      if (j - d >= 0) peak = peak && P > sP[j - d];
      if (j + d < F) peak = peak && P >= sP[j + d];
    }
    sLo[j] = peak ? j : -1;
    sHi[j] = peak ? j : kNoPeak;
  }
  __syncthreads();
  // sLo[j] <- the last peak at or below j (-1: none), sHi[j] <- the first peak at or above j (kNoPeak: none)
  for (int s = 1; s < F; s <<= 1) {
    int lo[kPrepPer], hi[kPrepPer];
#pragma unroll
    for (int k = 0; k < kPrepPer; ++k) {
      const int j = tid + k * kPrepBlock;
      if (j < F) {
        lo[k] = max(sLo[j], j >= s ? sLo[j - s] : -1);
        hi[k] = min(sHi[j], j + s < F ? sHi[j + s] : kNoPeak);
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPrepPer; ++k) {
      const int j = tid + k * kPrepBlock;
      if (j < F) {
        sLo[j] = lo[k];
        sHi[j] = hi[k];
      }
    }
    __syncthreads();
  }
  for (int j = tid; j < F; j += kPrepBlock) {
    const int lo = sLo[j], hi = sHi[j];
    int n = j;
    if (lo >= 0 && hi < kNoPeak) n = (j - lo <= hi - j) ? lo : hi;
    else if (lo >= 0) n = lo;
    else if (hi < kNoPeak) n = hi;
    near[j] = n;
  }
}

// where output frame u reads: p clamped, t <= T - 2, so that t + 1, ta and tm = max(t - 1, 0) are frames of the source
struct Where {
  int t, tm, ta;
  float f;
};

__device__ __forceinline__ Where where_of(float p, int T) {
  if (!(p >= 0.f)) p = 0.f;                       // NaN too
  const float last = (float)(T - 1);              // exact: T <= 2^24
  if (p > last) p = last;
  Where w;
  w.t = min((int)floorf(p), T - 2);
  w.f = p - (float)w.t;                           // exact
  w.tm = max(w.t - 1, 0);
  w.ta = w.f < 0.5f ? w.t : w.t + 1;
  return w;
}

template <int PER>
struct Loaded {                                   // what a lane reads from the workspace for one output frame
  float f;
  float a0[PER], a1[PER], d0[PER], d1[PER], ph[PER];
  int n[PER];
};

template <int PER>
__device__ __forceinline__ void load_frame(Loaded<PER> &v, const float p, const float *__restrict__ A,
                                           const float *__restrict__ PHI, const float *__restrict__ DEV,
                                           const int *__restrict__ NEAR, int T, int F) {
  const Where w = where_of(p, T);
  v.f = w.f;
  const int64_t r0 = (int64_t)w.t * F, r1 = r0 + F, rm = (int64_t)w.tm * F, ra = (int64_t)w.ta * F;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int j = min((int)(threadIdx.x + k * blockDim.x), F - 1);      // lanes past F repeat the last bin, write nothing
    v.a0[k] = A[r0 + j];
    v.a1[k] = A[r1 + j];
    v.d0[k] = DEV[rm + j];
    v.d1[k] = DEV[r0 + j];
    v.ph[k] = PHI[ra + j];
    v.n[k] = NEAR[ra + j];
  }
}

// PER bins per lane: 1 up to F = 1024 (the workgroup is then F rounded up to whole waves), 2 above
template <int PER>
__global__ __launch_bounds__(kBlock) void stretch_kernel(const float *__restrict__ X, const float *__restrict__ pos,
                                                         const int64_t pos_bstride, const float *__restrict__ A,
                                                         const float *__restrict__ PHI, const float *__restrict__ DEV,
                                                         const int *__restrict__ NEAR, float *__restrict__ out, const int T,
                                                         const int T_out, const int F, const int hop) {
  __shared__ float sC[2][kMaxF], sPh[2][kMaxF];
  __shared__ int sCopy;
  const int64_t b = blockIdx.x, F2 = 2 * (int64_t)F;
  const int tid = threadIdx.x, nt = blockDim.x, n_fft = 2 * F;
  pos += b * pos_bstride;
  X += b * T * F2;
  out += b * T_out * F2;
  A += b * T * F;
  PHI += b * T * F;
  DEV += b * T * F;
  NEAR += b * T * F;

  // the leading copy run
  if (tid == 0) sCopy = T_out;
  __syncthreads();
  const float p0 = pos[0];
  const bool whole = p0 >= 0.f && p0 <= (float)(T - 1) && p0 == floorf(p0);
  for (int u = tid; u < T_out; u += nt) {
    const float p = pos[u];
    if (!(whole && (double)p == (double)p0 + (double)u && p <= (float)(T - 1))) atomicMin(&sCopy, u);
  }
  __syncthreads();
  const int copy = sCopy;
  for (int u = 0; u < copy; ++u) {
    const float *src = X + ((int64_t)p0 + u) * F2;
    float *dst = out + u * F2;
    for (int j = tid; j < 2 * F; j += nt) dst[j] = src[j];
  }

  float Phi[PER], omega[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) omega[k] = omega_of(min(tid + k * nt, F - 1), hop, n_fft);
  int u0;
  if (copy > 0) {
    const int64_t row = ((int64_t)p0 + copy - 1) * F;
#pragma unroll
    for (int k = 0; k < PER; ++k) Phi[k] = PHI[row + min(tid + k * nt, F - 1)];
    u0 = copy;
  } else {                                        // frame 0 starts the chain from the source's own phase
    const Where w = where_of(p0, T);
    const float g = 1.f - w.f;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int j = tid + k * nt, jc = min(j, F - 1);
      const int64_t r0 = (int64_t)w.t * F + jc;
      const float full = turn_fraction((int64_t)(jc + 1) * hop, n_fft);
      Phi[k] = PHI[r0] + w.f * (full + DEV[r0]);
      const float M = g * A[r0] + w.f * A[r0 + F];
      float s, c;
      sincosf(Phi[k], &s, &c);
      if (j < F) {
        out[j] = M * c;
        out[F + j] = M * s;
      }
    }
    u0 = 1;
  }
  if (u0 >= T_out) return;

  Loaded<PER> cur, nxt, nxt2;
  load_frame(cur, pos[u0], A, PHI, DEV, NEAR, T, F);
  if (u0 + 1 < T_out) load_frame(nxt, pos[u0 + 1], A, PHI, DEV, NEAR, T, F);
  for (int u = u0; u < T_out; ++u) {
    if (u + 2 < T_out) load_frame(nxt2, pos[u + 2], A, PHI, DEV, NEAR, T, F);
    const int buf = u & 1;
    const float f = cur.f, g = 1.f - cur.f;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int j = tid + k * nt;
      if (j < F) {
        sC[buf][j] = Phi[k] + (omega[k] + (g * cur.d0[k] + f * cur.d1[k]));
        sPh[buf][j] = cur.ph[k];
      }
    }
    __syncthreads();
    float *dst = out + u * F2;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int j = tid + k * nt, n = cur.n[k];
      if (j < F) {
        Phi[k] = wrap_pi(sC[buf][n] + (cur.ph[k] - sPh[buf][n]));
        const float M = g * cur.a0[k] + f * cur.a1[k];
        float s, c;
        sincosf(Phi[k], &s, &c);
        dst[j] = M * c;
        dst[F + j] = M * s;
      }
    }
    cur = nxt;
    nxt = nxt2;
  }
}

}  // namespace

size_t stft_stretch_workspace_bytes(int B, int T, int F) {
  if (B < 1 || T < 2 || F < 1 || F > kMaxF || (__int128)B * T * F > ((__int128)1 << 30) - 4) return 0;
  return (size_t)4 * B * T * F * sizeof(float);
}

int stft_stretch_f32(const float *X, const float *pos, int pos_batch, float *out, void *workspace, size_t workspace_bytes,
                     int B, int T, int T_out, int F, int hop, hipStream_t st) {
  if (!X || !pos || !out || !workspace) return invalid("stft_stretch: null pointer");
  if (B < 1 || F < 1 || T_out < 1) return invalid("stft_stretch: B, F and T_out must be at least 1");
  if (T < 2) return invalid("stft_stretch: T must be at least 2 (a phase advance needs two frames)");
  if (pos_batch != 1 && pos_batch != B) return invalid("stft_stretch: pos_batch must be 1 or B");
  if (hop < 1 || (2 * (int64_t)F) % hop) return invalid("stft_stretch: hop must be positive and divide n_fft = 2 F");
  if (reinterpret_cast<uintptr_t>(workspace) & 3) return invalid("stft_stretch: workspace must be aligned to a float");
  if (F > kMaxF) return unsupported("stft_stretch: F above ISI_STFT_STRETCH_MAX_F");
  // positions are float32 frame numbers: T - 1 must be one; spans are what the 64-bit offsets and the grid are checked for
  const __int128 lim = ((__int128)1 << 30) - 4;
  if (T > (1 << 24) || (__int128)B * T * 2 * F > lim || (__int128)B * T_out * 2 * F > lim || (__int128)B * T_out > lim)
    return unsupported("stft_stretch: T must stay at or below 2^24 and every array below 2^30 - 4 elements");
  const size_t need = stft_stretch_workspace_bytes(B, T, F);
  if (workspace_bytes < need) {
    char buf[160];
    snprintf(buf, sizeof buf, "stft_stretch: workspace_bytes %zu < %zu (isi_stft_stretch_workspace_bytes)", workspace_bytes, need);
    set_last_error(buf);
    return ISI_E_WORKSPACE;
  }
  const int64_t plane = (int64_t)B * T * F;
  float *A = static_cast<float *>(workspace), *PHI = A + plane, *DEV = PHI + plane;
  int *NEAR = reinterpret_cast<int *>(DEV + plane);
  hipLaunchKernelGGL(stretch_prepare_kernel, dim3((unsigned)(B * (int64_t)T)), dim3(kPrepBlock), 0, st, X, A, PHI, DEV, NEAR, T, F,
                     hop);
  const int rc = check_launch("stft_stretch (preparation)");
  if (rc != ISI_OK) return rc;
  const int block = min(kBlock, (F + 63) / 64 * 64);
  const int64_t pos_bstride = pos_batch == 1 ? 0 : T_out;
  if (F <= kBlock)
    hipLaunchKernelGGL(stretch_kernel<1>, dim3(B), dim3(block), 0, st, X, pos, pos_bstride, A, PHI, DEV, NEAR, out, T, T_out, F, hop);
  else
    hipLaunchKernelGGL(stretch_kernel<kPer>, dim3(B), dim3(block), 0, st, X, pos, pos_bstride, A, PHI, DEV, NEAR, out, T, T_out, F,
                       hop);
  return check_launch("stft_stretch");
}

}  // namespace isi
