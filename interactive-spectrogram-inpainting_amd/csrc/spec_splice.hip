// Phase-locked splice of regenerated STFT frames into an original's STFT, and the sample blend behind it (gfx950).
//
// `to_audio` re-synthesises a whole sound from its (log-magnitude, IF) spectrogram; its phases are a running sum of
// the decoded IF started from zero.  For an uploaded sound of which only a region was edited, spec_splice_kernel keeps
// the original's own STFT frames outside the region and, inside it, starts the phase from the original's phase at the
// frame before the region, integrates the decoded IF, and spreads what is then missing at the frame after the region
// over the region as a constant per-bin detune (at most pi / (frames + 1) per frame).  The rules, per (b, k) row:
//
//   run = maximal [t0, t1) with w > 0;  phi_o = angle of the original's bin, psi = the running decoded phase
//   w == 0                         out = the original's two floats, bit for bit
//   both neighbours                c = wrap(phi_o[t1] - phi_o[t0-1] - (psi[t1] - psi[t0-1])) / (t1 - t0 + 1), wrap to (-pi, pi]
//                                  phi[t] = phi_o[t0-1] + (psi[t] - psi[t0-1]) + (t - t0 + 1) c
//   run from frame 0               phi[t] = phi_o[t1] - (psi[t1] - psi[t])
//   run to frame T                 phi[t] = phi_o[t0-1] + (psi[t] - psi[t0-1])
//   whole row                      phi[t] = psi[t]        (w == 1: the bits isi_spec_to_stft_f32 writes)
//   magnitude                      As (isi_spec_to_stft_f32's rule on `a`) where w == 1, else
//                                  exp((1 - w) log Ao + w log As), Ao = |original bin|; 0 when Ao or As is not positive
//   out = mag (cos phi | sin phi)
//
// Layout: F is the unit-stride axis of every array, a lane owns one (b, k) row and kChunk consecutive frames of it, so a
// wave reads and writes whole rows, frame after frame.  A lane's 5 kChunk loads are issued before anything waits.
// The correction of a run needs the run's far end before its first frame can be written: the lane reads the run's
// weights a second time (backwards to t0, forwards to t1, from wherever in the run its chunk starts, kScan frames per
// step) and then the two anchor frames.  The alternative, a first launch that leaves (t0, t1) per frame, would add
// 8 bytes per element written and read again to a kernel that moves 28; the second read of w stays in the caches (w is
// the smallest array and, with w_batch == 1, shared by the batch), and it is what lets the time axis be cut into chunks
// at all: B = 1 at F = 1024 is 16 waves by rows alone, 16 ceil(T / 8) with chunks.
//
// spec_splice_blend_kernel: the representation drops the DC bin, so analysis + synthesis does not return the input;
// outside the edited region the output must be the upload's own samples.  g[n] = share of the squared analysis window
// (periodic Hann, the helper's), over the frames that reach sample n with a non-zero window value, that belongs to
// touched frames; out = orig where g == 0 (bit for bit), else orig + g (ola - orig).
#include <cmath>

#include "isi_common.h"
#include "isi_internal.h"

namespace isi {

namespace {

constexpr float PI_F = 3.14159265358979323846f;
constexpr float TWO_PI_F = 6.28318530717958647692f;
constexpr float SPEC_EPS = 1e-6f;
constexpr int kBlock = 256;
constexpr int kChunk = 8;       // frames per lane
constexpr int kScan = 8;        // weights per step of the scan for a run's ends

// principal value in (-pi, pi]
__device__ __forceinline__ float wrap_pi(float d) { return d - TWO_PI_F * ceilf((d - PI_F) / TWO_PI_F); }

__global__ __launch_bounds__(kBlock) void spec_splice_kernel(const float *__restrict__ xo, const float *__restrict__ a,
                                                             const float *__restrict__ ph, const float *__restrict__ w,
                                                             const int64_t w_bstride, float *__restrict__ out, const int T,
                                                             const int F, const int mel) {
  const int f = blockIdx.x * kBlock + threadIdx.x;
  if (f >= F) return;
  const int64_t b = blockIdx.z, F1 = F, F2 = 2 * (int64_t)F;
  const int ts = blockIdx.y * kChunk;
  const float *xr = xo + b * T * F2 + f;
  const float *ar = a + b * T * F1 + f, *pr = ph + b * T * F1 + f, *wr = w + b * w_bstride + f;
  float *orow = out + b * T * F2 + f;

  float wv[kChunk], re[kChunk], im[kChunk], av[kChunk], pv[kChunk];
#pragma unroll
  for (int i = 0; i < kChunk; ++i) {
    const int64_t t = min(ts + i, T - 1);          // frames past the end repeat the last one and are never written
    wv[i] = wr[t * F1];
    re[i] = xr[t * F2];
    im[i] = xr[t * F2 + F1];
    av[i] = ar[t * F1];
    pv[i] = pr[t * F1];
  }

  int t0 = 0, t1 = 0;                               // the run the lane is in: [t0, t1), known while t < t1
  bool left = false, right = false;
  float phi_a = 0.f, psi_a = 0.f, phi_b = 0.f, psi_b = 0.f, c = 0.f;
#pragma unroll
  for (int i = 0; i < kChunk; ++i) {
    const int t = ts + i;
    if (t >= T) break;
    if (!(wv[i] > 0.f)) {
      orow[t * F2] = re[i];
      orow[t * F2 + F1] = im[i];
      continue;
    }
    if (t >= t1) {                                  // a run the lane has not met: its ends, from the weights
      // kScan weights per step, loaded together before any is looked at: the scan is a chain of dependent cache
      // reads, one per step (frames outside [0, T) repeat the nearest one and are never looked at)
      t0 = t;
      for (bool open = true; open && t0 > 0;) {
        float v[kScan];
#pragma unroll
        for (int u = 0; u < kScan; ++u) v[u] = wr[(int64_t)max(t0 - 1 - u, 0) * F1];
#pragma unroll
        for (int u = 0; u < kScan; ++u) {
          open = open && t0 > 0 && v[u] > 0.f;
          if (open) --t0;
        }
      }
      t1 = t + 1;
      for (bool open = true; open && t1 < T;) {
        float v[kScan];
#pragma unroll
        for (int u = 0; u < kScan; ++u) v[u] = wr[(int64_t)min(t1 + u, T - 1) * F1];
#pragma unroll
        for (int u = 0; u < kScan; ++u) {
          open = open && t1 < T && v[u] > 0.f;
          if (open) ++t1;
        }
      }
      left = t0 >= 1;
      right = t1 <= T - 1;
      if (left) {
        phi_a = atan2f(xr[(int64_t)(t0 - 1) * F2 + F1], xr[(int64_t)(t0 - 1) * F2]);
        psi_a = pr[(int64_t)(t0 - 1) * F1];
      }
      if (right) {
        phi_b = atan2f(xr[(int64_t)t1 * F2 + F1], xr[(int64_t)t1 * F2]);
        psi_b = pr[(int64_t)t1 * F1];
      }
      if (left && right) c = wrap_pi((phi_b - phi_a) - (psi_b - psi_a)) / (float)(t1 - t0 + 1);
    }
    const float psi = pv[i];
    float phi = psi;
    if (left && right) phi = (phi_a + (psi - psi_a)) + (float)(t - t0 + 1) * c;
    else if (left) phi = phi_a + (psi - psi_a);
    else if (right) phi = phi_b - (psi_b - psi);

    float mag = av[i];
    if (mel) mag = expf(0.5f * logf(fmaxf(mag, 0.f) + SPEC_EPS));
    const float wt = wv[i];
    if (wt != 1.f) {
      const float mo = sqrtf(re[i] * re[i] + im[i] * im[i]);
      mag = (mo > 0.f && mag > 0.f) ? expf((1.f - wt) * logf(mo) + wt * logf(mag)) : 0.f;
    }
    float s, cs;
    sincosf(phi, &s, &cs);
    orow[t * F2] = mag * cs;
    orow[t * F2 + F1] = mag * s;
  }
}

__global__ __launch_bounds__(kBlock) void spec_splice_blend_kernel(const float *__restrict__ orig,
                                                                   const float *__restrict__ ola,
                                                                   const uint8_t *__restrict__ touched,
                                                                   float *__restrict__ out, const int Tf, const int n_fft,
                                                                   const int hop, const int64_t L) {
  const int64_t n = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t b = blockIdx.y;
  if (n >= L) return;
  const int64_t pos = n + (n_fft - hop);            // position in the padded signal, as overlap_add_kernel counts it
  int64_t t_hi = pos / hop;
  if (t_hi > Tf - 1) t_hi = Tf - 1;
  const float step = TWO_PI_F / (float)n_fft;
  float num = 0.f, den = 0.f;
  for (int64_t t = t_hi; t >= 0; --t) {
    const int64_t k = pos - t * hop;
    if (k >= n_fft) break;
    const float wk = 0.5f - 0.5f * cosf((float)k * step);   // k == 0: exactly 0, the frame does not reach the sample
    const float w2 = wk * wk;
    den += w2;
    if (touched[b * Tf + t]) num += w2;
  }
  const float o = orig[b * L + n];
  float r = o;
  if (num != 0.f) r = o + (num / den) * (ola[b * L + n] - o);
  out[b * L + n] = r;
}

}  // namespace

int spec_splice_f32(const float *stft_orig, const float *a, const float *ph, const float *w, int w_batch, float *stft_out,
                    int B, int T, int F, int mel, hipStream_t st) {
  if (!stft_orig || !a || !ph || !w || !stft_out) return invalid("spec_splice: null pointer");
  if (B < 1 || T < 1 || F < 1) return invalid("spec_splice: B, T and F must be at least 1");
  if (w_batch != 1 && w_batch != B) return invalid("spec_splice: w_batch must be 1 or B");
  if (mel != 0 && mel != 1) return invalid("spec_splice: mel must be 0 or 1");
  // the launch is (F / 256, T / 8, B) workgroups; element offsets are 64-bit and the largest one is 2 B T F
  const int chunks = (T + kChunk - 1) / kChunk;
  if (B > 65535 || chunks > 65535 || (__int128)B * T * F >= ((__int128)1 << 59))
    return unsupported("spec_splice: B must stay below 65536, T below 524281 and B T F below 2^59");
  hipLaunchKernelGGL(spec_splice_kernel, dim3((F + kBlock - 1) / kBlock, chunks, B), dim3(kBlock), 0, st, stft_orig, a, ph, w,
                     w_batch == 1 ? (int64_t)0 : (int64_t)T * F, stft_out, T, F, mel);
  return check_launch("spec_splice");
}

int spec_splice_blend_f32(const float *audio_orig, const float *audio_ola, const uint8_t *touched, float *audio_out, int B,
                          int T_frames, int n_fft, int hop, int64_t L, hipStream_t st) {
  if (!audio_orig || !audio_ola || !touched || !audio_out) return invalid("spec_splice_blend: null pointer");
  if (B < 1 || T_frames < 1 || L < 1) return invalid("spec_splice_blend: B, T_frames and L must be at least 1");
  if (n_fft < 1 || hop < 1 || n_fft % hop) return invalid("spec_splice_blend: hop must be positive and divide n_fft");
  // the launch is (L / 256, B) workgroups; element offsets are 64-bit and stay below B L < 2^55
  if (B > 65535 || L >= ((int64_t)1 << 39)) return unsupported("spec_splice_blend: B must stay below 65536 and L below 2^39");
  hipLaunchKernelGGL(spec_splice_blend_kernel, dim3((unsigned)((L + kBlock - 1) / kBlock), B), dim3(kBlock), 0, st, audio_orig,
                     audio_ola, touched, audio_out, T_frames, n_fft, hop, L);
  return check_launch("spec_splice_blend");
}

}  // namespace isi
