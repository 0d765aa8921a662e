// Band-limited sample-rate conversion (gfx950): a polyphase Kaiser-windowed-sinc FIR in direct form.
//
// The reference's /analyze-audio hands whatever the browser recorded (44.1 or 48 kHz in practice) to
// `spectrograms_helper.from_wavfile(path, duration_n=...)`, which resamples to the models' rate with sox / torchaudio, and
// scales the duration by FS_HZ / original_fs_hz (flask_server.py:557-568, 624-667).  Neither package is here: the
// arithmetic is this project's own, specification tests/resample_spec.py ("Sample-rate conversion"):
//   orig = fs_in / gcd, new = fs_out / gcd, width = ceil(Z orig / (ROLLOFF min(orig, new))), taps = 2 width + orig
//   y[q new + r] = sum_i h[r][i] x[q orig + i - width],  x = 0 outside [0, L),  N_out = ceil(L new / orig)
// The coefficient table is made by the caller (float64 on the host, rounded once to fp32) and lies TAP-MAJOR on the
// device: h[r][i] at table[i * new + r], so lanes of adjacent phase read adjacent floats.
//
// One workgroup owns TQ whole frames q of one row: the input segment [q0 orig - width, (q0 + TQ - 1) orig + width + orig)
// is staged in LDS (zero outside [0, L)), then each of the TQ * new outputs is one thread's sequential fma chain over the
// taps, i ascending: the order is fixed per output, whatever the tile, the batch or the launch.  Lanes run over the phase r
// first.  LDS reads: lanes of one frame read ONE address (broadcast); across frames the stride between lanes is orig
// floats at new == 1 (odd orig: conflict-free over the 32 banks a ds_read_b32 sees; even orig: gcd(orig, 32)-way) and
// at most ceil(32 / new) distinct frames, orig floats apart, share a 32-lane group otherwise (orig = 2, new = 3: 11 even
// addresses below 32, conflict-free).  At new == 1 every lane wants the same coefficient: the table index is then
// wave-uniform and the coefficients come through the scalar cache.
// A direct-form FIR, not an isi_conv2d_f32 call: that route wants a channel count divisible by 4 (orig is 3 or 441 here)
// and would spend split-f16 matrix work on an operation whose 60 s worst case is under 1 GFLOP.
#include <cmath>

#include "isi_common.h"
#include "isi_internal.h"

namespace isi {

namespace {
constexpr double RS_Z = 64.0;                       // zero crossings
constexpr double RS_ROLLOFF = 0.9475937167399596;   // "kaiser best"
constexpr int RS_MAX_TAPS = 16384;                  // one frame's stage = taps floats <= 64 KB of LDS
constexpr int64_t RS_MAX_TABLE = (int64_t)1 << 22;  // new * taps floats
constexpr int RS_THREADS = 256;

// Frames per workgroup: as many as fit p passes of the 256 threads, for the smallest p <= 8 whose passes are filled to
// 85 % (else the best filling seen), within the LDS stage.  A function of the geometry alone -- not of L or B.
int frames_per_tile(int orig, int new_, int width) {
  const int64_t lds_max = ((int64_t)RS_MAX_TAPS - 2 * (int64_t)width) / orig;   // TQ orig + 2 width <= 16384 floats
  int best = 1;
  double best_fill = 0.0;
  for (int p = 1; p <= 8; ++p) {
    int64_t tq = (int64_t)p * RS_THREADS / new_;
    if (tq > lds_max) tq = lds_max;
    if (tq < 1) continue;
    const double fill = (double)(tq * new_) / (double)(p * RS_THREADS);
    if (fill > best_fill) { best_fill = fill; best = (int)tq; }
    if (fill >= 0.85) break;
  }
  return best;
}
}  // namespace

// ONE: new == 1 (one phase: frame = output, coefficient index wave-uniform)
template <bool ONE>
__global__ __launch_bounds__(RS_THREADS) void resample_fir_kernel(const float *__restrict__ x, int64_t x_stride,
                                                                  float *__restrict__ y, int64_t y_stride, int64_t L,
                                                                  int64_t n_out, int orig, int new_, int width, int taps,
                                                                  int tq, int tiles, const float *__restrict__ table) {
  extern __shared__ float stage[];   // [(tq - 1) * orig + taps]
  const int tile = (int)(blockIdx.x % (unsigned)tiles), b = (int)(blockIdx.x / (unsigned)tiles);
  const int tid = (int)threadIdx.x;
  const float *__restrict__ xr = x + (int64_t)b * x_stride;
  const int64_t q0 = (int64_t)tile * tq;
  const int64_t g0 = q0 * orig - width;                     // input index of stage[0]
  const int n_stage = (tq - 1) * orig + taps;
  const int64_t lo = g0 < 0 ? 0 : g0;                       // the part of [g0, g0 + n_stage) inside [0, L)
  int64_t hi = g0 + n_stage < L ? g0 + n_stage : L;
  if (hi < lo) hi = lo;
  // 16-byte aligned interior [va, vb) of [lo, hi): the row base and g0 are arbitrary, so the ends go scalar
  const int64_t mis = (int64_t)((reinterpret_cast<uintptr_t>(xr) >> 2) & 3);
  int64_t va = lo + ((4 - ((lo + mis) & 3)) & 3);
  if (va > hi) va = hi;
  const int64_t vb = va + ((hi - va) & ~(int64_t)3);
  for (int64_t s = tid; s < n_stage; s += RS_THREADS) {      // zeros outside [lo, hi), scalar loads in [lo, va) and [vb, hi)
    const int64_t g = g0 + s;
    if (g >= va && g < vb) continue;
    stage[s] = (g >= lo && g < hi) ? xr[g] : 0.f;
  }
  for (int64_t g = va + 4 * (int64_t)tid; g < vb; g += 4 * RS_THREADS) {
    const float4 v = *reinterpret_cast<const float4 *>(xr + g);
    float *d = stage + (g - g0);                             // not 16-byte aligned in general: four dword writes
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  __syncthreads();
  const int n_tile = tq * new_;
  const int64_t n_base = q0 * new_;
  float *__restrict__ yr = y + (int64_t)b * y_stride;
  for (int o = tid; o < n_tile; o += RS_THREADS) {
    const int64_t n = n_base + o;
    if (n >= n_out) break;
    const int ql = ONE ? o : o / new_;
    const int r = ONE ? 0 : o - ql * new_;
    const float *xs = stage + ql * orig;
    float acc = 0.f;
    if (ONE) {
#pragma unroll 8
      for (int i = 0; i < taps; ++i) acc = fmaf(table[i], xs[i], acc);
    } else {
      const float *__restrict__ h = table + r;
#pragma unroll 8
      for (int i = 0; i < taps; ++i) acc = fmaf(h[(size_t)i * new_], xs[i], acc);
    }
    yr[n] = acc;
  }
}

int resample_geometry(int fs_in, int fs_out, int *orig, int *new_, int *width, int *taps) {
  if (!orig || !new_ || !width || !taps) return invalid("resample_geometry: null pointer");
  if (fs_in <= 0 || fs_out <= 0) return invalid("resample_geometry: sampling rates must be positive");
  int a = fs_in, b = fs_out;
  while (b) { const int t = a % b; a = b; b = t; }
  const int o = fs_in / a, n = fs_out / a;
  const double f0 = RS_ROLLOFF * (double)(o < n ? o : n);
  const double w = std::ceil(RS_Z * (double)o / f0);
  const double t = 2.0 * w + (double)o;
  *orig = o;
  *new_ = n;
  *width = w < 2147483647.0 ? (int)w : 2147483647;
  *taps = t < 2147483647.0 ? (int)t : 2147483647;
  if (t > (double)RS_MAX_TAPS) return unsupported("resample_geometry: more than 16384 taps (the reduced ratio is too fine)");
  if ((double)n * t > (double)RS_MAX_TABLE) return unsupported("resample_geometry: coefficient table beyond 2^22 floats");
  return ISI_OK;
}

int64_t resample_out_len(int64_t L, int orig, int new_) {
  if (L < 0 || orig <= 0 || new_ <= 0) return ISI_E_INVALID;
  const unsigned __int128 n = ((unsigned __int128)L * (unsigned)new_ + (unsigned)(orig - 1)) / (unsigned)orig;
  return n > (unsigned __int128)INT64_MAX ? (int64_t)ISI_E_INVALID : (int64_t)n;
}

int resample_f32(const float *x, int64_t x_stride, float *y, int64_t y_stride, int B, int64_t L, int orig, int new_,
                 int width, const float *table, hipStream_t st) {
  if (!x || !y || !table) return invalid("resample: null pointer");
  if (B <= 0 || L <= 0 || orig <= 0 || new_ <= 0 || width <= 0) return invalid("resample: non-positive size");
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(table)) & 3)
    return invalid("resample: pointers must be aligned to a float");
  if (L >= ((int64_t)1 << 31)) return unsupported("resample: rows of 2^31 samples or more");
  const int64_t taps = 2 * (int64_t)width + orig;
  if (taps > RS_MAX_TAPS) return unsupported("resample: more than 16384 taps");
  if (taps * new_ > RS_MAX_TABLE) return unsupported("resample: coefficient table beyond 2^22 floats");
  const int64_t n_out = resample_out_len(L, orig, new_);
  if (x_stride < L || y_stride < n_out) return invalid("resample: a row stride shorter than the row");
  const int tq = frames_per_tile(orig, new_, width);
  const int64_t frames = (n_out + new_ - 1) / new_;
  const int64_t tiles = (frames + tq - 1) / tq;
  if (tiles * B >= ((int64_t)1 << 31)) return unsupported("resample: more than 2^31 workgroups");
  const size_t lds = (size_t)((int64_t)(tq - 1) * orig + taps) * sizeof(float);
  const dim3 grid((unsigned)(tiles * B)), block(RS_THREADS);
  if (new_ == 1)
    hipLaunchKernelGGL(resample_fir_kernel<true>, grid, block, lds, st, x, x_stride, y, y_stride, L, n_out, orig, new_, width,
                       (int)taps, tq, (int)tiles, table);
  else
    hipLaunchKernelGGL(resample_fir_kernel<false>, grid, block, lds, st, x, x_stride, y, y_stride, L, n_out, orig, new_, width,
                       (int)taps, tq, (int)tiles, table);
  return check_launch("resample");
}

}  // namespace isi
