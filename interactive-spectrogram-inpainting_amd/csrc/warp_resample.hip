// Time-warped band-limited read (gfx950): the resampler's Kaiser-windowed sinc with a position and a cutoff per output
// sample -- what turns a pitch curve into sound (GANsynth_pytorch/bend.py; specification
// tests/warp_resample_spec.py):
//   y[b, n] = sum_m c h(c (p - m)) x[b, m]  over the integers m in [0, L) with |c (p - m)| < Z,  m ascending, fp32 fma
//   p = pos[b or 0, n] (double, source samples),  c = min(max(cut[b or 0, n], ISI_WARP_CUT_MIN), 1)  (NaN: the minimum)
//   h(t) = sinc(t) I0(BETA sqrt(1 - (t / Z)^2)) / I0(BETA),  Z = 64, BETA = 14.769656459379492 ("kaiser best")
// There is no table: a position is any real number, so the weights are evaluated per tap.  floor(p) and the fraction are
// taken ONCE per output in double; after that a tap's distance is an exact small integer plus that fraction in fp32:
//   d = float(floor(p) - m) + frac,  th = c d,  tl = fma(c, d, -th): th + tl is the product exactly
//   sin(pi t) = (-1)^n r S(r^2),  n = rint(th), r = (th - n) + tl, S the degree-6 Taylor polynomial (|r| <= 1/2)
//   window: s = th / Z, v = s s, u = 1 - v, ul = what u lost of 1 - s^2;  A(u) = sum_k a_k u^k (k <= 23, a_k > 0, Horner:
//   nothing cancels), times 1 + 7.13 ul: near t = 0 the window moves 7 times as fast as u, and an ulp of u would be 4 of w
// The spec's fp32 emulation of exactly these operations is within 4.02 x 2^-24 c of the float64 weight.
//
// One output per lane, consecutive outputs in consecutive lanes: neighbouring outputs read neighbouring samples, a 4 s
// row is 256 KB and stays in L2, and the work is the 50-odd VALU operations per tap, not the loads -- no LDS stage.
// Bounds: an output is computed only for p in [-400, L + 400] (decided in double, which also drops NaN and infinities), so
// floor(p) is a small int64; the tap range is clamped to [0, L) before the loop.  No content of pos or cut reaches an
// address.  An output's bits depend on its own p, c and the samples under its support alone.
#include <cmath>

#include "isi_common.h"
#include "isi_internal.h"

namespace isi {

namespace {
constexpr int WR_THREADS = 256;
constexpr float WR_Z = 64.f;
constexpr float WR_CUT_MIN = ISI_WARP_CUT_MIN;
constexpr double WR_MARGIN = 400.0;   // > Z / ISI_WARP_CUT_MIN + 2 taps
static_assert(64.0 / ISI_WARP_CUT_MIN + 3.0 < WR_MARGIN, "the margin must cover the widest support");

// c h(c d): the operations of tests/warp_resample_spec.weights32, one for one
__device__ __forceinline__ float warp_weight(float c, float d, bool *taken) {
#pragma clang fp contract(off)
  const float th = c * d;
  const float tl = fmaf(c, d, -th);
  const float n = rintf(th);
  const float r = (th - n) + tl;
  const float z = r * r;
  float s = 0x1.e8f434p-12f;
  s = fmaf(s, z, -0x1.e3075p-8f);
  s = fmaf(s, z, 0x1.507834p-4f);
  s = fmaf(s, z, -0x1.32d2ccp-1f);
  s = fmaf(s, z, 0x1.466bc6p+1f);
  s = fmaf(s, z, -0x1.4abbcep+2f);
  s = fmaf(s, z, 0x1.921fb6p+1f);
  float sinpi = r * s;
  if ((int)n & 1) sinpi = -sinpi;
  const float den = 0x1.921fb6p+1f * th;
  const float sinc = fabsf(th) < 0x1p-20f ? 1.f : sinpi / den;
  const float sc = th * 0x1p-6f;
  const float v = sc * sc;
  const float vl = fmaf(sc, sc, -v);
  const float u = 1.f - v;
  const float ul = ((1.f - u) - v) - vl;
  float a = 0x1.a926eap-35f;
  a = fmaf(a, u, 0x1.01c012p-31f);
  a = fmaf(a, u, 0x1.1df07p-28f);
  a = fmaf(a, u, 0x1.210772p-25f);
  a = fmaf(a, u, 0x1.08fda2p-22f);
  a = fmaf(a, u, 0x1.b6872p-20f);
  a = fmaf(a, u, 0x1.45aa4cp-17f);
  a = fmaf(a, u, 0x1.af72aep-15f);
  a = fmaf(a, u, 0x1.fa52acp-13f);
  a = fmaf(a, u, 0x1.051e9ap-10f);
  a = fmaf(a, u, 0x1.d53a9p-9f);
  a = fmaf(a, u, 0x1.6b859ap-7f);
  a = fmaf(a, u, 0x1.dfef4ep-6f);
  a = fmaf(a, u, 0x1.0a3626p-4f);
  a = fmaf(a, u, 0x1.e8245p-4f);
  a = fmaf(a, u, 0x1.6a829ep-3f);
  a = fmaf(a, u, 0x1.a96be8p-3f);
  a = fmaf(a, u, 0x1.7e3d1ep-3f);
  a = fmaf(a, u, 0x1.f8a54p-4f);
  a = fmaf(a, u, 0x1.ceacbp-5f);
  a = fmaf(a, u, 0x1.0f7bfep-6f);
  a = fmaf(a, u, 0x1.666c6cp-9f);
  a = fmaf(a, u, 0x1.a4a026p-13f);
  a = fmaf(a, u, 0x1.ed9f56p-19f);
  a = fmaf(a, ul * 7.13f, a);
  *taken = fabsf(th) < WR_Z;
  return (c * sinc) * a;
}
}  // namespace

__global__ __launch_bounds__(WR_THREADS) void warp_resample_kernel(const float *__restrict__ x, int64_t x_stride,
                                                                   const double *__restrict__ pos,
                                                                   const float *__restrict__ cut, int pos_batch,
                                                                   float *__restrict__ y, int64_t y_stride, int64_t L,
                                                                   int64_t n_out, int tiles) {
  const int tile = (int)(blockIdx.x % (unsigned)tiles), b = (int)(blockIdx.x / (unsigned)tiles);
  const int64_t n = (int64_t)tile * WR_THREADS + (int)threadIdx.x;
  if (n >= n_out) return;
  const int64_t at = (pos_batch > 1 ? (int64_t)b * n_out : 0) + n;
  const double p = pos[at];
  float c = cut[at];
  c = c >= WR_CUT_MIN ? c : WR_CUT_MIN;                       // a NaN too
  c = c > 1.f ? 1.f : c;
  float acc = 0.f;
  if (p >= -WR_MARGIN && p <= (double)L + WR_MARGIN) {         // false for a NaN
    const double fl = floor(p);
    const float frac = (float)(p - fl);
    const int64_t ip = (int64_t)fl;                            // in [-400, L + 400]
    const int reach = (int)ceilf(WR_Z / c) + 1;                // <= 321
    int64_t m_lo = ip - reach, m_hi = ip + reach + 1;
    if (m_lo < 0) m_lo = 0;
    if (m_hi > L - 1) m_hi = L - 1;
    const float *__restrict__ xr = x + (int64_t)b * x_stride + m_lo;
    const int k0 = (int)(ip - m_lo);                           // the first tap's integer distance; |k0 - j| <= 722
    const int count = (int)(m_hi - m_lo) + 1;                  // <= 0 when the support misses [0, L)
    for (int j = 0; j < count; ++j) {
      bool taken;
      const float w = warp_weight(c, (float)(k0 - j) + frac, &taken);
      if (taken) acc = fmaf(w, xr[j], acc);
    }
  }
  y[(int64_t)b * y_stride + n] = acc;
}

int warp_resample_f32(const float *x, int64_t x_stride, const double *pos, const float *cut, int pos_batch, float *y,
                      int64_t y_stride, int B, int64_t L, int64_t n_out, hipStream_t st) {
  if (!x || !pos || !cut || !y) return invalid("warp_resample: null pointer");
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(cut) | reinterpret_cast<uintptr_t>(y)) & 3)
    return invalid("warp_resample: x, cut and y must be aligned to a float");
  if (reinterpret_cast<uintptr_t>(pos) & 7) return invalid("warp_resample: pos must be aligned to a double");
  if (B < 1 || L < 1 || n_out < 1) return invalid("warp_resample: non-positive size");
  if (pos_batch != 1 && pos_batch != B) return invalid("warp_resample: pos_batch must be 1 or B");
  if (L >= ((int64_t)1 << 31) || n_out >= ((int64_t)1 << 31)) return unsupported("warp_resample: rows of 2^31 samples or more");
  if (x_stride < L || y_stride < n_out) return invalid("warp_resample: a row stride shorter than the row");
  const int64_t tiles = (n_out + WR_THREADS - 1) / WR_THREADS;
  if (tiles * B >= ((int64_t)1 << 31)) return unsupported("warp_resample: more than 2^31 workgroups");
  hipLaunchKernelGGL(warp_resample_kernel, dim3((unsigned)(tiles * B)), dim3(WR_THREADS), 0, st, x, x_stride, pos, cut,
                     pos_batch, y, y_stride, L, n_out, (int)tiles);
  return check_launch("warp_resample");
}

}  // namespace isi
