// Per-cell weighted mixtures of codebook rows: the step in front of VQVAE.decode that turns M codemaps and M weight maps
// into a real-valued quantised map (timbre interpolation, sweeps between sounds, crossfades).
//
//   out[n, :] = sum over m ascending, of the terms with w[m, n] != 0, of  w[m, n] * E[id[m, n], :]
//
// A term whose weight compares equal to zero (+0.0 or -0.0) does not exist: its id is loaded but never looked at (it may
// be -1, K, the priors' mask token, 2^40) and its codebook row is never read.  A term with a non-zero weight (NaN
// included) and an id outside [0, K) turns all D channels of that cell, and only of that cell, into NaN; such an id is
// never used as an address (code_tables.hip's rule).  One lane's arithmetic is acc = -0.0f, then acc = fmaf(w, e, acc)
// for each existing term, m ascending: a cell whose only term has weight 1 is the codebook row bit for bit (x + -0 = x,
// -0.0 entries included), a cell without a term is -0.0, and a cell's bits depend on its own ids and weights alone.
//
// A lane owns 4 consecutive channels of one cell (float4 loads and stores); a cell takes D / 4 lanes, which need not be
// a power of two, so lanes are numbered through the whole launch and cells straddle waves and workgroups.  The ids and
// weights of source m are read along N: the lanes of a cell share an address, neighbouring cells are neighbours in
// memory.  The rows come from the codebook (128 KB at the models' size: L2).  No LDS, no barrier; nothing of
// device_prims.h applies (no buffer descriptor, no LDS image, no MFMA).  The floor is the output stream plus 12 M bytes
// per cell of ids and weights.
#include "isi_common.h"
#include "isi_internal.h"

namespace isi {

namespace {

constexpr int kBlock = 256;
constexpr int kMaxSources = 8;

// M is a template parameter: every load of a lane (M weights, M ids, M rows) is issued before the first fma waits
template <int M>
__global__ __launch_bounds__(kBlock) void embed_mix_kernel(const int64_t *__restrict__ ids, const int64_t ids_stride,
                                                           const float *__restrict__ weights, const int64_t w_stride,
                                                           const float *__restrict__ codes, float *__restrict__ out,
                                                           const int64_t ldo, const unsigned lanes, const unsigned lp,
                                                           const int K) {
  const unsigned i = blockIdx.x * (unsigned)kBlock + threadIdx.x;      // lanes < 2^31 (host)
  if (i >= lanes) return;
  const unsigned n = i / lp, c4 = i - n * lp;
  float w[M];
  int64_t id[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    w[m] = weights[m * w_stride + n];
    id[m] = ids[m * ids_stride + n];
  }
  bool bad = false;
  bool live[M];
  float4 e[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    live[m] = w[m] != 0.f;                                              // true for NaN, false for +0.0 and -0.0
    const bool in = (uint64_t)id[m] < (uint64_t)K;                      // one unsigned compare: negative and too large alike
    bad |= live[m] && !in;
    const uint64_t row = live[m] && in ? (uint64_t)id[m] : 0u;          // row 0 stands in for a row that is not used
    e[m] = reinterpret_cast<const float4 *>(codes)[row * lp + c4];
  }
  float4 acc = make_float4(-0.f, -0.f, -0.f, -0.f);
#pragma unroll
  for (int m = 0; m < M; ++m) {
    acc.x = live[m] ? __builtin_fmaf(w[m], e[m].x, acc.x) : acc.x;
    acc.y = live[m] ? __builtin_fmaf(w[m], e[m].y, acc.y) : acc.y;
    acc.z = live[m] ? __builtin_fmaf(w[m], e[m].z, acc.z) : acc.z;
    acc.w = live[m] ? __builtin_fmaf(w[m], e[m].w, acc.w) : acc.w;
  }
  if (bad) {
    const float nan = __builtin_nanf("");
    acc = make_float4(nan, nan, nan, nan);
  }
  *reinterpret_cast<float4 *>(out + (int64_t)n * ldo + 4 * c4) = acc;
}

template <int M>
void launch_mix(const int64_t *ids, int64_t ids_stride, const float *weights, int64_t w_stride, const float *codes, float *out,
                int64_t ldo, unsigned lanes, unsigned lp, int K, hipStream_t stream) {
  hipLaunchKernelGGL(embed_mix_kernel<M>, dim3((lanes + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, ids, ids_stride, weights,
                     w_stride, codes, out, ldo, lanes, lp, K);
}

}  // namespace

int embed_mix_f32(const int64_t *ids, int64_t ids_stride, const float *weights, int64_t w_stride, const float *codes, float *out,
                  int64_t ldo, int64_t N, int M, int D, int K, hipStream_t stream) {
  if (!ids || !weights || !codes || !out) return invalid("embed_mix: null pointer");
  if (N <= 0) return invalid("embed_mix: N must be positive");
  if (M < 1 || M > kMaxSources) return invalid("embed_mix: M must be 1..8");
  if (D <= 0 || (D & 3)) return invalid("embed_mix: D must be a positive multiple of 4");
  if (K <= 0) return invalid("embed_mix: K must be positive");
  if (((reinterpret_cast<uintptr_t>(codes) | reinterpret_cast<uintptr_t>(out)) & 15) || (ldo & 3))
    return invalid("embed_mix: codes and out must be 16-byte aligned and ldo a multiple of 4");
  if (ldo < D) return invalid("embed_mix: ldo must be at least D");
  if (ids_stride < N || w_stride < N) return invalid("embed_mix: ids_stride and w_stride must be at least N");
  // the kernel numbers its lanes in 32 bits (N D / 4 of them, rounded up to whole workgroups) and forms every address
  // in 64 bits from a source stride below 2^56 elements and an output stride below 2^31 floats
  if (N >= (1ll << 31) || N * (D / 4) >= (1ll << 31) || ids_stride >= (1ll << 56) || w_stride >= (1ll << 56) || ldo >= (1ll << 31))
    return unsupported("embed_mix: N D / 4 must stay below 2^31, the source strides below 2^56, ldo below 2^31");
  const unsigned lanes = (unsigned)(N * (D / 4)), lp = (unsigned)(D / 4);
  switch (M) {
    case 1: launch_mix<1>(ids, ids_stride, weights, w_stride, codes, out, ldo, lanes, lp, K, stream); break;
    case 2: launch_mix<2>(ids, ids_stride, weights, w_stride, codes, out, ldo, lanes, lp, K, stream); break;
    case 3: launch_mix<3>(ids, ids_stride, weights, w_stride, codes, out, ldo, lanes, lp, K, stream); break;
    case 4: launch_mix<4>(ids, ids_stride, weights, w_stride, codes, out, ldo, lanes, lp, K, stream); break;
    case 5: launch_mix<5>(ids, ids_stride, weights, w_stride, codes, out, ldo, lanes, lp, K, stream); break;
    case 6: launch_mix<6>(ids, ids_stride, weights, w_stride, codes, out, ldo, lanes, lp, K, stream); break;
    case 7: launch_mix<7>(ids, ids_stride, weights, w_stride, codes, out, ldo, lanes, lp, K, stream); break;
    default: launch_mix<8>(ids, ids_stride, weights, w_stride, codes, out, ldo, lanes, lp, K, stream); break;
  }
  return check_launch("embed_mix_f32");
}

}  // namespace isi
