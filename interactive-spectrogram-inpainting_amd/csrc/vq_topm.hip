// The M nearest codes of each vector, in order, among the codes its palette allows (the specification:
// isi_vq_nearest_topm_f32's comment in include/isi_hip.h; tests/vq_topm_spec.py in float64).
//
//   d[n,k]     = (|z_n|^2 - 2 z_n.e_k) + |e_k|^2                    (fp32, vq_dist.h: the stage of vq_nearest_kernel)
//   rank m     = the m-th smallest (d, k) pair, lexicographic, over the allowed k with d < +inf
//   missing    = id -1, distance +inf;  a vector whose |z|^2 is not finite: id -1, distance NaN at every rank
//
// Persistent workgroups; the codebook ([Kp][D + 4] fp32), |e|^2 and the palette rows ([P][Kp / 32] words) stay in LDS.
// A wave handles 32 vectors per pass, one vector per lane pair (l, l + 32): a lane sees 16 of a tile's 32 codes, in
// ascending code order over the whole search, and keeps its own sorted list of M (d, k) in registers -- M is a
// template parameter and every list operation is unrolled (an array indexed at run time would live in scratch).  Within
// a lane a strict `<` keeps the earlier (lower) code in front of an equal distance.  One palette word covers the 32
// codes of a tile, so the mask costs one LDS read per tile and one bit test per distance; without a palette (MASK
// false) neither is compiled.  At the end the partner's list arrives through 2 M cross-lane exchanges and is inserted
// under the (d, k) order: both lanes end with the same merged list; half 0 stores the ids, half 1 the distances.
//
// Not inserted, by the comparisons alone: a padding code (|e|^2 = +inf), a non-finite code (its |e|^2 is +inf or NaN:
// the distance is not < +inf; the matrix pipe keeps a code's NaN in that code's row), a code outside the palette.
#include "isi_common.h"
#include "isi_internal.h"
#include "prof.h"
#include "vq_dist.h"

namespace isi {

namespace {

constexpr int kTopmMaxM = 8;
constexpr int kTopmMaxPalettes = 64;   // palette rows kept in LDS (4 KiB at K = 512)

template <int M>
struct TopList {
  float d[M];
  int k[M];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int m = 0; m < M; ++m) { d[m] = INFINITY; k[m] = -1; }
  }
  // (dv, kv) behind every entry with d <= dv: the caller offers codes in ascending order
  __device__ __forceinline__ void insert_after_equal(const float dv, const int kv) {
    bool lt[M];
#pragma unroll
    for (int m = 0; m < M; ++m) lt[m] = dv < d[m];             // false for a NaN and for +inf against +inf
#pragma unroll
    for (int m = M - 1; m >= 0; --m) {
      const bool shift = m > 0 && lt[m > 0 ? m - 1 : 0];       // the entry above moves down into m
      d[m] = shift ? d[m > 0 ? m - 1 : 0] : (lt[m] ? dv : d[m]);
      k[m] = shift ? k[m > 0 ? m - 1 : 0] : (lt[m] ? kv : k[m]);
    }
  }
  // the same under the full (d, k) order (the partner's entries: other codes, in any order relative to this lane's)
  __device__ __forceinline__ void insert_ordered(const float dv, const int kv) {
    bool lt[M];
#pragma unroll
    for (int m = 0; m < M; ++m) lt[m] = dv < d[m] || (dv == d[m] && kv < k[m]);
#pragma unroll
    for (int m = M - 1; m >= 0; --m) {
      const bool shift = m > 0 && lt[m > 0 ? m - 1 : 0];
      d[m] = shift ? d[m > 0 ? m - 1 : 0] : (lt[m] ? dv : d[m]);
      k[m] = shift ? k[m > 0 ? m - 1 : 0] : (lt[m] ? kv : k[m]);
    }
  }
};

template <int D, int M, bool MASK>
__global__ __launch_bounds__(VQ_BLOCK) void vq_topm_kernel(
    const float *__restrict__ z, const float *__restrict__ codes, const float *__restrict__ e2g,
    const uint32_t *__restrict__ allowed, const int P, const int32_t *__restrict__ allowed_row,
    int64_t *__restrict__ ids_out, const int64_t ids_stride, float *__restrict__ dist_out, const int64_t dist_stride,
    const int64_t N, const int K) {
  constexpr int LDD = D + 4;
  constexpr int NQ = D / 8;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Kp = (K + 31) & ~31;
  const int W = Kp >> 5;                                        // palette words per row
  float *cb = smem;                                             // [Kp][LDD]
  float *e2 = smem + (size_t)Kp * LDD;                          // [Kp]
  uint32_t *pal = reinterpret_cast<uint32_t *>(e2 + Kp);        // [P][W]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int col = lane & 31;   // vector (MFMA column) handled by this lane
  const int half = lane >> 5;

  vq_fill_rows_f32<D>(cb, codes, K, Kp, tid);
  for (int i = tid; i < Kp; i += VQ_BLOCK) e2[i] = i < K ? e2g[i] : INFINITY;
  if (MASK)
    for (int i = tid; i < P * W; i += VQ_BLOCK) pal[i] = allowed[i];
  __syncthreads();

  const int64_t n_iter = (N + VQ_VEC_PER_BLOCK_ITER - 1) / VQ_VEC_PER_BLOCK_ITER;
  for (int64_t it = blockIdx.x; it < n_iter; it += gridDim.x) {
    const int64_t n = it * VQ_VEC_PER_BLOCK_ITER + wave * 32 + col;
    const bool valid = n < N;
    float4 zq[NQ];
    float x2p = 0.f;
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      const float4 v = vq_load_quad_f32(z, n, valid, 2 * j + half, D);
      zq[j] = v;
      x2p += vq_quad_norm2_f32(v.x, v.y, v.z, v.w);
    }
    const float x2 = x2p + __shfl_xor(x2p, 32);

    // the vector's palette row; a row outside [0, P) is never an address: that vector sees an empty palette
    const uint32_t *prow = pal;
    bool row_ok = true;
    if (MASK) {
      const int row = (allowed_row && valid) ? allowed_row[n] : 0;
      row_ok = (unsigned)row < (unsigned)P;
      prow = pal + (row_ok ? row : 0) * W;
    }

    TopList<M> top;
    top.clear();
    for (int kt = 0; kt < Kp; kt += 32) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      vq_tile_dots_f32<D>(acc, cb + (size_t)(kt + col) * LDD + half * 4, zq);
      uint32_t word = 0xFFFFFFFFu;
      if (MASK) word = row_ok ? prow[kt >> 5] : 0u;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = mfma_row(r, half);                      // ascending in r
        float d = vq_distance_f32(x2, acc[r], e2[kt + row]);
        if (MASK) d = ((word >> row) & 1u) ? d : INFINITY;      // +inf is never inserted
        top.insert_after_equal(d, kt + row);
      }
    }
    // merge the two half-waves (same vector, disjoint code rows): both lanes end with the same list
    {
      float od[M];
      int ok[M];
#pragma unroll
      for (int m = 0; m < M; ++m) { od[m] = __shfl_xor(top.d[m], 32); ok[m] = __shfl_xor(top.k[m], 32); }
#pragma unroll
      for (int m = 0; m < M; ++m) top.insert_ordered(od[m], ok[m]);
    }
    if (valid) {
      // a vector with a NaN / Inf component (|z|^2 not finite) has no distance at all: NaN instead of +inf
      const bool lost = !(x2 < INFINITY);
      if (half == 0) {
#pragma unroll
        for (int m = 0; m < M; ++m) ids_out[m * ids_stride + n] = lost ? -1 : top.k[m];
      } else {
#pragma unroll
        for (int m = 0; m < M; ++m) dist_out[m * dist_stride + n] = lost ? NAN : top.d[m];
      }
    }
  }
}

int topm_grid(int64_t N) {       // as the exact search: at most one persistent workgroup per CU
  const int64_t n_iter = (N + VQ_VEC_PER_BLOCK_ITER - 1) / VQ_VEC_PER_BLOCK_ITER;
  return (int)(n_iter < 256 ? n_iter : 256);
}

struct TopmArgs {
  const float *z, *codes, *e2;
  const uint32_t *allowed;
  int P;
  const int32_t *allowed_row;
  int64_t *ids;
  int64_t ids_stride;
  float *dist;
  int64_t dist_stride, N;
  int K;
  size_t smem;
  hipStream_t stream;
};

template <int D, int M, bool MASK>
int launch_topm(const TopmArgs &a) {
  auto kern = vq_topm_kernel<D, M, MASK>;
  if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.smem) != hipSuccess)
    return check_launch("hipFuncSetAttribute(vq_topm)");
  {
    prof::Scope scope(prof::K_VQ_NEAREST, 2.0 * a.N * a.K * D, 4.0 * ((double)a.N * D + (double)a.K * D) + 12.0 * a.N * M, a.stream);
    ISI_PROF_LAUNCH(scope, kern, dim3(topm_grid(a.N)), dim3(VQ_BLOCK), a.smem, a.stream, a.z, a.codes, a.e2, a.allowed, a.P,
                    a.allowed_row, a.ids, a.ids_stride, a.dist, a.dist_stride, a.N, a.K);
  }
  return check_launch("vq_nearest_topm_f32");
}

template <int D, bool MASK>
int launch_topm_m(const TopmArgs &a, int M) {
  switch (M) {
    case 1: return launch_topm<D, 1, MASK>(a);
    case 2: return launch_topm<D, 2, MASK>(a);
    case 3: return launch_topm<D, 3, MASK>(a);
    case 4: return launch_topm<D, 4, MASK>(a);
    case 5: return launch_topm<D, 5, MASK>(a);
    case 6: return launch_topm<D, 6, MASK>(a);
    case 7: return launch_topm<D, 7, MASK>(a);
    default: return launch_topm<D, 8, MASK>(a);
  }
}

template <int D>
int launch_topm_d(TopmArgs &a, int M) {
  const int Kp = (a.K + 31) & ~31;
  // the exact search's LDS formula (vq_dist.h) plus the palette rows
  a.smem = vq_exact_lds_bytes<D>(Kp) + (size_t)a.P * (Kp / 32) * sizeof(uint32_t);
  if (a.smem > kVqLdsBudget) return unsupported("vq_topm: codebook and palettes do not fit in LDS");
  return a.allowed ? launch_topm_m<D, true>(a, M) : launch_topm_m<D, false>(a, M);
}

}  // namespace

int vq_nearest_topm_f32(const float *z, const float *codes, const float *e2, const uint32_t *allowed, int P,
                        const int32_t *allowed_row, int64_t *ids, int64_t ids_stride, float *dist, int64_t dist_stride,
                        int64_t N, int D, int K, int M, hipStream_t stream) {
  if (!z || !codes || !e2 || !ids || !dist) return invalid("vq_topm: null pointer");
  if (N <= 0) return invalid("vq_topm: N must be positive");
  if (M < 1 || M > kTopmMaxM) return invalid("vq_topm: M must be 1..8");
  if (D != 8 && D != 16 && D != 32 && D != 64) return invalid("vq_topm: D must be 8, 16, 32 or 64");
  if (K <= 0) return invalid("vq_topm: K must be positive");
  if (ids_stride < N || dist_stride < N) return invalid("vq_topm: ids_stride and dist_stride must be at least N");
  if (!allowed && allowed_row) return invalid("vq_topm: allowed_row given without allowed");
  if (!allowed && P != 0) return invalid("vq_topm: P must be 0 without allowed");
  if (allowed && P <= 0) return invalid("vq_topm: P must be positive with allowed");
  if ((reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(codes)) & 15)
    return invalid("vq_topm: z and codes must be 16-byte aligned");
  if (P > kTopmMaxPalettes) return unsupported("vq_topm: at most 64 palette rows");
  // addresses are formed in 64 bits from n < N and a rank's stride: keep m * stride + n far from overflow
  if (N >= (1ll << 40) || ids_stride >= (1ll << 56) || dist_stride >= (1ll << 56))
    return unsupported("vq_topm: N must stay below 2^40 and the strides below 2^56");
  TopmArgs a{z, codes, e2, allowed, P, allowed_row, ids, ids_stride, dist, dist_stride, N, K, 0, stream};
  switch (D) {
    case 8: return launch_topm_d<8>(a, M);
    case 16: return launch_topm_d<16>(a, M);
    case 32: return launch_topm_d<32>(a, M);
    default: return launch_topm_d<64>(a, M);
  }
}

}  // namespace isi
