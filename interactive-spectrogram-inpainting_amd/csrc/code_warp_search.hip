// Time-warped search of a code database (gfx950): "which stored sound is like this one, played a little faster or slower".
// The arithmetic is this project's own (specification tests/code_warp_search_spec.py).  A grid has
// W query columns and T item columns; the query is one or two parts (isi_warp_part: a top layer, a bottom layer, or both),
// part p with F_p rows, r_p columns of its own per grid column, stored codes [N, F_p, T r_p], per-cell cost rows
// [Q, F_p * W r_p, K_p] (cell c = f * (W r_p) + (i r_p + u)) and weights [Q, F_p, W r_p] or null:
//   cost[i][t] = sum_p sum_f sum_u fl(w_p[f][i r_p + u] * rows_p[c][min(codes_p[n][f][t r_p + u], K_p - 1)])
// fp32 from +0, one rounding per product, added in the order parts, f, u; a cell of weight exactly 0 adds +0.  Query column
// i is matched to item column p(i), p(i+1) - p(i) in {0, 1, 2}, lo <= p(i) - i <= hi, 0 <= p(i) <= T - 1:
//   D[0][t] = cost[0][t];  D[i][t] = fl(cost[i][t] + min(D[i-1][t-1], D[i-1][t], D[i-1][t-2]));  dist = min_t D[W-1][t]
// with +inf wherever (i, t) is not admissible, the minimum taken by strict comparisons in the order t-1, t, t-2 and `end`
// the smallest t that attains dist.  No atomics: the bits of dist[j][n] depend on the query's rows and weights, the item's
// codes, T, W, lo and hi only.
//
// Search.  One workgroup (256 threads, one item per lane) owns 256 items and one query.  In band coordinates s = t - i - lo
// (S = hi - lo + 1 <= 64 positions) the three predecessors of D_i[s] are D_{i-1}[s], D_{i-1}[s+1] and D_{i-1}[s-1]: the
// running minima are a register array of B >= S floats with static indices (template argument, no scratch) and one column
// is one sweep over it.  The query is walked in groups of up to G columns; the costs of a group, cost[G][B], are a second
// set of band registers.  For every row (f, u) of a part the lane fetches the G + B - 1 codes of that row that the group's
// band reaches -- each once -- clamps them and scales them to byte offsets; a fetched code then serves every (column,
// band position) pair of the group that reaches it, G B look-ups in LDS from G + B - 1 fetches.  The rows of the group's
// cells are staged with stage_query_rows (device_prims.h) under the searches' common limit of kCodeStageFloats floats
// (64 KB): as many whole rows f of a part as fit at a time, the costs accumulating across those chunks in f order; where
// not even one row f of G columns fits (large K) the host narrows the group, down to one column, and below that one cell
// is staged at a time.  Look-ups for cells outside the item or the band read row offset 0 and are discarded: D is +inf
// there whatever the cost.
//
// Path.  isi_code_warp_path_f32 runs the same recurrence for M <= 64 chosen items per query: one wavefront per (query,
// item), lane s holds band position s, the column costs are read from the rows in global memory with the search's
// roundings (__fmul_rn / __fadd_rn: no contraction), the back-pointers go to the workspace [Q M][W][S] bytes and lane 0
// backtracks.  It is not tuned.
//
// Limits: S <= 64, K <= 16384, W <= 4096, Q <= 64 (grid.y), Q * N < 2^39, F * W * r and F * T * r below 2^31.
#include "isi_common.h"
#include "isi_internal.h"
#include "device_prims.h"

namespace isi {

namespace {
constexpr int WS_THREADS = 256;                    // one item per lane
constexpr int WS_MAX_BAND = 64;
constexpr int WS_MAX_K = kCodeStageFloats;
constexpr int WS_MAX_W = 4096;
constexpr int WS_MAX_Q = 64;
constexpr int WS_MAX_M = 64;

struct WarpParts {                                  // the kernel argument: isi_warp_part by value
  isi_warp_part part[2];
  int n_parts;
};

// One row (f, u) of a part for one group of columns: `row` points at codes[n][f][u], item column t lies at row[t * r];
// `a` is the item column of window element 0 (query column i0 at band position 0); lds is the staged row of the group's
// column 0 and col[gi] the byte offset of column gi's (clamped to the last column the group holds).
template <int B, int G>
__device__ __forceinline__ void warp_row_costs(float (&cost)[G][B], const char *lds, const unsigned (&col)[G],
                                               const uint16_t *__restrict__ row, int r, int a, int T, int S, bool valid,
                                               unsigned kmax) {
  unsigned off[G + B - 1];
#pragma unroll
  for (int k = 0; k < G + B - 1; ++k) {
    const int t = a + k;
    unsigned x = 0u;
    if (valid && t >= 0 && t < T) x = row[(size_t)t * (size_t)r];
    x = x < kmax ? x : kmax;
    off[k] = x << 2;
  }
#pragma unroll
  for (int s = 0; s < B; ++s) {
    if (s < S) {                                                  // (uniform)
#pragma unroll
      for (int gi = 0; gi < G; ++gi) cost[gi][s] += *reinterpret_cast<const float *>(lds + col[gi] + off[gi + s]);
    }
  }
}

template <int B, int G>
__global__ __launch_bounds__(WS_THREADS) void code_warp_search_kernel(const WarpParts P, const uint8_t *__restrict__ allowed,
                                                                      float *__restrict__ dist, int32_t *__restrict__ end,
                                                                      int64_t N, int T, int W, int lo, int S, int gcols) {
  extern __shared__ float rows[];
  const int tid = (int)threadIdx.x, j = (int)blockIdx.y;
  const int64_t n = (int64_t)blockIdx.x * WS_THREADS + tid;
  const bool valid = n < N;
  const float inf = __builtin_inff();
  float D[B];
#pragma unroll
  for (int s = 0; s < B; ++s) D[s] = inf;
  for (int i0 = 0; i0 < W; i0 += gcols) {
    const int ng = W - i0 < gcols ? W - i0 : gcols;
    float cost[G][B];
#pragma unroll
    for (int gi = 0; gi < G; ++gi)
#pragma unroll
      for (int s = 0; s < B; ++s) cost[gi][s] = 0.f;
    for (int p = 0; p < P.n_parts; ++p) {
      const int F = P.part[p].F, r = P.part[p].r, K = P.part[p].K;
      const int Tr = T * r, Wr = W * r, cells = F * Wr;
      const uint16_t *__restrict__ item = P.part[p].codes + (size_t)(valid ? n : 0) * ((size_t)F * Tr);
      const float *__restrict__ R = P.part[p].rows;
      const float *__restrict__ wj = P.part[p].weights ? P.part[p].weights + (size_t)j * cells : nullptr;
      const int vec_rows = (K % 4) == 0 && !(reinterpret_cast<uintptr_t>(R) & 15);
      const unsigned kmax = (unsigned)K - 1u;
      const int64_t per_f = (int64_t)gcols * r * K;               // floats of one row f of the group
      unsigned col[G];
      if (per_f <= kCodeStageFloats) {
        const int fc = kCodeStageFloats / (int)per_f;             // rows f per chunk
#pragma unroll
        for (int gi = 0; gi < G; ++gi) col[gi] = (unsigned)(gi < ng ? gi : ng - 1) * (unsigned)(r * K * 4);
        for (int f0 = 0; f0 < F; f0 += fc) {
          const int nf = F - f0 < fc ? F - f0 : fc;
          for (int ff = 0; ff < nf; ++ff)
            stage_query_rows<WS_THREADS>(rows + ff * (int)per_f, R, wj, j, cells, (f0 + ff) * Wr + i0 * r, ng * r, K, vec_rows);
          __syncthreads();
          for (int ff = 0; ff < nf; ++ff)
            for (int u = 0; u < r; ++u)
              warp_row_costs<B, G>(cost, reinterpret_cast<const char *>(rows + ff * (int)per_f + u * K), col,
                                   item + (size_t)(f0 + ff) * Tr + u, r, i0 + lo, T, S, valid, kmax);
          __syncthreads();
        }
      } else {                                                    // gcols == 1 (host): one cell at a time
#pragma unroll
        for (int gi = 0; gi < G; ++gi) col[gi] = 0u;
        for (int f = 0; f < F; ++f)
          for (int u = 0; u < r; ++u) {
            stage_query_rows<WS_THREADS>(rows, R, wj, j, cells, f * Wr + i0 * r + u, 1, K, vec_rows);
            __syncthreads();
            warp_row_costs<B, G>(cost, reinterpret_cast<const char *>(rows), col, item + (size_t)f * Tr + u, r, i0 + lo, T, S,
                                 valid, kmax);
            __syncthreads();
          }
      }
    }
    // the group's columns through the recurrence: D[s] is D_{i-1} at item column i - 1 + lo + s on entry
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
      if (gi < ng) {                                              // (uniform)
        const int i = i0 + gi, tb = i + lo;
        float left = inf;
#pragma unroll
        for (int s = 0; s < B; ++s) {
          const float cur = D[s], right = s + 1 < B ? D[s + 1] : inf;
          float m = cur;                                          // t - 1, then t, then t - 2: a later one wins only if smaller
          if (right < m) m = right;
          if (left < m) m = left;
          const float v = i == 0 ? cost[gi][s] : cost[gi][s] + m;
          const bool adm = s < S && tb + s >= 0 && tb + s < T;
          D[s] = adm ? v : inf;
          left = cur;
        }
      }
    }
  }
  if (!valid) return;
  float best = inf;
  int at = -1;
#pragma unroll
  for (int s = 0; s < B; ++s) {
    if (D[s] < best) {                                            // strict: ties go to the smallest t
      best = D[s];
      at = s;
    }
  }
  if (allowed && !allowed[n]) {
    best = inf;
    at = -1;
  }
  const size_t o = (size_t)j * (size_t)N + (size_t)n;
  dist[o] = best;
  if (end) end[o] = at < 0 ? -1 : W - 1 + lo + at;
}

// One wavefront per (query, chosen item); lane s = band position s.  D of the previous column lives in LDS (dsh[s + 1],
// +inf at both ends), the back-pointers (p(i) - p(i-1), 255 where (i, t) is not admissible) in the workspace.
__global__ __launch_bounds__(64) void code_warp_path_kernel(const WarpParts P, const int64_t *__restrict__ items, int M,
                                                            int32_t *__restrict__ path, float *__restrict__ dist,
                                                            uint8_t *__restrict__ back, int64_t N, int T, int W, int lo, int S) {
  __shared__ float dsh[WS_MAX_BAND + 2];
  const int s = (int)threadIdx.x, m = (int)blockIdx.x, j = (int)blockIdx.y;
  const size_t pair = (size_t)j * M + m;
  const int64_t n = items[pair];
  int32_t *__restrict__ out = path + pair * (size_t)W;
  const float inf = __builtin_inff();
  if (n < 0 || n >= N) {                                          // (uniform) no such item: no path
    for (int i = s; i < W; i += 64) out[i] = -1;
    if (s == 0) dist[pair] = inf;
    return;
  }
  uint8_t *__restrict__ bp = back + pair * (size_t)W * (size_t)S;
  dsh[s + 1] = inf;
  if (s == 0) dsh[0] = dsh[WS_MAX_BAND + 1] = inf;
  __syncthreads();
  for (int i = 0; i < W; ++i) {
    const int t = i + lo + s;
    const bool adm = s < S && t >= 0 && t < T;
    float cost = 0.f;
    if (adm) {
      for (int p = 0; p < P.n_parts; ++p) {
        const int F = P.part[p].F, r = P.part[p].r, K = P.part[p].K;
        const int Tr = T * r, Wr = W * r, cells = F * Wr;
        const uint16_t *__restrict__ item = P.part[p].codes + (size_t)n * ((size_t)F * Tr);
        const float *__restrict__ R = P.part[p].rows + (size_t)j * (size_t)cells * (size_t)K;
        const float *__restrict__ wj = P.part[p].weights ? P.part[p].weights + (size_t)j * cells : nullptr;
        const unsigned kmax = (unsigned)K - 1u;
        for (int f = 0; f < F; ++f)
          for (int u = 0; u < r; ++u) {
            const int c = f * Wr + i * r + u;
            const float w = wj ? wj[c] : 1.f;
            float term = 0.f;
            if (w != 0.f) {                                       // a cell of weight 0 adds +0: its row is not read
              unsigned x = item[(size_t)f * Tr + (size_t)t * r + u];
              x = x < kmax ? x : kmax;
              term = __fmul_rn(R[(size_t)c * K + x], w);
            }
            cost = __fadd_rn(cost, term);
          }
      }
    }
    const float cur = dsh[s + 1], right = dsh[s + 2], left = dsh[s];
    float best = cur;
    unsigned step = 1u;
    if (right < best) { best = right; step = 0u; }
    if (left < best) { best = left; step = 2u; }
    const float v = i == 0 ? cost : __fadd_rn(cost, best);
    __syncthreads();
    dsh[s + 1] = adm ? v : inf;
    if (s < S) bp[(size_t)i * S + s] = adm ? (uint8_t)step : (uint8_t)255;
    __syncthreads();
  }
  if (s != 0) return;
  float best = inf;
  int at = -1;
  for (int e = 0; e < S; ++e) {
    if (dsh[e + 1] < best) {
      best = dsh[e + 1];
      at = e;
    }
  }
  dist[pair] = best;
  if (at < 0) {
    for (int i = 0; i < W; ++i) out[i] = -1;
    return;
  }
  int t = W - 1 + lo + at;
  for (int i = W - 1; i >= 0; --i) {
    out[i] = t;
    if (i > 0) {
      int e = t - i - lo;                                         // (a cell of a finite path: in the band, its pointer 0, 1 or 2;
      e = e < 0 ? 0 : e >= S ? S - 1 : e;                         //  the clamps keep a NaN-ridden query inside the workspace)
      const int step = (int)bp[(size_t)i * S + e];
      t -= step > 2 ? 1 : step;
    }
  }
}

// What the two entry points share: every refusal about the parts and the grid.
int warp_check(const char *fn, const isi_warp_part *parts, int n_parts, int64_t N, int T, int W, int lo, int hi, int Q) {
  if (!parts) return refuse(ISI_E_INVALID, fn, "parts is a null pointer");
  if (n_parts < 1 || n_parts > 2) return refuse(ISI_E_INVALID, fn, "n_parts must be 1 or 2");
  if (N <= 0) return refuse(ISI_E_INVALID, fn, "N must be positive");
  if (T <= 0) return refuse(ISI_E_INVALID, fn, "T must be positive");
  if (W <= 0) return refuse(ISI_E_INVALID, fn, "W must be positive");
  if (Q < 1 || Q > WS_MAX_Q) return refuse(ISI_E_INVALID, fn, "Q must lie in 1..64");
  for (int p = 0; p < n_parts; ++p) {
    const isi_warp_part &part = parts[p];
    if (!part.codes) return refuse(ISI_E_INVALID, fn, "a part's codes is a null pointer");
    if (!part.rows) return refuse(ISI_E_INVALID, fn, "a part's rows is a null pointer");
    if (part.F <= 0) return refuse(ISI_E_INVALID, fn, "a part's F must be positive");
    if (part.r <= 0) return refuse(ISI_E_INVALID, fn, "a part's r must be positive");
    if (part.K <= 0) return refuse(ISI_E_INVALID, fn, "a part's K must be positive");
    if (reinterpret_cast<uintptr_t>(part.codes) & 1) return refuse(ISI_E_INVALID, fn, "codes must be aligned to 2 bytes");
    if (reinterpret_cast<uintptr_t>(part.rows) & 3) return refuse(ISI_E_INVALID, fn, "rows must be aligned to a float");
    if (reinterpret_cast<uintptr_t>(part.weights) & 3) return refuse(ISI_E_INVALID, fn, "weights must be aligned to a float");
  }
  if (lo > hi) return refuse(ISI_E_INVALID, fn, "lo must not exceed hi");
  if (hi < 0 || lo > T - 1)
    return refuse(ISI_E_INVALID, fn, "the band [lo, hi] leaves the first query column without an item column");
  if ((int64_t)W - 1 + hi < 0 || (int64_t)W - 1 + lo > (int64_t)T - 1)
    return refuse(ISI_E_INVALID, fn, "the band [lo, hi] leaves the last query column without an item column");
  if ((int64_t)hi - lo + 1 > WS_MAX_BAND) return refuse(ISI_E_UNSUPPORTED, fn, "a band of more than 64 drifts (hi - lo + 1)");
  if (W > WS_MAX_W) return refuse(ISI_E_UNSUPPORTED, fn, "W beyond 4096");
  for (int p = 0; p < n_parts; ++p) {
    const isi_warp_part &part = parts[p];
    if (part.K > 65535) return refuse(ISI_E_UNSUPPORTED, fn, "K beyond 65535 (stored codes are 16-bit)");
    if (part.K > WS_MAX_K) return refuse(ISI_E_UNSUPPORTED, fn, "K beyond 16384 (one row per staged cell must fit 64 KB of LDS)");
    const int64_t wide = (int64_t)(W > T ? W : T) * part.r;
    if (wide >= ((int64_t)1 << 31) || (unsigned __int128)part.F * (unsigned __int128)wide >= ((unsigned __int128)1 << 31))
      return refuse(ISI_E_UNSUPPORTED, fn, "F * W * r or F * T * r beyond 2^31 - 1 cells of one map");
  }
  return ISI_OK;
}

WarpParts warp_parts(const isi_warp_part *parts, int n_parts) {
  WarpParts P;
  memset(&P, 0, sizeof P);
  for (int p = 0; p < n_parts; ++p) P.part[p] = parts[p];
  P.n_parts = n_parts;
  return P;
}
}  // namespace

int code_warp_search_f32(const isi_warp_part *parts, int n_parts, const uint8_t *allowed, float *dist, int32_t *end, int64_t N,
                         int T, int W, int lo, int hi, int Q, hipStream_t st) {
  const char *fn = "code_warp_search";
  if (!dist) return refuse(ISI_E_INVALID, fn, "dist is a null pointer");
  if (reinterpret_cast<uintptr_t>(dist) & 3) return refuse(ISI_E_INVALID, fn, "dist must be aligned to a float");
  if (reinterpret_cast<uintptr_t>(end) & 3) return refuse(ISI_E_INVALID, fn, "end must be aligned to 4 bytes");
  if (const int rc = warp_check(fn, parts, n_parts, N, T, W, lo, hi, Q)) return rc;
  if ((unsigned __int128)N * (unsigned)Q >= ((unsigned __int128)1 << 39)) return refuse(ISI_E_UNSUPPORTED, fn, "Q * N beyond 2^39");
  const int64_t gx = (N + WS_THREADS - 1) / WS_THREADS;
  if (gx >= ((int64_t)1 << 31)) return refuse(ISI_E_UNSUPPORTED, fn, "N beyond 2^31 - 1 workgroups of items");
  const int S = hi - lo + 1;
  // band registers B >= S and columns per group G: {4, 9, 17} x 8, 32 x 4, 64 x 2
  const int G = S <= 17 ? 8 : S <= 32 ? 4 : 2;
  int gcols = G;                                                  // narrowed until one row f of every part fits the stage
  for (int p = 0; p < n_parts; ++p)
    while (gcols > 1 && (int64_t)gcols * parts[p].r * parts[p].K > kCodeStageFloats) --gcols;
  size_t lds_floats = 0;
  for (int p = 0; p < n_parts; ++p) {
    const int64_t per_f = (int64_t)gcols * parts[p].r * parts[p].K;
    size_t need = (size_t)parts[p].K;                             // one cell at a time
    if (per_f <= kCodeStageFloats) {
      const int64_t fc = kCodeStageFloats / per_f;
      need = (size_t)((fc < parts[p].F ? fc : parts[p].F) * per_f);
    }
    if (need > lds_floats) lds_floats = need;
  }
  const WarpParts P = warp_parts(parts, n_parts);
  const dim3 grid((unsigned)gx, (unsigned)Q), block(WS_THREADS);
  const size_t lds = lds_floats * sizeof(float);
#define ISI_WS_LAUNCH(B, G) \
  hipLaunchKernelGGL((code_warp_search_kernel<B, G>), grid, block, lds, st, P, allowed, dist, end, N, T, W, lo, S, gcols)
  if (S <= 4) ISI_WS_LAUNCH(4, 8);
  else if (S <= 9) ISI_WS_LAUNCH(9, 8);
  else if (S <= 17) ISI_WS_LAUNCH(17, 8);
  else if (S <= 32) ISI_WS_LAUNCH(32, 4);
  else ISI_WS_LAUNCH(64, 2);
#undef ISI_WS_LAUNCH
  return check_launch(fn);
}

size_t code_warp_path_workspace_bytes(int M, int W, int lo, int hi, int Q) {
  if (M < 1 || M > WS_MAX_M || W <= 0 || W > WS_MAX_W || Q < 1 || Q > WS_MAX_Q || lo > hi || (int64_t)hi - lo + 1 > WS_MAX_BAND)
    return 0;
  return round_up((size_t)Q * M * W * (size_t)(hi - lo + 1), 16);
}

int code_warp_path_f32(const isi_warp_part *parts, int n_parts, const int64_t *items, int M, int32_t *path, float *dist,
                       void *workspace, size_t workspace_bytes, int64_t N, int T, int W, int lo, int hi, int Q, hipStream_t st) {
  const char *fn = "code_warp_path";
  if (!items) return refuse(ISI_E_INVALID, fn, "items is a null pointer");
  if (!path) return refuse(ISI_E_INVALID, fn, "path is a null pointer");
  if (!dist) return refuse(ISI_E_INVALID, fn, "dist is a null pointer");
  if (!workspace) return refuse(ISI_E_INVALID, fn, "workspace is a null pointer");
  if (reinterpret_cast<uintptr_t>(items) & 7) return refuse(ISI_E_INVALID, fn, "items must be aligned to 8 bytes");
  if (reinterpret_cast<uintptr_t>(path) & 3) return refuse(ISI_E_INVALID, fn, "path must be aligned to 4 bytes");
  if (reinterpret_cast<uintptr_t>(dist) & 3) return refuse(ISI_E_INVALID, fn, "dist must be aligned to a float");
  if (M < 1 || M > WS_MAX_M) return refuse(ISI_E_INVALID, fn, "M must lie in 1..64");
  if (const int rc = warp_check(fn, parts, n_parts, N, T, W, lo, hi, Q)) return rc;
  const size_t need = code_warp_path_workspace_bytes(M, W, lo, hi, Q);
  if (workspace_bytes < need) {
    char buf[176];
    snprintf(buf, sizeof buf, "workspace_bytes %zu < %zu (isi_code_warp_path_workspace_bytes)", workspace_bytes, need);
    return refuse(ISI_E_WORKSPACE, fn, buf);
  }
  const WarpParts P = warp_parts(parts, n_parts);
  hipLaunchKernelGGL(code_warp_path_kernel, dim3((unsigned)M, (unsigned)Q), dim3(64), 0, st, P, items, M, path, dist,
                     static_cast<uint8_t *>(workspace), N, T, W, lo, hi - lo + 1);
  return check_launch(fn);
}

}  // namespace isi
