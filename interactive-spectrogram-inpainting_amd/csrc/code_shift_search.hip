// Shift-invariant search of a code database (gfx950): "which stored sound contains something like this fragment, wherever
// it sits in time".  The arithmetic is this project's own (specification
// tests/code_shift_search_spec.py): stored maps codes [N, F, T], query windows query [Q, F, W], W <= T, offsets
// o_s = shift0 + s * step, s = 0 .. S-1, every one with o_s + W <= T:
//   dist[j][s][n] = sum_f sum_t w[j][f][t] * T_[query[j][f][t]][codes[n][f][t + o_s]]     (query cells >= K count nothing)
// Query cells are numbered c = f * W + t; each product is rounded once, the products of a run of 256 consecutive c are
// added in c order from 0, the run sums in run order -- isi_code_search_f32's order with C = F * W, so at W == T the two
// agree bit for bit.  No atomics: the bits of dist[j][s][n] depend on query[j], weights[j], the item, the table, W and
// o_s only.
//
// Search.  One workgroup (256 threads, one item per lane) owns 256 items, one query, one run of 256 query cells and one
// pass of offsets.  It walks the run in chunks of `cc` cells whose weighted table rows are staged in LDS exactly as
// code_search_kernel stages them (rows[cl][k] = w * T_[q][k], zeros for a mask-token cell, 64 KB).  What differs is the
// use of a fetched code: the emulation with one cropped copy per offset streams the database S times and pays the unpack,
// the clamp and the address for every look-up; here a code is fetched, clamped and scaled to a byte offset once and then
// serves up to min(W, S) look-ups.
//   vector route (step 1 or 2, W % 8 == 0, T % 8 == 0, shift0 % 8 == 0, codes 16-byte aligned, K <= 2048): a pass is NB
//     blocks of 8 offsets, NB in {1, 2, 4, 7}, all 8 NB accumulators in registers.  For 8 query columns of one row f the
//     lane reads the NB * step + 1 aligned 16-byte vectors codes[n][f][t0 + o .. ] that the pass's offsets reach -- each
//     once -- and the fully unrolled block does its 64 look-ups per 8 offsets with static register indices (no scratch):
//     column i at offset e reads rows[cl0 + i][code[i + e * step]].  The stage is written once per chunk and pass.
//   scalar route (everything else): a pass is 8 offsets; each look-up fetches its own code (L1/L2 hits after the first
//     offset has touched the line).
// Both routes add a given offset's cells in ascending c, so they agree bit for bit.  The pass index is the fastest grid
// dimension: the workgroups that read the same items are dispatched together and share the lines in L2.
// Per-run sums go to the workspace [runs][Q][S][N] and a second launch adds them in run order and applies `accumulate`;
// with a single run (F * W <= 256, the maps this project stores) the search kernel writes dist itself -- the same bits,
// since x + 0-th partial is all the second launch would compute.
//
// Limits: K <= 16384, F * W <= 256 * 65535 (runs ride grid.y), Q <= 64 (grid.z), F * T < 2^31, Q * S * N < 2^39.
//
// isi_code_shift_search_rows_f32 is the same search with the stage fed from per-cell window rows
// R [Q][F * W][K] instead of table rows (template argument ROWS): everything after the stage is shared.
#include "isi_common.h"
#include "isi_internal.h"
#include "device_prims.h"

namespace isi {

namespace {
constexpr int SS_THREADS = 256;                    // one item per lane
constexpr int SS_RUN = 256;                        // cells per run: the summation order is F * W's alone (CS_SPLIT)
constexpr int SS_OB = 8;                           // offsets per block
constexpr int SS_MAX_NB = 7;                       // blocks per pass on the vector route (56 accumulators)
constexpr int SS_MAX_K = kCodeStageFloats;
constexpr int64_t SS_MAX_C = (int64_t)SS_RUN * 65535;
constexpr int SS_MAX_Q = 64;

int64_t shift_runs(int64_t C) { return (C + SS_RUN - 1) / SS_RUN; }

__device__ __forceinline__ void store_sum(float *__restrict__ out, size_t at, float v, int accumulate) {
  out[at] = accumulate ? out[at] + v : v;
}
}  // namespace

// The vector route.  blockIdx.x = item block * passes + pass; a pass covers the offsets s_base .. s_base + 8 NB - 1.
// ROWS (both routes): `table` holds per-cell window rows R [Q][F * W][K] (isi_code_shift_search_rows_f32) and `query` is
// unused; only the stage differs.
template <int STEP, int NB, bool ROWS>
__global__ __launch_bounds__(SS_THREADS) void code_shift_search_vec_kernel(
    const uint16_t *__restrict__ codes, const uint16_t *__restrict__ query, const float *__restrict__ weights,
    const float *__restrict__ table, float *__restrict__ out, int64_t N, int F, int T, int W, int shift0, int S, int K, int cc,
    int vec_table, int passes, int accumulate) {
  extern __shared__ float rows[];                   // [cc][K]
  constexpr int NV = NB * STEP + 1;                 // 16-byte vectors of a row that one group of 8 columns reaches
  const int tid = (int)threadIdx.x;
  const int pass = (int)(blockIdx.x % (unsigned)passes), run = (int)blockIdx.y, j = (int)blockIdx.z, Q = (int)gridDim.z;
  const int64_t n = (int64_t)(blockIdx.x / (unsigned)passes) * SS_THREADS + tid;
  const bool valid = n < N;
  const int C = F * W, c_begin = run * SS_RUN;
  const int c_end = C - c_begin < SS_RUN ? C : c_begin + SS_RUN;
  const int s_base = pass * (SS_OB * NB);
  const int v_base = (shift0 + s_base * STEP) >> 3;   // (shift0 % 8 == 0 on this route)
  const int v_row = T >> 3;
  const uint16_t *__restrict__ qj = ROWS ? nullptr : query + (size_t)j * C;   // (no query on the rows route)
  const float *__restrict__ wj = weights ? weights + (size_t)j * C : nullptr;
  const uint16_t *__restrict__ item = codes + (size_t)(valid ? n : 0) * ((size_t)F * T);
  const unsigned kmax = (unsigned)K - 1u;
  const int K4 = K * 4;
  float acc[SS_OB * NB];
#pragma unroll
  for (int a = 0; a < SS_OB * NB; ++a) acc[a] = 0.f;
  for (int c0 = c_begin; c0 < c_end; c0 += cc) {
    const int ncell = c_end - c0 < cc ? c_end - c0 : cc;          // a multiple of 8: W % 8 == 0 and cc % 8 == 0
    if constexpr (ROWS) stage_query_rows<SS_THREADS>(rows, table, wj, j, C, c0, ncell, K, vec_table);
    else stage_code_rows<SS_THREADS>(rows, qj, wj, table, c0, ncell, K, vec_table);
    __syncthreads();
    for (int g = 0; g < ncell; g += 8) {
      const int c = c0 + g, f = c / W, t0 = c - f * W;           // 8 columns t0 .. t0 + 7 of row f
      const uint4 *__restrict__ row = reinterpret_cast<const uint4 *>(item + (size_t)f * T);
      const int v0 = (t0 >> 3) + v_base;
      unsigned off[NV * 8];                                       // clamped codes as byte offsets into a table row
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        uint4 raw = make_uint4(0u, 0u, 0u, 0u);                   // past the row: only offsets >= S reach there
        if (valid && v0 + v < v_row) raw = row[v0 + v];
        const unsigned u[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          unsigned x0 = u[e] & 0xFFFFu, x1 = u[e] >> 16;
          x0 = x0 < kmax ? x0 : kmax;
          x1 = x1 < kmax ? x1 : kmax;
          off[v * 8 + 2 * e] = x0 << 2;
          off[v * 8 + 2 * e + 1] = x1 << 2;
        }
      }
      const char *rg = reinterpret_cast<const char *>(rows) + (size_t)g * K4;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int e = 0; e < SS_OB; ++e) {
          if (s_base + b * SS_OB + e < S) {                       // (uniform)
#pragma unroll
            for (int i = 0; i < 8; ++i)
              acc[b * SS_OB + e] += *reinterpret_cast<const float *>(rg + i * K4 + off[(b * SS_OB + e) * STEP + i]);
          }
        }
      }
    }
    __syncthreads();
  }
  if (valid) {
#pragma unroll
    for (int a = 0; a < SS_OB * NB; ++a) {
      const int s = s_base + a;
      if (s < S) store_sum(out, (((size_t)run * Q + j) * S + s) * (size_t)N + n, acc[a], accumulate);
    }
  }
}

// The scalar route: any W, step, shift0, alignment and K.  A pass is 8 offsets; every look-up fetches its own code.
template <bool ROWS>
__global__ __launch_bounds__(SS_THREADS) void code_shift_search_scalar_kernel(
    const uint16_t *__restrict__ codes, const uint16_t *__restrict__ query, const float *__restrict__ weights,
    const float *__restrict__ table, float *__restrict__ out, int64_t N, int F, int T, int W, int shift0, int step, int S, int K,
    int cc, int vec_table, int passes, int accumulate) {
  extern __shared__ float rows[];
  const int tid = (int)threadIdx.x;
  const int pass = (int)(blockIdx.x % (unsigned)passes), run = (int)blockIdx.y, j = (int)blockIdx.z, Q = (int)gridDim.z;
  const int64_t n = (int64_t)(blockIdx.x / (unsigned)passes) * SS_THREADS + tid;
  const bool valid = n < N;
  const int C = F * W, c_begin = run * SS_RUN;
  const int c_end = C - c_begin < SS_RUN ? C : c_begin + SS_RUN;
  const int s_base = pass * SS_OB;
  const uint16_t *__restrict__ qj = ROWS ? nullptr : query + (size_t)j * C;   // (no query on the rows route)
  const float *__restrict__ wj = weights ? weights + (size_t)j * C : nullptr;
  const uint16_t *__restrict__ item = codes + (size_t)(valid ? n : 0) * ((size_t)F * T) + shift0 + (size_t)s_base * step;
  const unsigned kmax = (unsigned)K - 1u;
  float acc[SS_OB];
#pragma unroll
  for (int e = 0; e < SS_OB; ++e) acc[e] = 0.f;
  for (int c0 = c_begin; c0 < c_end; c0 += cc) {
    const int ncell = c_end - c0 < cc ? c_end - c0 : cc;
    if constexpr (ROWS) stage_query_rows<SS_THREADS>(rows, table, wj, j, C, c0, ncell, K, vec_table);
    else stage_code_rows<SS_THREADS>(rows, qj, wj, table, c0, ncell, K, vec_table);
    __syncthreads();
    if (valid) {
      for (int cl = 0; cl < ncell; ++cl) {
        const int c = c0 + cl, f = c / W, t = c - f * W;
        const uint16_t *__restrict__ p = item + (size_t)f * T + t;
        const float *rc = rows + cl * K;
#pragma unroll
        for (int e = 0; e < SS_OB; ++e) {
          if (s_base + e < S) {                                   // (uniform; t + o_s < T for every s < S)
            unsigned x = p[(size_t)e * step];
            x = x < kmax ? x : kmax;
            acc[e] += rc[x];
          }
        }
      }
    }
    __syncthreads();
  }
  if (valid) {
#pragma unroll
    for (int e = 0; e < SS_OB; ++e) {
      const int s = s_base + e;
      if (s < S) store_sum(out, (((size_t)run * Q + j) * S + s) * (size_t)N + n, acc[e], accumulate);
    }
  }
}

__global__ __launch_bounds__(256) void code_shift_reduce_kernel(const float *__restrict__ partial, float *__restrict__ dist,
                                                                int64_t QSN, int runs, int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // (j * S + s) * N + n
  if (i >= QSN) return;
  float s = partial[i];
  for (int r = 1; r < runs; ++r) s += partial[(size_t)r * QSN + i];
  if (accumulate) s = dist[i] + s;
  dist[i] = s;
}

// best[j][n] = min_s dist[j][s][n], best_shift the smallest s that attains it; +inf and -1 where allowed[n] == 0.
__global__ __launch_bounds__(256) void code_shift_best_kernel(const float *__restrict__ dist, const uint8_t *__restrict__ allowed,
                                                              float *__restrict__ best, int32_t *__restrict__ best_shift,
                                                              int64_t N, int S, int64_t QN) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // j * N + n
  if (i >= QN) return;
  const int64_t j = i / N, n = i - j * N;
  if (allowed && !allowed[n]) {
    best[i] = __builtin_inff();
    best_shift[i] = -1;
    return;
  }
  const float *__restrict__ d = dist + (size_t)j * S * N + n;
  float m = d[0];
  int at = 0;
  for (int s = 1; s < S; ++s) {
    const float v = d[(size_t)s * N];
    if (v < m) {                                                  // strict: ties go to the smallest s
      m = v;
      at = s;
    }
  }
  best[i] = m;
  best_shift[i] = at;
}

size_t code_shift_search_workspace_bytes(int64_t N, int F, int T, int W, int S, int K, int Q) {
  if (N <= 0 || F <= 0 || T <= 0 || W <= 0 || S <= 0 || K <= 0 || Q <= 0 || Q > SS_MAX_Q || W > T) return 0;
  if ((int64_t)F * W > SS_MAX_C) return 0;
  const int64_t runs = shift_runs((int64_t)F * W);
  if (runs == 1) return 16;                                       // the search writes dist itself: nothing is staged
  const unsigned __int128 b = (unsigned __int128)runs * (unsigned)Q * (unsigned)S * (unsigned __int128)N * sizeof(float);
  return b > (unsigned __int128)SIZE_MAX ? 0 : (size_t)b;
}

namespace {
// What isi_code_shift_search_f32 and isi_code_shift_search_rows_f32 share: every refusal, the route and the launches.
// by_rows: `source` is window rows [Q, F * W, K] and there is no query; otherwise it is the table [K, K].
int code_shift_search_any(const char *fn, bool by_rows, const uint16_t *codes, const uint16_t *query, const float *weights,
                          const float *source, float *dist, int64_t N, int F, int T, int W, int shift0, int step, int S, int K,
                          int Q, int accumulate, void *workspace, size_t workspace_bytes, hipStream_t st) {
  if (!codes) return refuse(ISI_E_INVALID, fn, "codes is a null pointer");
  if (!by_rows && !query) return refuse(ISI_E_INVALID, fn, "query is a null pointer");
  if (!source) return refuse(ISI_E_INVALID, fn, by_rows ? "rows is a null pointer" : "table is a null pointer");
  if (!dist) return refuse(ISI_E_INVALID, fn, "dist is a null pointer");
  if (!workspace) return refuse(ISI_E_INVALID, fn, "workspace is a null pointer");
  if (N <= 0) return refuse(ISI_E_INVALID, fn, "N must be positive");
  if (F <= 0) return refuse(ISI_E_INVALID, fn, "F must be positive");
  if (T <= 0) return refuse(ISI_E_INVALID, fn, "T must be positive");
  if (W <= 0) return refuse(ISI_E_INVALID, fn, "W must be positive");
  if (S <= 0) return refuse(ISI_E_INVALID, fn, "S must be positive");
  if (K <= 0) return refuse(ISI_E_INVALID, fn, "K must be positive");
  if (step <= 0) return refuse(ISI_E_INVALID, fn, "step must be positive");
  if (shift0 < 0) return refuse(ISI_E_INVALID, fn, "shift0 must not be negative");
  if (W > T) return refuse(ISI_E_INVALID, fn, "W must not exceed T");
  if ((int64_t)shift0 + (int64_t)(S - 1) * step + W > T)
    return refuse(ISI_E_INVALID, fn, "shift0 + (S - 1) * step + W must not exceed T (the last offset leaves the stored map)");
  if (Q < 1 || Q > SS_MAX_Q) return refuse(ISI_E_INVALID, fn, "Q must lie in 1..64");
  if (accumulate != 0 && accumulate != 1) return refuse(ISI_E_INVALID, fn, "accumulate must be 0 or 1");
  if (reinterpret_cast<uintptr_t>(codes) & 1) return refuse(ISI_E_INVALID, fn, "codes must be aligned to 2 bytes");
  if (reinterpret_cast<uintptr_t>(query) & 1) return refuse(ISI_E_INVALID, fn, "query must be aligned to 2 bytes");
  if (reinterpret_cast<uintptr_t>(weights) & 3) return refuse(ISI_E_INVALID, fn, "weights must be aligned to a float");
  if (reinterpret_cast<uintptr_t>(source) & 3)
    return refuse(ISI_E_INVALID, fn, by_rows ? "rows must be aligned to a float" : "table must be aligned to a float");
  if (reinterpret_cast<uintptr_t>(dist) & 3) return refuse(ISI_E_INVALID, fn, "dist must be aligned to a float");
  if (reinterpret_cast<uintptr_t>(workspace) & 3) return refuse(ISI_E_INVALID, fn, "workspace must be aligned to a float");
  if (K > 65535) return refuse(ISI_E_UNSUPPORTED, fn, "K beyond 65535 (stored codes are 16-bit)");
  if (K > SS_MAX_K)
    return refuse(ISI_E_UNSUPPORTED, fn, by_rows ? "K beyond 16384 (one row per staged cell must fit 64 KB of LDS)"
                                                 : "K beyond 16384 (one table row per staged cell must fit 64 KB of LDS)");
  if ((int64_t)F * W > SS_MAX_C) return refuse(ISI_E_UNSUPPORTED, fn, "F * W beyond 256 * 65535 cells");
  if ((int64_t)F * T >= ((int64_t)1 << 31)) return refuse(ISI_E_UNSUPPORTED, fn, "F * T beyond 2^31 - 1 codes per stored map");
  if ((unsigned __int128)N * (unsigned)Q * (unsigned)S >= ((unsigned __int128)1 << 39))
    return refuse(ISI_E_UNSUPPORTED, fn, "Q * S * N beyond 2^39");
  const size_t need = code_shift_search_workspace_bytes(N, F, T, W, S, K, Q);
  if (need == 0) return refuse(ISI_E_UNSUPPORTED, fn, "the workspace size overflows size_t");
  if (workspace_bytes < need) {
    char buf[176];
    snprintf(buf, sizeof buf, "workspace_bytes %zu < %zu (isi_code_shift_search_workspace_bytes)", workspace_bytes, need);
    return refuse(ISI_E_WORKSPACE, fn, buf);
  }
  const int runs = (int)shift_runs((int64_t)F * W);
  const int cc = code_chunk_cells(K);
  const int vec_table = (K % 4) == 0 && !(reinterpret_cast<uintptr_t>(source) & 15);
  const bool vec = (step == 1 || step == 2) && cc >= 8 && (W % 8) == 0 && (T % 8) == 0 && (shift0 % 8) == 0 &&
                   !(reinterpret_cast<uintptr_t>(codes) & 15);
  const int nblk = (S + SS_OB - 1) / SS_OB;
  int passes = nblk, nb = 1;
  if (vec) {
    passes = (nblk + SS_MAX_NB - 1) / SS_MAX_NB;
    const int per = (nblk + passes - 1) / passes;                 // blocks a pass must hold; NB is the next of 1, 2, 4, 7
    nb = per <= 1 ? 1 : per <= 2 ? 2 : per <= 4 ? 4 : 7;
    passes = (nblk + nb - 1) / nb;
  }
  const int64_t gx = (N + SS_THREADS - 1) / SS_THREADS * passes;
  if (gx >= ((int64_t)1 << 31)) return refuse(ISI_E_UNSUPPORTED, fn, "N beyond 2^31 - 1 workgroups of items and offsets along x");
  const size_t lds = (size_t)cc * K * sizeof(float);
  const dim3 grid((unsigned)gx, (unsigned)runs, (unsigned)Q), block(SS_THREADS);
  const bool direct = runs == 1;
  float *out = direct ? dist : static_cast<float *>(workspace);
  const int acc_now = direct ? accumulate : 0;
#define ISI_SS_ARGS codes, query, weights, source, out, N, F, T, W, shift0
#define ISI_SS_LAUNCH(STEP, NB)                                                                                              \
  do {                                                                                                                       \
    if (by_rows)                                                                                                             \
      hipLaunchKernelGGL((code_shift_search_vec_kernel<STEP, NB, true>), grid, block, lds, st, ISI_SS_ARGS, S, K, cc,        \
                         vec_table, passes, acc_now);                                                                        \
    else                                                                                                                     \
      hipLaunchKernelGGL((code_shift_search_vec_kernel<STEP, NB, false>), grid, block, lds, st, ISI_SS_ARGS, S, K, cc,       \
                         vec_table, passes, acc_now);                                                                        \
  } while (0)
  if (!vec) {
    if (by_rows)
      hipLaunchKernelGGL(code_shift_search_scalar_kernel<true>, grid, block, lds, st, ISI_SS_ARGS, step, S, K, cc, vec_table,
                         passes, acc_now);
    else
      hipLaunchKernelGGL(code_shift_search_scalar_kernel<false>, grid, block, lds, st, ISI_SS_ARGS, step, S, K, cc, vec_table,
                         passes, acc_now);
  } else if (step == 1) {
    if (nb == 1) ISI_SS_LAUNCH(1, 1);
    else if (nb == 2) ISI_SS_LAUNCH(1, 2);
    else if (nb == 4) ISI_SS_LAUNCH(1, 4);
    else ISI_SS_LAUNCH(1, 7);
  } else {
    if (nb == 1) ISI_SS_LAUNCH(2, 1);
    else if (nb == 2) ISI_SS_LAUNCH(2, 2);
    else if (nb == 4) ISI_SS_LAUNCH(2, 4);
    else ISI_SS_LAUNCH(2, 7);
  }
#undef ISI_SS_ARGS
#undef ISI_SS_LAUNCH
  if (const int rc = check_launch(fn)) return rc;
  if (direct) return ISI_OK;
  const int64_t QSN = (int64_t)Q * S * N;
  hipLaunchKernelGGL(code_shift_reduce_kernel, dim3((unsigned)((QSN + 255) / 256)), dim3(256), 0, st,
                     static_cast<const float *>(workspace), dist, QSN, runs, accumulate);
  return check_launch(by_rows ? "code_shift_search_rows (reduce)" : "code_shift_search (reduce)");
}
}  // namespace

int code_shift_search_f32(const uint16_t *codes, const uint16_t *query, const float *weights, const float *table, float *dist,
                          int64_t N, int F, int T, int W, int shift0, int step, int S, int K, int Q, int accumulate,
                          void *workspace, size_t workspace_bytes, hipStream_t st) {
  return code_shift_search_any("code_shift_search", false, codes, query, weights, table, dist, N, F, T, W, shift0, step, S, K,
                               Q, accumulate, workspace, workspace_bytes, st);
}

int code_shift_search_rows_f32(const uint16_t *codes, const float *rows, const float *weights, float *dist, int64_t N, int F,
                               int T, int W, int shift0, int step, int S, int K, int Q, int accumulate, void *workspace,
                               size_t workspace_bytes, hipStream_t st) {
  return code_shift_search_any("code_shift_search_rows", true, codes, nullptr, weights, rows, dist, N, F, T, W, shift0, step,
                               S, K, Q, accumulate, workspace, workspace_bytes, st);
}

int code_shift_best_f32(const float *dist, const uint8_t *allowed, float *best, int32_t *best_shift, int64_t N, int S, int Q,
                        hipStream_t st) {
  if (!dist) return invalid("code_shift_best: dist is a null pointer");
  if (!best) return invalid("code_shift_best: best is a null pointer");
  if (!best_shift) return invalid("code_shift_best: best_shift is a null pointer");
  if (N <= 0) return invalid("code_shift_best: N must be positive");
  if (S <= 0) return invalid("code_shift_best: S must be positive");
  if (Q < 1 || Q > SS_MAX_Q) return invalid("code_shift_best: Q must lie in 1..64");
  if (reinterpret_cast<uintptr_t>(dist) & 3) return invalid("code_shift_best: dist must be aligned to a float");
  if (reinterpret_cast<uintptr_t>(best) & 3) return invalid("code_shift_best: best must be aligned to a float");
  if (reinterpret_cast<uintptr_t>(best_shift) & 3) return invalid("code_shift_best: best_shift must be aligned to 4 bytes");
  if ((unsigned __int128)N * (unsigned)Q * (unsigned)S >= ((unsigned __int128)1 << 39))
    return unsupported("code_shift_best: Q * S * N beyond 2^39");
  const int64_t QN = (int64_t)Q * N;
  hipLaunchKernelGGL(code_shift_best_kernel, dim3((unsigned)((QN + 255) / 256)), dim3(256), 0, st, dist, allowed, best,
                     best_shift, N, S, QN);
  return check_launch("code_shift_best");
}

}  // namespace isi
