// Query-by-example search of a code database (gfx950): weighted code-distance sums of Q query codemaps against N stored
// ones.  The arithmetic is this project's own (specification tests/code_search_spec.py):
//   T[a][b]    = sum_d (E[a][d] - E[b][d])^2                     (isi_code_distance_table_f32, fp32, d ascending)
//   dist[j][n] = sum_c w[j][c] * T[query[j][c]][codes[n][c]]     (isi_code_search_f32; query cells >= K count nothing)
//
// Search.  One workgroup (512 threads) owns 512 IPT items of one query and one SPLIT of the cell range (CS_SPLIT = 256
// consecutive cells).  It walks the split in chunks of `cc` cells: the chunk's table rows, already multiplied by the
// cell's weight (rows[cl][k] = w[c] * T[query[c]][k], one rounding; zeros for a mask-token cell), are staged in LDS -- K
// floats per cell, 64 KB per workgroup, two workgroups per CU -- and every lane then adds rows[cl][codes[n][c]] for its
// own items, c ascending, into one fp32 register per item.  An item's codes are fetched into registers BEFORE the stage
// is written.  At K <= 512 (32-cell chunks) a lane fetches the codes of TWO chunks at once -- the 128 bytes of a whole
// cache line of its item's row -- for IPT = 2 items; measured against one chunk at a time with IPT = 4: 3-5 % faster on
// the large cases, 26 % on the top maps with one query (twice as many workgroups in the launch's last wave).
// The look-ups are random 4-byte LDS reads: a ds_read_b32 serves 2 groups of 32 lanes over 32 banks.  Per-split sums go
// to the workspace [splits][Q][N]; a second kernel adds them, split ascending, and applies `allowed` and `accumulate`.
// The order of every addition is a function of C and the cell index alone: no atomics, and dist[j][n] has the same
// bits whatever N, Q, the item's place in the launch or the route the codes were read by.
//
// Limits: K <= 16384 (one table row per staged cell must fit the 64 KB stage), C <= 256 * 65535 (splits ride grid.y),
// Q <= 64 (grid.z).  Codes are read as 16-byte vectors when C % 8 == 0, the base is 16-byte aligned and K <= 2048 (a
// chunk then holds a multiple of 8 cells), one by one otherwise; table rows as float4 when K % 4 == 0 and the base is
// 16-byte aligned.  A stored code >= K is clamped to K - 1: nothing is read outside the stage.
//
// Search by encoder vectors (specification tests/code_soft_search_spec.py).  Nothing in the look-up
// cares where a staged row came from: isi_code_search_rows_f32 runs the same kernel with the stage fed from per-cell rows
// R [Q][C][K] (template argument ROWS; a zero weight stages zeros), and isi_code_query_rows_f32 builds such rows from
// vectors, R[c][k] = sum_d (z[c][d] - E[k][d])^2 -- the table's expression, so vectors that are codebook rows give the
// table's rows and the hard search's distances bit for bit.
#include "isi_common.h"
#include "isi_internal.h"
#include "device_prims.h"

namespace isi {

namespace {
constexpr int CS_THREADS = 512;
constexpr int CS_IPT = 4;                          // items per thread (2 on the whole-line route)
constexpr int CS_SPLIT = 256;                      // cells per split: a function of nothing, so the summation order is C's alone
constexpr int CS_MAX_CHUNK = 32;                   // cells per chunk at most (a multiple of 8 divides CS_SPLIT)
constexpr int CS_MAX_K = kCodeStageFloats;
constexpr int64_t CS_MAX_C = (int64_t)CS_SPLIT * 65535;
constexpr int CS_MAX_Q = 64;

int64_t num_splits(int64_t C) { return (C + CS_SPLIT - 1) / CS_SPLIT; }
}  // namespace

__global__ __launch_bounds__(256) void code_distance_table_kernel(const float *__restrict__ E, float *__restrict__ T, int K,
                                                                  int D) {
  const int b = (int)(blockIdx.x * 256 + threadIdx.x), a = (int)blockIdx.y;
  if (b >= K) return;
  const float *__restrict__ ea = E + (size_t)a * D, *__restrict__ eb = E + (size_t)b * D;
  float acc = 0.f;
  for (int d = 0; d < D; ++d) {
    const float diff = ea[d] - eb[d];              // (a, b) and (b, a): the same square, the same order -> the same bits
    acc = fmaf(diff, diff, acc);
  }
  T[(size_t)a * K + b] = acc;
}

// Rows of a query given as vectors: R[c][k] = sum_d (z[c][d] - E[k][d])^2 -- the table kernel's expression with the query
// on the `a` side, d ascending, one fma per d, so a vector that IS codebook row a gives T[a][:] bit for bit.  One workgroup
// (256 threads) owns QR_CELLS cells x 256 codes: lane k keeps one accumulator per cell and walks d in chunks of QR_D.  A
// chunk of the codebook tile is staged transposed, Et[d][k] with a row stride of 257 floats (the transposing writes and the
// lane-per-code reads are both conflict-free); the cells' vectors are staged as they lie and read back as uniform 16-byte
// broadcasts.  d beyond D is staged as 0 on both sides: fma(0, 0, acc) == acc for every acc this sum can hold (never -0).
// The stores of one cell are 256 consecutive floats of its row.
constexpr int QR_THREADS = 256;
constexpr int QR_CELLS = 32;
constexpr int QR_D = 32;
constexpr int QR_ESTRIDE = QR_THREADS + 1;

__global__ __launch_bounds__(QR_THREADS) void code_query_rows_kernel(const float *__restrict__ z, int64_t z_stride,
                                                                     const float *__restrict__ E, float *__restrict__ R,
                                                                     int64_t cells, int K, int D) {
  __shared__ float Et[QR_D * QR_ESTRIDE];
  __shared__ float4 zs[QR_CELLS * (QR_D / 4)];
  const int tid = (int)threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * QR_CELLS;
  const int k0 = (int)blockIdx.y * QR_THREADS;
  float acc[QR_CELLS];
#pragma unroll
  for (int cl = 0; cl < QR_CELLS; ++cl) acc[cl] = 0.f;
  for (int d0 = 0; d0 < D; d0 += QR_D) {
#pragma unroll 4
    for (int i = 0; i < QR_D; ++i) {                 // 256 codes x 32 d: a wave reads two 128-byte pieces of two codes
      const int idx = i * QR_THREADS + tid, kk = idx / QR_D, dd = idx % QR_D;
      float v = 0.f;
      if (k0 + kk < K && d0 + dd < D) v = E[(size_t)(k0 + kk) * D + d0 + dd];
      Et[dd * QR_ESTRIDE + kk] = v;
    }
#pragma unroll
    for (int i = 0; i < QR_CELLS * QR_D / QR_THREADS; ++i) {
      const int idx = i * QR_THREADS + tid, cl = idx / QR_D, dd = idx % QR_D;
      float v = 0.f;
      if (c0 + cl < cells && d0 + dd < D) v = z[(size_t)(c0 + cl) * (size_t)z_stride + d0 + dd];
      reinterpret_cast<float *>(zs)[cl * QR_D + dd] = v;
    }
    __syncthreads();
    for (int d4 = 0; d4 < QR_D / 4; ++d4) {
      const float e0 = Et[(4 * d4 + 0) * QR_ESTRIDE + tid], e1 = Et[(4 * d4 + 1) * QR_ESTRIDE + tid];
      const float e2 = Et[(4 * d4 + 2) * QR_ESTRIDE + tid], e3 = Et[(4 * d4 + 3) * QR_ESTRIDE + tid];
#pragma unroll
      for (int cl = 0; cl < QR_CELLS; ++cl) {
        const float4 zv = zs[cl * (QR_D / 4) + d4];
        float diff = zv.x - e0;
        acc[cl] = fmaf(diff, diff, acc[cl]);
        diff = zv.y - e1;
        acc[cl] = fmaf(diff, diff, acc[cl]);
        diff = zv.z - e2;
        acc[cl] = fmaf(diff, diff, acc[cl]);
        diff = zv.w - e3;
        acc[cl] = fmaf(diff, diff, acc[cl]);
      }
    }
    __syncthreads();
  }
  if (k0 + tid < K) {
#pragma unroll
    for (int cl = 0; cl < QR_CELLS; ++cl)
      if (c0 + cl < cells) R[(size_t)(c0 + cl) * (size_t)K + k0 + tid] = acc[cl];
  }
}

// G > 0: chunks of 8 G cells, an item's codes read as 16-byte vectors, SUB chunks' worth at a time (SUB = 2 at G = 4: the
// 128 bytes of a whole cache line per item); G == 0: chunks of cc cells, codes read one by one inside the look-up loop.
// ROWS: `table` holds per-cell rows R [Q][C][K] (isi_code_search_rows_f32) and `query` is unused; only the stage differs.
template <int G, int IPT, int SUB, bool ROWS>
__global__ __launch_bounds__(CS_THREADS) void code_search_kernel(const uint16_t *__restrict__ codes,
                                                                 const uint16_t *__restrict__ query,
                                                                 const float *__restrict__ weights,
                                                                 const float *__restrict__ table, float *__restrict__ partial,
                                                                 int64_t N, int C, int K, int cc, int vec_table) {
  extern __shared__ float rows[];                   // [cc][K]
  constexpr int NV = G > 0 ? G * SUB : 1;
  const int tid = (int)threadIdx.x;
  const int split = (int)blockIdx.y, j = (int)blockIdx.z, Q = (int)gridDim.z;
  const int64_t n0 = (int64_t)blockIdx.x * (CS_THREADS * IPT) + tid;
  const int c_begin = split * CS_SPLIT;
  const int c_end = C - c_begin < CS_SPLIT ? C : c_begin + CS_SPLIT;
  const uint16_t *__restrict__ qj = ROWS ? nullptr : query + (size_t)j * C;   // (no query on the rows route)
  const float *__restrict__ wj = weights ? weights + (size_t)j * C : nullptr;
  const unsigned kmax = (unsigned)K - 1u;
  if (G > 0) cc = 8 * G;
  float acc[IPT];
#pragma unroll
  for (int it = 0; it < IPT; ++it) acc[it] = 0.f;
  for (int cb = c_begin; cb < c_end; cb += cc * SUB) {
    uint4 v[IPT][NV];
    if (G > 0) {
#pragma unroll
      for (int it = 0; it < IPT; ++it) {
        const int64_t n = n0 + (int64_t)it * CS_THREADS;
#pragma unroll
        for (int g = 0; g < NV; ++g) {
          v[it][g] = make_uint4(0u, 0u, 0u, 0u);
          if (n < N && cb + 8 * g < c_end) v[it][g] = *reinterpret_cast<const uint4 *>(codes + (size_t)n * C + cb + 8 * g);
        }
      }
    }
#pragma unroll
    for (int sub = 0; sub < SUB; ++sub) {
      const int c0 = cb + sub * cc;
      if (c0 >= c_end) break;
      const int ncell = c_end - c0 < cc ? c_end - c0 : cc;
      if constexpr (ROWS) stage_query_rows<CS_THREADS>(rows, table, wj, j, C, c0, ncell, K, vec_table);
      else stage_code_rows<CS_THREADS>(rows, qj, wj, table, c0, ncell, K, vec_table);
      __syncthreads();
      if (G > 0) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
          if (8 * g < ncell) {                      // (ncell is a multiple of 8 on this route)
            const float *rg = rows + 8 * g * K;
#pragma unroll
            for (int it = 0; it < IPT; ++it) {
              const uint4 vv = v[it][sub * G + g];
              const unsigned u[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                unsigned x0 = u[e] & 0xFFFFu, x1 = u[e] >> 16;
                x0 = x0 < kmax ? x0 : kmax;
                x1 = x1 < kmax ? x1 : kmax;
                acc[it] += rg[(2 * e) * K + x0];
                acc[it] += rg[(2 * e + 1) * K + x1];
              }
            }
          }
        }
      } else {
#pragma unroll
        for (int it = 0; it < IPT; ++it) {
          const int64_t n = n0 + (int64_t)it * CS_THREADS;
          if (n < N) {
            const uint16_t *__restrict__ cn = codes + (size_t)n * C + c0;
            for (int cl = 0; cl < ncell; ++cl) {
              unsigned x = cn[cl];
              x = x < kmax ? x : kmax;
              acc[it] += rows[cl * K + x];
            }
          }
        }
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int it = 0; it < IPT; ++it) {
    const int64_t n = n0 + (int64_t)it * CS_THREADS;
    if (n < N) partial[((size_t)split * Q + j) * N + n] = acc[it];
  }
}

__global__ __launch_bounds__(256) void code_search_reduce_kernel(const float *__restrict__ partial,
                                                                 const uint8_t *__restrict__ allowed, float *__restrict__ dist,
                                                                 int64_t N, int64_t QN, int splits, int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // j * N + n
  if (i >= QN) return;
  float s = partial[i];
  for (int sp = 1; sp < splits; ++sp) s += partial[(size_t)sp * QN + i];
  if (accumulate) s = dist[i] + s;
  if (allowed && !allowed[i % N]) s = __builtin_inff();
  dist[i] = s;
}

int code_distance_table_f32(const float *codebook, float *table, int K, int D, hipStream_t st) {
  if (!codebook) return invalid("code_distance_table: codebook is a null pointer");
  if (!table) return invalid("code_distance_table: table is a null pointer");
  if (K <= 0) return invalid("code_distance_table: K must be positive");
  if (D <= 0) return invalid("code_distance_table: D must be positive");
  if (reinterpret_cast<uintptr_t>(codebook) & 3) return invalid("code_distance_table: codebook must be aligned to a float");
  if (reinterpret_cast<uintptr_t>(table) & 3) return invalid("code_distance_table: table must be aligned to a float");
  if (K > 65535) return unsupported("code_distance_table: K beyond 65535 (stored codes are 16-bit)");
  const dim3 grid((unsigned)((K + 255) / 256), (unsigned)K), block(256);
  hipLaunchKernelGGL(code_distance_table_kernel, grid, block, 0, st, codebook, table, K, D);
  return check_launch("code_distance_table");
}

int code_query_rows_f32(const float *z, int64_t z_stride, const float *codebook, float *rows, int64_t cells, int K, int D,
                        hipStream_t st) {
  if (!z) return invalid("code_query_rows: z is a null pointer");
  if (!codebook) return invalid("code_query_rows: codebook is a null pointer");
  if (!rows) return invalid("code_query_rows: rows is a null pointer");
  if (cells <= 0) return invalid("code_query_rows: cells must be positive");
  if (K <= 0) return invalid("code_query_rows: K must be positive");
  if (D <= 0) return invalid("code_query_rows: D must be positive");
  if (z_stride < D) return invalid("code_query_rows: z_stride must be at least D");
  if (reinterpret_cast<uintptr_t>(z) & 3) return invalid("code_query_rows: z must be aligned to a float");
  if (reinterpret_cast<uintptr_t>(codebook) & 3) return invalid("code_query_rows: codebook must be aligned to a float");
  if (reinterpret_cast<uintptr_t>(rows) & 3) return invalid("code_query_rows: rows must be aligned to a float");
  if (K > 65535) return unsupported("code_query_rows: K beyond 65535 (stored codes are 16-bit)");
  if ((unsigned __int128)cells * (unsigned)K >= ((unsigned __int128)1 << 39))
    return unsupported("code_query_rows: cells * K beyond 2^39");
  if ((cells + QR_CELLS - 1) / QR_CELLS >= ((int64_t)1 << 31))
    return unsupported("code_query_rows: cells beyond 2^31 - 1 workgroups of 32");
  if ((unsigned __int128)cells * (unsigned __int128)z_stride >= ((unsigned __int128)1 << 62))
    return unsupported("code_query_rows: cells * z_stride beyond 2^62");
  const dim3 grid((unsigned)((cells + QR_CELLS - 1) / QR_CELLS), (unsigned)((K + QR_THREADS - 1) / QR_THREADS)), block(QR_THREADS);
  hipLaunchKernelGGL(code_query_rows_kernel, grid, block, 0, st, z, z_stride, codebook, rows, cells, K, D);
  return check_launch("code_query_rows");
}

size_t code_search_workspace_bytes(int64_t N, int64_t C, int K, int Q) {
  if (N <= 0 || C <= 0 || K <= 0 || Q <= 0 || Q > CS_MAX_Q || C > CS_MAX_C) return 0;
  const unsigned __int128 b = (unsigned __int128)num_splits(C) * (unsigned)Q * (unsigned __int128)N * sizeof(float);
  return b > (unsigned __int128)SIZE_MAX ? 0 : (size_t)b;
}

namespace {
// What isi_code_search_f32 and isi_code_search_rows_f32 share: every refusal, the route and the two launches.  by_rows:
// `source` is rows [Q, C, K] and there is no query; otherwise it is the table [K, K].
int code_search_any(const char *fn, bool by_rows, const uint16_t *codes, const uint16_t *query, const float *weights,
                    const float *source, const uint8_t *allowed, float *dist, int64_t N, int64_t C, int K, int Q,
                    int accumulate, void *workspace, size_t workspace_bytes, hipStream_t st) {
  if (!codes) return refuse(ISI_E_INVALID, fn, "codes is a null pointer");
  if (!by_rows && !query) return refuse(ISI_E_INVALID, fn, "query is a null pointer");
  if (!source) return refuse(ISI_E_INVALID, fn, by_rows ? "rows is a null pointer" : "table is a null pointer");
  if (!dist) return refuse(ISI_E_INVALID, fn, "dist is a null pointer");
  if (!workspace) return refuse(ISI_E_INVALID, fn, "workspace is a null pointer");
  if (N <= 0) return refuse(ISI_E_INVALID, fn, "N must be positive");
  if (C <= 0) return refuse(ISI_E_INVALID, fn, "C must be positive");
  if (K <= 0) return refuse(ISI_E_INVALID, fn, "K must be positive");
  if (Q < 1 || Q > CS_MAX_Q) return refuse(ISI_E_INVALID, fn, "Q must lie in 1..64");
  if (accumulate != 0 && accumulate != 1) return refuse(ISI_E_INVALID, fn, "accumulate must be 0 or 1");
  if (reinterpret_cast<uintptr_t>(codes) & 1) return refuse(ISI_E_INVALID, fn, "codes must be aligned to 2 bytes");
  if (reinterpret_cast<uintptr_t>(query) & 1) return refuse(ISI_E_INVALID, fn, "query must be aligned to 2 bytes");
  if (reinterpret_cast<uintptr_t>(weights) & 3) return refuse(ISI_E_INVALID, fn, "weights must be aligned to a float");
  if (reinterpret_cast<uintptr_t>(source) & 3)
    return refuse(ISI_E_INVALID, fn, by_rows ? "rows must be aligned to a float" : "table must be aligned to a float");
  if (reinterpret_cast<uintptr_t>(dist) & 3) return refuse(ISI_E_INVALID, fn, "dist must be aligned to a float");
  if (reinterpret_cast<uintptr_t>(workspace) & 3) return refuse(ISI_E_INVALID, fn, "workspace must be aligned to a float");
  if (K > 65535) return refuse(ISI_E_UNSUPPORTED, fn, "K beyond 65535 (stored codes are 16-bit)");
  if (K > CS_MAX_K)
    return refuse(ISI_E_UNSUPPORTED, fn, by_rows ? "K beyond 16384 (one row per staged cell must fit 64 KB of LDS)"
                                                 : "K beyond 16384 (one table row per staged cell must fit 64 KB of LDS)");
  if (C > CS_MAX_C) return refuse(ISI_E_UNSUPPORTED, fn, "C beyond 256 * 65535 cells");
  if ((N + CS_THREADS - 1) / CS_THREADS >= ((int64_t)1 << 31) || (unsigned __int128)N * (unsigned)Q >= ((unsigned __int128)1 << 39))
    return refuse(ISI_E_UNSUPPORTED, fn, "N beyond 2^31 workgroups of items or Q * N beyond 2^39");
  const size_t need = code_search_workspace_bytes(N, C, K, Q);
  if (need == 0) return refuse(ISI_E_UNSUPPORTED, fn, "the workspace size overflows size_t");
  if (workspace_bytes < need) {
    char buf[160];
    snprintf(buf, sizeof buf, "workspace_bytes %zu < %zu (isi_code_search_workspace_bytes)", workspace_bytes, need);
    return refuse(ISI_E_WORKSPACE, fn, buf);
  }
  const int splits = (int)num_splits(C);
  const int cc = code_chunk_cells(K);
  const bool vec_codes = cc >= 8 && (C % 8) == 0 && !(reinterpret_cast<uintptr_t>(codes) & 15);
  const int vec_table = (K % 4) == 0 && !(reinterpret_cast<uintptr_t>(source) & 15);
  const size_t lds = (size_t)cc * K * sizeof(float);
  const bool lines = vec_codes && cc == CS_MAX_CHUNK;                  // two chunks = the 128 bytes of a whole line per item
  const int ipt = lines ? 2 : CS_IPT;
  const int64_t blocks = (N + CS_THREADS * ipt - 1) / (CS_THREADS * ipt);
  const dim3 grid((unsigned)blocks, (unsigned)splits, (unsigned)Q), block(CS_THREADS);
  float *partial = static_cast<float *>(workspace);
  const int Ci = (int)C;
#define ISI_CS_LAUNCH(G, IPT, SUB)                                                                                         \
  do {                                                                                                                     \
    if (by_rows)                                                                                                           \
      hipLaunchKernelGGL((code_search_kernel<G, IPT, SUB, true>), grid, block, lds, st, codes, query, weights, source,     \
                         partial, N, Ci, K, cc, vec_table);                                                                \
    else                                                                                                                   \
      hipLaunchKernelGGL((code_search_kernel<G, IPT, SUB, false>), grid, block, lds, st, codes, query, weights, source,    \
                         partial, N, Ci, K, cc, vec_table);                                                                \
  } while (0)
  if (!vec_codes) ISI_CS_LAUNCH(0, CS_IPT, 1);
  else if (lines) ISI_CS_LAUNCH(4, 2, 2);
  else if (cc == 24) ISI_CS_LAUNCH(3, CS_IPT, 1);
  else if (cc == 16) ISI_CS_LAUNCH(2, CS_IPT, 1);
  else ISI_CS_LAUNCH(1, CS_IPT, 1);
#undef ISI_CS_LAUNCH
  if (const int rc = check_launch(fn)) return rc;
  const int64_t QN = (int64_t)Q * N;
  hipLaunchKernelGGL(code_search_reduce_kernel, dim3((unsigned)((QN + 255) / 256)), dim3(256), 0, st, partial, allowed, dist,
                     N, QN, splits, accumulate);
  return check_launch(by_rows ? "code_search_rows (reduce)" : "code_search (reduce)");
}
}  // namespace

int code_search_f32(const uint16_t *codes, const uint16_t *query, const float *weights, const float *table,
                    const uint8_t *allowed, float *dist, int64_t N, int64_t C, int K, int Q, int accumulate, void *workspace,
                    size_t workspace_bytes, hipStream_t st) {
  return code_search_any("code_search", false, codes, query, weights, table, allowed, dist, N, C, K, Q, accumulate, workspace,
                         workspace_bytes, st);
}

int code_search_rows_f32(const uint16_t *codes, const float *rows, const float *weights, const uint8_t *allowed, float *dist,
                         int64_t N, int64_t C, int K, int Q, int accumulate, void *workspace, size_t workspace_bytes,
                         hipStream_t st) {
  return code_search_any("code_search_rows", true, codes, nullptr, weights, rows, allowed, dist, N, C, K, Q, accumulate,
                         workspace, workspace_bytes, st);
}

}  // namespace isi
