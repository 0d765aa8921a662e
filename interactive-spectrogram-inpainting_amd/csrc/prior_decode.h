// What the decoding loop's host plan (prior_sample_run.cpp) and its kernels (prior_decode.hip) share: the kernels' argument
// blocks, the constants the plan sizes things by, and one launcher per kernel family.  The plan never names a kernel; a
// launcher picks the template instantiation from its arguments and owns that kernel's one-time set-up.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace isi {

constexpr int MF_KC = 512;     // K chunk of a matrix tile (row_mfma32_kernel): longer rows are summed from partial products
constexpr int SS_RS = 16;      // floats per lane of a row held in registers: d <= 1024 (single_source_cross_kernel)
constexpr int SS_ROWS = 4;     // rows per workgroup, one per wave

// The argument block of the row kernels.  A KERNEL ARGUMENT: its layout is part of the device code.
struct RowLinArgs {
  const float *x; int x_stride;            // [M, K] input rows (pre-norm when ln_g)
  const float *ln_g, *ln_b;                // LayerNorm applied to x rows (nullable)
  const float *W, *bias;                   // [N, K] torch layout
  const float *res; int res_stride;        // [M, N] residual rows (nullable)
  const float *res_g, *res_b;              // LayerNorm applied to the residual rows (nullable)
  float *out; int out_stride;              // columns [0, split)
  float *out2; int out2_stride;            // columns [split, N) (nullable: split == N)
  int split, M, N, K, relu;
  float eps;
  // replayable launches (hipGraph): with pos != nullptr, x / res / out2 advance by these element
  // counts per sequence position read from device memory
  const int *pos;
  long x_pos, res_pos, out2_pos;
  // batched decoding on matrix tiles (row_mfma32_kernel): a pre-norm row is normalised by two launches of a position -- as the
  // INPUT of a projection and, one launch later, as the RESIDUAL of the out-projection / second feed-forward layer.  The
  // first writes the rows' statistics here ([M][2]: mean, 1 / std), the second reads them instead of loading the 32 x N
  // residual rows again in every workgroup and reducing them (6 % of a decoding step at B = 32, measured by ablation)
  float *stat_out;
  const float *res_stat;
  // ragged batches (isi_prior_sample_run_rows; the RAG instantiations): row m stands at position row_pos[t * M + m] of step
  // t = *pos (replayable) or t = 0 (row_pos already offset to the step), and x / res / out2 of row m advance by that
  // position times x_pos / res_pos / out2_pos
  const int *row_pos;
  // 16-bit key/value cache (isi_prior_state.kv_format = ISI_KV_BF16): out2 points at a bf16 array -- out2_stride / out2_pos still
  // count elements -- and the epilogue rounds to nearest-even as it stores (the KV16 instantiations; the launchers pick them
  // by this flag, the fp32 instantiations are the code they were)
  int out2_bf16;
};
static_assert(sizeof(RowLinArgs) == 200, "RowLinArgs is a kernel argument block: its layout must not change");

// The argument block of single_source_cross_kernel (isi_prior_state.cross_out).  A kernel argument like RowLinArgs.
struct SingleSourceArgs {
  const float *y1;             // [B, d] pre-norm rows
  const float *ln_g, *ln_b;    // LN1
  const float *table;          // this layer's [S_src, B, d]
  float *y2;                   // [B, d]
  float *stat_out;             // [B][2] mean, 1 / std of the y2 rows (nullable)
  const int *pos;              // replayable launches: the position from device memory (else `p`)
  int p, Cd, S_src, B, d;
  float eps;
  const int *row_pos;          // RAG: row m at position row_pos[t * B + m], t = *pos or 0 (RowLinArgs.row_pos)
  int table_B, table_sb;       // rows per source position of the table and the step between batch rows: (B, 1), or (1, 0) when
                               // all rows share one source (isi_prior_state.memory_shared)
};
static_assert(sizeof(SingleSourceArgs) == 96, "SingleSourceArgs is a kernel argument block: its layout must not change");

// LDS of row_linear_ln_kernel for M <= 8 rows of K floats: the rows at the kernel's row capacity (template MR: 1, 2, 4 or 8)
// and their statistics.  launch_row_linear_8 refuses what exceeds kRowLinearLdsMax
constexpr size_t kRowLinearLdsMax = 160 * 1024;
inline size_t row_linear_lds_bytes(int M, int K) {
  const int mr = M <= 1 ? 1 : M <= 2 ? 2 : M <= 4 ? 4 : 8;
  return ((size_t)mr * K + 2 * mr) * sizeof(float);
}
// rows of a group of row_gemvm_kernel for kq float4 per lane and row (prior_sample_run.cpp)
int row_gemvm_group(int M, int kq);

// ---- launchers (prior_decode.hip).  Ragged addressing is chosen by a.row_pos, the bf16 epilogue by a.out2 && a.out2_bf16.
// one row; `part` != nullptr: the input row is the merge of an attention's key-split partials [K / HD heads][NS][HD + 4]
int launch_row_gemv1(const RowLinArgs &a, const float *part, int NS, int HD, hipStream_t st);
// 2 .. 256 rows held in registers, in groups (row_gemvm_supported)
int launch_row_gemvm(const RowLinArgs &a, hipStream_t st);
// 32-row matrix tiles; K > MF_KC on few tiles: partial products into ksplit_ws and a finishing launch
int launch_row_mfma(const RowLinArgs &a, hipStream_t st, float *ksplit_ws, size_t ksplit_floats);
// up to 8 rows staged in LDS
int launch_row_linear_8(const RowLinArgs &a, hipStream_t st);
int launch_single_source_cross(const SingleSourceArgs &a, hipStream_t st);
// *pos = add ? *pos + value : value
int launch_set_pos(int *pos, int value, int add, hipStream_t st);

}  // namespace isi
