// Internal (C++-linkage) entry points behind the extern "C" API of isi_api.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include "isi_hip.h"

namespace isi {

int split_conv_weight_f16(const float *packed, float *out, int64_t n_floats, hipStream_t stream);
int pad_channels4_f32(const float *x, float *out, int B, int C, int H, int W, int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                      hipStream_t st);
int add_gate_rows_f32(float *out, const float *a, int64_t lda, const float *b, const float *y, int64_t M, int C, hipStream_t st);
int vq_bwd_rows_f32(float *dz, const float *dq, int64_t ldq, const float *z, const float *q_st, const float *g_diff, int64_t M,
                    int D, hipStream_t st);
int pack_multi(const void *table_dev, int n, int blocks_per_entry, hipStream_t stream);
bool conv_wgrad_halo_route(int Cout, int C0, int C1, int KH, int KW, int stride, int pad, int OH, int OW);
int reduce_jobs_f32(const isi_reduce_job *jobs, int n_jobs, hipStream_t stream);
// optimizer.hip
int64_t adam_num_chunks(const isi_adam_tensor *tensors, int n_tensors);
int grad_sumsq_f32(const isi_adam_tensor *tensors, int n_tensors, float *partials, int64_t n_partials, hipStream_t stream);
int grad_clip_coef_f32(const float *partials, int64_t n_partials, float max_norm, float *norm_coef, hipStream_t stream);
int adam_step_f32(const isi_adam_tensor *tensors, int n_tensors, const isi_adam_hyper *hyper, int n_groups, const float *coef,
                  hipStream_t stream);
int conv_wgrad_deferred_f32(const isi_src *s0, const isi_src *s1, const float *dy, float *dw, int cin_keep, float *db,
                            float *workspace, size_t workspace_floats, int B, int H, int W, int Cout, int KH, int KW, int stride,
                            int pad, int flags, hipStream_t stream, isi_reduce_job *jobs_out, int *n_jobs);
int pair_encode_f32(const float *x, float *out, int64_t n, hipStream_t stream);
int pair_decode_f32(const float *in, float *x, int64_t n, hipStream_t stream);
bool conv_first_applicable(const isi_src *s0, const isi_src *s1, const isi_src *res, const isi_dst *dst, int Cout,
                           int KH, int KW, int stride, int pad, int OH, int OW, int nz);
int conv_first_f32(const isi_src *s0, const float *packed_w, const float *bias, const isi_dst *dst, int B, int H,
                   int W, int Cout, int OH, int OW, int64_t in_extent, int flags, hipStream_t stream, float *twin = nullptr,
                   const float *gate = nullptr, int32_t *zero = nullptr, int zero_words = 0);
bool conv_pair_sources_ok(int C0, int C1, int Cout, int taps);
// conv_pair_f16.hip: the LDS-DMA implicit-GEMM kernel of the pair pipeline (pair8 sources, blocked W16 weights)
struct PairConvArgs {
  const float *in0, *in1, *w16, *bias;
  float *out;
  unsigned in0_bytes, in1_bytes, w_bytes, out_bytes;
  int C0, C1;
  int s0n, s0h, s0w, s1n, s1h, s1w;    // source element strides (channel stride 1)
  int on, oh, ow;                      // output strides in GEMM-grid pixels (channel stride 1)
  int H, W, OH, OW, Cout, Kpad, KH, KW, stride, pad, relu, M;
  int convT, w_phase_stride, dst_sh, dst_sw;
  int out_pair;
  float *twin;                         // with out_pair: dense channels-last fp32 copy of the output (training tape), or null
};
bool conv_pair_kernel_ok(int C0, int C1, int Cout, int taps);
int conv_pair_f16(const PairConvArgs &c, hipStream_t stream);
int conv_pair_debug_stamps(long long *host, int n);
// convT_pair_f16.hip: ConvTranspose2d(k4,s2,p1) of the pair pipeline with the output phases fused on one staged tile
bool convT_pair_ok(int Cin, int Cout);
bool decoder_tail_ok(int Cin, int Cmid, int Cout);
int decoder_tail_f32(const float *in_pair, const float *packed_w1, const float *bias1, const float *packed_w2,
                     const float *bias2, float *yprime_ws, const isi_dst *dst, int B, int H, int W, int Cin, int Cmid,
                     int Cout, hipStream_t stream);
int convT_pair_debug_stamps(long long *host, int n);
int convT_pair_f16(const float *in, const float *w16, const float *bias, float *out, int B, int H, int W, int Cin,
                   int Cout, int relu, int out_pair, hipStream_t stream, const float *w2 = nullptr, int n2 = 0,
                   float *twin = nullptr);
int conv2d_f32(const isi_src *s0, const isi_src *s1, const float *packed_w, const float *bias,
               const isi_src *res, const isi_dst *dst, int B, int H, int W, int Cout, int KH,
               int KW, int stride, int pad, int relu, hipStream_t stream, const float *gate = nullptr,
               float *twin = nullptr, int32_t *zero = nullptr, int zero_words = 0);
int conv2d_batched_f32(const isi_src *s0, const isi_src *s1, const float *packed_w, const float *bias,
                       const isi_src *res, const isi_dst *dst, int B, int H, int W, int Cout, int KH,
                       int KW, int stride, int pad, int relu, int nz, int64_t zs_in0, int64_t zs_w,
                       int64_t zs_res, int64_t zs_out, hipStream_t stream, const float *gate = nullptr,
                       float *twin = nullptr, int32_t *zero = nullptr, int zero_words = 0);
// (zero / zero_words: int32 words the launch clears for LATER launches of the stream -- by workgroup 0 of the 2-channel
// first-layer kernel, by a launch of their own in front of any other kernel)
int conv_transpose2d_k4s2_f32(const isi_src *s, const float *packed_w, const float *bias,
                              const isi_dst *dst, int B, int H, int W, int Cout, int relu,
                              hipStream_t stream, const float *gate = nullptr, float *twin = nullptr);
// isi_conv2d_route / isi_conv_transpose2d_k4s2_route: the validation and planning of the two calls above (one code path),
// nothing launched; the packed route (ISI_CONV_ROUTE_*, include/isi_hip.h) or the negative status of a refusal
int conv2d_route(const isi_src *s0, const isi_src *s1, const float *packed_w, const float *bias, const isi_src *res,
                 const isi_dst *dst, int B, int H, int W, int Cout, int KH, int KW, int stride, int pad, int relu,
                 const float *gate);
int conv_transpose2d_k4s2_route(const isi_src *s, const float *packed_w, const float *bias, const isi_dst *dst, int B, int H,
                                int W, int Cout, int relu, const float *gate);

bool resblock_fusable(int C, int R);
bool resblock_pair_ok(int C, int R);
bool resblock_pair_preferred(int B, int H, int W, int C, int R);
int resblock_pair_debug_stamps(long long *host, int n);
int resblock_pair_f16(const float *in, const float *w1_16, const float *b1, const float *w2_16, const float *b2, float *out,
                      int B, int H, int W, int C, int relu, int out_pair, hipStream_t stream, float *twin = nullptr,
                      float *hidden = nullptr);
int resblock_f32(const float *in, const float *w1, const float *b1, const float *w2, const float *b2,
                 float *out, int B, int H, int W, int C, int R, int relu, hipStream_t stream, float *twin = nullptr,
                 float *hidden = nullptr);
bool convT_small_applicable(int Cin, int Cout);
bool convT_small_pair_ok(int Cin, int Cout);
int convT_gather_f32(const float *yprime, const float *bias, float *out, int B, int H, int W, int Cout, int on, int oc,
                     int oh, int ow, int relu, hipStream_t stream);
int convT_k4s2_small_pair_f16(const float *in, const float *wn, const float *bias, float *out, int B, int H, int W,
                              int Cin, int Cout, int on, int oc, int oh, int ow, int relu, hipStream_t stream);
int pack_convT_small_weight_f32(const float *w, float *packed, int Cin, int Cout, hipStream_t stream);
int convT_k4s2_small_f32(const float *in, const float *wk, const float *bias, float *out, int B, int H,
                         int W, int Cin, int Cout, int64_t in_elems, int sn, int sc, int sh, int sw, int on,
                         int oc, int oh, int ow, int relu, hipStream_t stream);

int rel_attention_f32(const isi_attn_args *g, hipStream_t stream);
size_t rel_attention_workspace_bytes(const isi_attn_args *g);
int gemm_split_debug_stamps(long long *host, int n);
int rel_attention_bwd_debug_stamps(long long *host, int n);
size_t rel_attention_bwd_workspace_floats(const isi_attn_args *g);
int rel_attention_bwd_f32(const isi_attn_bwd_args *g, hipStream_t stream);
size_t layernorm_bwd_workspace_floats(int64_t M, int D);
int layernorm_bwd_f32(const float *x, const float *res, const float *gamma, const float *dy, float *dz,
                      float *dgamma, float *dbeta, float *workspace, int64_t M, int D, float eps,
                      hipStream_t stream, float *dx = nullptr, float drop_p = 0.f, uint64_t drop_seed = 0);
int label_smoothing_loss_f32(const float *logits, const int64_t *target, float *row_loss, float *dlogits, int64_t M,
                             int K, int num_classes, float smoothing, float grad_scale, hipStream_t stream);
int layernorm_f32(const float *x, const float *res, const float *gamma, const float *beta, float *out,
                  int64_t M, int D, float eps, hipStream_t stream, float drop_p = 0.f, uint64_t drop_seed = 0);
int linear_rows_f32(const float *x, int x_stride, const float *W, const float *bias, const float *res,
                    int res_stride, float *out, int out_stride, int M, int N, int K, int relu,
                    hipStream_t stream);

int rel_attention_decode_f32(const isi_attn_args *g, int q_pos, float *workspace, hipStream_t stream);
int rel_attention_decode_pos_f32(const isi_attn_args *g, int q_pos, const int *pos, int self_keys, float *workspace,
                                 hipStream_t stream);
size_t rel_attention_decode_workspace_floats(int B, int H, int head_dim);
// optional tail of the sampling kernel (the decoding loop): codes[row, p - i_off] = token; x_seq[p + 1][row, 0:eff] = table[token]
// (SampleCommitCore is what the draw kernel's instantiations without a log-probability receive: its 64 bytes are the kernel
// argument they always had)
struct SampleCommitCore {
  const float *table; int eff;
  int64_t *codes; int codes_stride;
  int p_value, i_off, S_t;
  float *x_seq; int x_stride;
  int *advance;      // ONE row only (a single workgroup: no other reader of the counter in the launch): *advance = position + 1
                     // behind the commit -- the decode loop's set_pos launch (4.3 us of a 280 us token) folded in
};
struct SampleCommit : SampleCommitCore {
  float *log_probs;  // [rows, codes_stride] or nullptr: beside every committed code, the MODEL's log-probability of it --
                     // log softmax of the row's raw logits (temperature 1, nothing filtered) at the token (isi_prior_state.token_log_probs)
};
// ragged batches (isi_prior_sample_run_rows): row r of the launch stands at position row_pos[t * rows + r] of step
// t = *pos (replayable) or t = 0 (row_pos, commit already offset to the step); it draws with u[(position - pos_off) * rows + r]
// and commits only where commit[t * rows + r] and the token lies in [0, S).  Per-row temperature / top_k / top_p or NULL.
struct SampleRows {
  const int *row_pos;
  const uint8_t *commit;
  const float *temperature;
  const int *top_k;
  const float *top_p;
  int S;
};
// logit bias (isi_prior_code_bias, isi_sample_row_bias_f32): the launch row at token i of its sequence -- the token the
// commit computes, position - i_off; 0 without a commit -- adds table[index[row * index_stride + i], 0:n] to its logits
// before temperature and filters.  index == nullptr: table row 0 on every row.  An index outside [0, count), or a token
// outside [0, S), means no bias and reads nothing from the table.  -inf bans a class.
struct SampleBias {
  const float *table; int table_stride;   // [count, table_stride], table_stride >= n
  int count;
  const int *index; int index_stride;     // [rows, S] (index_stride = S) or [S] shared by every row (index_stride = 0)
  int S;
};
// (what the draw kernel's BIAS instantiations receive in place of SampleRows: the others take the bytes they always took)
struct SampleRowsBias : SampleRows {
  SampleBias bias;
};
int sample_row_commit_f32(const float *logits, int stride, int rows, int n, float temperature, int top_k, float top_p,
                          const float *u, int64_t *out, float *filtered, const int *pos, int pos_off,
                          const SampleCommit &cm, hipStream_t stream, const SampleRows *ragged = nullptr,
                          const SampleBias *bias = nullptr);
// isi_sample_row_f32 with bias[bias_row[row], 0:n] (bias_row == nullptr: row 0) added to every row's logits
int sample_row_bias_f32(const float *logits, int stride, int rows, int n, float temperature, int top_k, float top_p,
                        const float *u, int64_t *out, float *filtered, const float *bias, int bias_stride, int bias_count,
                        const int32_t *bias_row, hipStream_t stream);
int sample_row_pos_f32(const float *logits, int stride, int rows, int n, float temperature, int top_k, float top_p,
                       const float *u, int64_t *out, float *filtered, const int *pos, int pos_off,
                       hipStream_t stream);
int sample_row_f32(const float *logits, int stride, int rows, int n, float temperature, int top_k, float top_p,
                   const float *u, int64_t *out, float *filtered, hipStream_t stream);
// the draw, and log_prob[row] = the model's log-probability of the drawn token (the decode loop's kernel and arithmetic)
int sample_row_log_prob_f32(const float *logits, int stride, int rows, int n, float temperature, int top_k, float top_p,
                            const float *u, int64_t *out, float *log_prob, hipStream_t stream);
// out[r] = log softmax(logits[r, 0:n])[codes[r]]; NaN for a code outside [0, n)
int token_log_prob_f32(const float *logits, int stride, int rows, int n, const int64_t *codes, float *out, hipStream_t stream);
int token_stats_f32(const float *logits, int stride, int rows, int n, const int64_t *codes, float *log_prob, float *entropy,
                    int *rank, int top_n, int64_t *top_codes, float *top_log_probs, hipStream_t stream);

int rel_attention_decode_splits(int Sk, int pairs);
int attention_tail_rows(int S, int mask_mode, bool dense_mask);   // rel_attention_f32.hip
// row_pos != nullptr (ragged batches): batch row b queries from position row_pos[t * B + b], t = *pos or 0 (row_pos
// then already offset to the step); self-attention reads that position + 1 keys, g->Sk is their upper bound
int rel_attention_decode_launch(const isi_attn_args *g, int q_pos, const int *pos, int self_keys, float *workspace,
                                int combine, hipStream_t stream, const int *row_pos = nullptr, int kv_format = 0);
// args->k / args->v read as bf16 (isi_rel_attention_decode_kv16_f32)
int rel_attention_decode_kv16_f32(const isi_attn_args *g, int q_pos, float *workspace, hipStream_t stream);
int rel_attention_decode_combine(const float *partial, float *out, int B, int H, int head_dim, int ns, int64_t o_sb,
                                 int64_t o_sh, hipStream_t stream);
// keys / values without a batch dimension (rel_attention_decode_shared.hip): one workgroup per (head, row block, key split)
int rel_attention_decode_shared_splits(int Sk, int B, int H);
int rel_attention_decode_shared_launch(const isi_attn_args *g, int q_pos, const int *pos, float *workspace, int combine,
                                       int kv_format, hipStream_t stream);
size_t decode_stage_workspace_floats(int M, int N, int K);
int decode_stage_f32(const float *x, int x_stride, const float *ln_g, const float *ln_b, const float *W, const float *bias,
                     const float *res, int res_stride, const float *res_g, const float *res_b, float *out, int out_stride,
                     int M, int N, int K, int relu, float eps, float *workspace, size_t workspace_floats, hipStream_t st);
// isi_decode_stage_ex_f32 / isi_decode_single_source_f32: a stage / the single-source block as the loop launches them
int decode_stage_ex_f32(isi_decode_stage_args *args, hipStream_t st);
int decode_single_source_f32(const isi_decode_single_source_args *args, hipStream_t st);
size_t prior_decode_scratch_floats(const isi_prior_w *w, int B);
// bias: isi_prior_sample_run_bias / isi_prior_sample_run_rows_bias; nullptr or a zeroed struct: off
int prior_sample_run(const isi_prior_w *w, const isi_prior_state *s, int p_begin, int p_end, float temperature,
                     int top_k, float top_p, hipStream_t stream, const isi_prior_code_bias *bias = nullptr);
int prior_sample_run_rows(const isi_prior_w *w, const isi_prior_state *s, const isi_prior_rows *rows, int t_begin, int t_end,
                          float temperature, int top_k, float top_p, hipStream_t stream,
                          const isi_prior_code_bias *bias = nullptr);

bool gemm_split_applicable(int M, int N, int K, int split_mode);
// tile: 1 = 128 x 64, 2 = 128 x 128, 3 = 256 x 128, 4 = 256 x 256; tail: the last rows, left to fp32 dot products
struct GemmRoute { int tile, tail; };
GemmRoute gemm_split_route(int M, int N, bool rows4, bool plain);
int gemm_split_linear_route(int M, int N, int K, int split_mode);   // isi_linear_route
// Optional extras of gemm_split_f32: a batch of nz independent products (grid y; element strides between them) and a
// band of the K range per 128-row tile -- rows [u win_rpu, (u + 1) win_rpu) only have non-zero A columns in
// [lo_slope u + lo_base, hi_slope u + hi_base] (slopes >= 0), the K chunks outside the tile's band are skipped
// (win_rpu = 0: no band).  The attention backward's dQ += G E^T uses both (rel_attention_bwd_f32.hip); the gate is the
// linear layers' (conv2d_f32 with a gate, 1x1).
struct GemmExtra {
  int nz;
  int64_t zs_a, zs_w, zs_res, zs_out;
  int win_rpu, lo_slope, lo_base, hi_slope, hi_base;
  const float *gate;      // optional (nz = 1): out = gate[m ldg + n] > 0 ? value : 0 (a ReLU's backward mask in the epilogue)
  int64_t ldg;
  float gate_scale;       // the gated value is multiplied by this (0 = 1: the inverse keep probability of a dropout folded in)
  float drop_p;           // inverted dropout on the (rectified) output, keep mask = attention_dropout_keep(seed, m ldo + n); 0: none
  uint64_t drop_seed;
};
// Optional device-resident term of every fused dropout's seed (isi_set_dropout_seed_base): a step replayed from a HIP
// graph carries its seeds as launch constants, the owner of the graph advances this counter between replays.
const uint64_t *dropout_seed_base();
// the keep decision of the fused dropout: a counter-based hash of (seed, flat output index) -- the same function in the
// forward epilogue and wherever a backward needs the mask again
// (round 6: two 32-bit multiplies instead of four -- v_mul_lo_u32 runs at a quarter of the vector rate, and the 128 keep
// decisions per lane of a 256 x 256 GEMM tile's epilogue cost the feed-forward layers 22 us of 86, tools/prof_steady.py:
// the "lowbias32" mixer (xorshift-multiply twice, full avalanche) over the index, the seed's words folded in behind
// each round)
__host__ __device__ inline bool dropout_keep(uint64_t seed, uint32_t idx, uint32_t thresh) {
  uint32_t h = idx;
  h ^= h >> 16; h *= 0x7FEB352Du;
  h ^= (uint32_t)seed;                  // (behind the first round: seeds that differ in a low bit must not just swap neighbours)
  // (the high word in FRONT of the second multiply, which carries its bits upward: folded in behind it, a bit of it reached
  // the hash's same bit and the one 16 below only, and `h >= thresh` reads the top bits -- seeds that differed in bits
  // 32 .. 61 alone drew the same mask, tests/test_linear_gemm_host.py::test_dropout_keep_mask)
  h ^= h >> 15; h ^= (uint32_t)(seed >> 32); h *= 0x846CA68Bu;
  h ^= h >> 16;
  return h >= thresh;
}
int gemm_split_f32(const float *a, int64_t lda, const float *w, const float *bias, const float *res, int64_t ldr, float *out,
                   int64_t ldo, int M, int N, int K, int relu, int split_mode, hipStream_t stream,
                   const float *w16 = nullptr, const GemmExtra *extra = nullptr);
size_t conv_wgrad_workspace_floats(int Cout, int K, int M, int nphase);
int conv_wgrad_f32(const isi_src *s0, const isi_src *s1, const float *dy, float *dw_packed, float *db,
                   float *workspace, size_t workspace_floats, int B, int H, int W, int Cout, int KH, int KW,
                   int stride, int pad, int transposed, hipStream_t stream, int torch_keep = 0);
// optional hint of conv_wgrad_batched_f32: output channel c of dY is non-zero only on the pixels of units
// [lo_slope c + lo_base, hi_slope c + hi_base] (slopes >= 0), a unit = win_rpu consecutive pixels of the GEMM grid
// Band-limited products over the attention backward's G (GemmExtra.win_rpu, WgradBand): G is zeroed only in margins around
// each row's band (rel_attention_bwd_f32.hip: kMargin), which must cover what a tile of either product reads beyond a row's
// own band: at most one tile of rows / columns plus the K-chunk rounding.  The kernels assert their tiles against these.
constexpr int kBandTileMax = 128;     // rows of a banded GEMM tile, columns of a banded weight-gradient tile: at most
constexpr int kBandChunk = 32;        // K chunk of both kernels
struct WgradBand { int win_rpu, lo_slope, lo_base, hi_slope, hi_base; int required; };   // required: fail rather than read outside the band (dY is only defined there)
int conv_wgrad_batched_f32(const isi_src *s0, const isi_src *s1, const float *dy, float *dw_packed, float *db,
                           float *workspace, size_t workspace_floats, int B, int H, int W, int Cout, int KH, int KW,
                           int stride, int pad, int transposed, int nz, int64_t zs_x0, int64_t zs_dy, int64_t zs_dw,
                           hipStream_t stream, int torch_keep = 0, const WgradBand *band = nullptr);
size_t conv_wgrad_batched_workspace_floats(int Cout, int K, int M, int nphase, int nz);
size_t vq_embed_sum_workspace_floats(int D, int K, int64_t N);
int relu_bwd_f32(float *dy, const float *y, int64_t n, hipStream_t st);
int axpy_f32(float *a, const float *b, float alpha, int64_t n, hipStream_t st);
int vq_bwd_f32(float *dz, const float *dq, const float *z, const float *q_st, const float *g_diff, int64_t n,
               hipStream_t st);
int colsum_num_partials(int64_t M);
int colsum_f32(const float *x, int64_t x_stride, float *out, float *workspace, int64_t M, int C, hipStream_t st);
int vq_embed_sum_f32(const float *z, const int64_t *idx, float *embed_sum_dk, float *workspace,
                     size_t workspace_floats, int64_t N, int D, int K, hipStream_t stream);
int vq_ema_update_f32(float *embed, float *cluster_size, float *embed_avg, const float *counts,
                      const float *embed_sum_dk, int D, int K, float decay, float eps, hipStream_t st);
// Random restarts of dead codes ("EMA codebook with random restarts"): the batch row that code k is redrawn
// from at `step`, a counter-based function (splitmix64's finaliser, all arithmetic modulo 2^64) shared by the device
// kernel and the host export isi_vq_restart_row.
__host__ __device__ inline uint64_t vq_restart_mix(uint64_t x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}
__host__ __device__ inline uint64_t vq_restart_row(uint64_t seed, uint64_t step, int k, int64_t N) {
  return vq_restart_mix(vq_restart_mix(seed ^ vq_restart_mix(step)) + (uint64_t)(int64_t)k) % (uint64_t)N;
}
int vq_restart_candidates_f32(const float *z, int64_t N, int D, int K, const int64_t *restart_state, int rank, int world,
                              float *cand_out, hipStream_t st);
int vq_ema_update_restart_f32(float *embed, float *cluster_size, float *embed_avg, const float *counts,
                              const float *embed_sum_dk, const float *cand, int D, int K, float decay, float eps,
                              float threshold, int initialize, int64_t *restart_state, hipStream_t st);

int vq_nearest_f32(const float *z, const float *codes, const float *e2, int64_t *idx, float *q,
                   int32_t *counts, float *sse_part, int64_t N, int D, int K, int flags, hipStream_t stream);
int vq_num_partials(int64_t N);
bool vq_conv1x1_fusable(int C0, int C1, int D, int K);
int vq_debug_stamps(long long *host, int n);
int vq_conv1x1_nearest_f32(const isi_src *s0, const isi_src *s1, const float *w16, const float *bias, const float *codes,
                           const float *e2, int64_t *idx, float *q, float *q_pair, int32_t *counts, float *sse_part,
                           float *workspace, int B, int H, int W, int D, int K, hipStream_t stream, bool zero_counts = false,
                           float *z_out = nullptr, const float *wfrag_packed = nullptr, const void *planes = nullptr);
// the pack-time image of a codebook's LDS content (planes, adjusted |e|^2, far words): what the fused search otherwise
// derives from codes_kd / e2 in every workgroup of every launch
size_t vq_planes_bytes(int K);
int vq_pack_planes_f32(const float *codes_kd, const float *e2, void *planes_out, int D, int K, hipStream_t stream);
int vq_pack_fragments_f32(const float *packed_w16, float *frag_out, int Kpad, hipStream_t stream);
// code_tables.hip: the two layers that read only the quantised top map, as sums of pack-time table rows
size_t vq_code_tables_bytes(int which, int K, int Cout);
int vq_pack_code_tables_f32(const float *w3_packed, int Cout3, const float *wT_packed, int CoutU, const float *codes_kd, int D,
                            int K, float *t3_out, float *tu_out, hipStream_t stream);
int vq_code_gather_f32(const int64_t *ids, const float *t3, const float *bias3, float *out3, int C3, int out3_pair, int relu3,
                       const float *tu, const float *biasU, float *outU, int CU, int outU_pair, int reluU, int B, int H, int W,
                       int K, hipStream_t stream);
size_t vq_conv1x1_workspace_floats(int C0, int C1, int D);
int vq_zero_counts(int32_t *counts, int K, hipStream_t stream);
int vq_unquantized_scalars(float *scalars2, hipStream_t stream);
int mse_loss_num_partials(int64_t n);
int mse_loss_f32(const float *a, const float *b, int64_t n, float *workspace, float *out, hipStream_t st);
int mse_loss_bwd_f32(const float *a, const float *b, const float *g, int64_t n, float *da, float *db, hipStream_t st);
int vq_finalize_f32(const float *sse_part, int n_part, const int32_t *counts, int K, int64_t N,
                    int D, float *out2, hipStream_t stream);
// both levels in one launch + out5[4] = diff_t + diff_b; the sum alone (out5[0] + out5[2]) for the two-launch paths
int vq_finalize2_f32(const float *sse_t, int np_t, const int32_t *counts_t, int K_t, int64_t N_t, const float *sse_b, int np_b,
                     const int32_t *counts_b, int K_b, int64_t N_b, int D, float *out5, hipStream_t stream);
int vq_scalars_sum_f32(float *out5, hipStream_t stream);
int embed_code_f32(const int64_t *idx, const float *codes, float *out, int64_t N, int D, int K,
                   hipStream_t stream);
// code_mix.hip: per-cell weighted mixtures of codebook rows (the spec: isi_embed_mix_f32 in isi_hip.h)
int embed_mix_f32(const int64_t *ids, int64_t ids_stride, const float *weights, int64_t w_stride, const float *codes, float *out,
                  int64_t ldo, int64_t N, int M, int D, int K, hipStream_t stream);
// vq_topm.hip: the M nearest codes of each vector among its palette's (the spec: isi_vq_nearest_topm_f32 in isi_hip.h)
int vq_nearest_topm_f32(const float *z, const float *codes, const float *e2, const uint32_t *allowed, int P,
                        const int32_t *allowed_row, int64_t *ids, int64_t ids_stride, float *dist, int64_t dist_stride,
                        int64_t N, int D, int K, int M, hipStream_t stream);

int relu_inplace_f32(float *x, int64_t n, hipStream_t stream);

int spec_polar_f32(const float *stft, float *a, float *ph, int B, int T, int F, int mel, hipStream_t st);
int spec_finish_f32(const float *a, const float *ph, float *out, int B, int T, int F, int mel, hipStream_t st);
int spec_inverse_prepare_f32(const float *spec, float *a, float *ph, int B, int T, int F, hipStream_t st);
int spec_to_stft_f32(const float *a, const float *ph, float *stft, int64_t rows, int F, int mel, hipStream_t st);
int spec_affine_mask_f32(const float *x, const float *ref, float *y, int64_t B, int64_t HW, float a0, float b0, float a1,
                         float b1, float thr, int use_mask, hipStream_t st);
int spec_distance_fwd_f32(const float *xp, const float *xt, float *partial, int B, int T, int F, int RS, float eps,
                          int rows_per_block, hipStream_t st);
int spec_distance_bwd_f32(const float *xp, const float *xt, float *dx, const float *clin, const float *clog, int B, int T,
                          int F, int RS, float eps, int kind, hipStream_t st);
int spec_to_stft_bwd_f32(const float *a, const float *ph, const float *dx, float *da, float *dph, int64_t rows, int F,
                         int mel, hipStream_t st);
int spec_inverse_prepare_bwd_f32(const float *spec, const float *da, const float *dph, float *dspec, int B, int T, int F,
                                 hipStream_t st);
int overlap_add_f32(const float *frames, float *audio, int B, int T, int n_fft, int hop, int left, int64_t L,
                    hipStream_t st);
// spec_splice.hip: phase-locked splice of regenerated frames into an original's STFT, and the sample blend behind it
int spec_splice_f32(const float *stft_orig, const float *a, const float *ph, const float *w, int w_batch, float *stft_out,
                    int B, int T, int F, int mel, hipStream_t st);
int spec_splice_blend_f32(const float *audio_orig, const float *audio_ola, const uint8_t *touched, float *audio_out, int B,
                          int T_frames, int n_fft, int hop, int64_t L, hipStream_t st);
// stft_stretch.hip: an STFT re-timed along a list of source positions, identity phase locking
size_t stft_stretch_workspace_bytes(int B, int T, int F);
int stft_stretch_f32(const float *X, const float *pos, int pos_batch, float *out, void *workspace, size_t workspace_bytes,
                     int B, int T, int T_out, int F, int hop, hipStream_t st);
// formant.hip: true-envelope formant correction of STFT frames
int formant_shift_f32(const float *Y, const float *ratio, int ratio_batch, const float *cos_table, float *out, float *env, int B,
                      int T, int F, int order, int iterations, float depth, float max_gain, hipStream_t st);
int resample_geometry(int fs_in, int fs_out, int *orig, int *new_, int *width, int *taps);
int64_t resample_out_len(int64_t L, int orig, int new_);
int resample_f32(const float *x, int64_t x_stride, float *y, int64_t y_stride, int B, int64_t L, int orig, int new_,
                 int width, const float *table, hipStream_t st);
// warp_resample.hip: the same windowed sinc read along a per-sample position and cutoff
int warp_resample_f32(const float *x, int64_t x_stride, const double *pos, const float *cut, int pos_batch, float *y,
                      int64_t y_stride, int B, int64_t L, int64_t n_out, hipStream_t st);
// pitch.hip
int64_t pitch_frames(int64_t L, int W, int hop, int tau_max);
int pitch_difference_f32(const float *x, int64_t x_stride, float *d, float *energy, int B, int64_t L, int W, int hop,
                         int tau_max, hipStream_t st);
int pitch_pick_f32(const float *d, int64_t n_frames, int tau_min, int tau_max, float threshold, float *period,
                   float *aperiodicity, hipStream_t st);
// code_search.hip
int code_distance_table_f32(const float *codebook, float *table, int K, int D, hipStream_t st);
size_t code_search_workspace_bytes(int64_t N, int64_t C, int K, int Q);
int code_search_f32(const uint16_t *codes, const uint16_t *query, const float *weights, const float *table,
                    const uint8_t *allowed, float *dist, int64_t N, int64_t C, int K, int Q, int accumulate, void *workspace,
                    size_t workspace_bytes, hipStream_t st);
int code_query_rows_f32(const float *z, int64_t z_stride, const float *codebook, float *rows, int64_t cells, int K, int D,
                        hipStream_t st);
int code_search_rows_f32(const uint16_t *codes, const float *rows, const float *weights, const uint8_t *allowed, float *dist,
                         int64_t N, int64_t C, int K, int Q, int accumulate, void *workspace, size_t workspace_bytes,
                         hipStream_t st);
// the stage both searches share (device_prims.h: stage_code_rows, stage_query_rows): 64 KB of LDS hold `cc` table rows of K floats, at most 32,
// a multiple of 8 from 8 cells on (code vectors hold 8 cells)
constexpr int kCodeStageFloats = 16384;
inline int code_chunk_cells(int K) {
  int cc = kCodeStageFloats / K;
  if (cc > 32) cc = 32;
  if (cc >= 8) cc &= ~7;
  return cc;
}
// code_shift_search.hip
size_t code_shift_search_workspace_bytes(int64_t N, int F, int T, int W, int S, int K, int Q);
int code_shift_search_f32(const uint16_t *codes, const uint16_t *query, const float *weights, const float *table, float *dist,
                          int64_t N, int F, int T, int W, int shift0, int step, int S, int K, int Q, int accumulate,
                          void *workspace, size_t workspace_bytes, hipStream_t st);
int code_shift_search_rows_f32(const uint16_t *codes, const float *rows, const float *weights, float *dist, int64_t N, int F,
                               int T, int W, int shift0, int step, int S, int K, int Q, int accumulate, void *workspace,
                               size_t workspace_bytes, hipStream_t st);
int code_shift_best_f32(const float *dist, const uint8_t *allowed, float *best, int32_t *best_shift, int64_t N, int S, int Q,
                        hipStream_t st);
// code_warp_search.hip
int code_warp_search_f32(const isi_warp_part *parts, int n_parts, const uint8_t *allowed, float *dist, int32_t *end, int64_t N,
                         int T, int W, int lo, int hi, int Q, hipStream_t st);
size_t code_warp_path_workspace_bytes(int M, int W, int lo, int hi, int Q);
int code_warp_path_f32(const isi_warp_part *parts, int n_parts, const int64_t *items, int M, int32_t *path, float *dist,
                       void *workspace, size_t workspace_bytes, int64_t N, int T, int W, int lo, int hi, int Q, hipStream_t st);

size_t packed_conv_weight_floats(int Cout, int Cin, int KH, int KW);
size_t packed_convT_k4s2_weight_floats(int Cin, int Cout);
int pack_conv_weight_w16_f32(const float *w, float *packed, int Cout, int Cin, int KH, int KW, hipStream_t stream);
int pack_conv_weight_f32(const float *w, float *packed, int Cout, int Cin, int KH, int KW,
                         hipStream_t stream);
int pack_linear_wT_bf16(const float *w, float *out, int N, int K, hipStream_t stream);
int pack_linear_wT_bf16_multi(const void *table_dev, int n, int blocks_per_weight, hipStream_t stream);
int pack_conv_dgrad_weight_f32(const float *w, float *packed, int Cout, int Cin, int KH, int KW, hipStream_t stream);
int pack_convT_k4s2_weight_f32(const float *w, float *packed, int Cin, int Cout,
                               hipStream_t stream);
int pack_codebook_f32(const float *embed, float *codes_kd, float *e2, int D, int K,
                      hipStream_t stream);

int vqvae_pair_activations(const isi_vqvae_w *w);
size_t vqvae_workspace_bytes(const isi_vqvae_w *w, int B, int H, int W);
int vqvae_run(const isi_vqvae_w *w, int mode, const float *x, int B, int H, int W,
              const isi_vqvae_out *out, void *workspace, size_t workspace_bytes,
              hipStream_t stream);

}  // namespace isi
