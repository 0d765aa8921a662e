// The host plan of the prior's key/value-cached sampling loop (isi_prior_sample_run, isi_prior_sample_run_rows): pure host
// code, no kernel.  The kernels and the launchers that pick their instantiations are prior_decode.hip (prior_decode.h), the
// cached attention transformer_ops.hip and rel_attention_decode_shared.hip.  tests/decode_plan_tracer.cpp links this file
// against recording stubs of all of them and pins every launch of every route (tests/decode_plan_trace.txt).
//
// One call runs, for every sequence position in [p_begin, p_end), the whole decoder stack on ONE new row per batch row, and
// for a sampled position the logits head, the categorical draw and the write of the sampled token's embedding into the
// next input row; the sampled index stays on the device.  Per layer that is a chain of 8 dependent launches,
//   LN + q|k|v (k, v straight into the cache slot) -> self-attention over key splits -> out-projection + residual ->
//   LN1 + cross-attention query -> cross-attention -> out-projection + residual -> LN2 + linear1 + ReLU -> linear2 + residual
// (6 with single-source cross-attention: one launch forms the whole cross block), ~66 per position of an 8-layer prior.
// The LayerNorms and the merge of an attention's key splits run in the prologue of the consuming stage.  A DEPENDENT launch
// costs ~3 us whatever its work, so single-stream decoding is bound by that count: every position-dependent address is
// therefore also readable on the device from a position counter, the launches of W = ISI_PRIOR_GRAPH consecutive
// positions are captured once into a hipGraph (two variants: every position samples / none does) and a window is replayed
// with one graph launch.  The executables are CACHED by the bytes of the call's arguments: nothing is destroyed at the end
// of a call and the call never waits for the stream.  The first position of a call, windows of mixed positions and the tail
// run as direct launches, which take the position by value.
//
// The file in order: which kernel runs a stage (ONE decision, for the launch and for the statistics hand-off); the stages'
// argument blocks by named parts; where a launch stands (Where) and what a call is made of (Route, Scratch); the blocks of
// a layer and enqueue_position; the checks, all before the first launch; the graph cache; the entry points.
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "isi_common.h"
#include "isi_internal.h"
#include "knobs.h"
#include "prior_decode.h"

namespace isi {

// rows of a group of the rows-in-registers kernel: as many as fit (kq * mr <= 16), at most 8
int row_gemvm_group(int M, int kq) {
  int mr = M <= 2 ? 2 : M <= 4 ? 4 : 8;
  while (kq * mr > 16) mr >>= 1;
  return mr;
}

namespace {

// ---------------------------------------------------------------- which kernel runs a stage
bool row_mfma_supported(const RowLinArgs &a) {
  // what the tile kernel holds per lane of a row while it forms LayerNorm statistics: 8 float4 of an input row, 8 floats of a
  // residual row.  Wider residual rows run on the tiles with their statistics handed (res_stat), as the loop hands them
  if (a.ln_g && a.K > 2048) return false;
  if (a.res && a.res_g && !a.res_stat && a.N > 512) return false;
  return a.M >= 2 && (a.K & 7) == 0 && (a.x_stride & 3) == 0 && (reinterpret_cast<uintptr_t>(a.x) & 15) == 0 &&
         (reinterpret_cast<uintptr_t>(a.W) & 15) == 0 && (!a.ln_g || ((reinterpret_cast<uintptr_t>(a.ln_g) | reinterpret_cast<uintptr_t>(a.ln_b)) & 15) == 0);
}
bool row_gemvm_supported(const RowLinArgs &a) {
  if (a.M < 1 || a.M > 256 || (a.K & 3) || a.K > 2048) return false;
  if (a.res && a.res_g && a.N > 512) return false;
  const int kq = a.K <= 256 ? 1 : a.K <= 512 ? 2 : a.K <= 1024 ? 4 : 8;
  return row_gemvm_group(a.M, kq) >= 2;
}
// `merged`: the input row is the merge of an attention's key-split partials
bool row_gemv1_supported(const RowLinArgs &a, bool merged) {
  if (a.M != 1 || (a.K & 3) || a.K > 2048) return false;
  if (a.res && a.res_g && a.N > 512) return false;
  return !merged || a.K <= 512;
}

// A stage (placed: a.row_pos says whether its rows are addressed one by one) runs as the one-row kernel; beyond
// `decode_mfma_rows` rows as 32-row tiles on the fp32 matrix pipe; up to there with every row in registers, the rows passing
// through in groups; else in groups of 8 rows staged in LDS, one launch each.  Per-row addressing exists in the two batched
// kernels only.
enum class StageKernel { kOneRow, kTiles, kRowsInRegisters, kGroupsOf8, kRefused };
StageKernel stage_kernel(const RowLinArgs &a, bool merged) {
  const bool rag = a.row_pos != nullptr;
  if (!rag && row_gemv1_supported(a, merged)) return StageKernel::kOneRow;
  if (a.M > knobs().decode_mfma_rows && row_mfma_supported(a)) return StageKernel::kTiles;
  if (row_gemvm_supported(a)) return StageKernel::kRowsInRegisters;
  return rag ? StageKernel::kRefused : StageKernel::kGroupsOf8;
}

// (host) out2 moved on by `elems` elements of its format
void advance_out2(RowLinArgs &a, long elems) {
  if (!a.out2) return;
  a.out2 = a.out2_bf16 ? reinterpret_cast<float *>(reinterpret_cast<uint16_t *>(a.out2) + elems) : a.out2 + elems;
}
// rows [m0, m0 + 8) of a stage
RowLinArgs row_group(const RowLinArgs &a, int m0) {
  RowLinArgs g = a;
  g.M = a.M - m0 < 8 ? a.M - m0 : 8;
  g.x += (size_t)m0 * a.x_stride;
  if (g.res) g.res += (size_t)m0 * a.res_stride;
  g.out += (size_t)m0 * a.out_stride;
  advance_out2(g, (long)m0 * a.out2_stride);
  return g;
}

// what the kernel of a stage cannot run: the same answer before anything is launched (check_stages) and at the launch
int stage_refusal(const RowLinArgs &a, StageKernel k) {
  if (k == StageKernel::kRefused) return unsupported("decode stage: ragged rows need the batched kernels (K <= 2048; a normalised residual of more than 512 features "
                       "on the tiles, with its statistics handed)");
  if (k == StageKernel::kGroupsOf8 && row_linear_lds_bytes(a.M, a.K) > kRowLinearLdsMax)
    return unsupported("row_linear: rows do not fit in LDS");
  return ISI_OK;
}

// Where launches go.  check_only: nothing is launched, a stage only answers whether its kernel would refuse it.
struct Queue {
  hipStream_t st;
  bool check_only;
};

// One stage on M rows.  `part` != nullptr (one row): the input row is the merge of that attention's key-split partials.
int launch_stage_rows(const RowLinArgs &a, const float *part, int ns, int hd, float *mf_ws, size_t mf_ws_floats, Queue q) {
  const StageKernel k = stage_kernel(a, part != nullptr);
  if (int rc = stage_refusal(a, k)) return rc;
  if (q.check_only) return ISI_OK;
  switch (k) {
    case StageKernel::kOneRow: return launch_row_gemv1(a, part, ns, hd, q.st);
    case StageKernel::kTiles: return launch_row_mfma(a, q.st, mf_ws, mf_ws_floats);
    case StageKernel::kRowsInRegisters: return launch_row_gemvm(a, q.st);
    default: break;
  }
  for (int m0 = 0; m0 < a.M; m0 += 8)
    if (int rc = launch_row_linear_8(row_group(a, m0), q.st)) return rc;
  return ISI_OK;
}

// ---------------------------------------------------------------- a stage's argument block, by named parts
// out[M][N] = x[M][K] W[N][K]^T + bias, dense rows; everything else is off until a setter turns it on
struct Stage {
  RowLinArgs a;
  Stage(const float *x, int K, const float *W, const float *bias, float *out, int N, int M) : a{} {
    a.x = x; a.x_stride = K; a.W = W; a.bias = bias; a.out = out; a.out_stride = N;
    a.split = N; a.M = M; a.N = N; a.K = K; a.eps = 1e-5f;
  }
  Stage &with_strides(int x_stride, int out_stride) { a.x_stride = x_stride; a.out_stride = out_stride; return *this; }
  Stage &with_eps(float eps) { a.eps = eps; return *this; }
  Stage &with_ln(const float *g, const float *b) { a.ln_g = g; a.ln_b = b; return *this; }                 // LayerNorm on x
  Stage &with_relu(bool on = true) { a.relu = on ? 1 : 0; return *this; }
  // + LN_res(res): g, b nullable
  Stage &with_residual(const float *res, int stride, const float *g, const float *b) {
    a.res = res; a.res_stride = stride; a.res_g = g; a.res_b = b;
    return *this;
  }
  // columns [split, N) go to out2 (bf16: a 16-bit array), `out` holds [0, split) densely
  Stage &with_out2(float *out2, int stride, int split, bool bf16) {
    a.out2 = out2; a.out2_stride = stride; a.split = split; a.out_stride = split; a.out2_bf16 = bf16 ? 1 : 0;
    return *this;
  }
  // x / res / out2 move on by these element counts per sequence position (Where says which position)
  Stage &advancing(long x_pos, long res_pos, long out2_pos) { a.x_pos = x_pos; a.res_pos = res_pos; a.out2_pos = out2_pos; return *this; }
};

// ---------------------------------------------------------------- where a launch stands
// The position of the launches of one enqueue_position.  By value (p >= 0, direct launches: no dependent load of the counter
// at the head of every kernel), or read on the device from the counter (p = -1: replayable launches).  Ragged plans: p / the
// counter is the STEP, and the rows stand at row_pos[.] -- offset to the step for a direct launch, the whole array beside
// the counter for a replayable one (`commit` likewise).
struct Where {
  int p;
  const int *counter;
  const int *row_pos;
  const uint8_t *commit;
  int by_value() const { return p < 0 ? 0 : p; }      // (what a launch that reads the counter gets in the value's place)
};
Where where_of(int p, int *counter, const isi_prior_rows *rows, int B) {
  const size_t step = p < 0 ? 0 : (size_t)p * B;
  return Where{p, p < 0 ? counter : nullptr, rows ? rows->pos + step : nullptr, rows ? rows->commit + step : nullptr};
}
// the stage at that position.  A stage none of whose addresses moves with the position is the same launch everywhere.
RowLinArgs placed(RowLinArgs a, const Where &at) {
  a.pos = nullptr;
  if (!a.x_pos && !a.res_pos && !a.out2_pos) return a;
  if (at.row_pos) {
    a.row_pos = at.row_pos;
    a.pos = at.counter;
  } else if (at.counter) {
    a.pos = at.counter;
  } else {
    a.x += (long)at.p * a.x_pos;
    if (a.res) a.res += (long)at.p * a.res_pos;
    advance_out2(a, (long)at.p * a.out2_pos);
  }
  return a;
}

// ---------------------------------------------------------------- what a call is made of
// the scratch, laid out once: prior_decode_scratch_floats is this function's `floats` for a null base
struct Scratch {
  float *q, *ao, *y1, *y2, *y3a, *y3b;   // [B, d] each: query, attention output, the layer's three pre-norm rows (y3 alternates)
  float *hid;                            // [B, dim_feedforward]
  float *logits;                         // [B, n_class]
  int64_t *sampled;                      // [B]
  float *attn_ws;                        // the cached attention's partial rows (16-byte aligned)
  int *pos;                              // the position counter (16-byte aligned, 4 ints)
  float *mf_ws;                          // K-chunk sums of the tile kernel (16-byte aligned)
  size_t mf_ws_floats;
  float *rowstat;                        // [B][2] LayerNorm statistics handed from launch to launch (RowLinArgs.stat_out)
  size_t floats;
};
// partial sums of the K chunks of linear2 (K = dim_feedforward, N = d_model) when a batch decodes on matrix tiles
size_t mfma_ksplit_floats(const isi_prior_w *w, int B) {
  return (size_t)B * ((w->dim_feedforward + MF_KC - 1) / MF_KC) * w->d_model;
}
Scratch carve(const isi_prior_w *w, int B, float *base) {
  const size_t d = w->d_model;
  uintptr_t at = reinterpret_cast<uintptr_t>(base);
  size_t bytes = 0;
  auto take = [&](size_t n) { const uintptr_t p = at; at += n; bytes += n; return p; };
  auto align = [&](uintptr_t to) { at = (at + to - 1) & ~(to - 1); };
  auto floats = [&](size_t n) { return reinterpret_cast<float *>(take(n * sizeof(float))); };
  Scratch sc;
  sc.q = floats(B * d); sc.ao = floats(B * d); sc.y1 = floats(B * d); sc.y2 = floats(B * d);
  sc.y3a = floats(B * d); sc.y3b = floats(B * d);
  sc.hid = floats((size_t)B * w->dim_feedforward);
  sc.logits = floats((size_t)B * w->n_class);
  at += ((B * w->n_class) & 1) * sizeof(float);                     // (an even number of floats in front of the int64s)
  sc.sampled = reinterpret_cast<int64_t *>(take((size_t)B * sizeof(int64_t)));
  at += 8;
  align(16);
  sc.attn_ws = floats(rel_attention_decode_workspace_floats(B, w->nhead, w->d_model / w->nhead));
  align(16);
  sc.pos = reinterpret_cast<int *>(take(4 * sizeof(int)));
  sc.mf_ws_floats = mfma_ksplit_floats(w, B);
  sc.mf_ws = floats(sc.mf_ws_floats);
  align(8);
  sc.rowstat = floats(2 * (size_t)B);
  // the skips and alignments above move `at` by less than 16 floats beyond the sizes taken, from any 4-byte aligned base
  sc.floats = bytes / sizeof(float) + 64 + 32 + 4;
  return sc;
}

constexpr int kSharedAttnRows = 48;   // isi_prior_state.memory_shared: batch size from which the row-block cached attention runs

// every fact of the route a call takes, derived once
struct Route {
  bool rag;              // a ragged plan: positions are steps, every position-dependent address is the row's own
  bool kv16;             // bf16 caches
  bool shared;           // one source for all rows: memory_kv / cross_out without a batch dimension
  int mem_B;             // rows per source position of memory_kv / cross_out
  bool single_source;    // state->cross_out: one launch for the cross block, memory_kv is not read
  // a shared memory: from kSharedAttnRows rows on, the kernel that fetches a key row once for a block of rows.  Below that
  // the per-row kernel reads the one copy with batch stride 0 -- the launches of a batched memory, every row's keys the
  // same cache lines: the row-block kernel walks its split in tiles behind barriers and only pays off once the per-row
  // stream is bandwidth (measured: 0.87-0.89x at 8 rows, 0.98-1.05x at 32, 1.29-1.51x at 128 on the [32,32] top prior)
  bool shared_attn;
  bool merge_in_gemv;    // one row of d <= 512: the out-projection merges the attention's key splits
  int ns_self, ns_cross; // key splits of the two attentions
  bool defer_self, defer_cross;   // ... left unmerged for the out-projection
  bool handoff;          // LayerNorm statistics are handed from launch to launch
  int B, d, hd, ff, i_off;        // i_off: the token predicted from position p is p - i_off
  size_t cache_layer, mem_layer;  // elements per layer of kv_cache / memory_kv
  float scale;
};
Route make_route(const isi_prior_w *w, const isi_prior_state *s, bool rag) {
  Route r;
  r.rag = rag;
  r.kv16 = s->kv_format == ISI_KV_BF16;
  r.shared = s->memory_shared == 1;
  r.mem_B = r.shared ? 1 : s->B;
  r.single_source = s->cross_out != nullptr;
  r.B = s->B; r.d = w->d_model; r.hd = r.d / w->nhead; r.ff = w->dim_feedforward; r.i_off = s->start_len - 1;
  r.shared_attn = r.shared && r.B >= kSharedAttnRows;
  r.merge_in_gemv = !rag && r.B == 1 && r.d <= 512 && (r.d & 3) == 0;
  r.ns_self = rel_attention_decode_splits(s->S_t, r.B * w->nhead);
  r.ns_cross = rel_attention_decode_splits(s->S_src, r.B * w->nhead);
  r.defer_self = r.merge_in_gemv && r.ns_self > 1;
  r.defer_cross = r.merge_in_gemv && r.ns_cross > 1;
  r.handoff = !knobs().decode_no_stat_handoff;
  r.cache_layer = (size_t)s->S_t * r.B * 2 * r.d;
  r.mem_layer = (size_t)s->S_src * r.mem_B * 2 * r.d;
  r.scale = 1.0f / sqrtf((float)r.hd);
  return r;
}

struct Call {
  const isi_prior_w *w;
  const isi_prior_state *s;
  const isi_prior_rows *rows;        // nullptr: isi_prior_sample_run
  const isi_prior_code_bias *cb;     // nullptr: off
  float temperature, top_p;
  int top_k;
  Route r;
  Scratch sc;
};

// element `elems` of a cache array in its format (layer strides, the k / v halves: all counted in elements)
float *kv_at(const Route &r, const float *base, size_t elems) {
  return r.kv16 ? reinterpret_cast<float *>(reinterpret_cast<uint16_t *>(const_cast<float *>(base)) + elems)
                : const_cast<float *>(base) + elems;
}

// ---------------------------------------------------------------- the launches of one position
int run_stage(const Call &c, const RowLinArgs &a, Queue q, const float *part = nullptr, int ns = 1) {
  return launch_stage_rows(a, part, ns, c.r.hd, c.sc.mf_ws, c.sc.mf_ws_floats, q);
}

// Two launches of a position normalise the same rows: `producer` as its input, `consumer` one launch later as its
// residual.  Where both run as the same kernel, the first hands the rows' statistics to the second.  (Kept to where it has
// been measured and tested: the tiles; the one-row kernel outside ragged plans; the rows-in-registers kernel for 2 ..
// `decode_mfma_rows` rows.)
void hand_stats(const Call &c, RowLinArgs &producer, RowLinArgs &consumer, bool consumer_merges = false) {
  if (!c.r.handoff || !producer.ln_g || !consumer.res_g) return;
  const StageKernel k = stage_kernel(producer, false);
  RowLinArgs handed = consumer;        // (the consumer as it would be launched: the tiles take wide residual rows only so)
  handed.res_stat = c.sc.rowstat;
  if (k != stage_kernel(handed, consumer_merges)) return;
  const bool on = k == StageKernel::kTiles || (k == StageKernel::kOneRow && !c.r.rag) ||
                  (k == StageKernel::kRowsInRegisters && producer.M > 1 && producer.M <= knobs().decode_mfma_rows);
  if (!on) return;
  producer.stat_out = c.sc.rowstat;
  consumer.res_stat = c.sc.rowstat;
}

// the cached attention of q over keys / values [Sk, B or 1, 2d] (k | v halves)
isi_attn_args cached_attention(const Call &c, const float *kv, bool batched, const isi_attn_w &aw, int Sk, int Ck, int Ek) {
  const Route &r = c.r;
  isi_attn_args g;
  memset(&g, 0, sizeof g);
  g.q = c.sc.q; g.k = kv; g.v = kv_at(r, kv, r.d); g.rel_embeddings = aw.rel_embeddings; g.out = c.sc.ao;
  g.Sq = 1; g.Sk = Sk; g.B = r.B; g.H = c.w->nhead; g.head_dim = r.hd;
  g.q_sb = r.d; g.q_sh = r.hd; g.k_ss = batched ? (int64_t)r.B * 2 * r.d : 2 * r.d; g.k_sb = batched ? 2 * r.d : 0; g.k_sh = r.hd;
  g.v_ss = g.k_ss; g.v_sb = g.k_sb; g.v_sh = r.hd; g.o_sb = r.d; g.o_sh = r.hd;
  g.Cq = c.w->Cd; g.Ck = Ck; g.Ek = Ek; g.rel_rows = aw.rel_rows; g.scale = r.scale;
  return g;
}

// what a layer reads: the rows of the layer below, pre-norm (x_seq: + position * yin_pos), and that layer's last LayerNorm
struct LayerInput {
  const float *yin;
  long yin_pos;
  const float *ln_g, *ln_b;
};

// y1 = LN_in(yin) + self_attention(LN_in(yin)) Wo^T + bo
int self_attention_block(const Call &c, const Where &at, Queue q, int l, const LayerInput &in) {
  const Route &r = c.r;
  const Scratch &sc = c.sc;
  const isi_attn_w &aw = c.w->layers[l].self_attn;
  const int B = r.B, d = r.d;
  float *cache = kv_at(r, c.s->kv_cache, l * r.cache_layer);
  // q | k,v  (k,v straight into the cache slot of this position)
  RowLinArgs qkv = placed(Stage(in.yin, d, aw.in_proj_weight, aw.in_proj_bias, sc.q, 3 * d, B).with_ln(in.ln_g, in.ln_b)
                              .with_out2(cache, 2 * d, d, r.kv16).advancing(in.yin_pos, 0, (long)B * 2 * d).a, at);
  RowLinArgs out = placed(Stage(sc.ao, d, aw.out_proj_weight, aw.out_proj_bias, sc.y1, d, B)
                              .with_residual(in.yin, d, in.ln_g, in.ln_b).advancing(0, in.yin_pos, 0).a, at);
  hand_stats(c, qkv, out, r.defer_self);
  int rc;
  if ((rc = run_stage(c, qkv, q))) return rc;
  if (!q.check_only) {
    const isi_attn_args g = cached_attention(c, cache, true, aw, c.s->S_t, c.w->Cd, c.w->Ed);
    if ((rc = rel_attention_decode_launch(&g, at.by_value(), at.counter, 1, sc.attn_ws, r.defer_self ? 0 : 1, q.st, at.row_pos, c.s->kv_format)))
      return rc;
  }
  return r.defer_self ? run_stage(c, out, q, sc.attn_ws, r.ns_self) : run_stage(c, out, q);
}

// y2 = LN1(y1) + cross_attention(LN1(y1), memory) Wo^T + bo
int cross_attention_block(const Call &c, const Where &at, Queue q, int l) {
  const Route &r = c.r;
  const Scratch &sc = c.sc;
  const isi_decoder_layer_w &L = c.w->layers[l];
  const isi_attn_w &aw = L.cross_attn;
  const int B = r.B, d = r.d;
  const float *memkv = kv_at(r, c.s->memory_kv, l * r.mem_layer);
  RowLinArgs query = placed(Stage(sc.y1, d, aw.in_proj_weight, aw.in_proj_bias, sc.q, d, B).with_ln(L.norm1_w, L.norm1_b).a, at);
  RowLinArgs out = placed(Stage(sc.ao, d, aw.out_proj_weight, aw.out_proj_bias, sc.y2, d, B)
                              .with_residual(sc.y1, d, L.norm1_w, L.norm1_b).a, at);
  hand_stats(c, query, out, r.defer_cross);
  int rc;
  if ((rc = run_stage(c, query, q))) return rc;
  if (!q.check_only) {
    const isi_attn_args g = cached_attention(c, memkv, !r.shared, aw, c.s->S_src, c.w->Ce, c.w->Ee);
    rc = r.shared_attn ? rel_attention_decode_shared_launch(&g, at.by_value(), at.counter, sc.attn_ws, 1, c.s->kv_format, q.st)
                       : rel_attention_decode_launch(&g, at.by_value(), at.counter, 0, sc.attn_ws, r.defer_cross ? 0 : 1, q.st,
                                                     at.row_pos, c.s->kv_format);
    if (rc) return rc;
  }
  return r.defer_cross ? run_stage(c, out, q, sc.attn_ws, r.ns_cross) : run_stage(c, out, q);
}

// single-source cross-attention: y2 = LN1(y1) + T_l[p / Cd] in one launch; y2's statistics go to linear2
int single_source_block(const Call &c, const Where &at, Queue q, int l) {
  if (q.check_only) return ISI_OK;
  const Route &r = c.r;
  const isi_decoder_layer_w &L = c.w->layers[l];
  SingleSourceArgs ss{};
  ss.y1 = c.sc.y1; ss.ln_g = L.norm1_w; ss.ln_b = L.norm1_b;
  ss.table = c.s->cross_out + (size_t)l * c.s->S_src * r.mem_B * r.d;
  ss.y2 = c.sc.y2; ss.stat_out = r.handoff ? c.sc.rowstat : nullptr;
  ss.pos = at.counter; ss.p = at.by_value(); ss.Cd = c.w->Cd; ss.S_src = c.s->S_src; ss.B = r.B; ss.d = r.d; ss.eps = 1e-5f;
  ss.row_pos = at.row_pos; ss.table_B = r.mem_B; ss.table_sb = r.shared ? 0 : 1;
  return launch_single_source_cross(ss, q.st);
}

// y3 = LN2(y2) + relu(LN2(y2) W1^T + b1) W2^T + b2.  y2_stats_ready: the launch that formed y2 left its statistics
int feed_forward_block(const Call &c, const Where &at, Queue q, int l, float *y3, bool y2_stats_ready) {
  const Route &r = c.r;
  const Scratch &sc = c.sc;
  const isi_decoder_layer_w &L = c.w->layers[l];
  RowLinArgs f1 = placed(Stage(sc.y2, r.d, L.linear1_w, L.linear1_b, sc.hid, r.ff, r.B).with_ln(L.norm2_w, L.norm2_b).with_relu().a, at);
  RowLinArgs f2 = placed(Stage(sc.hid, r.ff, L.linear2_w, L.linear2_b, y3, r.d, r.B).with_residual(sc.y2, r.d, L.norm2_w, L.norm2_b).a, at);
  if (!y2_stats_ready) hand_stats(c, f1, f2);
  else if (r.handoff) f2.res_stat = sc.rowstat;
  if (int rc = run_stage(c, f1, q)) return rc;
  return run_stage(c, f2, q);
}

// logits head, the draw, and the commit of the token into codes / the next input row
int sample_block(const Call &c, const Where &at, Queue q, const LayerInput &in) {
  const Route &r = c.r;
  const isi_prior_w *w = c.w;
  const isi_prior_state *s = c.s;
  const int B = r.B;
  if (int rc = run_stage(c, placed(Stage(in.yin, r.d, w->logits_w, w->logits_b, c.sc.logits, w->n_class, B).with_ln(in.ln_g, in.ln_b).a, at), q))
    return rc;
  if (q.check_only) return ISI_OK;
  // (a replayed position of ONE sequence: the commit also advances the position counter)
  const bool fold_advance = !r.rag && at.counter && B == 1;
  // (state->token_log_probs: the draw's instantiation that also stores the committed token's model log-probability)
  const SampleCommit cm{{w->embed_table, w->eff_dim, s->codes, s->S, at.p, r.i_off, s->S_t, s->x_seq, r.d, fold_advance ? c.sc.pos : nullptr},
                        s->token_log_probs};
  SampleRows sr{at.row_pos, at.commit, nullptr, nullptr, nullptr, s->S};
  if (r.rag) { sr.temperature = c.rows->temperature; sr.top_k = c.rows->top_k; sr.top_p = c.rows->top_p; }
  // (a code bias: the instantiation that adds the token's bias row to the logits)
  SampleBias sb{nullptr, w->n_class, 0, nullptr, 0, s->S};
  if (c.cb) sb = SampleBias{c.cb->code_bias, w->n_class, c.cb->code_bias_count, c.cb->code_bias_index,
                            c.cb->code_bias_batch == 1 ? 0 : s->S, s->S};
  // (by value: the uniforms of this position; else the kernel finds them from the position it reads)
  const float *u = (at.counter || r.rag) ? s->uniforms : s->uniforms + (size_t)(at.p - r.i_off) * B;
  return sample_row_commit_f32(c.sc.logits, w->n_class, B, w->n_class, c.temperature, c.top_k, c.top_p, u, c.sc.sampled, nullptr,
                               at.counter, r.i_off, cm, q.st, r.rag ? &sr : nullptr, c.cb ? &sb : nullptr);
}

// Every launch of one position.  Replayable (at.counter): the last launch advances the counter.
int enqueue_position(const Call &c, const Where &at, bool sample, Queue q) {
  const Route &r = c.r;
  LayerInput in{c.s->x_seq, (long)r.B * r.d, nullptr, nullptr};
  for (int l = 0; l < c.w->n_layers; ++l) {
    const isi_decoder_layer_w &L = c.w->layers[l];
    float *y3 = (l & 1) ? c.sc.y3b : c.sc.y3a;
    int rc;
    if ((rc = self_attention_block(c, at, q, l, in))) return rc;
    if ((rc = r.single_source ? single_source_block(c, at, q, l) : cross_attention_block(c, at, q, l))) return rc;
    if ((rc = feed_forward_block(c, at, q, l, y3, r.single_source))) return rc;
    in = LayerInput{y3, 0, L.norm3_w, L.norm3_b};
  }
  if (sample) {
    if (int rc = sample_block(c, at, q, in)) return rc;
    if (!r.rag && at.counter && r.B == 1) return ISI_OK;      // (the commit has advanced the counter)
  }
  if (!at.counter || q.check_only) return ISI_OK;
  return launch_set_pos(c.sc.pos, 1, 1, q.st);
}
int enqueue_position(const Call &c, int p, bool sample, hipStream_t st) {
  return enqueue_position(c, where_of(p, c.sc.pos, c.rows, c.r.B), sample, Queue{st, false});
}

bool sampled_at(const Call &c, int p) {
  if (c.r.rag) {             // some row commits at step p
    for (int b = 0; b < c.r.B; ++b) if (c.rows->commit_host[(size_t)p * c.r.B + b]) return true;
    return false;
  }
  const int i = p - c.r.i_off;
  return i >= 0 && i < c.s->S && c.s->mask[i];
}

// ---------------------------------------------------------------- the checks: every refusal precedes the first launch
// isi_prior_code_bias: both pointers or neither, a positive row count, one index row or one per batch row
int check_code_bias(const isi_prior_code_bias *cb, int B) {
  if (!cb) return ISI_OK;
  if ((cb->code_bias != nullptr) != (cb->code_bias_index != nullptr))
    return invalid("prior_sample_run: code_bias and code_bias_index go together");
  if (!cb->code_bias) return ISI_OK;
  if (cb->code_bias_count <= 0) return invalid("prior_sample_run: code_bias_count must be positive");
  if (cb->code_bias_batch != 1 && cb->code_bias_batch != B) return invalid("prior_sample_run: code_bias_batch must be 1 or B");
  return ISI_OK;
}

int check_call(const isi_prior_w *w, const isi_prior_state *s, const isi_prior_rows *rows, int p_begin, int p_end,
               const isi_prior_code_bias *cb) {
  const bool rag = rows != nullptr;
  if (!w || !s) return invalid("prior_sample_run: null pointer");
  if (w->n_layers <= 0 || w->n_layers > ISI_MAX_LAYERS) return invalid("prior_sample_run: bad layer count");
  if (s->B <= 0 || s->B > 256) return unsupported("prior_sample_run: batch size must be 1..256");
  if (p_begin < 0 || p_end > (rag ? rows->n_steps : s->S_t) || p_begin > p_end) return invalid("prior_sample_run: bad position range");
  if (int rc = check_code_bias(cb, s->B)) return rc;
  const bool single_source = s->cross_out != nullptr;     // memory_kv is not read then
  if (!s->x_seq || !s->kv_cache || (!single_source && !s->memory_kv) || !s->codes || (!rag && !s->mask) || !s->uniforms ||
      !s->scratch)
    return invalid("prior_sample_run: null state pointer");
  if (single_source) {
    if (w->Ce != 1) return unsupported("prior_sample_run: single-source cross-attention needs one source token per event (Ce == 1)");
    if (w->Cd <= 0 || s->S_src <= 0 || (s->S_t - 1) / w->Cd >= s->S_src)
      return invalid("prior_sample_run: single-source cross-attention: a target position without a source row ((S_t - 1) / Cd >= S_src)");
    if (w->d_model > 64 * SS_RS) return unsupported("prior_sample_run: single-source cross-attention needs d_model <= 1024");
  }
  if (s->scratch_floats < prior_decode_scratch_floats(w, s->B)) {
    set_last_error("prior_sample_run: scratch too small");
    return ISI_E_WORKSPACE;
  }
  if (w->d_model % 4 || w->dim_feedforward % 4 || w->d_model % w->nhead) return invalid("prior_sample_run: bad dims");
  if (s->kv_format != ISI_KV_F32 && s->kv_format != ISI_KV_BF16)
    return invalid("prior_sample_run: state->kv_format must be ISI_KV_F32 (0) or ISI_KV_BF16 (1)");
  if (s->memory_shared != 0 && s->memory_shared != 1) return invalid("prior_sample_run: state->memory_shared must be 0 or 1");
  if (s->kv_format == ISI_KV_BF16 &&
      (w->d_model % 8 || ((reinterpret_cast<uintptr_t>(s->kv_cache) | reinterpret_cast<uintptr_t>(s->memory_kv)) & 15)))
    return invalid("prior_sample_run: bf16 kv_cache / memory_kv need d_model % 8 == 0 and 16-byte aligned arrays");
  return ISI_OK;
}

// what a stage's kernel refuses (stage_refusal), asked of every stage of the call's positions: the stages of one position,
// with the sampling tail if any position of the range samples -- all positions launch the same shapes
int check_stages(const Call &c, int p_begin, int p_end) {
  bool samples = false;
  for (int p = p_begin; p < p_end && !samples; ++p) samples = sampled_at(c, p);
  return enqueue_position(c, where_of(p_begin, c.sc.pos, c.rows, c.r.B), samples, Queue{nullptr, true});
}

// ---------------------------------------------------------------- the cache of the loop's graph executables
constexpr size_t kDecodeGraphCacheMax = 8;
struct DecodeGraphs {
  std::vector<unsigned char> key;
  hipGraph_t graphs[2] = {nullptr, nullptr};          // [1]: every position of the window samples; [0]: none does
  hipGraphExec_t execs[2] = {nullptr, nullptr};
  bool failed[2] = {false, false};
  uint64_t used = 0;
  hipEvent_t done = nullptr;      // recorded behind the last replay: what dropping this entry has to wait for
};
std::mutex &decode_graph_mutex() { static std::mutex m; return m; }

template <class T>
void append_bytes(std::vector<unsigned char> &key, const T &v) {
  const size_t at = key.size();
  key.resize(at + sizeof(T));
  std::memcpy(key.data() + at, &v, sizeof(T));
}
// A graph bakes in nothing but the launches' arguments: every pointer and size of *w and *state (the HOST mask aside, which
// only steers which windows replay), the library switches, the sampling parameters, W and the device; a ragged plan's
// device arrays and sizes, not its host copies; a code bias's pointers and sizes (the contents are read at replay).
std::vector<unsigned char> decode_graph_key(const Call &c, int W, int device) {
  std::vector<unsigned char> key;
  append_bytes(key, *c.w);
  isi_prior_state sk = *c.s;
  sk.mask = nullptr;
  append_bytes(key, sk);
  append_bytes(key, knobs());
  struct Tail { float temperature, top_p; int top_k, W, device; } tail{c.temperature, c.top_p, c.top_k, W, device};
  append_bytes(key, tail);
  if (c.rows) {
    isi_prior_rows rk = *c.rows;
    rk.pos_host = nullptr;
    rk.commit_host = nullptr;
    append_bytes(key, rk);
  }
  if (c.cb) append_bytes(key, *c.cb);
  return key;
}
void drop_entry(DecodeGraphs *g) {
  if (g->done) {                                       // its last replay may still be running
    (void)hipEventSynchronize(g->done);
    (void)hipEventDestroy(g->done);
  } else {
    (void)hipDeviceSynchronize();
  }
  for (int j = 0; j < 2; ++j) {
    if (g->execs[j]) (void)hipGraphExecDestroy(g->execs[j]);
    if (g->graphs[j]) (void)hipGraphDestroy(g->graphs[j]);
  }
  delete g;
}
// (called with the mutex held)  The entry of these arguments, the least recently used one making room for a new one.
// nullptr: no device / allocation failure -- the caller then launches directly
DecodeGraphs *decode_graphs_for(const Call &c, int W) {
  static std::vector<DecodeGraphs *> cache;
  static uint64_t clock_ = 0;
  int device = -1;
  if (hipGetDevice(&device) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  std::vector<unsigned char> key = decode_graph_key(c, W, device);
  for (DecodeGraphs *g : cache)
    if (g->key == key) { g->used = ++clock_; return g; }
  if (cache.size() >= kDecodeGraphCacheMax) {
    size_t lru = 0;
    for (size_t i = 1; i < cache.size(); ++i) if (cache[i]->used < cache[lru]->used) lru = i;
    drop_entry(cache[lru]);
    cache.erase(cache.begin() + (long)lru);
  }
  DecodeGraphs *g = new (std::nothrow) DecodeGraphs();
  if (!g) return nullptr;
  g->key = std::move(key);
  g->used = ++clock_;
  cache.push_back(g);
  return g;
}
// variant k of the entry (k = 1: every position of the window samples), captured on `cap` when first needed; a variant
// that failed once is not tried again
bool build_variant(const Call &c, DecodeGraphs *G, int k, int W, hipStream_t &cap) {
  if (G->execs[k] || G->failed[k]) return G->execs[k] != nullptr;
  bool good = (cap != nullptr || hipStreamCreateWithFlags(&cap, hipStreamNonBlocking) == hipSuccess) &&
              hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal) == hipSuccess;
  int erc = ISI_OK;
  for (int i = 0; good && i < W && erc == ISI_OK; ++i) erc = enqueue_position(c, -1, k == 1, cap);
  hipGraph_t gph = nullptr;
  const bool ended = good && hipStreamEndCapture(cap, &gph) == hipSuccess;
  G->graphs[k] = gph;
  good = good && erc == ISI_OK && ended && gph != nullptr && hipGraphInstantiate(&G->execs[k], gph, nullptr, nullptr, 0) == hipSuccess;
  if (!good) { G->failed[k] = true; G->execs[k] = nullptr; (void)hipGetLastError(); }
  return good;
}
// Positions [p, p_end) as far as graphs carry them: windows of W positions that all sample / all keep replay their variant
// (the counter is set in front of a window that does not continue the last one), other positions launch directly.  Leaves
// `p` behind the last position it enqueued; stops early (rc 0) only where there is no cache entry.
int replay_windows(const Call &c, int W, int &p, int p_end, hipStream_t st) {
  std::lock_guard<std::mutex> lock(decode_graph_mutex());
  DecodeGraphs *G = decode_graphs_for(c, W);
  hipStream_t cap = nullptr;
  int rc = ISI_OK;
  int counter = -1;                      // value of the device counter (-1: unknown)
  while (G && p < p_end && rc == ISI_OK) {
    bool uniform = p + W <= p_end;
    const bool flag = sampled_at(c, p);
    for (int i = 1; uniform && i < W; ++i) uniform = sampled_at(c, p + i) == flag;
    if (uniform && build_variant(c, G, flag ? 1 : 0, W, cap)) {
      if (counter != p && (rc = launch_set_pos(c.sc.pos, p, 0, st))) break;
      if (hipGraphLaunch(G->execs[flag ? 1 : 0], st) != hipSuccess) { rc = check_launch("hipGraphLaunch(prior positions)"); break; }
      p += W;
      counter = p;
    } else {
      if ((rc = enqueue_position(c, p, flag, st))) break;
      ++p;
    }
  }
  if (cap) (void)hipStreamDestroy(cap);
  if (G && (G->execs[0] || G->execs[1])) {
    if (!G->done && hipEventCreateWithFlags(&G->done, hipEventDisableTiming) != hipSuccess) { G->done = nullptr; (void)hipGetLastError(); }
    if (G->done && hipEventRecord(G->done, st) != hipSuccess) (void)hipGetLastError();
  }
  return rc;
}

// rows == nullptr: isi_prior_sample_run, p_begin / p_end are positions.  rows != nullptr: isi_prior_sample_run_rows, they
// are steps of the plan (validated by the caller) and every position-dependent address is the row's own
int sample_run_impl(const isi_prior_w *w, const isi_prior_state *s, const isi_prior_rows *rows, int p_begin, int p_end,
                    float temperature, int top_k, float top_p, hipStream_t st, const isi_prior_code_bias *cb) {
  if (int rc = check_call(w, s, rows, p_begin, p_end, cb)) return rc;
  if (cb && !cb->code_bias) cb = nullptr;               // a zeroed struct: off
  if (p_begin == p_end) return ISI_OK;
  const Call c{w, s, rows, cb, temperature, top_p, top_k, make_route(w, s, rows != nullptr), carve(w, s->B, s->scratch)};
  if (int rc = check_stages(c, p_begin, p_end)) return rc;

  // the first position runs directly (it also performs the one-time kernel attribute set-up) ...
  int rc;
  if ((rc = enqueue_position(c, p_begin, sampled_at(c, p_begin), st))) return rc;
  int p = p_begin + 1;
  // ... the rest replays graphs of W positions where there are enough of them to pay for a capture.  Not while the CALLER
  // is capturing `st`: direct launches then, which a capture takes as they are.
  hipStreamCaptureStatus cap_status = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cap_status) != hipSuccess) { (void)hipGetLastError(); cap_status = hipStreamCaptureStatusNone; }
  const int W = cap_status == hipStreamCaptureStatusNone ? knobs().prior_graph : 0;
  if (W > 0 && p_end - p >= (W > 2 ? 2 * W : 4) && (rc = replay_windows(c, W, p, p_end, st))) return rc;
  for (; p < p_end; ++p)
    if ((rc = enqueue_position(c, p, sampled_at(c, p), st))) return rc;
  return ISI_OK;
}

}  // namespace

// A decoding-loop stage on its own (isi_decode_stage_f32): out[M][N] = act(LN(x)[M][K] W[N][K]^T + bias + LN_res(res)), the
// kernels prior_sample_run launches for M rows.  workspace: decode_stage_workspace_floats(M, N, K) floats, 16-byte aligned.
size_t decode_stage_workspace_floats(int M, int N, int K) { return 4 + (size_t)M * ((K + MF_KC - 1) / MF_KC) * N; }
int decode_stage_f32(const float *x, int x_stride, const float *ln_g, const float *ln_b, const float *W, const float *bias,
                     const float *res, int res_stride, const float *res_g, const float *res_b, float *out, int out_stride,
                     int M, int N, int K, int relu, float eps, float *workspace, size_t workspace_floats, hipStream_t st) {
  if (!x || !W || !out || M <= 0 || M > 256 || N <= 0 || K <= 0) return invalid("decode_stage: bad argument");
  if ((K & 3) || (x_stride & 3) || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(W)) & 15))
    return invalid("decode_stage: K and x_stride must be multiples of 4, x and W 16-byte aligned");
  if ((ln_g == nullptr) != (ln_b == nullptr) || (res_g == nullptr) != (res_b == nullptr) || (res_g && !res))
    return invalid("decode_stage: LayerNorm weight and bias come together (and the residual's with a residual)");
  if (res_g && N > 512) return unsupported("decode_stage: a normalised residual has at most 512 features");
  if (K > 2048) return unsupported("decode_stage: K <= 2048");
  const Stage stage = Stage(x, K, W, bias, out, N, M).with_strides(x_stride, out_stride).with_eps(eps).with_ln(ln_g, ln_b)
                          .with_residual(res, res_stride, res_g, res_b).with_relu(relu != 0);
  float *ws = (workspace && !(reinterpret_cast<uintptr_t>(workspace) & 15)) ? workspace : nullptr;
  return launch_stage_rows(stage.a, nullptr, 1, 64, ws, ws ? workspace_floats : 0, Queue{st, false});
}

// A stage as the loop describes it (isi_decode_stage_ex_f32): the argument block through Stage and placed(), the kernel by
// stage_kernel(), the launch by launch_stage_rows() -- the loop's own plan with nothing forced.  What is checked here is what
// check_call guarantees the loop's stages (alignment, pairs), and every field the chosen kernel would not read.
int decode_stage_ex_f32(isi_decode_stage_args *g, hipStream_t st) {
  if (!g) return invalid("decode_stage_ex: null argument");
  g->kernel = ISI_STAGE_REFUSED;
  auto misaligned = [](const void *p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) != 0; };
  if (!g->x || !g->W || !g->out || g->M <= 0 || g->M > 256 || g->N <= 0 || g->K <= 0) return invalid("decode_stage_ex: bad argument");
  if ((g->K & 3) || (g->x_stride & 3) || (g->x_pos & 3) || misaligned(g->x, 16) || misaligned(g->W, 16))
    return invalid("decode_stage_ex: K, x_stride and x_pos must be multiples of 4, x and W 16-byte aligned");
  if ((g->ln_g == nullptr) != (g->ln_b == nullptr) || (g->res_g == nullptr) != (g->res_b == nullptr) || (g->res_g && !g->res))
    return invalid("decode_stage_ex: LayerNorm weight and bias come together (and the residual's with a residual)");
  if (g->ln_g && (misaligned(g->ln_g, 16) || misaligned(g->ln_b, 16))) return invalid("decode_stage_ex: ln_g and ln_b must be 16-byte aligned");
  if (g->out2 ? (g->split <= 0 || g->split >= g->N) : g->split != g->N)
    return invalid("decode_stage_ex: out2 takes the columns [split, N), 0 < split < N; without out2 split == N");
  if (g->out2_format != ISI_KV_F32 && g->out2_format != ISI_KV_BF16)
    return invalid("decode_stage_ex: out2_format must be ISI_KV_F32 (0) or ISI_KV_BF16 (1)");
  if (g->out2 && misaligned(g->out2, g->out2_format == ISI_KV_BF16 ? 16 : 4))
    return invalid("decode_stage_ex: a bf16 out2 must be 16-byte aligned");
  const bool moves = g->x_pos || g->res_pos || g->out2_pos;
  if (!moves && g->counter) return invalid("decode_stage_ex: counter on a stage none of whose addresses moves (x_pos, res_pos, out2_pos)");
  if (!moves && g->row_pos) return invalid("decode_stage_ex: row_pos on a stage none of whose addresses moves (x_pos, res_pos, out2_pos)");
  if (moves && !g->counter && g->p < 0) return invalid("decode_stage_ex: p < 0");
  if ((g->res_pos && !g->res) || (g->out2_pos && !g->out2)) return invalid("decode_stage_ex: res_pos / out2_pos without res / out2");
  if (g->stat_out && (!g->ln_g || misaligned(g->stat_out, 8))) return invalid("decode_stage_ex: stat_out needs ln_g and 8-byte alignment");
  if (g->res_stat && (!g->res_g || misaligned(g->res_stat, 8))) return invalid("decode_stage_ex: res_stat needs res_g and 8-byte alignment");
  if (g->part) {
    if (g->part_ns < 1 || g->part_ns > 8 || g->part_hd < 4 || (g->part_hd & 3) || g->K % g->part_hd || misaligned(g->part, 16))
      return invalid("decode_stage_ex: part needs 1 <= part_ns <= 8, part_hd a multiple of 4 that divides K, 16-byte alignment");
    if (g->ln_g || g->stat_out) return invalid("decode_stage_ex: part replaces the input row: no ln_g, no stat_out");
  }
  Stage stage = Stage(g->x, g->K, g->W, g->bias, g->out, g->N, g->M).with_strides(g->x_stride, g->out_stride).with_eps(g->eps)
                    .with_ln(g->ln_g, g->ln_b).with_residual(g->res, g->res_stride, g->res_g, g->res_b).with_relu(g->relu != 0);
  if (g->out2) {
    stage.with_out2(static_cast<float *>(g->out2), g->out2_stride, g->split, g->out2_format == ISI_KV_BF16);
    stage.a.out_stride = g->out_stride;
  }
  stage.advancing((long)g->x_pos, (long)g->res_pos, (long)g->out2_pos);
  stage.a.stat_out = g->stat_out;
  stage.a.res_stat = g->res_stat;
  const int p = g->counter ? -1 : g->p;
  const Where at{p, g->counter, g->row_pos ? g->row_pos + (p < 0 ? 0 : (size_t)p * g->M) : nullptr, nullptr};
  const RowLinArgs a = placed(stage.a, at);
  const StageKernel k = stage_kernel(a, g->part != nullptr);
  g->kernel = k == StageKernel::kOneRow ? ISI_STAGE_ONE_ROW : k == StageKernel::kTiles ? ISI_STAGE_TILES
              : k == StageKernel::kRowsInRegisters ? ISI_STAGE_ROWS_IN_REGISTERS
              : k == StageKernel::kGroupsOf8 ? ISI_STAGE_GROUPS_OF_8 : ISI_STAGE_REFUSED;
  if (int rc = stage_refusal(a, k)) return rc;
  if (g->part && k != StageKernel::kOneRow) return unsupported("decode_stage_ex: part is merged by the one-row kernel only (M == 1, K <= 512)");
  if (k == StageKernel::kGroupsOf8) {
    if (g->stat_out) return unsupported("decode_stage_ex: stat_out is not written by the groups-of-8 kernel");
    if (g->res_stat) return unsupported("decode_stage_ex: res_stat is not read by the groups-of-8 kernel");
  }
  float *ws = (g->workspace && !misaligned(g->workspace, 16)) ? g->workspace : nullptr;
  return launch_stage_rows(a, g->part, g->part_ns, g->part_hd, ws, ws ? g->workspace_floats : 0, Queue{st, false});
}

// The single-source cross-attention block alone (isi_decode_single_source_f32): SingleSourceArgs as single_source_block fills it
int decode_single_source_f32(const isi_decode_single_source_args *g, hipStream_t st) {
  if (!g || !g->y1 || !g->ln_g || !g->ln_b || !g->table || !g->y2) return invalid("decode_single_source: null pointer");
  if (g->B <= 0 || g->B > 256 || g->d <= 0) return invalid("decode_single_source: bad B or d");
  if (g->d > 64 * SS_RS) return unsupported("decode_single_source: d <= 1024");
  if (g->Cd < 1 || g->S_src < 1 || g->p < 0) return invalid("decode_single_source: Cd >= 1, S_src >= 1, p >= 0");
  if (!((g->table_B == g->B && g->table_sb == 1) || (g->table_B == 1 && g->table_sb == 0)))
    return invalid("decode_single_source: (table_B, table_sb) is (B, 1), or (1, 0) for a shared table");
  if (g->stat_out && (reinterpret_cast<uintptr_t>(g->stat_out) & 7)) return invalid("decode_single_source: stat_out must be 8-byte aligned");
  if (g->row_pos && !g->row_pos_host) return invalid("decode_single_source: row_pos comes with its host copy row_pos_host");
  for (int m = 0; m < (g->row_pos ? g->B : 1); ++m) {
    const int pm = g->row_pos ? g->row_pos_host[(size_t)g->p * g->B + m] : g->p;
    if (pm < 0 || pm / g->Cd >= g->S_src) return invalid("decode_single_source: a position without a source row (p / Cd >= S_src)");
  }
  SingleSourceArgs ss{};
  ss.y1 = g->y1; ss.ln_g = g->ln_g; ss.ln_b = g->ln_b; ss.table = g->table; ss.y2 = g->y2; ss.stat_out = g->stat_out;
  ss.pos = g->counter; ss.p = g->counter ? 0 : g->p; ss.Cd = g->Cd; ss.S_src = g->S_src; ss.B = g->B; ss.d = g->d; ss.eps = g->eps;
  ss.row_pos = g->row_pos ? (g->counter ? g->row_pos : g->row_pos + (size_t)g->p * g->B) : nullptr;
  ss.table_B = g->table_B; ss.table_sb = g->table_sb;
  return launch_single_source_cross(ss, st);
}

size_t prior_decode_scratch_floats(const isi_prior_w *w, int B) {
  if (!w || B <= 0) return 0;
  return carve(w, B, nullptr).floats;
}

int prior_sample_run(const isi_prior_w *w, const isi_prior_state *s, int p_begin, int p_end, float temperature,
                     int top_k, float top_p, hipStream_t st, const isi_prior_code_bias *cb) {
  return sample_run_impl(w, s, nullptr, p_begin, p_end, temperature, top_k, top_p, st, cb);
}

// Ragged batches: the plan is checked on the host, from its host copies, before anything is launched.
int prior_sample_run_rows(const isi_prior_w *w, const isi_prior_state *s, const isi_prior_rows *rows, int t_begin, int t_end,
                          float temperature, int top_k, float top_p, hipStream_t st, const isi_prior_code_bias *cb) {
  if (!w || !s || !rows) return invalid("prior_sample_run_rows: null pointer");
  if (s->B <= 0 || s->B > 256) return unsupported("prior_sample_run_rows: batch size must be 1..256");
  if (int rc = check_code_bias(cb, s->B)) return rc;
  if (s->memory_shared)
    return unsupported("prior_sample_run_rows: memory_shared (one source for all rows) is not built for ragged plans -- rows of "
                       "a plan are independent requests");
  if (!rows->pos || !rows->commit || !rows->pos_host || !rows->commit_host) return invalid("prior_sample_run_rows: null plan pointer");
  if (rows->n_steps < 0 || t_begin < 0 || t_end > rows->n_steps || t_begin > t_end) return invalid("prior_sample_run_rows: bad step range");
  if (w->d_model > 2048) return unsupported("prior_sample_run_rows: ragged rows need d_model <= 2048");
  const int B = s->B, i_off = s->start_len - 1;
  for (int t = 0; t < rows->n_steps; ++t) {
    for (int b = 0; b < B; ++b) {
      const size_t tb = (size_t)t * B + b;
      const int p = rows->pos_host[tb];
      if (p < 0 || p >= s->S_t) return invalid("prior_sample_run_rows: a position outside [0, S_t)");
      if (t > 0) {
        const int dp = p - rows->pos_host[tb - B];
        if (dp != 0 && dp != 1) return invalid("prior_sample_run_rows: a row moves by other than 0 or 1 position per step");
      }
      if (rows->commit_host[tb] && (p - i_off < 0 || p - i_off >= s->S))
        return invalid("prior_sample_run_rows: a commit outside the token range [0, S)");
    }
  }
  return sample_run_impl(w, s, rows, t_begin, t_end, temperature, top_k, top_p, st, cb);
}

}  // namespace isi
