// Host tracer of the prior's decoding loop (csrc/prior_sample_run.cpp), no GPU.
//
// prior_sample_run.cpp is pure host code: it decides which kernels a sampling call enqueues, with which pointers, shapes
// and flags, which of them it captures into graphs and when it replays those.  This program links it against stubs of
// everything it calls: a launcher stub appends one line to a trace instead of launching, the attention's split counts
// are the shipped formulas, and the HIP runtime entry points record what they are asked -- a capture diverts the lines of
// its stream into a graph object, a graph launch appends `replay` with that graph's digest and launch count, events and
// synchronisations leave a line each.  Pointers are fake: every tensor, weight and the scratch is a "region" with a base
// address of its own, nothing on the device is dereferenced, a traced pointer reads `region+byte offset`.  Every case is
// enumerated below; nothing is random.  A case runs in a child process of its own: the graph cache is process-wide.
//
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I$ROCM_PATH/include -Iinclude -Iinteractive-spectrogram-inpainting_amd/csrc
//       tests/decode_plan_tracer.cpp interactive-spectrogram-inpainting_amd/csrc/prior_sample_run.cpp -o decode_plan_tracer
//   decode_plan_tracer               `# cases N`, then one line per case, its calls folded into it:
//                                    id  return codes  launches (one per call; a replay counts its graph's)
//                                    fnv1a64(the calls' traces)  launches per launcher
//   decode_plan_tracer --dump CASE   that case's whole trace (diff two builds' dumps to see what an edit changed)
// A call's trace starts with the size query (prior_decode_scratch_floats) and ends with the return code; a refused call's
// holds its message in between.
//
// tests/test_decode_plan_host.py holds the output to tests/decode_plan_trace.txt byte for byte.
//
// Case id: run/b<B>/d<d_model>.<nhead>.<dim_feedforward>/l<layers>/t<S_t>.<S_src>/o<options>/c<code bias>/
//          k<prior_graph>.<decode_mfma_rows>.<decode_no_stat_handoff>/p<positions>/m<mask>/x<scenario>/r<refusal>
//   o: 1 bf16 caches | 2 memory_shared | 4 cross_out (single-source) | 8 ragged plan | 16 token_log_probs
//   c: 0 off | 1 one index row | 2 one per batch row | 3 a zeroed struct
//   p: 0 empty | 1 one position | 2 three (too short for graphs) | 3 long: 44 positions, or all of a shorter sequence
//   m: 0 every position samples | 1 none | 2 alternating | 3 the first 20 sample, the rest keep
//   x: 0 one call | 1 the same call twice | 2 nine argument sets, then the first again | 3 the first instantiate fails,
//      the call twice | 4 the caller's stream is capturing
//   r: 0 none, else kRefusals[r - 1] (printed in the header)
// stage/m<M>/n<N>/k<K>/f<flags>/w<workspace>/r<refusal>: isi_decode_stage_f32 alone
//   f: 1 LayerNorm on the input | 2 residual | 4 LayerNorm on the residual | 8 ReLU;  w: 0 none | 1 given | 2 misaligned
// stagex/m<M>/n<N>/k<K>/s<split>/f<flags>/v<out2>/a<addressing>/w<workspace>/q<decode_mfma_rows>.<decode_stats_global>/
//        g<heads>.<head_dim>.<splits>.<kind>/h<hand-off>: isi_decode_stage_ex_f32, the route table of tests/tests_support.py
//   (DECODE_STAGE_CASES, the cases of tests/test_decode_stage_gpu.py; tests/test_decode_stage_host.py holds the two lists together)
//   v: 0 no out2 | 1 fp32 | 2 bf16;  a: 0 position by value | 1 device counter | 2 row_pos offset to its step | 3 row_pos beside
//   the counter;  w: 0 none | 1 given | 2 one float short;  g: merged attention partials (0.0.0.0: none);  h: 1 stat_out | 2 res_stat
#include <sys/wait.h>
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "isi_common.h"
#include "isi_internal.h"
#include "knobs.h"
#include "prior_decode.h"

namespace {

enum { O_KV16 = 1, O_SHARED = 2, O_SINGLE = 4, O_RAGGED = 8, O_LOGP = 16 };

const char *const kRefusals[] = {
    "w null", "state null", "0 layers", "17 layers", "B = 0", "B = 257", "p_begin < 0", "p_end beyond the sequence", "p_begin > p_end",
    "code_bias without its index", "code_bias_count 0", "code_bias_batch neither 1 nor B", "x_seq null", "kv_cache null",
    "memory_kv null", "codes null", "mask null", "uniforms null", "scratch null", "single-source with Ce = 2",
    "single-source without a source row for the last position", "scratch one float short", "dim_feedforward % 4", "d_model % nhead",
    "kv_format 2", "memory_shared 2", "bf16 caches, kv_cache 8 bytes off", "rows null", "plan pointer null", "n_steps < 0",
    "a position outside [0, S_t)", "a row moves by 2", "a commit outside [0, S)"};
constexpr int kNumRefusals = sizeof kRefusals / sizeof kRefusals[0];
enum { R_W_NULL = 1, R_S_NULL, R_LAYERS0, R_LAYERS17, R_B0, R_B257, R_PBEGIN, R_PEND, R_PORDER, R_CB_PAIR, R_CB_COUNT, R_CB_BATCH,
       R_XSEQ, R_KVCACHE, R_MEMKV, R_CODES, R_MASK, R_UNIFORMS, R_SCRATCH, R_SS_CE, R_SS_ROW, R_SHORT, R_FF4, R_DHEAD, R_KVFMT,
       R_SHAREDFMT, R_KV16_ALIGN, R_ROWS_NULL, R_PLAN_NULL, R_NSTEPS, R_POS_RANGE, R_POS_JUMP, R_COMMIT_RANGE };

// ---- the state of the running case
std::vector<std::string> g_regions;   // region i has base address (i + 1) << 40
std::string g_trace;
int g_launches;
std::map<std::string, int> g_kinds;   // launches per launcher (a replay adds its graph's)
isi::Knobs g_knobs;
bool g_caller_capturing;
int g_fail_instantiates;

struct Graph { std::string text; int launches = 0; std::map<std::string, int> kinds; };
Graph *g_capture;                     // lines of the capture stream go here
const hipStream_t kCaller = reinterpret_cast<hipStream_t>(0x10), kCapture = reinterpret_cast<hipStream_t>(0x20);

uint64_t fnv1a64(const std::string &s) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (unsigned char ch : s) { h ^= ch; h *= 0x100000001b3ull; }
  return h;
}
std::string hex(uint64_t v) { char b[24]; snprintf(b, sizeof b, "%016llx", (unsigned long long)v); return b; }

void *region(const std::string &name) {
  g_regions.push_back(name);
  return reinterpret_cast<void *>((uintptr_t)g_regions.size() << 40);
}
std::string ptr_text(const void *p) {
  if (!p) return "null";
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), r = a >> 40;
  if (r < 1 || r > g_regions.size()) return "wild:" + std::to_string(a);
  return g_regions[r - 1] + "+" + std::to_string(a & (((uintptr_t)1 << 40) - 1));
}
const char *stream_text(hipStream_t st) { return st == kCaller ? "caller" : st == kCapture ? "capture" : "wild"; }

void emit(const std::string &line, hipStream_t st, const char *kind) {   // kind: a launch; nullptr: a runtime call
  const bool captured = g_capture && st == kCapture;
  (captured ? g_capture->text : g_trace) += line + "\n";
  if (!kind) return;
  if (captured) { ++g_capture->launches; ++g_capture->kinds[kind]; }
  else { ++g_launches; ++g_kinds[kind]; }
}

struct Line {
  std::string s;
  const char *fn;
  explicit Line(const char *f) : s(f), fn(f) {}
  Line &i(const char *k, long long v) { s += ' '; s += k; s += '='; s += std::to_string(v); return *this; }
  Line &f(const char *k, double v) { char b[40]; snprintf(b, sizeof b, " %s=%.9g", k, v); s += b; return *this; }
  Line &p(const char *k, const void *v) { s += ' '; s += k; s += '='; s += ptr_text(v); return *this; }
  Line &rl(const isi::RowLinArgs &a) {
    return p("x", a.x).i("x_stride", a.x_stride).p("ln_g", a.ln_g).p("ln_b", a.ln_b).p("W", a.W).p("bias", a.bias).p("res", a.res)
        .i("res_stride", a.res_stride).p("res_g", a.res_g).p("res_b", a.res_b).p("out", a.out).i("out_stride", a.out_stride)
        .p("out2", a.out2).i("out2_stride", a.out2_stride).i("split", a.split).i("M", a.M).i("N", a.N).i("K", a.K).i("relu", a.relu)
        .f("eps", a.eps).p("pos", a.pos).i("x_pos", a.x_pos).i("res_pos", a.res_pos).i("out2_pos", a.out2_pos)
        .p("stat_out", a.stat_out).p("res_stat", a.res_stat).p("row_pos", a.row_pos).i("out2_bf16", a.out2_bf16);
  }
  Line &attn(const isi_attn_args &g) {
    return p("q", g.q).p("k", g.k).p("v", g.v).p("rel", g.rel_embeddings).p("dense_mask", g.dense_mask).p("out", g.out).i("Sq", g.Sq)
        .i("Sk", g.Sk).i("B", g.B).i("H", g.H).i("hd", g.head_dim).i("q_ss", g.q_ss).i("q_sb", g.q_sb).i("q_sh", g.q_sh)
        .i("k_ss", g.k_ss).i("k_sb", g.k_sb).i("k_sh", g.k_sh).i("v_ss", g.v_ss).i("v_sb", g.v_sb).i("v_sh", g.v_sh).i("o_ss", g.o_ss)
        .i("o_sb", g.o_sb).i("o_sh", g.o_sh).i("Cq", g.Cq).i("Ck", g.Ck).i("Ek", g.Ek).i("rel_rows", g.rel_rows)
        .i("mask_mode", g.mask_mode).f("scale", g.scale).p("lse", g.lse).i("precision", g.precision).p("logits", g.logits)
        .i("logits_ld", g.logits_ld).p("workspace", g.workspace).i("workspace_bytes", (long long)g.workspace_bytes);
  }
  int done(hipStream_t st) { s += " st="; s += stream_text(st); emit(s, st, fn); return ISI_OK; }
};
#define I(x) i(#x, (long long)(x))
#define F(x) f(#x, (double)(x))
#define P(x) p(#x, x)

void runtime_call(const std::string &line, hipStream_t st = nullptr) { emit(line, st, nullptr); }

}  // namespace

// ---------------------------------------------------------------- what prior_sample_run.cpp calls
namespace isi {

Knobs &knobs() { return g_knobs; }
void set_last_error(const char *msg) { g_trace += "error: "; g_trace += msg; g_trace += '\n'; }

// transformer_ops.hip, as shipped
int rel_attention_decode_splits(int Sk, int pairs) {
  const int by_keys = Sk <= 192 ? 1 : (Sk + 127) / 128 > 8 ? 8 : (Sk + 127) / 128;
  const int by_chip = pairs <= 0 ? 8 : (512 + pairs - 1) / pairs;
  return by_keys < by_chip ? by_keys : (by_chip < 1 ? 1 : by_chip);
}
size_t rel_attention_decode_workspace_floats(int B, int H, int head_dim) { return (size_t)B * H * 8 * (head_dim + 4); }
// rel_attention_decode_shared.hip, as shipped (row blocks of SH_RB = 16 rows, key tiles of SH_KT = 64)
int rel_attention_decode_shared_splits(int Sk, int B, int H) {
  const int groups = H * ((B + 15) / 16), tiles = (Sk + 63) / 64;
  const int by_keys = tiles > 8 ? 8 : tiles, by_chip = groups <= 0 ? 8 : (512 + groups - 1) / groups;
  const int ns = by_keys < by_chip ? by_keys : by_chip;
  return ns < 1 ? 1 : ns;
}

int launch_row_gemv1(const RowLinArgs &a, const float *part, int NS, int HD, hipStream_t st) {
  return Line("row_gemv1").rl(a).P(part).I(NS).I(HD).done(st);
}
int launch_row_gemvm(const RowLinArgs &a, hipStream_t st) { return Line("row_gemvm").rl(a).done(st); }
int launch_row_mfma(const RowLinArgs &a, hipStream_t st, float *ksplit_ws, size_t ksplit_floats) {
  return Line("row_mfma").rl(a).P(ksplit_ws).I(ksplit_floats).done(st);
}
int launch_row_linear_8(const RowLinArgs &a, hipStream_t st) {
  if (row_linear_lds_bytes(a.M, a.K) > kRowLinearLdsMax) return unsupported("row_linear: rows do not fit in LDS");   // as shipped
  return Line("row_linear_8").rl(a).done(st);
}
int launch_single_source_cross(const SingleSourceArgs &a, hipStream_t st) {
  return Line("single_source_cross").p("y1", a.y1).p("ln_g", a.ln_g).p("ln_b", a.ln_b).p("table", a.table).p("y2", a.y2)
      .p("stat_out", a.stat_out).p("pos", a.pos).i("p", a.p).i("Cd", a.Cd).i("S_src", a.S_src).i("B", a.B).i("d", a.d).f("eps", a.eps)
      .p("row_pos", a.row_pos).i("table_B", a.table_B).i("table_sb", a.table_sb).done(st);
}
int launch_set_pos(int *pos, int value, int add, hipStream_t st) { return Line("set_pos").P(pos).I(value).I(add).done(st); }
int rel_attention_decode_launch(const isi_attn_args *g, int q_pos, const int *pos, int self_keys, float *workspace, int combine,
                                hipStream_t st, const int *row_pos, int kv_format) {
  return Line("attention_decode").attn(*g).I(q_pos).P(pos).I(self_keys).P(workspace).I(combine).P(row_pos).I(kv_format).done(st);
}
int rel_attention_decode_shared_launch(const isi_attn_args *g, int q_pos, const int *pos, float *workspace, int combine,
                                       int kv_format, hipStream_t st) {
  return Line("attention_decode_shared").attn(*g).I(q_pos).P(pos).P(workspace).I(combine).I(kv_format)
      .i("splits", rel_attention_decode_shared_splits(g->Sk, g->B, g->H)).done(st);
}
int sample_row_commit_f32(const float *logits, int stride, int rows, int n, float temperature, int top_k, float top_p, const float *u,
                          int64_t *out, float *filtered, const int *pos, int pos_off, const SampleCommit &cm, hipStream_t st,
                          const SampleRows *ragged, const SampleBias *bias) {
  Line l("sample_row_commit");
  l.P(logits).I(stride).I(rows).I(n).F(temperature).I(top_k).F(top_p).P(u).P(out).P(filtered).P(pos).I(pos_off)
      .p("cm.table", cm.table).i("cm.eff", cm.eff).p("cm.codes", cm.codes).i("cm.codes_stride", cm.codes_stride)
      .i("cm.p_value", cm.p_value).i("cm.i_off", cm.i_off).i("cm.S_t", cm.S_t).p("cm.x_seq", cm.x_seq).i("cm.x_stride", cm.x_stride)
      .p("cm.advance", cm.advance).p("cm.log_probs", cm.log_probs);
  if (ragged)
    l.p("rows.row_pos", ragged->row_pos).p("rows.commit", ragged->commit).p("rows.temperature", ragged->temperature)
        .p("rows.top_k", ragged->top_k).p("rows.top_p", ragged->top_p).i("rows.S", ragged->S);
  else l.p("rows", nullptr);
  if (bias)
    l.p("bias.table", bias->table).i("bias.table_stride", bias->table_stride).i("bias.count", bias->count).p("bias.index", bias->index)
        .i("bias.index_stride", bias->index_stride).i("bias.S", bias->S);
  else l.p("bias", nullptr);
  return l.done(st);
}

}  // namespace isi

// ---------------------------------------------------------------- the HIP runtime entry points it calls
hipError_t hipGetDevice(int *device) { *device = 0; return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipStreamIsCapturing(hipStream_t st, hipStreamCaptureStatus *status) {
  *status = g_caller_capturing ? hipStreamCaptureStatusActive : hipStreamCaptureStatusNone;
  runtime_call(std::string("hipStreamIsCapturing st=") + stream_text(st) + " -> " + (g_caller_capturing ? "active" : "none"));
  return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *st, unsigned flags) {
  *st = kCapture;
  runtime_call("hipStreamCreateWithFlags flags=" + std::to_string(flags));
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t st) { runtime_call(std::string("hipStreamDestroy st=") + stream_text(st)); return hipSuccess; }
hipError_t hipStreamBeginCapture(hipStream_t st, hipStreamCaptureMode mode) {
  runtime_call(std::string("hipStreamBeginCapture st=") + stream_text(st) + " mode=" + std::to_string((int)mode));
  g_capture = new Graph();
  return hipSuccess;
}
hipError_t hipStreamEndCapture(hipStream_t st, hipGraph_t *graph) {
  Graph *g = g_capture;
  g_capture = nullptr;
  *graph = reinterpret_cast<hipGraph_t>(g);
  runtime_call(std::string("hipStreamEndCapture st=") + stream_text(st) + " graph=" + hex(fnv1a64(g->text)) + " launches=" +
               std::to_string(g->launches) + " {\n" + g->text + "}");
  return hipSuccess;
}
hipError_t hipGraphInstantiate(hipGraphExec_t *exec, hipGraph_t graph, hipGraphNode_t *, char *, size_t) {
  const bool fail = g_fail_instantiates > 0;
  if (fail) --g_fail_instantiates;
  runtime_call("hipGraphInstantiate graph=" + hex(fnv1a64(reinterpret_cast<Graph *>(graph)->text)) + (fail ? " -> fails" : ""));
  if (fail) return hipErrorOutOfMemory;
  *exec = reinterpret_cast<hipGraphExec_t>(graph);      // (an executable stands for its graph)
  return hipSuccess;
}
hipError_t hipGraphLaunch(hipGraphExec_t exec, hipStream_t st) {
  const Graph *g = reinterpret_cast<const Graph *>(exec);
  runtime_call("replay graph=" + hex(fnv1a64(g->text)) + " launches=" + std::to_string(g->launches) + " st=" + stream_text(st));
  g_launches += g->launches;
  for (const auto &kv : g->kinds) g_kinds[kv.first] += kv.second;
  return hipSuccess;
}
hipError_t hipGraphExecDestroy(hipGraphExec_t exec) {
  runtime_call("hipGraphExecDestroy graph=" + hex(fnv1a64(reinterpret_cast<Graph *>(exec)->text)));
  return hipSuccess;
}
hipError_t hipGraphDestroy(hipGraph_t graph) {
  runtime_call("hipGraphDestroy graph=" + hex(fnv1a64(reinterpret_cast<Graph *>(graph)->text)));
  delete reinterpret_cast<Graph *>(graph);
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *ev, unsigned flags) {
  static uintptr_t n = 0;
  *ev = reinterpret_cast<hipEvent_t>(++n);
  runtime_call("hipEventCreateWithFlags flags=" + std::to_string(flags) + " -> event" + std::to_string(n));
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t st) {
  runtime_call("hipEventRecord event" + std::to_string(reinterpret_cast<uintptr_t>(ev)) + " st=" + stream_text(st));
  return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t ev) {
  runtime_call("hipEventSynchronize event" + std::to_string(reinterpret_cast<uintptr_t>(ev)));
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t ev) {
  runtime_call("hipEventDestroy event" + std::to_string(reinterpret_cast<uintptr_t>(ev)));
  return hipSuccess;
}
hipError_t hipDeviceSynchronize() { runtime_call("hipDeviceSynchronize"); return hipSuccess; }

// ---------------------------------------------------------------- cases
namespace {

struct Case {
  bool stage = false, stagex = false;
  // stagex
  int split = 0, kv = 0, addr = 0, stats_global = 0, ph = 0, hd = 0, ns = 0, kind = 0, handoff = 0;
  // run
  int B = 1, d = 64, heads = 4, ff = 128, layers = 2, S_t = 64, S_src = 16, opts = 0, bias = 0;
  int graph = 8, mfma_rows = 16, no_handoff = 0, range = 3, mask = 0, scenario = 0, refuse = 0;
  // stage
  int M = 1, N = 64, K = 64, flags = 0, ws = 1;
};

std::string case_id(const Case &c) {
  char b[200];
  if (c.stagex)
    snprintf(b, sizeof b, "stagex/m%d/n%d/k%d/s%d/f%d/v%d/a%d/w%d/q%d.%d/g%d.%d.%d.%d/h%d", c.M, c.N, c.K, c.split, c.flags, c.kv, c.addr,
             c.ws, c.mfma_rows, c.stats_global, c.ph, c.hd, c.ns, c.kind, c.handoff);
  else if (c.stage) snprintf(b, sizeof b, "stage/m%d/n%d/k%d/f%d/w%d/r%d", c.M, c.N, c.K, c.flags, c.ws, c.refuse);
  else
    snprintf(b, sizeof b, "run/b%d/d%d.%d.%d/l%d/t%d.%d/o%d/c%d/k%d.%d.%d/p%d/m%d/x%d/r%d", c.B, c.d, c.heads, c.ff, c.layers, c.S_t,
             c.S_src, c.opts, c.bias, c.graph, c.mfma_rows, c.no_handoff, c.range, c.mask, c.scenario, c.refuse);
  return b;
}

const float *fregion(const std::string &name) { return static_cast<const float *>(region(name)); }
isi_attn_w attn_w(const std::string &name) {
  return isi_attn_w{fregion(name + ".in_w"), fregion(name + ".in_b"), fregion(name + ".out_w"), fregion(name + ".out_b"),
                    fregion(name + ".rel"), 31};
}

void set_knobs(const Case &c) {
  memset(&g_knobs, 0, sizeof g_knobs);
  g_knobs.decode_nt = 1;
  g_knobs.prior_graph = c.graph; g_knobs.decode_mfma_rows = c.mfma_rows; g_knobs.decode_no_stat_handoff = c.no_handoff;
  g_knobs.decode_stats_global = c.stats_global;
}

struct CallResult { int rc, launches; };

// one call of the case; `variant` > 0: another temperature (another graph-cache key)
CallResult run_call(const Case &c, int variant) {
  g_regions.clear(); g_trace.clear(); g_launches = 0;
  const int r = c.refuse, i_off = 1;
  isi_prior_w w;
  memset(&w, 0, sizeof w);
  w.d_model = c.d; w.nhead = c.heads; w.dim_feedforward = c.ff; w.n_layers = c.layers; w.n_class = 70;
  w.Cd = 4; w.Ed = (c.S_t + 3) / 4; w.Ce = (c.opts & O_SINGLE) ? 1 : 4; w.Ee = c.S_src; w.eff_dim = c.d - 8;
  if (r == R_LAYERS0) w.n_layers = 0;
  if (r == R_LAYERS17) w.n_layers = 17;
  if (r == R_SS_CE) w.Ce = 2;
  if (r == R_FF4) w.dim_feedforward += 2;
  if (r == R_DHEAD) w.nhead = c.heads + 1;
  for (int l = 0; l < c.layers; ++l) {
    const std::string n = "L" + std::to_string(l);
    isi_decoder_layer_w &L = w.layers[l];
    L.self_attn = attn_w(n + ".self"); L.cross_attn = attn_w(n + ".cross");
    L.linear1_w = fregion(n + ".linear1_w"); L.linear1_b = fregion(n + ".linear1_b");
    L.linear2_w = fregion(n + ".linear2_w"); L.linear2_b = fregion(n + ".linear2_b");
    L.norm1_w = fregion(n + ".norm1_w"); L.norm1_b = fregion(n + ".norm1_b"); L.norm2_w = fregion(n + ".norm2_w");
    L.norm2_b = fregion(n + ".norm2_b"); L.norm3_w = fregion(n + ".norm3_w"); L.norm3_b = fregion(n + ".norm3_b");
  }
  w.logits_w = fregion("logits_w"); w.logits_b = fregion("logits_b"); w.embed_table = fregion("embed_table");

  isi_prior_state s;
  memset(&s, 0, sizeof s);
  s.B = r == R_B0 ? 0 : r == R_B257 ? 257 : c.B;
  s.S_t = c.S_t; s.S_src = c.S_src; s.S = c.S_t - 1; s.start_len = i_off + 1;
  if (r == R_SS_ROW) s.S_src = (c.S_t - 1) / w.Cd;
  std::vector<uint8_t> mask((size_t)s.S);
  for (int i = 0; i < s.S; ++i) mask[i] = c.mask == 0 ? 1 : c.mask == 1 ? 0 : c.mask == 2 ? (i & 1) : i < 20;
  s.x_seq = r == R_XSEQ ? nullptr : static_cast<float *>(region("x_seq"));
  s.kv_cache = r == R_KVCACHE ? nullptr : static_cast<float *>(region("kv_cache"));
  if (r == R_KV16_ALIGN) s.kv_cache += 2;
  s.memory_kv = (r == R_MEMKV || (c.opts & O_SINGLE)) ? nullptr : fregion("memory_kv");
  s.codes = r == R_CODES ? nullptr : static_cast<int64_t *>(region("codes"));
  s.mask = (r == R_MASK || (c.opts & O_RAGGED)) ? nullptr : mask.data();
  s.uniforms = r == R_UNIFORMS ? nullptr : fregion("uniforms");
  s.scratch = r == R_SCRATCH ? nullptr : static_cast<float *>(region("scratch"));
  s.scratch_floats = isi::prior_decode_scratch_floats(&w, s.B);
  g_trace = "scratch_floats=" + std::to_string(s.scratch_floats) + "\n";
  if (r == R_SHORT) --s.scratch_floats;
  s.memory_shared = r == R_SHAREDFMT ? 2 : (c.opts & O_SHARED) ? 1 : 0;
  if (c.opts & O_SINGLE) s.cross_out = fregion("cross_out");
  s.kv_format = r == R_KVFMT ? 2 : (c.opts & O_KV16) ? ISI_KV_BF16 : ISI_KV_F32;
  if (c.opts & O_LOGP) s.token_log_probs = static_cast<float *>(region("token_log_probs"));

  isi_prior_code_bias cb;
  memset(&cb, 0, sizeof cb);
  if (c.bias == 1 || c.bias == 2) {
    cb.code_bias = fregion("code_bias");
    cb.code_bias_index = static_cast<const int32_t *>(region("code_bias_index"));
    cb.code_bias_count = 5;
    cb.code_bias_batch = c.bias == 1 ? 1 : c.B;
  }
  if (r == R_CB_PAIR) { cb.code_bias = fregion("code_bias"); cb.code_bias_index = nullptr; }
  if (r == R_CB_COUNT) cb.code_bias_count = 0;
  if (r == R_CB_BATCH) cb.code_bias_batch = c.B + 1;
  const isi_prior_code_bias *cbp = c.bias || r == R_CB_PAIR ? &cb : nullptr;

  // positions [p0, p1) -- steps of the plan when ragged: row b follows two steps behind per (b % 3)
  int p0 = 2, p1 = c.range == 0 ? 2 : c.range == 1 ? 3 : c.range == 2 ? 5 : (c.S_t - 2 < 46 ? c.S_t - 2 : 46);
  if (r == R_PBEGIN) p0 = -1;
  if (r == R_PORDER) { p0 = 5; p1 = 4; }
  const float temperature = 1.0f + 0.125f * variant, top_p = 0.9f;
  const int top_k = 40;
  int rc;
  if (c.opts & O_RAGGED) {
    const int n_steps = c.S_t - 2, B = c.B;
    std::vector<int32_t> pos_host((size_t)n_steps * B);
    std::vector<uint8_t> commit_host((size_t)n_steps * B);
    for (int t = 0; t < n_steps; ++t)
      for (int b = 0; b < B; ++b) {
        const int lag = t - (b % 3) * 2;
        pos_host[(size_t)t * B + b] = i_off + (lag < 0 ? 0 : lag);
        commit_host[(size_t)t * B + b] = lag >= 0 && (c.mask == 0 ? 1 : c.mask == 1 ? 0 : c.mask == 2 ? (t & 1) : t < 20);
      }
    if (r == R_POS_RANGE) pos_host[(size_t)(n_steps - 1) * B] = c.S_t;
    if (r == R_POS_JUMP) for (int t = 3; t < n_steps; ++t) pos_host[(size_t)t * B] += 1;
    if (r == R_COMMIT_RANGE) { for (int t = 0; t < n_steps; ++t) pos_host[(size_t)t * B] = 0; commit_host[0] = 1; }
    isi_prior_rows rows;
    memset(&rows, 0, sizeof rows);
    rows.pos = static_cast<const int32_t *>(region("rows.pos")); rows.commit = static_cast<const uint8_t *>(region("rows.commit"));
    rows.pos_host = pos_host.data(); rows.commit_host = commit_host.data();
    if (B > 1) {      // (per-row sampling parameters on the batched cases)
      rows.temperature = fregion("rows.temperature"); rows.top_k = static_cast<const int32_t *>(region("rows.top_k"));
      rows.top_p = fregion("rows.top_p");
    }
    rows.n_steps = r == R_NSTEPS ? -1 : n_steps;
    if (r == R_PLAN_NULL) rows.commit = nullptr;
    if (r == R_PEND) p1 = n_steps + 1;
    rc = isi::prior_sample_run_rows(r == R_W_NULL ? nullptr : &w, r == R_S_NULL ? nullptr : &s, r == R_ROWS_NULL ? nullptr : &rows, p0, p1,
                                    temperature, top_k, top_p, kCaller, cbp);
  } else {
    if (r == R_PEND) p1 = c.S_t + 1;
    rc = isi::prior_sample_run(r == R_W_NULL ? nullptr : &w, r == R_S_NULL ? nullptr : &s, p0, p1, temperature, top_k, top_p, kCaller, cbp);
  }
  g_trace += "return " + std::to_string(rc) + "\n";
  return {rc, g_launches};
}

CallResult run_stage(const Case &c) {
  g_regions.clear(); g_trace.clear(); g_launches = 0;
  const int r = c.refuse;
  const float *x = r == 1 ? nullptr : fregion("x"), *W = fregion("W"), *bias = fregion("bias");
  if (r == 2) x += 1;                                   // not 16-byte aligned
  const float *ln_g = (c.flags & 1) ? fregion("ln_g") : nullptr, *ln_b = (c.flags & 1) && r != 3 ? fregion("ln_b") : nullptr;
  const float *res = (c.flags & 2) ? fregion("res") : nullptr;
  const float *res_g = (c.flags & 4) ? fregion("res_g") : nullptr, *res_b = (c.flags & 4) ? fregion("res_b") : nullptr;
  float *out = static_cast<float *>(region("out")), *ws = c.ws ? static_cast<float *>(region("workspace")) : nullptr;
  if (c.ws == 2) ws += 1;
  const size_t ws_floats = isi::decode_stage_workspace_floats(c.M, c.N, c.K);
  g_trace = "workspace_floats=" + std::to_string(ws_floats) + "\n";
  const int rc = isi::decode_stage_f32(x, c.K, ln_g, ln_b, W, bias, res, c.N, res_g, res_b, out, c.N, r == 4 ? 257 : c.M, c.N, c.K,
                                       (c.flags & 8) ? 1 : 0, 1e-5f, ws, ws_floats, kCaller);
  g_trace += "return " + std::to_string(rc) + "\n";
  return {rc, g_launches};
}

// isi_decode_stage_ex_f32 on a case of the route table: three positions of every position-addressed array, position / step 1
CallResult run_stagex(const Case &c) {
  g_regions.clear(); g_trace.clear(); g_launches = 0;
  isi_decode_stage_args g;
  memset(&g, 0, sizeof g);
  const int n2 = c.N - c.split;
  g.x = fregion("x"); g.x_stride = c.K; g.W = fregion("W"); g.bias = fregion("bias");
  if (c.flags & 1) { g.ln_g = fregion("ln_g"); g.ln_b = fregion("ln_b"); }
  if (c.flags & 2) { g.res = fregion("res"); g.res_stride = c.N; g.res_pos = (int64_t)c.M * c.N; }
  if (c.flags & 4) { g.res_g = fregion("res_g"); g.res_b = fregion("res_b"); }
  g.out = static_cast<float *>(region("out")); g.out_stride = c.split;
  if (c.kv) { g.out2 = region("out2"); g.out2_stride = n2; g.out2_format = c.kv == 2 ? ISI_KV_BF16 : ISI_KV_F32; g.out2_pos = (int64_t)c.M * n2; }
  g.split = c.split; g.M = c.M; g.N = c.N; g.K = c.K; g.relu = (c.flags & 8) ? 1 : 0; g.eps = 1e-5f;
  g.p = 1; g.x_pos = (int64_t)c.M * c.K;
  if (c.addr == 1 || c.addr == 3) g.counter = static_cast<const int *>(region("counter"));
  if (c.addr >= 2) g.row_pos = static_cast<const int *>(region("row_pos"));
  if (c.handoff & 1) g.stat_out = static_cast<float *>(region("stat_out"));
  if (c.handoff & 2) g.res_stat = fregion("res_stat");
  if (c.ph) { g.part = fregion("part"); g.part_ns = c.ns; g.part_hd = c.hd; }
  const size_t chunks = (size_t)c.M * ((c.K + 511) / 512) * c.N;
  if (c.ws) { g.workspace = static_cast<float *>(region("workspace")); g.workspace_floats = c.ws == 2 ? chunks - 1 : chunks + 4; }
  const int rc = isi::decode_stage_ex_f32(&g, kCaller);
  g_trace += "kernel " + std::to_string(g.kernel) + "\nreturn " + std::to_string(rc) + "\n";
  return {rc, g_launches};
}

// the whole case: its calls' traces, return codes and launch counts
struct CaseResult { std::string trace, rcs, ns; };
CaseResult run_case(const Case &c) {
  set_knobs(c);
  g_kinds.clear();
  g_caller_capturing = c.scenario == 4;
  g_fail_instantiates = c.scenario == 3 ? 1 : 0;
  std::vector<int> variants{0};
  if (c.scenario == 1 || c.scenario == 3) variants = {0, 0};
  if (c.scenario == 2) variants = {0, 1, 2, 3, 4, 5, 6, 7, 8, 0};
  CaseResult res;
  for (size_t i = 0; i < variants.size(); ++i) {
    const CallResult cr = c.stagex ? run_stagex(c) : c.stage ? run_stage(c) : run_call(c, variants[i]);
    res.trace += "call " + std::to_string(i) + ": " + g_trace;
    res.rcs += (i ? "," : "") + std::to_string(cr.rc);
    res.ns += (i ? "," : "") + std::to_string(cr.launches);
  }
  return res;
}

std::vector<Case> g_cases;
std::set<std::string> g_seen;
void add(const Case &c) {
  if (g_seen.insert(case_id(c)).second) g_cases.push_back(c);
}

const int kBatches[] = {1, 2, 8, 9, 16, 17, 47, 48, 256};
// d_model . nhead . dim_feedforward: small; d > 512 (no merge in the GEMV, N > 512 with a normalised residual); K = 2048 and
// just beyond, on and off the tiles' K % 8; d = 1024 and just beyond (single-source); rows beyond row_linear's LDS
struct Dims { int d, heads, ff; };
const Dims kDims[] = {{64, 4, 128}, {512, 8, 1024}, {544, 17, 128}, {64, 4, 2048}, {64, 4, 2052}, {64, 4, 2056}, {1024, 16, 128},
                      {1056, 33, 128}, {64, 4, 5120}};

// isi_decode_stage_ex_f32: DECODE_STAGE_CASES of tests/tests_support.py (_decode_stage_table), loop for loop
Case xcase(int M, int N, int K, int split, int flags, int kv = 0, int addr = 0, int ws = 0, int handoff = 0) {
  Case c;
  c.stagex = true; c.M = M; c.N = N; c.K = K; c.split = kv ? split : N; c.flags = flags; c.kv = kv; c.addr = addr; c.ws = ws;
  c.handoff = handoff;
  return c;
}
void enumerate_stagex() {
  const int ALL = 15, cyc[6] = {15, 1, 7, 11, 0, 2};
  // the one-row kernel
  { const int Ks[] = {64, 256, 260, 512, 516, 1024, 1028, 2048};
    for (int i = 0; i < 8; ++i)
      for (int kv : {1, 2}) add(xcase(1, 40, Ks[i], 7, cyc[i % 6] | 1, kv, ((i + kv) & 1) ? 1 : 0)); }
  for (int K : {64, 1028})
    for (int N : {1, 7, 8, 9}) {
      add(xcase(1, N, K, N, N != 8 ? ALL : 2, 0, N == 9 ? 1 : 0));
      if (N > 1) add(xcase(1, N, K, 3, 1, N == 8 ? 2 : 1));
    }
  for (int K : {256, 1024}) {
    add(xcase(1, 40, K, 40, 1 | 8, 0, 0, 0, 1));
    add(xcase(1, 40, K, 40, 2 | 4, 0, 1, 0, 2));
  }
  { const int parts[7][4] = {{4, 16, 1, 0}, {2, 32, 3, 0}, {8, 32, 2, 1}, {4, 64, 8, 2}, {8, 64, 3, 1}, {16, 32, 8, 0}, {8, 64, 2, 2}};
    for (int j = 0; j < 7; ++j) {
      Case c = xcase(1, 40, parts[j][0] * parts[j][1], 40, 2 | 4, 0, j & 1, 0, j % 3 == 2 ? 2 : 0);
      c.ph = parts[j][0]; c.hd = parts[j][1]; c.ns = parts[j][2]; c.kind = parts[j][3];
      add(c);
    } }
  // rows in registers
  { const int KM[16][2] = {{256, 2}, {256, 3}, {256, 8}, {256, 9}, {260, 4}, {260, 5}, {260, 17}, {512, 2}, {512, 5}, {516, 2}, {516, 3},
                           {516, 9}, {1024, 4}, {1028, 2}, {1028, 3}, {2048, 5}};
    for (int i = 0; i < 16; ++i)
      for (int addr : {(i & 1) ? 1 : 0, (i & 1) ? 3 : 2})
        for (int kv : {1, 2}) add(xcase(KM[i][1], 24, KM[i][0], 7, cyc[i % 6] | 1, kv, addr)); }
  for (int j = 0; j < 2; ++j) {
    const int M = j ? 9 : 3, addr = j ? 2 : 0;
    add(xcase(M, 24, 512, 24, 1, 0, addr, 0, 1));
    add(xcase(M, 24, 512, 24, ALL & ~1, 0, addr, 0, 2));
  }
  // 32-row tiles
  for (int M : {2, 31, 32, 33, 40}) { Case c = xcase(M, 33, 512, 16, ALL, 1, 0, 1); c.mfma_rows = M == 2 ? 1 : 16; add(c); }
  for (int N : {31, 32, 48}) add(xcase(33, N, 512, 16, 1 | 2, 2, 0, 1));
  for (int K : {8, 520, 2048})
    for (int ws : {1, 0, 2}) add(xcase(33, 48, K, 16, ALL, ws == 1 ? 2 : 1, ws == 1 ? 1 : 0, ws));
  for (int K : {8, 512}) { Case c = xcase(33, 48, K, 16, ALL, 1); c.stats_global = 1; add(c); }
  { const int Kw[3][2] = {{512, 0}, {2048, 1}, {2048, 0}};
    for (int i = 0; i < 3; ++i)
      for (int kv : {1, 2}) add(xcase(33, 48, Kw[i][0], 16, ALL, kv, kv == 1 ? 2 : 3, Kw[i][1])); }
  { const int Kws[4][3] = {{512, 0, 0}, {512, 0, 1}, {2048, 1, 0}, {2048, 0, 0}};
    for (int i = 0; i < 4; ++i) {
      { Case c = xcase(33, 48, Kws[i][0], 48, 1, 0, 0, Kws[i][1], 1); c.stats_global = Kws[i][2]; add(c); }
      add(xcase(33, 48, Kws[i][0], 48, 2 | 4, 0, Kws[i][2] ? 2 : 0, Kws[i][1], 2));
    } }
  { const int Kw[2][2] = {{512, 0}, {2048, 1}};
    for (int i = 0; i < 2; ++i) {
      add(xcase(33, 516, Kw[i][0], 516, 2 | 4, 0, 0, Kw[i][1], 2));
      add(xcase(33, 516, Kw[i][0], 516, 2 | 4, 0, 0, Kw[i][1]));
    } }
  add(xcase(33, 516, 512, 516, 2 | 4, 0, 2, 0, 2));
  add(xcase(33, 516, 512, 516, 2 | 4, 0, 2));
  // groups of 8 rows in LDS
  { const int Ms[] = {1, 2, 3, 4, 5, 8, 9};
    for (int i = 0; i < 7; ++i)
      for (int K : {2052, 2560}) add(xcase(Ms[i], 24, K, 7, cyc[i % 6] | 1, ((i + K / 4) & 1) ? 2 : 1, i % 3 == 0 ? 1 : 0)); }
  { const int NM[4][2] = {{516, 1}, {516, 3}, {1024, 1}, {1024, 9}};
    for (int i = 0; i < 4; ++i) add(xcase(NM[i][1], NM[i][0], 512, NM[i][0], ALL, 0, NM[i][1] == 3 ? 1 : 0)); }
  add(xcase(17, 24, 2056, 24, 2 | 8));
  add(xcase(17, 24, 2056, 24, 1 | 2));
  add(xcase(8, 24, 5116, 24, 1));
  add(xcase(8, 24, 5120, 24, 1));
  add(xcase(3, 24, 2052, 7, 1, 1, 2));
}

// One axis varies while the others stay at their defaults (Case's initialisers), plus the combinations the routes depend on.
void enumerate() {
  const int kForms[] = {0, O_SINGLE, O_RAGGED, O_RAGGED | O_SINGLE};   // plain, single-source, ragged, ragged single-source
  // every batch size on the default model; the other models at a batch size of each kernel family (two groups of 8 too)
  for (int B : kBatches)
    for (int o : kForms) { Case c; c.B = B; c.opts = o; add(c); }
  for (const Dims &dm : kDims)
    for (int B : {1, 8, 9, 17})
      for (int o : kForms) {
        if ((o & O_SINGLE) && dm.d == 64) continue;                    // (single-source depends on d_model alone)
        if (o == (O_RAGGED | O_SINGLE) && B != 9) continue;
        Case c; c.B = B; c.d = dm.d; c.heads = dm.heads; c.ff = dm.ff; c.opts = o; add(c);
      }
  // every option alone and the combinations that share code (shared memory x ragged is a refusal)
  for (int B : {1, 17, 47, 48})
    for (int o : {1, 2, 16, 3, 5, 6, 7, 9, 10, 13, 20, 24, 31}) { Case c; c.B = B; c.opts = o; add(c); }
  // layers: y3a / y3b alternate
  for (int l = 1; l <= 3; ++l)
    for (int B : {1, 17})
      for (int o : {0, (int)O_SINGLE}) { Case c; c.layers = l; c.B = B; c.opts = o; add(c); }
  // key splits of the two attentions: 1, 2 and 8 (the out-projection merges them at one row of d <= 512, not beyond)
  for (int St : {64, 256, 1024})
    for (int Ss : {16, 256, 1024}) {
      for (int B : {1, 48})
        for (int o : {0, (int)O_SHARED, (int)O_RAGGED}) {
          if (B == 48 && o == O_RAGGED) continue;
          Case c; c.S_t = St; c.S_src = Ss; c.B = B; c.opts = o; add(c);
        }
      Case c; c.S_t = St; c.S_src = Ss; c.d = kDims[2].d; c.heads = kDims[2].heads; c.ff = kDims[2].ff; add(c);
    }
  // code bias
  for (int cbias = 0; cbias <= 3; ++cbias)
    for (int B : {1, 9})
      for (int o : {0, (int)O_RAGGED, (int)O_LOGP}) { Case c; c.bias = cbias; c.B = B; c.opts = o; add(c); }
  // knobs: positions per graph; the tile boundary moved; no statistics hand-off
  for (int o : {0, (int)O_SINGLE, (int)O_RAGGED}) {
    for (int g : {0, 1})
      for (int B : {1, 9, 17}) { Case c; c.graph = g; c.B = B; c.opts = o; add(c); }
    for (int B : {1, 8, 9, 16, 17}) {
      { Case c; c.mfma_rows = 8; c.B = B; c.opts = o; add(c); }
      { Case c; c.no_handoff = 1; c.B = B; c.opts = o; add(c); }
      { Case c; c.mfma_rows = 8; c.no_handoff = 1; c.B = B; c.opts = o; add(c); }
    }
  }
  // position ranges x masks x positions per graph (the mask steers the windows of a long range)
  for (int p = 0; p <= 3; ++p)
    for (int m = 0; m <= (p == 3 ? 3 : 1); ++m)
      for (int g : {0, 1, 8}) {
        if (g == 1 && p < 3) continue;
        { Case c; c.range = p; c.mask = m; c.graph = g; add(c); }
        { Case c; c.range = p; c.mask = m; c.graph = g; c.opts = O_RAGGED; c.B = 2; add(c); }
      }
  // a sequence shorter than two windows
  for (int g : {1, 8}) { Case c; c.S_t = 16; c.graph = g; add(c); }
  // the graph cache
  for (int x = 1; x <= 4; ++x)
    for (int o : {0, (int)O_RAGGED, (int)O_KV16})
      for (int m : {0, 3}) { Case c; c.scenario = x; c.opts = o; c.mask = m; add(c); }
  for (int x : {1, 2}) { Case c; c.scenario = x; c.bias = 1; add(c); }
  // refusals (the ragged entry's own on a ragged plan; the others on both entries)
  for (int r = 1; r <= kNumRefusals; ++r)
    for (int o : {0, (int)O_RAGGED}) {
      Case c; c.refuse = r; c.opts = o; c.B = 2;
      if (r == R_SS_CE || r == R_SS_ROW) c.opts |= O_SINGLE;
      if (r == R_KV16_ALIGN) c.opts |= O_KV16;
      if (r >= R_ROWS_NULL && !(o & O_RAGGED)) continue;
      if (r == R_MASK && (o & O_RAGGED)) continue;                    // (a plan does not read the mask)
      add(c);
    }
  { Case c; c.d = 68; c.heads = 17; c.opts = O_KV16; add(c); }                 // bf16 caches need d_model % 8 == 0
  { Case c; c.d = 2052; c.heads = 4; c.opts = O_RAGGED; c.B = 2; add(c); }      // ragged rows need d_model <= 2048
  // isi_decode_stage_f32: the four stage shapes of three models at a row count of each kernel family; the workspace on tiles
  for (const Dims &dm : {kDims[0], kDims[1], kDims[3]})
    for (int st = 0; st < 4; ++st)
      for (int M : {1, 2, 9, 17, 256})
        for (int w = 0; w <= (M == 17 ? 2 : 0); ++w) {
          Case c; c.stage = true; c.M = M; c.ws = w;
          c.N = st == 0 ? 3 * dm.d : st == 2 ? dm.ff : dm.d;
          c.K = st == 3 ? dm.ff : dm.d;
          c.flags = st == 0 ? 1 : st == 2 ? 9 : 6;
          add(c);
        }
  for (int r = 1; r <= 4; ++r) { Case c; c.stage = true; c.M = 2; c.flags = 1; c.refuse = r; add(c); }
  { Case c; c.stage = true; c.M = 2; c.K = 66; add(c); }                       // K % 4
  { Case c; c.stage = true; c.M = 2; c.flags = 4; add(c); }                    // a residual's LayerNorm without a residual
  { Case c; c.stage = true; c.M = 2; c.N = 544; c.flags = 6; add(c); }         // a normalised residual of more than 512 features
  { Case c; c.stage = true; c.M = 2; c.K = 2052; add(c); }                     // K > 2048
  // no statistics hand-off at d_model > 512 on the tiles: the out-projections and linear2 (a normalised residual of 1024 features,
  // which the tile kernel does not reduce itself) leave the tiles -- groups of 8, in a ragged plan too (no stage with a normalised
  // residual moves with the position)
  for (int o : {0, (int)O_RAGGED}) { Case c; c.d = 1024; c.heads = 16; c.B = 17; c.no_handoff = 1; c.opts = o; add(c); }
  enumerate_stagex();
}

}  // namespace

int main(int argc, char **argv) {
  enumerate();
  const bool dump = argc == 3 && !strcmp(argv[1], "--dump");
  if (argc != 1 && !dump) {
    fprintf(stderr, "usage: %s [--dump CASE]\n", argv[0]);
    return 2;
  }
  if (!dump) {
    for (int i = 0; i < kNumRefusals; ++i) printf("# refusal %d = %s\n", i + 1, kRefusals[i]);
    printf("# cases %zu\n", g_cases.size());
  }
  for (const Case &c : g_cases) {
    if (dump && case_id(c) != argv[2]) continue;
    fflush(stdout);
    const pid_t child = fork();                          // the graph cache is process-wide: a process per case
    if (child < 0) return perror("fork"), 1;
    if (child == 0) {
      const CaseResult res = run_case(c);
      if (dump) fputs(res.trace.c_str(), stdout);
      else {
        std::string kinds;
        for (const auto &kv : g_kinds) kinds += (kinds.empty() ? "" : ",") + kv.first + ":" + std::to_string(kv.second);
        printf("%s  %s  %s  %s  %s\n", case_id(c).c_str(), res.rcs.c_str(), res.ns.c_str(), hex(fnv1a64(res.trace)).c_str(),
               kinds.empty() ? "-" : kinds.c_str());
      }
      fflush(stdout);
      _exit(0);
    }
    int status = 0;
    if (waitpid(child, &status, 0) != child || !WIFEXITED(status) || WEXITSTATUS(status) != 0) {
      fprintf(stderr, "case %s: the child failed (status %d)\n", case_id(c).c_str(), status);
      return 1;
    }
    if (dump) return 0;
  }
  if (dump) fprintf(stderr, "no such case: %s\n", argv[2]);
  return dump ? 2 : 0;
}
