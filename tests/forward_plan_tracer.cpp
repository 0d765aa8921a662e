// Host tracer of the VQ-VAE forward's launch sequence (csrc/vqvae_run.cpp), no GPU.
//
// vqvae_run.cpp is pure host code: it decides which kernels an encode / decode / forward call enqueues, with which
// pointers, shapes and flags.  This program links it against stubs of everything it calls: a launcher stub appends one
// line to a trace instead of launching, a predicate stub answers with the shipped condition of the kernel file it
// stands for (or "no" where the case denies that predicate).  Pointers are fake: every tensor, weight and the
// workspace is a "region" with a base address of its own, nothing is dereferenced, a traced pointer reads
// `region+byte offset`.  Every case is enumerated below; nothing is random.
//
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I$ROCM_PATH/include -Iinclude -Iinteractive-spectrogram-inpainting_amd/csrc
//       tests/forward_plan_tracer.cpp interactive-spectrogram-inpainting_amd/csrc/vqvae_run.cpp -o forward_plan_tracer
//   forward_plan_tracer               one line per case, its shapes folded into it:
//                                     id  return codes  launch counts (one per shape)  fnv1a64(the shapes' traces)
//   forward_plan_tracer --dump CASE   that case's whole trace (diff two builds' dumps to see what an edit changed)
// A shape's trace starts with the size query (isi_vqvae_workspace_bytes, isi_vqvae_pair_activations) and ends with
// the return code; a refused call's holds its message in between.
//
// tests/test_forward_plan_host.py holds the output to tests/forward_plan_trace.txt byte for byte.
//
// Case id: geometry.variant/p<precision>/w<w16>/q<no_quantize>/t<code tables>/m<mode>/o<outputs>/k<knobs>/d<deny>/
// r<refusal>/s<shape set>.  o: 1 quant_t | 2 quant_b | 4 id_t | 8 id_b | 16 scalars given (else null).  k: 1 no_pairs
// | 2 no_conv_first | 4 no_vq_fusion | 8 no_setup_fusion | 16 no_code_tables.  d: bit i denies kDenyNames[i].
// r: 0 none | 1 x null | 2 dec null | 3 both | 4 n_upsample + 1 | 5 n_upsample 0 | 6 workspace one byte short.
// s: kShapeSets[s].
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "isi_common.h"
#include "isi_internal.h"
#include "knobs.h"

namespace {

enum Deny { D_RES_FUSABLE = 1, D_RES_PAIR = 2, D_PAIR_SOURCES = 4, D_CONVT_SMALL = 8, D_CONVT_SMALL_PAIR = 16, D_TAIL = 32,
            D_VQ_FUSABLE = 64, D_VQ_FUSABLE_2SRC = 128, D_VQ_FUSABLE_1SRC = 256 };
// (the last two deny vq_conv1x1_fusable for the bottom / the top level alone: a fused top with a two-launch bottom)
const char *const kDenyNames[] = {"resblock_fusable", "resblock_pair_preferred", "conv_pair_sources_ok", "convT_small_applicable",
                                  "convT_small_pair_ok", "decoder_tail_ok", "vq_conv1x1_fusable", "vq_conv1x1_fusable(two sources)",
                                  "vq_conv1x1_fusable(one source)"};
enum { K_NO_PAIRS = 1, K_NO_CONV_FIRST = 2, K_NO_VQ_FUSION = 4, K_NO_SETUP_FUSION = 8, K_NO_CODE_TABLES = 16 };

// ---- the state of the running case
std::vector<std::string> g_regions;   // region i has base address (i + 1) << 40
std::string g_trace;
int g_launches;
isi::Knobs g_knobs;
unsigned g_deny;

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

struct Line {
  std::string s;
  explicit Line(const char *fn) : s(fn) {}
  Line &i(const char *k, long long v) { s += ' '; s += k; s += '='; s += std::to_string(v); return *this; }
  Line &p(const char *k, const void *v) { s += ' '; s += k; s += '='; s += ptr_text(v); return *this; }
  Line &src(const char *k, const isi_src *v) {
    if (!v) return p(k, nullptr);
    s += ' '; s += k; s += "={" + ptr_text(v->ptr);
    for (long long x : {(long long)v->C, (long long)v->sn, (long long)v->sc, (long long)v->sh, (long long)v->sw}) s += " " + std::to_string(x);
    s += '}';
    return *this;
  }
  Line &dst(const char *k, const isi_dst *v) {
    if (!v) return p(k, nullptr);
    s += ' '; s += k; s += "={" + ptr_text(v->ptr);
    for (long long x : {(long long)v->sn, (long long)v->sc, (long long)v->sh, (long long)v->sw}) s += " " + std::to_string(x);
    s += '}';
    return *this;
  }
  int done() { g_trace += s; g_trace += '\n'; ++g_launches; return ISI_OK; }
};
#define I(x) i(#x, (long long)(x))
#define P(x) p(#x, x)

bool shipped_vq_fusable(int C0, int C1, int D, int K) {   // vq_nearest.hip: vq_conv1x1_fusable, vq_planes_lds_bytes
  const int Kp = (K + 31) & ~31;
  const size_t lds = (size_t)Kp * 64 * 2 * sizeof(unsigned short) + ((size_t)2 * Kp + 8 + 1 + Kp / 32 + 3) * sizeof(float);
  return D == 64 && C0 > 0 && C0 % 32 == 0 && C1 % 32 == 0 && C0 + C1 <= 256 && lds <= 150 * 1024;
}

}  // namespace

// ---------------------------------------------------------------- the 24 symbols vqvae_run.cpp needs
namespace isi {

Knobs &knobs() { return g_knobs; }
void set_last_error(const char *msg) { g_trace += "error: "; g_trace += msg; g_trace += '\n'; }
int vq_num_partials(int64_t N) {   // vq_nearest.hip: vq_grid
  const int64_t n = (N + 255) / 256;
  return (int)(n < 256 ? (n < 1 ? 1 : n) : 256);
}

// predicates: the shipped conditions (resblock_f32.hip, resblock_pair_f16.hip, conv_igemm_f32.hip, convT_small_f32.hip,
// convT_pair_f16.hip, vq_nearest.hip), pure functions of their arguments, the case's knobs and its deny mask
bool resblock_fusable(int C, int R) { return !(g_deny & D_RES_FUSABLE) && C % 32 == 0 && C >= 32 && C <= 128 && R >= 1 && R <= 32; }
bool resblock_pair_preferred(int, int H, int W, int C, int R) {
  if ((g_deny & D_RES_PAIR) || g_knobs.no_resblock_pair_kernel || R != 32 || (C != 64 && C != 128)) return false;
  return g_knobs.respair_th || (long)H * W >= 1024;
}
bool conv_pair_sources_ok(int C0, int C1, int Cout, int taps) {
  return !(g_deny & D_PAIR_SOURCES) && C0 > 0 && C0 % kBK == 0 && C1 % kBK == 0 && Cout > 32 && Cout % 8 == 0 && taps * (C0 + C1) >= 128;
}
bool convT_small_applicable(int Cin, int Cout) { return !(g_deny & D_CONVT_SMALL) && Cout >= 1 && Cout <= 4 && (Cin == 32 || Cin == 64); }
bool convT_small_pair_ok(int Cin, int Cout) { return !(g_deny & D_CONVT_SMALL_PAIR) && Cin == 64 && Cout >= 1 && Cout <= 2; }
bool decoder_tail_ok(int Cin, int Cmid, int Cout) {
  const bool pair_ok = !g_knobs.no_convt_pair_kernel && Cin >= 16 && Cin % 16 == 0 && Cmid % 64 == 0 && Cmid <= 1024;   // convT_pair_ok
  return !(g_deny & D_TAIL) && !g_knobs.no_tail_fusion && pair_ok && Cmid == 64 && Cout >= 1 && Cout <= 2;
}
bool vq_conv1x1_fusable(int C0, int C1, int D, int K) {
  if ((g_deny & D_VQ_FUSABLE) || (g_deny & (C1 ? D_VQ_FUSABLE_2SRC : D_VQ_FUSABLE_1SRC))) return false;
  return shipped_vq_fusable(C0, C1, D, K);
}

// launchers: one trace line each
int conv2d_f32(const isi_src *s0, const isi_src *s1, const float *packed_w, const float *bias, const isi_src *res,
               const isi_dst *dst, int B, int H, int W, int Cout, int KH, int KW, int stride, int pad, int relu, hipStream_t,
               const float *gate, float *twin, int32_t *zero, int zero_words) {
  return Line("conv2d_f32").src("s0", s0).src("s1", s1).P(packed_w).P(bias).src("res", res).dst("dst", dst).I(B).I(H).I(W)
      .I(Cout).I(KH).I(KW).I(stride).I(pad).I(relu).P(gate).P(twin).P(zero).I(zero_words).done();
}
int resblock_f32(const float *in, const float *w1, const float *b1, const float *w2, const float *b2, float *out, int B, int H,
                 int W, int C, int R, int relu, hipStream_t, float *twin, float *hidden) {
  return Line("resblock_f32").P(in).P(w1).P(b1).P(w2).P(b2).P(out).I(B).I(H).I(W).I(C).I(R).I(relu).P(twin).P(hidden).done();
}
int conv_transpose2d_k4s2_f32(const isi_src *s, const float *packed_w, const float *bias, const isi_dst *dst, int B, int H,
                              int W, int Cout, int relu, hipStream_t, const float *gate, float *twin) {
  return Line("conv_transpose2d_k4s2_f32").src("s", s).P(packed_w).P(bias).dst("dst", dst).I(B).I(H).I(W).I(Cout).I(relu)
      .P(gate).P(twin).done();
}
int decoder_tail_f32(const float *in_pair, const float *packed_w1, const float *bias1, const float *packed_w2,
                     const float *bias2, float *yprime_ws, const isi_dst *dst, int B, int H, int W, int Cin, int Cmid, int Cout,
                     hipStream_t) {
  return Line("decoder_tail_f32").P(in_pair).P(packed_w1).P(bias1).P(packed_w2).P(bias2).P(yprime_ws).dst("dst", dst).I(B).I(H)
      .I(W).I(Cin).I(Cmid).I(Cout).done();
}
int vq_zero_counts(int32_t *counts, int K, hipStream_t) { return Line("vq_zero_counts").P(counts).I(K).done(); }
int vq_nearest_f32(const float *z, const float *codes, const float *e2, int64_t *idx, float *q, int32_t *counts,
                   float *sse_part, int64_t N, int D, int K, int flags, hipStream_t) {
  return Line("vq_nearest_f32").P(z).P(codes).P(e2).P(idx).P(q).P(counts).P(sse_part).I(N).I(D).I(K).I(flags).done();
}
int vq_finalize_f32(const float *sse_part, int n_part, const int32_t *counts, int K, int64_t N, int D, float *out2, hipStream_t) {
  return Line("vq_finalize_f32").P(sse_part).I(n_part).P(counts).I(K).I(N).I(D).P(out2).done();
}
int vq_finalize2_f32(const float *sse_t, int np_t, const int32_t *counts_t, int K_t, int64_t N_t, const float *sse_b, int np_b,
                     const int32_t *counts_b, int K_b, int64_t N_b, int D, float *out5, hipStream_t) {
  return Line("vq_finalize2_f32").P(sse_t).I(np_t).P(counts_t).I(K_t).I(N_t).P(sse_b).I(np_b).P(counts_b).I(K_b).I(N_b).I(D)
      .P(out5).done();
}
int vq_conv1x1_nearest_f32(const isi_src *s0, const isi_src *s1, const float *w16, const float *bias, const float *codes,
                           const float *e2, int64_t *idx, float *q, float *q_pair, int32_t *counts, float *sse_part,
                           float *workspace, int B, int H, int W, int D, int K, hipStream_t, bool zero_counts, float *z_out,
                           const float *wfrag_packed, const void *planes) {
  return Line("vq_conv1x1_nearest_f32").src("s0", s0).src("s1", s1).P(w16).P(bias).P(codes).P(e2).P(idx).P(q).P(q_pair).P(counts)
      .P(sse_part).P(workspace).I(B).I(H).I(W).I(D).I(K).I(zero_counts).P(z_out).P(wfrag_packed).P(planes).done();
}
int vq_code_gather_f32(const int64_t *ids, const float *t3, const float *bias3, float *out3, int C3, int out3_pair, int relu3,
                       const float *tu, const float *biasU, float *outU, int CU, int outU_pair, int reluU, int B, int H, int W,
                       int K, hipStream_t) {
  return Line("vq_code_gather_f32").P(ids).P(t3).P(bias3).P(out3).I(C3).I(out3_pair).I(relu3).P(tu).P(biasU).P(outU).I(CU)
      .I(outU_pair).I(reluU).I(B).I(H).I(W).I(K).done();
}
int vq_scalars_sum_f32(float *out5, hipStream_t) { return Line("vq_scalars_sum_f32").P(out5).done(); }
int vq_unquantized_scalars(float *scalars2, hipStream_t) { return Line("vq_unquantized_scalars").P(scalars2).done(); }
int pair_encode_f32(const float *x, float *out, int64_t n, hipStream_t) { return Line("pair_encode_f32").P(x).P(out).I(n).done(); }

}  // namespace isi

// ---------------------------------------------------------------- models
namespace {

struct Geo { const char *name; int in, C, n_res, R, D, Kt, Kb, fb, ft, noq; };
const Geo kGeos[] = {
    {"default", 2, 128, 2, 32, 64, 512, 512, 4, 2, 0},      // the constructor's defaults on two-channel spectrograms
    {"default_in1", 1, 128, 2, 32, 64, 512, 512, 4, 2, 0},
    {"default_in3", 3, 128, 2, 32, 64, 512, 512, 4, 2, 0},  // (the constructor's own in_channel)
    {"small", 2, 32, 2, 8, 16, 64, 64, 4, 2, 0},            // tests/golden/vqvae_small.npz
    {"f8_f4", 2, 16, 1, 8, 8, 32, 32, 8, 4, 0},             // vqvae_f8_f4.npz
    {"f16_f2", 2, 16, 1, 8, 8, 32, 32, 16, 2, 0},           // vqvae_f16_f2.npz
    {"unquantized", 2, 32, 1, 8, 16, 64, 64, 4, 2, 1},      // vqvae_unquantized.npz
};
const char *const kVariants[] = {"base", "nres0", "nres1", "c32", "k544_512", "k512_1024"};
Geo variant(Geo g, int v) {
  if (v == 1) g.n_res = 0;
  if (v == 2) g.n_res = 1;
  if (v == 3) g.C = 32;                      // 32-channel layers: not pair-eligible
  if (v == 4) { g.Kt = 544; g.Kb = 512; }
  if (v == 5) { g.Kt = 512; g.Kb = 1024; }   // a bottom codebook beyond the fused search's LDS: fused top, two-launch bottom
  return g;
}

struct Shape { int B, H, W; };
// (3, 64, 136) is ragged: a cropped bottom grid.  Set 2, refused by their shape: grids whose halves do not double back,
// and (1, 8, 4): a one-column bottom grid under a top grid that up-samples to two columns
const std::vector<Shape> kShapeSets[] = {{{1, 8, 8}, {2, 16, 24}, {3, 64, 136}, {64, 256, 1024}},
                                         {{1, 8, 8}, {3, 64, 136}},
                                         {{1, 1, 8}, {1, 20, 32}, {1, 8, 4}}};

struct Case {
  int geo = 0, var = 0, prec = 4, w16 = 2, noq = -1, tab = 1, mode = 3, outs = 31, knobs = 0, deny = 0, refuse = 0, shapes = 0;
};

std::string model_id(const Case &c) {
  const Geo g = variant(kGeos[c.geo], c.var);
  char b[160];
  snprintf(b, sizeof b, "%s.%s/p%d/w%d/q%d/t%d", g.name, kVariants[c.var], c.prec, c.w16, c.noq < 0 ? g.noq : c.noq, c.tab);
  return b;
}
std::string case_id(const Case &c) {
  char b[96];
  snprintf(b, sizeof b, "/m%d/o%d/k%d/d%d/r%d/s%d", c.mode, c.outs, c.knobs, c.deny, c.refuse, c.shapes);
  return model_id(c) + b;
}

isi_conv_w conv(const std::string &name, int Cin, int Cout) {
  return isi_conv_w{static_cast<const float *>(region(name + ".w")), static_cast<const float *>(region(name + ".b")), Cin, Cout};
}
// channel ladders of the strided stacks (vqvae/encoder_decoder.py: _down_channels, _up_channels)
std::vector<int> ladder(int first, int C, int last, int factor, bool down) {
  std::vector<int> mid;
  if (factor == 16) mid = {C / 4, C / 2, 3 * C / 4};
  if (factor == 8) mid = {C / 2, C / 2};
  if (factor == 4) mid = {C / 2};
  std::vector<int> ch{down ? first : C};
  if (down) ch.insert(ch.end(), mid.begin(), mid.end()); else ch.insert(ch.end(), mid.rbegin(), mid.rend());
  ch.push_back(down ? C : last);
  if (down && factor == 2) ch.back() = C / 2;
  return ch;
}
template <class Stack>
void res_stack(Stack &s, const std::string &name, int C, int n_res, int R) {
  s.n_res = n_res;
  for (int i = 0; i < n_res; ++i) {
    s.res3[i] = conv(name + ".res3_" + std::to_string(i), C, R);
    s.res1[i] = conv(name + ".res1_" + std::to_string(i), R, C);
  }
}
isi_encoder_w encoder(const std::string &name, int in, int C, int n_res, int R, int factor) {
  isi_encoder_w e;
  memset(&e, 0, sizeof e);
  const std::vector<int> ch = ladder(in, C, 0, factor, true);
  e.n_down = (int)ch.size() - 1;
  for (int i = 0; i < e.n_down; ++i) e.down[i] = conv(name + ".down" + std::to_string(i), ch[i], ch[i + 1]);
  e.conv3 = conv(name + ".conv3", ch.back(), C);
  res_stack(e, name, C, n_res, R);
  return e;
}
isi_decoder_w decoder(const std::string &name, int in, int out, int C, int n_res, int R, int factor) {
  isi_decoder_w d;
  memset(&d, 0, sizeof d);
  d.conv3 = conv(name + ".conv3", in, C);
  res_stack(d, name, C, n_res, R);
  const std::vector<int> ch = ladder(0, C, out, factor, false);
  d.n_up = (int)ch.size() - 1;
  for (int i = 0; i < d.n_up; ++i) d.up[i] = conv(name + ".up" + std::to_string(i), ch[i], ch[i + 1]);
  return d;
}
isi_codebook_w codebook(const std::string &name, int D, int K, bool noq) {
  isi_codebook_w c;
  memset(&c, 0, sizeof c);
  c.D = D; c.K = K;
  if (noq) return c;               // UnquantizedBottleneck: the codebook is never read
  c.codes_kd = static_cast<const float *>(region(name + ".codes"));
  c.e2 = static_cast<const float *>(region(name + ".e2"));
  if (shipped_vq_fusable(32, 0, D, K)) c.planes = region(name + ".planes");
  return c;
}
isi_vqvae_w model(const Case &c) {
  const Geo g = variant(kGeos[c.geo], c.var);
  const bool noq = (c.noq < 0 ? g.noq : c.noq) != 0;
  isi_vqvae_w w;
  memset(&w, 0, sizeof w);
  w.in_channel = g.in;
  w.enc_b = encoder("enc_b", g.in, g.C, g.n_res, g.R, g.fb);
  w.enc_t = encoder("enc_t", g.C, g.C, g.n_res, g.R, g.ft);
  w.quantize_conv_t = conv("quantize_conv_t", g.C, g.D);
  w.quantize_conv_b = conv("quantize_conv_b", g.D + g.C, g.D);
  w.quantize_t = codebook("quantize_t", g.D, g.Kt, noq);
  w.quantize_b = codebook("quantize_b", g.D, g.Kb, noq);
  w.dec_t = decoder("dec_t", g.D, g.D, g.C, g.n_res, g.R, g.ft);
  w.dec = decoder("dec", 2 * g.D, g.in, g.C, g.n_res, g.R, g.fb);
  for (int f = g.ft; f > 1; f /= 2, ++w.n_upsample) w.upsample[w.n_upsample] = conv("upsample" + std::to_string(w.n_upsample), g.D, g.D);
  if (c.refuse == 4) ++w.n_upsample;
  if (c.refuse == 5) w.n_upsample = 0;
  w.w16 = c.w16; w.precision = c.prec; w.no_quantize = noq;
  if (c.tab) {
    w.code_table_conv3 = static_cast<const float *>(region("code_table_conv3"));
    w.code_table_upsample = static_cast<const float *>(region("code_table_upsample"));
  }
  return w;
}

void set_case_state(const Case &c) {
  g_regions.clear(); g_trace.clear(); g_launches = 0;
  memset(&g_knobs, 0, sizeof g_knobs);
  g_knobs.no_pairs = !!(c.knobs & K_NO_PAIRS); g_knobs.no_conv_first = !!(c.knobs & K_NO_CONV_FIRST);
  g_knobs.no_vq_fusion = !!(c.knobs & K_NO_VQ_FUSION); g_knobs.no_setup_fusion = !!(c.knobs & K_NO_SETUP_FUSION);
  g_knobs.no_code_tables = !!(c.knobs & K_NO_CODE_TABLES);
  g_deny = (unsigned)c.deny;
}

int run_case(const Case &c, const Shape &s, size_t short_by = 1) {
  set_case_state(c);
  const isi_vqvae_w w = model(c);
  isi_vqvae_out out;
  memset(&out, 0, sizeof out);
  const float *x = (c.refuse == 1 || c.refuse == 3) ? nullptr : static_cast<const float *>(region("x"));
  if (c.refuse != 2 && c.refuse != 3) out.dec = static_cast<float *>(region("dec"));
  if (c.outs & 1) out.quant_t = static_cast<float *>(region("quant_t"));
  if (c.outs & 2) out.quant_b = static_cast<float *>(region("quant_b"));
  if (c.outs & 4) out.id_t = static_cast<int64_t *>(region("id_t"));
  if (c.outs & 8) out.id_b = static_cast<int64_t *>(region("id_b"));
  if (c.outs & 16) out.scalars = static_cast<float *>(region("scalars"));
  size_t bytes = isi::vqvae_workspace_bytes(&w, s.B, s.H, s.W);
  // (a refused size query has left its message)
  g_trace = "shape " + std::to_string(s.B) + "x" + std::to_string(s.H) + "x" + std::to_string(s.W) + ": workspace_bytes=" +
            std::to_string(bytes) + " pair_activations=" + std::to_string(isi::vqvae_pair_activations(&w)) + "\n";
  if (c.refuse == 6 && bytes) bytes -= short_by;
  const int rc = isi::vqvae_run(&w, c.mode, x, s.B, s.H, s.W, &out, region("ws"), bytes, nullptr);
  // the size query rounds up to 256 bytes: "one byte short" is one byte below the smallest size that is accepted
  if (c.refuse == 6 && rc == ISI_OK && short_by < 256) return run_case(c, s, short_by + 1);
  g_trace += "return " + std::to_string(rc) + "\n";
  return rc;
}

uint64_t fnv1a64(const std::string &s) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (unsigned char ch : s) { h ^= ch; h *= 0x100000001b3ull; }
  return h;
}

// ---------------------------------------------------------------- the cases
std::vector<Case> g_cases;
std::set<std::string> g_seen;
void add(const Case &c) {
  if (g_seen.insert(case_id(c)).second) g_cases.push_back(c);
}

// One axis varies while the others stay at their defaults (Case's initialisers: the default model, forward, every
// output taken), plus the combinations the GPU tests exercise: pairs x fusion x tables x mode.
void enumerate() {
  const int n_geo = sizeof kGeos / sizeof kGeos[0], n_var = sizeof kVariants / sizeof kVariants[0];
  // every geometry and variant (in_channel 1 and 3: as they are), every mode
  for (int g = 0; g < n_geo; ++g)
    for (int v = 0; v < (g == 1 || g == 2 ? 1 : n_var); ++v)
      for (int m = 1; m <= 3; ++m) { Case c; c.geo = g; c.var = v; c.mode = m; add(c); }
  // the per-model settings, on a pair-eligible and on an fp32 geometry
  for (int g : {0, 3})
    for (int m = 1; m <= 3; ++m) {
      for (int p = 0; p <= 4; ++p) { Case c; c.geo = g; c.mode = m; c.prec = p; add(c); }
      for (int w16 = 0; w16 <= 2; ++w16) { Case c; c.geo = g; c.mode = m; c.w16 = w16; add(c); }
      for (int q = 0; q <= 1; ++q) { Case c; c.geo = g; c.mode = m; c.noq = q; add(c); }
      for (int t = 0; t <= 1; ++t) { Case c; c.geo = g; c.mode = m; c.tab = t; add(c); }
    }
  // which outputs the caller takes: all, none, all but one, one alone (a decode without quant_t or quant_b is
  // refused); fused / two-launch / fp32
  for (int bit = -1; bit < 5; ++bit)
    for (int o : {bit < 0 ? 31 : 31 ^ (1 << bit), bit < 0 ? 0 : 1 << bit})
      for (int m = 1; m <= 3; ++m)
        for (int k : {0, (int)K_NO_VQ_FUSION, (int)K_NO_PAIRS}) { Case c; c.outs = o; c.mode = m; c.knobs = k; c.shapes = 1; add(c); }
  // every knob alone and all together
  for (int k : {0, 1, 2, 4, 8, 16, 31})
    for (int m = 1; m <= 3; ++m) {
      for (int w16 = 1; w16 <= 2; ++w16) { Case c; c.w16 = w16; c.knobs = k; c.mode = m; add(c); }
      Case c; c.geo = 3; c.knobs = k; c.mode = m; add(c);
    }
  // every predicate denied alone (convT_small_pair_ok is only asked where the decoder tail is not fused: with it denied too)
  for (int bit = 0; bit <= 9; ++bit)
    for (int m = 1; m <= 3; ++m) { Case c; c.mode = m; c.deny = bit < 9 ? 1 << bit : D_TAIL | D_CONVT_SMALL_PAIR; add(c); }
  // pairs x fusion x tables x mode
  for (int k = 0; k < 32; ++k)
    if (!(k & (K_NO_CONV_FIRST | K_NO_SETUP_FUSION)))
      for (int t = 0; t <= 1; ++t)
        for (int m = 1; m <= 3; ++m) { Case c; c.knobs = k; c.tab = t; c.mode = m; add(c); }
  // one level fused, the other not: who finishes the statistics, with and without the caller's fp32 maps
  for (int d : {0, (int)D_VQ_FUSABLE_2SRC, (int)D_VQ_FUSABLE_1SRC})
    for (int k : {0, (int)K_NO_SETUP_FUSION})
      for (int w16 = 1; w16 <= 2; ++w16)
        for (int o : {0, 31})
          for (int m : {1, 3}) { Case c; c.deny = d; c.knobs = k; c.w16 = w16; c.outs = o; c.mode = m; add(c); }
  // refused calls
  for (int r = 1; r <= 6; ++r)
    for (int m = 1; m <= 3; ++m)
      for (int k : {0, (int)K_NO_SETUP_FUSION}) { Case c; c.refuse = r; c.mode = m; c.knobs = k; c.shapes = 1; add(c); }
  for (int g : {0, 4})
    for (int m = 1; m <= 3; ++m)
      for (int k : {0, (int)K_NO_SETUP_FUSION, (int)K_NO_PAIRS})
        for (int o : {31, 0}) { Case c; c.geo = g; c.mode = m; c.knobs = k; c.outs = o; c.shapes = 2; add(c); }
}

}  // namespace

int main(int argc, char **argv) {
  enumerate();
  const bool dump = argc == 3 && !strcmp(argv[1], "--dump");
  if (argc != 1 && !dump) {
    fprintf(stderr, "usage: %s [--dump CASE]\n", argv[0]);
    return 2;
  }
  if (!dump)
    for (size_t i = 0; i < sizeof kDenyNames / sizeof kDenyNames[0]; ++i) printf("# deny %d = %s\n", 1 << i, kDenyNames[i]);
  for (const Case &c : g_cases) {
    if (dump && case_id(c) != argv[2]) continue;
    std::string all, rcs, ns;
    for (const Shape &s : kShapeSets[c.shapes]) {
      const int rc = run_case(c, s);
      all += g_trace;
      rcs += (rcs.empty() ? "" : ",") + std::to_string(rc);
      ns += (ns.empty() ? "" : ",") + std::to_string(g_launches);
    }
    if (dump) return fputs(all.c_str(), stdout), 0;
    printf("%s  %s  %s  %016llx\n", case_id(c).c_str(), rcs.c_str(), ns.c_str(), (unsigned long long)fnv1a64(all));
  }
  if (dump) fprintf(stderr, "no such case: %s\n", argv[2]);
  return dump ? 2 : 0;
}
