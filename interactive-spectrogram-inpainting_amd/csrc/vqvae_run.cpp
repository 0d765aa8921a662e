// Host-side launch sequence of the two-level VQ-VAE (no allocation, no sync:
// every kernel is enqueued on the caller's stream, scratch comes from the
// caller's workspace).  Mirrors VQVAE.encode / decode / forward of the
// reference (vqvae/vqvae.py:245-286) and the Rosinality encoder / decoder
// stacks (vqvae/encoder_decoder.py:38-227), with these fusions:
//   * every ReLU is folded into the epilogue of the producing convolution
//     (all ReLUs on this path are in-place in the reference, so the tensor a
//     consumer sees is always the rectified one -- including the residual
//     input of RosinalityResBlock, encoder_decoder.py:22-35);
//   * torch.cat (vqvae.py:270,282) is replaced by two-source convolutions;
//   * NCHW<->NHWC permutes (vqvae.py:260-262,272-274) vanish: internal
//     activations are channels-last, strides describe the API tensors.
// A call is: check_shapes, carve (the workspace), check_call -- every refusal, before the first launch --, make_route
// (which kernels, which formats: derived once), then the launches.  tests/forward_plan_tracer.cpp turns the launch
// sequence of a few thousand calls into text on the host; run it before and after an edit of this file.
#include <algorithm>

#include "isi_common.h"
#include "isi_internal.h"
#include "knobs.h"

namespace isi {

namespace {

struct Act {  // dense channels-last activation
  float *p;
  int C, H, W;
};

isi_src src_nhwc(const float *p, int C, int H, int W, int Wstride = -1) {
  if (Wstride < 0) Wstride = W;
  isi_src s;
  s.ptr = p; s.C = C; s.sc = 1; s.sw = C; s.sh = (int64_t)Wstride * C; s.sn = (int64_t)H * Wstride * C;
  return s;
}
isi_dst dst_nhwc(float *p, int C, int H, int W) {
  isi_dst d;
  d.ptr = p; d.sc = 1; d.sw = C; d.sh = (int64_t)W * C; d.sn = (int64_t)H * W * C;
  return d;
}
isi_src src_nchw(const float *p, int C, int H, int W) {
  isi_src s;
  s.ptr = p; s.C = C; s.sw = 1; s.sh = W; s.sc = (int64_t)H * W; s.sn = (int64_t)C * H * W;
  return s;
}
isi_dst dst_nchw(float *p, int C, int H, int W) {
  isi_dst d;
  d.ptr = p; d.sw = 1; d.sh = W; d.sc = (int64_t)H * W; d.sn = (int64_t)C * H * W;
  return d;
}

inline int down_dim(int x) { return (x + 2 - 4) / 2 + 1; }
inline int up_dim(int x, int n_up) { return x << n_up; }   // behind n_up transposed convolutions (k4 s2 p1)
// the scratch buffer a layer writes: the one of s0 / s1 its input is not in
inline float *other(const float *cur, float *s0, float *s1) { return cur == s0 ? s1 : s0; }
// split-f16 products with pack-time weight pieces: what every kernel that reads or writes the pair format runs on
inline bool f16_pieces(int pf) { return (pf & ISI_CONV_F16X3) && (pf & ISI_CONV_W16); }
inline int dec_t_channels(const isi_vqvae_w &w) { return w.dec_t.n_up ? w.dec_t.up[w.dec_t.n_up - 1].Cout : w.dec_t.conv3.Cout; }
// precision: 0 all fp32 | 1 decoder split-bf16 (x3) | 2 everything x3 | 3 index-feeding layers six-term
// split (x6: fp32-grade products), decoder x3 | 4 split-f16 everywhere (fp32-grade products, f16 range)
// `feeds_codes`: the encoders, quantize_conv_*, dec_t; else the final decoder and upsample
int product_flags(const isi_vqvae_w &w, bool feeds_codes) {
  if (w.precision == 4) return ISI_CONV_F16X3 | (w.w16 ? ISI_CONV_W16 : 0);
  if (feeds_codes) return w.precision == 3 ? ISI_CONV_BF16X6 : w.precision == 2 ? ISI_CONV_BF16X3 : 0;
  return w.precision >= 1 ? ISI_CONV_BF16X3 : 0;
}

struct Bump {
  char *base;
  size_t cap, off;
  bool dry;  // size query only
  void *take(size_t bytes) {
    off = round_up(off, 256);
    void *p = dry ? nullptr : base + off;
    off += bytes;
    return p;
  }
  float *floats(size_t n) { return static_cast<float *>(take(n * sizeof(float))); }
};

struct Shapes {
  int Hb, Wb, Cb;  // bottom latent grid / hidden channels
  int Ht, Wt;
  int Wq;          // cropped bottom width (adapt_quantized_durations)
  size_t max_act;  // largest intermediate activation (floats)
};

bool encoder_out_dims(const isi_encoder_w &e, int &H, int &W, int B, size_t &max_act) {
  for (int i = 0; i < e.n_down; ++i) {
    H = down_dim(H); W = down_dim(W);
    if (H <= 0 || W <= 0) return false;
    max_act = std::max(max_act, (size_t)B * H * W * e.down[i].Cout);
  }
  max_act = std::max(max_act, (size_t)B * H * W * e.conv3.Cout);
  return true;
}

void decoder_max_act(const isi_decoder_w &d, int H, int W, int B, size_t &max_act) {
  max_act = std::max(max_act, (size_t)B * H * W * d.conv3.Cout);
  for (int i = 0; i < d.n_up; ++i) {
    H *= 2; W *= 2;
    max_act = std::max(max_act, (size_t)B * H * W * d.up[i].Cout);
  }
}

bool compute_shapes(const isi_vqvae_w &w, int B, int H, int W, Shapes &s) {
  s.max_act = 0;
  int h = H, ww = W;
  if (!encoder_out_dims(w.enc_b, h, ww, B, s.max_act)) return false;
  s.Hb = h; s.Wb = ww; s.Cb = w.enc_b.conv3.Cout;
  if (!encoder_out_dims(w.enc_t, h, ww, B, s.max_act)) return false;
  s.Ht = h; s.Wt = ww;
  if (up_dim(s.Ht, w.dec_t.n_up) != s.Hb) return false;  // torch.cat would fail in the reference
  s.Wq = std::min(up_dim(s.Wt, w.dec_t.n_up), s.Wb);
  decoder_max_act(w.dec_t, s.Ht, s.Wt, B, s.max_act);
  decoder_max_act(w.dec, s.Hb, s.Wq, B, s.max_act);
  return true;
}

// ---- the pair format (isi_hip.h, ISI_CONV_*_PAIR): who reads what.  One definition per fact: the predictors
// (*_pairs_ok, pairs_eligible) and the launchers (run_encoder, run_decoder) both ask these.

// Does the residual stack behind a convolution run in the pair format (resblock_pair_f16.hip: every block reads and
// writes pairs)?  Otherwise its blocks read fp32 and only the last one writes pairs.
bool res_stack_in_pairs(bool pairs, int n_res, const isi_conv_w *res3, int B, int H, int W, int C) {
  if (!pairs || n_res == 0) return false;
  for (int i = 0; i < n_res; ++i)
    if (!resblock_pair_preferred(B, H, W, C, res3[i].Cout)) return false;
  return true;
}
// Layer i of an encoder (i = n_down: conv3) reads its input's format if it is the first, else the pipeline's.
inline bool enc_reads_pair(int i, bool in_pair, bool pairs) { return i ? pairs : in_pair; }
// What up[i] of a decoder in the pair pipeline reads: pairs for the implicit-GEMM kernels and for the pair form of the
// few-channel kernel (64 input channels, <= 2 outputs, fp32 result: the last layer of the default model); fp32 for its
// exact-fp32 form.  `final_pair`: the format of the decoder's result.
enum UpRead { UP_F32_SMALL, UP_PAIR_SMALL, UP_PAIR_IGEMM };
inline int up_cin(const isi_decoder_w &d, int i) { return i ? d.up[i - 1].Cout : d.conv3.Cout; }
UpRead up_read(const isi_decoder_w &d, int i, bool final_pair, int pf) {
  if (!convT_small_applicable(up_cin(d, i), d.up[i].Cout)) return UP_PAIR_IGEMM;
  const bool pair_form = convT_small_pair_ok(up_cin(d, i), d.up[i].Cout) && i == d.n_up - 1 && !final_pair && f16_pieces(pf);
  return pair_form ? UP_PAIR_SMALL : UP_F32_SMALL;
}

// Rosinality residual stack shared by encoder and decoder: `cur` holds the rectified input r; each block writes
// relu(r + conv1(relu(conv3(r)))).  The last block writes to `final_out` when that is non-null.
// `in_pair` / `out_pair`: the stack's input / output tensors are in the pair format (only set when every block is
// fusable, see pairs_eligible); tensors between blocks follow `in_pair` (res_stack_in_pairs).
int run_res_stack(int n_res, const isi_conv_w *res3, const isi_conv_w *res1, Act &cur, int B,
                  float *s0, float *s1, float *hid, float *final_out, int pf, bool in_pair, bool out_pair,
                  hipStream_t st) {
  for (int i = 0; i < n_res; ++i) {
    const int R = res3[i].Cout;
    float *outp = (i == n_res - 1 && final_out) ? final_out : other(cur.p, s0, s1);
    if (resblock_fusable(cur.C, R)) {
      const bool op = (i == n_res - 1) ? out_pair : in_pair;
      int rc = resblock_f32(cur.p, res3[i].w, res3[i].bias, res1[i].w, res1[i].bias, outp, B, cur.H,
                            cur.W, cur.C, R, /*relu*/ 1 | pf | (in_pair ? ISI_CONV_IN0_PAIR : 0) |
                            (op ? ISI_CONV_OUT_PAIR : 0), st);
      if (rc) return rc;
      cur.p = outp;
      continue;
    }
    isi_src in = src_nhwc(cur.p, cur.C, cur.H, cur.W);
    isi_dst dh = dst_nhwc(hid, R, cur.H, cur.W);
    int rc = conv2d_f32(&in, nullptr, res3[i].w, res3[i].bias, nullptr, &dh, B, cur.H, cur.W, R, 3,
                        3, 1, 1, /*relu*/ 1 | pf, st);
    if (rc) return rc;
    isi_src hin = src_nhwc(hid, R, cur.H, cur.W);
    isi_dst dout = dst_nhwc(outp, cur.C, cur.H, cur.W);
    rc = conv2d_f32(&hin, nullptr, res1[i].w, res1[i].bias, &in, &dout, B, cur.H, cur.W, cur.C, 1,
                    1, 1, 0, /*relu*/ 1 | pf, st);
    if (rc) return rc;
    cur.p = outp;
  }
  return ISI_OK;
}

// RosinalityEncoder (encoder_decoder.py:38-126).  `in` may be NCHW; the result lands in `final_out`.
// `in_pair`: the input is in the pair format; `pairs`: every tensor this encoder writes (including its output) is.
// `zero` / `zero_words`: int32 words the encoder's FIRST launch clears for later launches of the stream (conv2d_f32).
int run_encoder(const isi_encoder_w &e, isi_src in, int B, int H, int W, float *s0, float *s1,
                float *hid, float *final_out, int pf, bool in_pair, bool pairs, hipStream_t st,
                int32_t *zero = nullptr, int zero_words = 0) {
  Act cur{nullptr, in.C, H, W};
  isi_src cs = in;
  const int op = pairs ? ISI_CONV_OUT_PAIR : 0;
  for (int i = 0; i < e.n_down; ++i) {
    const int OH = down_dim(cur.H), OW = down_dim(cur.W);
    float *o = other(cur.p, s0, s1);
    isi_dst d = dst_nhwc(o, e.down[i].Cout, OH, OW);
    int rc = conv2d_f32(&cs, nullptr, e.down[i].w, e.down[i].bias, nullptr, &d, B, cur.H, cur.W, e.down[i].Cout, 4, 4, 2, 1,
                        1 | pf | (enc_reads_pair(i, in_pair, pairs) ? ISI_CONV_IN0_PAIR : 0) | op, st, nullptr, nullptr,
                        zero, zero_words);
    if (rc) return rc;
    zero = nullptr;
    cur = Act{o, e.down[i].Cout, OH, OW};
    cs = src_nhwc(cur.p, cur.C, cur.H, cur.W);
  }
  // the fused residual block stages its input once per slice (not once per tap): it reads and writes fp32 between
  // blocks -- decoding the skip connection from pairs cost more than the conversion saved, 64 -> 72 us per block --
  // and only the stack's last block writes pairs, for the implicit-GEMM consumers of the encoder's output
  const bool stack_pairs = res_stack_in_pairs(pairs, e.n_res, e.res3, B, cur.H, cur.W, e.conv3.Cout);
  float *o = (e.n_res == 0) ? final_out : other(cur.p, s0, s1);
  isi_dst d = dst_nhwc(o, e.conv3.Cout, cur.H, cur.W);
  int rc = conv2d_f32(&cs, nullptr, e.conv3.w, e.conv3.bias, nullptr, &d, B, cur.H, cur.W, e.conv3.Cout, 3, 3, 1, 1,
                      1 | pf | (enc_reads_pair(e.n_down, in_pair, pairs) ? ISI_CONV_IN0_PAIR : 0) |
                      ((e.n_res && !stack_pairs) ? 0 : op), st, nullptr, nullptr, zero, zero_words);
  if (rc) return rc;
  cur = Act{o, e.conv3.Cout, cur.H, cur.W};
  return run_res_stack(e.n_res, e.res3, e.res1, cur, B, s0, s1, hid, final_out, pf, stack_pairs, pairs, st);
}

// RosinalityDecoder (encoder_decoder.py:129-227).  Input = cat(in0, in1) on
// channels (in1 optional); the last transposed conv writes through `final_dst`.
// `in0_pair` / `in1_pair`: formats of the two inputs; `pairs`: internal tensors are written in the pair format
// wherever their consumer reads it (the few-channel transposed-convolution kernel reads fp32); `final_pair`: format
// of the tensor written through `final_dst`.
// `tab` (dec_t of a pair-pipeline call that carries code tables, code_tables.hip): the input is the quantised map of
// the codes `tab->ids`; conv3 is then the table sum instead of a convolution, and the same launch writes the first
// upsample layer where `tab->tu` is set.
struct CodeTableJob {
  const int64_t *ids;
  int K;
  const float *t3;                      // null: conv3 stays a convolution
  const float *tu, *bias_u;             // null tu: no upsample half
  float *out_u;
  int C_u;
};
int run_decoder(const isi_decoder_w &d, const isi_src &in0, const isi_src *in1, int B, int H, int W,
                float *s0, float *s1, float *hid, const isi_dst &final_dst, int pf, bool in0_pair, bool in1_pair,
                bool pairs, bool final_pair, hipStream_t st, const CodeTableJob *tab = nullptr) {
  Act cur{s0, d.conv3.Cout, H, W};
  auto reads_pair = [&](int i) { return i == d.n_up ? final_pair : pairs && up_read(d, i, final_pair, pf) != UP_F32_SMALL; };
  const bool stack_pairs = res_stack_in_pairs(pairs, d.n_res, d.res3, B, H, W, cur.C);
  bool cp = reads_pair(0);   // format of `cur` behind the residual stack
  const isi_dst d3 = dst_nhwc(cur.p, cur.C, H, W);
  const bool op3 = d.n_res ? stack_pairs : cp;   // fp32 into a register-staged stack
  int rc = tab && tab->t3
               ? vq_code_gather_f32(tab->ids, tab->t3, d.conv3.bias, cur.p, cur.C, op3, /*relu*/ 1, tab->tu, tab->bias_u,
                                    tab->out_u, tab->C_u, /*pair*/ 1, /*relu*/ 0, B, H, W, tab->K, st)
               : conv2d_f32(&in0, in1, d.conv3.w, d.conv3.bias, nullptr, &d3, B, H, W, cur.C, 3, 3, 1,
                            1, 1 | pf | (in0_pair ? ISI_CONV_IN0_PAIR : 0) | (in1_pair ? ISI_CONV_IN1_PAIR : 0) |
                            (op3 ? ISI_CONV_OUT_PAIR : 0), st);
  if (rc) return rc;
  rc = run_res_stack(d.n_res, d.res3, d.res1, cur, B, s0, s1, hid, nullptr, pf, stack_pairs, cp, st);
  if (rc) return rc;
  for (int i = 0; i < d.n_up; ++i) {
    const bool last = (i == d.n_up - 1);
    isi_src s = src_nhwc(cur.p, cur.C, cur.H, cur.W);
    float *o = other(cur.p, s0, s1);
    // the last two transposed convolutions as one producer / consumer pair (convT_pair_f16.hip, YP mode): the
    // [B, 2H, 2W, 64] activation between them is never written
    if (i == d.n_up - 2 && cp && !final_pair && f16_pieces(pf) && decoder_tail_ok(cur.C, d.up[i].Cout, d.up[i + 1].Cout))
      return decoder_tail_f32(cur.p, d.up[i].w, d.up[i].bias, d.up[i + 1].w, d.up[i + 1].bias, o, &final_dst, B, cur.H,
                              cur.W, cur.C, d.up[i].Cout, d.up[i + 1].Cout, st);
    isi_dst dd = last ? final_dst : dst_nhwc(o, d.up[i].Cout, 2 * cur.H, 2 * cur.W);
    const bool op = reads_pair(i + 1);
    rc = conv_transpose2d_k4s2_f32(&s, d.up[i].w, d.up[i].bias, &dd, B, cur.H, cur.W, d.up[i].Cout,
                                   (last ? 0 : 1) | pf | (cp ? ISI_CONV_IN0_PAIR : 0) | (op ? ISI_CONV_OUT_PAIR : 0), st);
    if (rc) return rc;
    cp = op;
    cur = Act{o, d.up[i].Cout, 2 * cur.H, 2 * cur.W};
  }
  return ISI_OK;
}

// Can this model run with its internal activations in the split-f16 pair format (precision 4 with pack-time weight
// pieces)?  Every launch that would READ a pair tensor must be one that accepts it: the split-f16 convolution kernel
// (conv_pair_sources_ok) or the fused residual block.  All-or-nothing: one ineligible layer keeps the whole model on
// fp32 activations (ISI_NO_PAIRS in the environment forces that, for measurements).
bool stack_fusable(int C, int n_res, const isi_conv_w *res3) {
  for (int i = 0; i < n_res; ++i)
    if (!resblock_fusable(C, res3[i].Cout)) return false;
  return true;
}
bool encoder_pairs_ok(const isi_encoder_w &e, int Cin, bool in_pair) {
  int C = Cin;
  for (int i = 0; i < e.n_down; ++i) {
    if (enc_reads_pair(i, in_pair, true) && !conv_pair_sources_ok(C, 0, e.down[i].Cout, 16)) return false;
    C = e.down[i].Cout;
  }
  if (enc_reads_pair(e.n_down, in_pair, true) && !conv_pair_sources_ok(C, 0, e.conv3.Cout, 9)) return false;
  return stack_fusable(e.conv3.Cout, e.n_res, e.res3);
}
bool decoder_pairs_ok(const isi_decoder_w &d, int C0, int C1, bool in0_pair, bool in1_pair, bool final_pair, int pf) {
  if ((in0_pair || in1_pair) && !conv_pair_sources_ok(C0, C1, d.conv3.Cout, 9)) return false;
  if (!stack_fusable(d.conv3.Cout, d.n_res, d.res3)) return false;
  for (int i = 0; i < d.n_up; ++i)   // (the few-channel kernel takes either format as it comes)
    if (up_read(d, i, final_pair, pf) == UP_PAIR_IGEMM && !conv_pair_sources_ok(up_cin(d, i), 0, d.up[i].Cout, 4)) return false;
  return d.n_up >= 1;
}
bool pairs_eligible(const isi_vqvae_w &w) {
  const bool off = knobs().no_pairs != 0;   // tests compare both paths in one process (isi_knob_set)
  if (off || w.precision != 4 || !w.w16) return false;
  // the first layer must be able to WRITE pairs: the 2-channel kernel (conv_first_f32.hip) does, the generic gather
  // kernel does not
  if (knobs().no_conv_first || w.in_channel != 2 || w.enc_b.n_down < 1 ||
      (w.enc_b.down[0].Cout != 32 && w.enc_b.down[0].Cout != 64)) return false;
  const int D = w.quantize_t.D, pf = product_flags(w, true);
  if (w.quantize_b.D != D) return false;
  if (!encoder_pairs_ok(w.enc_b, w.in_channel, false)) return false;
  if (!encoder_pairs_ok(w.enc_t, w.enc_b.conv3.Cout, true)) return false;
  if (!conv_pair_sources_ok(w.enc_t.conv3.Cout, 0, D, 1)) return false;                 // quantize_conv_t
  if (!decoder_pairs_ok(w.dec_t, D, 0, true, false, true, pf)) return false;            // reads the pair copy of quant_t
  if (up_read(w.dec_t, w.dec_t.n_up - 1, true, pf) != UP_PAIR_IGEMM) return false;      // its output is written as pairs
  if (!conv_pair_sources_ok(dec_t_channels(w), w.enc_b.conv3.Cout, D, 1)) return false; // quantize_conv_b
  for (int i = 0; i < w.n_upsample; ++i) {
    if (convT_small_applicable(w.upsample[i].Cin, w.upsample[i].Cout)) return false;
    if (!conv_pair_sources_ok(w.upsample[i].Cin, 0, w.upsample[i].Cout, 4)) return false;
  }
  if (w.no_quantize) return false;   // the pair copies of quant_t / quant_b are made behind the codebook searches
  return decoder_pairs_ok(w.dec, D, D, true, true, false, pf);
}

// ---- which kernels a call runs: derived once, read by the launch code below
struct Route {
  int pf_enc, pf_dec;    // product flags of the layers that feed the quantisers / of the final decoder and upsample
  bool pairs;            // internal activations as split-f16 pairs (isi_hip.h: ISI_CONV_*_PAIR)
  bool fuse_t, fuse_b;   // quantize_conv_{t,b} fused into its codebook search (vq_nearest.hip: z stays in registers)
  bool frag_packed;      // the 1x1 weights carry their fragment-major copy: no pre-kernel in front of a fused search
  bool fuse_zero;        // both histograms zeroed by the first encoder launch instead of a launch of their own
  bool tab3, tabU;       // dec_t.conv3 / upsample[0] as sums of pack-time table rows (code_tables.hip)
  bool q_t_pair_read;    // somebody reads the pair copy of quant_t: dec_t.conv3 or upsample[0]
};
Route make_route(const isi_vqvae_w &w, int mode) {
  const bool enc = mode & ISI_MODE_ENCODE, dec = mode & ISI_MODE_DECODE;
  const int D = w.quantize_t.D;
  Route r;
  r.pf_enc = product_flags(w, true); r.pf_dec = product_flags(w, false);
  r.pairs = pairs_eligible(w);
  // the pair pipeline only (pair8 sources, blocked weights); a level whose shape the fused kernel does not take runs
  // as two launches beside a fused one
  const bool fuse_vq = r.pairs && !w.no_quantize && !knobs().no_vq_fusion;
  r.fuse_t = fuse_vq && vq_conv1x1_fusable(w.enc_t.conv3.Cout, 0, D, w.quantize_t.K);
  r.fuse_b = fuse_vq && vq_conv1x1_fusable(dec_t_channels(w), w.enc_b.conv3.Cout, D, w.quantize_b.K);
  r.frag_packed = fuse_vq && w.w16 == 2 && enc;
  // (the workspace is the caller's and arrives with any content: zeroed per call.  ISI_NO_SETUP_FUSION: the zeroing
  // launch, for the tests' A/B)
  r.fuse_zero = r.frag_packed && !knobs().no_setup_fusion;
  // The tables serve the pair pipeline of a call that produces the top codes itself.  encode() and forward() take the
  // same route to id_b; the choice does not depend on the fusion or flush switches (ids exist on all of those paths).
  const bool tab_ok = r.pairs && !w.no_quantize && w.precision == 4 && !knobs().no_code_tables && enc && D % 4 == 0;
  r.tab3 = tab_ok && w.code_table_conv3 && w.dec_t.conv3.Cin == D && w.dec_t.conv3.Cout % 8 == 0;
  r.tabU = tab_ok && dec && w.code_table_upsample && w.n_upsample >= 1 && w.upsample[0].Cin == D && w.upsample[0].Cout % 8 == 0;
  r.q_t_pair_read = !r.tab3 || (dec && !r.tabU);
  return r;
}

// ---- the workspace
struct Buffers {
  float *s0, *s1, *hid;          // ping-pong activations, hidden tensor of an unfused residual block
  float *enc_b, *enc_t, *dec_t, *zbuf, *up, *up2;
  float *q_t, *q_b;              // the quantised maps where the caller takes none
  float *q_t_pair, *q_b_pair;    // their pair-format copies: what the pair pipeline's convolutions read
  int64_t *id_t, *id_b;
  int32_t *counts;               // [2][Kmax]: bottom, top (side by side: one launch zeroes both)
  int Kmax;
  float *sse_part, *sse_top;     // sse_top: the top level's partial sums where its finish waits for the bottom search
  float *wfrag, *scal;
  int32_t *counts_top() const { return counts + Kmax; }
};
Buffers carve(const isi_vqvae_w &w, const Shapes &sh, int B, Bump &ws) {
  const int D = w.quantize_t.D;
  const size_t top = (size_t)B * sh.Ht * sh.Wt, bottom = (size_t)B * sh.Hb * sh.Wb, cropped = (size_t)B * sh.Hb * sh.Wq;
  Buffers b;
  b.s0 = ws.floats(sh.max_act); b.s1 = ws.floats(sh.max_act);
  const int Rmax = std::max({w.enc_b.n_res ? w.enc_b.res3[0].Cout : 0, w.enc_t.n_res ? w.enc_t.res3[0].Cout : 0,
                             w.dec_t.n_res ? w.dec_t.res3[0].Cout : 0, w.dec.n_res ? w.dec.res3[0].Cout : 0, 1});
  b.hid = ws.floats(bottom * Rmax);
  b.enc_b = ws.floats(bottom * sh.Cb);
  b.enc_t = ws.floats(top * w.enc_t.conv3.Cout);
  b.dec_t = ws.floats(bottom * D);
  b.zbuf = ws.floats(bottom * D);
  b.up = ws.floats(bottom * D); b.up2 = ws.floats(bottom * D);
  b.q_t = ws.floats(top * D); b.q_b = ws.floats(cropped * D);
  b.q_t_pair = ws.floats(top * D); b.q_b_pair = ws.floats(cropped * D);
  b.id_t = static_cast<int64_t *>(ws.take(top * sizeof(int64_t)));
  b.id_b = static_cast<int64_t *>(ws.take(cropped * sizeof(int64_t)));
  b.Kmax = std::max(w.quantize_t.K, w.quantize_b.K);
  b.counts = static_cast<int32_t *>(ws.take((size_t)2 * b.Kmax * sizeof(int32_t)));
  b.sse_part = ws.floats(256); b.sse_top = ws.floats(256);
  b.wfrag = ws.floats((size_t)D * round_up((size_t)std::max(w.quantize_conv_b.Cin, w.quantize_conv_t.Cin), kBK));
  b.scal = ws.floats(8);
  return b;
}

// ---- refusals: all of them before the first launch.  check_shapes: what model and shape decide (the size query's too)
int check_shapes(const isi_vqvae_w &w, int B, int H, int W, Shapes &sh) {
  if (!compute_shapes(w, B, H, W, sh)) return invalid("vqvae: input too small or odd top/bottom grid");
  if (w.n_upsample != w.dec_t.n_up) return invalid("vqvae: upsample depth must equal dec_t depth");
  return ISI_OK;
}
int check_call(const isi_vqvae_w &w, int mode, const float *x, const isi_vqvae_out &out, const Shapes &sh, const Bump &ws) {
  if (ws.off > ws.cap) return set_last_error("vqvae: workspace too small"), ISI_E_WORKSPACE;
  if ((mode & ISI_MODE_ENCODE) && !x) return invalid("vqvae: x is null");
  if (!(mode & ISI_MODE_DECODE)) return ISI_OK;
  if (!out.dec) return invalid("vqvae: dec output is null");
  if (!(mode & ISI_MODE_ENCODE) && (!out.quant_t || !out.quant_b)) return invalid("vqvae: decode needs quant_t and quant_b");
  // (a one-column bottom grid under a top grid that up-samples to two)
  if (up_dim(sh.Ht, w.n_upsample) != sh.Hb || up_dim(sh.Wt, w.n_upsample) != sh.Wq)
    return invalid("vqvae: upsampled top grid != bottom grid");
  return ISI_OK;
}

// ---- one quantisation level: quantize_conv (1x1) over cat(a, b) and the codebook search (vqvae.py:260-263, 266-275)
struct Level {
  const isi_codebook_w &cb;
  const isi_conv_w &w1x1;          // (its packed weight is followed by the blocked pair copy, then by the fragments)
  isi_src a;
  const isi_src *b;                // optional second source
  int H, W;
  int64_t *ids;
  float *q;                        // the fp32 map: the caller's or the workspace's
  bool q_unread;                   // nobody reads it: a fused search, which writes the pair copy itself, skips it
  float *q_pair;
  int32_t *counts;
  float *sse;                      // partial sums of the squared error
  float *scalars2;                 // diff, perplexity
};
int finish_level(const Level &l, int B, hipStream_t st) {
  const int64_t N = (int64_t)B * l.H * l.W;
  return vq_finalize_f32(l.sse, vq_num_partials(N), l.counts, l.cb.K, N, l.cb.D, l.scalars2, st);
}
// `fused`: one launch, with the pair-format copy of q written alongside; `finish` = false then leaves the statistics to
// the caller (one launch finishes both levels, vq_finalize2_f32).  Not fused: 1x1 convolution, then the search, finished
// at once; UnquantizedBottleneck (bottleneck.py:107-119): the convolution's output IS q, diff = 0, perplexity = inf.
int quantize_level(const isi_vqvae_w &w, const Route &r, const Level &l, int B, bool fused, bool finish, const Buffers &bf,
                   hipStream_t st) {
  const int D = l.cb.D;
  if (fused) {
    const int Kpad = (int)round_up((size_t)l.w1x1.Cin, kBK);
    // frag_packed: the caller has zeroed both levels' histograms -- no pre-kernel in front of the search
    int rc = vq_conv1x1_nearest_f32(&l.a, l.b, l.w1x1.w + (size_t)l.w1x1.Cout * Kpad, l.w1x1.bias, l.cb.codes_kd, l.cb.e2, l.ids,
                                    l.q_unread ? nullptr : l.q, l.q_pair, l.counts, l.sse, bf.wfrag, B, l.H, l.W, D, l.cb.K, st,
                                    /*zero_counts*/ !r.frag_packed, nullptr,
                                    r.frag_packed ? l.w1x1.w + (size_t)2 * l.w1x1.Cout * Kpad : nullptr,
                                    knobs().no_setup_fusion ? nullptr : l.cb.planes);
    return (rc || !finish) ? rc : finish_level(l, B, st);
  }
  isi_dst d = dst_nhwc(w.no_quantize ? l.q : bf.zbuf, D, l.H, l.W);
  int rc = conv2d_f32(&l.a, l.b, l.w1x1.w, l.w1x1.bias, nullptr, &d, B, l.H, l.W, D, 1, 1, 1, 0,
                      r.pf_enc | (r.pairs ? ISI_CONV_IN0_PAIR | (l.b ? ISI_CONV_IN1_PAIR : 0) : 0), st);
  if (rc) return rc;
  if (w.no_quantize) return vq_unquantized_scalars(l.scalars2, st);   // (a kernel: no memset nodes)
  if ((rc = vq_zero_counts(l.counts, l.cb.K, st))) return rc;
  // With ISI_CONV_F16X3 (the split-f16 mode) the K distances are computed on the f16 matrix pipe only to pick two
  // candidates; the decision between them is taken in fp32 (vq_nearest.hip) -- the same search as the fused kernel's.
  rc = vq_nearest_f32(bf.zbuf, l.cb.codes_kd, l.cb.e2, l.ids, l.q, l.counts, l.sse, (int64_t)B * l.H * l.W, D, l.cb.K,
                      r.pf_enc & ISI_CONV_F16X3, st);
  return rc ? rc : finish_level(l, B, st);
}

struct Call {   // what the launch code of one call shares
  const isi_vqvae_w &w;
  int mode, B;
  Shapes sh;
  Route r;
  Buffers b;
  float *quant_t, *quant_b, *scal;   // the caller's tensors, or the workspace's where it takes none
  int64_t *id_t, *id_b;
  hipStream_t st;
};

// VQVAE.encode (vqvae.py:251-278)
int run_encode(const Call &c, const float *x, int H, int W, const isi_vqvae_out &out) {
  const isi_vqvae_w &w = c.w;
  const Route &r = c.r;
  const Buffers &b = c.b;
  const Shapes &sh = c.sh;
  const int D = w.quantize_t.D, B = c.B, Cd = dec_t_channels(w), Wd = up_dim(sh.Wt, w.dec_t.n_up);
  const bool decodes = c.mode & ISI_MODE_DECODE, both_fused = r.fuse_t && r.fuse_b;
  int rc = run_encoder(w.enc_b, src_nchw(x, w.in_channel, H, W), B, H, W, b.s0, b.s1, b.hid, b.enc_b, r.pf_enc, false, r.pairs,
                       c.st, r.fuse_zero ? b.counts : nullptr, 2 * b.Kmax);
  if (rc) return rc;
  rc = run_encoder(w.enc_t, src_nhwc(b.enc_b, sh.Cb, sh.Hb, sh.Wb), B, sh.Hb, sh.Wb, b.s0, b.s1, b.hid, b.enc_t, r.pf_enc,
                   r.pairs, r.pairs, c.st);
  if (rc) return rc;
  // the top level.  Fused, its statistics wait in sse_top until the bottom search is done; in two launches they go
  // through the slot both levels share
  const Level top{w.quantize_t, w.quantize_conv_t, src_nhwc(b.enc_t, w.enc_t.conv3.Cout, sh.Ht, sh.Wt), nullptr, sh.Ht, sh.Wt,
                  c.id_t, c.quant_t, !out.quant_t && decodes, b.q_t_pair, b.counts_top(), r.fuse_t ? b.sse_top : b.sse_part,
                  c.scal + 0};
  rc = quantize_level(w, r, top, B, r.fuse_t, /*finish*/ false, b, c.st);
  if (rc) return rc;
  if (!r.fuse_t && r.pairs && r.q_t_pair_read) {
    rc = pair_encode_f32(c.quant_t, b.q_t_pair, (int64_t)B * sh.Ht * sh.Wt * D, c.st);
    if (rc) return rc;
  }
  // dec_t (vqvae.py:265): [B,Ht,Wt,D] -> [B,Hb,2^n Wt,D]
  const isi_src qs = src_nhwc(r.pairs ? b.q_t_pair : c.quant_t, D, sh.Ht, sh.Wt);
  const isi_dst dd = dst_nhwc(b.dec_t, Cd, sh.Hb, Wd);
  // one gather launch right behind the top search: the conv3 items, then the upsample items (both read only id_t)
  const CodeTableJob job{c.id_t, w.quantize_t.K, r.tab3 ? w.code_table_conv3 : nullptr, r.tabU ? w.code_table_upsample : nullptr,
                         w.upsample[0].bias, b.up, w.upsample[0].Cout};
  if (r.tabU && !r.tab3) {
    rc = vq_code_gather_f32(c.id_t, nullptr, nullptr, nullptr, 0, 0, 0, job.tu, job.bias_u, job.out_u, job.C_u, 1, 0, B, sh.Ht,
                            sh.Wt, job.K, c.st);
    if (rc) return rc;
  }
  rc = run_decoder(w.dec_t, qs, nullptr, B, sh.Ht, sh.Wt, b.s0, b.s1, b.hid, dd, r.pf_enc, r.pairs, false, r.pairs, r.pairs, c.st,
                   r.tab3 ? &job : nullptr);
  if (rc) return rc;
  if (r.fuse_t && !r.fuse_b) {   // (the bottom level takes the two-launch path: finish the top level on its own)
    rc = finish_level(top, B, c.st);
    if (rc) return rc;
  }
  // the bottom level, on cat([dec_t, enc_b]) cropped to Wq (vqvae.py:266-273)
  const isi_src eb = src_nhwc(b.enc_b, sh.Cb, sh.Hb, sh.Wq, sh.Wb);
  const Level bottom{w.quantize_b, w.quantize_conv_b, src_nhwc(b.dec_t, Cd, sh.Hb, sh.Wq, Wd), &eb, sh.Hb, sh.Wq,
                     c.id_b, c.quant_b, !out.quant_b && decodes, b.q_b_pair, b.counts, b.sse_part, c.scal + 2};
  rc = quantize_level(w, r, bottom, B, r.fuse_b, /*finish*/ !both_fused, b, c.st);
  if (rc) return rc;
  if (!both_fused) return vq_scalars_sum_f32(c.scal, c.st);       // scalars[4] = diff_t + diff_b
  const int64_t N_t = (int64_t)B * sh.Ht * sh.Wt, N_b = (int64_t)B * sh.Hb * sh.Wq;
  return vq_finalize2_f32(top.sse, vq_num_partials(N_t), top.counts, w.quantize_t.K, N_t, bottom.sse, vq_num_partials(N_b),
                          bottom.counts, w.quantize_b.K, N_b, D, c.scal, c.st);
}

// VQVAE.decode (vqvae.py:280-286); `q_t` / `q_b`: the quantised maps in the pipeline's format
int run_decode(const Call &c, const float *q_t, const float *q_b, float *dec_out) {
  const isi_vqvae_w &w = c.w;
  const Shapes &sh = c.sh;
  const bool pairs = c.r.pairs;
  const int D = w.quantize_t.D;
  // upsample_top_to_bottom: plain transposed convs, no ReLU (vqvae.py:183-201,281)
  const float *cur = q_t;
  int h = sh.Ht, ww = sh.Wt;
  for (int i = 0; i < w.n_upsample; ++i, h *= 2, ww *= 2) {
    float *o = (i % 2 == 0) ? c.b.up : c.b.up2;
    if (i || !c.r.tabU) {      // (else: written by the gather launch of run_encode)
      isi_src s = src_nhwc(cur, w.upsample[i].Cin, h, ww);
      isi_dst d = dst_nhwc(o, w.upsample[i].Cout, 2 * h, 2 * ww);
      int rc = conv_transpose2d_k4s2_f32(&s, w.upsample[i].w, w.upsample[i].bias, &d, c.B, h, ww, w.upsample[i].Cout,
                                         c.r.pf_dec | (pairs ? ISI_CONV_IN0_PAIR | ISI_CONV_OUT_PAIR : 0), c.st);
      if (rc) return rc;
    }
    cur = o;
  }
  isi_src a = src_nhwc(cur, D, sh.Hb, sh.Wq);
  isi_src b = src_nhwc(q_b, D, sh.Hb, sh.Wq);
  isi_dst d = dst_nchw(dec_out, w.in_channel, up_dim(sh.Hb, w.dec.n_up), up_dim(sh.Wq, w.dec.n_up));
  return run_decoder(w.dec, a, &b, c.B, sh.Hb, sh.Wq, c.b.s0, c.b.s1, c.b.hid, d, c.r.pf_dec, pairs, pairs, pairs, false, c.st);
}

}  // namespace

int vqvae_pair_activations(const isi_vqvae_w *w) { return (w && pairs_eligible(*w)) ? 1 : 0; }

size_t vqvae_workspace_bytes(const isi_vqvae_w *w, int B, int H, int W) {
  if (!w || B <= 0 || H <= 0 || W <= 0) return 0;
  Bump ws{nullptr, 0, 0, true};
  Shapes sh;
  if (check_shapes(*w, B, H, W, sh) != ISI_OK) return 0;
  carve(*w, sh, B, ws);
  return round_up(ws.off, 256);
}

int vqvae_run(const isi_vqvae_w *w, int mode, const float *x, int B, int H, int W,
              const isi_vqvae_out *out, void *workspace, size_t workspace_bytes,
              hipStream_t stream) {
  if (!w || !out || !workspace) return invalid("vqvae_run: null pointer");
  if (mode < 1 || mode > 3) return invalid("vqvae_run: bad mode");
  if (B <= 0 || H <= 0 || W <= 0) return invalid("vqvae_run: bad shape");
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return invalid("vqvae_run: workspace must be 256-byte aligned");
  Bump ws{static_cast<char *>(workspace), workspace_bytes, 0, false};
  Shapes sh;
  if (int rc = check_shapes(*w, B, H, W, sh)) return rc;
  const Buffers b = carve(*w, sh, B, ws);
  if (int rc = check_call(*w, mode, x, *out, sh, ws)) return rc;

  const Route r = make_route(*w, mode);
  const Call c{*w, mode, B, sh, r, b, out->quant_t ? out->quant_t : b.q_t, out->quant_b ? out->quant_b : b.q_b,
               out->scalars ? out->scalars : b.scal, out->id_t ? out->id_t : b.id_t, out->id_b ? out->id_b : b.id_b, stream};
  const int64_t D = w->quantize_t.D;
  const bool enc = mode & ISI_MODE_ENCODE, dec = mode & ISI_MODE_DECODE;
  if (r.frag_packed && !r.fuse_zero)
    if (int rc = vq_zero_counts(b.counts, 2 * b.Kmax, stream)) return rc;
  if (enc)
    if (int rc = run_encode(c, x, H, W, *out)) return rc;
  if (!dec) return ISI_OK;
  if (r.pairs) {
    // forward: quant_t was encoded behind its search (dec_t reads it), quant_b too where its search was fused;
    // decode: both maps arrive as fp32
    if (!enc)
      if (int rc = pair_encode_f32(c.quant_t, b.q_t_pair, (int64_t)B * sh.Ht * sh.Wt * D, stream)) return rc;
    if (!(enc && r.fuse_b))
      if (int rc = pair_encode_f32(c.quant_b, b.q_b_pair, (int64_t)B * sh.Hb * sh.Wq * D, stream)) return rc;
  }
  return run_decode(c, r.pairs ? b.q_t_pair : c.quant_t, r.pairs ? b.q_b_pair : c.quant_b, out->dec);
}

}  // namespace isi
