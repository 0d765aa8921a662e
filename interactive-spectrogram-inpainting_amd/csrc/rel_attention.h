// What the training-side relative attention's host plan (rel_attention_run.cpp) and its kernels share: the kernels' argument
// blocks, the constants the plan sizes things by, the host checks and the argument fill common to the forward and the
// backward entry point, and one launcher per kernel family.  The plan never names a kernel; a launcher picks the template
// instantiation from its arguments and owns that kernel's one-time set-up.  The kernels:
//   rel_attention_f32.hip      forward: exact fp32 and the one-row tail kernel
//   rel_attention_fwd2.hip     forward: the 64-key-tile 16-bit kernels
//   rel_attention_fwd3.hip     forward: the plane-staged 16-bit kernel and its pack launch
//   rel_attention_bwd_f32.hip  backward: every kernel of it
// This header compiles as plain C++ with the HIP headers; what only device code reads is rel_attention_dev.h.
#pragma once
#include <hip/hip_runtime.h>

#include "isi_common.h"

namespace isi {

// The argument block of the forward kernels.  A KERNEL ARGUMENT: its layout is part of the device code.
struct AttnKArgs {
  const float *q, *k, *v, *e, *mask;
  float *out, *lse;
  unsigned q_bytes, k_bytes, v_bytes, e_bytes;
  int Sq, Sk, H, B;
  int nblk;       // query blocks the 16-bit kernels run (all, or only the full ones: the tail rows go to the one-row kernel)
  int q_ss, q_sb, q_sh, k_ss, k_sb, k_sh, v_ss, v_sb, v_sh, o_ss, o_sb, o_sh;  // element strides
  int Cq, Ck, Ek, R;
  int mask_mode;  // 0 none, 1 causal (j <= i), 2 anti-causal (j >= i)
  float scale;
  int split;      // 16-bit precision class of the call: 0 exact fp32, 1 three-term split-bf16 products, 2 single-term
  float *logits;  // optional [B,H,Sq,ldl]: base-2 logits of the allowed pairs, kept for the backward (rel_attention_fwd2.hip)
  int ldl;
};
static_assert(sizeof(AttnKArgs) == 184, "AttnKArgs is a kernel argument block: its layout must not change");

// The argument block of the backward kernels.  A kernel argument like AttnKArgs.
struct AttnBwdKArgs {
  const float *q, *k, *v, *e, *mask, *dout, *out, *lse;
  float *dsum;            // [B,H,Sq]
  float *dq, *dk, *dv;
  float *g;               // [H][Sq][B][Rp]: rows query-major, so that the rows of a GEMM tile share their band of columns
  unsigned q_bytes, k_bytes, v_bytes, e_bytes, o_bytes;
  int Sq, Sk, H, B;
  int nqb, nkb;           // stationary query / key blocks the split kernels run (all, or only the full ones)
  int q_ss, q_sb, q_sh, k_ss, k_sb, k_sh, v_ss, v_sb, v_sh, o_ss, o_sb, o_sh;  // element strides
  int Cq, Ck, Ek, R, Rp;
  int rho_lo;             // G column c holds table row rho_lo + c (causal modes only touch half of the table)
  int g_band_only;        // G is zeroed only around its band: EVERY (query, key) pair the mask allows is stored (zeros too)
  int mask_mode;
  float scale;
  const float *logits;    // optional [B,H,Sq,ldl]: the forward's base-2 logits of the allowed pairs (isi_attn_args.logits):
  int ldl;                // the split kernels read them instead of forming Q K^T and the skewed band product again
  int g_from_kv;          // (kept logits, Cq = Ck = 1, band-only G) the KEY-stationary kernel stores dS into G -- lanes run
                          // along keys: 128-byte runs of a query's row -- and the query-stationary kernel only reads it back
                          // for dQ += dS K: no second exp / dO V^T / dS pass, no V tiles, no scatter
};
static_assert(sizeof(AttnBwdKArgs) == 248, "AttnBwdKArgs is a kernel argument block: its layout must not change");

constexpr int QB = 128;        // queries (in the backward's key-stationary kernels: keys) per workgroup
constexpr int BAND = 160;      // rows of e a 128 x 32 tile can touch (>= 127/Cq + 31/Ck + 1, and the same with Cq, Ck swapped)

// Where the plane-staged forward keeps its 16-bit operand planes in the caller's workspace (rel_attention_run.cpp computes
// it, the launchers of rel_attention_fwd3.hip read it): plane element counts and byte offsets
struct PlaneLayout { int Skp, npl; size_t kv_plane, e_plane, k_off, v_off, e_off, total; };

// ---- launchers.  head_dim is 16, 32 or 64 (the plane-staged kernel: 32 or 64); anything else is refused
// rel_attention_f32.hip: exact fp32, all query blocks
int launch_attn_fwd_exact(const AttnKArgs &a, int head_dim, hipStream_t st);
// the query rows [row0, row0 + rows) in exact fp32, one workgroup per (batch, head) and row
int launch_attn_fwd_tail_rows(const AttnKArgs &a, int head_dim, int row0, int rows, hipStream_t st);
// rel_attention_fwd2.hip: any Cq, Ck >= 1.  precision: 1 three-term split-bf16, 2 single-term bf16, 3 single-term f16;
// nW persistent workgroups per (batch, head) pair
int launch_attn_fwd2(const AttnKArgs &a, int head_dim, int precision, int nW, hipStream_t st);
int rel_attention_fwd2_debug_stamps(long long *host, int n);
// rel_attention_fwd3.hip: one channel per event (Cq = Ck = 1), head_dim 32 / 64, precision 1 .. 3.  TWO launches: K, V and
// e are split into 16-bit planes in `workspace` (L.total bytes, 256-byte aligned) by a pack launch, then the kernel
int launch_attn_fwd3(const AttnKArgs &a, int head_dim, int precision, const PlaneLayout &L, void *workspace, int nW,
                     hipStream_t st);
int rel_attention_fwd3_debug_stamps(long long *host, int n);
// rel_attention_bwd_f32.hip.  D[b,h,i] = dO_i . O_i into a.dsum
int launch_attn_dsum(const AttnBwdKArgs &a, int head_dim, hipStream_t st);
// G zeroed: all n4 float4 of it, or, on `rows` = (head, query, batch) rows of Rp columns, the margins of each row's band
// [lo_slope i + lo_base, hi_slope i + hi_base]
int launch_attn_zero_g(float *g, size_t n4, hipStream_t st);
int launch_attn_zero_g_margins(float *g, long rows, int Sq, int B, int Rp, int lo_slope, int lo_base, int hi_slope, int hi_base,
                               hipStream_t st);
// the split-bf16 pair.  one: single-term products; saved: the kept logits a.logits are read; which: 1 = the key-stationary
// kernel (dK, dV), 2 = the query-stationary one (dQ, G), 3 = both, in that order
int launch_attn_bwd_split(const AttnBwdKArgs &a, int head_dim, bool one, bool saved, int which, hipStream_t st);
// the last tail_q query rows and tail_k keys in exact fp32, one launch for both
int launch_attn_bwd_tails(const AttnBwdKArgs &a, int head_dim, int tail_q, int tail_k, hipStream_t st);
// the exact-fp32 pair: key-stationary (dK, dV), then query-stationary (dQ, G)
int launch_attn_bwd_exact(const AttnBwdKArgs &a, int head_dim, hipStream_t st);
// packed GEMM operand of every head's table rows [lo, lo + n), transposed and zero padded to Kpad; and back:
// d_rel[h][r][d] = dw[h][r - lo][d] on those rows, 0 elsewhere (dw rows padded to Rp, columns to Kp)
int launch_pack_rel_T(const float *e, float *out, int H, int R, int HD, int Kpad, int lo, int n, hipStream_t st);
int launch_unpack_drel(const float *dw, float *out, int H, int R, int HD, int Rp, int Kp, int lo, int n, hipStream_t st);

// ---- host: what rel_attention_f32() and rel_attention_bwd_f32() check and fill alike

// elements from a [S, B, H, hd] tensor's first to one past its last
inline int64_t span(int64_t S, int64_t ss, int64_t B, int64_t sb, int64_t H, int64_t sh, int64_t hd) {
  return (S - 1) * ss + (B - 1) * sb + (H - 1) * sh + hd;
}
struct AttnSpans { int64_t q, k, v, o; };

// The refusals of the part of isi_attn_args both directions read; `who` ("rel_attention", "rel_attention_bwd") opens the
// message, `more_ptrs` is the OR of the caller's further pointers that have to be 16-byte aligned.  ISI_OK: `sp` is set.
inline int attn_check_common(const isi_attn_args *g, const char *who, uintptr_t more_ptrs, AttnSpans *sp) {
  char msg[160];
  auto refuse = [&](int code, const char *what) {
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    set_last_error(msg);
    return code;
  };
  if (!g || !g->q || !g->k || !g->v || !g->out) return refuse(ISI_E_INVALID, "null pointer");
  if (g->Sq <= 0 || g->Sk <= 0 || g->B <= 0 || g->H <= 0) return refuse(ISI_E_INVALID, "bad shape");
  if (g->Cq <= 0 || g->Ck <= 0 || g->Ek <= 0) return refuse(ISI_E_INVALID, "bad event layout");
  if (g->mask_mode < 0 || g->mask_mode > 2) return refuse(ISI_E_INVALID, "bad mask mode");
  if (127 / g->Cq + 31 / g->Ck + 1 > BAND) return refuse(ISI_E_UNSUPPORTED, "band too wide");
  const int64_t lim = (int64_t)1 << 30;
  sp->q = span(g->Sq, g->q_ss, g->B, g->q_sb, g->H, g->q_sh, g->head_dim);
  sp->k = span(g->Sk, g->k_ss, g->B, g->k_sb, g->H, g->k_sh, g->head_dim);
  sp->v = span(g->Sk, g->v_ss, g->B, g->v_sb, g->H, g->v_sh, g->head_dim);
  sp->o = span(g->Sq, g->o_ss, g->B, g->o_sb, g->H, g->o_sh, g->head_dim);
  if (sp->q > lim || sp->k > lim || sp->v > lim || sp->o > lim) return refuse(ISI_E_UNSUPPORTED, "tensor spans 4 GiB or more");
  const int64_t all = g->q_ss | g->q_sb | g->q_sh | g->k_ss | g->k_sb | g->k_sh | g->v_ss | g->v_sb | g->v_sh |
                      g->o_ss | g->o_sb | g->o_sh;
  const uintptr_t ptrs = reinterpret_cast<uintptr_t>(g->q) | reinterpret_cast<uintptr_t>(g->k) |
                         reinterpret_cast<uintptr_t>(g->v) | reinterpret_cast<uintptr_t>(g->out) |
                         reinterpret_cast<uintptr_t>(g->rel_embeddings) | more_ptrs;
  if ((all & 3) || (ptrs & 15))
    return refuse(ISI_E_INVALID, "strides must be multiples of 4 floats and pointers 16-byte aligned");
  return ISI_OK;
}

// the fields AttnKArgs and AttnBwdKArgs have in common, from a call that passed attn_check_common
template <class KArgs>
inline void attn_fill_common(KArgs &a, const isi_attn_args *g, const AttnSpans &sp) {
  a.q = g->q; a.k = g->k; a.v = g->v; a.e = g->rel_embeddings; a.mask = g->dense_mask; a.out = g->out; a.lse = g->lse;
  a.q_bytes = (unsigned)(sp.q * 4); a.k_bytes = (unsigned)(sp.k * 4); a.v_bytes = (unsigned)(sp.v * 4);
  a.R = g->rel_rows;
  a.e_bytes = (unsigned)((size_t)g->H * g->rel_rows * g->head_dim * 4);
  a.Sq = g->Sq; a.Sk = g->Sk; a.H = g->H; a.B = g->B;
  a.q_ss = (int)g->q_ss; a.q_sb = (int)g->q_sb; a.q_sh = (int)g->q_sh;
  a.k_ss = (int)g->k_ss; a.k_sb = (int)g->k_sb; a.k_sh = (int)g->k_sh;
  a.v_ss = (int)g->v_ss; a.v_sb = (int)g->v_sb; a.v_sh = (int)g->v_sh;
  a.o_ss = (int)g->o_ss; a.o_sb = (int)g->o_sb; a.o_sh = (int)g->o_sh;
  a.Cq = g->Cq; a.Ck = g->Ck; a.Ek = g->Ek;
  a.mask_mode = g->mask_mode; a.scale = g->scale;
}

}  // namespace isi
