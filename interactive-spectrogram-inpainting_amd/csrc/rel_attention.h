// What the relative-attention translation units share: the kernel-side arguments of the forward kernels
// (rel_attention_f32.hip: exact fp32 and the one-row tail kernel; rel_attention_fwd2.hip: the 64-key-tile kernels;
// rel_attention_fwd3.hip: the plane-staged kernel) and the launchers the dispatcher hands over to; the host checks and
// the argument fill common to the forward and the backward entry point (rel_attention_bwd_f32.hip); the constants and
// the 16-bit operand trait of the two 16-bit forward files.
#pragma once
#include <hip/hip_runtime.h>

#include "device_prims.h"
#include "isi_common.h"
#include "split_bf16.h"

namespace isi {

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

// rel_attention_fwd2.hip: any Cq, Ck >= 1, head_dim 16 / 32 / 64.  precision: 1 three-term split-bf16, 2 single-term bf16,
// 3 single-term f16.
int rel_attention_fwd2(const AttnKArgs &a, int head_dim, int precision, hipStream_t stream);
int rel_attention_fwd2_debug_stamps(long long *host, int n);

// rel_attention_fwd3.hip: one channel per event (Cq = Ck = 1), head_dim 32 / 64, precision 1 .. 3; K, V and e are split into
// 16-bit planes in `workspace` (rel_attention_fwd3_workspace_bytes, 256-byte aligned) by a pack launch in front of the kernel.
bool rel_attention_fwd3_ok(const AttnKArgs &a, int head_dim, int precision);
size_t rel_attention_fwd3_workspace_bytes(const AttnKArgs &a, int head_dim, int precision);
int rel_attention_fwd3(const AttnKArgs &a, int head_dim, int precision, void *workspace, size_t workspace_bytes, hipStream_t stream);
int rel_attention_fwd3_debug_stamps(long long *host, int n);

// ---- host: what rel_attention_f32() and rel_attention_bwd_f32() check and fill alike

constexpr int BAND = 160;      // rows of e a 128 x 32 tile can touch (>= 127/Cq + 31/Ck + 1, and the same with Cq, Ck swapped)

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

// ---- device: constants of all the attention kernels; LD and the operand trait Prec are the 16-bit forward kernels'
// (rel_attention_fwd2.hip, rel_attention_fwd3.hip)

typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

constexpr unsigned OOB = 0xFFFFFFF0u;   // a buffer offset beyond every descriptor: the load returns zeros
constexpr float NEG = -1e30f;
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
constexpr int QB = 128;    // queries (in the backward's key-stationary kernels: keys) per workgroup
constexpr int LD = 68;     // floats per query row of the skew buffer (64 band rows + 4)

// the 16-bit operand type of a mode: conversions (round to nearest even) and the matrix instruction
template <bool F16> struct Prec;
template <> struct Prec<false> {
  static __device__ __forceinline__ unsigned pack2(const float a, const float b) {
    const f32x2_t v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
  }
  static __device__ __forceinline__ void split2(const float a, const float b, unsigned &hi, unsigned &lo) { isi::split2(a, b, hi, lo); }
  static __device__ __forceinline__ f32x16 mfma(const s16x8_t a, const s16x8_t b, const f32x16 c) { return ISI_MFB(a, b, c); }
};
template <> struct Prec<true> {
  static __device__ __forceinline__ unsigned pack2(const float a, const float b) {
    const f32x2_t v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2_t));
  }
  static __device__ __forceinline__ void split2(const float a, const float b, unsigned &hi, unsigned &lo) {
    const f32x2_t v = {a, b};
    const f16x2_t h = __builtin_convertvector(v, f16x2_t);
    const f16x2_t l = __builtin_convertvector(v - __builtin_convertvector(h, f32x2_t), f16x2_t);
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, l);
  }
  static __device__ __forceinline__ f32x16 mfma(const s16x8_t a, const s16x8_t b, const f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
  }
};

}  // namespace isi
