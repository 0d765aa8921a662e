// The host plan of the training-side relative attention (isi_rel_attention_f32, isi_rel_attention_bwd_f32 and their size
// queries): pure host code, no kernel.  The kernels and the launchers that pick their instantiations are
// rel_attention_f32.hip, rel_attention_fwd2.hip, rel_attention_fwd3.hip and rel_attention_bwd_f32.hip (rel_attention.h);
// the two products over G run on gemm_split_f32.hip / conv_igemm_f32.hip and conv_wgrad_f32.hip.
// tests/attention_plan_tracer.cpp links this file against recording stubs of all of them and pins every launch of every
// route (tests/attention_plan_trace.txt).
//
// Forward: one kernel -- exact fp32, the 64-key-tile 16-bit kernel, or, with a workspace, a pack launch and the
// plane-staged 16-bit kernel -- and behind a 16-bit kernel the one-row kernel for one or two rows beyond the last full
// block (attention_tail_rows).
// Backward:  D = rowsum(dO o O);  G zeroed (all of it, or the margins of its band);  the attention kernels (exact fp32
// pair | split pair | key-stationary, tails, query-stationary when the key-stationary kernel stores dS for the other) with
// the tail kernel;  then, with a table,  dQ += G E  (banded GEMM, or the batched 1x1 convolution) and  dE = G^T Q  (the
// batched weight-gradient GEMM) between a pack and an unpack launch of the table rows G covers.
//
// The file in order: the forward (layout of the planes, route, checks, entry points); the backward (the table rows and
// the band of G, the workspace, the route, the checks, one function per phase, entry points).
#include <algorithm>
#include <cstring>

#include "isi_common.h"
#include "isi_internal.h"
#include "knobs.h"
#include "rel_attention.h"

namespace isi {

// Rows (keys, in the backward's key-stationary kernel) beyond the last full 128-row block that are NOT given a block of
// their own: 1 or 2 of them behind at least two full blocks, unmasked attention only (under a causal mask the ragged
// block is made the cheapest one instead, see the kernels: measured better than the extra launch).
// One or two rows beyond the last full block (the prior's sequences are 1024 codes + a start row) would be a block of
// their own that runs as long as a full one: 576 instead of 512 workgroups on 256 CUs -- a third round for one row per
// (batch, head) (forward 244 vs 165 us, backward 1252 vs 1007 us, dense, B 8 x H 8 x 1025 x 1025).  They go through the
// one-row kernels instead (exact fp32, one workgroup per (batch, head) and row).
int attention_tail_rows(int S, int mask_mode, bool dense_mask) {
  const int tail = S % QB;
  return (tail >= 1 && tail <= 2 && S >= 2 * QB && !dense_mask && mask_mode == 0) ? tail : 0;
}

namespace {

bool one_channel_per_event(const isi_attn_args *g) { return g->Cq == 1 && g->Ck == 1; }
int blocks(int S, int tail) { return tail ? S / QB : (S + QB - 1) / QB; }     // stationary blocks of S rows, `tail` of them left out

// ================================================================ forward

// The 16-bit planes of K, V and the table in the caller's workspace (rel_attention_fwd3.hip)
PlaneLayout plane_layout(const isi_attn_args *g) {
  PlaneLayout L;
  L.Skp = (g->Sk + 31) & ~31;
  L.npl = g->precision == 1 ? 2 : 1;      // hi and lo for three-term products
  L.kv_plane = (size_t)g->H * g->B * L.Skp * g->head_dim;
  L.e_plane = g->rel_embeddings ? (size_t)g->H * g->rel_rows * g->head_dim : 0;
  L.k_off = 0;
  L.v_off = round_up(L.k_off + L.npl * L.kv_plane * 2, 256);
  L.e_off = round_up(L.v_off + L.npl * L.kv_plane * 2, 256);
  L.total = round_up(L.e_off + L.npl * L.e_plane * 2, 256);
  return L;
}
// what the plane-staged kernel takes
bool planes_ok(const isi_attn_args *g) {
  if (!one_channel_per_event(g) || !(g->head_dim == 64 || g->head_dim == 32) || g->precision < 1 || g->precision > 3 ||
      !g->rel_embeddings)
    return false;
  const PlaneLayout L = plane_layout(g);
  // one buffer descriptor per operand over all its planes (32-bit offsets)
  return L.npl * L.kv_plane * 2 < ((size_t)1 << 31) && L.npl * L.e_plane * 2 < ((size_t)1 << 31);
}

// The one routing decision of the forward.  Exact fp32 has its own kernel; the 16-bit precisions run the 64-key-tile
// kernels (rel_attention_fwd2.hip) or, with a workspace for its operand planes, the plane-staged kernel
// (rel_attention_fwd3.hip) where that one takes the shape.
enum class AttnFwd { F32, Tiles64, Planes };
enum class AttnWs { None, Given, Query };   // Query: no workspace yet, the caller asks whether to bring one
AttnFwd attn_fwd_route(const isi_attn_args *g, AttnWs ws) {
  if (g->precision == 0) return AttnFwd::F32;
  // the plane-staged kernel pays a pack launch (10-13 us at B 8 x H 8 x S 1025): measured, it wins with three-term products
  // (causal 91 vs 96 us, unmasked 127 vs 141) and loses 3-4 us with single-term ones -- those ask for no workspace unless
  // ISI_ATTN_FWD3_ALL is set (a caller that hands one over anyway gets the plane-staged kernel)
  if (ws == AttnWs::Query && g->precision != 1 && !knobs().attn_fwd3_all) return AttnFwd::Tiles64;
  if (ws == AttnWs::None || knobs().attn_no_fwd3 || !planes_ok(g)) return AttnFwd::Tiles64;
  return AttnFwd::Planes;
}

// Persistent workgroups per (batch, head) pair of the two 16-bit kernels: one per block while the chip is not full;
// otherwise as many as give every CU one workgroup, at most one per two blocks under a mask (a heavy and a light block each)
int persistent_workgroups(const AttnKArgs &a) {
  const int pairs = a.H * a.B, cus = current_device_cu_count();
  if ((int64_t)pairs * a.nblk <= cus) return a.nblk;
  return std::max(1, std::min(a.mask_mode ? (a.nblk + 1) / 2 : a.nblk, cus / pairs));
}

// every refusal of the forward but the workspace's, which only the plane-staged route reads
int check_fwd_call(const isi_attn_args *g, AttnSpans *sp) {
  if (const int rc = attn_check_common(g, "rel_attention", 0, sp)) return rc;
  if (g->precision < 0 || g->precision > 3) return invalid("rel_attention: precision must be 0 .. 3");
  if (g->logits) {
    if (g->logits_ld < ((g->Sk + 31) & ~31) || (g->logits_ld & 3) || (reinterpret_cast<uintptr_t>(g->logits) & 15))
      return invalid("rel_attention: logits_ld must be a multiple of 4, at least Sk rounded up to 32; logits 16-byte aligned");
    if ((int64_t)g->B * g->H * g->Sq * g->logits_ld > ((int64_t)1 << 40)) return unsupported("rel_attention: logits buffer too large");
    if (g->precision == 0)
      return unsupported("rel_attention: the logits are stored by the 64-key-tile kernels only (precision >= 1)");
  }
  if (g->rel_embeddings && g->rel_rows <= 0) return invalid("rel_attention: rel_rows must be positive");
  if (g->head_dim != 16 && g->head_dim != 32 && g->head_dim != 64)
    return unsupported("rel_attention: head_dim must be 16, 32 or 64");
  return ISI_OK;
}

}  // namespace

int rel_attention_f32(const isi_attn_args *g, hipStream_t stream) {
  AttnSpans sp;
  if (const int rc = check_fwd_call(g, &sp)) return rc;
  const AttnFwd route = attn_fwd_route(g, g->workspace ? AttnWs::Given : AttnWs::None);
  const int HD = g->head_dim;
  // the 16-bit kernels leave the tail rows to the one-row kernel
  const int tail = route == AttnFwd::F32 ? 0 : attention_tail_rows(g->Sq, g->mask_mode, g->dense_mask != nullptr);
  AttnKArgs a;
  attn_fill_common(a, g, sp);
  // 0 fp32 pipe | 1 three-term split-bf16 | 2 single-term bf16 | 3 single-term f16
  a.split = g->precision == 1 ? 1 : g->precision >= 2 ? 2 : 0;
  a.logits = g->logits; a.ldl = (int)g->logits_ld;
  a.nblk = blocks(g->Sq, tail);
  int rc;
  switch (route) {
    case AttnFwd::Planes: {
      const PlaneLayout L = plane_layout(g);
      if (g->workspace_bytes < L.total || (reinterpret_cast<uintptr_t>(g->workspace) & 255))
        return invalid("rel_attention: workspace too small or not 256-byte aligned (isi_rel_attention_workspace_bytes)");
      rc = launch_attn_fwd3(a, HD, g->precision, L, g->workspace, persistent_workgroups(a), stream);      // (pack + kernel)
      break;
    }
    case AttnFwd::Tiles64: rc = launch_attn_fwd2(a, HD, g->precision, persistent_workgroups(a), stream); break;
    default: rc = launch_attn_fwd_exact(a, HD, stream); break;
  }
  if (rc || !tail) return rc;
  return launch_attn_fwd_tail_rows(a, HD, g->Sq - tail, tail, stream);
}

// bytes of isi_attn_args.workspace that let the forward run its plane-staged kernel (0: that kernel does not take the call)
size_t rel_attention_workspace_bytes(const isi_attn_args *g) {
  if (!g || g->Sq <= 0 || g->Sk <= 0 || g->B <= 0 || g->H <= 0 || g->precision < 1 || g->precision > 3) return 0;
  return attn_fwd_route(g, AttnWs::Query) == AttnFwd::Planes ? plane_layout(g).total : 0;
}

// ================================================================ backward
namespace {

// Table rows a (query, key) pair can select: causal / anti-causal self-attention (Cq == Ck) only ever
// reaches the upper / lower half of the table, which halves G and the two GEMMs over it.  No table: no rows.
struct TableRows { int lo, n; };
TableRows rho_range(const isi_attn_args *g) {
  const int R = g->rel_rows;
  if (!g->rel_embeddings || R <= 0) return {0, 0};
  TableRows t{0, R};
  if (g->Cq == g->Ck && !g->dense_mask) {
    if (g->mask_mode == 1) { t.lo = std::min(std::max(g->Ek - 1, 0), R - 1); t.n = R - t.lo; }   // j <= i: rho >= Ek - 1
    if (g->mask_mode == 2) { t.n = std::max(1, std::min(R, g->Ek)); }                             // j >= i: rho <= Ek - 1
  }
  return t;
}

// The band of G (one channel per event on both sides; columns = table row - rho.lo): query i is non-zero only in
// [lo_slope i + lo_base, hi_slope i + hi_base] -- [i + bot, i + top] unmasked, [top, i + top] causal, [i + bot, top]
// anti-causal.  The ONE definition: the margins kernel zeroes around it, and both products over G skip what lies
// outside it, each told in its own terms (gemm_window, wgrad_band).
struct GBand { int lo_slope, lo_base, hi_slope, hi_base; };
GBand g_band(const isi_attn_args *g, const TableRows &rho) {
  const int top = g->Ek - 1 - rho.lo, bot = g->Ek - g->Sk - rho.lo;
  return {g->mask_mode == 1 ? 0 : 1, g->mask_mode == 1 ? top : bot, g->mask_mode == 2 ? 0 : 1, top};
}
// dQ += G E: rows of G are (query, batch) -- a unit of B rows shares a band of K chunks, the kernel skips the others (a
// 128-row tile holds 128 / B queries, its band is about half of the table)
void gemm_window(GemmExtra *gx, const GBand &band, int B) {
  gx->win_rpu = B;
  gx->lo_slope = band.lo_slope; gx->lo_base = band.lo_base; gx->hi_slope = band.hi_slope; gx->hi_base = band.hi_base;
}
// dE = G^T Q: the band read along the other axis -- column c is non-zero on the queries i with
// lo_slope i + lo_base <= c <= hi_slope i + hi_base: from c - hi_base on where the upper edge moves with the query (from
// the first query where it does not: anti-causal), up to c - lo_base where the lower edge moves (to the last query where
// it does not: causal).  required: G is only defined inside the band, the kernel must not read outside it
WgradBand wgrad_band(const GBand &band, int B, int Sq, bool required) {
  return WgradBand{B, band.hi_slope, band.hi_slope ? -band.hi_base : 0, band.lo_slope, band.lo_slope ? -band.lo_base : Sq - 1,
                   required ? 1 : 0};
}

// The workspace, in floats; also the answer of the size query
struct BwdLayout {
  TableRows rho;                             // the table rows G covers
  int Rp, Kp;                                // those rows / the head dim as GEMM dimensions: whole K chunks (G is a GEMM operand as it stands)
  size_t dsum, g, wT, dw, wg, total;         // offsets: D | G | the packed table rows, transposed | dE of those rows | the weight-gradient GEMM's own
  size_t wg_floats;
};
BwdLayout carve(const isi_attn_args *g) {
  BwdLayout L;
  L.rho = rho_range(g);
  L.Rp = (int)round_up((size_t)std::max(L.rho.n, 1), kBK);
  L.Kp = (int)round_up((size_t)g->head_dim, kBK);
  size_t off = 0;
  auto take = [&](size_t n) { const size_t o = off; off += round_up(n, 64); return o; };
  L.dsum = take((size_t)g->B * g->H * g->Sq);
  L.g = L.wT = L.dw = L.wg = 0; L.wg_floats = 0;
  if (L.rho.n > 0) {
    L.g = take((size_t)g->H * g->B * g->Sq * L.Rp);
    L.wT = take((size_t)g->H * g->head_dim * L.Rp);
    L.dw = take((size_t)g->H * L.Rp * L.Kp);
    L.wg_floats = conv_wgrad_batched_workspace_floats(L.Rp, g->head_dim, g->B * g->Sq, 1, g->H);
    L.wg = take(L.wg_floats);
  }
  L.total = off;
  return L;
}

// Every condition of the backward's route, each derived once
struct BwdRoute {
  bool has_e;        // a table: G, the two products over it, d_rel
  bool split;        // precision >= 1: the split-bf16 kernel pair (512 threads); else the exact-fp32 pair
  bool one;          // ... with single-term products, like the forward of precision 2 (precision 3 runs three-term ones)
  bool saved;        // ... reading the forward's kept logits
  bool unit;         // one channel per event on both sides: every (query, key) pair has its own element of G, G is banded
  bool gemm_path;    // dQ += G E on the banded GEMM kernel (else the batched 1x1 convolution)
  bool band_only;    // only the margins of G's band are zeroed: the kernels store the whole band, zeros included
  bool g_from_kv;    // the key-stationary kernel (and the one-key kernel) store dS into G, the query-stationary kernel runs
                     // last and reads it back (AttnBwdKArgs.g_from_kv; ISI_ATTN_G_FROM_KV=0: every kernel forms its own dS)
  int tail_q, tail_k;   // rows / keys beyond the last full block that go through the one-row kernels (split pair only)
  GBand band;
};
BwdRoute make_route(const isi_attn_args *g, const BwdLayout &L) {
  BwdRoute r;
  r.has_e = L.rho.n > 0;
  r.split = g->precision >= 1;
  r.one = g->precision == 2;
  r.saved = r.split && g->logits != nullptr;      // (check_bwd_call: kept logits come with precision >= 1 only)
  r.unit = one_channel_per_event(g);
  // the GEMM kernel reads G and dq as [Sq B, .] matrices: q rows of consecutive (query, batch) a constant stride apart
  r.gemm_path = r.has_e && r.split && g->q_ss == (int64_t)g->B * g->q_sb && gemm_split_applicable(g->Sq * g->B, g->head_dim, L.Rp, 1) &&
                !knobs().no_gemm_kernel;
  // both products over G must skip what is not zeroed: the banded GEMM does, the 1x1 convolution reads all of G
  r.band_only = r.unit && r.gemm_path && !knobs().attn_full_zero;
  r.g_from_kv = r.band_only && r.saved && knobs().attn_g_from_kv;
  const bool dense = g->dense_mask != nullptr;
  // (the G row of a tail query is written with one key per column, which needs Ck = 1)
  r.tail_q = (r.split && (!r.has_e || g->Ck == 1)) ? attention_tail_rows(g->Sq, g->mask_mode, dense) : 0;
  r.tail_k = r.split ? attention_tail_rows(g->Sk, g->mask_mode, dense) : 0;
  r.band = g_band(g, L.rho);
  return r;
}

// every refusal of the backward, the workspace's included
int check_bwd_call(const isi_attn_bwd_args *ga, AttnSpans *sp, BwdLayout *L) {
  if (!ga) return invalid("rel_attention_bwd: null pointer");
  const isi_attn_args *g = &ga->fwd;
  if (!g->lse || !ga->d_out || !ga->dq || !ga->dk || !ga->dv || !ga->workspace) return invalid("rel_attention_bwd: null pointer");
  const uintptr_t own_ptrs = reinterpret_cast<uintptr_t>(ga->d_out) | reinterpret_cast<uintptr_t>(ga->dq) |
                             reinterpret_cast<uintptr_t>(ga->dk) | reinterpret_cast<uintptr_t>(ga->dv) |
                             reinterpret_cast<uintptr_t>(ga->workspace);
  if (const int rc = attn_check_common(g, "rel_attention_bwd", own_ptrs, sp)) return rc;
  if (g->head_dim != 16 && g->head_dim != 32 && g->head_dim != 64)
    return unsupported("rel_attention_bwd: head_dim must be 16, 32 or 64");
  if (31 / g->Cq + 127 / g->Ck + 1 > BAND) return unsupported("rel_attention_bwd: band too wide");   // the key-stationary tiles
  const bool has_e = g->rel_embeddings != nullptr;
  if (has_e && (g->rel_rows <= 0 || !ga->d_rel)) return invalid("rel_attention_bwd: rel_rows / d_rel missing");
  *L = carve(g);
  if (ga->workspace_floats < L->total) { set_last_error("rel_attention_bwd: workspace too small"); return ISI_E_WORKSPACE; }
  if (has_e && (int64_t)g->H * g->B * g->Sq * L->Rp > ((int64_t)1 << 30))
    return unsupported("rel_attention_bwd: G spans 4 GiB or more");
  if (g->logits) {      // the forward's logits (isi_attn_args.logits): read by the split kernels
    if (g->precision < 1) return unsupported("rel_attention_bwd: kept logits go with the 16-bit modes (precision >= 1)");
    if (g->logits_ld < ((g->Sk + 31) & ~31) || (g->logits_ld & 3) || (reinterpret_cast<uintptr_t>(g->logits) & 15) ||
        g->logits_ld > ((int64_t)1 << 30))
      return invalid("rel_attention_bwd: logits_ld must be a multiple of 4, at least Sk rounded up to 32; logits 16-byte aligned");
  }
  return ISI_OK;
}

// The kernels' argument block: first what the call hands over (all the statistics kernel reads) ...
AttnBwdKArgs tensor_args(const isi_attn_bwd_args *ga, const AttnSpans &sp, const BwdLayout &L) {
  const isi_attn_args *g = &ga->fwd;
  AttnBwdKArgs a;
  memset(&a, 0, sizeof a);
  attn_fill_common(a, g, sp);
  a.dout = ga->d_out;
  a.dsum = ga->workspace + L.dsum;
  a.dq = ga->dq; a.dk = ga->dk; a.dv = ga->dv;
  a.g = L.rho.n > 0 ? ga->workspace + L.g : nullptr;
  a.o_bytes = (unsigned)(sp.o * 4);
  a.Rp = L.Rp; a.rho_lo = L.rho.lo;
  if (g->logits) { a.logits = g->logits; a.ldl = (int)g->logits_ld; }
  return a;
}
// ... then what the attention kernels read of the route
void route_args(AttnBwdKArgs *a, const BwdRoute &r) {
  a->g_band_only = r.band_only ? 1 : 0;
  a->g_from_kv = r.g_from_kv ? 1 : 0;
  a->nqb = blocks(a->Sq, r.tail_q);
  a->nkb = blocks(a->Sk, r.tail_k);
}

// ---- phase 1: D, and G zeroed where the kernels will not store it
int enqueue_statistics_and_zero(const isi_attn_args *g, const AttnBwdKArgs &a, const BwdLayout &L, const BwdRoute &r, hipStream_t stream) {
  if (const int rc = launch_attn_dsum(a, g->head_dim, stream)) return rc;
  if (!r.has_e) return ISI_OK;
  if (r.band_only)
    return launch_attn_zero_g_margins(a.g, (long)g->H * g->Sq * g->B, g->Sq, g->B, L.Rp, r.band.lo_slope, r.band.lo_base, r.band.hi_slope,
                                      r.band.hi_base, stream);
  return launch_attn_zero_g(a.g, (size_t)g->H * g->B * g->Sq * L.Rp / 4, stream);      // Rp is a multiple of 4
}

// ---- phase 2: dK, dV, dQ (without the table's share) and G
int enqueue_attention(const AttnBwdKArgs &a, const BwdRoute &r, int HD, hipStream_t stream) {
  if (!r.split) return launch_attn_bwd_exact(a, HD, stream);      // (all blocks: no tails)
  const bool tails = r.tail_q || r.tail_k;
  // g_from_kv: the key-stationary kernel first, the one-key kernel next (it stores its column of G), the reader of G last
  int rc = launch_attn_bwd_split(a, HD, r.one, r.saved, r.g_from_kv ? 1 : 3, stream);
  if (!rc && tails) rc = launch_attn_bwd_tails(a, HD, r.tail_q, r.tail_k, stream);
  if (!rc && r.g_from_kv) rc = launch_attn_bwd_split(a, HD, r.one, r.saved, 2, stream);
  return rc;
}

// ---- phase 3: dQ += G E  and  dE = G^T Q, all heads in one launch each (grid z = head), on the GEMM kernels
int enqueue_products_over_g(const isi_attn_bwd_args *ga, const AttnBwdKArgs &a, const BwdLayout &L, const BwdRoute &r,
                            hipStream_t stream) {
  const isi_attn_args *g = &ga->fwd;
  const int HD = g->head_dim, R = g->rel_rows;
  float *wT = ga->workspace + L.wT, *dw = ga->workspace + L.dw;
  if (const int rc = launch_pack_rel_T(g->rel_embeddings, wT, g->H, R, HD, L.Rp, L.rho.lo, L.rho.n, stream)) return rc;
  const int gemm_flags = r.split ? ISI_CONV_BF16X3 : 0;   // same product mode as the attention kernels
  const int64_t zs_g = (int64_t)g->B * g->Sq * L.Rp, zs_w = (int64_t)HD * L.Rp;      // a head's G and packed table rows
  // G_h [Sq B, Rp] x E_h^T, accumulated into dq's head slice
  int rc;
  if (r.gemm_path) {
    GemmExtra gx;
    memset(&gx, 0, sizeof gx);
    gx.nz = g->H; gx.zs_a = zs_g; gx.zs_w = zs_w; gx.zs_res = g->q_sh; gx.zs_out = g->q_sh;
    if (r.unit) gemm_window(&gx, r.band, g->B);
    rc = gemm_split_f32(a.g, L.Rp, wT, nullptr, ga->dq, g->q_sb, ga->dq, g->q_sb, g->Sq * g->B, HD, L.Rp, 0, 1, stream, nullptr, &gx);
  } else {
    isi_src sg;
    memset(&sg, 0, sizeof sg);
    sg.ptr = a.g; sg.C = L.Rp; sg.sn = (int64_t)g->B * L.Rp; sg.sc = 1; sg.sh = L.Rp; sg.sw = L.Rp;   // "image" = [Sq][B][1]
    isi_src res;
    memset(&res, 0, sizeof res);
    res.ptr = ga->dq; res.C = HD; res.sn = g->q_ss; res.sc = 1; res.sh = g->q_sb; res.sw = g->q_sb;
    isi_dst dst;
    memset(&dst, 0, sizeof dst);
    dst.ptr = ga->dq; dst.sn = g->q_ss; dst.sc = 1; dst.sh = g->q_sb; dst.sw = g->q_sb;
    rc = conv2d_batched_f32(&sg, nullptr, wT, nullptr, &res, &dst, g->Sq, g->B, 1, HD, 1, 1, 1, 0, gemm_flags, g->H, zs_g, zs_w,
                            g->q_sh, g->q_sh, stream);
  }
  if (rc) return rc;
  // dE_h = G_h^T Q_h, the pixel-reduction GEMM, over the rows of the band only
  const WgradBand wb = wgrad_band(r.band, g->B, g->Sq, r.band_only);
  isi_src sq;
  memset(&sq, 0, sizeof sq);
  sq.ptr = g->q; sq.C = HD; sq.sn = g->q_ss; sq.sc = 1; sq.sh = g->q_sb; sq.sw = g->q_sb;
  rc = conv_wgrad_batched_f32(&sq, nullptr, a.g, dw, nullptr, ga->workspace + L.wg, L.wg_floats, g->Sq, g->B, 1, L.Rp, 1, 1, 1, 0,
                              gemm_flags, g->H, g->q_sh, zs_g, (int64_t)L.Rp * L.Kp, stream, 0, r.unit ? &wb : nullptr);
  if (rc) return rc;
  return launch_unpack_drel(dw, ga->d_rel, g->H, R, HD, L.Rp, L.Kp, L.rho.lo, L.rho.n, stream);
}

}  // namespace

size_t rel_attention_bwd_workspace_floats(const isi_attn_args *g) {
  if (!g || g->B <= 0 || g->H <= 0 || g->Sq <= 0) return 0;
  return carve(g).total;
}

int rel_attention_bwd_f32(const isi_attn_bwd_args *ga, hipStream_t stream) {
  AttnSpans sp;
  BwdLayout L;
  if (const int rc = check_bwd_call(ga, &sp, &L)) return rc;
  const isi_attn_args *g = &ga->fwd;
  const BwdRoute r = make_route(g, L);
  AttnBwdKArgs a = tensor_args(ga, sp, L);
  if (const int rc = enqueue_statistics_and_zero(g, a, L, r, stream)) return rc;
  route_args(&a, r);
  if (const int rc = enqueue_attention(a, r, g->head_dim, stream)) return rc;
  return r.has_e ? enqueue_products_over_g(ga, a, L, r, stream) : ISI_OK;
}

}  // namespace isi
