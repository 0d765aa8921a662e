// Cached attention of one query row per batch row against keys / values WITHOUT a batch dimension
// (isi_rel_attention_decode_shared_f32; isi_prior_state.memory_shared = 1): N variations of one request share the encoder
// memory, so a layer's projected memory is ONE [S_src, 2d] array.  rel_attention_decode_f32_kernel runs one workgroup per
// (row, head, key split) and streams that row's keys for one query: B identical copies per position.  Here a workgroup owns
// (head, key split) and ALL rows of a block of SH_RB rows; a key / value / table row is fetched once per workgroup and used
// by every row of the block, so the bytes a position fetches do not grow with B beyond the number of row blocks.
//   s_bj = scale * q_b . (k_j + e_r),  r = clamp(q_pos / Cq - j / Ck + Ek - 1, 0, R - 1)   (no table: e = 0)
//   out_b = sum_j softmax_j(s_b.) v_j                                                       (all of it fp32)
// The arithmetic contract is the per-row kernels'; the order of the sums differs (equal up to rounding).
//
// Keys pass through in tiles of SH_KT = 64.  Per tile:
//   stage   256 threads fetch the tile's k (+ e) and v rows, 16 bytes per lane and coalesced along the row, into LDS as fp32
//           (bf16 rows are widened exactly, bits << 16); the NEXT tile's rows are requested into registers before this tile's
//           arithmetic starts, so the memory round trip overlaps it
//   scores  lane = key, wave w = rows 4 w .. 4 w + 3 of the block: the lane holds its key row in registers (read once from
//           LDS, row stride HD + 4 floats: 16 lanes x 16 B cover the 64 banks) and takes the four q rows as LDS broadcasts
//   softmax a row's 64 scores of the tile lie in the 64 lanes of ONE wave: running maximum / sum per row by wave reductions
//           (flash-decoding's rescaling), no exchange between waves; the tile's probabilities go to the wave's own LDS rows
//   values  lane = feature (64 / HD key phases for head_dim < 64): o_r[d] += p_rj v_j[d], v from LDS without conflicts
// A split ends with the per-row kernels' partial row (un-normalised output, maximum, sum) in the caller's workspace, or with
// the normalised output when there is one split.  Keys beyond the count in use are never read (their rows may hold NaN).
// LDS 41984 bytes at head_dim 64; registers per lane: profiles/shared_memory_resource_usage.txt.
#include "isi_common.h"
#include "isi_internal.h"

namespace isi {

namespace {

constexpr int SH_KT = 64;      // keys per tile: one per lane of the score phase
constexpr int SH_RB = 16;      // rows per workgroup: four per wave

__device__ __forceinline__ float4 sh_widen_lo(const uint4 w) {
  return make_float4(__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u), __uint_as_float(w.y << 16),
                     __uint_as_float(w.y & 0xffff0000u));
}
__device__ __forceinline__ float4 sh_widen_hi(const uint4 w) {
  return make_float4(__uint_as_float(w.z << 16), __uint_as_float(w.z & 0xffff0000u), __uint_as_float(w.w << 16),
                     __uint_as_float(w.w & 0xffff0000u));
}

// KV16: k / v are bf16 arrays (strides in elements either way).  A staging unit is 16 bytes of a key row: 4 floats or 8 bf16.
template <int HD, bool KV16>
__global__ __launch_bounds__(256) void rel_attention_decode_shared_kernel(
    const float *__restrict__ q, const void *__restrict__ k_, const void *__restrict__ v_, const float *__restrict__ e,
    float *__restrict__ out, int B, int Sk, int64_t q_sb, int64_t q_sh, int64_t k_ss, int64_t k_sh, int64_t v_ss,
    int64_t v_sh, int64_t o_sb, int64_t o_sh, int q_pos, int Cq, int Ck, int Ek, int R, float scale, int chunk,
    float *__restrict__ partial, const int *__restrict__ pos) {
  constexpr int KS = HD + 4;                       // LDS stride of a staged key row
  constexpr int EPU = KV16 ? 8 : 4;                // elements per 16-byte unit
  constexpr int UPR = HD / EPU;                    // units per row
  constexpr int NU = (SH_KT * UPR + 255) / 256;    // units per thread and tile: 4 / 2 / 1 (fp32), 2 / 1 / 1 (bf16)
  constexpr int G = 64 / HD;                       // key phases of the value pass: 1, 2 or 4
  __shared__ __attribute__((aligned(16))) float ks[SH_KT * KS];
  __shared__ __attribute__((aligned(16))) float vs[SH_KT * HD];
  __shared__ __attribute__((aligned(16))) float qs[SH_RB * HD];
  __shared__ __attribute__((aligned(16))) float ps[SH_RB * SH_KT];
  if (pos) q_pos = *pos;                           // replayable launch: the position from device memory
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = blockIdx.x, b0 = blockIdx.y * SH_RB, split = blockIdx.z, ns = gridDim.z;
  const int kbeg = split * chunk;
  const int nk = max(min(Sk - kbeg, chunk), 0);    // keys of this split
  const int nrows = min(B - b0, SH_RB);
  if (nk <= 0) {                                   // empty split: the neutral partial of the per-row kernels
    for (int i = tid; i < nrows * HD; i += 256) {
      const int r = i / HD, dd = i % HD;
      float *pp = partial + (((size_t)(b0 + r) * gridDim.x + h) * ns + split) * (HD + 4);
      pp[dd] = 0.f;
      if (dd == 0) { pp[HD] = -1e30f; pp[HD + 1] = 0.f; }
    }
    return;
  }
  const int evq = q_pos / Cq;
  const char *kbase = reinterpret_cast<const char *>(k_), *vbase = reinterpret_cast<const char *>(v_);
  constexpr int ES = KV16 ? 2 : 4;                 // bytes per element
  const float *eh = e ? e + (size_t)h * R * HD : nullptr;

  // the block's q rows (zero rows beyond the batch)
  for (int i = tid; i < SH_RB * HD / 4; i += 256) {
    const int r = i / (HD / 4), c = i % (HD / 4);
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < nrows) t = *reinterpret_cast<const float4 *>(q + (b0 + r) * q_sb + h * q_sh + c * 4);
    *reinterpret_cast<float4 *>(qs + r * HD + c * 4) = t;
  }

  uint4 kr[NU], vr[NU];
  float4 ea[NU], eb[NU];
  auto fetch = [&](int t0) {                       // tile starting at local key t0 -> registers
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int i = tid + 256 * u, j = i / UPR, c = i % UPR;
      kr[u] = vr[u] = make_uint4(0u, 0u, 0u, 0u);
      ea[u] = eb[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (j < SH_KT && t0 + j < nk) {
        const int64_t key = kbeg + t0 + j;
        kr[u] = *reinterpret_cast<const uint4 *>(kbase + (key * k_ss + h * k_sh + c * EPU) * ES);
        vr[u] = *reinterpret_cast<const uint4 *>(vbase + (key * v_ss + h * v_sh + c * EPU) * ES);
        if (eh) {
          int r = evq - (int)(key / Ck) + Ek - 1;
          r = r < 0 ? 0 : (r >= R ? R - 1 : r);
          ea[u] = *reinterpret_cast<const float4 *>(eh + (size_t)r * HD + c * EPU);
          if (KV16) eb[u] = *reinterpret_cast<const float4 *>(eh + (size_t)r * HD + c * EPU + 4);
        }
      }
    }
  };
  auto add4 = [](const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); };
  auto stage = [&]() {                             // registers -> LDS (keys with the table row added)
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int i = tid + 256 * u, j = i / UPR, c = i % UPR;
      if (j >= SH_KT) continue;
      if constexpr (KV16) {
        *reinterpret_cast<float4 *>(ks + j * KS + c * 8) = add4(sh_widen_lo(kr[u]), ea[u]);
        *reinterpret_cast<float4 *>(ks + j * KS + c * 8 + 4) = add4(sh_widen_hi(kr[u]), eb[u]);
        *reinterpret_cast<float4 *>(vs + j * HD + c * 8) = sh_widen_lo(vr[u]);
        *reinterpret_cast<float4 *>(vs + j * HD + c * 8 + 4) = sh_widen_hi(vr[u]);
      } else {
        const float4 kf = make_float4(__uint_as_float(kr[u].x), __uint_as_float(kr[u].y), __uint_as_float(kr[u].z),
                                      __uint_as_float(kr[u].w));
        *reinterpret_cast<float4 *>(ks + j * KS + c * 4) = add4(kf, ea[u]);
        *reinterpret_cast<float4 *>(vs + j * HD + c * 4) =
            make_float4(__uint_as_float(vr[u].x), __uint_as_float(vr[u].y), __uint_as_float(vr[u].z), __uint_as_float(vr[u].w));
      }
    }
  };

  float m[4], l[4], o[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m[r] = -1e30f; l[r] = 0.f; o[r] = 0.f; }
  const float *qw = qs + wave * 4 * HD;            // this wave's four q rows
  float *pw = ps + wave * 4 * SH_KT;               // ... and their probabilities of the tile
  const int dd = lane % HD, kp = lane / HD;        // value pass: feature and key phase of this lane

  fetch(0);
  for (int t0 = 0; t0 < nk; t0 += SH_KT) {
    stage();
    __syncthreads();
    if (t0 + SH_KT < nk) fetch(t0 + SH_KT);
    // ---- scores of key t0 + lane against the wave's four rows
    float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < HD / 4; ++c) {
      const float4 kk = *reinterpret_cast<const float4 *>(ks + lane * KS + c * 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float4 qq = *reinterpret_cast<const float4 *>(qw + r * HD + c * 4);
        s[r] += (qq.x * kk.x + qq.y * kk.y) + (qq.z * kk.z + qq.w * kk.w);
      }
    }
    const bool live = t0 + lane < nk;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float sv = live ? s[r] * scale : -1e30f;
      const float mn = fmaxf(m[r], wave64_max(sv));          // (the tile holds at least one live key: mn is a real score)
      const float alpha = __expf(m[r] - mn);
      const float pj = live ? __expf(sv - mn) : 0.f;
      l[r] = l[r] * alpha + wave64_sum(pj);
      o[r] *= alpha;
      m[r] = mn;
      pw[r * SH_KT + lane] = pj;
    }
    __syncthreads();
    // ---- values: o_r[dd] += p_rj v_j[dd] over the keys of this lane's phase
#pragma unroll 4
    for (int j4 = 0; j4 < SH_KT; j4 += 4 * G) {
      const int j = j4 + kp * 4;
      float4 p4[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) p4[r] = *reinterpret_cast<const float4 *>(pw + r * SH_KT + j);
      const float v0 = vs[(j + 0) * HD + dd], v1 = vs[(j + 1) * HD + dd], v2 = vs[(j + 2) * HD + dd], v3 = vs[(j + 3) * HD + dd];
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] += (p4[r].x * v0 + p4[r].y * v1) + (p4[r].z * v2 + p4[r].w * v3);
    }
    __syncthreads();                               // the next tile overwrites ks / vs
  }
  // the key phases of a feature meet (head_dim < 64)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int off = HD; off < 64; off <<= 1) o[r] += __shfl_xor(o[r], off);
  }
  if (kp != 0) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = b0 + wave * 4 + r;
    if (b >= B) continue;
    if (ns == 1) {
      out[b * o_sb + h * o_sh + dd] = o[r] / l[r];
    } else {
      float *pp = partial + (((size_t)b * gridDim.x + h) * ns + split) * (HD + 4);
      pp[dd] = o[r];
      if (dd == 0) { pp[HD] = m[r]; pp[HD + 1] = l[r]; }
    }
  }
}

}  // namespace

int rel_attention_decode_shared_row_blocks(int B) { return (B + SH_RB - 1) / SH_RB; }

// key splits of one (head, row block): tiles of 64 keys, at most 8 (the workspace and the merge of the per-row kernels are
// kept), and no more than it takes to put ~512 workgroups on the chip -- the grid is heads x row blocks x splits, so a batch
// of 32 rows (two row blocks x 8 heads) still takes all 8
int rel_attention_decode_shared_splits(int Sk, int B, int H) {
  const int groups = H * rel_attention_decode_shared_row_blocks(B);
  const int tiles = (Sk + SH_KT - 1) / SH_KT;
  const int by_keys = tiles > 8 ? 8 : tiles;
  const int by_chip = groups <= 0 ? 8 : (512 + groups - 1) / groups;
  const int ns = by_keys < by_chip ? by_keys : by_chip;
  return ns < 1 ? 1 : ns;
}

// pos != nullptr: the query position is read from device memory (replayable launch).  combine = 0: with several splits the
// partial rows stay in `workspace` ([B, H, splits, head_dim + 4], the per-row kernels' layout) for the caller to merge.
int rel_attention_decode_shared_launch(const isi_attn_args *g, int q_pos, const int *pos, float *workspace, int combine,
                                       int kv_format, hipStream_t stream) {
  if (!g || !g->q || !g->k || !g->v || !g->out) return invalid("attention_decode_shared: null pointer");
  if (kv_format != ISI_KV_F32 && kv_format != ISI_KV_BF16)
    return invalid("attention_decode_shared: kv_format must be ISI_KV_F32 or ISI_KV_BF16");
  if (g->k_sb != 0 || g->v_sb != 0)
    return invalid("attention_decode_shared: k_sb and v_sb must be 0 (the keys / values have no batch dimension)");
  if (g->Sk <= 0 || g->B <= 0 || g->H <= 0 || g->Cq <= 0 || g->Ck <= 0) return invalid("attention_decode_shared: bad shape");
  if (g->B > 256) return unsupported("attention_decode_shared: at most 256 rows");
  if (g->Sk > 65536) return unsupported("attention_decode_shared: more than 65536 keys");
  const bool kv16 = kv_format == ISI_KV_BF16;
  const int unit = kv16 ? 8 : 4;                   // elements of a 16-byte load
  if (((reinterpret_cast<uintptr_t>(g->q) | reinterpret_cast<uintptr_t>(g->k) | reinterpret_cast<uintptr_t>(g->v) |
        reinterpret_cast<uintptr_t>(g->rel_embeddings)) & 15) ||
      ((g->k_ss | g->k_sh | g->v_ss | g->v_sh) & (unit - 1)) || ((g->q_sb | g->q_sh) & 3))
    return invalid("attention_decode_shared: q, k, v, rel_embeddings 16-byte aligned; k / v strides multiples of 4 (bf16: 8) elements, q strides of 4");
  const int ns = workspace ? rel_attention_decode_shared_splits(g->Sk, g->B, g->H) : 1;
  const int chunk = (g->Sk + ns - 1) / ns;
  dim3 grid(g->H, rel_attention_decode_shared_row_blocks(g->B), ns), block(256);
#define ISI_DEC_SHARED(HD, KV16)                                                                                        \
  hipLaunchKernelGGL((rel_attention_decode_shared_kernel<HD, KV16>), grid, block, 0, stream, g->q, g->k, g->v,           \
                     g->rel_embeddings, g->out, g->B, g->Sk, g->q_sb, g->q_sh, g->k_ss, g->k_sh, g->v_ss, g->v_sh,      \
                     g->o_sb, g->o_sh, q_pos, g->Cq, g->Ck, g->Ek, g->rel_rows, g->scale, chunk, workspace, pos)
  switch (g->head_dim) {
    case 16: if (kv16) ISI_DEC_SHARED(16, true); else ISI_DEC_SHARED(16, false); break;
    case 32: if (kv16) ISI_DEC_SHARED(32, true); else ISI_DEC_SHARED(32, false); break;
    case 64: if (kv16) ISI_DEC_SHARED(64, true); else ISI_DEC_SHARED(64, false); break;
    default: return unsupported("attention_decode_shared: head_dim must be 16, 32 or 64");
  }
#undef ISI_DEC_SHARED
  int rc = check_launch("rel_attention_decode_shared");
  if (rc || ns == 1 || !combine) return rc;
  return rel_attention_decode_combine(workspace, g->out, g->B, g->H, g->head_dim, ns, g->o_sb, g->o_sh, stream);
}

}  // namespace isi
