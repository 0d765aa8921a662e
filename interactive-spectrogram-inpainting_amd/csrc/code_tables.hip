// The two layers of the VQ-VAE forward that read nothing but the quantised TOP map, as sums of pack-time table rows.
//
// Every pixel of quant_t is one of the K codebook rows E[k], and dec_t's first 3x3 convolution and
// upsample_top_to_bottom[0] (ConvTranspose2d k4 s2 p1) are linear in it: bias, zero padding, no ReLU in front of the
// sum.  The per-pixel products W[tap] . E[id] can therefore take only taps x K values, computed once per version of the
// codebook and of the two weights:
//   T3 [tap = kh*3 + kw][code][Cout]              T3[t][k][n]     = sum_c W3[n][t*Cin + c]    E[k][c]
//   TU [phase = py*2 + px][tap = ty*2 + tx][code][Cout]
//                                                 TU[ph][t][k][n] = sum_c Wph[ph][n][t*Cin + c] E[k][c]
// (W3: the packed 3x3 weight [Cout][Kpad]; Wph: the packed phase matrices [4][Cout][Kpad] of pack.hip), each entry
// accumulated in double and rounded to fp32 once.  A gathered row is Cout floats, contiguous and 16-byte aligned.  Behind
// the last block every table carries one PAD ROW of -0.0: what a tap outside the map gathers (x + -0 = x bit for bit).
//   conv3[b,y,x,:]       = relu(bias + sum_{taps inside the map} T3[tap][id[b, y+kh-1, x+kw-1]])
//   up[b,2y+py,2x+px,:]  =      bias + sum_{ty,tx inside the map} TU[ph][t][id[b, y-1+py+ty, x-1+px+tx]]
// The taps are added in ascending tap order after the bias, a tap outside the map adds nothing: the bits of an output
// pixel depend on its window's codes alone, not on the batch or the launch geometry.  No MFMA, no LDS, no barrier.
#include <algorithm>

#include "isi_common.h"
#include "isi_internal.h"
#include "split_f16.h"

namespace isi {

namespace {

constexpr int kBlock = 256;

// table[(s * T + t)][k][n] = sum_c M[s][n][t * Cin + c] * E[k][c]; one thread per entry, n fastest
__global__ __launch_bounds__(kBlock) void code_table_pack_kernel(const float *__restrict__ M, const float *__restrict__ E,
                                                                 float *__restrict__ table, int sets, int taps, int Cout, int Cin,
                                                                 int Kpad, int K) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t entries = (int64_t)sets * taps * K * Cout;
  if (i >= entries + Cout) return;
  if (i >= entries) {       // the pad row behind the last block: what a tap outside the map gathers
    table[i] = -0.f;
    return;
  }
  const int n = (int)(i % Cout);
  const int64_t r = i / Cout;
  const int k = (int)(r % K);
  const int st = (int)(r / K);
  const int s = st / taps, t = st - s * taps;
  const float *m = M + ((int64_t)s * Cout + n) * Kpad + (int64_t)t * Cin;
  const float *e = E + (int64_t)k * Cin;
  double acc = 0.0;
  for (int c = 0; c < Cin; ++c) acc += (double)m[c] * (double)e[c];
  table[i] = (float)acc;
}

struct GatherHalf {
  const float *table;   // null: this half is not run
  const float *bias;
  float *out;           // dense channels-last [B, OH, OW, C]
  int C;                // channels (multiple of 4, <= 1024)
  int pair;             // output in the pair format (split_f16.h) instead of fp32
  int relu;
  int lp;               // lanes per code-map column = C / 4
  int ppb;              // code-map columns per workgroup = kBlock / lp
  unsigned lp_recip;    // ceil(2^20 / lp): tid / lp = (tid * lp_recip) >> 20 for tid < 256
  unsigned chunks;      // workgroups per output row
  unsigned row_bytes;   // 4 C
};

__device__ __forceinline__ float4 f4_add(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// acc (the bias, then the taps' sum) -> the output format, 4 channels at byte offset `off` of the output row
__device__ __forceinline__ void store_pixel(float4 acc, const bool bad, const GatherHalf &h, char *orow, const unsigned off, const int c4) {
  if (bad) {
    const float nan = __builtin_nanf("");
    acc = make_float4(nan, nan, nan, nan);
  }
  if (h.relu)   // NaN-propagating, like the convolution kernels' epilogues
    acc = make_float4(fmaxf(acc.x, 0.f) + (acc.x - acc.x), fmaxf(acc.y, 0.f) + (acc.y - acc.y), fmaxf(acc.z, 0.f) + (acc.z - acc.z),
                      fmaxf(acc.w, 0.f) + (acc.w - acc.w));
  if (h.pair) {
    // pair8 group of 8 channels = {hi[8] | lo[8]} (32 bytes): this lane's 4 channels are one half of both 16-byte pieces
    uint2 hi, lo;
    f16s::split4(acc, f16s::kScaleA, hi, lo);
    uint2 *g = reinterpret_cast<uint2 *>(orow + (off & ~31u));
    g[c4 & 1] = hi;
    g[2 + (c4 & 1)] = lo;
  } else {
    *reinterpret_cast<float4 *>(orow + off) = acc;
  }
}

// The 4 channels `c4` of code-map column x in output row `row`: UP = false one pixel from its 3x3 window, UP = true the
// two output pixels (2x, 2x + 1) of that row from the 2 x 3 window they share.  `ids`: the int64 code map read as
// 32-bit words (low word first).  Every tap is loaded: a tap outside the map, and a code outside [0, K) -- the search's
// -1 for an activation beyond the f16 range, never used as an address --, reads the table's pad row of -0.0, whose
// addition changes no bit (x + -0 = x for every x): the same bits as skipping the tap.  A bad code inside the window
// turns the pixel into NaN.  Offsets are 32-bit on uniform 64-bit bases (the host checks the sizes).
template <bool UP>
__device__ __forceinline__ void gather_item(const unsigned *__restrict__ ids, const GatherHalf &h, const int b, const int row,
                                            const int x, const int c4, const int H, const int W, const unsigned K) {
  constexpr int NR = UP ? 2 : 3, TAPS = UP ? 4 : 9, TOTAL = UP ? 16 : 9;
  const int y0 = UP ? (row >> 1) - 1 + (row & 1) : row - 1;     // first window row in the code map (uniform)
  const int py = UP ? (row & 1) : 0;
  unsigned id[NR][3];
  bool in[NR][3];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int yy = y0 + r;
    const bool rv = (unsigned)yy < (unsigned)H;
    const unsigned *irow = ids + 2 * (((size_t)b * H + (size_t)min(max(yy, 0), H - 1)) * W);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int xx = x - 1 + j;
      in[r][j] = rv && (unsigned)xx < (unsigned)W;
      id[r][j] = irow[2u * (unsigned)min(max(xx, 0), W - 1)];
    }
  }
  const unsigned c16 = 16u * (unsigned)c4;
  bool bad[2] = {false, false};
  float4 v[UP ? 2 : 1][TAPS];
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const bool lt = id[r][j] < K;          // one unsigned compare: negative and too-large codes alike
      const bool ok = in[r][j] && lt, b_ = in[r][j] && !lt;
#pragma unroll
      for (int px = 0; px < (UP ? 2 : 1); ++px) {
        const int tx = UP ? j - px : j;      // this window column as a tap of output pixel px
        if (tx < 0 || tx >= (UP ? 2 : 3)) continue;
        const int t = UP ? r * 2 + tx : r * 3 + j;
        const unsigned tap = UP ? (unsigned)(py * 2 + px) * TAPS + t : (unsigned)t;     // uniform
        // row `id` of this tap's block, or the pad row behind the last block (K (TOTAL - tap) rows further on)
        const unsigned rsel = ok ? id[r][j] : K * (TOTAL - tap);
        const char *tb = reinterpret_cast<const char *>(h.table) + (size_t)tap * K * h.row_bytes;
        v[px][t] = *reinterpret_cast<const float4 *>(tb + (__umul24(rsel, h.row_bytes) + c16));
        bad[px] |= b_;
      }
    }
  const float *bp = reinterpret_cast<const float *>(reinterpret_cast<const char *>(h.bias) + c16);
  const float4 bias = make_float4(bp[0], bp[1], bp[2], bp[3]);
  const int OW = UP ? 2 * W : W, OH = UP ? 2 * H : H;
  char *orow = reinterpret_cast<char *>(h.out) + ((size_t)b * OH + row) * OW * h.row_bytes;
#pragma unroll
  for (int px = 0; px < (UP ? 2 : 1); ++px) {
    float4 acc = bias;
#pragma unroll
    for (int t = 0; t < TAPS; ++t) acc = f4_add(acc, v[px][t]);      // ascending tap order after the bias
    store_pixel(acc, bad[px], h, orow, (unsigned)(UP ? 2 * x + px : x) * h.row_bytes + c16, c4);
  }
}

// Workgroups [0, blocks3) run the conv3 half, the rest the upsample half: one table at a time is the working set.
// A workgroup covers `ppb` consecutive code-map columns of one output row; a lane owns 4 consecutive channels.
__global__ __launch_bounds__(kBlock) void code_gather_kernel(const unsigned *__restrict__ ids, const GatherHalf h3, const GatherHalf hu,
                                                             const unsigned blocks3, const int H, const int W, const unsigned K) {
  const bool up = blockIdx.x >= blocks3;
  const unsigned bid = up ? blockIdx.x - blocks3 : blockIdx.x;
  const unsigned chunks = up ? hu.chunks : h3.chunks, lp = up ? hu.lp : h3.lp, ppb = up ? hu.ppb : h3.ppb;
  const unsigned r = bid / chunks, chunk = bid - r * chunks;
  const unsigned OH = up ? 2 * H : H;
  const int b = (int)(r / OH), row = (int)(r - (unsigned)b * OH);
  const unsigned pl = (threadIdx.x * (up ? hu.lp_recip : h3.lp_recip)) >> 20;
  const int c4 = (int)(threadIdx.x - pl * lp);
  const int x = (int)(chunk * ppb + pl);
  if (pl >= ppb || x >= W) return;
  if (up) gather_item<true>(ids, hu, b, row, x, c4, H, W, K);
  else gather_item<false>(ids, h3, b, row, x, c4, H, W, K);
}

bool fill_half(GatherHalf &h, const float *table, const float *bias, float *out, int C, int pair, int relu, int W) {
  h = GatherHalf{};
  if (!table) return true;
  if (!bias || !out || C <= 0 || (C & 3) || C > 4 * kBlock || (pair && (C & 7))) return false;
  if ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(out)) & 15) return false;
  if (reinterpret_cast<uintptr_t>(bias) & 3) return false;
  h.table = table; h.bias = bias; h.out = out; h.C = C; h.pair = pair ? 1 : 0; h.relu = relu ? 1 : 0;
  h.lp = C / 4;
  h.ppb = kBlock / h.lp;
  h.lp_recip = (unsigned)(((1u << 20) + h.lp - 1) / h.lp);
  h.chunks = (unsigned)((W + h.ppb - 1) / h.ppb);
  h.row_bytes = 4u * (unsigned)C;
  return true;
}

}  // namespace

size_t vq_code_tables_bytes(int which, int K, int Cout) {
  if (K <= 0 || Cout <= 0 || (which != 0 && which != 1)) return 0;
  return ((size_t)(which == 0 ? 9 : 16) * K + 1) * Cout * sizeof(float);   // + the pad row
}

int vq_pack_code_tables_f32(const float *w3_packed, int Cout3, const float *wT_packed, int CoutU, const float *codes_kd, int D,
                            int K, float *t3_out, float *tu_out, hipStream_t stream) {
  if (!codes_kd || D <= 0 || K <= 0 || (!t3_out && !tu_out)) return invalid("vq_pack_code_tables: bad argument");
  if ((t3_out && (!w3_packed || Cout3 <= 0 || (Cout3 & 3))) || (tu_out && (!wT_packed || CoutU <= 0 || (CoutU & 3))))
    return invalid("vq_pack_code_tables: a table needs its packed weight and a channel count that is a multiple of 4");
  if ((reinterpret_cast<uintptr_t>(t3_out) | reinterpret_cast<uintptr_t>(tu_out)) & 15)
    return invalid("vq_pack_code_tables: tables must be 16-byte aligned");
  if (tu_out && convT_small_applicable(D, CoutU))
    return unsupported("vq_pack_code_tables: the few-channel transposed-convolution layout has no phase matrices");
  if (t3_out) {
    const int64_t total = ((int64_t)9 * K + 1) * Cout3;
    hipLaunchKernelGGL(code_table_pack_kernel, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, w3_packed,
                       codes_kd, t3_out, 1, 9, Cout3, D, (int)round_up((size_t)9 * D, kBK), K);
    if (int rc = check_launch("vq_pack_code_tables_f32 (conv3)")) return rc;
  }
  if (tu_out) {
    const int64_t total = ((int64_t)16 * K + 1) * CoutU;
    hipLaunchKernelGGL(code_table_pack_kernel, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, wT_packed,
                       codes_kd, tu_out, 4, 4, CoutU, D, (int)round_up((size_t)4 * D, kBK), K);
    if (int rc = check_launch("vq_pack_code_tables_f32 (upsample)")) return rc;
  }
  return ISI_OK;
}

int vq_code_gather_f32(const int64_t *ids, const float *t3, const float *bias3, float *out3, int C3, int out3_pair, int relu3,
                       const float *tu, const float *biasU, float *outU, int CU, int outU_pair, int reluU, int B, int H, int W,
                       int K, hipStream_t stream) {
  if (!ids || (reinterpret_cast<uintptr_t>(ids) & 7) || B <= 0 || H <= 0 || W <= 0 || K <= 0 || (!t3 && !tu))
    return invalid("vq_code_gather: bad argument");
  GatherHalf h3, hu;
  if (!fill_half(h3, t3, bias3, out3, C3, out3_pair, relu3, W) || !fill_half(hu, tu, biasU, outU, CU, outU_pair, reluU, W))
    return invalid("vq_code_gather: channels a multiple of 4 (8 for pair output) up to 1024, tables and outputs 16-byte aligned");
  const int64_t blocks3 = t3 ? (int64_t)B * H * h3.chunks : 0;
  const int64_t blocksU = tu ? (int64_t)B * 2 * H * hu.chunks : 0;
  const int Cmax = std::max(t3 ? C3 : 0, tu ? CU : 0);
  // the kernel's 32-bit offsets: a whole table and one output row below 4 GiB, row indices within 24 bits
  if (blocks3 + blocksU >= (1ll << 31) || (int64_t)B * H * W >= (1ll << 30) || ((int64_t)16 * K + 1) * Cmax >= (1ll << 30) ||
      K >= (1 << 20) || (int64_t)W * Cmax >= (1ll << 29))
    return unsupported("vq_code_gather: map or table too large");
  hipLaunchKernelGGL(code_gather_kernel, dim3((unsigned)(blocks3 + blocksU)), dim3(kBlock), 0, stream,
                     reinterpret_cast<const unsigned *>(ids), h3, hu, (unsigned)blocks3, H, W, (unsigned)K);
  return check_launch("vq_code_gather_f32");
}

}  // namespace isi
