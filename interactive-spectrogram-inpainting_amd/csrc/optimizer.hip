// Adam with device-resident hyper-parameters (include/isi_hip.h: isi_adam_step_f32, isi_grad_sumsq_f32,
// isi_grad_clip_coef_f32).  One streaming pass over (p, g, m, v): 16 bytes read and 12 written per element, no reuse, so
// the only design questions are access width and bytes in flight.
//
// Work split.  Every tensor is cut into chunks of kChunk elements counted from ITS OWN start; a workgroup owns one chunk.
// The table of tensors travels by value in the kernel arguments (like reduce_jobs_kernel's job table), together with the
// running chunk count behind every entry: a workgroup finds its tensor by a binary search over at most kTensorsPerLaunch
// scalars.  Nothing the kernel dereferences lives in device memory except the hyper-parameter block and the clip
// coefficient, so a stream capture bakes the addresses like any other launch's, and the host changes lr / betas of a
// recorded step by rewriting 64 bytes per param group.
//
// Access width.  A chunk whose four addresses share one residue mod 16 runs `head` (< 4) elements one by one, then float4
// loads / stores, then a tail of < 4 elements; dense 16-byte-aligned tensors (the normal case) have no head.  A chunk whose
// addresses disagree mod 16 (a sliced parameter with an aligned gradient) runs element-wise throughout.  Every element
// goes through the same adam_update(), so the route does not change the bits.
#include <algorithm>

#include "isi_common.h"
#include "isi_internal.h"

namespace isi {
namespace {

constexpr int kChunk = 2048;              // elements per workgroup: 2 float4 per lane and array, 8 loads in flight per lane
constexpr int kThreads = 256;
constexpr int kTensorsPerLaunch = 64;

struct AdamPack {
  isi_adam_tensor t[kTensorsPerLaunch];
  int chunk_end[kTensorsPerLaunch];       // chunks of entries 0..i (inclusive running count)
  int n;
};
static_assert(sizeof(AdamPack) <= 3800, "the tensor table must fit the kernel-argument segment");

__host__ __device__ inline int64_t chunks_of(int64_t n) { return (n + kChunk - 1) / kChunk; }

// (uniform per workgroup) entry of chunk `c`: the first i with c < chunk_end[i]
__device__ __forceinline__ int find_entry(const AdamPack &pack, int c) {
  int lo = 0, hi = pack.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (c < pack.chunk_end[mid]) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// Every line is evaluated in double from double hyper-parameters and rounded to fp32 once; only g' = g * coef is an fp32
// product (clip_grad_norm_ scales the fp32 gradient in place, and the spec follows it).  Why not fp32 throughout: torch's
// fused Adam keeps lr / betas / eps as doubles, so its two moment lines are double expressions rounded once (measured:
// 0.50 ulp of m and v against the float64 spec), and the kernel is held to twice torch's error with a floor of 1 ulp
// (tests/test_optimizer_gpu.py).  The all-fp32 form with fused multiply-adds, emulated in IEEE fp32 on the same inputs,
// is 2.3 - 4.2 ulp off in v and tens of thousands of ulp in m where b1 m and (1 - b1) g cancel
// (profiles/optimizer_step.json, "all_fp32_form_emulated").  p = p - update cancels the same way for elements that land
// near zero, where any rounding of the update is hundreds of ulp of the result (torch: 922 - 968, the all-fp32 form
// 498 - 1325); in double the result is the correctly rounded one.  The pass moves 28 bytes per element, and the fp64 work
// (two fma lines, one sqrt, one division) is not free: on the top prior's 76 M parameters the bare step reaches 4.0 TB/s of
// those bytes where torch's fused Adam reaches 4.5 TB/s (0.53 against 0.47 ms; with clipping 0.55 against 0.93 ms); the
// replayed training step is the same within its spread (profiles/optimizer_step.json).
__device__ __forceinline__ void adam_update(float &p, const float g, float &m, float &v, const isi_adam_hyper &h,
                                            const float coef) {
  const double gs = (double)(g * coef);
  const double md = fma(h.b1, (double)m, h.one_minus_b1 * gs);
  const double vd = fma(h.b2, (double)v, (h.one_minus_b2 * gs) * gs);
  const double denom = fma(sqrt(vd), h.inv_sqrt_bc2, h.eps);
  p = (float)fma(-h.step_size, md / denom, (double)p);
  m = (float)md;
  v = (float)vd;
}

// elements [0, head) and [head + 4 nvec, len) one by one, float4 in between; head = len: all element-wise
struct ChunkSplit { int head, nvec, tail0, len; };
__device__ __forceinline__ ChunkSplit split_chunk(uintptr_t a0, uintptr_t a1, uintptr_t a2, uintptr_t a3, int len) {
  const unsigned r = (unsigned)(a0 & 15);
  ChunkSplit s;
  s.len = len;
  if ((a1 & 15) != r || (a2 & 15) != r || (a3 & 15) != r) { s.head = len; s.nvec = 0; s.tail0 = len; return s; }
  s.head = min((int)(((16u - r) & 15u) >> 2), len);
  s.nvec = (len - s.head) >> 2;
  s.tail0 = s.head + 4 * s.nvec;
  return s;
}

__global__ __launch_bounds__(kThreads) void adam_step_kernel(const AdamPack pack, const isi_adam_hyper *__restrict__ hyper,
                                                             const float *__restrict__ coef_ptr) {
  const int c = (int)blockIdx.x;
  const int e = find_entry(pack, c);
  const isi_adam_tensor &t = pack.t[e];
  const int64_t start = (int64_t)(c - (e ? pack.chunk_end[e - 1] : 0)) * kChunk;
  const int len = (int)min((int64_t)kChunk, t.n - start);
  float *p = t.p + start;
  const float *g = t.g + start;
  float *m = t.m + start, *v = t.v + start;
  const isi_adam_hyper h = hyper[t.group];
  const float coef = coef_ptr ? coef_ptr[0] : 1.0f;
  const ChunkSplit s = split_chunk((uintptr_t)p, (uintptr_t)g, (uintptr_t)m, (uintptr_t)v, len);
  const int tid = (int)threadIdx.x;

  float4 *p4 = reinterpret_cast<float4 *>(p + s.head);
  const float4 *g4 = reinterpret_cast<const float4 *>(g + s.head);
  float4 *m4 = reinterpret_cast<float4 *>(m + s.head), *v4 = reinterpret_cast<float4 *>(v + s.head);
  constexpr int kIter = kChunk / 4 / kThreads;
  float4 P[kIter], G[kIter], M[kIter], V[kIter];
#pragma unroll
  for (int i = 0; i < kIter; ++i) {             // every load of the chunk is issued before the first use
    const int j = tid + i * kThreads;
    if (j < s.nvec) { P[i] = p4[j]; G[i] = g4[j]; M[i] = m4[j]; V[i] = v4[j]; }
  }
#pragma unroll
  for (int i = 0; i < kIter; ++i) {
    const int j = tid + i * kThreads;
    if (j < s.nvec) {
      adam_update(P[i].x, G[i].x, M[i].x, V[i].x, h, coef);
      adam_update(P[i].y, G[i].y, M[i].y, V[i].y, h, coef);
      adam_update(P[i].z, G[i].z, M[i].z, V[i].z, h, coef);
      adam_update(P[i].w, G[i].w, M[i].w, V[i].w, h, coef);
      p4[j] = P[i]; m4[j] = M[i]; v4[j] = V[i];
    }
  }
  // head and tail (< 4 elements each), or the whole chunk when the addresses disagree mod 16
  for (int j = tid; j < s.head; j += kThreads) {
    float pj = p[j], mj = m[j], vj = v[j];
    adam_update(pj, g[j], mj, vj, h, coef);
    p[j] = pj; m[j] = mj; v[j] = vj;
  }
  for (int j = s.tail0 + tid; j < s.len; j += kThreads) {
    float pj = p[j], mj = m[j], vj = v[j];
    adam_update(pj, g[j], mj, vj, h, coef);
    p[j] = pj; m[j] = mj; v[j] = vj;
  }
}

// sum of g^2 over one chunk -> partials[chunk0 + blockIdx.x].  Fixed order: a lane's elements in index order, the lanes of a
// wave by the DPP tree, the four waves in wave order.
__global__ __launch_bounds__(kThreads) void grad_sumsq_kernel(const AdamPack pack, float *__restrict__ partials,
                                                              const int64_t chunk0) {
  __shared__ float red[kThreads / 64];
  const int c = (int)blockIdx.x;
  const int e = find_entry(pack, c);
  const isi_adam_tensor &t = pack.t[e];
  const int64_t start = (int64_t)(c - (e ? pack.chunk_end[e - 1] : 0)) * kChunk;
  const int len = (int)min((int64_t)kChunk, t.n - start);
  const float *g = t.g + start;
  const uintptr_t a = (uintptr_t)g;
  const ChunkSplit s = split_chunk(a, a, a, a, len);
  const int tid = (int)threadIdx.x;
  const float4 *g4 = reinterpret_cast<const float4 *>(g + s.head);
  float acc = 0.0f;
  for (int j = tid; j < s.head; j += kThreads) acc = fmaf(g[j], g[j], acc);
  constexpr int kIter = kChunk / 4 / kThreads;
  float4 G[kIter];
#pragma unroll
  for (int i = 0; i < kIter; ++i) {
    const int j = tid + i * kThreads;
    G[i] = j < s.nvec ? g4[j] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int i = 0; i < kIter; ++i) {
    acc = fmaf(G[i].x, G[i].x, acc);
    acc = fmaf(G[i].y, G[i].y, acc);
    acc = fmaf(G[i].z, G[i].z, acc);
    acc = fmaf(G[i].w, G[i].w, acc);
  }
  for (int j = s.tail0 + tid; j < s.len; j += kThreads) acc = fmaf(g[j], g[j], acc);
  acc = wave64_sum(acc);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) partials[chunk0 + c] = ((red[0] + red[1]) + red[2]) + red[3];
}

// One workgroup: lane t sums partials t, t + 256, ... in double, the 256 sums meet in a fixed tree.
// out[0] = total_norm, out[1] = min(1, max_norm / (total_norm + 1e-6)); a NaN norm gives a NaN coefficient
// (torch.clamp keeps NaN, fminf would not).
__global__ __launch_bounds__(kThreads) void grad_clip_coef_kernel(const float *__restrict__ partials, const int64_t n,
                                                                  const float max_norm, float *__restrict__ out) {
  __shared__ double red[kThreads];
  const int tid = (int)threadIdx.x;
  double acc = 0.0;
  for (int64_t j = tid; j < n; j += kThreads) acc += (double)partials[j];
  red[tid] = acc;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    const float norm = (float)sqrt(red[0]);
    const float c = max_norm / (norm + 1e-6f);
    out[0] = norm;
    out[1] = c > 1.0f ? 1.0f : c;
  }
}

bool aligned4(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 3) == 0; }

// argument checks shared by the entry points; `full`: the Adam step needs p, m, v and the group as well
int check_table(const isi_adam_tensor *tensors, int n_tensors, int n_groups, bool full, const char *who) {
  char buf[160];
  if (n_tensors < 0 || (n_tensors && !tensors)) { snprintf(buf, sizeof buf, "%s: null tensor table", who); return invalid(buf); }
  for (int i = 0; i < n_tensors; ++i) {
    const isi_adam_tensor &t = tensors[i];
    if (!t.g || (full && (!t.p || !t.m || !t.v))) { snprintf(buf, sizeof buf, "%s: null pointer in entry %d", who, i); return invalid(buf); }
    if (t.n <= 0) { snprintf(buf, sizeof buf, "%s: entry %d has no elements", who, i); return invalid(buf); }
    if (!aligned4(t.g) || (full && (!aligned4(t.p) || !aligned4(t.m) || !aligned4(t.v)))) {
      snprintf(buf, sizeof buf, "%s: entry %d is not aligned to a float", who, i);
      return invalid(buf);
    }
    if (full && (t.group < 0 || t.group >= n_groups)) { snprintf(buf, sizeof buf, "%s: entry %d names param group %d of %d", who, i, t.group, n_groups); return invalid(buf); }
    if (chunks_of(t.n) > (int64_t)1 << 24) { snprintf(buf, sizeof buf, "%s: entry %d is beyond 2^35 elements", who, i); return unsupported(buf); }
  }
  return ISI_OK;
}

// fills the pack for entries [i0, i0 + m); returns its chunk count
int fill_pack(AdamPack &pack, const isi_adam_tensor *tensors, int i0, int m) {
  memset(&pack, 0, sizeof pack);
  int chunks = 0;
  for (int i = 0; i < m; ++i) {
    pack.t[i] = tensors[i0 + i];
    chunks += (int)chunks_of(tensors[i0 + i].n);
    pack.chunk_end[i] = chunks;
  }
  for (int i = m; i < kTensorsPerLaunch; ++i) pack.chunk_end[i] = chunks;
  pack.n = m;
  return chunks;
}

}  // namespace

int64_t adam_num_chunks(const isi_adam_tensor *tensors, int n_tensors) {
  if (n_tensors < 0 || (n_tensors && !tensors)) return 0;
  int64_t total = 0;
  for (int i = 0; i < n_tensors; ++i) total += tensors[i].n > 0 ? chunks_of(tensors[i].n) : 0;
  return total;
}

int grad_sumsq_f32(const isi_adam_tensor *tensors, int n_tensors, float *partials, int64_t n_partials, hipStream_t stream) {
  if (const int rc = check_table(tensors, n_tensors, 0, false, "grad_sumsq")) return rc;
  if (n_tensors == 0) return invalid("grad_sumsq: empty tensor table");
  if (!partials) return invalid("grad_sumsq: null partials");
  if (n_partials != adam_num_chunks(tensors, n_tensors)) return invalid("grad_sumsq: n_partials is not isi_adam_num_chunks of the table");
  int64_t chunk0 = 0;
  for (int i0 = 0; i0 < n_tensors; i0 += kTensorsPerLaunch) {
    AdamPack pack;
    const int chunks = fill_pack(pack, tensors, i0, std::min(kTensorsPerLaunch, n_tensors - i0));
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)chunks), dim3(kThreads), 0, stream, pack, partials, chunk0);
    if (const int rc = check_launch("grad_sumsq")) return rc;
    chunk0 += chunks;
  }
  return ISI_OK;
}

int grad_clip_coef_f32(const float *partials, int64_t n_partials, float max_norm, float *norm_coef, hipStream_t stream) {
  if (!partials || !norm_coef) return invalid("grad_clip_coef: null pointer");
  if (n_partials <= 0) return invalid("grad_clip_coef: no partials");
  if (!(max_norm > 0.0f)) return invalid("grad_clip_coef: max_norm must be positive");
  hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(kThreads), 0, stream, partials, n_partials, max_norm, norm_coef);
  return check_launch("grad_clip_coef");
}

int adam_step_f32(const isi_adam_tensor *tensors, int n_tensors, const isi_adam_hyper *hyper, int n_groups, const float *coef,
                  hipStream_t stream) {
  if (n_groups <= 0) return invalid("adam_step: no param groups");
  if (!hyper) return invalid("adam_step: null hyper-parameter block");
  if (const int rc = check_table(tensors, n_tensors, n_groups, true, "adam_step")) return rc;
  for (int i0 = 0; i0 < n_tensors; i0 += kTensorsPerLaunch) {
    AdamPack pack;
    const int chunks = fill_pack(pack, tensors, i0, std::min(kTensorsPerLaunch, n_tensors - i0));
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)chunks), dim3(kThreads), 0, stream, pack, hyper, coef);
    if (const int rc = check_launch("adam_step")) return rc;
  }
  return ISI_OK;
}

}  // namespace isi
