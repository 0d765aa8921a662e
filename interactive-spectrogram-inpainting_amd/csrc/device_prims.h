// Device primitives the MFMA kernels rest on, each defined ONCE: buffer loads, buffer descriptors, the LDS-DMA, the
// 32x32 accumulator layout and the swizzle of the bf16 LDS planes -- and the two row stages (table-fed, rows-fed) the
// code-database searches share.  All of them are __forceinline__: a kernel's machine code does not depend on where they are written
// down.  Helpers with a single user stay in that user's file.
#pragma once
#ifndef __HIPCC__
#error "device_prims.h holds device code: include it from sources compiled by hipcc only"
#endif
#include <hip/hip_runtime.h>

namespace isi {

typedef float f32x16 __attribute__((ext_vector_type(16)));   // the accumulator of a 32x32 MFMA
typedef int i32x4 __attribute__((ext_vector_type(4)));       // 16 bytes of a buffer load; a buffer descriptor

// 16 bytes at rsrc.base + byte_off (per lane) + uniform_off (scalar); zeros beyond the descriptor's num_records
__device__ __forceinline__ float4 buf_load4(__amdgpu_buffer_rsrc_t rsrc, unsigned byte_off, unsigned uniform_off = 0) {
  i32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, byte_off, uniform_off, 0);
  return *reinterpret_cast<float4 *>(&v);
}
// component e of v with e known at compile time after unrolling (an indexed float4 would go through scratch)
__device__ __forceinline__ float elem(const float4 &v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
// row of a 32x32 accumulator tile that register r of a lane in half-wave `half` holds
__device__ __forceinline__ int mfma_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }
// element offset of 16-byte slot `slot` in a 64-byte row of a bf16 LDS plane: the four slots of a row are XOR-swizzled
// with (row >> 2) & 3 (conflict-free ds_read_b128 lane groups and ds_write_b64 groups, see conv_igemm_f32.hip)
__device__ __forceinline__ int bf_slot(int row, int slot) { return (slot ^ ((row >> 2) & 3)) * 8; }

// raw buffer descriptor over [ptr, ptr + bytes) as the four dwords inline assembly takes in SGPRs
__device__ __forceinline__ i32x4 make_rsrc(const void *ptr, const unsigned bytes) {
  const unsigned long long b = (unsigned long long)ptr;
  return i32x4{(int)(unsigned)b, (int)((unsigned)(b >> 32) & 0xffffu), (int)bytes, 0x00020000};
}

// one LDS-DMA (`buffer_load_dwordx4 ... lds`): lane l's 16 bytes at rsrc.base + voff + soff land at lds_addr + 16 l,
// with no staging registers.  Out of range the DMA writes zeros, and the range check looks at voff alone -- soff is not
// part of it (established with tools/probes/lds_dma_probe.hip): the callers' zero padding is an out-of-range voff.
// M0 CONTRACT: M0 carries the wave-uniform LDS address; it is written here, for every piece, and never restored.  A
// kernel that calls this must not use M0 for anything else (none of the callers does: no other m0 in their generated
// code).  rel_attention_fwd3.hip has the form that keeps M0 fixed over many pieces and tells them apart by the
// instruction's immediate offset.
__device__ __forceinline__ void dma16(const unsigned lds_addr, const unsigned voff, const i32x4 rsrc, const unsigned soff) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
               :: "s"(lds_addr), "v"(voff), "s"(rsrc), "s"(soff) : "memory");
}

// The stage of the code-database searches (code_search.hip, code_shift_search.hip): the weighted table rows of the `ncell`
// query cells from c0 on, rows[cl][k] = w[c0 + cl] * T[query[c0 + cl]][k] (one rounding; zeros for a cell >= K, the priors'
// mask token), written by a workgroup of THREADS threads.  Wave w takes the cells w, w + THREADS / 64, ...: the row index
// and the weight are wave-uniform.  wj may be null (weight 1); vec_table: K % 4 == 0 and a 16-byte-aligned table.
template <int THREADS>
__device__ __forceinline__ void stage_code_rows(float *rows, const uint16_t *__restrict__ qj, const float *__restrict__ wj,
                                                const float *__restrict__ table, int c0, int ncell, int K, int vec_table) {
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  for (int cl = wave; cl < ncell; cl += THREADS / 64) {
    const unsigned r = qj[c0 + cl];
    const bool live = r < (unsigned)K;
    const float wv = wj ? wj[c0 + cl] : 1.f;
    const float *__restrict__ src = table + (size_t)(live ? r : 0u) * K;
    float *dst = rows + cl * K;
    if (vec_table) {
      for (int k4 = lane; k4 < (K >> 2); k4 += 64) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) {
          t = reinterpret_cast<const float4 *>(src)[k4];
          t.x *= wv; t.y *= wv; t.z *= wv; t.w *= wv;
        }
        reinterpret_cast<float4 *>(dst)[k4] = t;
      }
    } else {
      for (int k = lane; k < K; k += 64) dst[k] = live ? src[k] * wv : 0.f;
    }
  }
}

// The same stage fed with per-cell rows instead of table rows (the searches by encoder vectors): query j's rows R[j][c][:]
// lie at R + (j * cells + c) * K (a size_t offset: Q * cells * K floats pass 2^31), rows[cl][k] = w[c0 + cl] * R[j][c0 + cl][k],
// one rounding.  A cell whose weight is exactly 0 -- the vector query's mask -- is written as zeros whatever its row holds
// (0 * NaN would not be 0); nothing of its row is read.  wj may be null (weight 1); vec_rows: K % 4 == 0 and a
// 16-byte-aligned R, so every row is.
template <int THREADS>
__device__ __forceinline__ void stage_query_rows(float *rows, const float *__restrict__ R, const float *__restrict__ wj, int j,
                                                 int cells, int c0, int ncell, int K, int vec_rows) {
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  for (int cl = wave; cl < ncell; cl += THREADS / 64) {
    const float wv = wj ? wj[c0 + cl] : 1.f;
    const bool live = wv != 0.f;
    const float *__restrict__ src = R + ((size_t)j * (size_t)cells + (size_t)(c0 + cl)) * (size_t)K;
    float *dst = rows + cl * K;
    if (vec_rows) {
      for (int k4 = lane; k4 < (K >> 2); k4 += 64) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) {
          t = reinterpret_cast<const float4 *>(src)[k4];
          t.x *= wv; t.y *= wv; t.z *= wv; t.w *= wv;
        }
        reinterpret_cast<float4 *>(dst)[k4] = t;
      }
    } else {
      for (int k = lane; k < K; k += 64) dst[k] = live ? src[k] * wv : 0.f;
    }
  }
}

}  // namespace isi
