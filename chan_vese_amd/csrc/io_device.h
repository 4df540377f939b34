// io_device.h — what the member-table kernels that move uint8 planes share (io_kernels.hip, pyramid_kernels.hip): the global address
// space, 16-byte pieces at any byte address, the member search, and the exact plane sums of the ingest.
#pragma once
#include "cvh_internal.h"

namespace {

// The table hands the kernels generic pointers; everything they point at is global memory (device, managed or mapped host memory: checked
// by the host), so the kernels address it in the global address space -- global_load / global_store, not flat operations, which would also
// count against LDS.
#define CVH_GLOBAL __attribute__((address_space(1)))
typedef CVH_GLOBAL const uint8_t *gbytes_in;
typedef CVH_GLOBAL uint8_t *gbytes_out;

// 16 bytes at ANY byte address (a caller's tensor view): the code object runs in unaligned-access mode, where one global dwordx4
// instruction takes them; the context's own buffers are addressed as uint4 (16-byte aligned by construction)
typedef unsigned v4u __attribute__((ext_vector_type(4)));   // (compiler vector types: a class type cannot live in an address space)
typedef v4u v4u_any __attribute__((aligned(1)));
typedef double v2d __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint4 load16_any(gbytes_in p)
{
  const v4u v = *(CVH_GLOBAL const v4u_any *)p;
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void store16_any(gbytes_out p, uint4 v)
{
  const v4u o = {v.x, v.y, v.z, v.w};
  *(CVH_GLOBAL v4u_any *)p = o;
}
__device__ __forceinline__ uint4 load16(gbytes_in p, size_t q)    // piece q of a 16-byte aligned buffer
{
  const v4u v = ((CVH_GLOBAL const v4u *)p)[q];
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void store16(gbytes_out p, size_t q, uint4 v)
{
  const v4u o = {v.x, v.y, v.z, v.w};
  ((CVH_GLOBAL v4u *)p)[q] = o;
}

// the member whose section holds this workgroup (first is ascending, tab[0].first == 0): wave-uniform
__device__ __forceinline__ int io_member(const CvhIoMember *tab, int nmem)
{
  int lo = 0, hi = nmem - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].first <= blockIdx.x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// sum p and sum p^2 of a plane: a lane adds its bytes into 32-bit s1 / s2 (add_bytes) and moves them into the 64-bit pair acc[0 .. 1]
// every kFlushPieces pieces of 16 bytes -- 256 * 16 * 65025 < 2^32 -- and behind its last byte (flush)
constexpr int kFlushPieces = 256;

__device__ __forceinline__ void add_bytes(const uint4 v, unsigned &s1, unsigned &s2)
{
  const unsigned wds[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int b = 0; b < 4; ++b) { const unsigned x = (wds[i] >> (8 * b)) & 0xffu; s1 += x; s2 += x * x; }
  }
}

__device__ __forceinline__ void flush(unsigned long long *acc, unsigned &s1, unsigned &s2)
{
  acc[0] += s1; acc[1] += s2; s1 = s2 = 0;
}

// the lanes' acc[0 .. 2C-1] of a workgroup of CVH_BLOCK are added to out[0 .. 2C-1]: wave reduction, LDS, ONE 64-bit atomic per sum
// (exact integers: the result does not depend on the grid or the order)
__device__ __forceinline__ void add_sums(const unsigned long long acc[6], int C, unsigned long long *out)
{
  __shared__ unsigned long long sh[4][6];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    unsigned long long v = acc[s];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) sh[wave][s] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < 2 * C) atomicAdd(&out[threadIdx.x], sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x]);
}

}  // namespace
