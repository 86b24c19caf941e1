// Device-side helpers shared by the MFMA kernels (igemm_kernel.h, wgrad_kernel.h, conv3x3_bf16.hip, wgrad3x3.hip): one copy of each.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

namespace tgm {

// byte offset beyond any (< 2 GiB) tensor: through a buffer descriptor, loads at it return 0 and stores are dropped (no branch, no select)
constexpr uint32_t OOB_OFF = 0x80000000u;

constexpr int BK = 32;    // reduction depth per LDS tile of the generic kernels (igemm_kernel.h, wgrad_kernel.h)

// XCD-aware bijective remap (8 XCDs, blocks b and b+8 share one): every XCD works on a contiguous run of logical tiles,
// so the n-tiles that re-read one A tile and neighbouring m-tiles (shared halo rows) hit the same L2.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, x = bid & 7;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}

// 2 fp32 -> 2 bf16 (RNE): one v_cvt_pk_bf16_f32
__device__ __forceinline__ uint32_t pack2(uint32_t a, uint32_t b) {
  const f32x2 f = {__builtin_bit_cast(float, a), __builtin_bit_cast(float, b)};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, bf16x2));
}

// 4 fp32 -> 4 bf16 (RNE), 8 bytes, channel order kept
__device__ __forceinline__ u32x2 pack4(u32x4 v) {
  u32x2 r;
  r.x = pack2(v.x, v.y);
  r.y = pack2(v.z, v.w);
  return r;
}

// s_waitcnt vmcnt(N) lgkmcnt(0) + s_barrier: the N youngest vector-memory operations of this wave stay in flight across the barrier
template <int N>
__device__ __forceinline__ void barrier_keep() { asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory"); }

// LDS byte offset of 16-B chunk `ch` of row `row` in an image of 256-byte rows (128 bf16): the chunk index is XOR-swizzled by
// ((row & 3) << 2) | ((row >> 2) & 3), so that row stores and the transposing ds_read_b64_tr_b16 are both bank-conflict free.
__device__ __forceinline__ int swz256(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

// four floats as one 16-byte store through a buffer descriptor (an OOB_OFF offset drops it)
__device__ __forceinline__ void store4(float a, float b, float c, float d, __amdgpu_buffer_rsrc_t rsrc, uint32_t off) {
  const u32x4 pk = {__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b), __builtin_bit_cast(uint32_t, c), __builtin_bit_cast(uint32_t, d)};
  __builtin_amdgcn_raw_buffer_store_b128(pk, rsrc, off, 0, 0);
}

}  // namespace tgm
