// Device-side helpers shared by the elementwise / norm / rng kernels.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/tg_kernels.h"

namespace tgd {

// The activation with the library exponential (expf): every kernel but the generic conv GEMM.
__device__ __forceinline__ float act(float v, int a, float alpha) {
  switch (a) {
    case TG_ACT_LRELU: return v > 0.f ? v : alpha * v;       // relu(x) - alpha*relu(-x), Good_GAN_cifar10.py:26-27
    case TG_ACT_RELU: return v > 0.f ? v : 0.f;
    case TG_ACT_TANH: return tanhf(v);
    case TG_ACT_SIGMOID: return 1.f / (1.f + expf(-v));
    case TG_ACT_SOFTPLUS: return v > 20.f ? v : log1pf(expf(v));
    default: return v;
  }
}

// The same activation with the hardware exponential (__expf) in sigmoid and softplus: the epilogues of the generic conv GEMM
// (igemm_kernel.h).  The two differ in the last bits of those two activations and stay apart: stored outputs are pinned bit for bit.
__device__ __forceinline__ float act_fast(float v, int a, float alpha) {
  switch (a) {
    case TG_ACT_LRELU: return v > 0.f ? v : alpha * v;
    case TG_ACT_RELU: return v > 0.f ? v : 0.f;
    case TG_ACT_TANH: return tanhf(v);
    case TG_ACT_SIGMOID: return 1.f / (1.f + __expf(-v));
    case TG_ACT_SOFTPLUS: return v > 20.f ? v : log1pf(__expf(v));
    default: return v;
  }
}

// derivative expressed through the activation OUTPUT y (what the forward pass keeps)
__device__ __forceinline__ float act_grad(float y, int a, float alpha) {
  switch (a) {
    case TG_ACT_LRELU: return y > 0.f ? 1.f : alpha;
    case TG_ACT_RELU: return y > 0.f ? 1.f : 0.f;
    case TG_ACT_TANH: return 1.f - y * y;
    case TG_ACT_SIGMOID: return y * (1.f - y);
    case TG_ACT_SOFTPLUS: return 1.f - expf(-y);             // y = log(1+e^x) -> sigmoid(x) = 1 - e^-y
    default: return 1.f;
  }
}

struct u4 { uint32_t x, y, z, w; };

// Philox4x32-10 (Random123): counter (c0..c3), key (k0, k1).  Shared by the step's draws (rng.hip) and the input augmentation
// (elementwise.hip).
__device__ __forceinline__ u4 philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return u4{c0, c1, c2, c3};
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Sum of v over a workgroup of WAVES wavefronts, the same bits in every thread: wave_sum, one LDS slot per wave (red[WAVES]), the waves
// added in index order.  Begins with a barrier, so red may be reused by the next call.
template <int WAVES>
__device__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int i = 1; i < WAVES; ++i) s += red[i];
  return s;
}

}  // namespace tgd
