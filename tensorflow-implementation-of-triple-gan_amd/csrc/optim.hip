// Multi-tensor Adam (TF form), momentum SGD, RMSProp and EMA over a network's FLAT parameter buffer: one launch per network,
// Adam 28 B/param (read p,g,m,v; write p,m,v), momentum 20 B/param, RMSProp 28 B/param — HBM-bound, 16-B lanes, grid-stride.
// Hyper-parameters that change between iterations (learning rate, step count) live in device memory so that
// a captured hipGraph replays with fresh values.
//   tf.train.AdamOptimizer (Training/train_base.py:91-97) in its ApplyAdam functor form: alpha = lr*sqrt(1-b2^t)/(1-b1^t);
//   m += (g-m)(1-b1); v += (g^2-v)(1-b2); p -= m*alpha/(sqrt(v)+eps)              [UNVERIFIED-TF]
//   tf.train.MomentumOptimizer(lr, momentum), use_nesterov=False (Training/train_base.py:86-89), slot `momentum` zero-initialised:
//   accum = accum*momentum + g; p -= lr*accum                                      [UNVERIFIED-TF]
//   tf.train.RMSPropOptimizer(lr, decay=0.9, momentum=0, epsilon=1e-10, centered=False) (Training/train_base.py:99-105), slot `rms`
//   initialised to ONES, slot `momentum` to zeros: ms += (g^2-ms)(1-decay); mom = mom*momentum + (g*lr)/sqrt(ms+eps); p -= mom
//   (epsilon INSIDE the root)                                                      [UNVERIFIED-TF]
//   Neither keeps a step count.  Every operation is written in the order above so that each is one fp32 rounding (-ffp-contract=off).
//   tf.train.ExponentialMovingAverage(0.9999).apply (Training/Train_goodGAN.py:101-103): s -= (1-d)(s-p)
//   tf.clip_by_global_norm(grads, clip) over a network's flat gradient buffer (config.CLIP_NORM)    [UNVERIFIED-TF]:
//   norm = grad_scale*sqrt(sum g^2), factor = clip*min(1/norm, 1/clip) (NaN for a non-finite norm), both in fp64 and rounded to fp32 once
//   (tg_grad_norm_clip_f32: fixed-shape fp64 reduction in two launches, no atomics, grid sized from n alone => bit-reproducible); the
//   *_clip_* optimisers are the same kernel bodies with g_used = (g*grad_scale)*factor, factor read from the device.
#include "tg_common.h"

namespace {

__global__ void step_inc(int* t) { if (threadIdx.x == 0 && blockIdx.x == 0) t[0] += 1; }

// (the bodies take the loop's start and step as arguments: read inside an inlined __device__ function, blockDim / gridDim compile to the
// general form for non-uniform workgroups instead of the kernels' own, and the unclipped kernels would stop being the code they were)
#define GRID_I0 ((int64_t)blockIdx.x * blockDim.x + threadIdx.x)
#define GRID_STRIDE ((int64_t)gridDim.x * blockDim.x)

template <bool CLIP>
__device__ __forceinline__ float scaled_grad(float g, float grad_scale, float factor) {
  const float gg = g * grad_scale;
  if (CLIP) return gg * factor;
  return gg;
}

// The optimiser bodies are written once and instantiated twice: CLIP = false is the launch the unclipped entry points always made (the
// `factor` argument is dead there), CLIP = true multiplies the scaled gradient by the device-resident clip factor — one more fp32
// rounding.  i0 / stride are the grid-stride loop's start and step, formed in the kernel itself (GRID_I0 / GRID_STRIDE).
template <bool CLIP>
__device__ __forceinline__ void adam_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                          int64_t n, const float* __restrict__ lr_ptr, float beta1, float beta2, float eps,
                                          const int* __restrict__ t_ptr, float grad_scale, float factor, int64_t i0, int64_t stride) {
  const int t = t_ptr[0];
  const float lr_t = (float)((double)lr_ptr[0] * sqrt(1.0 - pow((double)beta2, (double)t)) / (1.0 - pow((double)beta1, (double)t)));
  const float omb1 = 1.f - beta1, omb2 = 1.f - beta2;
  const int64_t n4 = n / 4;
  for (int64_t i = i0; i < n4; i += stride) {
    float4 pv = reinterpret_cast<float4*>(p)[i], gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
    float* pp = &pv.x; float* gp = &gv.x; float* mp = &mv.x; float* vp = &vv.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gg = scaled_grad<CLIP>(gp[k], grad_scale, factor);
      mp[k] = mp[k] + (gg - mp[k]) * omb1;
      vp[k] = vp[k] + (gg * gg - vp[k]) * omb2;
      pp[k] = pp[k] - mp[k] * lr_t / (sqrtf(vp[k]) + eps);
    }
    reinterpret_cast<float4*>(p)[i] = pv; reinterpret_cast<float4*>(m)[i] = mv; reinterpret_cast<float4*>(v)[i] = vv;
  }
  for (int64_t i = n4 * 4 + i0; i < n; i += stride) {
    const float gg = scaled_grad<CLIP>(g[i], grad_scale, factor);
    const float mm = m[i] + (gg - m[i]) * omb1, vv = v[i] + (gg * gg - v[i]) * omb2;
    m[i] = mm; v[i] = vv;
    p[i] = p[i] - mm * lr_t / (sqrtf(vv) + eps);
  }
}

template <bool CLIP>
__device__ __forceinline__ void momentum_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ accum, int64_t n,
                                              const float* __restrict__ lr_ptr, float momentum, float grad_scale, float factor, int64_t i0, int64_t stride) {
  const float lr = lr_ptr[0];
  const int64_t n4 = n / 4;
  for (int64_t i = i0; i < n4; i += stride) {
    float4 pv = reinterpret_cast<float4*>(p)[i], gv = reinterpret_cast<const float4*>(g)[i], av = reinterpret_cast<float4*>(accum)[i];
    float* pp = &pv.x; float* gp = &gv.x; float* ap = &av.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gg = scaled_grad<CLIP>(gp[k], grad_scale, factor);
      ap[k] = ap[k] * momentum + gg;
      pp[k] = pp[k] - lr * ap[k];
    }
    reinterpret_cast<float4*>(p)[i] = pv; reinterpret_cast<float4*>(accum)[i] = av;
  }
  for (int64_t i = n4 * 4 + i0; i < n; i += stride) {
    const float gg = scaled_grad<CLIP>(g[i], grad_scale, factor);
    const float aa = accum[i] * momentum + gg;
    accum[i] = aa;
    p[i] = p[i] - lr * aa;
  }
}

template <bool CLIP>
__device__ __forceinline__ void rmsprop_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ rms, float* __restrict__ mom,
                                             int64_t n, const float* __restrict__ lr_ptr, float decay, float momentum, float eps,
                                             float grad_scale, float factor, int64_t i0, int64_t stride) {
  const float lr = lr_ptr[0];
  const float omd = 1.f - decay;
  const int64_t n4 = n / 4;
  for (int64_t i = i0; i < n4; i += stride) {
    float4 pv = reinterpret_cast<float4*>(p)[i], gv = reinterpret_cast<const float4*>(g)[i];
    float4 rv = reinterpret_cast<float4*>(rms)[i], mv = reinterpret_cast<float4*>(mom)[i];
    float* pp = &pv.x; float* gp = &gv.x; float* rp = &rv.x; float* mp = &mv.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gg = scaled_grad<CLIP>(gp[k], grad_scale, factor);
      rp[k] = rp[k] + (gg * gg - rp[k]) * omd;
      mp[k] = mp[k] * momentum + (gg * lr) / sqrtf(rp[k] + eps);
      pp[k] = pp[k] - mp[k];
    }
    reinterpret_cast<float4*>(p)[i] = pv; reinterpret_cast<float4*>(rms)[i] = rv; reinterpret_cast<float4*>(mom)[i] = mv;
  }
  for (int64_t i = n4 * 4 + i0; i < n; i += stride) {
    const float gg = scaled_grad<CLIP>(g[i], grad_scale, factor);
    const float rr = rms[i] + (gg * gg - rms[i]) * omd;
    const float mm = mom[i] * momentum + (gg * lr) / sqrtf(rr + eps);
    rms[i] = rr; mom[i] = mm;
    p[i] = p[i] - mm;
  }
}

__global__ void __launch_bounds__(256) adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                   int64_t n, const float* __restrict__ lr_ptr, float beta1, float beta2, float eps,
                                                   const int* __restrict__ t_ptr, float grad_scale) {
  adam_body<false>(p, g, m, v, n, lr_ptr, beta1, beta2, eps, t_ptr, grad_scale, 1.f, GRID_I0, GRID_STRIDE);
}

__global__ void __launch_bounds__(256) adam_clip_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, int64_t n, const float* __restrict__ lr_ptr, float beta1, float beta2,
                                                        float eps, const int* __restrict__ t_ptr, float grad_scale,
                                                        const float* __restrict__ factor_ptr) {
  adam_body<true>(p, g, m, v, n, lr_ptr, beta1, beta2, eps, t_ptr, grad_scale, factor_ptr[0], GRID_I0, GRID_STRIDE);
}

__global__ void __launch_bounds__(256) momentum_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ accum, int64_t n,
                                                       const float* __restrict__ lr_ptr, float momentum, float grad_scale) {
  momentum_body<false>(p, g, accum, n, lr_ptr, momentum, grad_scale, 1.f, GRID_I0, GRID_STRIDE);
}

__global__ void __launch_bounds__(256) momentum_clip_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ accum, int64_t n,
                                                            const float* __restrict__ lr_ptr, float momentum, float grad_scale,
                                                            const float* __restrict__ factor_ptr) {
  momentum_body<true>(p, g, accum, n, lr_ptr, momentum, grad_scale, factor_ptr[0], GRID_I0, GRID_STRIDE);
}

__global__ void __launch_bounds__(256) rmsprop_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ rms, float* __restrict__ mom,
                                                      int64_t n, const float* __restrict__ lr_ptr, float decay, float momentum, float eps,
                                                      float grad_scale) {
  rmsprop_body<false>(p, g, rms, mom, n, lr_ptr, decay, momentum, eps, grad_scale, 1.f, GRID_I0, GRID_STRIDE);
}

__global__ void __launch_bounds__(256) rmsprop_clip_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ rms,
                                                           float* __restrict__ mom, int64_t n, const float* __restrict__ lr_ptr, float decay,
                                                           float momentum, float eps, float grad_scale, const float* __restrict__ factor_ptr) {
  rmsprop_body<true>(p, g, rms, mom, n, lr_ptr, decay, momentum, eps, grad_scale, factor_ptr[0], GRID_I0, GRID_STRIDE);
}

#undef GRID_I0
#undef GRID_STRIDE

// ---- global gradient norm + clip factor (tg_grad_norm_clip_f32) ---------------------------------------------------------------------
// Launch 1: workgroup b squares and sums, in fp64, the 16-byte units b*GN_UNITS + u*256 + tid (u < GN_UNROLL) of every chunk it owns
// (chunks b, b + grid, ...; the grid is a function of n alone), then the scalar tail in workgroup 0; lanes -> wave by a __shfl_down tree
// (32, 16, ..., 1), waves -> workgroup in LDS in wave order; partial[b] goes to the workspace.  Launch 2: one workgroup adds the partials,
// thread t those of index t, t + 256, ... in index order, through the same tree, and thread 0 writes {norm, factor}.  Every addition has a
// fixed place, so two runs agree in every bit on any stream and in any launch order.
constexpr int GN_THREADS = 256, GN_UNROLL = 8, GN_UNITS = GN_THREADS * GN_UNROLL, GN_MAX_BLOCKS = 1024;

__device__ __forceinline__ double gn_block_sum(double acc) {
  __shared__ double wave_sum[GN_THREADS / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < GN_THREADS / 64; ++w) s += wave_sum[w];
  }
  return s;                                                    // valid in thread 0
}

__global__ void __launch_bounds__(GN_THREADS) grad_sumsq_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ partial) {
  const int64_t n4 = n / 4, n_chunks = (n4 + GN_UNITS - 1) / GN_UNITS;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  double acc = 0.0;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    float4 v[GN_UNROLL];
#pragma unroll
    for (int u = 0; u < GN_UNROLL; ++u) {
      const int64_t i = c * GN_UNITS + u * GN_THREADS + threadIdx.x;
      v[u] = i < n4 ? g4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < GN_UNROLL; ++u) {
      acc += (double)v[u].x * (double)v[u].x;
      acc += (double)v[u].y * (double)v[u].y;
      acc += (double)v[u].z * (double)v[u].z;
      acc += (double)v[u].w * (double)v[u].w;
    }
  }
  if (blockIdx.x == 0 && n4 * 4 + threadIdx.x < n) {           // scalar tail: at most three elements
    const double x = (double)g[n4 * 4 + threadIdx.x];
    acc += x * x;
  }
  const double s = gn_block_sum(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void __launch_bounds__(GN_THREADS) grad_norm_final_kernel(const double* __restrict__ partial, int blocks, float grad_scale,
                                                                     const float* __restrict__ clip_ptr, float* __restrict__ out2) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < blocks; i += GN_THREADS) acc += partial[i];
  const double s = gn_block_sum(acc);
  if (threadIdx.x == 0) {
    const double norm = (double)grad_scale * sqrt(s), clip = (double)clip_ptr[0];
    const double inv = fmin(1.0 / norm, 1.0 / clip);
    out2[0] = (float)norm;
    out2[1] = isfinite(norm) ? (float)(clip * inv) : __builtin_nanf("");   // TensorFlow: a non-finite norm poisons every gradient
  }
}

int gn_blocks(int64_t n) {
  const int64_t chunks = (n / 4 + GN_UNITS - 1) / GN_UNITS;
  return (int)(chunks < 1 ? 1 : (chunks > GN_MAX_BLOCKS ? GN_MAX_BLOCKS : chunks));
}

__global__ void __launch_bounds__(256) ema_kernel(float* __restrict__ s, const float* __restrict__ p, int64_t n, float one_minus_decay) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    s[i] = s[i] - one_minus_decay * (s[i] - p[i]);
}

int ew_grid(int64_t work) {
  int64_t b = (work + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

}  // namespace

extern "C" {

int tg_adam_f32(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_dev, float beta1, float beta2, float eps, int* step_dev,
                float grad_scale, void* stream) {
  TG_REQUIRE(p && g && m && v && lr_dev && step_dev && n > 0, "adam: bad args");
  TG_REQUIRE(((uintptr_t)p % 16 == 0) && ((uintptr_t)g % 16 == 0) && ((uintptr_t)m % 16 == 0) && ((uintptr_t)v % 16 == 0), "adam: buffers must be 16-B aligned");
  hipStream_t s = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_OPTIM, 0, 28.0 * n, s);
  hipLaunchKernelGGL(step_inc, dim3(1), dim3(64), 0, s, step_dev);
  TG_CHECK_LAUNCH("step_inc");
  hipLaunchKernelGGL(adam_kernel, dim3(ew_grid(n / 4 + 1)), dim3(256), 0, s, p, g, m, v, n, lr_dev, beta1, beta2, eps, step_dev, grad_scale);
  TG_CHECK_LAUNCH("adam_kernel");
  return TG_OK;
}

int tg_momentum_f32(float* p, const float* g, float* accum, int64_t n, const float* lr_dev, float momentum, float grad_scale, void* stream) {
  TG_REQUIRE(p && g && accum && lr_dev && n > 0, "momentum: bad args");
  TG_REQUIRE(((uintptr_t)p % 16 == 0) && ((uintptr_t)g % 16 == 0) && ((uintptr_t)accum % 16 == 0), "momentum: buffers must be 16-B aligned");
  hipStream_t s = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_OPTIM, 0, 20.0 * n, s);
  hipLaunchKernelGGL(momentum_kernel, dim3(ew_grid(n / 4 + 1)), dim3(256), 0, s, p, g, accum, n, lr_dev, momentum, grad_scale);
  TG_CHECK_LAUNCH("momentum_kernel");
  return TG_OK;
}

int tg_rmsprop_f32(float* p, const float* g, float* rms, float* mom, int64_t n, const float* lr_dev, float decay, float momentum, float eps,
                   float grad_scale, void* stream) {
  TG_REQUIRE(p && g && rms && mom && lr_dev && n > 0, "rmsprop: bad args");
  TG_REQUIRE(((uintptr_t)p % 16 == 0) && ((uintptr_t)g % 16 == 0) && ((uintptr_t)rms % 16 == 0) && ((uintptr_t)mom % 16 == 0),
             "rmsprop: buffers must be 16-B aligned");
  hipStream_t s = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_OPTIM, 0, 28.0 * n, s);
  hipLaunchKernelGGL(rmsprop_kernel, dim3(ew_grid(n / 4 + 1)), dim3(256), 0, s, p, g, rms, mom, n, lr_dev, decay, momentum, eps, grad_scale);
  TG_CHECK_LAUNCH("rmsprop_kernel");
  return TG_OK;
}

int tg_adam_clip_f32(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_dev, float beta1, float beta2, float eps,
                     int* step_dev, float grad_scale, const float* factor_dev, void* stream) {
  TG_REQUIRE(p && g && m && v && lr_dev && step_dev && factor_dev && n > 0, "adam_clip: bad args");
  TG_REQUIRE(((uintptr_t)p % 16 == 0) && ((uintptr_t)g % 16 == 0) && ((uintptr_t)m % 16 == 0) && ((uintptr_t)v % 16 == 0),
             "adam_clip: buffers must be 16-B aligned");
  hipStream_t s = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_OPTIM, 0, 28.0 * n, s);
  hipLaunchKernelGGL(step_inc, dim3(1), dim3(64), 0, s, step_dev);
  TG_CHECK_LAUNCH("step_inc");
  hipLaunchKernelGGL(adam_clip_kernel, dim3(ew_grid(n / 4 + 1)), dim3(256), 0, s, p, g, m, v, n, lr_dev, beta1, beta2, eps, step_dev, grad_scale,
                     factor_dev);
  TG_CHECK_LAUNCH("adam_clip_kernel");
  return TG_OK;
}

int tg_momentum_clip_f32(float* p, const float* g, float* accum, int64_t n, const float* lr_dev, float momentum, float grad_scale,
                         const float* factor_dev, void* stream) {
  TG_REQUIRE(p && g && accum && lr_dev && factor_dev && n > 0, "momentum_clip: bad args");
  TG_REQUIRE(((uintptr_t)p % 16 == 0) && ((uintptr_t)g % 16 == 0) && ((uintptr_t)accum % 16 == 0), "momentum_clip: buffers must be 16-B aligned");
  hipStream_t s = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_OPTIM, 0, 20.0 * n, s);
  hipLaunchKernelGGL(momentum_clip_kernel, dim3(ew_grid(n / 4 + 1)), dim3(256), 0, s, p, g, accum, n, lr_dev, momentum, grad_scale, factor_dev);
  TG_CHECK_LAUNCH("momentum_clip_kernel");
  return TG_OK;
}

int tg_rmsprop_clip_f32(float* p, const float* g, float* rms, float* mom, int64_t n, const float* lr_dev, float decay, float momentum, float eps,
                        float grad_scale, const float* factor_dev, void* stream) {
  TG_REQUIRE(p && g && rms && mom && lr_dev && factor_dev && n > 0, "rmsprop_clip: bad args");
  TG_REQUIRE(((uintptr_t)p % 16 == 0) && ((uintptr_t)g % 16 == 0) && ((uintptr_t)rms % 16 == 0) && ((uintptr_t)mom % 16 == 0),
             "rmsprop_clip: buffers must be 16-B aligned");
  hipStream_t s = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_OPTIM, 0, 28.0 * n, s);
  hipLaunchKernelGGL(rmsprop_clip_kernel, dim3(ew_grid(n / 4 + 1)), dim3(256), 0, s, p, g, rms, mom, n, lr_dev, decay, momentum, eps, grad_scale,
                     factor_dev);
  TG_CHECK_LAUNCH("rmsprop_clip_kernel");
  return TG_OK;
}

int64_t tg_grad_norm_workspace_bytes(int64_t n) {
  if (n <= 0) { tg::set_error("grad_norm_workspace_bytes: n must be positive"); return -1; }
  return (int64_t)gn_blocks(n) * (int64_t)sizeof(double);
}

int tg_grad_norm_clip_f32(const float* g, int64_t n, float grad_scale, const float* clip_dev, float* out2, void* workspace, int64_t workspace_bytes,
                          void* stream) {
  TG_REQUIRE(g && clip_dev && out2 && workspace && n > 0, "grad_norm_clip: bad args");
  TG_REQUIRE(((uintptr_t)g % 16 == 0) && ((uintptr_t)workspace % 16 == 0), "grad_norm_clip: gradient and workspace must be 16-B aligned");
  const int blocks = gn_blocks(n);
  TG_REQUIRE(workspace_bytes >= (int64_t)blocks * (int64_t)sizeof(double), "grad_norm_clip: workspace smaller than tg_grad_norm_workspace_bytes(n)");
  hipStream_t s = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_OPTIM, 0, 4.0 * n, s);
  double* partial = static_cast<double*>(workspace);
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(GN_THREADS), 0, s, g, n, partial);
  TG_CHECK_LAUNCH("grad_sumsq_kernel");
  hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(GN_THREADS), 0, s, partial, blocks, grad_scale, clip_dev, out2);
  TG_CHECK_LAUNCH("grad_norm_final_kernel");
  return TG_OK;
}

int tg_ema_f32(float* shadow, const float* p, int64_t n, float decay, void* stream) {
  TG_REQUIRE(shadow && p && n > 0, "ema: bad args");
  hipStream_t s = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_OPTIM, 0, 12.0 * n, s);
  hipLaunchKernelGGL(ema_kernel, dim3(ew_grid(n)), dim3(256), 0, s, shadow, p, n, 1.f - decay);
  TG_CHECK_LAUNCH("ema_kernel");
  return TG_OK;
}

}  // extern "C"
