// WGAN-GP loss of Train_base (Training/train_base.py:576-620): the interpolation of _gradient_penalty, the penalty on the input
// gradient of the discriminator, and the WGAN loss head.  The sweeps through the discriminator (forward, input gradient, tangent
// forward, filter gradients) run on the implicit-GEMM launches; these are the arithmetic around them.  Reductions are deterministic:
// fixed per-thread orders, fixed block trees, and the block partials of the penalty summed by one workgroup in index order.
#include "tg_common.h"
#include "tg_device.h"

namespace {

constexpr int BLK = 256;

// out[i,p,k] = real[i,p,k] + alpha[i]*(fake[i,p,k] - real[i,p,k]) for k < c, 0 for c <= k < ld_out
__global__ void __launch_bounds__(BLK) wgan_interp(const float* __restrict__ real, int ld_r, const float* __restrict__ fake, int ld_f,
                                                   const float* __restrict__ alpha, float* __restrict__ out, int ld_out, int n, int hw, int c) {
  const int64_t total = (int64_t)n * hw * ld_out;
  for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < total; i += (int64_t)gridDim.x * BLK) {
    const int64_t row = i / ld_out;
    const int k = (int)(i - row * ld_out);
    float v = 0.f;
    if (k < c) {
      const float a = real[row * ld_r + k], b = fake[row * ld_f + k];
      v = a + alpha[row / hw] * (b - a);
    }
    out[i] = v;
  }
}

__device__ double block_sum_d(double v, double* red) {   // BLK threads = 4 waves, fixed order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// One thread per column (i, x, k) of the padded [n, w, ld_r] index: s = sqrt(sum_y g[i,y,x,k]^2) (the reference's reduce_sum over
// axis 1 of an NHWC tensor, i.e. over H), r[i,y,x,k] = weight * 2 (s - 1) / s * g / (n w c); padding columns k >= c get r = 0.
// partials[block] = sum over the block's columns of (s - 1)^2 in double.
__global__ void __launch_bounds__(BLK) gp_columns(const float* __restrict__ g, int ld_g, int n, int h, int w, int c, float weight, float* __restrict__ r,
                                                  int ld_r, double* __restrict__ partials) {
  __shared__ double red[4];
  const int64_t cols = (int64_t)n * w * ld_r;
  const int64_t q = (int64_t)blockIdx.x * BLK + threadIdx.x;
  double part = 0.0;
  if (q < cols) {
    const int64_t ix = q / ld_r;                       // i * w + x
    const int k = (int)(q - ix * ld_r);
    const int64_t i = ix / w, x = ix - i * w;
    const int64_t g0 = (i * h * w + x) * ld_g + k, r0 = (i * h * w + x) * ld_r + k;
    const int64_t gs = (int64_t)w * ld_g, rs = (int64_t)w * ld_r;
    if (k < c) {
      float ss = 0.f;
      for (int y = 0; y < h; ++y) {
        const float v = g[g0 + y * gs];
        ss += v * v;
      }
      const float s = sqrtf(ss);
      const float coef = 2.f * (s - 1.f) / s * (weight / (float)((int64_t)n * w * c));   // s = 0: non-finite, as TF's sqrt gradient
      for (int y = 0; y < h; ++y) r[r0 + y * rs] = coef * g[g0 + y * gs];
      const double d = (double)s - 1.0;
      part = d * d;
    } else {
      for (int y = 0; y < h; ++y) r[r0 + y * rs] = 0.f;
    }
  }
  part = block_sum_d(part, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = part;
}

__global__ void __launch_bounds__(BLK) gp_finish(const double* __restrict__ partials, int nb, double scale, float* __restrict__ gp) {
  __shared__ double red[4];
  double v = 0.0;
  for (int b = threadIdx.x; b < nb; b += BLK) v += partials[b];
  v = block_sum_d(v, red);
  if (threadIdx.x == 0) gp[0] = (float)(v * scale);
}

// One workgroup per image row of a rank-2 input gradient gx [n, f] (the port's [N, F] image layout, h = w = 1): the reference's axis 1
// is then the feature axis, s_i = sqrt(sum_k gx[i,k]^2), r[i,k] = weight * 2 (s_i - 1) / s_i * gx[i,k] / n, padding columns f..ld_r
// written 0, partials[i] = (s_i - 1)^2 in double.  Loads are coalesced across the row (float4 where the layout allows, V = 4); the
// row's first RB*BLK vectors (RB per thread) stay in registers between the sum and the r write, longer rows re-read the rest.  The sum is
// taken in double in a fixed order (per-thread strides, then block_sum_d): bit-identical run to run.
constexpr int RB = 4;

__device__ __forceinline__ double sq_sum(float v) { return (double)v * v; }
__device__ __forceinline__ double sq_sum(float4 v) { return (((double)v.x * v.x + (double)v.y * v.y) + (double)v.z * v.z) + (double)v.w * v.w; }
__device__ __forceinline__ float scaled(float v, float a) { return v * a; }
__device__ __forceinline__ float4 scaled(float4 v, float a) { return make_float4(v.x * a, v.y * a, v.z * a, v.w * a); }
template <typename T> __device__ __forceinline__ T zero_of();
template <> __device__ __forceinline__ float zero_of<float>() { return 0.f; }
template <> __device__ __forceinline__ float4 zero_of<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }

template <typename T>
__global__ void __launch_bounds__(BLK) gp_rows(const float* __restrict__ g, int ld_g, int f, float weight, int n, float* __restrict__ r, int ld_r,
                                               double* __restrict__ partials) {
  __shared__ double red[4];
  constexpr int V = sizeof(T) / sizeof(float);
  const int64_t i = blockIdx.x;
  const T* __restrict__ gi = reinterpret_cast<const T*>(g + i * ld_g);
  T* __restrict__ ri = reinterpret_cast<T*>(r + i * ld_r);
  const int fv = f / V, lv = ld_r / V;
  T keep[RB];
  double ss = 0.0;
#pragma unroll
  for (int j = 0; j < RB; ++j) {
    const int q = threadIdx.x + j * BLK;
    keep[j] = q < fv ? gi[q] : zero_of<T>();
    ss += sq_sum(keep[j]);
  }
  for (int q = threadIdx.x + RB * BLK; q < fv; q += BLK) ss += sq_sum(gi[q]);
  ss = block_sum_d(ss, red);
  const double s = sqrt(ss);
  const float coef = (float)(2.0 * (s - 1.0) / s * ((double)weight / (double)n));      // s = 0: non-finite, as TF's sqrt gradient
#pragma unroll
  for (int j = 0; j < RB; ++j) {
    const int q = threadIdx.x + j * BLK;
    if (q < lv) ri[q] = q < fv ? scaled(keep[j], coef) : zero_of<T>();
  }
  for (int q = threadIdx.x + RB * BLK; q < lv; q += BLK) ri[q] = q < fv ? scaled(gi[q], coef) : zero_of<T>();
  if (threadIdx.x == 0) partials[i] = (s - 1.0) * (s - 1.0);
}

// ---- R1 (config.R1_GAMMA): the zero-centred penalty on the input gradient at the real rows, per image.
// One workgroup per image i = `rows` rows of c valid floats (row stride ld_g): ss_i = sum of g^2 over all rows * c elements, every square
// taken in double (exact), per-thread strides then block_sum_d: bit-identical run to run.  r = scale * g with scale = (float)(gamma / n),
// one fp32 multiply per element; padding columns c..ld_r of r written 0.  The image is read twice (the sum, then r): nothing is kept in
// registers, so an image of any size goes through one workgroup.  V = 4: rows start 16-byte aligned in g and r, a row is ceil(c / 4)
// float4s whose components at or beyond c count as 0.
template <int V> struct R1Vec;
template <> struct R1Vec<1> {
  static __device__ __forceinline__ float4 load(const float* p) { return make_float4(p[0], 0.f, 0.f, 0.f); }
  static __device__ __forceinline__ float4 first(float4 v, int left) { return v; }
  static __device__ __forceinline__ void store(float* p, float4 v) { p[0] = v.x; }
};
template <> struct R1Vec<4> {
  static __device__ __forceinline__ float4 load(const float* p) { return *reinterpret_cast<const float4*>(p); }
  static __device__ __forceinline__ float4 first(float4 v, int left) {            // the first `left` components, 0 behind them
    return make_float4(left > 0 ? v.x : 0.f, left > 1 ? v.y : 0.f, left > 2 ? v.z : 0.f, left > 3 ? v.w : 0.f);
  }
  static __device__ __forceinline__ void store(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
};

template <int V>
__global__ void __launch_bounds__(BLK) r1_rows(const float* __restrict__ g, int ld_g, int n, int rows, int c, const float* __restrict__ gamma_dev,
                                               float* __restrict__ r, int ld_r, double* __restrict__ partials) {
  __shared__ double red[4];
  using Vec = R1Vec<V>;
  const float* __restrict__ gi = g + (int64_t)blockIdx.x * rows * ld_g;
  float* __restrict__ ri = r + (int64_t)blockIdx.x * rows * ld_r;
  const int cv = (c + V - 1) / V, lv = ld_r / V;                    // vectors of a row that hold valid columns / that r has
  double ss = 0.0;
  for (int q = threadIdx.x; q < rows * cv; q += BLK) {              // (rows * ld < 2^31: the entry point checks)
    const int row = q / cv, k = (q - row * cv) * V;
    ss += sq_sum(Vec::first(Vec::load(gi + (int64_t)row * ld_g + k), c - k));
  }
  ss = block_sum_d(ss, red);
  const float scale = (float)((double)gamma_dev[0] / (double)n);
  for (int q = threadIdx.x; q < rows * lv; q += BLK) {
    const int row = q / lv, k = (q - row * lv) * V;
    float4 v = zero_of<float4>();
    if (k < c) v = Vec::first(scaled(Vec::load(gi + (int64_t)row * ld_g + k), scale), c - k);
    Vec::store(ri + (int64_t)row * ld_r + k, v);
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = ss;
}

// out[0] = gamma / 2 * mean_i ss_i, out[1] = mean_i ss_i: the n partials summed by one workgroup in index order
__global__ void __launch_bounds__(BLK) r1_finish(const double* __restrict__ partials, int n, const float* __restrict__ gamma_dev, float* __restrict__ out) {
  __shared__ double red[4];
  double v = 0.0;
  for (int b = threadIdx.x; b < n; b += BLK) v += partials[b];
  v = block_sum_d(v, red);
  if (threadIdx.x == 0) {
    const double m = v / (double)n;
    out[0] = (float)(0.5 * (double)gamma_dev[0] * m);
    out[1] = (float)m;
  }
}

constexpr int WV = BLK / 64;

// The Wasserstein distances of both loss heads below, written once.  Rows [real | fake | unl] of the discriminator logits (column 0, row
// stride ld): writes dz = d d_loss / dz (column 0, padding 0) and returns, the same in every thread,
//   wd1 = 1/2 (mean real - mean fake), wd2 = 1/2 (mean real - mean unl), wd3 = 1/2 (mean unl - mean fake),
//   d_loss = -(wd1 + l1 wd2 + l2 wd3) and mean fake.
// Every thread sums a fixed strided set of rows, tgd::block_sum adds the waves in index order: bit-identical run to run.
struct Wd { float d_loss, m_fake, wd1, wd2, wd3; };

__device__ Wd wasserstein(const float* __restrict__ z, int ld, int n_real, int n_fake, int n_unl, float l1, float l2, float* __restrict__ dz, int ld_d,
                          float* red) {
  const int n = n_real + n_fake + n_unl;
  float s[3] = {0.f, 0.f, 0.f};
  const float w_real = (-0.5f - 0.5f * l1) / n_real, w_fake = (0.5f + 0.5f * l2) / n_fake, w_unl = (0.5f * l1 - 0.5f * l2) / n_unl;
  for (int r = threadIdx.x; r < n; r += BLK) {
    const float v = z[(int64_t)r * ld];
    const int which = r < n_real ? 0 : (r < n_real + n_fake ? 1 : 2);
    s[which] += v;
    float* o = dz + (int64_t)r * ld_d;
    o[0] = which == 0 ? w_real : (which == 1 ? w_fake : w_unl);
    for (int k = 1; k < ld_d; ++k) o[k] = 0.f;
  }
  const float m_real = tgd::block_sum<WV>(s[0], red) / n_real;
  const float m_fake = tgd::block_sum<WV>(s[1], red) / n_fake;
  const float m_unl = tgd::block_sum<WV>(s[2], red) / n_unl;
  const float wd1 = 0.5f * (m_real - m_fake), wd2 = 0.5f * (m_real - m_unl), wd3 = 0.5f * (m_unl - m_fake);
  return Wd{-(wd1 + l1 * wd2 + l2 * wd3), m_fake, wd1, wd2, wd3};
}

// the stand-alone loss (Train_base._loss_WGAN_GP), lambdas from the host: g_loss = -mean fake, dfake (optional) = d g_loss / d fake logits;
// loss[5] = {d_loss, g_loss, wd1, wd2, wd3}
__global__ void __launch_bounds__(BLK) wgan_loss(const float* __restrict__ z, int ld, int n_real, int n_fake, int n_unl, float l1, float l2,
                                                 float* __restrict__ dz, int ld_d, float* __restrict__ dfake, int ld_df, float* __restrict__ loss) {
  __shared__ float red[WV];
  const Wd w = wasserstein(z, ld, n_real, n_fake, n_unl, l1, l2, dz, ld_d, red);
  if (dfake)
    for (int r = threadIdx.x; r < n_fake; r += BLK) {
      float* f = dfake + (int64_t)r * ld_df;
      f[0] = -1.f / n_fake;
      for (int k = 1; k < ld_df; ++k) f[k] = 0.f;
    }
  if (threadIdx.x == 0) {
    loss[0] = w.d_loss;
    loss[1] = -w.m_fake;
    loss[2] = w.wd1;
    loss[3] = w.wd2;
    loss[4] = w.wd3;
  }
}

// ---- loss heads of the three-player step (Training/Train_goodGAN.py with config.LOSS = 'WGAN_GP').  Unlike wgan_loss they read lambda_1 /
// lambda_2 from device memory (the trainer's hyper[2:4]) and the weighted penalty from the device scalar the sweeps wrote, so a recorded
// launch plan or graph follows set_hyper().  One workgroup each, fixed summation order: bit-identical run to run.

// rows [real | fake | unl]: dz = d d_loss / dz (column 0, padding 0), loss[0] = -(wd1 + l1 wd2 + l2 wd3) + gp_w[0],
// terms[4] = {wd1, wd2, wd3, gp_w[0] / gp_weight}
__global__ void __launch_bounds__(BLK) wgan_d_head(const float* __restrict__ z, int ld, int n_real, int n_fake, int n_unl, const float* __restrict__ lam,
                                                   const float* __restrict__ gp_w, float gp_weight, float* __restrict__ dz, int ld_d,
                                                   float* __restrict__ loss, float* __restrict__ terms) {
  __shared__ float red[WV];
  const Wd w = wasserstein(z, ld, n_real, n_fake, n_unl, lam[0], lam[1], dz, ld_d, red);
  if (threadIdx.x == 0) {
    const float gp = gp_w[0];
    loss[0] = w.d_loss + gp;
    if (terms) {
      terms[0] = w.wd1;
      terms[1] = w.wd2;
      terms[2] = w.wd3;
      terms[3] = gp / gp_weight;
    }
  }
}

// g_loss = -mean z over n rows (column 0): dz = -1/n, padding 0
__global__ void __launch_bounds__(BLK) wgan_g_head(const float* __restrict__ z, int ld, int n, float* __restrict__ dz, int ld_d, float* __restrict__ loss) {
  __shared__ float red[WV];
  float s = 0.f;
  for (int r = threadIdx.x; r < n; r += BLK) {
    s += z[(int64_t)r * ld];
    float* o = dz + (int64_t)r * ld_d;
    o[0] = -1.f / n;
    for (int k = 1; k < ld_d; ++k) o[k] = 0.f;
  }
  const float m = tgd::block_sum<WV>(s, red) / n;
  if (threadIdx.x == 0) loss[0] = -m;
}

// A third way of computing a softmax CE (a run-time loop over the k classes in one thread, expf evaluated again for the gradient): its
// bits differ from softmax_ce of loss.hip, so it does not fold into that file's layout template and stays as it is.
// rows [real | zero (n_zero) | fake] of k logits: c_loss = mean CE(y_real, real) + lam[1] mean CE(y_fake, fake), CE = lse sum_j y_j - y . l;
// dl = w (softmax * sum_j y_j - y) / n on the labelled rows, 0 on the zero rows, padding columns k..ld_d 0; terms[2] = the two means
__global__ void __launch_bounds__(BLK) wgan_c_head(const float* __restrict__ cl, int ld, int n_real, int n_zero, int n_fake, int k,
                                                   const float* __restrict__ y_real, const float* __restrict__ y_fake, const float* __restrict__ lam,
                                                   float* __restrict__ dl, int ld_d, float* __restrict__ loss, float* __restrict__ terms) {
  __shared__ float red[WV];
  const float l2 = n_fake > 0 ? lam[1] : 0.f;
  float ce[2] = {0.f, 0.f};
  for (int pass = 0; pass < 2; ++pass) {
    const int n = pass == 0 ? n_real : n_fake, off = pass == 0 ? 0 : n_real + n_zero;
    const float* y = pass == 0 ? y_real : y_fake;
    const float w = (pass == 0 ? 1.f : l2) / n;
    for (int r = threadIdx.x; r < n; r += BLK) {
      const float* l = cl + (int64_t)(off + r) * ld;
      const float* yr = y + (int64_t)r * k;
      float m = l[0];
      for (int j = 1; j < k; ++j) m = fmaxf(m, l[j]);
      float se = 0.f, ysum = 0.f, yl = 0.f;
      for (int j = 0; j < k; ++j) {
        se += expf(l[j] - m);
        ysum += yr[j];
        yl += yr[j] * l[j];
      }
      const float lse = m + logf(se), inv = 1.f / se;
      ce[pass] += lse * ysum - yl;
      float* o = dl + (int64_t)(off + r) * ld_d;
      for (int j = 0; j < k; ++j) o[j] = w * (expf(l[j] - m) * inv * ysum - yr[j]);
      for (int j = k; j < ld_d; ++j) o[j] = 0.f;
    }
  }
  for (int64_t i = threadIdx.x; i < (int64_t)n_zero * ld_d; i += BLK) dl[(int64_t)n_real * ld_d + i] = 0.f;
  const float t_real = tgd::block_sum<WV>(ce[0], red) / n_real;
  const float t_fake = n_fake > 0 ? tgd::block_sum<WV>(ce[1], red) / n_fake : 0.f;
  if (threadIdx.x == 0) {
    loss[0] = t_real + l2 * t_fake;
    if (terms) {
      terms[0] = t_real;
      terms[1] = t_fake;
    }
  }
}

}  // namespace

extern "C" {

int tg_wgan_interp_f32(const float* real, int ld_r, const float* fake, int ld_f, const float* alpha, float* out, int ld_out, int n, int hw, int c,
                       void* stream) {
  TG_REQUIRE(real && fake && alpha && out && n > 0 && hw > 0 && c > 0 && c <= ld_r && c <= ld_f && c <= ld_out,
             "wgan_interp: bad args (n=%d hw=%d c=%d ld_r=%d ld_f=%d ld_out=%d)", n, hw, c, ld_r, ld_f, ld_out);
  hipStream_t s = tg::as_stream(stream);
  const int64_t total = (int64_t)n * hw * ld_out;
  tg::ProfScope prof(tg::PC_ELEMWISE, 0, 4.0 * (double)n * hw * (2 * c + ld_out), s);
  const int64_t b = (total + BLK - 1) / BLK;
  hipLaunchKernelGGL(wgan_interp, dim3((unsigned)(b > 4096 ? 4096 : b)), dim3(BLK), 0, s, real, ld_r, fake, ld_f, alpha, out, ld_out, n, hw, c);
  TG_CHECK_LAUNCH("wgan_interp");
  return TG_OK;
}

int tg_grad_penalty_f32(const float* gx, int ld_g, int n, int h, int w, int c, float weight, float* r, int ld_r, double* partials, float* gp,
                        void* stream) {
  TG_REQUIRE(gx && r && partials && gp && n > 0 && h > 0 && w > 0 && c > 0 && c <= ld_g && c <= ld_r,
             "grad_penalty: bad args (n=%d h=%d w=%d c=%d ld_g=%d ld_r=%d)", n, h, w, c, ld_g, ld_r);
  const int64_t cols = (int64_t)n * w * ld_r, nb = (cols + BLK - 1) / BLK;
  TG_REQUIRE(nb < (1LL << 31), "grad_penalty: %lld columns", (long long)cols);
  hipStream_t s = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_LOSS, 0, 4.0 * (double)n * h * w * (2 * c + ld_r), s);
  hipLaunchKernelGGL(gp_columns, dim3((unsigned)nb), dim3(BLK), 0, s, gx, ld_g, n, h, w, c, weight, r, ld_r, partials);
  TG_CHECK_LAUNCH("gp_columns");
  hipLaunchKernelGGL(gp_finish, dim3(1), dim3(BLK), 0, s, partials, (int)nb, (double)weight / (double)((int64_t)n * w * c), gp);
  TG_CHECK_LAUNCH("gp_finish");
  return TG_OK;
}

int tg_grad_penalty_rows_f32(const float* gx, int ld_g, int n, int f, float weight, float* r, int ld_r, double* partials, float* gp, void* stream) {
  TG_REQUIRE(gx && r && partials && gp && n > 0 && f > 0 && f <= ld_g && f <= ld_r, "grad_penalty_rows: bad args (n=%d f=%d ld_g=%d ld_r=%d)", n, f,
             ld_g, ld_r);
  hipStream_t s = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_LOSS, 0, 4.0 * (double)n * (f + ld_r), s);
  const bool vec = f % 4 == 0 && ld_g % 4 == 0 && ld_r % 4 == 0 && reinterpret_cast<uintptr_t>(gx) % 16 == 0 && reinterpret_cast<uintptr_t>(r) % 16 == 0;
  if (vec)
    hipLaunchKernelGGL(gp_rows<float4>, dim3((unsigned)n), dim3(BLK), 0, s, gx, ld_g, f, weight, n, r, ld_r, partials);
  else
    hipLaunchKernelGGL(gp_rows<float>, dim3((unsigned)n), dim3(BLK), 0, s, gx, ld_g, f, weight, n, r, ld_r, partials);
  TG_CHECK_LAUNCH("gp_rows");
  hipLaunchKernelGGL(gp_finish, dim3(1), dim3(BLK), 0, s, partials, n, (double)weight / (double)n, gp);
  TG_CHECK_LAUNCH("gp_finish");
  return TG_OK;
}

int tg_r1_penalty_f32(const float* gx, int ld_g, int n, int rows, int c, const float* gamma_dev, float* r, int ld_r, double* partials, float* out,
                      void* stream) {
  TG_REQUIRE(gx && gamma_dev && r && partials && out && n > 0 && n <= (1 << 20) && rows > 0 && c > 0 && c <= ld_g && c <= ld_r,
             "r1_penalty: bad args (n=%d rows=%d c=%d ld_g=%d ld_r=%d)", n, rows, c, ld_g, ld_r);
  TG_REQUIRE((int64_t)rows * c <= (1LL << 21) && (int64_t)rows * ld_g < (1LL << 31) && (int64_t)rows * ld_r < (1LL << 31),
             "r1_penalty: an image of %d rows (c=%d ld_g=%d ld_r=%d) is beyond one workgroup's pass", rows, c, ld_g, ld_r);
  hipStream_t s = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_LOSS, 0, 4.0 * (double)n * rows * (2 * c + ld_r), s);
  const bool vec = ld_g % 4 == 0 && ld_r % 4 == 0 && reinterpret_cast<uintptr_t>(gx) % 16 == 0 && reinterpret_cast<uintptr_t>(r) % 16 == 0;
  if (vec)
    hipLaunchKernelGGL(r1_rows<4>, dim3((unsigned)n), dim3(BLK), 0, s, gx, ld_g, n, rows, c, gamma_dev, r, ld_r, partials);
  else
    hipLaunchKernelGGL(r1_rows<1>, dim3((unsigned)n), dim3(BLK), 0, s, gx, ld_g, n, rows, c, gamma_dev, r, ld_r, partials);
  TG_CHECK_LAUNCH("r1_rows");
  hipLaunchKernelGGL(r1_finish, dim3(1), dim3(BLK), 0, s, partials, n, gamma_dev, out);
  TG_CHECK_LAUNCH("r1_finish");
  return TG_OK;
}

int tg_wgan_loss_f32(const float* logits, int ld, int n_real, int n_fake, int n_unl, float lambda_1, float lambda_2, float* dlogits, int ld_d,
                     float* dfake, int ld_df, float* loss, void* stream) {
  TG_REQUIRE(logits && dlogits && loss && n_real > 0 && n_fake > 0 && n_unl > 0 && ld >= 1 && ld_d >= 1 && (!dfake || ld_df >= 1),
             "wgan_loss: bad args");
  hipStream_t s = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_LOSS, 0, 0, s);
  hipLaunchKernelGGL(wgan_loss, dim3(1), dim3(BLK), 0, s, logits, ld, n_real, n_fake, n_unl, lambda_1, lambda_2, dlogits, ld_d, dfake, ld_df, loss);
  TG_CHECK_LAUNCH("wgan_loss");
  return TG_OK;
}

int tg_wgan_d_head_f32(const float* logits, int ld, int n_real, int n_fake, int n_unl, const float* lambdas, const float* gp_w, float gp_weight,
                       float* dlogits, int ld_d, float* loss, float* terms, void* stream) {
  TG_REQUIRE(logits && lambdas && gp_w && dlogits && loss && n_real > 0 && n_fake > 0 && n_unl > 0 && ld >= 1 && ld_d >= 1 && gp_weight != 0.f,
             "wgan_d_head: bad args (n=%d/%d/%d ld=%d ld_d=%d)", n_real, n_fake, n_unl, ld, ld_d);
  hipStream_t s = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_LOSS, 0, 0, s);
  hipLaunchKernelGGL(wgan_d_head, dim3(1), dim3(BLK), 0, s, logits, ld, n_real, n_fake, n_unl, lambdas, gp_w, gp_weight, dlogits, ld_d, loss, terms);
  TG_CHECK_LAUNCH("wgan_d_head");
  return TG_OK;
}

int tg_wgan_g_head_f32(const float* logits, int ld, int n, float* dlogits, int ld_d, float* loss, void* stream) {
  TG_REQUIRE(logits && dlogits && loss && n > 0 && ld >= 1 && ld_d >= 1, "wgan_g_head: bad args (n=%d ld=%d ld_d=%d)", n, ld, ld_d);
  hipStream_t s = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_LOSS, 0, 0, s);
  hipLaunchKernelGGL(wgan_g_head, dim3(1), dim3(BLK), 0, s, logits, ld, n, dlogits, ld_d, loss);
  TG_CHECK_LAUNCH("wgan_g_head");
  return TG_OK;
}

int tg_wgan_c_head_f32(const float* logits, int ld, int n_real, int n_zero, int n_fake, int k, const float* y_real, const float* y_fake,
                       const float* lambdas, float* dlogits, int ld_d, float* loss, float* terms, void* stream) {
  TG_REQUIRE(logits && y_real && dlogits && loss && n_real > 0 && n_zero >= 0 && n_fake >= 0 && k > 0 && k <= ld && k <= ld_d &&
                 (n_fake == 0 || (y_fake && lambdas)),
             "wgan_c_head: bad args (n=%d/%d/%d k=%d ld=%d ld_d=%d)", n_real, n_zero, n_fake, k, ld, ld_d);
  hipStream_t s = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_LOSS, 0, 0, s);
  hipLaunchKernelGGL(wgan_c_head, dim3(1), dim3(BLK), 0, s, logits, ld, n_real, n_zero, n_fake, k, y_real, y_fake, lambdas, dlogits, ld_d, loss,
                     terms);
  TG_CHECK_LAUNCH("wgan_c_head");
  return TG_OK;
}

}  // extern "C"
