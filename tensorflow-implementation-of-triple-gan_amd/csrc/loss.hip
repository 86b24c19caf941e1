// Loss heads of Train_base._loss_GAN (Training/train_base.py:113-154) fused per network into ONE
// single-workgroup launch each: value + gradient wrt the logits.  These are latency-bound (<= 250 rows of a few logits); reductions are
// wavefront shuffles + one LDS hop (tgd::block_sum).  The classifier's heads (c_loss, true_fake, softmax_ce, entropy_terms) are each ONE
// body written against a compile-time layout (struct Layout below) and instantiated twice: one thread per row for the reference's ten
// classes, one wave per row for any other 2 <= K <= 1024.  Also the feature-matching and pull-away
// terms of train_base.py:172-182,202-207 (unit parity; not on the Train_goodGAN.py path) and the
// streaming accuracy counter of Train_goodGAN.py:428-447.
#include "tg_common.h"
#include "tg_device.h"

namespace {

__device__ __forceinline__ float bce(float z, float t) { return fmaxf(z, 0.f) - z * t + log1pf(expf(-fabsf(z))); }
__device__ __forceinline__ float sigm(float z) { return 1.f / (1.f + expf(-z)); }

// rows ordered [real | fake | unl]; d_loss = BCE(real,1) + .5 BCE(fake,0) + .5 BCE(unl,0)
__global__ void __launch_bounds__(256) d_loss_kernel(const float* __restrict__ z, int ld, int n_real, int n_fake, int n_unl, float* __restrict__ dz, int ld_d,
                                                     float* __restrict__ loss, float* __restrict__ terms) {
  __shared__ float red[4];
  const int n = n_real + n_fake + n_unl;
  float acc = 0.f, tr[3] = {0.f, 0.f, 0.f};
  for (int r = threadIdx.x; r < n; r += 256) {
    const float v = z[(int64_t)r * ld];
    float t, w;
    int which;
    if (r < n_real) { t = 1.f; w = 1.f / n_real; which = 0; }
    else if (r < n_real + n_fake) { t = 0.f; w = 0.5f / n_fake; which = 1; }
    else { t = 0.f; w = 0.5f / n_unl; which = 2; }
    acc += w * bce(v, t);
    tr[which] += w * bce(v, t);
    float* o = dz + (int64_t)r * ld_d;
    o[0] = w * (sigm(v) - t);
    for (int k = 1; k < ld_d; ++k) o[k] = 0.f;
  }
  acc = tgd::block_sum<4>(acc, red);
  if (threadIdx.x == 0) loss[0] = acc;
  if (terms)                                             // {BCE(real,1), .5 BCE(fake,0), .5 BCE(unl,0)}
    for (int i = 0; i < 3; ++i) {
      const float sum = tgd::block_sum<4>(tr[i], red);
      if (threadIdx.x == 0) terms[i] = sum;
    }
}

// g_loss = 0.5 * BCE(D_fake, 1)
__global__ void __launch_bounds__(256) g_loss_kernel(const float* __restrict__ z, int ld, int n, float* __restrict__ dz, int ld_d, float* __restrict__ loss) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int r = threadIdx.x; r < n; r += 256) {
    const float v = z[(int64_t)r * ld];
    acc += 0.5f / n * bce(v, 1.f);
    float* o = dz + (int64_t)r * ld_d;
    o[0] = 0.5f / n * (sigm(v) - 1.f);
    for (int k = 1; k < ld_d; ++k) o[k] = 0.f;
  }
  acc = tgd::block_sum<4>(acc, red);
  if (threadIdx.x == 0) loss[0] = acc;
}

// ---- the classifier's heads: one body each, two layouts ---------------------------------------------------------------------------------
// Who owns which row and class.  One workgroup of THREADS threads; LANES threads share a row, each holding SLOTS of its classes in
// registers (class j = slot * LANES + lane); the THREADS / LANES row owners stride over the rows.
//   Ten  = <1, 10, 256>     K = 10 (every config of the reference): one thread per row, the row reductions are the identity
//   Wide = <64, 16, 1024>   any other 2 <= K <= 1024: one wave per row, the row reductions are xor butterflies (the same bits in every lane)
// Scalar terms are counted on lane 0 of a row and summed over the workgroup in thread order.  No atomics: two launches on the same inputs
// are bit-identical.  The two layouts run the same arithmetic; where their ORDER differs (both are kept, bit for bit) it is decided
// here and in class_marginals / balance_entropy / row_argmax, not in the heads:
//   BAL_SEEDS  c_loss: the weighted balance entropy seeds thread 0's loss accumulator before the row terms (Ten), or is added to the
//              workgroup's sum after them (Wide).
// c_loss<Wide> sits AT the 128 VGPRs a 1024-thread workgroup allows, without scratch; the order of its statements was chosen for that
// (-Rpass-analysis=kernel-resource-usage after any edit: one more value live across the unlabelled rows spills).
template <int LANES_, int SLOTS_, int THREADS_>
struct Layout {
  static_assert(LANES_ == 1 || LANES_ == 64, "a row belongs to one thread or to one wave");
  static constexpr int LANES = LANES_, SLOTS = SLOTS_, THREADS = THREADS_;
  static constexpr int WAVES = THREADS / 64, OWNERS = THREADS / LANES, KMAX = LANES * SLOTS;
  static constexpr bool ROW_PER_THREAD = LANES == 1, BAL_SEEDS = ROW_PER_THREAD;
  const int k, lane, owner;                              // classes (a constant when a thread holds the whole row); this thread's place
  __device__ explicit Layout(int k_)
      : k(ROW_PER_THREAD ? KMAX : k_), lane(threadIdx.x % LANES), owner(threadIdx.x / LANES) {}
  __device__ __forceinline__ int cls(int s) const { return s * LANES + lane; }
  __device__ __forceinline__ bool live(int s) const { return ROW_PER_THREAD || cls(s) < k; }
  // over the lanes of a row
  static __device__ __forceinline__ float row_sum(float v) { if constexpr (!ROW_PER_THREAD) v = tgd::wave_sum(v); return v; }
  static __device__ __forceinline__ float row_max(float v) { if constexpr (!ROW_PER_THREAD) v = tgd::wave_max(v); return v; }
  // over the row owners of a wave (64 of them, or the one)
  static __device__ __forceinline__ float owners_sum(float v) { if constexpr (ROW_PER_THREAD) v = tgd::wave_sum(v); return v; }
  // gradient columns k..ld of a row, and with `both` of a second one
  __device__ __forceinline__ void zero_pad(float* o, int ld, float* o2 = nullptr, bool both = false) const {
    for (int j = k + lane; j < ld; j += LANES) { o[j] = 0.f; if (both) o2[j] = 0.f; }
  }
};
using Ten = Layout<1, 10, 256>;
using Wide = Layout<64, 16, 1024>;

// LDS of the balance term: the class marginals q and their per-wave partials, sized by the layout (200 B for Ten, 68 KB for Wide)
template <class L>
struct Marginals { float part[L::WAVES][L::KMAX], q[L::KMAX]; };

// softmax of one row: l, p per slot (0 for classes >= k, never read), lse row-uniform
template <class L>
__device__ __forceinline__ void softmax_row(const L& t, const float* __restrict__ row, float (&l)[L::SLOTS], float (&p)[L::SLOTS], float* lse) {
  float m = -INFINITY;
#pragma unroll
  for (int s = 0; s < L::SLOTS; ++s) {
    l[s] = t.live(s) ? row[t.cls(s)] : 0.f;
    if (t.live(s)) m = fmaxf(m, l[s]);
  }
  m = L::row_max(m);
  float sum = 0.f;
#pragma unroll
  for (int s = 0; s < L::SLOTS; ++s) {
    p[s] = t.live(s) ? expf(l[s] - m) : 0.f;
    sum += p[s];
  }
  sum = L::row_sum(sum);
  const float inv = 1.f / sum;
#pragma unroll
  for (int s = 0; s < L::SLOTS; ++s) p[s] *= inv;
  *lse = m + logf(sum);
}

// mg.q[j] = mean over the n rows of softmax(z)_j, j < k: every row owner sums its rows, the row owners of a wave are reduced, the per-wave
// partials are added in wave order.  Ends with a barrier.
template <class L>
__device__ void class_marginals(const L& t, const float* __restrict__ z, int ld, int n, Marginals<L>& mg) {
  float l[L::SLOTS], p[L::SLOTS], lse, qa[L::SLOTS];
#pragma unroll
  for (int s = 0; s < L::SLOTS; ++s) qa[s] = 0.f;
  for (int r = t.owner; r < n; r += L::OWNERS) {
    softmax_row(t, z + (int64_t)r * ld, l, p, &lse);
#pragma unroll
    for (int s = 0; s < L::SLOTS; ++s) qa[s] += p[s];
  }
#pragma unroll
  for (int s = 0; s < L::SLOTS; ++s) {
    const float v = L::owners_sum(qa[s]);
    if ((threadIdx.x & 63) < L::LANES && t.live(s)) mg.part[threadIdx.x >> 6][t.cls(s)] = v;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < t.k; j += L::THREADS) {
    float s = mg.part[0][j];
    for (int i = 1; i < L::WAVES; ++i) s += mg.part[i][j];
    mg.q[j] = s / n;
  }
  __syncthreads();
}

// -sum_j (1/k) log(q_j + 1e-12), workgroup-uniform: in class order by every thread (Ten), or strided over the threads and block-summed (Wide)
template <class L>
__device__ float balance_entropy(const L& t, const float* q, float* red) {
  float b = 0.f;
  for (int j = L::ROW_PER_THREAD ? 0 : threadIdx.x; j < t.k; j += L::ROW_PER_THREAD ? 1 : L::THREADS) b -= logf(q[j] + 1e-12f) / t.k;
  if constexpr (!L::ROW_PER_THREAD) b = tgd::block_sum<L::WAVES>(b, red);
  return b;
}

// (sum_j y_j, sum_j y_j l_j) of one label row, row-uniform
template <class L>
__device__ __forceinline__ void label_dots(const L& t, const float* __restrict__ y, const float (&l)[L::SLOTS], float* ysum, float* yl) {
  float a = 0.f, b = 0.f;
#pragma unroll
  for (int s = 0; s < L::SLOTS; ++s)
    if (t.live(s)) { const float v = y[t.cls(s)]; a += v; b += v * l[s]; }
  *ysum = L::row_sum(a);
  *yl = L::row_sum(b);
}

// (max_j p_j, its class), row-uniform: the first maximum of a thread's classes, then over the lanes the lowest class among equal maxima
template <class L>
__device__ __forceinline__ void row_argmax(const L& t, const float (&p)[L::SLOTS], float* pmax, int* amax) {
  float pm = -1.f;
  int am = L::KMAX;
#pragma unroll
  for (int s = 0; s < L::SLOTS; ++s)
    if (t.live(s) && p[s] > pm) { pm = p[s]; am = t.cls(s); }
  if constexpr (!L::ROW_PER_THREAD) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float pv = __shfl_xor(pm, o, 64);
      const int av = __shfl_xor(am, o, 64);
      if (pv > pm || (pv == pm && av < am)) { pm = pv; am = av; }
    }
  }
  *pmax = pm;
  *amax = am;
}

// term weights of the classifier loss: {CE(real), c_unl, H(unl), Bal(unl), CE(fake), MSE(unl,rep)}; the last two are used when the
// device pair `lam` is absent (_loss_GAN keeps lambda_1 / lambda_2 in device memory so that schedule changes reach replayed graphs)
struct CW { float real, unl, h, bal, fake, mse; };

// rows ordered [real | unl | unl_rep (n_rep = n_unl or 0) | fake (n_fake may be 0)] of k logits; labels dense [n][k]
// c_loss = w.unl*c_unl + w.real*CE(real) + w.h*H(unl) + w.bal*Bal(unl) + lam1*CE(fake) + lam2*MSE(unl,rep)
// (_loss_GAN: {1, 0.005, 1e-6, 1e-3}; the variants of train_base.py:156-574 differ in the weights only).  terms (optional): the six
// unweighted term values.
template <class L>
__global__ void __launch_bounds__(L::THREADS) c_loss_kernel(const float* __restrict__ cl, int ld, int n_real, int n_unl, int n_rep, int n_fake, int k,
                                                            const float* __restrict__ y_real, const float* __restrict__ y_fake,
                                                            const float* __restrict__ d_unl, int ld_dunl, const float* __restrict__ lam, CW w,
                                                            float* __restrict__ dl, int ld_d, float* __restrict__ loss, float* __restrict__ terms) {
  __shared__ float red[L::WAVES];
  __shared__ Marginals<L> mg;
  const L t(k);
  const float* q = mg.q;
  const float lam1 = lam ? lam[0] : w.fake, lam2 = n_rep > 0 ? (lam ? lam[1] : w.mse) : 0.f;
  const int o_unl = n_real, o_rep = n_real + n_unl, o_fake = o_rep + n_rep;
  // pass A: the class marginals q_j = mean_n softmax(C_unl)_j of the balance entropy
  class_marginals(t, cl + (int64_t)o_unl * ld, ld, n_unl, mg);
  // row terms are row-uniform and counted on lane 0; the MSE is per-thread partials counted on every lane
  float acc = 0.f, t_real = 0.f, t_fake = 0.f, t_unl = 0.f, t_h = 0.f, t_mse = 0.f, bal = 0.f;
  if constexpr (L::BAL_SEEDS) {
    bal = balance_entropy(t, q, red);
    if (threadIdx.x == 0) acc += w.bal * bal;
  }
  float l[L::SLOTS], p[L::SLOTS], lse;
  for (int pass = 0; pass < 2; ++pass) {                 // labelled rows (real, then fake)
    const int n = pass == 0 ? n_real : n_fake, off = pass == 0 ? 0 : o_fake;
    const float* y = pass == 0 ? y_real : y_fake;
    const float wt = pass == 0 ? w.real : lam1;
    for (int r = t.owner; r < n; r += L::OWNERS) {
      softmax_row(t, cl + (int64_t)(off + r) * ld, l, p, &lse);
      const float* yr = y + (int64_t)r * t.k;
      float ysum, yl;
      label_dots(t, yr, l, &ysum, &yl);
      if (t.lane == 0) {
        acc += wt * (lse * ysum - yl) / n;
        if (pass == 0) t_real += (lse * ysum - yl) / n; else t_fake += (lse * ysum - yl) / n;
      }
      float* o = dl + (int64_t)(off + r) * ld_d;
#pragma unroll
      for (int s = 0; s < L::SLOTS; ++s)
        if (t.live(s)) o[t.cls(s)] = wt * (p[s] * ysum - yr[t.cls(s)]) / n;
      t.zero_pad(o, ld_d);
    }
  }
  for (int r = t.owner; r < n_unl; r += L::OWNERS) {     // unlabelled rows
    softmax_row(t, cl + (int64_t)(o_unl + r) * ld, l, p, &lse);
    const float rr = d_unl ? bce(d_unl[(int64_t)r * ld_dunl], 1.f) : 0.f;
    float pm, pl = 0.f, pdq = 0.f;
    int am;
#pragma unroll
    for (int s = 0; s < L::SLOTS; ++s)
      if (t.live(s)) {
        pl += p[s] * l[s];
        pdq += p[s] * (-1.f / (t.k * (q[t.cls(s)] + 1e-12f)) / n_unl);   // d Bal / d q_j, recomputed below (registers)
      }
    pl = L::row_sum(pl);
    pdq = L::row_sum(pdq);
    row_argmax(t, p, &pm, &am);
    if (t.lane == 0) {
      acc += w.unl * pm * rr / n_unl + w.h * (lse - pl) / n_unl;
      t_unl += pm * rr / n_unl;
      t_h += (lse - pl) / n_unl;
    }
    float* o = dl + (int64_t)(o_unl + r) * ld_d;
    float* orep = dl + (int64_t)(o_rep + r) * ld_d;
    const float* lrep = cl + (int64_t)(o_rep + r) * ld;
#pragma unroll
    for (int s = 0; s < L::SLOTS; ++s) {
      const int j = t.cls(s);
      if (s * L::LANES >= t.k) break;                    // no lane has a class in this slot or a later one
      if (!t.live(s)) continue;
      float g = w.unl * rr * pm * ((j == am ? 1.f : 0.f) - p[s]) / n_unl;       // C fools D (train_base.py:133-137)
      g += w.h * (p[s] - p[s] * (1.f + l[s] - pl)) / n_unl;                     // entropy
      g += w.bal * p[s] * (-1.f / (t.k * (q[j] + 1e-12f)) / n_unl - pdq);        // balance entropy
      if (n_rep > 0) {
        const float d = lrep[j] - l[s];
        const float gm = lam2 * 2.f * d / (n_unl * t.k);
        acc += lam2 * d * d / (n_unl * t.k);
        t_mse += d * d / (n_unl * t.k);
        g -= gm;
        orep[j] = gm;
      }
      o[j] = g;
    }
    t.zero_pad(o, ld_d, orep, n_rep > 0);
  }
  acc = tgd::block_sum<L::WAVES>(acc, red);
  if constexpr (!L::BAL_SEEDS) {
    bal = balance_entropy(t, q, red);
    acc += w.bal * bal;
  }
  if (threadIdx.x == 0) loss[0] = acc;
  if (terms) {                                           // block-uniform
    const float v[6] = {t_real, t_unl, t_h, 0.f, t_fake, t_mse};
    for (int i = 0; i < 6; ++i) {
      const float sum = i == 3 ? bal : tgd::block_sum<L::WAVES>(v[i], red);
      if (threadIdx.x == 0) terms[i] = sum;
    }
  }
}

__device__ __forceinline__ float softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// bad-GAN "true-fake" terms of the classifier (train_base.py:162-166, 226-229, 296-298): with lse = logsumexp_k logits,
//   T_unl  = mean_unl(-0.5 lse + 0.5 softplus(lse)),   T_fake = 0.5 mean_fake softplus(lse);
// loss = {w_unl T_unl + w_fake T_fake, T_unl, T_fake}; d/dlogits = coefficient * softmax, written or (acc_* != 0) added.
template <class L>
__global__ void __launch_bounds__(L::THREADS) true_fake_kernel(const float* __restrict__ unl, int ld_u, int n_unl, const float* __restrict__ fake,
                                                               int ld_f, int n_fake, int k, float w_unl, float w_fake, float* __restrict__ d_unl,
                                                               int ld_du, int acc_unl, float* __restrict__ d_fake, int ld_df, int acc_fake,
                                                               float* __restrict__ loss) {
  __shared__ float red[L::WAVES];
  const L t(k);
  float l[L::SLOTS], p[L::SLOTS], lse, t_u = 0.f, t_f = 0.f;
  for (int pass = 0; pass < 2; ++pass) {
    const int n = pass == 0 ? n_unl : n_fake;
    const float* src = pass == 0 ? unl : fake;
    const int ld = pass == 0 ? ld_u : ld_f, ldo = pass == 0 ? ld_du : ld_df, accum = pass == 0 ? acc_unl : acc_fake;
    float* dst = pass == 0 ? d_unl : d_fake;
    for (int r = t.owner; r < n; r += L::OWNERS) {
      softmax_row(t, src + (int64_t)r * ld, l, p, &lse);
      float coef;
      if (pass == 0) { if (t.lane == 0) t_u += (-0.5f * lse + 0.5f * softplus(lse)) / n; coef = w_unl * (-0.5f + 0.5f * sigm(lse)) / n; }
      else { if (t.lane == 0) t_f += 0.5f * softplus(lse) / n; coef = w_fake * 0.5f * sigm(lse) / n; }
      float* o = dst + (int64_t)r * ldo;
#pragma unroll
      for (int s = 0; s < L::SLOTS; ++s)
        if (t.live(s)) o[t.cls(s)] = (accum ? o[t.cls(s)] : 0.f) + coef * p[s];
      if (!accum) t.zero_pad(o, ldo);
    }
  }
  t_u = tgd::block_sum<L::WAVES>(t_u, red);
  t_f = tgd::block_sum<L::WAVES>(t_f, red);
  if (threadIdx.x == 0) { loss[0] = w_unl * t_u + w_fake * t_f; loss[1] = t_u; loss[2] = t_f; }
}

// T = mean_n sum_k (a - b)^2 (train_base.py:299: consistency of the classifier under a perturbation of the bad generator's sample);
// loss = {w T, T}; da = 2 w (a - b) / n, db = -da, written or added.
__global__ void __launch_bounds__(256) sqdiff_rows_kernel(const float* __restrict__ a, int ld_a, const float* __restrict__ b, int ld_b, int n, int k,
                                                          float w, float* __restrict__ da, int ld_da, int acc_a, float* __restrict__ db, int ld_db,
                                                          int acc_b, float* __restrict__ loss) {
  __shared__ float red[4];
  float t = 0.f;
  for (int i = threadIdx.x; i < n * k; i += 256) {
    const int r = i / k, c = i - r * k;
    const float d = a[(int64_t)r * ld_a + c] - b[(int64_t)r * ld_b + c];
    t += d * d / n;
    const float g = 2.f * w * d / n;
    if (da) { float* o = da + (int64_t)r * ld_da + c; *o = (acc_a ? *o : 0.f) + g; }
    if (db) { float* o = db + (int64_t)r * ld_db + c; *o = (acc_b ? *o : 0.f) - g; }
  }
  if (!acc_a && da) for (int i = threadIdx.x; i < n * (ld_da - k); i += 256) da[(int64_t)(i / (ld_da - k)) * ld_da + k + i % (ld_da - k)] = 0.f;
  if (!acc_b && db) for (int i = threadIdx.x; i < n * (ld_db - k); i += 256) db[(int64_t)(i / (ld_db - k)) * ld_db + k + i % (ld_db - k)] = 0.f;
  t = tgd::block_sum<4>(t, red);
  if (threadIdx.x == 0) { loss[0] = w * t; loss[1] = t; }
}

// fm = mean_c | mean_n f_fake - mean_n f_unl |   (train_base.py:172); one thread per feature column
__global__ void __launch_bounds__(256) feature_match_kernel(const float* __restrict__ ff, int n_f, const float* __restrict__ fu, int n_u, int c,
                                                            float* __restrict__ dff, float* __restrict__ dfu, float* __restrict__ loss) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int k = threadIdx.x; k < c; k += 256) {
    float a = 0.f, b = 0.f;
    for (int r = 0; r < n_f; ++r) a += ff[r * c + k];
    for (int r = 0; r < n_u; ++r) b += fu[r * c + k];
    const float d = a / n_f - b / n_u;
    acc += fabsf(d) / c;
    const float s = (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) / c;
    for (int r = 0; r < n_f; ++r) dff[r * c + k] = s / n_f;
    for (int r = 0; r < n_u; ++r) dfu[r * c + k] = -s / n_u;
  }
  acc = tgd::block_sum<4>(acc, red);
  if (threadIdx.x == 0) loss[0] = acc;
}

// pull-away term over N feature rows of width c (N <= 256, c <= 256); masked (train_base.py:175-181) or not (:204-207).
// scratch: N*c normalised rows + N*N cosines + N norms.
__global__ void __launch_bounds__(256) pull_away_kernel(const float* __restrict__ f, int n, int c, int masked, float* __restrict__ scratch,
                                                        float* __restrict__ df, float* __restrict__ loss) {
  __shared__ float red[4];
  float* fn = scratch;
  float* cs = scratch + n * c;
  float* nr = cs + n * n;
  for (int r = threadIdx.x; r < n; r += 256) {
    float ss = 0.f;
    for (int k = 0; k < c; ++k) ss += f[r * c + k] * f[r * c + k];
    const float nn = sqrtf(ss);
    nr[r] = nn;
    for (int k = 0; k < c; ++k) fn[r * c + k] = f[r * c + k] / nn;
  }
  __syncthreads();
  float acc = 0.f;
  for (int i = threadIdx.x; i < n * n; i += 256) {
    const int a = i / n, b = i % n;
    float d = 0.f;
    for (int k = 0; k < c; ++k) d += fn[a * c + k] * fn[b * c + k];
    if (masked) {
      const float mm = a == b ? 0.f : 1.f;
      acc += 0.8f * d * d * mm / (n * (n - 1));
      cs[i] = 0.8f * 2.f * d * mm / (n * (n - 1));      // d loss / d cos
    } else {
      acc += 0.8f * d / (n * n);
      cs[i] = 0.8f / (n * n);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n * c; i += 256) {
    const int r = i / c, k = i % c;
    float g = 0.f;
    for (int b = 0; b < n; ++b) g += (cs[r * n + b] + cs[b * n + r]) * fn[b * c + k];
    df[i] = g;                                            // d loss / d fn (projected below)
  }
  __syncthreads();
  for (int r = threadIdx.x; r < n; r += 256) {
    float dot = 0.f;
    for (int k = 0; k < c; ++k) dot += df[r * c + k] * fn[r * c + k];
    for (int k = 0; k < c; ++k) df[r * c + k] = (df[r * c + k] - fn[r * c + k] * dot) / nr[r];
  }
  acc = tgd::block_sum<4>(acc, red);
  if (threadIdx.x == 0) loss[0] = acc;
}

// Stand-alone heads behind the reference's Train_base helper methods (train_base.py:43-57,75-84): each is value + d/dlogits, the
// gradient written or (acc != 0) added so that a loss assembled from several helper calls accumulates into one gradient buffer.
// mean_n softmax-CE(labels, logits)  (tf.nn.softmax_cross_entropy_with_logits_v2 + reduce_mean); loss = {w T, T}
template <class L>
__global__ void __launch_bounds__(L::THREADS) softmax_ce_kernel(const float* __restrict__ z, int ld, const float* __restrict__ y, int n, int k, float w,
                                                                float* __restrict__ dz, int ld_d, int acc, float* __restrict__ loss) {
  __shared__ float red[L::WAVES];
  const L t(k);
  float l[L::SLOTS], p[L::SLOTS], lse, tt = 0.f;
  for (int r = t.owner; r < n; r += L::OWNERS) {
    softmax_row(t, z + (int64_t)r * ld, l, p, &lse);
    const float* yr = y + (int64_t)r * t.k;
    float ysum, yl;
    label_dots(t, yr, l, &ysum, &yl);
    if (t.lane == 0) tt += (lse * ysum - yl) / n;
    if (dz) {
      float* o = dz + (int64_t)r * ld_d;
#pragma unroll
      for (int s = 0; s < L::SLOTS; ++s)
        if (t.live(s)) o[t.cls(s)] = (acc ? o[t.cls(s)] : 0.f) + w * (p[s] * ysum - yr[t.cls(s)]) / n;
      if (!acc) t.zero_pad(o, ld_d);
    }
  }
  tt = tgd::block_sum<L::WAVES>(tt, red);
  if (threadIdx.x == 0) { loss[0] = w * tt; loss[1] = tt; }
}

// mean over n*c elements of sigmoid-CE(labels, logits)  (tf.nn.sigmoid_cross_entropy_with_logits + reduce_mean); labels NULL: the
// constant `label` everywhere (tf.ones_like / tf.zeros_like, train_base.py:123-128); loss = {w T, T}
__global__ void __launch_bounds__(256) bce_logits_kernel(const float* __restrict__ z, int ld, const float* __restrict__ y, int ld_y, float label, int n,
                                                         int c, float w, float* __restrict__ dz, int ld_d, int acc, float* __restrict__ loss) {
  __shared__ float red[4];
  float t = 0.f;
  const float inv = 1.f / ((float)n * c);
  for (int i = threadIdx.x; i < n * c; i += 256) {
    const int r = i / c, k = i - r * c;
    const float v = z[(int64_t)r * ld + k], tt = y ? y[(int64_t)r * ld_y + k] : label;
    t += bce(v, tt) * inv;
    if (dz) { float* o = dz + (int64_t)r * ld_d + k; *o = (acc ? *o : 0.f) + w * (sigm(v) - tt) * inv; }
  }
  if (dz && !acc && ld_d > c)
    for (int i = threadIdx.x; i < n * (ld_d - c); i += 256) dz[(int64_t)(i / (ld_d - c)) * ld_d + c + i % (ld_d - c)] = 0.f;
  t = tgd::block_sum<4>(t, red);
  if (threadIdx.x == 0) { loss[0] = w * t; loss[1] = t; }
}

// H = mean_n(lse - sum_k p_k l_k) (Train_base._entropy, train_base.py:43-48) and Bal = -sum_k (1/K) log(mean_n p_k + 1e-12)
// (_balance_entropy, :50-57); loss = {w_h H + w_bal Bal, H, Bal}
template <class L>
__global__ void __launch_bounds__(L::THREADS) entropy_terms_kernel(const float* __restrict__ z, int ld, int n, int k, float w_h, float w_bal,
                                                                   float* __restrict__ dz, int ld_d, int acc, float* __restrict__ loss) {
  __shared__ float red[L::WAVES];
  __shared__ Marginals<L> mg;
  const L t(k);
  const float* q = mg.q;
  class_marginals(t, z, ld, n, mg);
  float l[L::SLOTS], p[L::SLOTS], lse, t_h = 0.f;
  for (int r = t.owner; r < n; r += L::OWNERS) {
    softmax_row(t, z + (int64_t)r * ld, l, p, &lse);
    float pl = 0.f, pdq = 0.f, dq[L::SLOTS];             // dq: d Bal / d q_j
#pragma unroll
    for (int s = 0; s < L::SLOTS; ++s)
      if (t.live(s)) { pl += p[s] * l[s]; dq[s] = -1.f / (t.k * (q[t.cls(s)] + 1e-12f)) / n; pdq += p[s] * dq[s]; }
    pl = L::row_sum(pl);
    pdq = L::row_sum(pdq);
    if (t.lane == 0) t_h += (lse - pl) / n;
    if (dz) {
      float* o = dz + (int64_t)r * ld_d;
#pragma unroll
      for (int s = 0; s < L::SLOTS; ++s) {
        const int j = t.cls(s);
        if (t.live(s))
          o[j] = (acc ? o[j] : 0.f) + w_h * (p[s] - p[s] * (1.f + l[s] - pl)) / n + w_bal * p[s] * (dq[s] - pdq);
      }
      if (!acc) t.zero_pad(o, ld_d);
    }
  }
  t_h = tgd::block_sum<L::WAVES>(t_h, red);
  const float bal = balance_entropy(t, q, red);
  if (threadIdx.x == 0) { loss[0] = w_h * t_h + w_bal * bal; loss[1] = t_h; loss[2] = bal; }
}

// counters[0] += #(argmax logits == argmax labels), counters[1] += n     (tf.metrics.accuracy, Train_goodGAN.py:428-447)
__global__ void __launch_bounds__(256) accuracy_kernel(const float* __restrict__ logits, int ld, const float* __restrict__ labels, int n, int k,
                                                       float* __restrict__ counters) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int r = threadIdx.x; r < n; r += 256) {
    int a = 0, b = 0;
    for (int j = 1; j < k; ++j) {
      if (logits[(int64_t)r * ld + j] > logits[(int64_t)r * ld + a]) a = j;
      if (labels[r * k + j] > labels[r * k + b]) b = j;
    }
    acc += a == b ? 1.f : 0.f;
  }
  acc = tgd::block_sum<4>(acc, red);
  if (threadIdx.x == 0) { counters[0] += acc; counters[1] += (float)n; }
}

#define LOSS_LAUNCH_T(kern, threads, ...)                                    \
  hipStream_t s__ = tg::as_stream(stream);                                   \
  tg::ProfScope prof__(tg::PC_LOSS, 0, 0, s__);                              \
  hipLaunchKernelGGL(kern, dim3(1), dim3(threads), 0, s__, __VA_ARGS__);     \
  TG_CHECK_LAUNCH(#kern);                                                    \
  return TG_OK;
#define LOSS_LAUNCH(kern, ...) LOSS_LAUNCH_T(kern, 256, __VA_ARGS__)
// a classifier head over k classes: the layout that owns k
#define HEAD_LAUNCH(kern, k, ...)                                            \
  if ((k) == Ten::KMAX) { LOSS_LAUNCH_T(kern<Ten>, Ten::THREADS, __VA_ARGS__) } \
  LOSS_LAUNCH_T(kern<Wide>, Wide::THREADS, __VA_ARGS__)

// the class count of a classifier head
#define REQUIRE_K(name, k)                                                                                                          \
  TG_REQUIRE((k) >= 2 && (k) <= Wide::KMAX, "%s: k = %d classes is outside the supported range 2 <= k <= %d", name, (int)(k), Wide::KMAX)

// The one check and launch of each head that has several entry points.  `name` is the entry point the messages speak of.
int d_loss_head(const char* name, const float* logits, int ld, int n_real, int n_fake, int n_unl, float* dlogits, int ld_d, float* loss, float* terms,
                void* stream) {
  TG_REQUIRE(logits && dlogits && loss && n_real > 0 && n_fake > 0 && n_unl > 0 && ld >= 1 && ld_d >= 1, "%s: bad args", name);
  LOSS_LAUNCH(d_loss_kernel, logits, ld, n_real, n_fake, n_unl, dlogits, ld_d, loss, terms)
}

// lw: the DEVICE pair {lambda_1, lambda_2} beside the weights of _loss_GAN (every buffer and row group present), or with host_weights
// the HOST weights[6] (n_fake may be 0 and y_fake then NULL; d_unl_logits may be NULL when the C-fools-D weight is 0; terms optional)
int c_loss_head(const char* name, bool host_weights, const float* c_logits, int ld, int n_real, int n_unl, int n_rep, int n_fake, int k,
                const float* y_real, const float* y_fake, const float* d_unl_logits, int ld_dunl, const float* lw, float* dlogits, int ld_d,
                float* loss, float* terms, void* stream) {
  REQUIRE_K(name, k);
  TG_REQUIRE(c_logits && y_real && lw && dlogits && loss && (host_weights || (y_fake && d_unl_logits)), "%s: null buffer", name);
  TG_REQUIRE(n_real > 0 && n_unl > 0 && n_fake >= (host_weights ? 0 : 1) && (n_rep == 0 || n_rep == n_unl) && ld >= k && ld_d >= k, "%s: bad sizes",
             name);
  if (host_weights) {
    TG_REQUIRE(n_fake == 0 || y_fake, "%s: y_fake is NULL with %d generated rows", name, n_fake);
    TG_REQUIRE(d_unl_logits || lw[1] == 0.f, "%s: d_unl_logits is NULL but the C-fools-D weight is %g", name, (double)lw[1]);
  }
  const CW w = host_weights ? CW{lw[0], lw[1], lw[2], lw[3], lw[4], lw[5]} : CW{1.f, 0.005f, 1e-6f, 1e-3f, 0.f, 0.f};
  HEAD_LAUNCH(c_loss_kernel, k, c_logits, ld, n_real, n_unl, n_rep, n_fake, k, y_real, y_fake, d_unl_logits, ld_dunl,
              host_weights ? (const float*)nullptr : lw, w, dlogits, ld_d, loss, terms)
}

}  // namespace

extern "C" {

int tg_d_loss_f32(const float* logits, int ld, int n_real, int n_fake, int n_unl, float* dlogits, int ld_d, float* loss, void* stream) {
  return d_loss_head("d_loss", logits, ld, n_real, n_fake, n_unl, dlogits, ld_d, loss, nullptr, stream);
}

int tg_d_loss_terms_f32(const float* logits, int ld, int n_real, int n_fake, int n_unl, float* dlogits, int ld_d, float* loss, float* terms,
                        void* stream) {
  TG_REQUIRE(terms, "d_loss_terms: bad args");
  return d_loss_head("d_loss_terms", logits, ld, n_real, n_fake, n_unl, dlogits, ld_d, loss, terms, stream);
}

int tg_g_loss_f32(const float* logits, int ld, int n, float* dlogits, int ld_d, float* loss, void* stream) {
  TG_REQUIRE(logits && dlogits && loss && n > 0 && ld >= 1 && ld_d >= 1, "g_loss: bad args");
  LOSS_LAUNCH(g_loss_kernel, logits, ld, n, dlogits, ld_d, loss)
}

int tg_c_loss_f32(const float* c_logits, int ld, int n_real, int n_unl, int n_rep, int n_fake, const float* y_real, const float* y_fake,
                  const float* d_unl_logits, int ld_dunl, const float* lambdas, float* dlogits, int ld_d, float* loss, void* stream) {
  return tg_c_loss_k_f32(c_logits, ld, n_real, n_unl, n_rep, n_fake, Ten::KMAX, y_real, y_fake, d_unl_logits, ld_dunl, lambdas, dlogits, ld_d, loss,
                         stream);
}

int tg_c_loss_terms_f32(const float* c_logits, int ld, int n_real, int n_unl, int n_rep, int n_fake, const float* y_real, const float* y_fake,
                        const float* d_unl_logits, int ld_dunl, const float* weights, float* dlogits, int ld_d, float* loss, float* terms,
                        void* stream) {
  return tg_c_loss_terms_k_f32(c_logits, ld, n_real, n_unl, n_rep, n_fake, Ten::KMAX, y_real, y_fake, d_unl_logits, ld_dunl, weights, dlogits, ld_d,
                               loss, terms, stream);
}

int tg_c_loss_k_f32(const float* c_logits, int ld, int n_real, int n_unl, int n_rep, int n_fake, int k, const float* y_real, const float* y_fake,
                    const float* d_unl_logits, int ld_dunl, const float* lambdas, float* dlogits, int ld_d, float* loss, void* stream) {
  return c_loss_head("c_loss_k", false, c_logits, ld, n_real, n_unl, n_rep, n_fake, k, y_real, y_fake, d_unl_logits, ld_dunl, lambdas, dlogits, ld_d,
                     loss, nullptr, stream);
}

int tg_c_loss_terms_k_f32(const float* c_logits, int ld, int n_real, int n_unl, int n_rep, int n_fake, int k, const float* y_real,
                          const float* y_fake, const float* d_unl_logits, int ld_dunl, const float* weights, float* dlogits, int ld_d, float* loss,
                          float* terms, void* stream) {
  return c_loss_head("c_loss_terms_k", true, c_logits, ld, n_real, n_unl, n_rep, n_fake, k, y_real, y_fake, d_unl_logits, ld_dunl, weights, dlogits,
                     ld_d, loss, terms, stream);
}

int tg_true_fake_loss_f32(const float* unl_logits, int ld_u, int n_unl, const float* fake_logits, int ld_f, int n_fake, float w_unl, float w_fake,
                          float* d_unl, int ld_du, int accumulate_unl, float* d_fake, int ld_df, int accumulate_fake, float* loss, void* stream) {
  return tg_true_fake_loss_k_f32(unl_logits, ld_u, n_unl, fake_logits, ld_f, n_fake, Ten::KMAX, w_unl, w_fake, d_unl, ld_du, accumulate_unl, d_fake,
                                 ld_df, accumulate_fake, loss, stream);
}

int tg_true_fake_loss_k_f32(const float* unl_logits, int ld_u, int n_unl, const float* fake_logits, int ld_f, int n_fake, int k, float w_unl,
                            float w_fake, float* d_unl, int ld_du, int accumulate_unl, float* d_fake, int ld_df, int accumulate_fake, float* loss,
                            void* stream) {
  REQUIRE_K("true_fake_loss_k", k);
  TG_REQUIRE(unl_logits && fake_logits && d_unl && d_fake && loss, "true_fake_loss_k: null buffer");
  TG_REQUIRE(n_unl > 0 && n_fake > 0 && ld_u >= k && ld_f >= k && ld_du >= k && ld_df >= k, "true_fake_loss_k: bad sizes");
  HEAD_LAUNCH(true_fake_kernel, k, unl_logits, ld_u, n_unl, fake_logits, ld_f, n_fake, k, w_unl, w_fake, d_unl, ld_du, accumulate_unl, d_fake, ld_df,
              accumulate_fake, loss)
}

int tg_sqdiff_rows_loss_f32(const float* a, int ld_a, const float* b, int ld_b, int n, int k, float w, float* da, int ld_da, int accumulate_a,
                            float* db, int ld_db, int accumulate_b, float* loss, void* stream) {
  TG_REQUIRE(a && b && loss && n > 0 && k > 0 && k <= ld_a && k <= ld_b, "sqdiff_rows_loss: bad args");
  TG_REQUIRE((!da || k <= ld_da) && (!db || k <= ld_db), "sqdiff_rows_loss: gradient stride smaller than k=%d", k);
  LOSS_LAUNCH(sqdiff_rows_kernel, a, ld_a, b, ld_b, n, k, w, da, ld_da, accumulate_a, db, ld_db, accumulate_b, loss)
}

int tg_feature_match_f32(const float* f_fake, int n_fake, const float* f_unl, int n_unl, int c, float* df_fake, float* df_unl, float* loss,
                         void* stream) {
  TG_REQUIRE(f_fake && f_unl && df_fake && df_unl && loss && n_fake > 0 && n_unl > 0 && c > 0, "feature_match: bad args");
  LOSS_LAUNCH(feature_match_kernel, f_fake, n_fake, f_unl, n_unl, c, df_fake, df_unl, loss)
}

/* scratch: n*c + n*n + n floats */
int tg_pull_away_f32(const float* f, int n, int c, int masked, float* scratch, float* df, float* loss, void* stream) {
  TG_REQUIRE(f && scratch && df && loss && n > 1 && c > 0, "pull_away: bad args");
  LOSS_LAUNCH(pull_away_kernel, f, n, c, masked, scratch, df, loss)
}

int tg_softmax_ce_f32(const float* logits, int ld, const float* labels, int n, int k, float w, float* dlogits, int ld_d, int accumulate, float* loss,
                      void* stream) {
  REQUIRE_K("softmax_ce", k);
  TG_REQUIRE(logits && labels && loss && n > 0 && ld >= k && (!dlogits || ld_d >= k), "softmax_ce: bad args");
  HEAD_LAUNCH(softmax_ce_kernel, k, logits, ld, labels, n, k, w, dlogits, ld_d, accumulate, loss)
}

int tg_bce_logits_f32(const float* logits, int ld, const float* labels, int ld_y, float label, int n, int c, float w, float* dlogits, int ld_d,
                      int accumulate, float* loss, void* stream) {
  TG_REQUIRE(logits && loss && n > 0 && c > 0 && c <= ld && (!labels || c <= ld_y) && (!dlogits || c <= ld_d), "bce_logits: bad args");
  LOSS_LAUNCH(bce_logits_kernel, logits, ld, labels, ld_y, label, n, c, w, dlogits, ld_d, accumulate, loss)
}

int tg_entropy_terms_f32(const float* logits, int ld, int n, int k, float w_h, float w_bal, float* dlogits, int ld_d, int accumulate, float* loss,
                         void* stream) {
  REQUIRE_K("entropy_terms", k);
  TG_REQUIRE(logits && loss && n > 0 && ld >= k && (!dlogits || ld_d >= k), "entropy_terms: bad args");
  HEAD_LAUNCH(entropy_terms_kernel, k, logits, ld, n, k, w_h, w_bal, dlogits, ld_d, accumulate, loss)
}

int tg_accuracy_count_f32(const float* logits, int ld, const float* labels, int n, int k, float* counters, void* stream) {
  TG_REQUIRE(logits && labels && counters && n > 0 && k > 0 && k <= ld, "accuracy_count: bad args");
  LOSS_LAUNCH(accuracy_kernel, logits, ld, labels, n, k, counters)
}

}  // extern "C"
