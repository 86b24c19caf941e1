// Per-class evaluation report of a classifier's logits (tg_eval_report_f32; tg.metrics.ClassifierReport): the confusion
// matrix, the histogram of the target's rank, the calibration bins and the fp64 sums of NLL and Brier score of a batch, accumulated
// into the caller's buffers.
//   launch 1  one 64-lane wavefront per row, four rows per workgroup.  The row's k <= 1024 logits and labels are read once, lane L
//             holding columns L, 64 + L, ... in registers.  Target t and prediction p are the arg-max of accuracy_kernel's scan
//             (loss.hip): start at 0, move on strictly greater — that is index 0 when element 0 is a NaN, else the lowest index of the
//             greatest non-NaN element, which a cross-lane selection on (value descending, index ascending) finds whatever the order
//             the lanes are combined in.  Rank counts are integer wave sums; the fp64 sums over the classes are per-lane partial
//             sums in column order followed by one xor butterfly (a fixed tree; a + b == b + a, so every lane holds the same bits).
//             One lane per row adds 1 to confusion[t][p] (k*k destinations, no contention worth reducing) and to the workgroup's LDS
//             copies of the rank / bin / non-finite counters, which go out as one integer atomic per non-zero counter and workgroup.
//             The row's {NLL, Brier, conf, bin} go to the workspace as four doubles (a non-finite row: {0, 0, 0, -1}).
//   launch 2  66 workgroups, one per calibration bin (those >= nb leave at once) and one each for NLL and Brier: thread T adds the rows
//             T, 256 + T, ... in ascending order, a fixed LDS tree adds the 256 partial sums, and thread 0 accumulates into
//             bin_conf / sums.
// Integer sums do not depend on arrival order, nothing floating-point is atomic and both grids are functions of n alone: every output
// is bit-identical from run to run, on any stream.  Columns k..ld-1 / k..ld_y-1 and rows >= n are never read.
#include "tg_common.h"

namespace {

constexpr int ER_THREADS = 256, ER_ROWS = 4, ER_MAX_K = 1024, ER_MAX_RANKS = 32, ER_MAX_BINS = 64, ER_ROW_WORDS = 4;
constexpr int ER_FINAL_BLOCKS = ER_MAX_BINS + 2;

typedef unsigned long long er_count;          // the int64 counters, as the type atomicAdd takes (two's complement: the same bits)

struct Best { float v; int i; };              // i < 0: nothing yet

// what the sequential scan keeps of two candidates: the greater value, of equal ones the lower index
__device__ __forceinline__ Best better(Best a, Best b) {
  const bool take_b = b.i >= 0 && (a.i < 0 || b.v > a.v || (b.v == a.v && b.i < a.i));
  return take_b ? b : a;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// accuracy_kernel's arg-max of a row held as x[s] = row[s * 64 + lane]: `a = 0; for j: if (row[j] > row[a]) a = j`
template <int SLOTS>
__device__ __forceinline__ int scan_argmax(const float (&x)[SLOTS], int k, int lane) {
  Best b{0.f, -1};
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int j = s * 64 + lane;
    if (j < k && x[s] == x[s] && (b.i < 0 || x[s] > b.v)) b = Best{x[s], j};
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) b = better(b, Best{__shfl_xor(b.v, o, 64), __shfl_xor(b.i, o, 64)});
  const float x0 = __shfl(x[0], 0, 64);
  return x0 == x0 ? b.i : 0;                  // a NaN at index 0 is never left: nothing compares greater than it
}

// element `idx` of the row, in every lane
template <int SLOTS>
__device__ __forceinline__ float row_element(const float (&x)[SLOTS], int idx) {
  float mine = 0.f;
#pragma unroll
  for (int s = 0; s < SLOTS; ++s)
    if (s == (idx >> 6)) mine = x[s];
  return __shfl(mine, idx & 63, 64);
}

template <int SLOTS>
__global__ void __launch_bounds__(ER_THREADS) er_rows_kernel(const float* __restrict__ logits, int ld, const float* __restrict__ labels, int ld_y, int n,
                                                             int k, int nr, int nb, er_count* __restrict__ confusion, er_count* __restrict__ rank_hist,
                                                             er_count* __restrict__ bin_count, er_count* __restrict__ bin_correct,
                                                             er_count* __restrict__ nonfinite, double* __restrict__ rows) {
  __shared__ int h_rank[ER_MAX_RANKS], h_bin[ER_MAX_BINS], h_ok[ER_MAX_BINS], h_bad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < ER_MAX_BINS) { h_bin[tid] = 0; h_ok[tid] = 0; }
  if (tid < ER_MAX_RANKS) h_rank[tid] = 0;
  if (tid == 0) h_bad = 0;
  __syncthreads();
  const int r = blockIdx.x * ER_ROWS + wave;
  if (r < n) {                                 // (the same for the whole wave)
    const float* lrow = logits + (int64_t)r * ld;
    const float* yrow = labels + (int64_t)r * ld_y;
    float l[SLOTS], y[SLOTS];
    bool bad = false;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int j = s * 64 + lane;
      l[s] = j < k ? lrow[j] : 0.f;
      y[s] = j < k ? yrow[j] : 0.f;
      bad = bad || !(fabsf(l[s]) <= 3.402823466e+38f);
    }
    bad = __any(bad);
    const int t = scan_argmax<SLOTS>(y, k, lane), p = scan_argmax<SLOTS>(l, k, lane);
    double* out = rows + (int64_t)r * ER_ROW_WORDS;
    if (bad) {
      if (lane == 0) {
        atomicAdd(&confusion[(int64_t)t * k + p], (er_count)1);
        atomicAdd(&h_bad, 1);
        out[0] = 0.0; out[1] = 0.0; out[2] = 0.0; out[3] = -1.0;
      }
    } else {
      const float lt = row_element<SLOTS>(l, t), m = row_element<SLOTS>(l, p);
      int above = 0;
      double e[SLOTS], part = 0.0;
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        const int j = s * 64 + lane;
        e[s] = 0.0;
        if (j < k) {
          above += (l[s] > lt || (j < t && l[s] == lt)) ? 1 : 0;
          e[s] = exp((double)l[s] - (double)m);
          part += e[s];
        }
      }
      const int rank = wave_sum_int(above);
      const double sum = wave_sum_f64(part);
      const double conf = 1.0 / sum;
      const double nll = log(sum) + ((double)m - (double)lt);
      double bpart = 0.0;
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        const int j = s * 64 + lane;
        if (j < k) {
          const double d = e[s] / sum - (j == t ? 1.0 : 0.0);
          bpart += d * d;
        }
      }
      const double brier = wave_sum_f64(bpart);
      int b = (int)(conf * (double)nb);
      b = b > nb - 1 ? nb - 1 : b;
      if (lane == 0) {
        atomicAdd(&confusion[(int64_t)t * k + p], (er_count)1);
        atomicAdd(&h_rank[rank < nr - 1 ? rank : nr - 1], 1);
        atomicAdd(&h_bin[b], 1);
        if (p == t) atomicAdd(&h_ok[b], 1);
        out[0] = nll; out[1] = brier; out[2] = conf; out[3] = (double)b;
      }
    }
  }
  __syncthreads();
  if (tid < nb) {
    if (h_bin[tid]) atomicAdd(&bin_count[tid], (er_count)h_bin[tid]);
    if (h_ok[tid]) atomicAdd(&bin_correct[tid], (er_count)h_ok[tid]);
  }
  if (tid >= 64 && tid - 64 < nr && h_rank[tid - 64]) atomicAdd(&rank_hist[tid - 64], (er_count)h_rank[tid - 64]);
  if (tid == 128 && h_bad) atomicAdd(&nonfinite[0], (er_count)h_bad);
}

__global__ void __launch_bounds__(ER_THREADS) er_final_kernel(const double* __restrict__ rows, int n, int nb, double* __restrict__ bin_conf,
                                                              double* __restrict__ sums) {
  __shared__ double red[ER_THREADS];
  const int q = blockIdx.x, tid = threadIdx.x;               // q < 64: calibration bin q; 64: NLL; 65: Brier
  if (q < ER_MAX_BINS && q >= nb) return;                    // (the whole workgroup)
  double acc = 0.0;
  for (int r = tid; r < n; r += ER_THREADS) {
    const double* row = rows + (int64_t)r * ER_ROW_WORDS;
    if (q >= ER_MAX_BINS) acc += row[q - ER_MAX_BINS];
    else if (row[3] == (double)q) acc += row[2];
  }
  red[tid] = acc;
  __syncthreads();
  for (int w = ER_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    if (q < ER_MAX_BINS) bin_conf[q] += red[0];
    else sums[q - ER_MAX_BINS] += red[0];
  }
}

bool er_shape_ok(int n, int k) { return n >= 0 && k >= 2 && k <= ER_MAX_K; }

}  // namespace

extern "C" {

int64_t tg_eval_report_workspace_bytes(int n, int k) {
  if (!er_shape_ok(n, k)) { tg::set_error("eval_report_workspace_bytes: needs n >= 0 and 2 <= k <= %d (got n %d, k %d)", ER_MAX_K, n, k); return -1; }
  return (int64_t)n * ER_ROW_WORDS * (int64_t)sizeof(double);
}

int tg_eval_report_f32(const float* logits, int ld, const float* labels, int ld_y, int n, int k, int nr, int nb, int64_t* confusion,
                       int64_t* rank_hist, int64_t* bin_count, int64_t* bin_correct, double* bin_conf, double* sums, int64_t* nonfinite,
                       void* workspace, int64_t workspace_bytes, void* stream) {
  TG_REQUIRE(k >= 2 && k <= ER_MAX_K, "eval_report: k = %d classes is outside the supported range 2 <= k <= %d", k, ER_MAX_K);
  TG_REQUIRE(ld >= k && ld_y >= k, "eval_report: ld (%d) and ld_y (%d) must be at least k (%d)", ld, ld_y, k);
  TG_REQUIRE(nr >= 1 && nr <= ER_MAX_RANKS, "eval_report: nr must be in 1..%d, got %d", ER_MAX_RANKS, nr);
  TG_REQUIRE(nb >= 1 && nb <= ER_MAX_BINS, "eval_report: nb must be in 1..%d, got %d", ER_MAX_BINS, nb);
  TG_REQUIRE(n >= 0, "eval_report: n must not be negative, got %d", n);
  if (n == 0) return TG_OK;
  TG_REQUIRE(logits && labels && confusion && rank_hist && bin_count && bin_correct && bin_conf && sums && nonfinite && workspace,
             "eval_report: null pointer");
  TG_REQUIRE(((uintptr_t)confusion | (uintptr_t)rank_hist | (uintptr_t)bin_count | (uintptr_t)bin_correct | (uintptr_t)bin_conf | (uintptr_t)sums |
              (uintptr_t)nonfinite) % 8 == 0 && (uintptr_t)workspace % 16 == 0,
             "eval_report: the outputs must be 8-B aligned, the workspace 16-B aligned");
  const int64_t need = (int64_t)n * ER_ROW_WORDS * (int64_t)sizeof(double);
  TG_REQUIRE(workspace_bytes >= need, "eval_report: workspace of %lld bytes is smaller than tg_eval_report_workspace_bytes(n, k) = %lld",
             (long long)workspace_bytes, (long long)need);
  double* rows = static_cast<double*>(workspace);
  hipStream_t s = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_LOSS, 0, 8.0 * n * (double)k, s, "eval_report");
  const dim3 grid((n + ER_ROWS - 1) / ER_ROWS), block(ER_THREADS);
#define ER_LAUNCH(SLOTS)                                                                                                                  \
  hipLaunchKernelGGL(er_rows_kernel<SLOTS>, grid, block, 0, s, logits, ld, labels, ld_y, n, k, nr, nb, (er_count*)confusion, (er_count*)rank_hist, \
                     (er_count*)bin_count, (er_count*)bin_correct, (er_count*)nonfinite, rows)
  if (k <= 64) ER_LAUNCH(1);
  else if (k <= 128) ER_LAUNCH(2);
  else if (k <= 256) ER_LAUNCH(4);
  else ER_LAUNCH(16);
#undef ER_LAUNCH
  TG_CHECK_LAUNCH("er_rows_kernel");
  hipLaunchKernelGGL(er_final_kernel, dim3(ER_FINAL_BLOCKS), block, 0, s, rows, n, nb, bin_conf, sums);
  TG_CHECK_LAUNCH("er_final_kernel");
  return TG_OK;
}

}  // extern "C"
