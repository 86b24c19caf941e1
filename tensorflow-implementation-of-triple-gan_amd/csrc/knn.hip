// k-nearest-neighbour distances on fp32 feature rows (tg_knn_self_f32, tg_manifold_query_f32; tg.metrics.manifold_metrics).
// The distance is the fp32 chain of include/tg_kernels.h:  acc = 0; for ch ascending: d = a[ch] - b[ch]; p = d * d; acc = acc + p
// — three separately rounded operations per channel (the Makefile builds with -ffp-contract=off and nothing here calls fmaf), one
// accumulator per pair.  The distance matrix is never written to memory:
//   launch 1  workgroup (query tile, reference range) walks the 64-row reference tiles of its range.  Per tile its 256 threads hold a
//             4 x 4 block of pairs each (16 independent chains); channel chunks of 32 of both row tiles are staged in LDS channel-major,
//             so a thread reads its 4 query and 4 reference values of a channel as two 16-byte words, and the chunks follow each other
//             in channel order into the same accumulators.  A channel beyond c or a row beyond the matrix is staged as 0 and never
//             read from memory: it adds d = 0, p = 0, acc + 0 = acc, exactly.  The finished 64 x 64 tile goes through LDS to one
//             thread per query row, which folds it, reference index ascending, into its partial: a sorted list of the smallest values
//             (self), or the count, the minimum and its first index (query).  The partial of (range, row) goes to the workspace.
//   launch 2  one thread per row merges its partials in range order.
// Ranges ascend and every comparison is strict, so the first index of a minimum is the lowest; the grid is a function of the shapes
// alone and nothing is atomic: bit-identical from run to run, on any stream.  Rows >= n and columns >= c are never read.
#include "tg_common.h"

#include <math.h>

namespace {

constexpr int KN_TILE = 64, KN_CH = 32, KN_LD = KN_TILE + 4, KN_THREADS = 256, KN_MAX_C = 512, KN_MAX_K = 16, KN_MAX_RANGES = 64,
              KN_TARGET_BLOCKS = 1024;

struct KnShared {
  alignas(16) float Q[KN_CH][KN_LD];  // [channel][row]: rows of 272 bytes keep every 4-row group 16-byte aligned
  alignas(16) float R[KN_CH][KN_LD];
  float D[KN_TILE][KN_TILE + 1];    // the finished tile, [query][reference]
};

struct KnCut { int ranges, tiles_per; };

int kn_tiles(int rows) { return (rows + KN_TILE - 1) / KN_TILE; }

// reference ranges: enough workgroups to fill the device, whole tiles, none empty, at most KN_MAX_RANGES (the workspace grows with it)
KnCut kn_cut(int n_query, int n_ref) {
  const int qt = kn_tiles(n_query), rt = kn_tiles(n_ref);
  int want = (KN_TARGET_BLOCKS + qt - 1) / qt;
  want = want > KN_MAX_RANGES ? KN_MAX_RANGES : want;
  want = want > rt ? rt : want;
  want = want < 1 ? 1 : want;
  KnCut cut;
  cut.tiles_per = (rt + want - 1) / want;
  cut.ranges = (rt + cut.tiles_per - 1) / cut.tiles_per;
  return cut;
}

__device__ __forceinline__ void kn_stage(float (*dst)[KN_LD], const float* __restrict__ x, int ld, int rows, int row0, int c, int c0) {
  for (int i = threadIdx.x; i < KN_TILE * KN_CH; i += KN_THREADS) {
    const int r = i / KN_CH, ch = i % KN_CH;
    const bool in = row0 + r < rows && c0 + ch < c;
    dst[ch][r] = in ? x[(int64_t)(row0 + r) * ld + c0 + ch] : 0.f;
  }
}

// sh.D[a][b] = d2(q[q0 + a], r[r0 + b]) for the whole tile (entries of rows beyond m / n are those of zero rows: finite, never used).
// Ends with a barrier; the barrier after the first staging of the next call orders that call's writes to D after this tile's readers.
__device__ __forceinline__ void kn_tile_d2(KnShared& sh, const float* __restrict__ q, int ld_q, int m, int q0, const float* __restrict__ r,
                                           int ld_r, int n, int r0, int c) {
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
  for (int c0 = 0; c0 < c; c0 += KN_CH) {
    kn_stage(sh.Q, q, ld_q, m, q0, c, c0);
    kn_stage(sh.R, r, ld_r, n, r0, c, c0);
    __syncthreads();
#pragma unroll 4
    for (int ch = 0; ch < KN_CH; ++ch) {
      const float4 qa = *reinterpret_cast<const float4*>(&sh.Q[ch][ty * 4]);
      const float4 rb = *reinterpret_cast<const float4*>(&sh.R[ch][tx * 4]);
      const float av[4] = {qa.x, qa.y, qa.z, qa.w}, bv[4] = {rb.x, rb.y, rb.z, rb.w};
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const float d = av[a] - bv[b];
          const float p = d * d;
          acc[a][b] = acc[a][b] + p;
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) sh.D[ty * 4 + a][tx * 4 + b] = acc[a][b];
  __syncthreads();
}

// keep the KB smallest values seen, ascending: v sinks to its place and the largest falls off the end (static indices: registers)
template <int KB>
__device__ __forceinline__ void kn_insert(float (&list)[KB], float v) {
#pragma unroll
  for (int t = 0; t < KB; ++t) {
    const bool below = v < list[t];
    const float up = below ? list[t] : v;
    list[t] = below ? v : list[t];
    v = up;
  }
}

// part[(range * n + row) * k + t]: the k smallest of the range (+inf where the range has fewer candidates).  KB >= k values are kept.
template <int KB>
__global__ void __launch_bounds__(KN_THREADS) kn_self_kernel(const float* __restrict__ x, int ld, int n, int c, int k, int tiles_per,
                                                             float* __restrict__ part) {
  __shared__ KnShared sh;
  const int q0 = blockIdx.x * KN_TILE, p = blockIdx.y;
  const int all = (n + KN_TILE - 1) / KN_TILE;
  const int t_begin = p * tiles_per, t_end = min(all, t_begin + tiles_per);
  const int row = q0 + (int)threadIdx.x;
  const bool owner = threadIdx.x < KN_TILE && row < n;
  float list[KB];
#pragma unroll
  for (int t = 0; t < KB; ++t) list[t] = INFINITY;
  for (int tile = t_begin; tile < t_end; ++tile) {
    const int r0 = tile * KN_TILE;
    kn_tile_d2(sh, x, ld, n, q0, x, ld, n, r0, c);
    if (owner) {
      const int cols = min(KN_TILE, n - r0);
      for (int j = 0; j < cols; ++j) {
        const float v = sh.D[threadIdx.x][j];
        if (r0 + j != row && v < list[KB - 1]) kn_insert<KB>(list, v);
      }
    }
  }
  if (owner) {
    float* out = part + ((int64_t)p * n + row) * k;
#pragma unroll
    for (int t = 0; t < KB; ++t)
      if (t < k) out[t] = list[t];
  }
}

template <int KB>
__global__ void __launch_bounds__(KN_THREADS) kn_self_final_kernel(const float* __restrict__ part, int n, int k, int ranges,
                                                                   float* __restrict__ out_d2) {
  const int row = blockIdx.x * KN_THREADS + threadIdx.x;
  if (row >= n) return;
  float list[KB];
#pragma unroll
  for (int t = 0; t < KB; ++t) list[t] = INFINITY;
  for (int p = 0; p < ranges; ++p) {
    const float* in = part + ((int64_t)p * n + row) * k;
    for (int t = 0; t < k; ++t) {
      const float v = in[t];
      if (v < list[KB - 1]) kn_insert<KB>(list, v);
    }
  }
  float* out = out_d2 + (int64_t)row * k;
#pragma unroll
  for (int t = 0; t < KB; ++t)
    if (t < k) out[t] = list[t];
}

// pmin / pidx / pcnt [range * m + row]
__global__ void __launch_bounds__(KN_THREADS) kn_query_kernel(const float* __restrict__ q, int ld_q, int m, const float* __restrict__ r, int ld_r,
                                                              int n, int c, const float* __restrict__ r2, int tiles_per,
                                                              float* __restrict__ pmin, int32_t* __restrict__ pidx, int32_t* __restrict__ pcnt) {
  __shared__ KnShared sh;
  const int q0 = blockIdx.x * KN_TILE, p = blockIdx.y;
  const int all = (n + KN_TILE - 1) / KN_TILE;
  const int t_begin = p * tiles_per, t_end = min(all, t_begin + tiles_per);
  const int row = q0 + (int)threadIdx.x;
  const bool owner = threadIdx.x < KN_TILE && row < m;
  float best = INFINITY;
  int best_j = t_begin * KN_TILE, hits = 0;
  for (int tile = t_begin; tile < t_end; ++tile) {
    const int r0 = tile * KN_TILE;
    kn_tile_d2(sh, q, ld_q, m, q0, r, ld_r, n, r0, c);
    if (owner) {
      const int cols = min(KN_TILE, n - r0);
      for (int j = 0; j < cols; ++j) {
        const float v = sh.D[threadIdx.x][j];
        if (v < best) { best = v; best_j = r0 + j; }
        if (r2 != nullptr && v <= r2[r0 + j]) ++hits;
      }
    }
  }
  if (owner) {
    const int64_t at = (int64_t)p * m + row;
    pmin[at] = best;
    pidx[at] = best_j;
    pcnt[at] = hits;
  }
}

__global__ void __launch_bounds__(KN_THREADS) kn_query_final_kernel(const float* __restrict__ pmin, const int32_t* __restrict__ pidx,
                                                                    const int32_t* __restrict__ pcnt, int m, int ranges, bool counted,
                                                                    int32_t* __restrict__ count, float* __restrict__ nn_d2,
                                                                    int32_t* __restrict__ nn_idx) {
  const int row = blockIdx.x * KN_THREADS + threadIdx.x;
  if (row >= m) return;
  float best = pmin[row];
  int best_j = pidx[row], hits = pcnt[row];
  for (int p = 1; p < ranges; ++p) {
    const int64_t at = (int64_t)p * m + row;
    const float v = pmin[at];
    if (v < best) { best = v; best_j = pidx[at]; }
    hits += pcnt[at];
  }
  nn_d2[row] = best;
  nn_idx[row] = best_j;
  if (counted) count[row] = hits;
}

int64_t kn_self_bytes(int n, int k) { return (int64_t)kn_cut(n, n).ranges * n * k * (int64_t)sizeof(float); }
int64_t kn_query_bytes(int m, int n) { return (int64_t)kn_cut(m, n).ranges * m * 3 * (int64_t)sizeof(float); }

}  // namespace

extern "C" {

int64_t tg_knn_self_workspace_bytes(int n, int k) {
  if (k < 1 || k > KN_MAX_K || n < k + 1) {
    tg::set_error("knn_self_workspace_bytes: needs 1 <= k <= %d and n >= k + 1 (got n %d, k %d)", KN_MAX_K, n, k);
    return -1;
  }
  return kn_self_bytes(n, k);
}

int tg_knn_self_f32(const float* x, int ld, int n, int c, int k, float* out_d2, void* workspace, int64_t workspace_bytes, void* stream) {
  TG_REQUIRE(c >= 1 && c <= KN_MAX_C, "knn_self: c must be in 1..%d, got %d", KN_MAX_C, c);
  TG_REQUIRE(k >= 1 && k <= KN_MAX_K, "knn_self: k must be in 1..%d, got %d", KN_MAX_K, k);
  TG_REQUIRE(n >= k + 1, "knn_self: n (%d) must be at least k + 1 (k %d): a row is not its own neighbour", n, k);
  TG_REQUIRE(ld >= c, "knn_self: ld (%d) must be at least c (%d)", ld, c);
  TG_REQUIRE(x && out_d2 && workspace, "knn_self: null pointer");
  TG_REQUIRE(((uintptr_t)x % 4 == 0) && ((uintptr_t)out_d2 % 4 == 0) && ((uintptr_t)workspace % 16 == 0),
             "knn_self: x / out_d2 must be 4-B aligned, the workspace 16-B aligned");
  const int64_t need = kn_self_bytes(n, k);
  TG_REQUIRE(workspace_bytes >= need, "knn_self: workspace of %lld bytes is smaller than tg_knn_self_workspace_bytes(n, k) = %lld",
             (long long)workspace_bytes, (long long)need);
  const KnCut cut = kn_cut(n, n);
  float* part = static_cast<float*>(workspace);
  hipStream_t s = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_ELEMWISE, 3.0 * n * (double)n * c, 8.0 * n * (double)c * kn_tiles(n), s, "knn_self");
  const dim3 grid(kn_tiles(n), cut.ranges), fgrid((n + KN_THREADS - 1) / KN_THREADS);
  if (k <= 4) {
    hipLaunchKernelGGL(kn_self_kernel<4>, grid, dim3(KN_THREADS), 0, s, x, ld, n, c, k, cut.tiles_per, part);
    TG_CHECK_LAUNCH("kn_self_kernel");
    hipLaunchKernelGGL(kn_self_final_kernel<4>, fgrid, dim3(KN_THREADS), 0, s, part, n, k, cut.ranges, out_d2);
  } else {
    hipLaunchKernelGGL(kn_self_kernel<KN_MAX_K>, grid, dim3(KN_THREADS), 0, s, x, ld, n, c, k, cut.tiles_per, part);
    TG_CHECK_LAUNCH("kn_self_kernel");
    hipLaunchKernelGGL(kn_self_final_kernel<KN_MAX_K>, fgrid, dim3(KN_THREADS), 0, s, part, n, k, cut.ranges, out_d2);
  }
  TG_CHECK_LAUNCH("kn_self_final_kernel");
  return TG_OK;
}

int64_t tg_manifold_query_workspace_bytes(int m, int n) {
  if (m < 1 || n < 1) {
    tg::set_error("manifold_query_workspace_bytes: needs m >= 1 and n >= 1 (got m %d, n %d)", m, n);
    return -1;
  }
  return kn_query_bytes(m, n);
}

int tg_manifold_query_f32(const float* q, int ld_q, int m, const float* r, int ld_r, int n, int c, const float* r2, int32_t* count,
                          float* nn_d2, int32_t* nn_idx, void* workspace, int64_t workspace_bytes, void* stream) {
  TG_REQUIRE(c >= 1 && c <= KN_MAX_C, "manifold_query: c must be in 1..%d, got %d", KN_MAX_C, c);
  TG_REQUIRE(m >= 1 && n >= 1, "manifold_query: m and n must be at least 1, got m %d, n %d", m, n);
  TG_REQUIRE(ld_q >= c && ld_r >= c, "manifold_query: ld_q (%d) and ld_r (%d) must be at least c (%d)", ld_q, ld_r, c);
  TG_REQUIRE(q && r && nn_d2 && nn_idx && workspace, "manifold_query: null pointer");
  TG_REQUIRE(r2 == nullptr || count != nullptr, "manifold_query: r2 is given, so count must not be null");
  TG_REQUIRE(((uintptr_t)q % 4 == 0) && ((uintptr_t)r % 4 == 0) && ((uintptr_t)r2 % 4 == 0) && ((uintptr_t)count % 4 == 0) &&
                 ((uintptr_t)nn_d2 % 4 == 0) && ((uintptr_t)nn_idx % 4 == 0) && ((uintptr_t)workspace % 16 == 0),
             "manifold_query: the arrays must be 4-B aligned, the workspace 16-B aligned");
  const int64_t need = kn_query_bytes(m, n);
  TG_REQUIRE(workspace_bytes >= need, "manifold_query: workspace of %lld bytes is smaller than tg_manifold_query_workspace_bytes(m, n) = %lld",
             (long long)workspace_bytes, (long long)need);
  const KnCut cut = kn_cut(m, n);
  const int64_t slots = (int64_t)cut.ranges * m;
  float* pmin = static_cast<float*>(workspace);
  int32_t* pidx = reinterpret_cast<int32_t*>(pmin + slots);
  int32_t* pcnt = pidx + slots;
  hipStream_t s = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_ELEMWISE, 3.0 * m * (double)n * c, 8.0 * m * (double)c * kn_tiles(n), s, "manifold_query");
  hipLaunchKernelGGL(kn_query_kernel, dim3(kn_tiles(m), cut.ranges), dim3(KN_THREADS), 0, s, q, ld_q, m, r, ld_r, n, c, r2, cut.tiles_per,
                     pmin, pidx, pcnt);
  TG_CHECK_LAUNCH("kn_query_kernel");
  hipLaunchKernelGGL(kn_query_final_kernel, dim3((m + KN_THREADS - 1) / KN_THREADS), dim3(KN_THREADS), 0, s, pmin, pidx, pcnt, m, cut.ranges,
                     r2 != nullptr, count, nn_d2, nn_idx);
  TG_CHECK_LAUNCH("kn_query_final_kernel");
  return TG_OK;
}

}  // extern "C"
