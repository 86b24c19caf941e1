// First and second moments of an fp32 feature matrix in fp64 (tg_feature_moments_f32; Train.sample_metrics):
//   sum[k] += sum_r (double)f[r][k]          gram[a*c + b] += sum_r (double)f[r][a] * (double)f[r][b]
// A product of two fp32 values has at most 48 significant bits: it is exact in fp64, fused or not, so the only rounding is that of the
// fp64 additions — and every addition has a fixed place:
//   launch 1  the rows are cut into FM chunks(n, c) equal ranges and the columns into tiles of 32; workgroup (pair, p) owns the
//             32 x 32 block (ta, tb), ta <= tb, of row range p: it stages 64 rows of both column tiles in LDS, each of its 256 threads
//             adds the products of its 2 x 2 outputs in row order, and the block goes to the workspace as partial[p][a][b]; the
//             workgroups on the diagonal (ta == tb) also add their 32 column sums, in row order, into psum[p][k].
//   launch 2  one thread per output element adds its partials in range order p = 0, 1, ... and accumulates into sum / gram; element
//             (a, b) reads the partial of (min(a, b), max(a, b)), so both triangles of gram receive the same bits.
// The grid is a function of (n, c) alone and nothing floating-point is atomic: bit-identical from run to run, on any stream.
// Columns c..ld-1 and rows >= n are never read; tile entries beyond c are never stored.
#include "tg_common.h"

namespace {

constexpr int FM_TILE = 32, FM_ROWS = 64, FM_THREADS = 256, FM_MAX_C = 512, FM_MAX_CHUNKS = 64, FM_TARGET_BLOCKS = 1024;

int fm_tiles(int c) { return (c + FM_TILE - 1) / FM_TILE; }
int fm_pairs(int c) { const int t = fm_tiles(c); return t * (t + 1) / 2; }

// row ranges: enough workgroups to fill the device, at least FM_ROWS rows each, at most FM_MAX_CHUNKS (the workspace grows with it)
int fm_chunks(int n, int c) {
  int most = FM_TARGET_BLOCKS / fm_pairs(c);
  most = most < 1 ? 1 : (most > FM_MAX_CHUNKS ? FM_MAX_CHUNKS : most);
  const int want = (n + FM_ROWS - 1) / FM_ROWS;
  return want < 1 ? 1 : (want > most ? most : want);
}

__global__ void __launch_bounds__(FM_THREADS) fm_partial_kernel(const float* __restrict__ f, int ld, int n, int c, int tiles, int rows_per,
                                                                double* __restrict__ partial, double* __restrict__ psum) {
  __shared__ float A[FM_ROWS][FM_TILE + 1];
  __shared__ float B[FM_ROWS][FM_TILE + 1];
  // pair index -> (ta, tb), ta <= tb, row-major over the upper triangle
  int ta = 0, rest = blockIdx.x;
  while (rest >= tiles - ta) { rest -= tiles - ta; ++ta; }
  const int tb = ta + rest;
  const int p = blockIdx.y;
  const int r_begin = p * rows_per, r_end = min(n, r_begin + rows_per);
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int a0 = ta * FM_TILE, b0 = tb * FM_TILE;
  double acc00 = 0.0, acc01 = 0.0, acc10 = 0.0, acc11 = 0.0, csum = 0.0;
  for (int r0 = r_begin; r0 < r_end; r0 += FM_ROWS) {
    const int rows = min(FM_ROWS, r_end - r0);
    for (int i = threadIdx.x; i < FM_ROWS * FM_TILE; i += FM_THREADS) {
      const int r = i / FM_TILE, k = i % FM_TILE;
      const bool in_rows = r < rows;
      const int64_t base = (int64_t)(r0 + r) * ld;
      A[r][k] = (in_rows && a0 + k < c) ? f[base + a0 + k] : 0.f;
      B[r][k] = (in_rows && b0 + k < c) ? f[base + b0 + k] : 0.f;
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      const double x0 = (double)A[r][2 * ty], x1 = (double)A[r][2 * ty + 1];
      const double y0 = (double)B[r][2 * tx], y1 = (double)B[r][2 * tx + 1];
      acc00 = fma(x0, y0, acc00);                              // the product is exact: fma(x, y, s) == x * y + s
      acc01 = fma(x0, y1, acc01);
      acc10 = fma(x1, y0, acc10);
      acc11 = fma(x1, y1, acc11);
    }
    if (ta == tb && threadIdx.x < FM_TILE)
      for (int r = 0; r < rows; ++r) csum += (double)A[r][threadIdx.x];
    __syncthreads();
  }
  double* out = partial + (int64_t)p * c * c;
  const int a = a0 + 2 * ty, b = b0 + 2 * tx;
  if (a < c && b < c) out[(int64_t)a * c + b] = acc00;
  if (a < c && b + 1 < c) out[(int64_t)a * c + b + 1] = acc01;
  if (a + 1 < c && b < c) out[(int64_t)(a + 1) * c + b] = acc10;
  if (a + 1 < c && b + 1 < c) out[(int64_t)(a + 1) * c + b + 1] = acc11;
  if (ta == tb && threadIdx.x < FM_TILE && a0 + (int)threadIdx.x < c) psum[(int64_t)p * c + a0 + threadIdx.x] = csum;
}

__global__ void __launch_bounds__(FM_THREADS) fm_final_kernel(const double* __restrict__ partial, const double* __restrict__ psum, int c, int chunks,
                                                              double* __restrict__ sum, double* __restrict__ gram) {
  const int i = blockIdx.x * FM_THREADS + threadIdx.x;
  const int cc = c * c;
  if (i < cc) {
    const int a = i / c, b = i % c;
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    double s = 0.0;
    for (int p = 0; p < chunks; ++p) s += partial[(int64_t)p * cc + (int64_t)lo * c + hi];
    gram[i] += s;
  } else if (i < cc + c) {
    const int k = i - cc;
    double s = 0.0;
    for (int p = 0; p < chunks; ++p) s += psum[(int64_t)p * c + k];
    sum[k] += s;
  }
}

}  // namespace

extern "C" {

int64_t tg_feature_moments_workspace_bytes(int n, int c) {
  if (n < 0 || c < 1 || c > FM_MAX_C) { tg::set_error("feature_moments_workspace_bytes: needs n >= 0 and 1 <= c <= %d (got n %d, c %d)", FM_MAX_C, n, c); return -1; }
  if (n == 0) return 0;
  return (int64_t)fm_chunks(n, c) * ((int64_t)c * c + c) * (int64_t)sizeof(double);
}

int tg_feature_moments_f32(const float* f, int ld, int n, int c, double* sum, double* gram, void* workspace, int64_t workspace_bytes,
                           void* stream) {
  TG_REQUIRE(c >= 1 && c <= FM_MAX_C, "feature_moments: c must be in 1..%d, got %d", FM_MAX_C, c);
  TG_REQUIRE(ld >= c, "feature_moments: ld (%d) must be at least c (%d)", ld, c);
  TG_REQUIRE(n >= 0, "feature_moments: n must not be negative, got %d", n);
  if (n == 0) return TG_OK;
  TG_REQUIRE(f && sum && gram && workspace, "feature_moments: null pointer");
  TG_REQUIRE(((uintptr_t)sum % 8 == 0) && ((uintptr_t)gram % 8 == 0) && ((uintptr_t)workspace % 16 == 0),
             "feature_moments: sum / gram must be 8-B aligned, the workspace 16-B aligned");
  const int chunks = fm_chunks(n, c), tiles = fm_tiles(c);
  const int64_t need = (int64_t)chunks * ((int64_t)c * c + c) * (int64_t)sizeof(double);
  TG_REQUIRE(workspace_bytes >= need, "feature_moments: workspace of %lld bytes is smaller than tg_feature_moments_workspace_bytes(n, c) = %lld",
             (long long)workspace_bytes, (long long)need);
  double* partial = static_cast<double*>(workspace);
  double* psum = partial + (int64_t)chunks * c * c;
  const int rows_per = (n + chunks - 1) / chunks;
  hipStream_t s = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_ELEMWISE, 2.0 * n * (double)c * c, 4.0 * n * (double)c * tiles, s, "feature_moments");
  hipLaunchKernelGGL(fm_partial_kernel, dim3(fm_pairs(c), chunks), dim3(FM_THREADS), 0, s, f, ld, n, c, tiles, rows_per, partial, psum);
  TG_CHECK_LAUNCH("fm_partial_kernel");
  hipLaunchKernelGGL(fm_final_kernel, dim3((c * c + c + FM_THREADS - 1) / FM_THREADS), dim3(FM_THREADS), 0, s, partial, psum, c, chunks, sum, gram);
  TG_CHECK_LAUNCH("fm_final_kernel");
  return TG_OK;
}

}  // extern "C"
