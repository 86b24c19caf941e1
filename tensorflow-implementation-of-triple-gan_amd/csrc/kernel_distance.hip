// Sums of the cubic polynomial kernel over pairs of fp32 feature rows (tg_poly3_sums_f32; tg.metrics.kernel_distance): for
// every segment s of a host table,  out[s] = sum over i in A_s, j in B_s of k(a_i, b_j),  k(x, y) = t * t * t,  t = <x, y> / c + 1  — the
// three sums the unbiased MMD^2 ("kernel inception distance", Binkowski et al. 2018) is made of.  The arithmetic is the interface's:
//   <x, y>   every fp32 feature is widened to fp64 at the fragment read (so every product is exact) and the dot product is accumulated in
//            fp64 on v_mfma_f64_16x16x4_f64, channels ascending.
//   k        t = dot / (double)c; t = t + 1; k = (t * t) * t — fp64, separately rounded (the Makefile builds with -ffp-contract=off).
//   sums     a lane adds its 16 values of a tile in a fixed order, lanes -> wave by a __shfl_down tree, waves -> workgroup in LDS in wave
//            order: one fp64 partial per tile in the workspace.  A finishing launch (one workgroup per segment) adds a segment's partials,
//            thread t taking the tiles t, t + 256, ... in tile order, through the same tree.  Nothing floating-point is atomic.
// The Gram matrix is never written.  A 256-thread workgroup owns a 64 x 64 tile of pairs of ONE segment; each of its 4 waves holds 2 x 2
// accumulators of 16 x 16 (four independent chains).  Channel chunks of 32 of both row tiles are staged in LDS as fp32, [row][channel] with
// rows of 36 floats (a fragment read — 16 rows x 4 channels — touches 64 different banks).  A row beyond its segment's end and a channel
// beyond c are staged as 0 and never read from memory; the pairs of such rows, and with exclude_diag the pairs i - seg_a[s] == j - seg_b[s],
// are left out of the sum BY INDEX in the epilogue, which is the one place that sees the f64 MFMA's C/D map:
//   col = lane & 15, row = (lane >> 4) + 4 * reg          (NOT the f32 map, whose row is 4 * (lane >> 4) + reg)
// Launch sequence (as tg_tf_histogram_f32): the (segment, tile-row, tile-column) map and the per-segment table are built on the host from
// the offsets and copied into the workspace, one workgroup per tile, one workgroup per segment.  The grid depends on the segment table
// alone: the output is bit-identical from run to run, on any stream.
#include <vector>
#include "tg_common.h"

namespace {

constexpr int PD_TILE = 64, PD_CH = 32, PD_LD = PD_CH + 4, PD_THREADS = 256, PD_MAX_C = 512, PD_MAX_SEG = 1024;
constexpr int64_t PD_MAX_TILES = (int64_t)1 << 24;

typedef double pd_f64x4 __attribute__((ext_vector_type(4)));

struct pd_tile {                         // one workgroup's share: tile (tr, tc) of segment `seg`
  int32_t seg, tr, tc, pad;
};
struct pd_seg {                          // a segment: rows [a0, a0 + an) x [b0, b0 + bn), its partials partial[first .. first + tiles)
  int32_t a0, an, b0, bn, first, tiles, pad0, pad1;
};

int64_t pd_align16(int64_t v) { return (v + 15) / 16 * 16; }

struct pd_layout {                       // workspace: [tile map][segment table][per-tile partial sums]
  int64_t tiles, off_seg, off_partial, bytes;
};

// false when the tables are malformed (a negative or decreasing offset) or ask for more than PD_MAX_TILES tiles
bool pd_plan(const int32_t* seg_a, const int32_t* seg_b, int nseg, pd_layout* L) {
  if (seg_a[0] < 0 || seg_b[0] < 0) return false;
  int64_t tiles = 0;
  for (int s = 0; s < nseg; ++s) {
    if (seg_a[s + 1] < seg_a[s] || seg_b[s + 1] < seg_b[s]) return false;
    const int64_t ta = ((int64_t)seg_a[s + 1] - seg_a[s] + PD_TILE - 1) / PD_TILE, tb = ((int64_t)seg_b[s + 1] - seg_b[s] + PD_TILE - 1) / PD_TILE;
    tiles += ta * tb;
    if (tiles > PD_MAX_TILES) return false;
  }
  L->tiles = tiles;
  L->off_seg = pd_align16(tiles * (int64_t)sizeof(pd_tile));
  L->off_partial = pd_align16(L->off_seg + (int64_t)nseg * (int64_t)sizeof(pd_seg));
  L->bytes = L->off_partial + (tiles > 0 ? tiles : 1) * (int64_t)sizeof(double);
  return true;
}

// fixed-order sum of a workgroup: valid in thread 0
__device__ __forceinline__ double pd_block_sum(double acc, double* slot) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = acc;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < PD_THREADS / 64; ++w) s += slot[w];
  }
  return s;
}

// rows row0 .. row0 + 63 of x, channels c0 .. c0 + 31 -> dst[row][channel]; a row at or beyond `rows` (the tile's count) and a channel at or
// beyond c are staged as 0 without being read
__device__ __forceinline__ void pd_stage(float (*dst)[PD_LD], const float* __restrict__ x, int ld, int64_t row0, int rows, int c, int c0) {
  for (int i = threadIdx.x; i < PD_TILE * PD_CH; i += PD_THREADS) {
    const int r = i / PD_CH, ch = i % PD_CH;
    const bool in = r < rows && c0 + ch < c;
    dst[r][ch] = in ? x[(row0 + r) * ld + c0 + ch] : 0.f;
  }
}

__global__ void __launch_bounds__(PD_THREADS) poly3_tile_kernel(const float* __restrict__ a, int ld_a, const float* __restrict__ b, int ld_b, int c,
                                                                const pd_tile* __restrict__ map, const pd_seg* __restrict__ segs, int nseg,
                                                                int rows_a, int rows_b, int exclude_diag, double* __restrict__ partial) {
  __shared__ float sA[PD_TILE][PD_LD];
  __shared__ float sB[PD_TILE][PD_LD];
  __shared__ double red[PD_THREADS / 64];
  const pd_tile tl = map[blockIdx.x];
  // the map and the table are the host's, checked there; an entry that does not fit the matrices is still never followed
  int i0 = 0, j0 = 0, an = 0, bn = 0;
  int64_t arow = 0, brow = 0;
  if (tl.seg >= 0 && tl.seg < nseg && tl.tr >= 0 && tl.tc >= 0) {
    const pd_seg sg = segs[tl.seg];
    const int64_t li = (int64_t)tl.tr * PD_TILE, lj = (int64_t)tl.tc * PD_TILE;
    if (sg.a0 >= 0 && sg.an >= 0 && sg.a0 <= rows_a - sg.an && sg.b0 >= 0 && sg.bn >= 0 && sg.b0 <= rows_b - sg.bn && li < sg.an && lj < sg.bn) {
      i0 = (int)li; j0 = (int)lj;
      an = min(PD_TILE, sg.an - i0); bn = min(PD_TILE, sg.bn - j0);
      arow = (int64_t)sg.a0 + i0; brow = (int64_t)sg.b0 + j0;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;               // the wave's 32 x 32 quarter of the tile
  const int fr = lane & 15, fk = lane >> 4;                            // A[row fr][k fk], B[k fk][col fr]: one value per lane
  pd_f64x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = pd_f64x4{0.0, 0.0, 0.0, 0.0};
  for (int c0 = 0; c0 < c; c0 += PD_CH) {
    pd_stage(sA, a, ld_a, arow, an, c, c0);
    pd_stage(sB, b, ld_b, brow, bn, c, c0);
    __syncthreads();
    const int steps = (min(PD_CH, c - c0) + 3) / 4;                    // uniform; the channels of the last step beyond c hold 0
    for (int ks = 0; ks < steps; ++ks) {
      const int ch = ks * 4 + fk;
      const double a0 = (double)sA[wr + fr][ch], a1 = (double)sA[wr + 16 + fr][ch];
      const double b0 = (double)sB[wc + fr][ch], b1 = (double)sB[wc + 16 + fr][ch];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
  // C/D of the f64 MFMA: register r of a lane is row (lane >> 4) + 4 r, column lane & 15 of the 16 x 16 block
  const double cd = (double)c;
  double sum = 0.0;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wr + i * 16 + (lane >> 4) + 4 * r, col = wc + j * 16 + (lane & 15);
        const bool in = row < an && col < bn && !(exclude_diag && i0 + row == j0 + col);
        double t = acc[i][j][r] / cd;
        t = t + 1.0;
        const double k = (t * t) * t;
        sum = sum + (in ? k : 0.0);
      }
  const double total = pd_block_sum(sum, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

__global__ void __launch_bounds__(PD_THREADS) poly3_final_kernel(const pd_seg* __restrict__ segs, const double* __restrict__ partial,
                                                                 double* __restrict__ out, int64_t tiles) {
  __shared__ double red[PD_THREADS / 64];
  pd_seg sg = segs[blockIdx.x];
  if (sg.first < 0 || sg.tiles < 0 || sg.first > tiles - sg.tiles) sg.tiles = 0;
  double sum = 0.0;
  for (int t = threadIdx.x; t < sg.tiles; t += PD_THREADS) sum += partial[(int64_t)sg.first + t];
  const double total = pd_block_sum(sum, red);
  if (threadIdx.x == 0) out[blockIdx.x] = total;
}

}  // namespace

extern "C" {

int64_t tg_poly3_sums_workspace_bytes(const int32_t* seg_a, const int32_t* seg_b, int nseg) {
  if (nseg < 1 || nseg > PD_MAX_SEG || !seg_a || !seg_b) {
    tg::set_error("poly3_sums_workspace_bytes: needs 1 <= nseg <= %d and both offset tables (got nseg %d)", PD_MAX_SEG, nseg);
    return -1;
  }
  pd_layout L;
  if (!pd_plan(seg_a, seg_b, nseg, &L)) {
    tg::set_error("poly3_sums_workspace_bytes: the offsets must be non-negative and non-decreasing, and cover at most %lld tiles of %d x %d pairs",
                  (long long)PD_MAX_TILES, PD_TILE, PD_TILE);
    return -1;
  }
  return L.bytes;
}

int tg_poly3_sums_f32(const float* a, int ld_a, const float* b, int ld_b, int c, const int32_t* seg_a, const int32_t* seg_b, int nseg,
                      int exclude_diag, double* out, void* workspace, int64_t workspace_bytes, void* stream) {
  TG_REQUIRE(c >= 1 && c <= PD_MAX_C, "poly3_sums: c must be in 1..%d, got %d", PD_MAX_C, c);
  TG_REQUIRE(nseg >= 1 && nseg <= PD_MAX_SEG, "poly3_sums: nseg must be in 1..%d, got %d", PD_MAX_SEG, nseg);
  TG_REQUIRE(ld_a >= c && ld_b >= c, "poly3_sums: ld_a (%d) and ld_b (%d) must be at least c (%d)", ld_a, ld_b, c);
  TG_REQUIRE(exclude_diag == 0 || exclude_diag == 1, "poly3_sums: exclude_diag must be 0 or 1, got %d", exclude_diag);
  TG_REQUIRE(a && b && seg_a && seg_b && out && workspace, "poly3_sums: null pointer");
  TG_REQUIRE(((uintptr_t)a % 4 == 0) && ((uintptr_t)b % 4 == 0) && ((uintptr_t)out % 8 == 0) && ((uintptr_t)workspace % 16 == 0),
             "poly3_sums: a / b must be 4-B aligned, out 8-B aligned, the workspace 16-B aligned");
  pd_layout L;
  TG_REQUIRE(pd_plan(seg_a, seg_b, nseg, &L), "poly3_sums: the offsets must be non-negative and non-decreasing, and cover at most %lld tiles",
             (long long)PD_MAX_TILES);
  TG_REQUIRE(workspace_bytes >= L.bytes, "poly3_sums: workspace of %lld bytes is smaller than tg_poly3_sums_workspace_bytes(...) = %lld",
             (long long)workspace_bytes, (long long)L.bytes);
  hipStream_t st = tg::as_stream(stream);
  double pairs = 0.0;
  // the map, built here and copied: [tiles of segment 0, row-major][of segment 1]... then the segment table
  std::vector<char> host((size_t)L.off_partial, 0);
  pd_tile* map = reinterpret_cast<pd_tile*>(host.data());
  pd_seg* segs = reinterpret_cast<pd_seg*>(host.data() + L.off_seg);
  int32_t t = 0;
  for (int s = 0; s < nseg; ++s) {
    pd_seg& sg = segs[s];
    sg.a0 = seg_a[s]; sg.an = seg_a[s + 1] - seg_a[s];
    sg.b0 = seg_b[s]; sg.bn = seg_b[s + 1] - seg_b[s];
    sg.first = t;
    const int ta = (sg.an + PD_TILE - 1) / PD_TILE, tb = (sg.bn + PD_TILE - 1) / PD_TILE;
    for (int tr = 0; tr < ta; ++tr)
      for (int tc = 0; tc < tb; ++tc, ++t) {
        map[t].seg = s; map[t].tr = tr; map[t].tc = tc;
      }
    sg.tiles = t - sg.first;
    pairs += (double)sg.an * (double)sg.bn;
  }
  tg::ProfScope prof(tg::PC_ELEMWISE, 2.0 * pairs * c, 4.0 * c * PD_TILE * 2.0 * (double)L.tiles, st, "poly3_sums");
  char* ws = static_cast<char*>(workspace);
  hipError_t e = hipMemcpyAsync(ws, host.data(), host.size(), hipMemcpyHostToDevice, st);    // pageable source: read before the call returns
  if (e != hipSuccess) return tg::hip_fail(e, "hipMemcpyAsync(poly3 tile map)");
  double* partial = reinterpret_cast<double*>(ws + L.off_partial);
  const pd_seg* segs_dev = reinterpret_cast<const pd_seg*>(ws + L.off_seg);
  if (L.tiles > 0) {
    hipLaunchKernelGGL(poly3_tile_kernel, dim3((unsigned)L.tiles), dim3(PD_THREADS), 0, st, a, ld_a, b, ld_b, c, reinterpret_cast<const pd_tile*>(ws),
                       segs_dev, nseg, (int)seg_a[nseg], (int)seg_b[nseg], exclude_diag, partial);
    TG_CHECK_LAUNCH("poly3_tile_kernel");
  }
  hipLaunchKernelGGL(poly3_final_kernel, dim3(nseg), dim3(PD_THREADS), 0, st, segs_dev, partial, out, L.tiles);
  TG_CHECK_LAUNCH("poly3_final_kernel");
  return TG_OK;
}

}  // extern "C"
