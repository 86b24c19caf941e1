// Exact k-nearest rows between two sets of uint8 images (tg_nearest_u8_i32; tg.metrics.nearest_pixels, Train.nearest_training),
// and the quantiser that turns generated images back into the input pipeline's bytes (tg_f32_quantize_u8).
// The distance is part of the interface: d2(a, b) = sum_ch (a[ch] - b[ch])^2 as an exact integer.  With x' = (x ^ 0x80) read as int8
// (= x - 128, csrc/gram.hip) it is |q'|^2 + |r'|^2 - 2 q'.r', which the shared offset leaves unchanged; for d <= 16 384 every term is
// below 2^29 in magnitude, so all of it is exact in int32.  The distance matrix is never written to memory:
//   launch 1  workgroup (query tile of 64, reference range) walks the 64-row reference tiles of its range.  Per tile, 128-byte channel
//             chunks of both row tiles are staged in LDS (the next chunk's global loads fly under this chunk's MFMAs); each of the four
//             waves owns a 32 x 32 quarter of the tile and multiplies it with v_mfma_i32_32x32x32_i8.  The loader threads add up the
//             squares of the very bytes they stage, four threads per row: the norms come out of the same pass.  A channel beyond d or
//             a row beyond the matrix is staged as x' = 0 and never read from memory: it adds 0 to the dot product and to the norm.
//             The finished 64 x 64 tile of d2 goes through LDS to one thread per query row, which folds it, reference index ascending,
//             into its sorted list of the k smallest keys (d2 << 32 | index).  The list of (range, row) goes to the workspace.
//   launch 2  one wave per query row merges its lists — and, with `merge`, the k pairs already in best_* — by key.
// Keys compare as (d2, index) pairs and no two candidates share an index, so the k smallest are one set whatever the order they arrive
// in: the answer does not depend on the cut, on the chunking of the reference set or on the order of its chunks.  No atomics, the grid a
// function of the shapes alone: bit-identical from run to run, on any stream.  Rows >= m / n and columns >= d are never read.
#include "tg_common.h"

#include <cmath>

namespace {

constexpr int NR_TILE = 64;             // rows of a query tile and of a reference tile
constexpr int NR_KC = 128;              // channels (bytes) per LDS stage: 8 chunks of 16 bytes per row
constexpr int NR_THREADS = 256;         // 4 waves, each a 32 x 32 quarter of the tile
constexpr int NR_FINAL_THREADS = 64;     // the finishing launch: one wave per query row
constexpr int NR_MAX_D = 16384, NR_MAX_K = 16, NR_MAX_RANGES = 512, NR_TARGET_BLOCKS = 1024;
constexpr long long NR_NONE = ((long long)INT32_MAX << 32) | 0xffffffffLL;    // the pair (INT32_MAX, -1): above every real key

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

struct NrCut { int ranges, tiles_per; };

int nr_tiles(int rows) { return (rows + NR_TILE - 1) / NR_TILE; }

// reference ranges: enough workgroups to fill the device, whole tiles, none empty, at most NR_MAX_RANGES (the workspace grows with it)
NrCut nr_cut(int m, int n) {
  const int qt = nr_tiles(m), rt = nr_tiles(n);
  int want = (NR_TARGET_BLOCKS + qt - 1) / qt;
  want = want > NR_MAX_RANGES ? NR_MAX_RANGES : want;
  want = want > rt ? rt : want;
  want = want < 1 ? 1 : want;
  NrCut cut;
  cut.tiles_per = (rt + want - 1) / want;
  cut.ranges = (rt + cut.tiles_per - 1) / cut.tiles_per;
  return cut;
}

int64_t nr_bytes(int m, int n, int k) { return (int64_t)nr_cut(m, n).ranges * m * k * (int64_t)sizeof(long long); }

struct NrShared {
  alignas(16) uint8_t Q[NR_TILE * NR_KC];   // one 128-byte row per tile row; its eight 16-byte chunks XOR-swizzled by row bits 0..2
  alignas(16) uint8_t R[NR_TILE * NR_KC];
  int nq[NR_TILE], nr[NR_TILE];             // |q'|^2, |r'|^2 of the tile's rows
  int D[NR_TILE][NR_TILE + 1];              // the finished tile, [query][reference]
};

// byte offset of 16-byte chunk `chunk` of row `row` in a panel: eight consecutive rows put one chunk index on eight distinct 4-bank groups
__device__ __forceinline__ int nr_off(int row, int chunk) { return row * NR_KC + ((chunk ^ (row & 7)) << 4); }

// the 16 bytes x'[c0 .. c0 + 15] of row `row` (x' = x ^ 0x80); zeros — x' = 0 — for a row >= rows and for channels >= d
template <bool VEC>
__device__ __forceinline__ uint4 nr_load16(const uint8_t* __restrict__ x, int rows, int row, int d, int c0) {
  uint4 v = make_uint4(0, 0, 0, 0);
  if (row >= rows || c0 >= d) return v;
  const uint8_t* p = x + (int64_t)row * d + c0;
  if (VEC) {                                            // d % 16 == 0 and x 16-byte aligned: the whole chunk is inside the row
    v = *reinterpret_cast<const uint4*>(p);
    v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
  } else {
    uint32_t w[4] = {0, 0, 0, 0};
    for (int b = 0; b < 16; ++b)
      if (c0 + b < d) w[b >> 2] |= (uint32_t)(p[b] ^ 0x80u) << (8 * (b & 3));
    v = make_uint4(w[0], w[1], w[2], w[3]);
  }
  return v;
}

__device__ __forceinline__ int nr_sq4(uint32_t w) {
  const int a = (int8_t)(w & 0xff), b = (int8_t)((w >> 8) & 0xff), c = (int8_t)((w >> 16) & 0xff), e = (int8_t)(w >> 24);
  return a * a + b * b + c * c + e * e;
}

__device__ __forceinline__ int nr_sq16(const uint4& v) { return nr_sq4(v.x) + nr_sq4(v.y) + nr_sq4(v.z) + nr_sq4(v.w); }

// keep the KB smallest keys seen, ascending: v sinks to its place and the largest falls off the end (static indices: registers)
template <int KB>
__device__ __forceinline__ void nr_insert(long long (&list)[KB], long long v) {
#pragma unroll
  for (int t = 0; t < KB; ++t) {
    const bool below = v < list[t];
    const long long up = below ? list[t] : v;
    list[t] = below ? v : list[t];
    v = up;
  }
}

// part[(range * m + row) * k + t]: the k smallest keys (d2 << 32 | base + j) of the range, ascending; NR_NONE where it has fewer rows
template <int KB, bool VEC>
__global__ void __launch_bounds__(NR_THREADS) nr_range_kernel(const uint8_t* __restrict__ q, int m, const uint8_t* __restrict__ r, int n, int d,
                                                              int k, int base, int tiles_per, long long* __restrict__ part) {
  __shared__ NrShared sh;
  const int q0 = blockIdx.x * NR_TILE, p = blockIdx.y;
  const int all = (n + NR_TILE - 1) / NR_TILE;
  const int t_begin = p * tiles_per, t_end = min(all, t_begin + tiles_per);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // loader role: thread (lrow, lc) stages chunks 2 lc and 2 lc + 1 of row lrow of both panels
  const int lrow = tid >> 2, lc = (tid & 3) * 2;
  // MFMA role: wave quarter (wi: query half, wj: reference half), lane (rr, h)
  const int wi = wave & 1, wj = wave >> 1, rr = lane & 31, h = lane >> 5;
  const int row = q0 + tid;
  const bool owner = tid < NR_TILE && row < m;
  long long list[KB];
#pragma unroll
  for (int t = 0; t < KB; ++t) list[t] = NR_NONE;

  for (int tile = t_begin; tile < t_end; ++tile) {
    const int r0 = tile * NR_TILE;
    v16i acc;
    for (int e = 0; e < 16; ++e) acc[e] = 0;
    int sq_q = 0, sq_r = 0;
    uint4 gq[2], gr[2];
    for (int u = 0; u < 2; ++u) {
      gq[u] = nr_load16<VEC>(q, m, q0 + lrow, d, (lc + u) * 16);
      gr[u] = nr_load16<VEC>(r, n, r0 + lrow, d, (lc + u) * 16);
    }
    for (int c0 = 0; c0 < d; c0 += NR_KC) {
      __syncthreads();                                  // the previous stage's fragment reads are done
      for (int u = 0; u < 2; ++u) {
        *reinterpret_cast<uint4*>(sh.Q + nr_off(lrow, lc + u)) = gq[u];
        *reinterpret_cast<uint4*>(sh.R + nr_off(lrow, lc + u)) = gr[u];
        sq_q += nr_sq16(gq[u]);
        sq_r += nr_sq16(gr[u]);
      }
      __syncthreads();
      if (c0 + NR_KC < d)                               // the next stage's global loads fly under this stage's MFMAs
        for (int u = 0; u < 2; ++u) {
          gq[u] = nr_load16<VEC>(q, m, q0 + lrow, d, c0 + NR_KC + (lc + u) * 16);
          gr[u] = nr_load16<VEC>(r, n, r0 + lrow, d, c0 + NR_KC + (lc + u) * 16);
        }
      for (int kk = 0; kk < NR_KC / 32; ++kk) {
        // lane half h takes channels 32 kk + 16 h .. + 15 of its row, in the same byte order for A and B: whatever k order the
        // instruction assigns to the 16 bytes of a lane half, both operands agree on it (csrc/gram.hip)
        const v4i fa = *reinterpret_cast<const v4i*>(sh.Q + nr_off(wi * 32 + rr, 2 * kk + h));
        const v4i fb = *reinterpret_cast<const v4i*>(sh.R + nr_off(wj * 32 + rr, 2 * kk + h));
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb, acc, 0, 0, 0);
      }
    }
    // the four loader threads of a row are neighbouring lanes
    sq_q += __shfl_xor(sq_q, 1); sq_q += __shfl_xor(sq_q, 2);
    sq_r += __shfl_xor(sq_r, 1); sq_r += __shfl_xor(sq_r, 2);
    if ((tid & 3) == 0) { sh.nq[lrow] = sq_q; sh.nr[lrow] = sq_r; }
    __syncthreads();                                    // (the previous tile's readers of D passed the stage barriers: they are done)
    // 32x32 C/D map: column (reference) lane & 31, row (query) (e & 3) + 8 (e >> 2) + 4 h
    for (int e = 0; e < 16; ++e) {
      const int a = wi * 32 + (e & 3) + 8 * (e >> 2) + 4 * h, b = wj * 32 + rr;
      sh.D[a][b] = sh.nq[a] + sh.nr[b] - 2 * acc[e];
    }
    __syncthreads();
    if (owner) {
      const int cols = min(NR_TILE, n - r0);
      for (int j = 0; j < cols; ++j) {
        const long long key = ((long long)sh.D[tid][j] << 32) | (long long)(uint32_t)(base + r0 + j);
        if (key < list[KB - 1]) nr_insert<KB>(list, key);
      }
    }
  }
  if (owner) {
    long long* out = part + ((int64_t)p * m + row) * k;
#pragma unroll
    for (int t = 0; t < KB; ++t)
      if (t < k) out[t] = list[t];
  }
}

// one wave per query row: lane l merges the lists of ranges l, l + 64, ... (lane 0 also the k pairs already in best_*), then lane 0
// merges the 64 lane lists — each ascending, so a lane's list is done at its first key that does not make the cut
template <int KB>
__global__ void __launch_bounds__(NR_FINAL_THREADS) nr_final_kernel(const long long* __restrict__ part, int m, int k, int ranges, int merge,
                                                                    int32_t* best_d2, int32_t* best_idx) {
  __shared__ long long lists[NR_FINAL_THREADS][KB];
  const int row = blockIdx.x, lane = threadIdx.x;
  long long list[KB];
#pragma unroll
  for (int t = 0; t < KB; ++t) list[t] = NR_NONE;
  if (merge && lane == 0)
    for (int t = 0; t < k; ++t) {
      const long long key = ((long long)best_d2[(int64_t)row * k + t] << 32) | (long long)(uint32_t)best_idx[(int64_t)row * k + t];
      if (key < list[KB - 1]) nr_insert<KB>(list, key);
    }
  for (int p = lane; p < ranges; p += NR_FINAL_THREADS) {
    const long long* in = part + ((int64_t)p * m + row) * k;
    for (int t = 0; t < k; ++t) {
      const long long key = in[t];
      if (key < list[KB - 1]) nr_insert<KB>(list, key);
    }
  }
#pragma unroll
  for (int t = 0; t < KB; ++t) lists[lane][t] = list[t];
  __syncthreads();
  if (lane != 0) return;
  for (int l = 1; l < NR_FINAL_THREADS; ++l)
    for (int t = 0; t < KB; ++t) {
      const long long key = lists[l][t];
      if (key >= list[KB - 1]) break;
      nr_insert<KB>(list, key);
    }
#pragma unroll
  for (int t = 0; t < KB; ++t)
    if (t < k) {
      best_d2[(int64_t)row * k + t] = (int32_t)(list[t] >> 32);
      best_idx[(int64_t)row * k + t] = (int32_t)(uint32_t)(list[t] & 0xffffffffLL);
    }
}

template <int KB>
int nr_launch(const uint8_t* q, int m, const uint8_t* r, int n, int d, int k, int base, int merge, int32_t* best_d2, int32_t* best_idx,
              long long* part, hipStream_t s) {
  const NrCut cut = nr_cut(m, n);
  const dim3 grid(nr_tiles(m), cut.ranges);
  const bool vec = d % 16 == 0 && (reinterpret_cast<uintptr_t>(q) & 15) == 0 && (reinterpret_cast<uintptr_t>(r) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL((nr_range_kernel<KB, true>), grid, dim3(NR_THREADS), 0, s, q, m, r, n, d, k, base, cut.tiles_per, part);
  else
    hipLaunchKernelGGL((nr_range_kernel<KB, false>), grid, dim3(NR_THREADS), 0, s, q, m, r, n, d, k, base, cut.tiles_per, part);
  TG_CHECK_LAUNCH("nr_range_kernel");
  hipLaunchKernelGGL(nr_final_kernel<KB>, dim3(m), dim3(NR_FINAL_THREADS), 0, s, part, m, k, cut.ranges, merge, best_d2, best_idx);
  TG_CHECK_LAUNCH("nr_final_kernel");
  return TG_OK;
}

// the inverse of u8_affine (csrc/elementwise.hip): three separately rounded fp32 operations (the Makefile builds with -ffp-contract=off),
// round half up, clamp; a NaN fails the first comparison and gives 0
__global__ void quantize_u8(const float* __restrict__ src, uint8_t* __restrict__ dst, int64_t n, float inv, float shift) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float t = (src[i] - shift) * inv;
    const float u = floorf(t + 0.5f);
    dst[i] = (uint8_t)(u > 0.f ? (u < 255.f ? u : 255.f) : 0.f);
  }
}

bool nr_shape_ok(int m, int n) { return m >= 1 && n >= 1; }

}  // namespace

extern "C" {

int64_t tg_nearest_u8_workspace_bytes(int m, int n, int d, int k) {
  if (!nr_shape_ok(m, n) || d < 1 || d > NR_MAX_D || k < 1 || k > NR_MAX_K) {
    tg::set_error("nearest_u8_workspace_bytes: needs m >= 1, n >= 1, 1 <= d <= %d and 1 <= k <= %d (got m %d, n %d, d %d, k %d)", NR_MAX_D,
                  NR_MAX_K, m, n, d, k);
    return -1;
  }
  return nr_bytes(m, n, k);
}

int tg_nearest_u8_ranges(int m, int n) {
  if (!nr_shape_ok(m, n)) {
    tg::set_error("nearest_u8_ranges: needs m >= 1 and n >= 1 (got m %d, n %d)", m, n);
    return -1;
  }
  return nr_cut(m, n).ranges;
}

int tg_nearest_u8_i32(const uint8_t* q, int m, const uint8_t* r, int n, int d, int k, int32_t base, int merge, int32_t* best_d2,
                      int32_t* best_idx, void* workspace, int64_t workspace_bytes, void* stream) {
  TG_REQUIRE(m >= 1 && n >= 1, "nearest_u8: m and n must be at least 1, got m %d, n %d", m, n);
  TG_REQUIRE(d >= 1 && d <= NR_MAX_D, "nearest_u8: d must be in 1..%d (255^2 d stays below 2^31), got %d", NR_MAX_D, d);
  TG_REQUIRE(k >= 1 && k <= NR_MAX_K, "nearest_u8: k must be in 1..%d, got %d", NR_MAX_K, k);
  TG_REQUIRE(base >= 0 && (int64_t)base + n <= (int64_t)INT32_MAX, "nearest_u8: base (%d) must be >= 0 and base + n (%d) at most INT32_MAX",
             base, n);
  TG_REQUIRE(q && r && best_d2 && best_idx && workspace, "nearest_u8: null pointer");
  TG_REQUIRE(((uintptr_t)best_d2 % 4 == 0) && ((uintptr_t)best_idx % 4 == 0) && ((uintptr_t)workspace % 16 == 0),
             "nearest_u8: best_d2 / best_idx must be 4-B aligned, the workspace 16-B aligned");
  const int64_t need = nr_bytes(m, n, k);
  TG_REQUIRE(workspace_bytes >= need, "nearest_u8: workspace of %lld bytes is smaller than tg_nearest_u8_workspace_bytes(m, n, d, k) = %lld",
             (long long)workspace_bytes, (long long)need);
  hipStream_t s = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_IGEMM, 2.0 * m * (double)n * d, (double)nr_tiles(m) * n * (double)d + (double)m * d * nr_tiles(n), s, "nearest_u8");
  long long* part = static_cast<long long*>(workspace);
  if (k <= 4) return nr_launch<4>(q, m, r, n, d, k, base, merge, best_d2, best_idx, part, s);
  return nr_launch<NR_MAX_K>(q, m, r, n, d, k, base, merge, best_d2, best_idx, part, s);
}

int tg_f32_quantize_u8(const float* src, uint8_t* dst, int64_t n, float scale, float shift, void* stream) {
  TG_REQUIRE(n >= 0, "f32_quantize_u8: n must not be negative, got %lld", (long long)n);
  TG_REQUIRE(scale != 0.f && std::isfinite(scale) && std::isfinite(shift), "f32_quantize_u8: scale must be finite and not 0, shift finite");
  if (n == 0) return TG_OK;
  TG_REQUIRE(src && dst, "f32_quantize_u8: null pointer");
  const float inv = 255.0f / scale;
  hipStream_t s = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_ELEMWISE, 4.0 * n, 5.0 * n, s, "f32_quantize_u8");
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(quantize_u8, dim3((unsigned)(blocks > 65535 ? 65535 : blocks)), dim3(256), 0, s, src, dst, n, inv, shift);
  TG_CHECK_LAUNCH("quantize_u8");
  return TG_OK;
}

}  // extern "C"
