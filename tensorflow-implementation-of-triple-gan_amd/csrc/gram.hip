// Exact integer Gram matrix of uint8 images (the data term of the CIFAR ZCA fit, Model/Good_GAN_cifar10.py cifar10_ZCA.fit):
//   gram[d][d] += sum_n x'_n x'_n^T,  colsum[d] += sum_n x'_n,  x' = x - 128 = (x ^ 0x80) read as int8 (exact for 0..255).
// One workgroup computes one 128 x 128 tile (i-block <= j-block: the upper triangle only) over one range of at most GRAM_ROWS_MAX images
// with v_mfma_i32_32x32x32_i8 into int32 accumulators (|x'x'| <= 2^14, so 131 071 rows cannot overflow), then adds the tile to the int64
// output, once for (i, j) and once transposed for (j, i): with plain loads and stores when one image range covers all n (each output
// element has one owner), with global atomics when several do.  Integer additions commute, so the result does not depend on the order in
// which the image ranges land: it is bit-exact and deterministic for any n.
#include <type_traits>

#include "tg_common.h"

namespace {

constexpr int GT = 128;                 // output tile edge (features)
constexpr int GK = 64;                  // images per LDS stage
constexpr int GTHREADS = 256;           // 4 waves, each a 64 x 64 quarter of the tile (2 x 2 MFMA tiles of 32 x 32)
constexpr int CPAD = GT + 1;            // epilogue tile row stride (int32): column reads without bank conflicts
constexpr int64_t GRAM_ROWS_MAX = 131008;   // images per workgroup: a multiple of GK, <= 131071 (the int32 window)
constexpr int GRAM_TARGET_BLOCKS = 1024;
constexpr int64_t GRAM_ROWS_MIN = 32768;  // images per workgroup before the grid is split further: the int64 adds of a tile
                                           // (256 KB) must not outweigh its MFMA work

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// Staging panel: one 64-byte row per feature (GK images as int8), the four 16-byte chunks of a row XOR-swizzled by row bits 2..3, so
// that the ds_read_b128 fragment reads of 16 consecutive rows land on 16 distinct 4-bank groups.
__device__ __forceinline__ int panel_off(int f, int chunk) { return f * GK + ((chunk ^ ((f >> 2) & 3)) << 4); }

// byte q of the 16 bytes held in v (little-endian)
__device__ __forceinline__ uint32_t byte_of(const uint4& v, int q) {
  const uint32_t w = q < 4 ? v.x : q < 8 ? v.y : q < 12 ? v.z : v.w;
  return (w >> (8 * (q & 3))) & 0xffu;
}

__device__ __forceinline__ int sbyte_sum(uint32_t w) {
  return (int)(int8_t)(w & 0xff) + (int)(int8_t)((w >> 8) & 0xff) + (int)(int8_t)((w >> 16) & 0xff) + (int)(int8_t)(w >> 24);
}

// 16 bytes (features f0..f0+15) of image row n as x' = x ^ 0x80; zeros (x' = 0 adds nothing) outside the image range or past d.
template <bool VEC>
__device__ __forceinline__ uint4 load16(const uint8_t* __restrict__ x, int64_t n, int64_t n_end, int d, int f0) {
  uint4 v = make_uint4(0, 0, 0, 0);
  if (n >= n_end || f0 >= d) return v;
  const uint8_t* row = x + n * (int64_t)d + f0;
  if (VEC) {                                            // d % 16 == 0 and x 16-byte aligned: the whole group is inside
    v = *reinterpret_cast<const uint4*>(row);
    v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
  } else {
    uint32_t w[4] = {0, 0, 0, 0};
    for (int q = 0; q < 16; ++q)
      if (f0 + q < d) w[q >> 2] |= (uint32_t)(row[q] ^ 0x80u) << (8 * (q & 3));
    v = make_uint4(w[0], w[1], w[2], w[3]);
  }
  return v;
}

// *p += v: an int64 atomic when several workgroups add into the element, a plain read-modify-write when this one owns it
template <bool ATOMIC>
__device__ __forceinline__ void add_i64(long long* p, long long v, std::integral_constant<bool, ATOMIC>) {
  if (ATOMIC) atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
  else *p += v;
}

template <bool VEC, bool ATOMIC>
__global__ void __launch_bounds__(GTHREADS) gram_u8_i64(const uint8_t* __restrict__ x, int64_t n, int d, int tiles_1d, int64_t rows,
                                                        long long* __restrict__ gram, long long* __restrict__ colsum) {
  // 2 x 8 KB staging panels during the main loop; the 128 x 129 int32 tile in the epilogue
  __shared__ __attribute__((aligned(16))) int smem[GT * CPAD];
  uint8_t* As = reinterpret_cast<uint8_t*>(smem);
  uint8_t* Bs = As + GT * GK;

  // triangular tile index -> (bi, bj), bi <= bj
  int t = blockIdx.x, bi = 0;
  while (t >= tiles_1d - bi) { t -= tiles_1d - bi; ++bi; }
  const int bj = bi + t;
  const bool diag = bi == bj;
  const int i0 = bi * GT, j0 = bj * GT;
  const int64_t k_begin = (int64_t)blockIdx.y * rows;
  const int64_t k_end = min(n, k_begin + rows);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // loader role: threads 0..127 fill panel A (features i0..), 128..255 panel B (features j0..; idle on a diagonal tile, whose B is A).
  // A thread owns 16 consecutive features (fg) of 4 consecutive images (ig) of each stage.
  const int panel = tid >> 7, u = tid & 127, ig = u & 15, fg = u >> 4;
  const bool loader = panel == 0 || !diag;
  const int fbase = (panel == 0 ? i0 : j0) + fg * 16;
  uint8_t* P = panel == 0 ? As : Bs;
  // MFMA role: wave quarter (wi, wj), lane (r, h)
  const int wi = wave & 1, wj = wave >> 1, r = lane & 31, h = lane >> 5;
  const uint8_t* Bsrc = diag ? As : Bs;

  v16i acc[2][2];
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b)
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0;
  int cs[16];                                           // column sums of this thread's 16 features (diagonal tiles, panel A)
  for (int q = 0; q < 16; ++q) cs[q] = 0;

  uint4 img[4];
  for (int m = 0; m < 4; ++m)
    img[m] = loader ? load16<VEC>(x, k_begin + ig * 4 + m, k_end, d, fbase) : make_uint4(0, 0, 0, 0);

  for (int64_t k0 = k_begin; k0 < k_end; k0 += GK) {
    // transpose 4 images x 16 features into 16 words of 4 images each (word q = feature fbase + q)
    uint32_t wq[16];
    for (int q = 0; q < 16; ++q)
      wq[q] = byte_of(img[0], q) | (byte_of(img[1], q) << 8) | (byte_of(img[2], q) << 16) | (byte_of(img[3], q) << 24);
    if (diag && panel == 0)
      for (int q = 0; q < 16; ++q) cs[q] += sbyte_sum(wq[q]);
    __syncthreads();                                    // the previous stage's fragment reads are done
    if (loader)
      for (int q = 0; q < 16; ++q)
        *reinterpret_cast<uint32_t*>(P + panel_off(fg * 16 + q, ig >> 2) + (ig & 3) * 4) = wq[q];
    __syncthreads();
    if (k0 + GK < k_end)                                // next stage's global loads fly under this stage's MFMAs
      for (int m = 0; m < 4; ++m)
        img[m] = loader ? load16<VEC>(x, k0 + GK + ig * 4 + m, k_end, d, fbase) : make_uint4(0, 0, 0, 0);
    for (int kk = 0; kk < GK / 32; ++kk) {
      // lane half h takes images 32kk + 16h .. +15 of its feature row, in the same byte order for A and B: whatever k order the
      // instruction assigns to the 16 bytes of a lane half, A and B agree on it, so the product sums over exactly these 32 images
      v4i fa[2], fb[2];
      for (int a = 0; a < 2; ++a)
        fa[a] = *reinterpret_cast<const v4i*>(As + panel_off(wi * 64 + a * 32 + r, 2 * kk + h));
      for (int b = 0; b < 2; ++b)
        fb[b] = *reinterpret_cast<const v4i*>(Bsrc + panel_off(wj * 64 + b * 32 + r, 2 * kk + h));
      for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[a], fb[b], acc[a][b], 0, 0, 0);
    }
  }

  if (diag && panel == 0)
    for (int q = 0; q < 16; ++q)
      if (fbase + q < d) atomicAdd(reinterpret_cast<unsigned long long*>(colsum + fbase + q), (unsigned long long)(long long)cs[q]);

  // epilogue: accumulators -> LDS tile C[i][j] (32x32 C/D map: column lane & 31, row (e & 3) + 8 (e >> 2) + 4 h), then int64 adds of
  // whole rows: C into gram[i0 + i][j0 + j], and (off the diagonal) C^T into gram[j0 + j][i0 + i]
  __syncthreads();
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b)
      for (int e = 0; e < 16; ++e)
        smem[(wi * 64 + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * h) * CPAD + wj * 64 + b * 32 + r] = acc[a][b][e];
  __syncthreads();
  const int i_lim = min(GT, d - i0), j_lim = min(GT, d - j0);
  for (int e = tid; e < GT * GT; e += GTHREADS) {
    const int row = e >> 7, col = e & (GT - 1);
    if (row < i_lim && col < j_lim)
      add_i64(gram + (int64_t)(i0 + row) * d + j0 + col, (long long)smem[row * CPAD + col], std::integral_constant<bool, ATOMIC>());
  }
  if (!diag)
    for (int e = tid; e < GT * GT; e += GTHREADS) {
      const int jj = e >> 7, ii = e & (GT - 1);
      if (jj < j_lim && ii < i_lim)
        add_i64(gram + (int64_t)(j0 + jj) * d + i0 + ii, (long long)smem[ii * CPAD + jj], std::integral_constant<bool, ATOMIC>());
    }
}

}  // namespace

extern "C" {

int tg_gram_u8_i64(const uint8_t* x, int64_t n, int d, int64_t* gram, int64_t* colsum, void* stream) {
  TG_REQUIRE(x && gram && colsum && n >= 0 && d > 0, "gram_u8_i64: bad args (n %lld, d %d)", (long long)n, d);
  if (n == 0) return TG_OK;
  const int tiles_1d = (d + GT - 1) / GT;
  const int64_t tiles = (int64_t)tiles_1d * (tiles_1d + 1) / 2;
  TG_REQUIRE(tiles <= 0x7fffffff, "gram_u8_i64: d %d too large", d);
  // image ranges: enough for the int32 window, and about GRAM_TARGET_BLOCKS workgroups while each keeps >= GRAM_ROWS_MIN images
  const int64_t s_min = (n + GRAM_ROWS_MAX - 1) / GRAM_ROWS_MAX;
  const int64_t s_par = std::min<int64_t>((GRAM_TARGET_BLOCKS + tiles - 1) / tiles, (n + GRAM_ROWS_MIN - 1) / GRAM_ROWS_MIN);
  const int64_t s = std::max<int64_t>(s_min, s_par);
  int64_t rows = (n + s - 1) / s;
  rows = (rows + GK - 1) / GK * GK;                     // <= GRAM_ROWS_MAX (a multiple of GK)
  const int64_t splits = (n + rows - 1) / rows;
  TG_REQUIRE(splits <= 65535, "gram_u8_i64: n %lld too large", (long long)n);
  hipStream_t st = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_IGEMM, (double)n * d * (d + 1), (double)n * d + 8.0 * d * (d + 1), st);
  const bool vec = d % 16 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  dim3 grid((unsigned)tiles, (unsigned)splits);
  long long* g = reinterpret_cast<long long*>(gram);
  long long* c = reinterpret_cast<long long*>(colsum);
  if (vec && splits > 1)
    hipLaunchKernelGGL((gram_u8_i64<true, true>), grid, dim3(GTHREADS), 0, st, x, n, d, tiles_1d, rows, g, c);
  else if (vec)
    hipLaunchKernelGGL((gram_u8_i64<true, false>), grid, dim3(GTHREADS), 0, st, x, n, d, tiles_1d, rows, g, c);
  else if (splits > 1)
    hipLaunchKernelGGL((gram_u8_i64<false, true>), grid, dim3(GTHREADS), 0, st, x, n, d, tiles_1d, rows, g, c);
  else
    hipLaunchKernelGGL((gram_u8_i64<false, false>), grid, dim3(GTHREADS), 0, st, x, n, d, tiles_1d, rows, g, c);
  TG_CHECK_LAUNCH("gram_u8_i64");
  return TG_OK;
}

}  // extern "C"
