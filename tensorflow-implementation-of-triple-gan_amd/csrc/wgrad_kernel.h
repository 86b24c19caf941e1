// The generic filter-gradient kernel (wgrad_f32_kernel) and its parameter block; included by igemm.hip only.
#pragma once
#include "tg_common.h"
#include "tg_mfma.h"

namespace {

using namespace tgm;

// ------------------------------------------------------------------------------------------------
// filter gradient: rows = reduction channel c of `in`, cols = n of `dout`, reduction over pixels.
// LDS tiles are the natural NHWC rows [32 px][CT] / [32 px][NT]; the MFMA k index of step s, lane half h
// is pixel s+16h, read with conflict-free ds_read_b32 (32 consecutive dwords per lane half).
// ------------------------------------------------------------------------------------------------
struct WgradParams {
  const float* in;
  const float* dout;
  float* slab;
  tg_igemm_desc d;
  int M, n_split, px_per_split, c_tiles, n_tiles;
  uint32_t in_bytes, dout_bytes;
};

template <int CT, int NT, int WAVES_C, int WAVES_N, int WAVES_K, bool BF16>
__global__ void __launch_bounds__(256, 2) wgrad_f32_kernel(WgradParams p) {
  static_assert(WAVES_C * WAVES_N * WAVES_K == 4, "4 waves");
  constexpr int WC = CT / WAVES_C, WN = NT / WAVES_N, MI = WC / 32, NI = WN / 32;
  constexpr int AR = CT / 32, BR = NT / 32;            // 16-B loads per thread per tile
  constexpr int ASEG = CT / 4, BSEG = NT / 4;          // 16-B segments per pixel row
  constexpr int TILE = BK * (CT + NT);
  // bf16 operands, 128 x 128 tiles (the classifier's large layers): both LDS images hold bf16 in 256-byte pixel rows — converted once on
  // the global -> LDS path — and the pixel-major (K-major) fragments are read with the transposing ds_read_b64_tr_b16: two reads per
  // 32x32x16 fragment instead of eight ds_read_b32 + four conversions, half the LDS bytes.  16-byte chunk index XOR-swizzled by
  // ((row & 3) << 2) | ((row >> 2) & 3): row stores and transposed reads are then both conflict-free.  Other tile shapes keep fp32 images.
  constexpr bool TR = BF16 && CT == 128 && NT == 128;
  constexpr int RED = (WAVES_K > 1) ? (WAVES_K - 1) * 64 * 16 * MI * NI * WAVES_C * WAVES_N : 0;
  constexpr int SM = (2 * TILE > RED ? 2 * TILE : RED) + 8 * BK;
  __shared__ __attribute__((aligned(16))) float smem[SM];
  int* tbl = reinterpret_cast<int*>(smem + (2 * TILE > RED ? 2 * TILE : RED));   // [4 slots][2][BK]: in_off, out_off of pixel tile t in slot t & 3

  const tg_igemm_desc& d = p.d;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // XCD-aware order: consecutive logical workgroups (the tiles and the 9 taps of one pixel split, which stream the same
  // `dout` rows and neighbouring `in` rows at the same pace) run on ONE XCD and meet in its L2
  int b = xcd_remap(blockIdx.x, gridDim.x);
  const int nt = b % p.n_tiles; b /= p.n_tiles;
  const int ct = b % p.c_tiles; b /= p.c_tiles;
  const int tap = b % d.n_taps;
  const int split = b / d.n_taps;
  const int c0 = ct * CT, n0 = nt * NT;
  const int p_begin = split * p.px_per_split;
  const int p_end = min(p.M, p_begin + p.px_per_split);
  const int nk = (p_end > p_begin) ? (p_end - p_begin + BK - 1) / BK : 0;
  const int dy = d.dy[tap], dx = d.dx[tap];

  // threads < BK walk their pixel (img, vy, vx) forward by BK per K-tile instead of dividing: the table fill sits on
  // wave 0's path to the barrier, two integer divisions per tile cost ~10 % of the MFMA time.
  int f_img = 0, f_vy = 0, f_vx = 0, f_px = p_begin + tid;
  if (tid < BK) {
    const int hw = d.h_v * d.w_v;
    f_img = f_px / hw;
    const int rem = f_px - f_img * hw;
    f_vy = rem / d.w_v;
    f_vx = rem - f_vy * d.w_v;
  }
  auto fill_tbl = [&](int it) {          // threads < BK: offsets of pixel tile `it`; MUST be called for it = 0, 1, 2, ... in order
    uint32_t io = OOB_OFF, oo = OOB_OFF;
    if (f_px < p_end) {
      const int iy = f_vy * d.s_y + dy, ix = f_vx * d.s_x + dx;
      if ((unsigned)iy < (unsigned)d.h_in && (unsigned)ix < (unsigned)d.w_in)
        io = (uint32_t)(((f_img * d.h_in + iy) * d.w_in + ix) * d.ld_in) * 4u;
      oo = (uint32_t)(((f_img * d.h_out + f_vy * d.os_y + d.oo_y) * d.w_out + f_vx * d.os_x + d.oo_x) * d.ld_out) * 4u;
    }
    tbl[(it & 3) * 2 * BK + tid] = (int)io;
    tbl[(it & 3) * 2 * BK + BK + tid] = (int)oo;
    f_px += BK;
    f_vx += BK;
    while (f_vx >= d.w_v) { f_vx -= d.w_v; ++f_vy; }
    while (f_vy >= d.h_v) { f_vy -= d.h_v; ++f_img; }
  };

  const int aseg = tid % ASEG, arow = tid / ASEG;      // rows advance by 256/ASEG per pass
  const int bseg = tid % BSEG, brow = tid / BSEG;
  // both operands through buffer descriptors: masked pixels carry OOB_OFF and read zeros without a branch, so the
  // loads stay in flight behind the MFMAs (see igemm_f32_kernel)
  const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in), 0, p.in_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_do = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.dout), 0, p.dout_bytes, 0x00020000);
  const uint32_t a_add = (uint32_t)(c0 + aseg * 4) * 4u, b_add = (uint32_t)(n0 + bseg * 4) * 4u;
  u32x4 ra[AR], rb[BR];
  auto gload = [&](int it) {
    const int* ti = tbl + (it & 3) * 2 * BK;
#pragma unroll
    for (int j = 0; j < AR; ++j) ra[j] = __builtin_amdgcn_raw_buffer_load_b128(rs_in, (uint32_t)ti[arow + j * (256 / ASEG)] + a_add, 0, 0);
#pragma unroll
    for (int j = 0; j < BR; ++j) rb[j] = __builtin_amdgcn_raw_buffer_load_b128(rs_do, (uint32_t)ti[BK + brow + j * (256 / BSEG)] + b_add, 0, 0);
  };
  auto sstore = [&](int buf) {
    float* a = smem + buf * TILE;
    float* bb = a + BK * CT;
    if constexpr (TR) {
      unsigned char* a8 = reinterpret_cast<unsigned char*>(a);
      unsigned char* b8 = a8 + BK * 256;
#pragma unroll
      for (int j = 0; j < AR; ++j) {
        const int row = arow + j * (256 / ASEG);
        *reinterpret_cast<u32x2*>(a8 + swz256(row, aseg >> 1) + 8 * (aseg & 1)) = pack4(ra[j]);
      }
#pragma unroll
      for (int j = 0; j < BR; ++j) {
        const int row = brow + j * (256 / BSEG);
        *reinterpret_cast<u32x2*>(b8 + swz256(row, bseg >> 1) + 8 * (bseg & 1)) = pack4(rb[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < AR; ++j) *reinterpret_cast<u32x4*>(a + (arow + j * (256 / ASEG)) * CT + aseg * 4) = ra[j];
#pragma unroll
      for (int j = 0; j < BR; ++j) *reinterpret_cast<u32x4*>(bb + (brow + j * (256 / BSEG)) * NT + bseg * 4) = rb[j];
    }
  };

  const int wk = wave % WAVES_K;
  const int wcn = wave / WAVES_K;
  const int wc0 = (wcn / WAVES_N) * WC, wn0 = (wcn % WAVES_N) * WN;
  f32x16 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  // same two-deep software pipeline as igemm_f32_kernel: registers hold tile it+1, LDS buffer `buf` tile it.  The offset
  // table has 4 slots: iteration it reads slot (it+2)&3 for its loads and fills slot (it+3)&3 (last read two iterations
  // ago) before the barrier that publishes it.
  const int half = lane >> 5, col = lane & 31;
  int buf = 0;
  if (nk > 0) {
    if (tid < BK) { fill_tbl(0); if (nk > 1) fill_tbl(1); if (nk > 2) fill_tbl(2); }
    __syncthreads();
    gload(0);
    sstore(0);
    if (nk > 1) gload(1);
    __syncthreads();
  }
  for (int it = 0; it < nk; ++it) {
    if (it + 1 < nk) sstore(buf ^ 1);
    if (it + 2 < nk) gload(it + 2);
    if (tid < BK && it + 3 < nk) fill_tbl(it + 3);
    const float* A = smem + buf * TILE + (16 * half) * CT + wc0 + col;
    const float* B = smem + buf * TILE + BK * CT + (16 * half) * NT + wn0 + col;
    if constexpr (TR) {
      // fragment of lane (column i = lane & 31, k-group h = lane >> 5): pixels 16G + 8h + {0..7} of channel (tile column) i.  A transposed
      // read serves 16 lanes with a block of 4 pixel rows x 16 channels: lane 4q + p of the group addresses row q, channels 4p..4p+3 and
      // receives the four rows of channel (lane & 15); two blocks (rows +0..3, +4..7) make the eight k values.
      const unsigned char* a8 = reinterpret_cast<const unsigned char*>(smem + buf * TILE);
      const unsigned char* b8 = a8 + BK * 256;
      const int q = (lane >> 2) & 3, cq = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);        // row within the block, first channel this lane addresses
#pragma unroll
      for (int G = wk; G < BK / 16; G += WAVES_K) {
        bf16x8 a[MI], bv[NI];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          const int cs = wc0 + mi * 32 + cq;
          const int r0 = 16 * G + 8 * half + q;
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a8 + swz256(r0, cs >> 3) + 8 * ((cs >> 2) & 1)));
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a8 + swz256(r0 + 4, cs >> 3) + 8 * ((cs >> 2) & 1)));
          a[mi] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
        }
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
          const int cs = wn0 + ni * 32 + cq;
          const int r0 = 16 * G + 8 * half + q;
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(b8 + swz256(r0, cs >> 3) + 8 * ((cs >> 2) & 1)));
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(b8 + swz256(r0 + 4, cs >> 3) + 8 * ((cs >> 2) & 1)));
          bv[ni] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
        }
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi], bv[ni], acc[mi][ni], 0, 0, 0);
      }
    } else if constexpr (BF16) {
      // lane half h supplies pixels 16G + 8h + {0..7} of 16-pixel group G (eight conflict-free ds_read_b32 per fragment)
      const float* Ab = smem + buf * TILE + (8 * half) * CT + wc0 + col;
      const float* Bb = smem + buf * TILE + BK * CT + (8 * half) * NT + wn0 + col;
#pragma unroll
      for (int G = wk; G < BK / 16; G += WAVES_K) {
        bf16x8 a[MI], bv[NI];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int j = 0; j < 8; ++j) a[mi][j] = (__bf16)Ab[(16 * G + j) * CT + mi * 32];
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
          for (int j = 0; j < 8; ++j) bv[ni][j] = (__bf16)Bb[(16 * G + j) * NT + ni * 32];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi], bv[ni], acc[mi][ni], 0, 0, 0);
      }
    } else {
#pragma unroll
    for (int s = wk; s < 16; s += WAVES_K) {
      float a[MI], bv[NI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) a[mi] = A[s * CT + mi * 32];
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) bv[ni] = B[s * NT + ni * 32];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi], bv[ni], acc[mi][ni], 0, 0, 0);
    }
    }
    __syncthreads();
    buf ^= 1;
  }

  if (WAVES_K > 1) {   // cross-wave reduction of the split reduction (small-channel layers)
    float* red = smem;
    __syncthreads();
    if (wk > 0) {
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            red[((((wk - 1) * WAVES_C * WAVES_N + wcn) * MI * NI + mi * NI + ni) * 16 + r) * 64 + lane] = acc[mi][ni][r];
    }
    __syncthreads();
    if (wk == 0) {
#pragma unroll
      for (int k = 1; k < WAVES_K; ++k)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r)
              acc[mi][ni][r] += red[((((k - 1) * WAVES_C * WAVES_N + wcn) * MI * NI + mi * NI + ni) * 16 + r) * 64 + lane];
    }
  }
  if (wk == 0) {
    float* out = p.slab + ((int64_t)(split * d.n_taps + tap) * d.ld_in) * d.c_out;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int c = c0 + wc0 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          int n = n0 + wn0 + ni * 32 + col;
          if (c < d.ld_in && n < d.c_out) out[(int64_t)c * d.c_out + n] = acc[mi][ni][r];
        }
  }
}

}  // namespace
