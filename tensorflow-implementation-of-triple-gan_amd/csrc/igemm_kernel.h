// The generic implicit-GEMM convolution kernel (igemm_f32_kernel) and its parameter block; included by igemm.hip only, which holds the
// parameter packing, routing, dispatch and C ABI.  The file comment of igemm.hip describes the CDNA4 mapping.
#pragma once
#include "tg_common.h"
#include "tg_device.h"
#include "tg_mfma.h"

namespace {

using namespace tgm;

constexpr int LDT = 36;   // padded LDS row stride (floats)
constexpr int LDH = 80;   // bf16 variant: LDS row stride in BYTES (32 bf16 = 64 B + 16 B pad: the 16 rows of a ds_read_b128 lane group hit 16 different 16-B bank slots)

#ifdef TG_STAMP
// Diagnostic build (never shipped): per-phase cycle sums of the K loop for a few workgroups, wave 0, read back with
// tg_debug_read_stamps.  Stamp values go only to this buffer; no output depends on them.
__device__ unsigned long long tg_stamps[8 * 8];
__device__ unsigned long long tg_block_times[3 * 8192];   // per workgroup: start, end (s_memrealtime, 100 MHz), HW ids
#define STAMP(var)                                                                 \
  do {                                                                             \
    __builtin_amdgcn_sched_barrier(0);                                             \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var)::"memory");    \
    __builtin_amdgcn_sched_barrier(0);                                             \
  } while (0)
#else
#define STAMP(var) do {} while (0)
#endif

constexpr int MAX_SUB = 4;   // sub-problems per launch (the 4 output parities of a stride-2 transposed conv / dgrad)

// kernel-side view of one tg_igemm_desc: tap tables repacked to one dword per tap so that the (block-uniform) tap
// lookup is a scalar s_load_dword — int8/int16 arrays indexed dynamically compile to VECTOR byte loads plus a
// vmcnt wait at the top of every K-tile.
struct SubDesc {
  int32_t h_v, w_v, s_y, s_x, h_out, w_out, ld_out, os_y, os_x, oo_y, oo_x, n_store, n_taps, act;
  float alpha;
  int32_t n_group;
  int32_t taps[TG_MAX_TAPS];     // (tapw << 16) | ((dy & 0xff) << 8) | (dx & 0xff)
};

struct IgemmParams {
  const float* in;
  const float* w;
  const float* bias;
  float* out;
  SubDesc d[MAX_SUB];
  int64_t w_sn, w_st;
  int n_img, h_in, w_in, ld_in, c_out;
  int n_sub, M, m_tiles, n_tiles;
  uint32_t in_bytes, w_bytes, out_bytes;
  double* colsum;                 // COLSUM variant: [nseg][c_out] fp64 accumulators (zeroed by the launcher)
  const float* ymul;              // COLSUM variant, optional: out = acc * act'(ymul[same position]) (tg_igemm_actsum_*)
  int ymul_act;
  float ymul_alpha;
  int stat2;                      // COLSUM variant: 2 = the stored value is the accumulator (a gradient dy) and colsum is [nseg][2][c_out]: sums of dy and of
                                  // dy * ymul (a batch norm's backward statistics, tg_igemm_bnbwdstat_*); 1 = the stored value is v = act(acc + bias) and colsum is [nseg][2][c_out]: sums of v and of v*v
                                  // (statistics of a batch norm behind the layer, tg_igemm_bnstat_*)
  int nseg, seg_rows[8];
  // tg_igemm_labels_*: a _conv_cond_concat follows (Model/modle_base.py:239-244) — the output buffer is the concatenated tensor and the workgroups of
  // the last column tile also write channels [lab_c0, lab_c0 + lab_n) = the image's label vector and zeros from there up to ld_out
  const float* lab;
  int lab_n, lab_c0;
  // ---- work units (tg::igemm_schedule, geom.cpp).  A unit is one output tile over a K range; tiles whose K range is cut into ks > 1
  // units leave raw partial accumulators in `ws` and are finished by the fix-up launch (same kernel, FIXUP = true).
  int n_units;                    // grid of the main launch
  int n_fix;                      // grid of the fix-up launch (tiles that were cut), 0: none
  int nfull;                      // pat_len == 0 (one sub-problem): tiles [0, nfull) are whole, tiles [nfull, T) are cut into ks[0] units
  int ks[MAX_SUB];                // units per tile of each sub-problem
  int pat_len;                    // > 0: every tile index owns pat_len consecutive units, unit w of the pattern = (sub, K segment)
  int n_pat_split;                // pattern entries that are partial (per tile index: that many ws slots)
  int n_split_sub;                // sub-problems with ks > 1 (fix-up grid = tiles * n_split_sub)
  int8_t pat_sub[16], pat_k[16], pat_slot[16];      // pat_slot: ws slot of the entry inside its tile index's group, -1: whole tile
  int8_t split_sub[MAX_SUB], first_slot[MAX_SUB];   // the i-th cut sub-problem and the slot of its first K segment
  float* ws;
};

// ================================================================================================================================
// The stages of igemm_f32_kernel, in the order its body runs them.  All are inlined; they take the scalars they need by value.
// ================================================================================================================================

// ---- work unit ---------------------------------------------------------------------------------------------------------------------
// One workgroup = one unit: an output tile of a sub-problem over K segment kseg of kcut.
struct Unit {
  int sub, tile;     // sub-problem; tile index (column tile minor)
  int kseg, kcut;
  int slot;          // workspace slot of the unit's partial sums (FIXUP: of the tile's first K segment); -1: a whole tile, epilogue here
};

// Unit -> (sub-problem, tile, K segment).  Several sub-problems (the 9/6/6/4-tap parities of a stride-2 transposed conv) and / or cut
// tiles: tile-index-major, pattern-minor — every tile index owns pat_len units (sub-problem s contributes ks[s] of them) — and the
// order inside the pattern rotates every 32 workgroups: workgroups go to the 32 compute units of an XCD round-robin, all resident at
// once for these small launches, so with a fixed order unit j would get pattern entry j % pat_len every time (measured: the units
// holding only 9-tap workgroups finish at 190 us, the median at 100); rotating gives every unit the same mix.
// FIXUP: one workgroup per cut tile, in the order the main launch numbered their slots.
template <bool FIXUP>
__device__ __forceinline__ Unit decode_unit(const IgemmParams& p, int bid) {
  Unit u{0, 0, 0, 1, -1};
  if constexpr (FIXUP) {
    if (p.pat_len > 0) {
      u.tile = bid / p.n_split_sub;
      const int j = bid - u.tile * p.n_split_sub;
      u.sub = p.split_sub[j];
      u.slot = u.tile * p.n_pat_split + p.first_slot[j];
    } else {
      u.tile = p.nfull + bid;
      u.slot = bid * p.ks[0];
    }
    u.kcut = p.ks[u.sub];
  } else {
    const int lid = xcd_remap(bid, p.n_units);
    if (p.pat_len > 0) {
      const int L = p.pat_len;
      u.tile = lid / L;
      const int w = (32 % L == 0) ? (lid + (lid >> 5)) % L : lid - u.tile * L;
      u.sub = p.pat_sub[w]; u.kseg = p.pat_k[w]; u.kcut = p.ks[u.sub];
      u.slot = p.pat_slot[w] < 0 ? -1 : u.tile * p.n_pat_split + p.pat_slot[w];
    } else if (lid < p.nfull) {
      u.tile = lid;
    } else {
      const int v = lid - p.nfull;
      u.kcut = p.ks[0];
      u.tile = p.nfull + v / u.kcut;
      u.kseg = v - (u.tile - p.nfull) * u.kcut;
      u.slot = v;
    }
  }
  return u;
}

// ---- row table ---------------------------------------------------------------------------------------------------------------------
// Thread `row` < BM writes tile row `row` (output position m): the element offset of its image in the gathered tensor, the window origin
// (y0, x0) the taps are added to, and the byte offset of its output pixel.  A row beyond M gets an origin no tap brings into the image
// and OOB_OFF as its output offset.
__device__ __forceinline__ void fill_row_table(int row, int m, int M, const SubDesc& d, int h_in, int w_in, int ld_in, int* t_base, int* t_y, int* t_x,
                                               int* t_out) {
  int base = 0, y0 = -30000, x0 = 0, oo = (int)OOB_OFF;
  if (m < M) {
    int hw = d.h_v * d.w_v;
    int img = m / hw, rem = m - img * hw;
    int vy = rem / d.w_v, vx = rem - vy * d.w_v;
    base = img * h_in * w_in * ld_in;
    y0 = vy * d.s_y;
    x0 = vx * d.s_x;
    oo = ((img * d.h_out + vy * d.os_y + d.oo_y) * d.w_out + vx * d.os_x + d.oo_x) * d.ld_out * 4;   // byte offset
  }
  t_base[row] = base; t_y[row] = y0; t_x[row] = x0; t_out[row] = oo;
}

// ---- partial sums of a cut tile ---------------------------------------------------------------------------------------------------------
// A unit's accumulators lie in the workspace as they lie in the registers, 16 B per lane (1 KB per wave-instruction): slot s holds
// MI * NI * 4 float4 pieces per thread, piece (mi, ni, q) of thread t at float4 index (s * MI * NI * 4 + (mi * NI + ni) * 4 + q) * 256 + t.
template <int MI, int NI>
__device__ __forceinline__ f32x4* ws_slot(float* ws, int slot, int tid) { return reinterpret_cast<f32x4*>(ws) + ((int64_t)slot * (MI * NI * 4)) * 256 + tid; }
template <int NI>
__device__ __forceinline__ constexpr int ws_piece(int mi, int ni, int q) { return ((mi * NI + ni) * 4 + q) * 256; }

// a cut tile's unit: the accumulators go to slot `slot`; the fix-up launch adds the tile's K segments up and runs the epilogue
template <int MI, int NI>
__device__ __forceinline__ void spill_partials(float* ws, int slot, int tid, const f32x16 (&acc)[MI][NI]) {
  f32x4* dst = ws_slot<MI, NI>(ws, slot, tid);
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 v = {acc[mi][ni][4 * q], acc[mi][ni][4 * q + 1], acc[mi][ni][4 * q + 2], acc[mi][ni][4 * q + 3]};
        dst[ws_piece<NI>(mi, ni, q)] = v;
      }
}

// the fix-up launch: the accumulators are the sum of the tile's kcut partials from slot `slot` on, in K-segment order — the result does
// not depend on which unit finished first
template <int MI, int NI>
__device__ __forceinline__ void sum_partials(float* ws, int slot, int kcut, int tid, f32x16 (&acc)[MI][NI]) {
  for (int k = 0; k < kcut; ++k) {
    const f32x4* src = ws_slot<MI, NI>(ws, slot + k, tid);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 v = src[ws_piece<NI>(mi, ni, q)];
          acc[mi][ni][4 * q] += v[0]; acc[mi][ni][4 * q + 1] += v[1]; acc[mi][ni][4 * q + 2] += v[2]; acc[mi][ni][4 * q + 3] += v[3];
        }
  }
}

// ---- statistics epilogues (COLSUM) --------------------------------------------------------------------------------------------------
// Mean-only-BN and batch-norm variants.  The pixel operand was the MFMA row operand, so a lane holds ONE output channel and its 16
// registers hold rows: storing from that layout means 64 dword stores per lane (and, for tg_igemm_actsum_*, 64 dword loads of the
// activation).  The tile goes through LDS instead (the operand tiles are dead after the K loop) and leaves it row-wise: every thread
// moves 16-B pieces of pixel rows — coalesced stores, coalesced activation loads — and the column sums are taken from LDS by
// (column, row-range) threads.  Sums are fp32 per thread and per workgroup, then ONE fp64 atomic per (column, segment, moment) and tile.
template <int BN>
constexpr int TLD = BN + 4;                               // LDS row stride of the row-wise tile (floats)

// A tile may straddle ONE application boundary (every segment has at least BM rows: launcher check): tile rows below `bnd` belong to
// segment `seg`, the others — if `two` — to seg + 1.
struct SegSplit {
  int seg, bnd;      // bnd >= 1; >= BM when the tile lies inside one segment
  bool two;
};

template <int BM>
__device__ __forceinline__ SegSplit locate_segment(const int (&seg_rows)[8], int nseg, int m0) {
  int seg = 0, acc_rows = seg_rows[0];
  while (seg < nseg - 1 && m0 >= acc_rows) acc_rows += seg_rows[++seg];
  const int bnd = acc_rows - m0;
  return SegSplit{seg, bnd, bnd < BM && seg + 1 < nseg};
}

// the accumulators (lane = channel, registers = rows) -> the row-wise tile in LDS
template <int BM, int BN, int MI, int NI>
__device__ __forceinline__ void tile_to_lds(float* tile, const f32x16 (&acc)[MI][NI], int wm0, int wn0, int lane) {
  static_assert(BM * TLD<BN> <= 2 * BM * LDT + 2 * BN * LDT, "the output tile must fit into the operand tiles' LDS");
  const int half = lane >> 5, col = lane & 31;
#pragma unroll
  for (int ni = 0; ni < NI; ++ni)
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        tile[(wm0 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * TLD<BN> + wn0 + ni * 32 + col] = acc[mi][ni][r];
}

// The atomics of every statistics flavour.  Column n of a tile adds its sums over the rows of segment sg.seg — s[0], and with `moments`
// ([nseg][2][c_out] accumulators) the second sum q[0] behind it — and, where the tile straddles a boundary, s[1] / q[1] to the next segment.
__device__ __forceinline__ void add_colsums(double* colsum, int c_out, int n, int n_store, SegSplit sg, bool moments, const float (&s)[2], const float (&q)[2]) {
  if (n >= n_store) return;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (j == 1 && !sg.two) break;
    double* dst = colsum + ((int64_t)(sg.seg + j) * (moments ? 2 : 1)) * c_out + n;
    atomicAdd(dst, (double)s[j]);
    if (moments) atomicAdd(dst + c_out, (double)q[j]);
  }
}

// Row-wise pass: piece i of the tile is the 16 B of tile row rl, columns n .. n + 3 (4 cg .. 4 cg + 3 of the tile); `off` is its byte offset in
// the output — and in any tensor of the output's layout — or OOB_OFF for a row beyond M / a column group beyond n_store.
struct RowPiece {
  int rl, cg, n;
  uint32_t ro, off;
};

template <int BN>
__device__ __forceinline__ RowPiece row_piece(int i, const uint32_t* t_ob, int n0, int n_store) {
  constexpr int G4 = BN / 4;                              // 16-B pieces per tile row
  RowPiece r;
  r.rl = i / G4; r.cg = i - r.rl * G4;
  r.ro = t_ob[r.rl];
  r.n = n0 + r.cg * 4;
  r.off = ((r.ro & OOB_OFF) || r.n >= n_store) ? OOB_OFF : r.ro + (uint32_t)r.n * 4u;
  return r;
}

// tg_igemm_colsum_*: the tile is stored as it is
template <int BM, int BN>
__device__ __forceinline__ void rows_store(const float* tile, const uint32_t* t_ob, int tid, int n0, int n_store, __amdgpu_buffer_rsrc_t rsrc_o) {
  for (int i = tid; i < BM * (BN / 4); i += 256) {
    const RowPiece r = row_piece<BN>(i, t_ob, n0, n_store);
    const float4 tv = *reinterpret_cast<const float4*>(tile + r.rl * TLD<BN> + r.cg * 4);
    store4(tv.x, tv.y, tv.z, tv.w, rsrc_o, r.off);
  }
}

// tg_igemm_actsum_*: the input gradient times the activation derivative of the layer that produced this conv's input (y: its output);
// the product replaces the tile
template <int BM, int BN>
__device__ __forceinline__ void rows_actsum(float* tile, const uint32_t* t_ob, int tid, int n0, int n_store, __amdgpu_buffer_rsrc_t rsrc_o,
                                            __amdgpu_buffer_rsrc_t rsrc_y, int y_act, float y_alpha) {
  for (int i = tid; i < BM * (BN / 4); i += 256) {
    const RowPiece r = row_piece<BN>(i, t_ob, n0, n_store);
    const float4 tv = *reinterpret_cast<const float4*>(tile + r.rl * TLD<BN> + r.cg * 4);
    float va[4] = {tv.x, tv.y, tv.z, tv.w};
    const u32x4 yb = __builtin_amdgcn_raw_buffer_load_b128(rsrc_y, r.off, 0, 0);          // masked positions read 0
    const uint32_t y0 = yb.x, y1 = yb.y, y2 = yb.z, y3 = yb.w;         // (a bit_cast straight from a vector element reads element 0: take scalars first)
    va[0] *= tgd::act_grad(__builtin_bit_cast(float, y0), y_act, y_alpha);
    va[1] *= tgd::act_grad(__builtin_bit_cast(float, y1), y_act, y_alpha);
    va[2] *= tgd::act_grad(__builtin_bit_cast(float, y2), y_act, y_alpha);
    va[3] *= tgd::act_grad(__builtin_bit_cast(float, y3), y_act, y_alpha);
    *reinterpret_cast<float4*>(tile + r.rl * TLD<BN> + r.cg * 4) = make_float4(va[0], va[1], va[2], va[3]);
    store4(va[0], va[1], va[2], va[3], rsrc_o, r.off);
  }
}

// tg_igemm_bnstat_*: a batch norm behind the layer — bias + activation here, statistics of the result, which replaces the tile; rows
// beyond M must stay exact zeros
template <int BM, int BN>
__device__ __forceinline__ void rows_bnstat(float* tile, const uint32_t* t_ob, int tid, int n0, int n_store, __amdgpu_buffer_rsrc_t rsrc_o,
                                            const float* bias, int act, float alpha) {
  for (int i = tid; i < BM * (BN / 4); i += 256) {
    const RowPiece r = row_piece<BN>(i, t_ob, n0, n_store);
    const float4 tv = *reinterpret_cast<const float4*>(tile + r.rl * TLD<BN> + r.cg * 4);
    float va[4] = {tv.x, tv.y, tv.z, tv.w};
    const bool live = !(r.ro & OOB_OFF);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float t = va[e] + ((bias != nullptr && r.n + e < n_store) ? bias[r.n + e] : 0.f);
      va[e] = live ? tgd::act_fast(t, act, alpha) : 0.f;
    }
    *reinterpret_cast<float4*>(tile + r.rl * TLD<BN> + r.cg * 4) = make_float4(va[0], va[1], va[2], va[3]);
    store4(va[0], va[1], va[2], va[3], rsrc_o, r.off);
  }
}

// tg_igemm_bnbwdstat_*: the stored value is the accumulator (a gradient dy); sums of dy and of dy * x, x read at the output's addresses.
// A thread's pieces all belong to ONE 4-column group (256 % G4 == 0), so its sums stay in registers until the tile is done; then — the
// tile is dead — they go through its LDS as [sum kind][e][thread], and column n0 + 4 cg + e adds up threads cg, cg + G4, ...
template <int BM, int BN>
__device__ __forceinline__ void stats_bnbwdstat(float* tile, const uint32_t* t_ob, int tid, int n0, int n_store, __amdgpu_buffer_rsrc_t rsrc_o,
                                                __amdgpu_buffer_rsrc_t rsrc_x, SegSplit sg, double* colsum, int c_out) {
  constexpr int G4 = BN / 4;
  float bs[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, bq[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (int i = tid; i < BM * G4; i += 256) {
    const RowPiece r = row_piece<BN>(i, t_ob, n0, n_store);
    const float4 tv = *reinterpret_cast<const float4*>(tile + r.rl * TLD<BN> + r.cg * 4);
    const float va[4] = {tv.x, tv.y, tv.z, tv.w};
    const u32x4 xb = __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, r.off, 0, 0);          // masked positions read 0 (and hold acc = 0)
    const uint32_t x0 = xb.x, x1 = xb.y, x2 = xb.z, x3 = xb.w;         // (a bit_cast straight from a vector element reads element 0: take scalars first)
    const float xs[4] = {__builtin_bit_cast(float, x0), __builtin_bit_cast(float, x1), __builtin_bit_cast(float, x2), __builtin_bit_cast(float, x3)};
    const float m0_ = r.rl < sg.bnd ? 1.f : 0.f, m1_ = 1.f - m0_;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float pr = va[e] * xs[e];
      bs[0][e] += m0_ * va[e]; bs[1][e] += m1_ * va[e];
      bq[0][e] += m0_ * pr;    bq[1][e] += m1_ * pr;
    }
    store4(va[0], va[1], va[2], va[3], rsrc_o, r.off);
  }
  __syncthreads();
  static_assert(16 * 256 <= BM * TLD<BN>, "the per-thread sums must fit into the tile");
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    tile[(0 * 4 + e) * 256 + tid] = bs[0][e];
    tile[(1 * 4 + e) * 256 + tid] = bs[1][e];
    tile[(2 * 4 + e) * 256 + tid] = bq[0][e];
    tile[(3 * 4 + e) * 256 + tid] = bq[1][e];
  }
  __syncthreads();
  if (tid < BN) {
    const int cg = tid >> 2, e = tid & 3;
    float s[2] = {0.f, 0.f}, q[2] = {0.f, 0.f};
    for (int t2 = cg; t2 < 256; t2 += G4) {
      s[0] += tile[(0 * 4 + e) * 256 + t2]; s[1] += tile[(1 * 4 + e) * 256 + t2];
      q[0] += tile[(2 * 4 + e) * 256 + t2]; q[1] += tile[(3 * 4 + e) * 256 + t2];
    }
    add_colsums(colsum, c_out, n0 + tid, n_store, sg, true, s, q);
  }
}

// Column sums of the row-wise tile (colsum, actsum, bnstat): thread (column c, part q) adds rows q, q + PARTS, ... of its column (masked rows hold
// exact zeros) — the sum and, for `moments`, the sum of squares, per segment — then one thread per column adds the parts up
template <int BM, int BN>
__device__ __forceinline__ void column_sums(float* tile, int tid, int n0, int n_store, SegSplit sg, bool moments, double* colsum, int c_out) {
  constexpr int PARTS = 256 / BN;
  float* red = tile + BM * TLD<BN>;                       // [4][PARTS][BN] partial sums (two segments; also of the squares), behind the tile
  static_assert(BM * TLD<BN> + 4 * PARTS * BN <= 2 * BM * LDT + 2 * BN * LDT, "partial sums must fit as well");
  {
    const int c = tid % BN, q = tid / BN;
    float s1 = 0.f, s2 = 0.f, q1 = 0.f, q2 = 0.f;
    for (int rl = q; rl < BM; rl += PARTS) {
      const float v = tile[rl * TLD<BN> + c];
      if (rl < sg.bnd) { s1 += v; q1 += v * v; } else { s2 += v; q2 += v * v; }
    }
    red[q * BN + c] = s1;
    red[(PARTS + q) * BN + c] = s2;
    red[(2 * PARTS + q) * BN + c] = q1;
    red[(3 * PARTS + q) * BN + c] = q2;
  }
  __syncthreads();
  if (tid < BN) {
    float s[2] = {0.f, 0.f}, q[2] = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < PARTS; ++k) {
      s[0] += red[k * BN + tid]; s[1] += red[(PARTS + k) * BN + tid];
      q[0] += red[(2 * PARTS + k) * BN + tid]; q[1] += red[(3 * PARTS + k) * BN + tid];
    }
    add_colsums(colsum, c_out, n0 + tid, n_store, sg, moments, s, q);
  }
}

// ---- plain epilogue -------------------------------------------------------------------------------------------------------------------
// The MFMAs were issued with the FILTER as the row operand, so a lane holds ONE output pixel (lane & 31) and its 16 registers hold
// channels 8q + 4h + (0..3): four consecutive channels of that pixel are adjacent in NHWC memory -> 16 dwordx4 stores per lane instead
// of 64 dword stores (measured: the store tail of a 128x128 tile drops from ~36k to ~10k cycles).  +bias, activation; masked rows carry
// an out-of-range byte offset in the row table, masked channel groups get one here, and the buffer range check drops those stores (no
// branches).  ng > 0: grouped columns, column -> (output-pixel parity, channel), see tg_igemm_desc.
// ROLL: the loops over the wave's 32-row and 32-column blocks stay rolled (the accumulators are then indexed in scratch).  The epilogue
// is straight-line code that a workgroup runs once, so it costs what its instruction fetch costs.  In the fix-up launch of 128x128
// tiles, whose workgroups do nothing else, the four blocks as one loop body are a quarter of the code: 21 us per launch, against 31 us
// unrolled and the 23 us of a body of two blocks (profiles/conv_gemm_stages.txt, section 7a).
template <int MI, int NI, bool ROLL>
__device__ __forceinline__ void epilogue_plain(const f32x16 (&acc)[MI][NI], const uint32_t* t_ob, int lane, int wm0, int n_first, __amdgpu_buffer_rsrc_t rsrc_o,
                                               const float* bias, int act, float alpha, int n_store, int ld_out, int w_out, int os_x, int os_y, int ng) {
  constexpr int UNROLL_MI = ROLL ? 1 : MI, UNROLL_NI = ROLL ? 1 : NI;
  const int half = lane >> 5, col = lane & 31;
  const bool vec_ok = (n_store & 3) == 0 && (ld_out & 3) == 0 && (ng & 3) == 0;
#pragma unroll UNROLL_MI
  for (int mi = 0; mi < MI; ++mi) {
    const uint32_t ro = t_ob[wm0 + mi * 32 + col];
#pragma unroll UNROLL_NI
    for (int ni = 0; ni < NI; ++ni) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = n_first + ni * 32 + 8 * q + 4 * half;
        int ch[4];
        uint32_t goff[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (ng > 0) {
            const int g = (n + e) / ng;
            ch[e] = n + e - g * ng;
            goff[e] = (uint32_t)(((g / os_x) * w_out + (g % os_x)) * ld_out) * 4u;
            if (g >= os_x * os_y) ch[e] = n_store;                // padding columns behind the last group: never stored
          } else {
            ch[e] = n + e;
            goff[e] = 0;
          }
        }
        float va[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float t = acc[mi][ni][4 * q + e];
          if (bias != nullptr && ch[e] < n_store) t += bias[ch[e]];
          va[e] = tgd::act_fast(t, act, alpha);
        }
        if (vec_ok) {
          const uint32_t off = ((ro & OOB_OFF) || ch[0] >= n_store) ? OOB_OFF : ro + goff[0] + (uint32_t)ch[0] * 4u;
          store4(va[0], va[1], va[2], va[3], rsrc_o, off);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const uint32_t off = ((ro & OOB_OFF) || ch[e] >= n_store) ? OOB_OFF : ro + goff[e] + (uint32_t)ch[e] * 4u;
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, va[e]), rsrc_o, off, 0, 0);
          }
        }
      }
    }
  }
}

// ---- label epilogue (tg_igemm_labels_*) --------------------------------------------------------------------------------------------------
// The label channels [lab_c0, lab_c0 + lab_n) and the channel padding up to ld_out of the concatenated tensor, written by the waves of
// the last column tile that hold its first columns: lane = output pixel, the two lane halves alternate 16-byte groups.
template <int MI>
__device__ __forceinline__ void epilogue_labels(const uint32_t* t_ob, int lane, int wm0, int m0, int hw, __amdgpu_buffer_rsrc_t rsrc_o, const float* lab,
                                                int lab_n, int lab_c0, int ld_out) {
  const int half = lane >> 5, col = lane & 31;
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int rl = wm0 + mi * 32 + col;
    const uint32_t ro = t_ob[rl];
    const bool live = !(ro & OOB_OFF);
    const float* lrow = lab + (int64_t)((m0 + rl) / hw) * lab_n;
    for (int c4 = lab_c0 + 4 * half; c4 < ld_out; c4 += 8) {
      float va[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ch = c4 + e - lab_c0;
        va[e] = (live && ch < lab_n) ? lrow[ch] : 0.f;
      }
      store4(va[0], va[1], va[2], va[3], rsrc_o, live ? ro + (uint32_t)c4 * 4u : OOB_OFF);
    }
  }
}

#ifdef TG_STAMP
// the five workgroups whose phase stamps are kept (tg_stamps rows), -1: none
__device__ __forceinline__ int stamp_slot() {
  return blockIdx.x == 0 ? 0 : (blockIdx.x == 7 ? 1 : (blockIdx.x == 300 ? 2 : (blockIdx.x == 700 ? 3 : (blockIdx.x == 1500 ? 4 : -1))));
}
#endif

// ================================================================================================================================
// The kernel: decode the unit, fill the row table, run the K pipeline, then spill the partial sums of a cut tile or run one epilogue
// (statistics flavours, or plain + labels).  The K pipeline (set_tap, gload, sstore, compute, ktile, the steady and drain loops) is
// written out in the body: its lambdas share the register stages and the cursor.
// FIXUP = true: the second launch of a schedule with cut tiles — no K loop: the accumulators are the sum (in K-segment order, so
// deterministic) of the partials the main launch left in p.ws, then the SAME epilogue.
template <int BM, int BN, int WAVES_M, int WAVES_N, bool COLSUM, bool BF16, bool FIXUP = false>
__global__ void __launch_bounds__(256, 2) igemm_f32_kernel(IgemmParams p) {
  static_assert(WAVES_M * WAVES_N == 4, "4 waves");
  constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N, MI = WM / 32, NI = WN / 32;
  constexpr int AR = BM / 32, BR = BN / 32;   // 16-B loads per thread per tile
  // register stages of the K pipeline (see the K loop): one for 128x128 tiles, two for the smaller ones, with fp32 and bf16 operands alike
  constexpr int NBUF = 2;                     // LDS buffers per operand
  constexpr int PF = FIXUP ? 1 : (BM * BN >= 128 * 128 ? 1 : 2);
  __shared__ __attribute__((aligned(16))) float smem[NBUF * BM * LDT + NBUF * BN * LDT + 4 * BM];
  float* As = smem;
  float* Bs = smem + NBUF * BM * LDT;
  int* t_base = reinterpret_cast<int*>(smem + NBUF * BM * LDT + NBUF * BN * LDT);
  int* t_y = t_base + BM;
  int* t_x = t_y + BM;
  int* t_out = t_x + BM;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#ifdef TG_STAMP
  unsigned long long t_entry = 0;
  STAMP(t_entry);
  const unsigned long long rt0 = __builtin_amdgcn_s_memrealtime();
#endif
  // ---- stage 1: which unit, and the row table of its tile
  const Unit u = decode_unit<FIXUP>(p, blockIdx.x);
  const int kseg = u.kseg, kcut = u.kcut, slot = u.slot;
  const SubDesc& d = p.d[u.sub];
  const int nt = u.tile % p.n_tiles, mt = u.tile / p.n_tiles;
  const int m0 = mt * BM, n0 = nt * BN;

  if (tid < BM) fill_row_table(tid, m0 + tid, p.M, d, p.h_in, p.w_in, p.ld_in, t_base, t_y, t_x, t_out);
  __syncthreads();

  // ---- K pipeline, set-up: this thread's rows of both operand tiles, the register stages and the LDS writes
  const int seg = tid & 7, lrow = tid >> 3;
  int abase[AR], ay[AR], ax[AR];
#pragma unroll
  for (int j = 0; j < AR; ++j) {
    int r = lrow + 32 * j;
    abase[j] = t_base[r] + seg * 4; ay[j] = t_y[r]; ax[j] = t_x[r];
  }

  // Both operands are read through buffer descriptors with the K-tile position in the SCALAR offset operand:
  //   gathered rows : voffset = byte offset of (pixel, tap) — recomputed once per TAP, not per K-tile — or
  //                   OOB_OFF for an out-of-image tap (the hardware range check returns zeros: no branch, no select);
  //   filter rows   : voffset fixed for the whole kernel;   soffset = (tap, channel chunk) for both.
  // On gfx950 the fp32 MFMA runs on the vector ALUs, so every VALU instruction of the address arithmetic is time the
  // matrix work does not get (stamped build: a wave's load-issue phase is starved for the whole MFMA phase of its SIMD
  // partner).  Per K-tile this loop now issues 8 loads, 8 LDS writes, 16 LDS reads and ~10 scalar instructions.
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in), 0, p.in_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w), 0, p.w_bytes, 0x00020000);
  uint32_t wvoff[BR];
#pragma unroll
  for (int j = 0; j < BR; ++j) wvoff[j] = (uint32_t)(((int64_t)(n0 + lrow + 32 * j) * p.w_sn + seg * 4) * 4);

  u32x4 ra[PF][AR], rb[PF][BR];
  uint32_t avoff[AR];
  const int cchunks = p.ld_in / BK;
  const int nk = d.n_taps * cchunks;
  const int h_in = p.h_in, w_in = p.w_in, ld_in = p.ld_in;
  int w_tap_off = 0;                                    // element offset of the current tap's filter slice

  auto set_tap = [&](int tap) {
    const int tp = d.taps[tap];
    const int dy = (int)(int8_t)(tp >> 8), dx = (int)(int8_t)tp;
    w_tap_off = (tp >> 16) * (int)p.w_st;
#pragma unroll
    for (int j = 0; j < AR; ++j) {
      const int iy = ay[j] + dy, ix = ax[j] + dx;
      const bool ok = (unsigned)iy < (unsigned)h_in && (unsigned)ix < (unsigned)w_in;
      avoff[j] = ok ? (uint32_t)(abase[j] + (iy * w_in + ix) * ld_in) * 4u : OOB_OFF;
    }
  };
  auto gload = [&](int c0, int rs) {                     // rs: register stage (a compile-time constant after unrolling)
    const uint32_t sa = (uint32_t)__builtin_amdgcn_readfirstlane(c0 * 4);
    const uint32_t sw = (uint32_t)__builtin_amdgcn_readfirstlane((w_tap_off + c0) * 4);
#pragma unroll
    for (int j = 0; j < AR; ++j) ra[rs][j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, avoff[j], sa, 0);
#pragma unroll
    for (int j = 0; j < BR; ++j) rb[rs][j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, wvoff[j], sw, 0);
  };
  auto sstore = [&](int buf, int rs) {
    if constexpr (BF16) {
      // bf16 LDS images (round 3): the operands are rounded ONCE on the global -> LDS path (v_cvt_pk_bf16_f32, RNE) and a 32-deep row is
      // 64 bytes — half the LDS bytes of the fp32 image, and the fragments below need no conversion (round 2 converted every fragment
      // on its way LDS -> registers: eight packed conversions per operand fragment next to the MFMAs)
      unsigned char* a = reinterpret_cast<unsigned char*>(As) + (buf * BM + lrow) * LDH + seg * 8;
      unsigned char* b = reinterpret_cast<unsigned char*>(Bs) + (buf * BN + lrow) * LDH + seg * 8;
#pragma unroll
      for (int j = 0; j < AR; ++j) *reinterpret_cast<u32x2*>(a + 32 * j * LDH) = pack4(ra[rs][j]);
#pragma unroll
      for (int j = 0; j < BR; ++j) *reinterpret_cast<u32x2*>(b + 32 * j * LDH) = pack4(rb[rs][j]);
    } else {
      float* a = As + buf * BM * LDT + lrow * LDT + seg * 4;
      float* b = Bs + buf * BN * LDT + lrow * LDT + seg * 4;
#pragma unroll
      for (int j = 0; j < AR; ++j) *reinterpret_cast<u32x4*>(a + 32 * j * LDT) = ra[rs][j];
#pragma unroll
      for (int j = 0; j < BR; ++j) *reinterpret_cast<u32x4*>(b + 32 * j * LDT) = rb[rs][j];
    }
  };

  const int wm0 = (wave / WAVES_N) * WM, wn0 = (wave % WAVES_N) * WN;
  f32x16 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  const int frag = (lane & 31) * LDT + (lane >> 5) * 4;

  // ---- stage 2: the accumulators — the fix-up launch adds up what the cut tile's units left, every other launch runs the K pipeline
  if constexpr (FIXUP) {
    sum_partials<MI, NI>(p.ws, slot, kcut, tid, acc);
  } else {
  // K range of this unit: K-tiles [it0, it1) of the tile's nk (balanced integer cut)
  const int it0 = (int)((int64_t)nk * kseg / kcut), it1 = (int)((int64_t)nk * (kseg + 1) / kcut);

  // Register-staged pipeline over a two-buffer LDS image, PF register stages deep: while tile `it` is multiplied, the loads of tiles
  // it+1 .. it+PF are in flight (tile it+PF is issued at the top of iteration it into the stage that tile it occupied), and tile it+1 is
  // written to the other LDS buffer after the MFMAs (one barrier per K-tile).  PF = 1 is the round-1 scheme: enough for the 128x128 tile
  // (64 MFMAs = 1.7 us per K-tile cover a global-load latency) with two workgroups per CU; a 64x64 / 128x32 tile has 16 MFMAs = 0.43 us
  // per K-tile, and the launches that use them are the under-filled ones (one workgroup on most CUs), so one tile of lookahead leaves the
  // load latency exposed in EVERY K-tile — three stages cover ~1.3 us.
  int tap = it0 / cchunks, c0 = (it0 - tap * cchunks) * BK, buf = 0, issued = it0;
  set_tap(tap);
  auto advance = [&]() __attribute__((always_inline)) {  // the (tap, channel chunk) cursor, behind the loads of tile `issued`
    ++issued;
    c0 += BK;
    if (c0 == ld_in) { c0 = 0; ++tap; if (issued < it1) set_tap(tap); }
  };
  auto issue = [&](int rs) {                             // loads of tile `issued` into register stage rs; advances the cursor
    gload(c0, rs);
    advance();
  };
#ifdef TG_STAMP
  unsigned long long ts0 = 0, ts1 = 0, ts2 = 0, ts3 = 0, ts4 = 0, acc_load = 0, acc_mfma = 0, acc_store = 0, acc_bar = 0, t_begin = 0;
#endif
#pragma unroll
  for (int rs = 0; rs < PF; ++rs)
    if (it0 + rs < it1) issue(rs);
  sstore(0, 0);
  __syncthreads();

#ifdef TG_STAMP
  STAMP(t_begin);
#endif
  // one K-tile: the MFMAs of the tile in LDS buffer `b`
  auto compute = [&](int b) {
    if constexpr (BF16) {
      // lane (row r = lane & 31, half h = lane >> 5) supplies k = 16 G + 8 h + (0..7) of 16-deep group G for BOTH operands: one 16-byte read
      const unsigned char* Ab = reinterpret_cast<const unsigned char*>(As) + (b * BM + wm0 + (lane & 31)) * LDH + (lane >> 5) * 16;
      const unsigned char* Bb = reinterpret_cast<const unsigned char*>(Bs) + (b * BN + wn0 + (lane & 31)) * LDH + (lane >> 5) * 16;
#pragma unroll
      for (int G = 0; G < BK / 16; ++G) {
        bf16x8 fa[MI], fb[NI];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) fa[mi] = *reinterpret_cast<const bf16x8*>(Ab + mi * 32 * LDH + G * 32);
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) fb[ni] = *reinterpret_cast<const bf16x8*>(Bb + ni * 32 * LDH + G * 32);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
            if (COLSUM) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[mi], fb[ni], acc[mi][ni], 0, 0, 0);
            else acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[ni], fa[mi], acc[mi][ni], 0, 0, 0);
      }
    } else {
      const float* A = As + b * BM * LDT + wm0 * LDT + frag;
      const float* B = Bs + b * BN * LDT + wn0 * LDT + frag;
#pragma unroll
      for (int g = 0; g < BK / 8; ++g) {
        f32x4 fa[MI], fb[NI];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) fa[mi] = *reinterpret_cast<const f32x4*>(A + mi * 32 * LDT + g * 8);
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) fb[ni] = *reinterpret_cast<const f32x4*>(B + ni * 32 * LDT + g * 8);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
              if (COLSUM) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[mi][s], fb[ni][s], acc[mi][ni], 0, 0, 0);   // D[m][n]: lane = channel
              else acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[ni][s], fa[mi][s], acc[mi][ni], 0, 0, 0);        // D[n][m]: lane = pixel
      }
    }
  };
  int it = it0;
  // steady state, PF iterations at a time, each issuing one tile UNCONDITIONALLY: straight-line code, so the wait in front of the LDS
  // write of stage rs + 1 is a counted one (the PF - 1 younger tiles stay in flight) — with a branch around the issue the compiler has to
  // assume the youngest loads are the ones it needs and drains the queue every iteration
  if constexpr (MI == 1 && NI == 1 && !BF16 && PF >= 2 && 2 * (AR + BR) <= 10) {
    // Tiles with ONE accumulator per wave (64x64, 128x32, 32x128): the 16 MFMAs of a K-tile form one dependent chain, and a wave issues in
    // order — while MFMA k runs (64 cycles) the wave sits at MFMA k+1, so anything placed before or behind the chain is time the matrix pipe
    // idles when no second wave shares the SIMD (launches with at most one workgroup per CU: profiles/r04_stamp_small.txt).  Here every
    // memory instruction of the K-tile — six fragment reads, the AR + BR global loads of tile it+PF, the AR + BR LDS writes of tile it+1 —
    // sits in its own slot BEHIND one MFMA (fenced, so that the compiler keeps it there) and issues in that MFMA's shadow
    // (profiles/r04_interleave_ab.txt: -6.5 % over the generic launches of the step, -15 ... -18 % where one workgroup owns a CU).
    constexpr int NL = AR + BR;
    // one K-tile; rs (register stage of the tile being loaded) is a constant at every call site.  do_load / do_write: the steady state passes
    // true (straight-line code, counted waits), the drain what is left to load / to write
    auto ktile = [&](const int rs, const bool do_load, const bool do_write) __attribute__((always_inline)) {
      const int ws = (rs + 1) % PF;                       // register stage of tile it+1 (its loads are a whole iteration old)
      const uint32_t sa = (uint32_t)__builtin_amdgcn_readfirstlane(c0 * 4);
      const uint32_t sw = (uint32_t)__builtin_amdgcn_readfirstlane((w_tap_off + c0) * 4);
      const float* A = As + buf * BM * LDT + wm0 * LDT + frag;
      const float* B = Bs + buf * BN * LDT + wn0 * LDT + frag;
      float* wa = As + (buf ^ 1) * BM * LDT + lrow * LDT + seg * 4;
      float* wb = Bs + (buf ^ 1) * BN * LDT + lrow * LDT + seg * 4;
      f32x4 fa[2], fb[2];
      fa[0] = *reinterpret_cast<const f32x4*>(A);
      fb[0] = *reinterpret_cast<const f32x4*>(B);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int g = k >> 2, sft = k & 3, cur = g & 1;
        if (COLSUM) acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[cur][sft], fb[cur][sft], acc[0][0], 0, 0, 0);
        else acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[cur][sft], fa[cur][sft], acc[0][0], 0, 0, 0);
        // slot k: k = 4g, 4g+1 (g < 3): the fragments of group g+1; the other ten slots: NL loads, then NL LDS writes
        if (sft == 0 && g < 3) fa[cur ^ 1] = *reinterpret_cast<const f32x4*>(A + (g + 1) * 8);
        else if (sft == 1 && g < 3) fb[cur ^ 1] = *reinterpret_cast<const f32x4*>(B + (g + 1) * 8);
        else {
          const int j = (g < 3) ? 2 * g + (sft - 2) : 6 + sft;           // 0 .. 9 over the free slots (2,3,6,7,10,11,12..15)
          if (j < NL) {
            if (do_load) {
              if (j < AR) ra[rs][j < AR ? j : 0] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, avoff[j < AR ? j : 0], sa, 0);
              else rb[rs][j >= AR ? j - AR : 0] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, wvoff[j >= AR ? j - AR : 0], sw, 0);
            }
          } else if (j < 2 * NL) {
            const int q = j - NL;
            if (do_write) {
              if (q < AR) *reinterpret_cast<u32x4*>(wa + 32 * (q < AR ? q : 0) * LDT) = ra[ws][q < AR ? q : 0];
              else *reinterpret_cast<u32x4*>(wb + 32 * (q >= AR ? q - AR : 0) * LDT) = rb[ws][q >= AR ? q - AR : 0];
            }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (do_load) advance();                              // the tile just issued
      __syncthreads();
      buf ^= 1;
    };
    while (issued + PF <= it1) {
#pragma unroll
      for (int rs = 0; rs < PF; ++rs) ktile(rs, true, true);
      it += PF;
    }
    for (; it < it1; it += PF) {                           // drain (and K ranges shorter than the pipeline)
#pragma unroll
      for (int rs = 0; rs < PF; ++rs)
        if (it + rs < it1) ktile(rs, issued < it1, it + rs + 1 < it1);
    }
  }
  while (issued + PF <= it1) {
#pragma unroll
    for (int rs = 0; rs < PF; ++rs) {
      STAMP(ts0);
      issue(rs);                                         // stage rs went to LDS in the previous iteration (or in the prologue)
      STAMP(ts1);
      compute(buf);
      STAMP(ts2);
      sstore(buf ^ 1, (rs + 1) % PF);
      STAMP(ts3);
      __syncthreads();
      STAMP(ts4);
#ifdef TG_STAMP
      acc_load += ts1 - ts0; acc_mfma += ts2 - ts1; acc_store += ts3 - ts2; acc_bar += ts4 - ts3;
#endif
      buf ^= 1;
    }
    it += PF;
  }
  // drain (and K ranges shorter than the pipeline): fewer than 2 PF iterations; the stage loop must unroll completely — its index names
  // registers — hence guards, not breaks
  for (; it < it1; it += PF) {
#pragma unroll
    for (int rs = 0; rs < PF; ++rs) {
      if (it + rs < it1) {
        if (issued < it1) issue(rs);
        compute(buf);
        if (it + rs + 1 < it1) sstore(buf ^ 1, (rs + 1) % PF);
        __syncthreads();
        buf ^= 1;
      }
    }
  }
#ifdef TG_STAMP
  {
    unsigned long long t_end;
    STAMP(t_end);
    const int sslot = stamp_slot();
    if (sslot >= 0 && tid == 0) {
      tg_stamps[sslot * 8 + 0] = acc_load; tg_stamps[sslot * 8 + 1] = acc_mfma; tg_stamps[sslot * 8 + 2] = acc_store;
      tg_stamps[sslot * 8 + 3] = acc_bar; tg_stamps[sslot * 8 + 4] = t_end - t_begin; tg_stamps[sslot * 8 + 5] = it1 - it0;
      tg_stamps[sslot * 8 + 6] = t_begin - t_entry;
    }
  }
#endif
  if (slot >= 0) {                                       // a cut tile: no epilogue here
    spill_partials<MI, NI>(p.ws, slot, tid, acc);
    return;
  }
  }  // !FIXUP
#ifdef TG_STAMP
  unsigned long long t_epi0 = 0;
  STAMP(t_epi0);
#endif

  // ---- stage 3: the epilogue of a whole tile.  Masked rows carry OOB_OFF in the row table; the buffer range check drops their stores.
  const __amdgpu_buffer_rsrc_t rsrc_o = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, p.out_bytes, 0x00020000);
  const uint32_t* t_ob = reinterpret_cast<const uint32_t*>(t_out);
  if constexpr (COLSUM) {
    float* tile = smem;                                   // the operand tiles are dead
    const SegSplit sg = locate_segment<BM>(p.seg_rows, p.nseg, m0);
    tile_to_lds<BM, BN>(tile, acc, wm0, wn0, lane);
    __syncthreads();
    if (p.stat2 == 2) {
      const __amdgpu_buffer_rsrc_t rsrc_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.ymul), 0, p.out_bytes, 0x00020000);
      stats_bnbwdstat<BM, BN>(tile, t_ob, tid, n0, d.n_store, rsrc_o, rsrc_x, sg, p.colsum, p.c_out);
      return;
    }
    // (igemm_bnstat refuses an activation-gradient multiplier, so the two never meet)
    if (p.stat2) rows_bnstat<BM, BN>(tile, t_ob, tid, n0, d.n_store, rsrc_o, p.bias, d.act, d.alpha);
    else if (p.ymul != nullptr) {
      const __amdgpu_buffer_rsrc_t rsrc_y = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.ymul), 0, p.out_bytes, 0x00020000);
      rows_actsum<BM, BN>(tile, t_ob, tid, n0, d.n_store, rsrc_o, rsrc_y, p.ymul_act, p.ymul_alpha);
    } else rows_store<BM, BN>(tile, t_ob, tid, n0, d.n_store, rsrc_o);
    if (p.ymul != nullptr || p.stat2) __syncthreads();    // the tile was rewritten
    column_sums<BM, BN>(tile, tid, n0, d.n_store, sg, p.stat2 != 0, p.colsum, p.c_out);
    return;
  } else {
    epilogue_plain<MI, NI, FIXUP && (MI > 1)>(acc, t_ob, lane, wm0, n0 + wn0, rsrc_o, p.bias, d.act, d.alpha, d.n_store, d.ld_out, d.w_out, d.os_x, d.os_y, d.n_group);
    if (p.lab != nullptr && nt == p.n_tiles - 1 && wn0 == 0)
      epilogue_labels<MI>(t_ob, lane, wm0, m0, d.h_v * d.w_v, rsrc_o, p.lab, p.lab_n, p.lab_c0, d.ld_out);
  }
#ifdef TG_STAMP
  {
    unsigned long long t_epi1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    STAMP(t_epi1);
    const int sslot = stamp_slot();
    if (sslot >= 0 && tid == 0) tg_stamps[sslot * 8 + 7] = t_epi1 - t_epi0;
    if (tid == 0 && blockIdx.x < 8192) {
      tg_block_times[3 * blockIdx.x] = rt0;
      tg_block_times[3 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
      tg_block_times[3 * blockIdx.x + 2] = ((unsigned long long)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11)) << 32) |
                                           (unsigned)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));
    }
  }
#endif
}

}  // namespace
