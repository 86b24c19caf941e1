// MFMA implicit-GEMM convolution family for gfx950 (MI355X), fp32 in / fp32 accumulate.
//
//   tg_igemm_f32 : out[p,n] = act(sum_{t,c} in[pix(p,t),c] * w[n,t,c] + bias[n])
//   tg_wgrad_f32 : slab[s][t][c][n] = sum_{p in split s} in[pix(p,t),c] * dout[p,n]
//
// One kernel family serves conv fwd (SAME/VALID, stride 1/2), conv input-gradient, 5x5 s2 transposed conv
// (the four output parities as sub-problems of ONE launch), dense / NiN / ZCA (1 tap) — the geometry lives in tg_igemm_desc.
// Template variants: COLSUM (tg_igemm_colsum_*: the mean-only-BN column sums of the output accumulated in the epilogue, lane =
// channel operand order) and BF16 (tg_*_bf16: operands rounded to bf16 on the way LDS -> registers, v_mfma_f32_32x32x16_bf16).
//
// CDNA4 mapping
//  * v_mfma_f32_32x32x2_f32 (exact fp32, 64 FLOP/clk/SIMD = the fp32 roofline, 157 TFLOP/s chip).
//    Lane l supplies A[row l&31][k l>>5], B[k l>>5][col l&31]; D: col = l&31, row = (r&3)+8(r>>2)+4(l>>5).
//  * the reduction index is permuted so that one ds_read_b128 feeds four MFMA k-steps: lane half h of
//    k-group g supplies k = 8g+4h+s in step s for BOTH operands (the sum over k is order-free).
//  * LDS tiles are [row][32 k] with a 16-B row pad (stride 36 floats): ds_read_b128 and ds_write_b128 are
//    bank-conflict free for the 16-lane / 8-lane groups of gfx950.
//  * register-staged double buffering: global loads of tile i+1 are issued before the 64 MFMAs of tile i and
//    written to the other LDS buffer after them; one barrier per K-tile; 2 workgroups per CU (76 KB LDS each).
//  * NHWC gathers are 16 B per lane, 128 B contiguous per 8 lanes, through buffer descriptors: an out-of-image tap is an
//    out-of-range offset that the hardware turns into zeros (no branch, no select); the K-tile position rides in the scalar
//    offset operand.  The fp32 MFMA executes on the vector ALUs, so the K loop carries next to no VALU address arithmetic.
//  * workgroup order is XCD-aware in both kernels (tiles that share operand rows meet in one XCD's L2).
//
// The kernels live in igemm_kernel.h and wgrad_kernel.h (one translation unit); this file packs their parameters, routes and dispatches
// the launches and holds the C ABI.
#include <cstdio>
#include <cstring>
#include "tg_common.h"
#include "tg_device.h"
#include "tg_geom.h"
#include "tg_conv3x3_bf16.h"
#include "igemm_kernel.h"
#include "wgrad_kernel.h"

namespace {

int check_desc(const tg_igemm_desc* d) {
  TG_REQUIRE(d != nullptr, "igemm: null descriptor");
  TG_REQUIRE(d->ld_in > 0 && d->ld_in % 32 == 0, "igemm: ld_in=%d must be a positive multiple of 32", d->ld_in);
  TG_REQUIRE(d->c_out > 0 && d->c_out % 32 == 0, "igemm: c_out=%d must be a positive multiple of 32", d->c_out);
  TG_REQUIRE(d->n_taps >= 1 && d->n_taps <= TG_MAX_TAPS, "igemm: n_taps=%d out of range", d->n_taps);
  TG_REQUIRE(d->n_img > 0 && d->h_v > 0 && d->w_v > 0 && d->h_in > 0 && d->w_in > 0, "igemm: empty geometry");
  TG_REQUIRE(d->n_store >= 0 && d->n_store <= d->c_out && d->n_store <= d->ld_out, "igemm: n_store=%d vs c_out=%d ld_out=%d",
             d->n_store, d->c_out, d->ld_out);
  TG_REQUIRE(d->n_group >= 0 && (d->n_group == 0 || (d->n_store <= d->n_group && d->n_group * d->os_y * d->os_x <= d->c_out)),
             "igemm: n_group=%d vs n_store=%d c_out=%d os=%dx%d", d->n_group, d->n_store, d->c_out, d->os_y, d->os_x);
  const int gy_ = d->n_group ? d->os_y - 1 : 0, gx_ = d->n_group ? d->os_x - 1 : 0;
  TG_REQUIRE((d->h_v - 1) * d->os_y + d->oo_y + gy_ < d->h_out && (d->w_v - 1) * d->os_x + d->oo_x + gx_ < d->w_out && d->oo_y >= 0 && d->oo_x >= 0,
             "igemm: virtual grid %dx%d (stride %d,%d offset %d,%d) exceeds output %dx%d", d->h_v, d->w_v, d->os_y, d->os_x,
             d->oo_y, d->oo_x, d->h_out, d->w_out);
  TG_REQUIRE((int64_t)d->n_img * d->h_in * d->w_in * d->ld_in < (1LL << 31) && (int64_t)d->n_img * d->h_out * d->w_out * d->ld_out < (1LL << 31),
             "igemm: tensor exceeds 2^31 elements");
  return TG_OK;
}

}  // namespace

// A bf16-stored input (tg_igemm_*bf16in_bf16) on the images the halo kernel does not take: widened to fp32 in the caller's scratch (exact), then
// the generic bf16 kernel rounds each value back to the same bf16 on its way into LDS — the operands are the stored bits.
__global__ void __launch_bounds__(256) widen_bf16_kernel(const uint2* __restrict__ in, float4* __restrict__ out, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const uint2 v = in[i];
    out[i] = make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xffff0000u));
  }
}

static int64_t widen_bytes(const tg_igemm_desc* d) { return ((int64_t)d->n_img * d->h_in * d->w_in * d->ld_in * 4 + 255) / 256 * 256; }

template <int BM, int BN, int WM_, int WN_>
static void launch_igemm(IgemmParams& p, hipStream_t s, bool bf16) {
  const dim3 grid(p.n_units);               // one workgroup per work unit (tg::igemm_schedule); the last column tile may overhang: filter rows >= c_out read zeros / unused data, stores are masked by n_store
  if (bf16) {
    if (p.colsum) hipLaunchKernelGGL((igemm_f32_kernel<BM, BN, WM_, WN_, true, true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((igemm_f32_kernel<BM, BN, WM_, WN_, false, true>), grid, dim3(256), 0, s, p);
  } else {
    if (p.colsum) hipLaunchKernelGGL((igemm_f32_kernel<BM, BN, WM_, WN_, true, false>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((igemm_f32_kernel<BM, BN, WM_, WN_, false, false>), grid, dim3(256), 0, s, p);
  }
  if (p.n_fix > 0) {                        // tiles that were cut along K: add their partial sums up, then the usual epilogue (operand type plays no part)
    if (p.colsum) hipLaunchKernelGGL((igemm_f32_kernel<BM, BN, WM_, WN_, true, false, true>), dim3(p.n_fix), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((igemm_f32_kernel<BM, BN, WM_, WN_, false, false, true>), dim3(p.n_fix), dim3(256), 0, s, p);
  }
}

using tg::IgemmCall;

// ---- the route of a launch: decided once, by igemm_route, for igemm_launch (which executes it) and tg_igemm_workspace_bytes (which
// returns its scratch_bytes) -----------------------------------------------------------------------------------------------------------------
//   HEAD_TAIL  a 3x3 layer of the halo kernel's shape whose launch does not fill whole rounds of one workgroup per CU (conv3x3_bf16.hip):
//              the leading images that do are one launch, the few left over another — disjoint image ranges of the same buffers, the
//              statistics of both accumulating into the same per-segment accumulators.  Each part is routed as a launch of its own.
//   WIDEN      a bf16-stored input on images the halo kernel does not take: widened into the front of the scratch, then GENERIC on the rest
//   HALO       conv3x3_bf16.hip (both operand types); bf16 operands REQUIRE the scratch for the packed filter
//   GENERIC    igemm_f32_kernel: the cost model's tile (geom.cpp) and the schedule that cuts tiles along K through all the scratch it wants
enum RouteKind { ROUTE_HEAD_TAIL, ROUTE_WIDEN, ROUTE_HALO, ROUTE_GENERIC };
struct IgemmRoute {
  RouteKind kind;
  int64_t scratch_bytes;                                   // scratch the launch can use
  int head, nh, nt, k0;                                    // HEAD_TAIL: images of the head, segments of the parts, first segment of the tail
  tg_igemm_desc dh, dt;
  int32_t seg_h[8], seg_t[8];
  int64_t widen_bytes;                                     // WIDEN
  int bm, bn, nk[MAX_SUB];                                 // WIDEN, GENERIC: tile (0: none fits), K-tiles per sub-problem in kernel order,
  int64_t tiles;                                           // tiles per sub-problem and the schedule WITH scratch
  tg::IgemmSched sched;
};

// nseg = 0: no statistics.  labels: tg_igemm_labels_* (always GENERIC; the size query cannot know and answers as without labels)
static IgemmRoute igemm_route(const tg_igemm_desc* descs, int n_desc, const int32_t* seg_rows, int nseg, tg::IgemmOperands ops, bool labels) {
  IgemmRoute r{};
  const tg_igemm_desc* d = &descs[0];
  const bool bf16 = ops != tg::IGEMM_F32;
  r.head = labels ? 0 : tg::conv3x3_bf16_split_images(descs, n_desc, seg_rows, nseg, bf16);
  if (r.head) {
    r.kind = ROUTE_HEAD_TAIL;
    r.dh = r.dt = *d;
    r.dh.n_img = r.head;
    r.dt.n_img = d->n_img - r.head;
    int64_t left = (int64_t)r.head * d->h_in * d->w_in;     // rows of the head still to hand out
    for (int i = 0; i < nseg; ++i) {
      const int64_t rows = seg_rows[i], take = rows < left ? rows : left;
      if (take > 0) r.seg_h[r.nh++] = (int32_t)take;
      if (rows - take > 0) {
        if (r.nt == 0) r.k0 = i;
        r.seg_t[r.nt++] = (int32_t)(rows - take);
      }
      left -= take;
    }
    const int64_t a = igemm_route(&r.dh, 1, r.seg_h, r.nh, ops, false).scratch_bytes, b = igemm_route(&r.dt, 1, r.seg_t, r.nt, ops, false).scratch_bytes;
    r.scratch_bytes = a > b ? a : b;                        // one after the other
    return r;
  }
  if (!labels && tg::conv3x3_bf16_applicable(descs, n_desc, seg_rows, nseg, bf16)) {
    r.kind = ROUTE_HALO;
    r.scratch_bytes = bf16 ? tg::conv3x3_bf16_pack_bytes(descs, n_desc) : 0;
    return r;
  }
  r.kind = ops == tg::IGEMM_BF16_IN16 ? ROUTE_WIDEN : ROUTE_GENERIC;
  r.scratch_bytes = r.widen_bytes = r.kind == ROUTE_WIDEN ? widen_bytes(d) : 0;
  // tile choice by the quantisation cost model of geom.cpp (tg::igemm_pick_tile; also behind tg_igemm_tile / tg_igemm_colsum_supported)
  if (!tg::igemm_pick_tile(descs, n_desc, nseg > 0, seg_rows, nseg, bf16, &r.bm, &r.bn)) return r;
  // work units: tiles of an under-filled launch / of the long sub-problems are cut along K through the caller's scratch
  int order[MAX_SUB] = {0, 1, 2, 3};
  tg::igemm_sub_order(descs, n_desc, order);
  for (int i = 0; i < n_desc; ++i) r.nk[i] = descs[order[i]].n_taps * (d->ld_in / BK);
  const int64_t M = (int64_t)d->n_img * d->h_v * d->w_v;
  r.tiles = ((M + r.bm - 1) / r.bm) * ((d->c_out + r.bn - 1) / r.bn);
  tg::igemm_schedule(n_desc, r.nk, r.tiles, r.bm, r.bn, 2 * tg::halo_compute_units(), true, &r.sched);
  r.scratch_bytes += r.sched.ws_bytes;
  return r;
}

static int igemm_validate(const IgemmCall& c) {
  TG_REQUIRE(c.descs && c.n_desc >= 1 && c.n_desc <= MAX_SUB, "igemm: n_desc=%d out of range", c.n_desc);
  TG_REQUIRE(c.in && c.w && c.out, "igemm: null buffer");
  if (c.lab) {
    const tg_igemm_desc* e = &c.descs[0];
    TG_REQUIRE(c.n_desc == 1 && !c.sums && e->n_group == 0 && e->os_x == 1 && e->os_y == 1 && c.lab_n >= 1 && (e->n_store & 3) == 0 && (e->ld_out & 3) == 0 &&
               e->ld_out >= e->n_store + c.lab_n,
               "igemm_labels: needs one ungrouped sub-problem with os = 1, 4 | n_store, 4 | ld_out and ld_out >= n_store + n_labels (n_store %d, ld_out %d, n_labels %d)",
               e->n_store, e->ld_out, c.lab_n);
  }
  TG_REQUIRE(!c.in16() || (c.bf16() && !c.lab && !c.ymul && c.n_desc == 1), "igemm: a bf16-stored input is served for one bf16 sub-problem without labels / multiplier");
  return TG_OK;
}

// the kernel's view of the call: checked descriptors in kernel order, the three buffer-descriptor extents, everything but the schedule
static int igemm_pack(const IgemmCall& c, IgemmParams& p) {
  const tg_igemm_desc* descs = c.descs;
  const int n_desc = c.n_desc;
  p.in = c.in; p.w = c.w; p.bias = c.bias; p.out = c.out; p.n_sub = n_desc;
  p.colsum = c.sums; p.nseg = c.nseg;
  p.ymul = c.ymul; p.ymul_act = c.ymul_act; p.ymul_alpha = c.ymul_alpha;
  p.stat2 = c.stat2();
  p.lab = c.lab; p.lab_n = c.lab_n; p.lab_c0 = descs[0].n_store;
  for (int i = 0; i < 8; ++i) p.seg_rows[i] = (c.seg_rows && i < c.nseg) ? c.seg_rows[i] : 0;
  const tg_igemm_desc* d = &descs[0];
  // sub-problems longest first: workgroups are dispatched in index order, so the 9-tap parity of a 5x5 s2 transposed
  // conv starts before the 4-tap one instead of forming the tail
  int order[MAX_SUB] = {0, 1, 2, 3};
  tg::igemm_sub_order(descs, n_desc, order);
  for (int i = 0; i < n_desc; ++i) {
    int rc = check_desc(&descs[order[i]]);
    if (rc != TG_OK) return rc;
    const tg_igemm_desc& e = descs[order[i]];
    TG_REQUIRE(e.n_img == d->n_img && e.h_v == d->h_v && e.w_v == d->w_v && e.c_out == d->c_out && e.ld_in == d->ld_in && e.h_in == d->h_in &&
               e.w_in == d->w_in && e.w_sn == d->w_sn && e.w_st == d->w_st, "igemm: sub-problem %d differs in M / N / gathered tensor / filter strides", i);
    SubDesc& k = p.d[i];
    k.h_v = e.h_v; k.w_v = e.w_v; k.s_y = e.s_y; k.s_x = e.s_x; k.h_out = e.h_out; k.w_out = e.w_out; k.ld_out = e.ld_out;
    k.os_y = e.os_y; k.os_x = e.os_x; k.oo_y = e.oo_y; k.oo_x = e.oo_x; k.n_store = e.n_store; k.n_taps = e.n_taps; k.act = e.act;
    k.alpha = e.alpha;
    k.n_group = e.n_group;
    for (int t = 0; t < e.n_taps; ++t)
      k.taps[t] = ((int32_t)e.tapw[t] << 16) | (((int32_t)e.dy[t] & 0xff) << 8) | ((int32_t)e.dx[t] & 0xff);
  }
  p.w_sn = d->w_sn; p.w_st = d->w_st;
  p.n_img = d->n_img; p.h_in = d->h_in; p.w_in = d->w_in; p.ld_in = d->ld_in; p.c_out = d->c_out;
  p.M = d->n_img * d->h_v * d->w_v;
  const int64_t in_bytes = (int64_t)d->n_img * d->h_in * d->w_in * d->ld_in * 4;
  TG_REQUIRE(in_bytes < 0x7FFFFFF0LL, "igemm: gathered tensor exceeds the 2 GiB buffer-descriptor range");
  p.in_bytes = (uint32_t)in_bytes;
  int max_tapw = 0;
  for (int i = 0; i < n_desc; ++i)
    for (int t = 0; t < descs[i].n_taps; ++t) max_tapw = descs[i].tapw[t] > max_tapw ? descs[i].tapw[t] : max_tapw;
  const int64_t w_bytes = ((int64_t)(d->c_out - 1) * d->w_sn + (int64_t)max_tapw * d->w_st + d->ld_in) * 4;
  TG_REQUIRE(w_bytes > 0 && w_bytes < 0x7FFFFFF0LL && d->w_st >= 0 && d->w_sn >= 0 && (int64_t)max_tapw * d->w_st < 0x7FFFFFFFLL,
             "igemm: filter extent outside the 2 GiB buffer-descriptor range");
  p.w_bytes = (uint32_t)w_bytes;
  int64_t out_bytes = 0;
  for (int i = 0; i < n_desc; ++i) {
    const int64_t ob = (int64_t)descs[i].n_img * descs[i].h_out * descs[i].w_out * descs[i].ld_out * 4;
    out_bytes = ob > out_bytes ? ob : out_bytes;
  }
  TG_REQUIRE(out_bytes < 0x7FFFFFF0LL, "igemm: output tensor exceeds the 2 GiB buffer-descriptor range");
  p.out_bytes = (uint32_t)out_bytes;
  return TG_OK;
}

static int launch_generic(IgemmParams& p, const tg::IgemmSched& sc, int bm, int bn, hipStream_t s, bool bf16) {
  p.n_units = sc.n_units; p.n_fix = sc.n_fix; p.nfull = sc.nfull; p.pat_len = sc.pat_len; p.n_pat_split = sc.n_pat_split; p.n_split_sub = sc.n_split_sub;
  for (int i = 0; i < MAX_SUB; ++i) { p.ks[i] = sc.ks[i]; p.split_sub[i] = sc.split_sub[i]; p.first_slot[i] = sc.first_slot[i]; }
  for (int i = 0; i < 16; ++i) { p.pat_sub[i] = sc.pat_sub[i]; p.pat_k[i] = sc.pat_k[i]; p.pat_slot[i] = sc.pat_slot[i]; }
  if (bm == 128 && bn == 128) launch_igemm<128, 128, 2, 2>(p, s, bf16);
  else if (bm == 64 && bn == 128) launch_igemm<64, 128, 2, 2>(p, s, bf16);
  else if (bm == 64 && bn == 64) launch_igemm<64, 64, 2, 2>(p, s, bf16);
  else if (bm == 32 && bn == 128) launch_igemm<32, 128, 1, 4>(p, s, bf16);
  else launch_igemm<128, 32, 4, 1>(p, s, bf16);
  TG_CHECK_LAUNCH("igemm_f32_kernel");
  return TG_OK;
}

// HALO and GENERIC (and what WIDEN leaves): one kernel over the whole call
static int igemm_run(const IgemmCall& c, const IgemmRoute& r) {
  IgemmParams p;
  int rc = igemm_pack(c, p);
  if (rc != TG_OK) return rc;
  const tg_igemm_desc* d = &c.descs[0];
  const bool halo = r.kind == ROUTE_HALO;                  // the classifier's 3x3 layers: halo-tiled kernel (both operand types)
  double taps = 0;
  for (int i = 0; i < c.n_desc; ++i) taps += c.descs[i].n_taps;
  const double flops = 2.0 * p.M * d->c_out * taps * d->ld_in;
  const double bytes = (c.in16() ? 2.0 : 4.0) * p.M * d->ld_in + 4.0 * ((double)p.M * d->n_store * c.n_desc + (double)d->c_out * taps * d->ld_in);
  tg::IgemmSched sc = r.sched;
  if (!halo) {
    TG_REQUIRE(r.bm, "igemm: no tile fits c_out=%d with the given segments", d->c_out);
    p.m_tiles = (p.M + r.bm - 1) / r.bm;
    p.n_tiles = (p.c_out + r.bn - 1) / r.bn;
    // no scratch, less than the cut needs, or misaligned: the one-launch schedule (one unit per tile)
    if (sc.ws_bytes > 0 && (!c.scratch || sc.ws_bytes > c.scratch_bytes || (reinterpret_cast<uintptr_t>(c.scratch) & 15)))
      tg::igemm_schedule(c.n_desc, r.nk, r.tiles, r.bm, r.bn, 2 * tg::halo_compute_units(), false, &sc);
  }
  hipStream_t s = tg::as_stream(c.stream);
  char desc[128];
  snprintf(desc, sizeof(desc), "M=%dx%d N=%d K=%gx%d in=%dx%d s=%d os=%d%s tile=%dx%d units=%d fix=%d ks=%d/%d/%d/%d", c.n_desc, p.M, d->c_out, taps, d->ld_in, d->h_in,
           d->w_in, d->s_y, d->os_y, c.bf16() ? " bf16" : "", r.bm, r.bn, sc.n_units, sc.n_fix, sc.ks[0], sc.ks[1], sc.ks[2], sc.ks[3]);
  tg::ProfScope prof(tg::PC_IGEMM, flops, bytes, s, desc);
  if (halo) return tg::conv3x3_bf16_launch(c, c.in16() ? p.in_bytes / 2 : p.in_bytes, p.w_bytes, p.out_bytes);
  p.ws = static_cast<float*>(c.scratch);
  return launch_generic(p, sc, r.bm, r.bn, s, c.bf16());
}

static int igemm_launch(const IgemmCall& c);

static int launch_head_tail(const IgemmCall& c, const IgemmRoute& r) {
  const tg_igemm_desc* d = &c.descs[0];
  const int64_t rows = (int64_t)r.head * d->h_in * d->w_in, o_in = rows * d->ld_in, o_out = rows * d->ld_out;
  IgemmCall h = c, t = c;
  h.descs = &r.dh; h.seg_rows = r.seg_h; h.nseg = r.nh;
  int rc = igemm_launch(h);
  if (rc != TG_OK) return rc;
  t.descs = &r.dt; t.seg_rows = r.seg_t; t.nseg = r.nt;
  t.in = reinterpret_cast<const float*>(reinterpret_cast<const char*>(c.in) + o_in * (c.in16() ? 2 : 4));
  t.out = c.out + o_out;
  if (c.sums) t.sums = c.sums + (int64_t)r.k0 * d->c_out * (c.stat2() ? 2 : 1);
  if (c.ymul) t.ymul = c.ymul + o_out;
  return igemm_launch(t);                                  // (stream-ordered behind the head: both may use the same scratch)
}

static int launch_widen(const IgemmCall& c, const IgemmRoute& r) {
  const tg_igemm_desc* d = &c.descs[0];
  TG_REQUIRE(check_desc(d) == TG_OK, "igemm: bad descriptor");
  const int64_t wb = r.widen_bytes;
  TG_REQUIRE(c.scratch != nullptr && c.scratch_bytes >= wb && (reinterpret_cast<uintptr_t>(c.scratch) & 15) == 0,
             "igemm (bf16-stored input): this launch needs %lld bytes of 16-byte aligned scratch to widen its input, got %lld (query "
             "tg_igemm_workspace_bytes(..., bf16 = 2))", (long long)wb, (long long)(c.scratch ? c.scratch_bytes : 0));
  const int64_t n4 = (int64_t)d->n_img * d->h_in * d->w_in * d->ld_in / 4;
  const int64_t nb = (n4 + 255) / 256;
  hipLaunchKernelGGL(widen_bf16_kernel, dim3(nb < 4096 ? nb : 4096), dim3(256), 0, tg::as_stream(c.stream), reinterpret_cast<const uint2*>(c.in),
                     static_cast<float4*>(c.scratch), n4);
  TG_CHECK_LAUNCH("widen_bf16_kernel");
  IgemmCall g = c;                                         // the generic kernel on the widened copy, its cut tiles in the rest of the scratch
  g.in = static_cast<const float*>(c.scratch);
  g.ops = tg::IGEMM_BF16;
  g.scratch = c.scratch_bytes > wb ? static_cast<char*>(c.scratch) + wb : nullptr;
  g.scratch_bytes = c.scratch_bytes - wb;
  return igemm_run(g, r);
}

static int igemm_launch(const IgemmCall& c) {
  int rc = igemm_validate(c);
  if (rc != TG_OK) return rc;
  const IgemmRoute r = igemm_route(c.descs, c.n_desc, c.seg_rows, c.sums ? c.nseg : 0, c.ops, c.lab != nullptr);
  if (r.kind == ROUTE_HEAD_TAIL) return launch_head_tail(c, r);
  if (r.kind == ROUTE_WIDEN) return launch_widen(c, r);
  return igemm_run(c, r);
}

#ifdef TG_STAMP
extern "C" int tg_debug_read_block_times(unsigned long long* out, int n) {
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(tg_block_times), sizeof(unsigned long long) * 3 * n);
  return e == hipSuccess ? 0 : -2;
}

extern "C" int tg_debug_read_stamps(unsigned long long* out) {
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(tg_stamps), sizeof(unsigned long long) * 64);
  return e == hipSuccess ? 0 : -2;
}
#endif

extern "C" int tg_igemm_multi_f32(const tg_igemm_desc* descs, int n_desc, const float* in, const float* w, const float* bias, float* out,
                                  void* scratch, int64_t scratch_bytes, void* stream) {
  return igemm_launch({.descs = descs, .n_desc = n_desc, .in = in, .w = w, .bias = bias, .out = out, .ops = tg::IGEMM_F32, .scratch = scratch,
                       .scratch_bytes = scratch_bytes, .stream = stream});
}

extern "C" int tg_igemm_multi_bf16(const tg_igemm_desc* descs, int n_desc, const float* in, const float* w, const float* bias, float* out,
                                   void* scratch, int64_t scratch_bytes, void* stream) {
  return igemm_launch({.descs = descs, .n_desc = n_desc, .in = in, .w = w, .bias = bias, .out = out, .ops = tg::IGEMM_BF16, .scratch = scratch,
                       .scratch_bytes = scratch_bytes, .stream = stream});
}

extern "C" int tg_igemm_f32(const tg_igemm_desc* d, const float* in, const float* w, const float* bias, float* out, void* scratch,
                            int64_t scratch_bytes, void* stream) {
  return tg_igemm_multi_f32(d, 1, in, w, bias, out, scratch, scratch_bytes, stream);
}

extern "C" int tg_igemm_bf16(const tg_igemm_desc* d, const float* in, const float* w, const float* bias, float* out, void* scratch,
                             int64_t scratch_bytes, void* stream) {
  return tg_igemm_multi_bf16(d, 1, in, w, bias, out, scratch, scratch_bytes, stream);
}

extern "C" int tg_igemm_labels_f32(const tg_igemm_desc* d, const float* in, const float* w, const float* bias, const float* labels, int n_labels, float* out,
                                   void* scratch, int64_t scratch_bytes, void* stream) {
  TG_REQUIRE(labels != nullptr, "igemm_labels: null labels");
  return igemm_launch({.descs = d, .n_desc = 1, .in = in, .w = w, .bias = bias, .out = out, .ops = tg::IGEMM_F32, .lab = labels, .lab_n = n_labels,
                       .scratch = scratch, .scratch_bytes = scratch_bytes, .stream = stream});
}

extern "C" int tg_igemm_labels_bf16(const tg_igemm_desc* d, const float* in, const float* w, const float* bias, const float* labels, int n_labels, float* out,
                                    void* scratch, int64_t scratch_bytes, void* stream) {
  TG_REQUIRE(labels != nullptr, "igemm_labels: null labels");
  return igemm_launch({.descs = d, .n_desc = 1, .in = in, .w = w, .bias = bias, .out = out, .ops = tg::IGEMM_BF16, .lab = labels, .lab_n = n_labels,
                       .scratch = scratch, .scratch_bytes = scratch_bytes, .stream = stream});
}

// the gathered activation is stored as bf16 (include/tg_kernels.h): only layers of the halo kernels' shape
static int require_halo_shape(const tg_igemm_desc* d, const char* what) {
  TG_REQUIRE(d != nullptr, "%s: null descriptor", what);
  TG_REQUIRE(d->n_taps == 9 && d->n_group == 0 && d->s_y == 1 && d->s_x == 1 && d->os_y == 1 && d->os_x == 1 && d->oo_y == 0 && d->oo_x == 0 &&
             d->h_v == d->h_in && d->w_v == d->w_in && d->h_out == d->h_in && d->w_out == d->w_in && (d->w_in == 16 || d->w_in == 32 || d->w_in == 64) &&
             (d->h_in * d->w_in) % 256 == 0 && d->ld_in % 64 == 0 && d->c_out % 128 == 0,
             "%s: a bf16-stored input is served for 3x3 / stride-1 / SAME layers of width 16 / 32 / 64 with 64 | ld_in and 128 | c_out only", what);
  return TG_OK;
}

extern "C" int tg_igemm_bf16in_bf16(const tg_igemm_desc* d, const void* in, const float* w, const float* bias, float* out, void* scratch,
                                    int64_t scratch_bytes, void* stream) {
  int rc = require_halo_shape(d, "igemm_bf16in");
  if (rc != TG_OK) return rc;
  return igemm_launch({.descs = d, .n_desc = 1, .in = static_cast<const float*>(in), .w = w, .bias = bias, .out = out, .ops = tg::IGEMM_BF16_IN16,
                       .scratch = scratch, .scratch_bytes = scratch_bytes, .stream = stream});
}

// scratch a launch of these descriptors can use: the halo kernel's packed bf16 filter (REQUIRED by such a launch), the widened copy of a
// bf16-stored input (required) and the partial sums of the tiles the generic kernel's schedule cuts along K (optional); a launch that is
// cut into a halo head and a generic tail uses the scratch for one after the other.  The launch executes the same igemm_route.
extern "C" int64_t tg_igemm_workspace_bytes(const tg_igemm_desc* descs, int n_desc, const int32_t* seg_rows, int nseg, int bf16) {
  if (!descs || n_desc < 1 || n_desc > MAX_SUB || nseg < 0 || nseg > 8 || (nseg > 0 && !seg_rows)) { tg::set_error("igemm_workspace_bytes: bad arguments"); return TG_ERR_INVALID; }
  for (int i = 0; i < n_desc; ++i)
    if (descs[i].ld_in <= 0 || descs[i].c_out <= 0 || descs[i].n_taps <= 0 || descs[i].n_taps > TG_MAX_TAPS || descs[i].n_img <= 0) { tg::set_error("igemm_workspace_bytes: bad descriptor"); return TG_ERR_INVALID; }
  return igemm_route(descs, n_desc, seg_rows, nseg, bf16 == 2 ? tg::IGEMM_BF16_IN16 : bf16 ? tg::IGEMM_BF16 : tg::IGEMM_F32, false).scratch_bytes;
}

// ---- the statistics families ---------------------------------------------------------------------------------------------------------------
// Common to the three: every application segment holds at least one 32-row tile, the segments add up to the launch's rows, and the
// n_sums fp64 accumulators are zeroed here unless the caller did.
static int igemm_stat_launch(const IgemmCall& c, const char* who, int64_t n_sums, int zeroed, const char* memset_what) {
  const tg_igemm_desc* d = c.descs;
  int tot = 0;
  for (int i = 0; i < c.nseg; ++i) { TG_REQUIRE(c.seg_rows[i] >= 32, "%s: segment %d has %d rows (need at least one 32-row tile)", who, i, c.seg_rows[i]); tot += c.seg_rows[i]; }
  TG_REQUIRE(tot == d->n_img * d->h_v * d->w_v, "%s: segments sum to %d rows, launch has %d", who, tot, d->n_img * d->h_v * d->w_v);
  if (!zeroed) {
    hipError_t e = hipMemsetAsync(c.sums, 0, sizeof(double) * n_sums, tg::as_stream(c.stream));
    if (e != hipSuccess) return tg::hip_fail(e, memset_what);
  }
  return igemm_launch(c);
}

// column sums of the raw output; with ymul: of out = acc * act'(ymul) (tg_igemm_actsum_*)
static int igemm_colsum(const IgemmCall& c, int zeroed) {
  const tg_igemm_desc* d = c.descs;
  TG_REQUIRE(d && c.sums && c.seg_rows && c.nseg >= 1 && c.nseg <= 8, "igemm_colsum: bad args");
  TG_REQUIRE(d->n_group == 0, "igemm_colsum: grouped columns are not supported");
  TG_REQUIRE(d->act == TG_ACT_NONE, "igemm_colsum: the statistics are of the raw convolution output (no activation)");
  return igemm_stat_launch(c, "igemm_colsum", (int64_t)c.nseg * d->c_out, zeroed, "hipMemsetAsync(colsum)");
}

extern "C" int tg_igemm_colsum_f32(const tg_igemm_desc* d, const float* in, const float* w, float* out, const int32_t* seg_rows, int nseg,
                                   double* colsum, int colsum_zeroed, void* scratch, int64_t scratch_bytes, void* stream) {
  return igemm_colsum({.descs = d, .n_desc = 1, .in = in, .w = w, .out = out, .ops = tg::IGEMM_F32, .sums = colsum, .seg_rows = seg_rows, .nseg = nseg,
                       .stat = tg::IGEMM_STAT_COLSUM, .scratch = scratch, .scratch_bytes = scratch_bytes, .stream = stream}, colsum_zeroed);
}

extern "C" int tg_igemm_colsum_bf16(const tg_igemm_desc* d, const float* in, const float* w, float* out, const int32_t* seg_rows, int nseg,
                                    double* colsum, int colsum_zeroed, void* scratch, int64_t scratch_bytes, void* stream) {
  return igemm_colsum({.descs = d, .n_desc = 1, .in = in, .w = w, .out = out, .ops = tg::IGEMM_BF16, .sums = colsum, .seg_rows = seg_rows, .nseg = nseg,
                       .stat = tg::IGEMM_STAT_COLSUM, .scratch = scratch, .scratch_bytes = scratch_bytes, .stream = stream}, colsum_zeroed);
}

extern "C" int tg_igemm_actsum_f32(const tg_igemm_desc* d, const float* in, const float* w, const float* yact, int act, float alpha, float* out,
                                   const int32_t* seg_rows, int nseg, double* colsum, int colsum_zeroed, void* scratch, int64_t scratch_bytes,
                                   void* stream) {
  TG_REQUIRE(yact != nullptr, "igemm_actsum: yact is NULL");
  return igemm_colsum({.descs = d, .n_desc = 1, .in = in, .w = w, .out = out, .ops = tg::IGEMM_F32, .sums = colsum, .seg_rows = seg_rows, .nseg = nseg,
                       .stat = tg::IGEMM_STAT_COLSUM, .ymul = yact, .ymul_act = act, .ymul_alpha = alpha, .scratch = scratch, .scratch_bytes = scratch_bytes,
                       .stream = stream}, colsum_zeroed);
}

extern "C" int tg_igemm_actsum_bf16(const tg_igemm_desc* d, const float* in, const float* w, const float* yact, int act, float alpha, float* out,
                                    const int32_t* seg_rows, int nseg, double* colsum, int colsum_zeroed, void* scratch, int64_t scratch_bytes,
                                    void* stream) {
  TG_REQUIRE(yact != nullptr, "igemm_actsum: yact is NULL");
  return igemm_colsum({.descs = d, .n_desc = 1, .in = in, .w = w, .out = out, .ops = tg::IGEMM_BF16, .sums = colsum, .seg_rows = seg_rows, .nseg = nseg,
                       .stat = tg::IGEMM_STAT_COLSUM, .ymul = yact, .ymul_act = act, .ymul_alpha = alpha, .scratch = scratch, .scratch_bytes = scratch_bytes,
                       .stream = stream}, colsum_zeroed);
}

// conv + bias + activation whose output feeds a batch norm: the statistics of the ACTIVATED output are taken in the epilogue
static int igemm_bnstat(const IgemmCall& c, int zeroed) {
  const tg_igemm_desc* d = c.descs;
  TG_REQUIRE(d && c.sums && c.seg_rows && c.nseg >= 1 && c.nseg <= 8, "igemm_bnstat: bad args");
  TG_REQUIRE(d->n_group == 0, "igemm_bnstat: grouped columns are not supported");
  TG_REQUIRE(c.ymul == nullptr, "igemm_bnstat: no activation-gradient multiplier (the epilogue runs one row-wise pass)");
  TG_REQUIRE(d->act == TG_ACT_NONE || d->act == TG_ACT_RELU || d->act == TG_ACT_LRELU, "igemm_bnstat: activation %d is not none / relu / leaky relu", d->act);
  return igemm_stat_launch(c, "igemm_bnstat", (int64_t)8 * 2 * c.nseg * d->c_out, zeroed, "hipMemsetAsync(bn statistics)");      // all eight replicas of the batch norm's buffer
}

extern "C" int tg_igemm_bnstat_f32(const tg_igemm_desc* d, const float* in, const float* w, const float* bias, float* out, const int32_t* seg_rows, int nseg,
                                   double* sums, int sums_zeroed, void* scratch, int64_t scratch_bytes, void* stream) {
  return igemm_bnstat({.descs = d, .n_desc = 1, .in = in, .w = w, .bias = bias, .out = out, .ops = tg::IGEMM_F32, .sums = sums, .seg_rows = seg_rows,
                       .nseg = nseg, .stat = tg::IGEMM_STAT_BN, .scratch = scratch, .scratch_bytes = scratch_bytes, .stream = stream}, sums_zeroed);
}

extern "C" int tg_igemm_bnstat_bf16(const tg_igemm_desc* d, const float* in, const float* w, const float* bias, float* out, const int32_t* seg_rows, int nseg,
                                    double* sums, int sums_zeroed, void* scratch, int64_t scratch_bytes, void* stream) {
  return igemm_bnstat({.descs = d, .n_desc = 1, .in = in, .w = w, .bias = bias, .out = out, .ops = tg::IGEMM_BF16, .sums = sums, .seg_rows = seg_rows,
                       .nseg = nseg, .stat = tg::IGEMM_STAT_BN, .scratch = scratch, .scratch_bytes = scratch_bytes, .stream = stream}, sums_zeroed);
}

extern "C" int tg_igemm_bnstat_bf16in_bf16(const tg_igemm_desc* d, const void* in, const float* w, const float* bias, float* out, const int32_t* seg_rows,
                                           int nseg, double* sums, int sums_zeroed, void* scratch, int64_t scratch_bytes, void* stream) {
  int rc = require_halo_shape(d, "igemm_bnstat_bf16in");
  if (rc != TG_OK) return rc;
  return igemm_bnstat({.descs = d, .n_desc = 1, .in = static_cast<const float*>(in), .w = w, .bias = bias, .out = out, .ops = tg::IGEMM_BF16_IN16, .sums = sums,
                       .seg_rows = seg_rows, .nseg = nseg, .stat = tg::IGEMM_STAT_BN, .scratch = scratch, .scratch_bytes = scratch_bytes, .stream = stream},
                      sums_zeroed);
}

// input gradient (or any conv) whose output dy is consumed by a batch norm's backward pass: that pass's statistics in the epilogue
static int igemm_bnbwdstat(const IgemmCall& c, int zeroed) {
  const tg_igemm_desc* d = c.descs;
  TG_REQUIRE(d && c.sums && c.ymul && c.seg_rows && c.nseg >= 1 && c.nseg <= 8, "igemm_bnbwdstat: bad args");
  TG_REQUIRE(d->n_group == 0 && d->act == TG_ACT_NONE, "igemm_bnbwdstat: grouped columns / a fused activation are not supported");
  return igemm_stat_launch(c, "igemm_bnbwdstat", (int64_t)8 * 2 * c.nseg * d->c_out, zeroed, "hipMemsetAsync(bn backward statistics)");
}

extern "C" int tg_igemm_bnbwdstat_f32(const tg_igemm_desc* d, const float* in, const float* w, const float* x, float* out, const int32_t* seg_rows, int nseg,
                                      double* sums, int sums_zeroed, void* scratch, int64_t scratch_bytes, void* stream) {
  return igemm_bnbwdstat({.descs = d, .n_desc = 1, .in = in, .w = w, .out = out, .ops = tg::IGEMM_F32, .sums = sums, .seg_rows = seg_rows, .nseg = nseg,
                          .stat = tg::IGEMM_STAT_BNBWD, .ymul = x, .ymul_act = TG_ACT_NONE, .scratch = scratch, .scratch_bytes = scratch_bytes, .stream = stream},
                         sums_zeroed);
}

extern "C" int tg_igemm_bnbwdstat_bf16(const tg_igemm_desc* d, const float* in, const float* w, const float* x, float* out, const int32_t* seg_rows, int nseg,
                                       double* sums, int sums_zeroed, void* scratch, int64_t scratch_bytes, void* stream) {
  return igemm_bnbwdstat({.descs = d, .n_desc = 1, .in = in, .w = w, .out = out, .ops = tg::IGEMM_BF16, .sums = sums, .seg_rows = seg_rows, .nseg = nseg,
                          .stat = tg::IGEMM_STAT_BNBWD, .ymul = x, .ymul_act = TG_ACT_NONE, .scratch = scratch, .scratch_bytes = scratch_bytes, .stream = stream},
                         sums_zeroed);
}

template <int CT, int NT, int WC, int WN, int WK>
static void launch_wgrad(WgradParams& p, hipStream_t s, bool bf16) {
  p.c_tiles = (p.d.ld_in + CT - 1) / CT;      // last tiles may overhang (masked at the store)
  p.n_tiles = (p.d.c_out + NT - 1) / NT;
  int blocks = p.n_split * p.d.n_taps * p.c_tiles * p.n_tiles;
  if (bf16) hipLaunchKernelGGL((wgrad_f32_kernel<CT, NT, WC, WN, WK, true>), dim3(blocks), dim3(256), 0, s, p);
  else hipLaunchKernelGGL((wgrad_f32_kernel<CT, NT, WC, WN, WK, false>), dim3(blocks), dim3(256), 0, s, p);
}

// in16 (tg_wgrad_bf16in_bf16): the activation is stored as bf16 — always wgrad3x3 (its shape rule without the occupancy rule of the default
// policy: any n_split is served)
static int wgrad_impl(const tg_igemm_desc* d, const float* in, const float* dout, float* slab, int n_split, void* stream, bool bf16, bool in16 = false) {
  const char* who = in16 ? "wgrad_bf16in" : "wgrad";
  int rc = check_desc(d);
  if (rc != TG_OK) return rc;
  TG_REQUIRE(in && dout && slab, "%s: null buffer", who);
  TG_REQUIRE(n_split >= 1, "%s: n_split=%d", who, n_split);
  if (in16) {
    TG_REQUIRE(tg::wgrad3x3_applicable(d, n_split, true, 1, tg::halo_compute_units()),
               "wgrad_bf16in: a bf16-stored input is served for 3x3 / stride-1 / SAME layers of width 16 / 32 / 64 (128 pixels per tile), 32 | ld_in, "
               "128 | c_out only");
  } else {
    TG_REQUIRE(d->c_out <= d->ld_out, "wgrad: c_out=%d exceeds ld_out=%d", d->c_out, d->ld_out);
    TG_REQUIRE(d->n_group == 0, "wgrad: grouped columns are not supported");
  }
  WgradParams p{in, dout, slab, *d, 0, n_split, 0, 0, 0, 0, 0};
  p.M = d->n_img * d->h_v * d->w_v;
  const int64_t ib = (int64_t)d->n_img * d->h_in * d->w_in * d->ld_in * (in16 ? 2 : 4), ob = (int64_t)d->n_img * d->h_out * d->w_out * d->ld_out * 4;
  TG_REQUIRE(ib < 0x7FFFFFF0LL && ob < 0x7FFFFFF0LL, "%s: operand exceeds the 2 GiB buffer-descriptor range", who);
  p.in_bytes = (uint32_t)ib; p.dout_bytes = (uint32_t)ob;
  p.px_per_split = (((p.M + n_split - 1) / n_split) + BK - 1) / BK * BK;
  const double flops = 2.0 * p.M * d->c_out * d->n_taps * d->ld_in;
  const double bytes = (in16 ? 2.0 : 4.0) * p.M * d->ld_in + 4.0 * ((double)p.M * d->c_out + (double)n_split * d->c_out * d->n_taps * d->ld_in);
  char desc[96];
  if (in16) snprintf(desc, sizeof(desc), "M=%lld N=%d K=%dx%d in=%dx%d split=%d bf16in", (long long)p.M, d->c_out, d->n_taps, d->ld_in, d->h_in, d->w_in, n_split);
  else snprintf(desc, sizeof(desc), "M=%d N=%d K=%dx%d in=%dx%d s=%d split=%d%s", p.M, d->c_out, d->n_taps, d->ld_in, d->h_in, d->w_in, d->s_y, n_split, bf16 ? " bf16" : "");
  hipStream_t s = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_WGRAD, flops, bytes, s, desc);
  if (in16 || tg::wgrad3x3_applicable(d, n_split, bf16, tg::halo_policy(), tg::halo_compute_units())) {      // the classifier's 3x3 layers: wgrad3x3.hip
    tg::halo_count_launch();
    return tg::wgrad3x3_launch(d, in, dout, slab, n_split, p.in_bytes, p.dout_bytes, s, bf16, in16);
  }
  // channel tiles: tg::wgrad_tile (geom.cpp; tg_wgrad_splits sizes the pixel split with the same rule)
  const int ct = tg::wgrad_tile(d->ld_in), nt = tg::wgrad_tile(d->c_out);
  if (ct == 128 && nt == 128) launch_wgrad<128, 128, 2, 2, 1>(p, s, bf16);
  else if (ct == 128 && nt == 64) launch_wgrad<128, 64, 2, 2, 1>(p, s, bf16);
  else if (ct == 128 && nt == 32) launch_wgrad<128, 32, 4, 1, 1>(p, s, bf16);
  else if (ct == 64 && nt == 128) launch_wgrad<64, 128, 2, 2, 1>(p, s, bf16);
  else if (ct == 64 && nt == 64) launch_wgrad<64, 64, 2, 2, 1>(p, s, bf16);
  else if (ct == 64 && nt == 32) launch_wgrad<64, 32, 2, 1, 2>(p, s, bf16);
  else if (ct == 32 && nt == 128) launch_wgrad<32, 128, 1, 4, 1>(p, s, bf16);
  else if (ct == 32 && nt == 64) launch_wgrad<32, 64, 1, 2, 2>(p, s, bf16);
  else launch_wgrad<32, 32, 1, 1, 4>(p, s, bf16);
  TG_CHECK_LAUNCH("wgrad_f32_kernel");
  return TG_OK;
}

extern "C" int tg_wgrad_f32(const tg_igemm_desc* d, const float* in, const float* dout, float* slab, int n_split, void* stream) {
  return wgrad_impl(d, in, dout, slab, n_split, stream, false);
}

extern "C" int tg_wgrad_bf16(const tg_igemm_desc* d, const float* in, const float* dout, float* slab, int n_split, void* stream) {
  return wgrad_impl(d, in, dout, slab, n_split, stream, true);
}

extern "C" int tg_wgrad_bf16in_bf16(const tg_igemm_desc* d, const void* in, const float* dout, float* slab, int n_split, void* stream) {
  return wgrad_impl(d, static_cast<const float*>(in), dout, slab, n_split, stream, true, true);
}
