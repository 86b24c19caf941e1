// tf.summary.histogram over a network's FLAT buffer (config.SUMMARY_HISTOGRAM): what tensorflow::histogram::Histogram holds
// after Add((double)x) for every element of each variable, all variables of a ParamStore buffer in one launch sequence.  [UNVERIFIED-TF]
//   limits   1 551 doubles built ON THE HOST (tg_tf_histogram_limits: v = 1e-12; while v < 1e20 {push v; v *= 1.1}; push DBL_MAX; the
//            negated list reversed, 0, the list) and handed in as a device pointer: the kernel only compares against them.
//   bucket   upper_bound(limits, (double)x) - limits: a fixed-depth binary search over the table held in LDS (11 compares of fp64).
//   counts   per workgroup in LDS (32-bit integer atomics), the non-empty bins added to the output with 64-bit global integer atomics:
//            integers, so the order does not matter.  A wave whose 64 lanes all fall into ONE bin (a freshly initialised bias: all zeros)
//            issues one LDS add of 64 instead of 64 serialised adds of 1.
//   stats    min / max exact; num, sum, sum of squares in fp64 from (double)x.  Thread t of a chunk's workgroup takes the elements
//            t, t + 256, ... in that order, lanes -> wave by a __shfl_down tree, waves -> workgroup in LDS in wave order, one partial per
//            chunk in the workspace; a second launch (one workgroup per segment) adds a segment's partials in chunk order through the same
//            tree.  The chunk map depends on the segment table alone and nothing floating-point is atomic: the statistics are
//            bit-identical from run to run, on any stream.
//   NaN / +-Inf are counted per segment and enter neither the buckets nor any statistic (TensorFlow's op fails on them; the caller does).
// Launch sequence: the chunk map (built on the host from the segment table) is copied into the workspace, the counts are zeroed, one
// workgroup per (segment, chunk of HS_CHUNK elements) bins, one workgroup per segment finishes.
#include <float.h>
#include <vector>
#include "tg_common.h"

namespace {

constexpr int HS_LIMITS = 1551, HS_SIDE = 774, HS_THREADS = 256, HS_PER_THREAD = 64, HS_CHUNK = HS_THREADS * HS_PER_THREAD;
constexpr int HS_STATS = 8;              // min, max, num, sum, sum_squares, #NaN, #Inf, (unused)

struct hs_chunk {                        // one workgroup's share: elements [start, start + count) of x, all of segment `seg`
  int64_t start;
  int32_t count;
  int32_t seg;
};
struct hs_seg_chunks {                   // a segment's chunks: partial[first .. first + n)
  int32_t first;
  int32_t n;
};

int64_t hs_align16(int64_t v) { return (v + 15) / 16 * 16; }

struct hs_layout {                       // workspace: [chunk map][per-segment chunk ranges][per-chunk partial statistics]
  int64_t chunks, off_seg, off_partial, bytes;
};

// false when the table is malformed (negative offset / count, or more than 2^31 - 1 chunks)
bool hs_plan(const int64_t* segs, int nseg, hs_layout* L) {
  int64_t chunks = 0;
  for (int s = 0; s < nseg; ++s) {
    if (segs[2 * s] < 0 || segs[2 * s + 1] < 0) return false;
    chunks += (segs[2 * s + 1] + HS_CHUNK - 1) / HS_CHUNK;
    if (chunks > 0x7fffffff) return false;
  }
  L->chunks = chunks;
  L->off_seg = hs_align16(chunks * (int64_t)sizeof(hs_chunk));
  L->off_partial = hs_align16(L->off_seg + (int64_t)nseg * (int64_t)sizeof(hs_seg_chunks));
  L->bytes = L->off_partial + chunks * HS_STATS * (int64_t)sizeof(double);
  return true;
}

// fixed-order sums of a workgroup: valid in thread 0.  `slot` is one of the reduction's LDS rows.
__device__ __forceinline__ double hs_block_sum(double acc, double* slot) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = acc;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < HS_THREADS / 64; ++w) s += slot[w];
  }
  return s;
}

__device__ __forceinline__ double hs_block_min(double acc, double* slot) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc = fmin(acc, __shfl_down(acc, off, 64));
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = acc;
  __syncthreads();
  double s = DBL_MAX;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < HS_THREADS / 64; ++w) s = fmin(s, slot[w]);
  }
  return s;
}

__device__ __forceinline__ double hs_block_max(double acc, double* slot) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc = fmax(acc, __shfl_down(acc, off, 64));
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = acc;
  __syncthreads();
  double s = -DBL_MAX;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < HS_THREADS / 64; ++w) s = fmax(s, slot[w]);
  }
  return s;
}

// the seven statistics of a workgroup's threads -> out[0..8) by thread 0 (each reduction has its own LDS row: one barrier apiece)
__device__ __forceinline__ void hs_block_stats(double mn, double mx, double num, double sum, double sq, double nan, double inf,
                                               double* __restrict__ out) {
  __shared__ double red[7][HS_THREADS / 64];
  const double r0 = hs_block_min(mn, red[0]), r1 = hs_block_max(mx, red[1]), r2 = hs_block_sum(num, red[2]), r3 = hs_block_sum(sum, red[3]);
  const double r4 = hs_block_sum(sq, red[4]), r5 = hs_block_sum(nan, red[5]), r6 = hs_block_sum(inf, red[6]);
  if (threadIdx.x == 0) {
    out[0] = r0; out[1] = r1; out[2] = r2; out[3] = r3; out[4] = r4; out[5] = r5; out[6] = r6; out[7] = 0.0;
  }
}

__global__ void __launch_bounds__(HS_THREADS) tf_histogram_chunk_kernel(const float* __restrict__ x, const hs_chunk* __restrict__ map,
                                                                        const double* __restrict__ limits,
                                                                        unsigned long long* __restrict__ counts, double* __restrict__ partial,
                                                                        int64_t n, int nseg) {
  __shared__ double lim[HS_LIMITS];
  __shared__ unsigned int hist[HS_LIMITS];
  hs_chunk ck = map[blockIdx.x];
  // the map is the host's, checked there; an entry that does not fit the buffer is still never followed (it reads nothing, counts nothing)
  if (ck.start < 0 || ck.count < 0 || ck.count > HS_CHUNK || ck.start > n - ck.count || ck.seg < 0 || ck.seg >= nseg) { ck.count = 0; ck.seg = 0; ck.start = 0; }
  for (int i = threadIdx.x; i < HS_LIMITS; i += HS_THREADS) { lim[i] = limits[i]; hist[i] = 0u; }
  __syncthreads();
  const float* __restrict__ xs = x + ck.start;
  double mn = DBL_MAX, mx = -DBL_MAX, num = 0.0, sum = 0.0, sq = 0.0, nan = 0.0, inf = 0.0;
  const int trips = (ck.count + HS_THREADS - 1) / HS_THREADS;          // uniform over the workgroup: the ballots below see whole waves
  for (int k = 0; k < trips; ++k) {
    const int i = k * HS_THREADS + threadIdx.x;
    int b = -1;
    if (i < ck.count) {
      const float xf = xs[i];
      const double xd = (double)xf;
      if (xf != xf) {
        nan += 1.0;
      } else if (xf == __builtin_inff() || xf == -__builtin_inff()) {
        inf += 1.0;
      } else {
        int lo = 0, hi = HS_LIMITS;                                    // upper_bound: first index whose limit is > xd
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (lim[mid] <= xd) lo = mid + 1; else hi = mid;
        }
        b = lo < HS_LIMITS ? lo : HS_LIMITS - 1;                       // (no finite float reaches the last limit, DBL_MAX)
        mn = fmin(mn, xd); mx = fmax(mx, xd);
        num += 1.0; sum += xd; sq += xd * xd;
      }
    }
    const int first = __builtin_amdgcn_readfirstlane(b);
    if (__all(b == first)) {                                           // one bin for the whole wave: one add of the lane count
      if (first >= 0 && (threadIdx.x & 63) == 0) atomicAdd(&hist[first], 64u);
    } else if (b >= 0) {
      atomicAdd(&hist[b], 1u);
    }
  }
  __syncthreads();
  unsigned long long* __restrict__ dst = counts + (int64_t)ck.seg * HS_LIMITS;
  for (int i = threadIdx.x; i < HS_LIMITS; i += HS_THREADS) {
    const unsigned int c = hist[i];
    if (c) atomicAdd(&dst[i], (unsigned long long)c);
  }
  hs_block_stats(mn, mx, num, sum, sq, nan, inf, partial + (int64_t)blockIdx.x * HS_STATS);
}

__global__ void __launch_bounds__(HS_THREADS) tf_histogram_final_kernel(const hs_seg_chunks* __restrict__ segc, const double* __restrict__ partial,
                                                                        double* __restrict__ stats, int chunks) {
  hs_seg_chunks sc = segc[blockIdx.x];
  if (sc.first < 0 || sc.n < 0 || sc.first > chunks - sc.n) sc.n = 0;
  double mn = DBL_MAX, mx = -DBL_MAX, num = 0.0, sum = 0.0, sq = 0.0, nan = 0.0, inf = 0.0;
  for (int c = threadIdx.x; c < sc.n; c += HS_THREADS) {
    const double* __restrict__ p = partial + (int64_t)(sc.first + c) * HS_STATS;
    mn = fmin(mn, p[0]); mx = fmax(mx, p[1]);
    num += p[2]; sum += p[3]; sq += p[4]; nan += p[5]; inf += p[6];
  }
  hs_block_stats(mn, mx, num, sum, sq, nan, inf, stats + (int64_t)blockIdx.x * HS_STATS);
}

}  // namespace

extern "C" {

int tg_tf_histogram_limits(double* limits_out, int n) {
  TG_REQUIRE(limits_out && n == HS_LIMITS, "tf_histogram_limits: the table has %d entries, got room for %d", HS_LIMITS, n);
  std::vector<double> pos;
  volatile double v = 1e-12;                       // volatile: every product is rounded to double, whatever the host compiler keeps in registers
  while (v < 1e20) {
    pos.push_back((double)v);
    v = v * 1.1;
  }
  TG_REQUIRE((int)pos.size() == HS_SIDE, "tf_histogram_limits: %d positive limits below 1e20, expected %d", (int)pos.size(), HS_SIDE);
  pos.push_back(DBL_MAX);
  const int np = (int)pos.size();
  for (int i = 0; i < np; ++i) limits_out[i] = -pos[np - 1 - i];
  limits_out[np] = 0.0;
  for (int i = 0; i < np; ++i) limits_out[np + 1 + i] = pos[i];
  return TG_OK;
}

int64_t tg_tf_histogram_workspace_bytes(const int64_t* segs, int nseg) {
  if (nseg < 0 || (nseg > 0 && !segs)) { tg::set_error("tf_histogram_workspace_bytes: bad segment table"); return -1; }
  hs_layout L;
  if (!hs_plan(segs, nseg, &L)) { tg::set_error("tf_histogram_workspace_bytes: a segment has a negative offset or count"); return -1; }
  return L.bytes;                                  // 0 for an empty table: nothing is launched, no scratch is touched
}

int tg_tf_histogram_f32(const float* x, int64_t n, const int64_t* segs, int nseg, const double* limits_dev, int64_t* counts, double* stats,
                        void* workspace, int64_t workspace_bytes, void* stream) {
  TG_REQUIRE(nseg >= 0, "tf_histogram: negative segment count");
  if (nseg == 0) return TG_OK;
  TG_REQUIRE(x && segs && limits_dev && counts && stats && workspace && n >= 0, "tf_histogram: bad args");
  TG_REQUIRE(((uintptr_t)workspace % 16 == 0) && ((uintptr_t)counts % 8 == 0) && ((uintptr_t)stats % 8 == 0) && ((uintptr_t)limits_dev % 8 == 0),
             "tf_histogram: workspace must be 16-B aligned, counts / stats / limits 8-B aligned");
  hs_layout L;
  TG_REQUIRE(hs_plan(segs, nseg, &L), "tf_histogram: a segment has a negative offset or count");
  for (int s = 0; s < nseg; ++s)
    TG_REQUIRE(segs[2 * s] <= n && segs[2 * s + 1] <= n - segs[2 * s], "tf_histogram: segment %d = [%lld, +%lld) leaves the buffer of %lld floats", s,
               (long long)segs[2 * s], (long long)segs[2 * s + 1], (long long)n);
  TG_REQUIRE(workspace_bytes >= L.bytes, "tf_histogram: workspace smaller than tg_tf_histogram_workspace_bytes(segs, nseg)");
  hipStream_t st = tg::as_stream(stream);
  tg::ProfScope prof(tg::PC_ELEMWISE, 0, 0.0, st);
  // the map, built here and copied: [chunks of segment 0][of segment 1]... then each segment's range of them
  std::vector<char> host((size_t)L.off_partial, 0);
  hs_chunk* map = reinterpret_cast<hs_chunk*>(host.data());
  hs_seg_chunks* segc = reinterpret_cast<hs_seg_chunks*>(host.data() + L.off_seg);
  int32_t c = 0;
  for (int s = 0; s < nseg; ++s) {
    const int64_t off = segs[2 * s], cnt = segs[2 * s + 1];
    segc[s].first = c;
    for (int64_t done = 0; done < cnt; done += HS_CHUNK, ++c) {
      map[c].start = off + done;
      map[c].count = (int32_t)(cnt - done < HS_CHUNK ? cnt - done : HS_CHUNK);
      map[c].seg = s;
    }
    segc[s].n = c - segc[s].first;
  }
  char* ws = static_cast<char*>(workspace);
  hipError_t e = hipMemcpyAsync(ws, host.data(), host.size(), hipMemcpyHostToDevice, st);    // pageable source: read before the call returns
  if (e != hipSuccess) return tg::hip_fail(e, "hipMemcpyAsync(histogram chunk map)");
  e = hipMemsetAsync(counts, 0, sizeof(int64_t) * (size_t)nseg * HS_LIMITS, st);
  if (e != hipSuccess) return tg::hip_fail(e, "hipMemsetAsync(histogram counts)");
  double* partial = reinterpret_cast<double*>(ws + L.off_partial);
  if (L.chunks > 0) {
    hipLaunchKernelGGL(tf_histogram_chunk_kernel, dim3((unsigned)L.chunks), dim3(HS_THREADS), 0, st, x, reinterpret_cast<const hs_chunk*>(ws),
                       limits_dev, reinterpret_cast<unsigned long long*>(counts), partial, n, nseg);
    TG_CHECK_LAUNCH("tf_histogram_chunk_kernel");
  }
  hipLaunchKernelGGL(tf_histogram_final_kernel, dim3(nseg), dim3(HS_THREADS), 0, st, reinterpret_cast<const hs_seg_chunks*>(ws + L.off_seg),
                     partial, stats, (int)L.chunks);
  TG_CHECK_LAUNCH("tf_histogram_final_kernel");
  return TG_OK;
}

}  // extern "C"
