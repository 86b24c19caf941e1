// Internal: the halo-tiled bf16 3x3 convolution (conv3x3_bf16.hip) that igemm_launch (igemm.hip) routes matching launches to, and the
// request both of them execute.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/tg_kernels.h"

namespace tg {

enum IgemmOperands { IGEMM_F32 = 0, IGEMM_BF16 = 1, IGEMM_BF16_IN16 = 2 };   // tg_igemm_workspace_bytes' `bf16`; IN16: `in` holds bf16
// epilogue statistics: column sums [nseg][c_out] (tg_igemm_colsum_* / _actsum_*); [nseg][2][c_out] sums and sums of squares of the activated
// output for a batch norm behind the layer (_bnstat_*) or that batch norm's backward sums of dy and dy * ymul (_bnbwdstat_*)
enum IgemmStat { IGEMM_STAT_NONE = 0, IGEMM_STAT_COLSUM, IGEMM_STAT_BN, IGEMM_STAT_BNBWD };

// One implicit-GEMM launch as its entry point received it.  Entry points name the fields they set; the rest is zero.
struct IgemmCall {
  const tg_igemm_desc* descs; int n_desc;
  const float *in, *w, *bias; float* out;
  IgemmOperands ops;
  double* sums; const int32_t* seg_rows; int nseg; IgemmStat stat;      // statistics group (stat = NONE: sums = NULL)
  const float* ymul; int ymul_act; float ymul_alpha;                    // out = acc * act'(ymul) (actsum); the batch norm's input x (bnbwdstat)
  const float* lab; int lab_n;                                          // tg_igemm_labels_*
  void* scratch; int64_t scratch_bytes; void* stream;                   // caller-owned scratch, sized by tg_igemm_workspace_bytes
  bool bf16() const { return ops != IGEMM_F32; }
  bool in16() const { return ops == IGEMM_BF16_IN16; }
  int stat2() const { return stat == IGEMM_STAT_BN ? 1 : stat == IGEMM_STAT_BNBWD ? 2 : 0; }   // the kernels' STAT2 parameter
};

// 9 taps of a 3x3 window, stride 1, output grid = input grid (SAME), width 16 / 32 / 64 with 256 / width dividing the height, 64 | ld_in,
// 128 | c_out, segments of whole images
bool conv3x3_bf16_applicable(const tg_igemm_desc* d, int n_desc, const int32_t* seg_rows, int nseg, bool bf16);   // bf16 = false: the exact-fp32 form (32 | ld_in)
// > 0: the launch has the kernel's shape but does not fill whole rounds of one workgroup per CU; that many leading images do
int conv3x3_bf16_split_images(const tg_igemm_desc* d, int n_desc, const int32_t* seg_rows, int nseg, bool bf16);
// c.descs[0] on the halo kernel; the byte extents of its three tensors (in_bytes counts bf16 bytes for a bf16-stored input)
int conv3x3_bf16_launch(const IgemmCall& c, uint32_t in_bytes, uint32_t w_bytes, uint32_t out_bytes);
// bytes of caller-owned scratch a bf16 launch of these descriptors needs for the packed filter (0: the layer never takes the halo kernel)
int64_t conv3x3_bf16_pack_bytes(const tg_igemm_desc* d, int n_desc);

// shared by the halo kernels (conv3x3_bf16.hip owns the state): tg_conv3x3_policy's value, the device's CU count, the launch counter
int halo_policy();
int halo_compute_units();
void halo_count_launch();

// wgrad3x3.hip: the filter gradient of the same layers with the activation tile read once for the nine taps
bool wgrad3x3_applicable(const tg_igemm_desc* d, int n_split, bool bf16, int policy, int compute_units);
int wgrad3x3_splits(const tg_igemm_desc* d, bool bf16, int policy, int compute_units);
int wgrad3x3_launch(const tg_igemm_desc* d, const float* in, const float* dout, float* slab, int n_split, uint32_t in_bytes, uint32_t dout_bytes,
                    hipStream_t s, bool bf16, bool in16 = false);   // in16: `in` holds bf16 (in_bytes counts its bytes)

}  // namespace tg
