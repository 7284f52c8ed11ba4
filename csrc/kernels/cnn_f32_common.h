// What the two fp32 kernel sets share: cnn_f32_exact.hip (every product on the fp32 MFMA) and
// cnn_f32x3.hip (split-bf16 products, the default; holds the launch_f32_* dispatchers).
//
// MFMA 16x16x4 f32 operand layout, lane l = 16 g + i: A[m = i][k = g], B[k = g][n = i],
// D[m = 4 g + r][n = i] for r = 0..3.
#pragma once
#include "cnn_common.h"

namespace cnn {

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

constexpr int FT = 512;                            // threads of the fwd / conv_bwd workgroups
constexpr int CB_R = 4, CB_S = H2 / CB_R;          // conv_bwd row band: 4 conv2 rows, 6 per image
constexpr int SLB_DB2 = CNN_CONV_SLAB_DB2, SLB_DW1 = CNN_CONV_SLAB_DW1, SLB_DB1 = CNN_CONV_SLAB_DB1;

// fc1_bwd tiles (both sets: one grid shape)
constexpr int DWF = 64;                 // dW tile: 128 n x 64 features
constexpr int DW_T = FEAT / DWF;        // 144
constexpr int DXF = 256;                // dX tile: 32 rows x 256 features
constexpr int DX_T = FEAT / DXF;        // 36 per 32 rows
constexpr int HRB = (HEAD_SLAB + 63) / 64;   // head-slab reduction workgroups (23)

// head-slab reduction (fc1_bwd's third role, both product modes): 64 slab columns x 4 groups
// per workgroup, fixed order (the bf16 fc1_bwd_kernel in fc1_bwd.hip has its own copy)
__device__ __forceinline__ void head_slab_reduce(float* sm, int hb, const float* __restrict__ head_slab,
                                                 int head_blocks, int B, float* __restrict__ gwf2,
                                                 float* __restrict__ gbf2, float* __restrict__ gbf1,
                                                 double* __restrict__ metrics) {
  const int tid = threadIdx.x;
  {
    float* rs = sm;
    double* rd = reinterpret_cast<double*>(sm + 256);
    const int e = hb * 64 + (tid & 63), grp = tid >> 6;
    const int ec = min(e, HEAD_SLAB - 1);
    float sacc = 0.f;
    double sd = 0.0;
    for (int j0 = grp; j0 < head_blocks; j0 += 4 * 8) {   // 8 loads in flight, fixed order
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = head_slab[(int64_t)min(j0 + 4 * u, head_blocks - 1) * HEAD_SLAB + ec];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float x = (j0 + 4 * u < head_blocks) ? v[u] : 0.f;
        sacc += x;
        sd += (double)x;
      }
    }
    rs[tid] = sacc;
    rd[tid] = sd;
    __syncthreads();
    if (tid < 64 && e < HEAD_SLAB) {
      sacc = ((rs[tid] + rs[64 + tid]) + rs[128 + tid]) + rs[192 + tid];
      sd = ((rd[tid] + rd[64 + tid]) + rd[128 + tid]) + rd[192 + tid];
      if (e < NCLS * HID) gwf2[e] = sacc;
      else if (e < NCLS * HID + NCLS) gbf2[e - NCLS * HID] = sacc;
      else if (e < NCLS * HID + NCLS + HID) gbf1[e - NCLS * HID - NCLS] = sacc;
      else if (e == HEAD_SLAB - 2) { metrics[0] += sd; metrics[2] += (double)B; }
      else metrics[1] += sd;
    }
  }
}

}  // namespace cnn

// the exact set's launchers (cnn_f32_exact.hip): launch_f32_* (kernels.h) without the x3 arguments
void launch_f32_exact_fwd(const uint8_t* images, const int32_t* labels, int64_t nrow,
                          const int64_t* ctr, StepRows sr, int B, const float* w1, const float* b1,
                          const float* w2, const float* b2, float* pool, uint8_t* pmask, float* a1g,
                          float* xng, int32_t* ylab, hipStream_t st);
void launch_f32_exact_fc1_fwd(const float* pool, const float* w1, float* part, int B, int splitk,
                              hipStream_t st);
void launch_f32_exact_fc1_bwd(const float* dh, int ldt, const float* pool, const float* w1, int B,
                              float* gwf1, float* dpool, const float* head_slab, int head_blocks,
                              float* gwf2, float* gbf2, float* gbf1, double* metrics, hipStream_t st);
void launch_f32_exact_conv_bwd(const float* a1g, const float* xng, const float* dpool,
                               const uint8_t* pmask, const float* w2, int B, int ipb, float* slab,
                               hipStream_t st);
