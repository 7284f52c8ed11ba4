// North-star CNN forward on gfx950, third kernel.
//
//   cnn_head: fc1 split-K reduction + bias + ReLU, fc2, log-softmax/NLL, argmax,
//             and (training) the whole head backward: dlogits, fc2 weight/bias
//             partials, dh = dlogits.W2 * relu'(h) (bf16, + transposed copy for the
//             fc1 weight-gradient GEMM), fc1 bias partials; advances step counters.
//   cnn_head_smooth: cnn_head<train> with label-smoothed targets (--label-smoothing E):
//             t_c = (1 - E) [c = y] + E / 10 in dlogits and the loss, nothing else differs
//             (docs/kernels.md "Label-smoothing head").
// Compiled with the iterative-ilp machine scheduler (build.py FILE_FLAGS).
#include "cnn_common.h"

namespace {

using namespace cnn;

// ---- head: fc1 reduce + bias + ReLU, fc2, CE, and (train) the head backward ----
// One wave per batch row (HEAD_ROWS = 4 rows per workgroup, B/4 workgroups): lane j owns
// hidden units 2j, 2j+1, so the fc2 logits are plain wave reductions and the split-K
// partial loads of a row are spread over a whole wave.

// workgroup blk of nblk (the head's grid).  SMOOTH (train only): the targets are smoothed by
// `eps`, a per-run constant; at eps = 0 every output has the plain head's bits (1 - 0 + 0 / 10 =
// 1, 0 + 0 / 10 = 0 and loss + 0 * x = loss are exact).
template <bool TRAIN, bool SMOOTH = false>
__device__ __forceinline__ void head_body(
    const int blk, const int nblk, const float* __restrict__ part, int S, int B,
    const float* __restrict__ bf1, const float* __restrict__ wf2, const float* __restrict__ bf2,
    const int32_t* __restrict__ ylab, bf16* __restrict__ dh, bf16* __restrict__ dht, int ldt,
    float* __restrict__ slab, double* __restrict__ metrics, int64_t* c0, int64_t* c1, unsigned* c2,
    float* __restrict__ dh32, const LrSched ls, const float eps = 0.f) {
  static_assert(HEAD_ROWS == 4, "one wave per row, 4 waves");
  static_assert(TRAIN || !SMOOTH, "evaluation always uses the plain NLL");
  __shared__ float hs[HEAD_ROWS][HID];
  __shared__ float dhs[HEAD_ROWS][HID];
  __shared__ float dls[HEAD_ROWS][NCLS];
  __shared__ float red[HEAD_ROWS][2];
  const int tid = threadIdx.x, r = tid >> 6, j = tid & 63;
  const int ngroups = (TRAIN ? ldt : B + HEAD_ROWS - 1) / HEAD_ROWS;
  // per-thread slab accumulators across this workgroup's row groups (train)
  float sw[5] = {0.f, 0.f, 0.f, 0.f, 0.f};   // dWfc2 entries tid + 256k
  float sx = 0.f;                             // dbfc2 / dbfc1 / loss / correct entry
  double el = 0.0, ec = 0.0;                  // eval metrics (thread 0)
  int en = 0;
  PDM_STAMP(10);   // head phases in slots 10-15 of this file's buffer (tools/stamps.py)
  const float2 bias = reinterpret_cast<const float2*>(bf1)[j];
  // fc2 weights of this lane's two hidden units, loaded once up front and used by both the
  // logits and dh (reloading them for dh was another memory round trip in the chain)
  float2 w2v[NCLS];
#pragma unroll
  for (int c = 0; c < NCLS; ++c) w2v[c] = reinterpret_cast<const float2*>(wf2 + c * HID)[j];
  for (int grp = blk; grp < ngroups; grp += nblk) {
    const int row = grp * HEAD_ROWS + r;
    const bool valid = row < B;
    const int y = valid ? ylab[row] : 0;
    float2 h = bias;
    const int rc = min(row, B - 1);
    if (S == 32) {
      // the training split count at B <= 256: every partial load in flight at once (one
      // memory round trip -- the partials come from other XCDs' writes, ~1.4 us away)
      float2 u[32];
#pragma unroll
      for (int q = 0; q < 32; ++q)
        u[q] = *reinterpret_cast<const float2*>(part + ((int64_t)q * B + rc) * HID + 2 * j);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < 32; ++q) {
        h.x += u[q].x;
        h.y += u[q].y;
      }
    } else {
      // split-K partials in batches of 16 loads in flight (clamped addresses + selects),
      // summed in split order
      for (int s0 = 0; s0 < S; s0 += 16) {
        float2 u[16];
#pragma unroll
        for (int q = 0; q < 16; ++q)
          u[q] = *reinterpret_cast<const float2*>(part + ((int64_t)min(s0 + q, S - 1) * B + rc) * HID +
                                                  2 * j);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const bool on = s0 + q < S;
          h.x += on ? u[q].x : 0.f;
          h.y += on ? u[q].y : 0.f;
        }
      }
    }
    PDM_STAMP(11);
    h.x = valid ? fmaxf(h.x, 0.f) : 0.f;
    h.y = valid ? fmaxf(h.y, 0.f) : 0.f;

    float lg[NCLS];
#pragma unroll
    for (int c = 0; c < NCLS; ++c) lg[c] = wave_sum_dpp(fmaf(h.y, w2v[c].y, h.x * w2v[c].x)) + bf2[c];
    float prob[NCLS];
    int correct;
    float loss = row_xent<NCLS>(lg, y, prob, correct);
    if (SMOOTH) loss = smooth_loss<NCLS>(lg, y, loss, eps);
    PDM_STAMP(12);
    if (j == 0) {
      red[r][0] = valid ? loss : 0.f;
      red[r][1] = valid ? (float)correct : 0.f;
    }

    if (TRAIN) {
      const float invB = 1.f / (float)B;
      float dl[NCLS];
      if (SMOOTH) {
        const SmoothTarget t(eps, NCLS);
#pragma unroll
        for (int c = 0; c < NCLS; ++c) dl[c] = valid ? (prob[c] - t(c == y)) * invB : 0.f;
      } else {
#pragma unroll
        for (int c = 0; c < NCLS; ++c) dl[c] = valid ? (prob[c] - (c == y ? 1.f : 0.f)) * invB : 0.f;
      }
      float2 dhv = make_float2(0.f, 0.f);
#pragma unroll
      for (int c = 0; c < NCLS; ++c) {
        dhv.x = fmaf(dl[c], w2v[c].x, dhv.x);
        dhv.y = fmaf(dl[c], w2v[c].y, dhv.y);
      }
      dhv.x = h.x > 0.f ? dhv.x : 0.f;
      dhv.y = h.y > 0.f ? dhv.y : 0.f;
      // row < ldt always: rows >= B write zeros (GEMM padding)
      if (dh32 != nullptr) {
        // fp32 step (cnn_f32_*.hip): dh row-major in fp32 (rows >= B are zero, GEMM padding)
        st_ho<8>(reinterpret_cast<float2*>(dh32 + (int64_t)row * HID) + j, dhv);
      } else {
        const bf16x2 o = {to_bf16(dhv.x), to_bf16(dhv.y)};
        // both copies fragment-major (kernels.h frag_pos), the layouts fc1_bwd's dW (dh^T: m =
        // hidden unit, k = batch row) and dX (dh: m = batch row, k = hidden unit) tiles load
        st_ho<8>(&dht[frag_pos(2 * j, row, ldt)], o[0]);
        st_ho<8>(&dht[frag_pos(2 * j + 1, row, ldt)], o[1]);
        st_ho<8>(reinterpret_cast<bf16x2*>(dh + frag_pos(row, 2 * j, HID)), o);
      }
      reinterpret_cast<float2*>(hs[r])[j] = h;
      reinterpret_cast<float2*>(dhs[r])[j] = dhv;
      if (j == 0) {
#pragma unroll
        for (int c = 0; c < NCLS; ++c) dls[r][c] = dl[c];
      }
    }
    PDM_STAMP(13);
    __syncthreads();
    if (TRAIN) {
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const int e = tid + 256 * k;
        const int c = e / HID, n = e - c * HID;
        float a = sw[k];
#pragma unroll
        for (int i = 0; i < HEAD_ROWS; ++i) a = fmaf(dls[i][c], hs[i][n], a);
        sw[k] = a;
      }
      if (tid < NCLS) {
        for (int i = 0; i < HEAD_ROWS; ++i) sx += dls[i][tid];
      } else if (tid >= 16 && tid < 16 + HID) {
        for (int i = 0; i < HEAD_ROWS; ++i) sx += dhs[i][tid - 16];
      } else if (tid == 254 || tid == 255) {
        for (int i = 0; i < HEAD_ROWS; ++i) sx += red[i][tid - 254];
      }
    } else if (tid == 0) {
      for (int i = 0; i < HEAD_ROWS; ++i) {
        el += red[i][0];
        ec += red[i][1];
        en += (grp * HEAD_ROWS + i < B);
      }
    }
    PDM_STAMP(14);
    __syncthreads();   // LDS is rewritten by the next row group
  }
  if (!TRAIN) {
    if (tid == 0) {
      atomicAdd(&metrics[0], el);
      atomicAdd(&metrics[1], ec);
      atomicAdd(&metrics[2], (double)en);
    }
    return;
  }
  float* out = slab + (int64_t)blk * HEAD_SLAB;
#pragma unroll
  for (int k = 0; k < 5; ++k) st_ho<8>(&out[tid + 256 * k], sw[k]);
  if (tid < NCLS) st_ho<8>(&out[NCLS * HID + tid], sx);
  else if (tid >= 16 && tid < 16 + HID) st_ho<8>(&out[NCLS * HID + NCLS + tid - 16], sx);
  else if (tid == 254 || tid == 255) st_ho<8>(&out[HEAD_SLAB - 2 + (tid - 254)], sx);
  if (blk == 0 && tid == 0) {          // pdm_bump_counters for the head's first workgroup
    if (c0) *c0 += 1;
    if (c1) *c1 += 1;
    if (c2) *c2 += 1;
    pdm_lr_advance(ls);                // the step's scheduled learning rate, with its count
  }
  PDM_STAMP(15);
}


template <bool TRAIN>
__global__ __launch_bounds__(256) void cnn_head_kernel(
    const float* __restrict__ part, int S, int B, const float* __restrict__ bf1,
    const float* __restrict__ wf2, const float* __restrict__ bf2, const int32_t* __restrict__ ylab,
    bf16* __restrict__ dh, bf16* __restrict__ dht, int ldt, float* __restrict__ slab,
    double* __restrict__ metrics, int64_t* c0, int64_t* c1, unsigned* c2, float* __restrict__ dh32,
    const LrSched ls) {
  head_body<TRAIN>(blockIdx.x, gridDim.x, part, S, B, bf1, wf2, bf2, ylab, dh, dht, ldt, slab,
                   metrics, c0, c1, c2, dh32, ls);
}

// the training head with smoothed targets: head_body<true>'s geometry, slab layout, stores,
// counter bumps and schedule advance
__global__ __launch_bounds__(256) void cnn_head_smooth_kernel(
    const float* __restrict__ part, int S, int B, const float* __restrict__ bf1,
    const float* __restrict__ wf2, const float* __restrict__ bf2, const int32_t* __restrict__ ylab,
    bf16* __restrict__ dh, bf16* __restrict__ dht, int ldt, float* __restrict__ slab, int64_t* c0,
    int64_t* c1, unsigned* c2, float* __restrict__ dh32, const LrSched ls, const float eps) {
  head_body<true, true>(blockIdx.x, gridDim.x, part, S, B, bf1, wf2, bf2, ylab, dh, dht, ldt, slab,
                        nullptr, c0, c1, c2, dh32, ls, eps);
}

}  // namespace

void launch_cnn_head(const float* part, int splitk, int B, const float* bf1, const float* wf2,
                     const float* bf2, const int32_t* ylab, bool train, __bf16* dh, __bf16* dht,
                     int ldt, float* slab, double* metrics, int64_t* c0, int64_t* c1,
                     unsigned* c2, float* dh32, hipStream_t st, LrSched ls) {
  const int groups = (train ? ldt : B + HEAD_ROWS - 1) / HEAD_ROWS;
  const int nblk = cnn_head_blocks(groups);
  if (train)
    cnn_head_kernel<true><<<nblk, 256, 0, st>>>(part, splitk, B, bf1, wf2, bf2, ylab, dh, dht, ldt,
                                                slab, metrics, c0, c1, c2, dh32, ls);
  else
    cnn_head_kernel<false><<<nblk, 256, 0, st>>>(part, splitk, B, bf1, wf2, bf2, ylab, dh, dht,
                                                 ldt, slab, metrics, c0, c1, c2, dh32,
                                                 LrSched());   // evaluation advances nothing
}

void launch_cnn_head_smooth(const float* part, int splitk, int B, const float* bf1,
                            const float* wf2, const float* bf2, const int32_t* ylab, __bf16* dh,
                            __bf16* dht, int ldt, float* slab, int64_t* c0, int64_t* c1,
                            unsigned* c2, float* dh32, float eps, hipStream_t st, LrSched ls) {
  const int nblk = cnn_head_blocks(ldt / HEAD_ROWS);
  cnn_head_smooth_kernel<<<nblk, 256, 0, st>>>(part, splitk, B, bf1, wf2, bf2, ylab, dh, dht, ldt,
                                               slab, c0, c1, c2, dh32, ls, eps);
}

int cnn_head_blocks(int groups) { return groups < CNN_HEAD_MAX_BLOCKS ? groups : CNN_HEAD_MAX_BLOCKS; }

PDM_STAMP_READER(head)
