// Dropout on the CNN's 128 hidden units: the masking twin of cnn_head<train> (cnn_head.hip).
//
//   cnn_head_dropout: fc1 split-K reduction + bias + ReLU, the dropout mask, fc2,
//             log-softmax/NLL, argmax and the whole head backward, in cnn_head's geometry (one
//             wave per row, HEAD_ROWS rows per group, grid-stride over groups), with its slab
//             layout, dh / dh^T fragment-major stores, dh32 mode, counter bumps and metrics.
//             Train-only: evaluation and prediction keep their kernels.
//   dropout_mask_rows: the keep mask alone, uint8 [B][128], from the same device function.
//
// The mask is integer-only (docs/kernels.md "Dropout head"; the CPU twin and oracle is
// data/dropout.py): for the sample with dataset index i, epoch e and hidden unit n,
// Philox4x32-10 with counter (i, e, 1, n >> 3) and key (seed lo, seed hi); r = output word
// (n >> 1) & 3; u = r's low 16 bits for even n, its high 16 bits for odd n; keep iff u >= T.
// Kept units are scaled by scale = fp32(65536 / (65536 - T)), dropped ones are zero.  Lane j
// owns units 2j and 2j + 1: one Philox block (n >> 3 = j >> 2), one word (j & 3).
//
// Which sample a row is comes with its label: ylab[row] = label | (dataset index << 4), as the
// step code uploads the training labels when dropout is on (the forward kernels and the epoch
// gathers copy label words verbatim).  The epoch is a device word the program fills in stream
// order at each epoch boundary, so one set of step graphs serves every epoch.
// Compiled with cnn_head's machine scheduler (build.py FILE_FLAGS).
#include "cnn_common.h"
#include "philox.h"

namespace {

using namespace cnn;

// the 32-bit draw of lane j's two hidden units (2j: low half, 2j + 1: high half)
__device__ __forceinline__ uint32_t dropout_draw(uint32_t index, uint32_t epoch, int j, uint32_t k0,
                                                 uint32_t k1) {
  uint32_t r[4];
  philox4x32_10(index, epoch, 1u, (uint32_t)(j >> 2), k0, k1, r);
  const int w = j & 3;
  return w == 0 ? r[0] : w == 1 ? r[1] : w == 2 ? r[2] : r[3];
}
__device__ __forceinline__ bool dropout_keep_even(uint32_t draw, uint32_t T) { return (draw & 0xffffu) >= T; }
__device__ __forceinline__ bool dropout_keep_odd(uint32_t draw, uint32_t T) { return (draw >> 16) >= T; }

// head_body<true> of cnn_head.hip with the mask between the ReLU and fc2; at T = 0 (scale 1)
// every output is bit-identical to cnn_head's (tests/test_gpu_dropout.py).  eps: label
// smoothing of the targets as in cnn_head_smooth; eps = 0 gives the unsmoothed bits
// (tests/test_gpu_label_smoothing.py).
__global__ __launch_bounds__(256) void cnn_head_dropout_kernel(
    const float* __restrict__ part, int S, int B, const float* __restrict__ bf1,
    const float* __restrict__ wf2, const float* __restrict__ bf2, const int32_t* __restrict__ ylab,
    bf16* __restrict__ dh, bf16* __restrict__ dht, int ldt, float* __restrict__ slab, int64_t* c0,
    int64_t* c1, unsigned* c2, float* __restrict__ dh32, const uint32_t* __restrict__ epoch_word,
    uint32_t k0, uint32_t k1, uint32_t T, float scale, const LrSched ls, const float eps) {
  static_assert(HEAD_ROWS == 4, "one wave per row, 4 waves");
  __shared__ float hs[HEAD_ROWS][HID];
  __shared__ float dhs[HEAD_ROWS][HID];
  __shared__ float dls[HEAD_ROWS][NCLS];
  __shared__ float red[HEAD_ROWS][2];
  const int blk = blockIdx.x, nblk = gridDim.x;
  const int tid = threadIdx.x, r = tid >> 6, j = tid & 63;
  const int ngroups = ldt / HEAD_ROWS;
  // per-thread slab accumulators across this workgroup's row groups
  float sw[5] = {0.f, 0.f, 0.f, 0.f, 0.f};   // dWfc2 entries tid + 256k
  float sx = 0.f;                             // dbfc2 / dbfc1 / loss / correct entry
  const uint32_t epoch = *epoch_word;
  const float2 bias = reinterpret_cast<const float2*>(bf1)[j];
  float2 w2v[NCLS];
#pragma unroll
  for (int c = 0; c < NCLS; ++c) w2v[c] = reinterpret_cast<const float2*>(wf2 + c * HID)[j];
  for (int grp = blk; grp < ngroups; grp += nblk) {
    const int row = grp * HEAD_ROWS + r;
    const bool valid = row < B;
    // label word: class in the low 4 bits, dataset index above (padding rows: no draw needed,
    // their h is zero either way)
    const uint32_t word = valid ? (uint32_t)ylab[row] : 0u;
    const int y = (int)(word & 15u);
    __builtin_amdgcn_sched_barrier(0);   // the label load is issued ahead of the partial loads
    uint32_t draw;
    float2 h = bias;
    const int rc = min(row, B - 1);
    if (S == 32) {
      float2 u[32];
#pragma unroll
      for (int q = 0; q < 32; ++q)
        u[q] = *reinterpret_cast<const float2*>(part + ((int64_t)q * B + rc) * HID + 2 * j);
      __builtin_amdgcn_sched_barrier(0);
      // the draw needs the label word only (loaded before the partials): its ~80 integer
      // operations run while the partial loads are in flight
      draw = dropout_draw(word >> 4, epoch, j, k0, k1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < 32; ++q) {
        h.x += u[q].x;
        h.y += u[q].y;
      }
    } else {
      draw = dropout_draw(word >> 4, epoch, j, k0, k1);
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
    h.x = valid ? fmaxf(h.x, 0.f) : 0.f;
    h.y = valid ? fmaxf(h.y, 0.f) : 0.f;
    const bool kx = dropout_keep_even(draw, T), ky = dropout_keep_odd(draw, T);
    // hd: what fc2 sees
    const float2 hd = make_float2(kx ? h.x * scale : 0.f, ky ? h.y * scale : 0.f);

    float lg[NCLS];
#pragma unroll
    for (int c = 0; c < NCLS; ++c) lg[c] = wave_sum_dpp(fmaf(hd.y, w2v[c].y, hd.x * w2v[c].x)) + bf2[c];
    float prob[NCLS];
    int correct;
    const float loss = smooth_loss<NCLS>(lg, y, row_xent<NCLS>(lg, y, prob, correct), eps);
    if (j == 0) {
      red[r][0] = valid ? loss : 0.f;
      red[r][1] = valid ? (float)correct : 0.f;
    }

    const float invB = 1.f / (float)B;
    float dl[NCLS];
    const SmoothTarget t(eps, NCLS);
#pragma unroll
    for (int c = 0; c < NCLS; ++c) dl[c] = valid ? (prob[c] - t(c == y)) * invB : 0.f;
    float2 dhv = make_float2(0.f, 0.f);
#pragma unroll
    for (int c = 0; c < NCLS; ++c) {
      dhv.x = fmaf(dl[c], w2v[c].x, dhv.x);
      dhv.y = fmaf(dl[c], w2v[c].y, dhv.y);
    }
    // dh = (dl . W2) * (keep ? scale : 0) * [h > 0]; a dropped unit's entry is exactly +0
    dhv.x = (h.x > 0.f && kx) ? dhv.x * scale : 0.f;
    dhv.y = (h.y > 0.f && ky) ? dhv.y * scale : 0.f;
    // row < ldt always: rows >= B write zeros (GEMM padding)
    if (dh32 != nullptr) {
      st_ho<8>(reinterpret_cast<float2*>(dh32 + (int64_t)row * HID) + j, dhv);
    } else {
      const bf16x2 o = {to_bf16(dhv.x), to_bf16(dhv.y)};
      st_ho<8>(&dht[frag_pos(2 * j, row, ldt)], o[0]);
      st_ho<8>(&dht[frag_pos(2 * j + 1, row, ldt)], o[1]);
      st_ho<8>(reinterpret_cast<bf16x2*>(dh + frag_pos(row, 2 * j, HID)), o);
    }
    reinterpret_cast<float2*>(hs[r])[j] = hd;
    reinterpret_cast<float2*>(dhs[r])[j] = dhv;
    if (j == 0) {
#pragma unroll
      for (int c = 0; c < NCLS; ++c) dls[r][c] = dl[c];
    }
    __syncthreads();
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
    __syncthreads();   // LDS is rewritten by the next row group
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
}

// one wave per row, lane j writing the keep bytes of units 2j, 2j + 1
__global__ __launch_bounds__(256) void dropout_mask_rows_kernel(
    const int32_t* __restrict__ ylab, int B, const uint32_t* __restrict__ epoch_word, uint32_t k0,
    uint32_t k1, uint32_t T, uint8_t* __restrict__ out) {
  const int row = blockIdx.x * HEAD_ROWS + (threadIdx.x >> 6), j = threadIdx.x & 63;
  if (row >= B) return;
  const uint32_t draw = dropout_draw((uint32_t)ylab[row] >> 4, *epoch_word, j, k0, k1);
  reinterpret_cast<uchar2*>(out + (int64_t)row * HID)[j] =
      make_uchar2(dropout_keep_even(draw, T) ? 1 : 0, dropout_keep_odd(draw, T) ? 1 : 0);
}

}  // namespace

void launch_cnn_head_dropout(const float* part, int splitk, int B, const float* bf1,
                             const float* wf2, const float* bf2, const int32_t* ylab, __bf16* dh,
                             __bf16* dht, int ldt, float* slab, int64_t* c0, int64_t* c1,
                             unsigned* c2, float* dh32, const uint32_t* epoch, uint64_t seed,
                             uint32_t T, float scale, hipStream_t st, LrSched ls, float eps) {
  const int nblk = cnn_head_blocks(ldt / HEAD_ROWS);
  cnn_head_dropout_kernel<<<nblk, 256, 0, st>>>(
      part, splitk, B, bf1, wf2, bf2, ylab, dh, dht, ldt, slab, c0, c1, c2, dh32, epoch,
      (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), T, scale, ls, eps);
}

void launch_dropout_mask_rows(const int32_t* ylab, int B, const uint32_t* epoch, uint64_t seed,
                              uint32_t T, uint8_t* out, hipStream_t st) {
  if (B <= 0) return;
  dropout_mask_rows_kernel<<<(B + HEAD_ROWS - 1) / HEAD_ROWS, 256, 0, st>>>(
      ylab, B, epoch, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), T, out);
}
