// The CNN head, defined once for every kernel that runs it (docs/kernels.md "cnn_head"):
//   cnn_head.hip       cnn_head<train>, cnn_head<eval>, cnn_head_smooth
//   cnn_head_drop.hip  cnn_head_dropout
//   cnn_head_mix.hip   cnn_head_mixup
//   predict.hip        cnn_predict_head
// One wave per batch row (HEAD_ROWS = 4 rows per workgroup), a grid-stride over the row groups
// on at most CNN_HEAD_MAX_BLOCKS workgroups: lane j owns hidden units 2j, 2j+1, so the fc2
// logits are plain wave reductions and the split-K partial loads of a row are spread over a
// whole wave.  The variants are compile-time switches of head_body: a kernel's instruction
// stream holds nothing of the others.
#pragma once
#include "cnn_common.h"
#include "mixup.h"
#include "philox.h"

namespace cnn {

// ---- dropout on the 128 hidden units (docs/kernels.md "Dropout head") ----
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

// what the dropout and mixup variants take beyond the plain head's arguments
struct HeadDraws {
  const uint32_t* epoch_word;          // the device epoch word
  uint32_t k0, k1, T;                  // dropout: Philox key, threshold
  float scale;                         //          fp32(65536 / (65536 - T))
  const int32_t* train_labels;         // mixup: the tagged training labels, their count,
  uint32_t ntrain;                     //        the blend-weight table and the Philox key
  const int32_t* qt;
  uint32_t mk0, mk1;
};

// what the prediction variant writes per row (predict.hip; docs/kernels.md "Prediction head")
struct HeadRows {
  float* logp;          // fp32 [B][10] log-softmax
  int32_t* pred;        // int32 [B] first maximum
  int64_t* confusion;   // int64 [10][10] or null
};

// ---- mixup (docs/kernels.md "Mixup") ----
// row_xent (common.h) for two classes: the same operations in the same order for y, plus
// the partner's nll2 = lse - l_y2
template <int N>
__device__ __forceinline__ float row_xent2(const float (&lg)[N], int y, int y2, float (&p)[N],
                                           int& correct, float& nll2) {
  float m = lg[0];
  int am = 0;
#pragma unroll
  for (int n = 1; n < N; ++n)
    if (lg[n] > m) { m = lg[n]; am = n; }
  float s = 0.f;
#pragma unroll
  for (int n = 0; n < N; ++n) { p[n] = expf(lg[n] - m); s += p[n]; }
  const float lse = m + logf(s);
  const float inv = 1.f / s;
#pragma unroll
  for (int n = 0; n < N; ++n) p[n] *= inv;
  correct = (am == y);
  float ly = lg[0], ly2 = lg[0];
#pragma unroll
  for (int n = 1; n < N; ++n) {
    ly = (n == y) ? lg[n] : ly;
    ly2 = (n == y2) ? lg[n] : ly2;
  }
  nll2 = lse - ly2;
  return lse - ly;
}

// ---- the head: fc1 reduce + bias + ReLU, fc2, CE, and (train) the head backward ----
// Workgroup blk of nblk (the head's grid).  The variants that exist:
//   <false>                     evaluation: the plain NLL into metrics
//   <false, ..., PREDICT>       + logp / pred / confusion per row (pr); labels and metrics optional
//   <true>                      training
//   <true, true>                + targets smoothed by `eps`, a per-run constant; at eps = 0 every
//                               output has the plain head's bits (1 - 0 + 0 / 10 = 1, 0 + 0 / 10 =
//                               0 and loss + 0 * x = loss are exact)
//   <true, true, true>          + dropout between the ReLU and fc2.  ylab[row] = label | (dataset
//                               index << 4); at T = 0 (scale 1) every output has the bits above
//   <true, true, true, true>    + the target mixed with the partner's (mixup.h): lambda = q / 256
//                               and 1 - lambda are exact, so with q = 256 every output has the
//                               bits above (1 * on + 0 * x and loss + 0 * finite are exact)
template <bool TRAIN, bool SMOOTH = false, bool DROP = false, bool MIX = false, bool PREDICT = false>
__device__ __forceinline__ void head_body(
    const int blk, const int nblk, const float* __restrict__ part, int S, int B,
    const float* __restrict__ bf1, const float* __restrict__ wf2, const float* __restrict__ bf2,
    const int32_t* __restrict__ ylab, bf16* __restrict__ dh, bf16* __restrict__ dht, int ldt,
    float* __restrict__ slab, double* __restrict__ metrics, int64_t* c0, int64_t* c1, unsigned* c2,
    float* __restrict__ dh32, const LrSched ls, const float eps = 0.f,
    const HeadDraws dr = HeadDraws(), const HeadRows pr = HeadRows()) {
  static_assert(HEAD_ROWS == 4, "one wave per row, 4 waves");
  static_assert((TRAIN || !SMOOTH) && (SMOOTH || !DROP) && (DROP || !MIX),
                "evaluation always uses the plain NLL; each training variant adds to the last");
  static_assert(!PREDICT || !TRAIN, "prediction is evaluation plus per-row outputs");
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
  uint32_t epoch = 0u;
  if constexpr (DROP) epoch = *dr.epoch_word;
  // head phases in slots 10-15 of the including file's stamp buffer; only cnn_head.hip has a
  // reader (tools/stamps.py), the other files' stamps go unread
  PDM_STAMP(10);
  const float2 bias = reinterpret_cast<const float2*>(bf1)[j];
  // fc2 weights of this lane's two hidden units, loaded once up front and used by both the
  // logits and dh (reloading them for dh was another memory round trip in the chain)
  float2 w2v[NCLS];
#pragma unroll
  for (int c = 0; c < NCLS; ++c) w2v[c] = reinterpret_cast<const float2*>(wf2 + c * HID)[j];
  for (int grp = blk; grp < ngroups; grp += nblk) {
    const int row = grp * HEAD_ROWS + r;
    const bool valid = row < B;
    // the label; DROP: the class in the low 4 bits of the word, the dataset index above (padding
    // rows draw as sample 0: their loads stay in range, and nothing of theirs is kept)
    int y = (valid && (!PREDICT || ylab != nullptr)) ? ylab[row] : 0;   // PREDICT: labels optional
    uint32_t index = 0u, draw = 0u;
    int y2 = 0, mq = 256;
    if constexpr (DROP) {
      index = (uint32_t)y >> 4;
      y &= 15;
      // the label load is issued ahead of the partial loads
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (MIX) {
      // the row's pair (the same in every lane: one wave per row): the Philox block and the two
      // dependent loads, QT[.] and the partner's label, go out ahead of the partials too
      int mj;
      mixup_draw(index, epoch, dr.mk0, dr.mk1, dr.ntrain, dr.qt, mj, mq);
      y2 = dr.train_labels[mj] & 15;
      __builtin_amdgcn_sched_barrier(0);
    }
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
      if constexpr (DROP) {
        // the draw needs the label word only (loaded before the partials): its ~80 integer
        // operations run while the partial loads are in flight
        draw = dropout_draw(index, epoch, j, dr.k0, dr.k1);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int q = 0; q < 32; ++q) {
        h.x += u[q].x;
        h.y += u[q].y;
      }
    } else {
      if constexpr (DROP) draw = dropout_draw(index, epoch, j, dr.k0, dr.k1);
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
    if constexpr (DROP) {   // from here on h is what fc2 sees
      h.x = dropout_keep_even(draw, dr.T) ? h.x * dr.scale : 0.f;
      h.y = dropout_keep_odd(draw, dr.T) ? h.y * dr.scale : 0.f;
    }

    float lg[NCLS];
#pragma unroll
    for (int c = 0; c < NCLS; ++c) lg[c] = wave_sum_dpp(fmaf(h.y, w2v[c].y, h.x * w2v[c].x)) + bf2[c];
    float prob[NCLS];
    int correct;
    float loss, lam = 1.f, oml = 0.f;
    if constexpr (MIX) {
      float nll2;   // the partner's
      loss = row_xent2<NCLS>(lg, y, y2, prob, correct, nll2);
      // lambda = q / 256 and 1 - lambda, both exact
      lam = (float)mq * (1.f / 256.f), oml = (float)(256 - mq) * (1.f / 256.f);
      loss = lam * smooth_loss<NCLS>(lg, y, loss, eps) + oml * smooth_loss<NCLS>(lg, y2, nll2, eps);
    } else if constexpr (PREDICT) {
      const int am = row_logp<NCLS>(lg, y, prob, loss);   // prob: the log-probabilities here
      correct = (am == y);
      // lane c's own class (selects, not a register-array index: that would go to scratch)
      float mine = prob[0];
#pragma unroll
      for (int c = 1; c < NCLS; ++c) mine = (j == c) ? prob[c] : mine;
      if (valid && j < NCLS) pr.logp[(int64_t)row * NCLS + j] = mine;
      if (valid && j == 0) {
        pr.pred[row] = am;
        if (pr.confusion != nullptr) count_confusion<NCLS>(pr.confusion, y, am);
      }
      if (metrics == nullptr) continue;   // (kernel-uniform) the evaluation sums are optional
    } else {
      loss = row_xent<NCLS>(lg, y, prob, correct);
      if (SMOOTH) loss = smooth_loss<NCLS>(lg, y, loss, eps);
    }
    PDM_STAMP(12);
    if (j == 0) {
      red[r][0] = valid ? loss : 0.f;
      red[r][1] = valid ? (float)correct : 0.f;
    }

    if (TRAIN) {
      const float invB = 1.f / (float)B;
      float dl[NCLS];
      if constexpr (MIX) {
        const SmoothTarget t(eps, NCLS);
#pragma unroll
        for (int c = 0; c < NCLS; ++c) {
          const float tc = lam * t(c == y) + oml * t(c == y2);
          dl[c] = valid ? (prob[c] - tc) * invB : 0.f;
        }
      } else if (SMOOTH) {
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
      if constexpr (DROP) {
        // dh = (dl . W2) * (keep ? scale : 0) * [ReLU > 0]: the masked h is positive exactly
        // where the unit was kept and its ReLU was (scale >= 1); a dropped unit's entry is +0
        dhv.x = h.x > 0.f ? dhv.x * dr.scale : 0.f;
        dhv.y = h.y > 0.f ? dhv.y * dr.scale : 0.f;
      } else {
        dhv.x = h.x > 0.f ? dhv.x : 0.f;
        dhv.y = h.y > 0.f ? dhv.y : 0.f;
      }
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
    if constexpr (PREDICT) {
      if (metrics == nullptr) return;
    }
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

}  // namespace cnn
