// Mixup in the CNN's training head: the two-class twin of cnn_head_dropout (cnn_head_drop.hip).
//
//   cnn_head_mixup: cnn_head_dropout -- fc1 split-K reduction + bias + ReLU, the dropout mask,
//             fc2, log-softmax, argmax and the whole head backward, in cnn_head's geometry, with
//             its slab layout, dh / dh^T fragment-major stores, dh32 mode, counter bumps and
//             metrics -- with the row's target mixed with its partner's:
//                 t    = lambda t(y) + (1 - lambda) t(y2),   t(.) the label-smoothed one-hot
//                 loss = lambda loss_E(y) + (1 - lambda) loss_E(y2)
//                 dlogits = (softmax - t) / B,   correct against y (the primary sample).
//             One kernel composes mixup with dropout (T, scale; T = 0: none) and label
//             smoothing (E; 0: none).  Train-only.
//   mixup_pairs_rows: (j, q, y2) of B rows alone, int32 [B][3], from the same device function.
//
// The pair is the epoch gather's (kernels/mixup.h; docs/kernels.md "Mixup"; the CPU twin and
// oracle is data/mixup.py): a row's dataset index i comes in its label word, ylab[row] = label |
// (i << 4), the epoch is the device epoch word (both as the dropout head's), and Philox counter
// (i, e, 3, 0) gives the partner j of the N training samples and q = QT[.], lambda = q / 256.
// y2 is read from the tagged training labels, train_labels[j] & 15.  lambda and 1 - lambda are
// exact in fp32 (q is an integer in 128..256), so with QT == 256 everywhere every output is
// cnn_head_dropout's bit for bit: 1 * on + 0 * x and loss + 0 * finite are exact.
// Compiled with cnn_head's machine scheduler (build.py FILE_FLAGS).
#include "cnn_common.h"
#include "philox.h"
#include "mixup.h"

namespace {

using namespace cnn;

// cnn_head_drop.hip's draw: the 32-bit draw of lane j's two hidden units
__device__ __forceinline__ uint32_t dropout_draw(uint32_t index, uint32_t epoch, int j, uint32_t k0,
                                                 uint32_t k1) {
  uint32_t r[4];
  philox4x32_10(index, epoch, 1u, (uint32_t)(j >> 2), k0, k1, r);
  const int w = j & 3;
  return w == 0 ? r[0] : w == 1 ? r[1] : w == 2 ? r[2] : r[3];
}
__device__ __forceinline__ bool dropout_keep_even(uint32_t draw, uint32_t T) { return (draw & 0xffffu) >= T; }
__device__ __forceinline__ bool dropout_keep_odd(uint32_t draw, uint32_t T) { return (draw >> 16) >= T; }

// row_xent (cnn_common.h) for two classes: the same operations in the same order for y, plus
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

__global__ __launch_bounds__(256) void cnn_head_mixup_kernel(
    const float* __restrict__ part, int S, int B, const float* __restrict__ bf1,
    const float* __restrict__ wf2, const float* __restrict__ bf2, const int32_t* __restrict__ ylab,
    bf16* __restrict__ dh, bf16* __restrict__ dht, int ldt, float* __restrict__ slab, int64_t* c0,
    int64_t* c1, unsigned* c2, float* __restrict__ dh32, const uint32_t* __restrict__ epoch_word,
    uint32_t k0, uint32_t k1, uint32_t T, float scale, const LrSched ls, const float eps,
    const int32_t* __restrict__ train_labels, uint32_t ntrain, const int32_t* __restrict__ qt,
    uint32_t mk0, uint32_t mk1) {
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
    // label word: class in the low 4 bits, dataset index above (padding rows draw as sample 0:
    // their loads stay in range, and nothing of theirs is kept)
    const uint32_t word = valid ? (uint32_t)ylab[row] : 0u;
    const int y = (int)(word & 15u);
    __builtin_amdgcn_sched_barrier(0);   // the label load is issued ahead of the partial loads
    // the row's pair (the same in every lane: one wave per row): the Philox block and the two
    // dependent loads, QT[.] and the partner's label, go out ahead of the partials too
    int mj, mq;
    mixup_draw(word >> 4, epoch, mk0, mk1, ntrain, qt, mj, mq);
    const int y2 = train_labels[mj] & 15;
    __builtin_amdgcn_sched_barrier(0);
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
    float nll2;
    const float nll = row_xent2<NCLS>(lg, y, y2, prob, correct, nll2);
    // lambda = q / 256 and 1 - lambda, both exact
    const float lam = (float)mq * (1.f / 256.f), oml = (float)(256 - mq) * (1.f / 256.f);
    const float loss1 = smooth_loss<NCLS>(lg, y, nll, eps);
    const float loss2 = smooth_loss<NCLS>(lg, y2, nll2, eps);
    const float loss = lam * loss1 + oml * loss2;
    if (j == 0) {
      red[r][0] = valid ? loss : 0.f;
      red[r][1] = valid ? (float)correct : 0.f;
    }

    const float invB = 1.f / (float)B;
    float dl[NCLS];
    const SmoothTarget t(eps, NCLS);
#pragma unroll
    for (int c = 0; c < NCLS; ++c) {
      const float tc = lam * t(c == y) + oml * t(c == y2);
      dl[c] = valid ? (prob[c] - tc) * invB : 0.f;
    }
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

// one thread per row: (j, q, y2)
__global__ __launch_bounds__(256) void mixup_pairs_rows_kernel(
    const int32_t* __restrict__ ylab, int B, const uint32_t* __restrict__ epoch_word,
    const int32_t* __restrict__ train_labels, uint32_t ntrain, const int32_t* __restrict__ qt,
    uint32_t mk0, uint32_t mk1, int32_t* __restrict__ out) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= B) return;
  int mj, mq;
  mixup_draw((uint32_t)ylab[row] >> 4, *epoch_word, mk0, mk1, ntrain, qt, mj, mq);
  out[3 * row] = mj;
  out[3 * row + 1] = mq;
  out[3 * row + 2] = train_labels[mj] & 15;
}

}  // namespace

void launch_cnn_head_mixup(const float* part, int splitk, int B, const float* bf1, const float* wf2,
                           const float* bf2, const int32_t* ylab, __bf16* dh, __bf16* dht, int ldt,
                           float* slab, int64_t* c0, int64_t* c1, unsigned* c2, float* dh32,
                           const uint32_t* epoch, uint64_t seed, uint32_t T, float scale,
                           const int32_t* train_labels, int ntrain, const int32_t* qt,
                           uint64_t mixup_seed, hipStream_t st, LrSched ls, float eps) {
  const int nblk = cnn_head_blocks(ldt / HEAD_ROWS);
  cnn_head_mixup_kernel<<<nblk, 256, 0, st>>>(
      part, splitk, B, bf1, wf2, bf2, ylab, dh, dht, ldt, slab, c0, c1, c2, dh32, epoch,
      (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), T, scale, ls, eps, train_labels,
      (uint32_t)ntrain, qt, (uint32_t)(mixup_seed & 0xffffffffu), (uint32_t)(mixup_seed >> 32));
}

void launch_mixup_pairs_rows(const int32_t* ylab, int B, const uint32_t* epoch,
                             const int32_t* train_labels, int ntrain, const int32_t* qt,
                             uint64_t mixup_seed, int32_t* out, hipStream_t st) {
  if (B <= 0) return;
  mixup_pairs_rows_kernel<<<(B + 255) / 256, 256, 0, st>>>(
      ylab, B, epoch, train_labels, (uint32_t)ntrain, qt, (uint32_t)(mixup_seed & 0xffffffffu),
      (uint32_t)(mixup_seed >> 32), out);
}
