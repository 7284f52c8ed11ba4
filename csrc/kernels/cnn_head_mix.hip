// Mixup in the CNN's training head: the two-class variant of the training head
// (cnn_head_body.h).
//
//   cnn_head_mixup: cnn_head_dropout (cnn_head_drop.hip) with the row's target mixed with its
//             partner's:
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
#include "cnn_head_body.h"

namespace {

using namespace cnn;

__global__ __launch_bounds__(256) void cnn_head_mixup_kernel(
    const float* __restrict__ part, int S, int B, const float* __restrict__ bf1,
    const float* __restrict__ wf2, const float* __restrict__ bf2, const int32_t* __restrict__ ylab,
    bf16* __restrict__ dh, bf16* __restrict__ dht, int ldt, float* __restrict__ slab, int64_t* c0,
    int64_t* c1, unsigned* c2, float* __restrict__ dh32, const uint32_t* __restrict__ epoch_word,
    uint32_t k0, uint32_t k1, uint32_t T, float scale, const LrSched ls, const float eps,
    const int32_t* __restrict__ train_labels, uint32_t ntrain, const int32_t* __restrict__ qt,
    uint32_t mk0, uint32_t mk1) {
  head_body<true, true, true, true>(
      blockIdx.x, gridDim.x, part, S, B, bf1, wf2, bf2, ylab, dh, dht, ldt, slab, nullptr, c0, c1,
      c2, dh32, ls, eps, HeadDraws{epoch_word, k0, k1, T, scale, train_labels, ntrain, qt, mk0, mk1});
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
