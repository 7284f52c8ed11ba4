// Dropout on the CNN's 128 hidden units: the masking variant of the training head
// (cnn_head_body.h).
//
//   cnn_head_dropout: the training head with the dropout mask between the ReLU and fc2 (and on
//             dh).  Train-only: evaluation and prediction keep their kernels.
//   dropout_mask_rows: the keep mask alone, uint8 [B][128], from the same device function
//             (cnn_head_body.h dropout_draw).
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
#include "cnn_head_body.h"

namespace {

using namespace cnn;

// head_body<train, smooth> with the mask between the ReLU and fc2; at T = 0 (scale 1) every
// output is bit-identical to cnn_head's (tests/test_gpu_dropout.py).  eps: label smoothing of
// the targets as in cnn_head_smooth; eps = 0 gives the unsmoothed bits
// (tests/test_gpu_label_smoothing.py).
__global__ __launch_bounds__(256) void cnn_head_dropout_kernel(
    const float* __restrict__ part, int S, int B, const float* __restrict__ bf1,
    const float* __restrict__ wf2, const float* __restrict__ bf2, const int32_t* __restrict__ ylab,
    bf16* __restrict__ dh, bf16* __restrict__ dht, int ldt, float* __restrict__ slab, int64_t* c0,
    int64_t* c1, unsigned* c2, float* __restrict__ dh32, const uint32_t* __restrict__ epoch_word,
    uint32_t k0, uint32_t k1, uint32_t T, float scale, const LrSched ls, const float eps) {
  head_body<true, true, true>(blockIdx.x, gridDim.x, part, S, B, bf1, wf2, bf2, ylab, dh, dht, ldt,
                              slab, nullptr, c0, c1, c2, dh32, ls, eps,
                              HeadDraws{epoch_word, k0, k1, T, scale, nullptr, 0u, nullptr, 0u, 0u});
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
