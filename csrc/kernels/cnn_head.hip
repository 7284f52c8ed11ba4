// North-star CNN forward on gfx950, third kernel.
//
//   cnn_head: fc1 split-K reduction + bias + ReLU, fc2, log-softmax/NLL, argmax,
//             and (training) the whole head backward: dlogits, fc2 weight/bias
//             partials, dh = dlogits.W2 * relu'(h) (bf16, + transposed copy for the
//             fc1 weight-gradient GEMM), fc1 bias partials; advances step counters.
//   cnn_head_smooth: cnn_head<train> with label-smoothed targets (--label-smoothing E):
//             t_c = (1 - E) [c = y] + E / 10 in dlogits and the loss, nothing else differs
//             (docs/kernels.md "Label-smoothing head").
// Both are instances of the one head body (cnn_head_body.h), as are the dropout and mixup heads
// (cnn_head_drop.hip, cnn_head_mix.hip).
// Compiled with the iterative-ilp machine scheduler (build.py FILE_FLAGS).
#include "cnn_head_body.h"

namespace {

using namespace cnn;

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

// the training head with smoothed targets
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
