// Prediction heads: the inference forms of the evaluation heads (cnn_head<eval>, an instance of
// the same cnn_head_body.h; lin_eval in linear.hip).  Where those fold a row's logits into three
// fp64 sums,
// these write what the model said about every row:
//   logp      fp32  [B][10]   log-softmax of the logits
//   pred      int32 [B]       first maximum (torch.argmax; row_xent's `correct` rule)
//   confusion int64 [10][10]  confusion[y][pred] += 1 (labels given; integer atomics, so the
//                             counts do not depend on the order rows arrive in)
//   metrics   fp64  [3]       optionally the evaluation head's (loss sum, correct, count)
// The CNN kernel is the evaluation head's body itself, and the Linear one computes its logits
// with lin_eval's operations in their order (the same DPP wave sum, the same expf / logf calls),
// so argmax(logp) is the prediction the printed accuracy counted and -logp[y] is the row loss
// the printed loss summed, bit for bit.
#include "cnn_head_body.h"
#include "lin_common.h"

namespace {

constexpr int NC = CNN_NCLS;
static_assert(CNN_NCLS == LIN_N, "both models classify 10 digits");

// ---- CNN: the evaluation head (cnn_head_body.h head_body, PREDICT) with the per-row outputs ----
// Lane c < 10 stores logp[row][c] (one 40-B segment per wave), lane 0 stores pred and counts.
__global__ __launch_bounds__(256) void cnn_predict_head_kernel(
    const float* __restrict__ part, int S, int B, const float* __restrict__ bf1,
    const float* __restrict__ wf2, const float* __restrict__ bf2, const int32_t* __restrict__ ylab,
    float* __restrict__ logp, int32_t* __restrict__ pred, int64_t* __restrict__ confusion,
    double* __restrict__ metrics) {
  cnn::head_body<false, false, false, false, true>(
      blockIdx.x, gridDim.x, part, S, B, bf1, wf2, bf2, ylab, nullptr, nullptr, 0, nullptr, metrics,
      nullptr, nullptr, nullptr, nullptr, LrSched(), 0.f, cnn::HeadDraws(),
      cnn::HeadRows{logp, pred, confusion});
}

// ---- Linear: lin_eval's staging and wave_logits, 16 rows per workgroup, 4 per wave ----
__global__ __launch_bounds__(256) void lin_predict_kernel(
    const uint8_t* __restrict__ images, const int32_t* __restrict__ labels, int n_total,
    const float* __restrict__ W, const float* __restrict__ bias, float* __restrict__ logp,
    int32_t* __restrict__ pred, int64_t* __restrict__ confusion, double* __restrict__ metrics) {
  using namespace lin;
  constexpr int EROWS = LIN_EVAL_ROWS;               // 16: 4 rows per wave
  __shared__ __attribute__((aligned(16))) float xs[EROWS][K];
  __shared__ float lut[256];
  __shared__ float red[EROWS][2];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int row0 = blockIdx.x * EROWS;
  const int nrows = min(EROWS, n_total - row0);
  constexpr int NPIECE = EROWS * Q16;                // 784 pieces, 4 per thread at most
  uint4 px[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = tid + 256 * u, r = i / Q16;
    px[u] = make_uint4(0u, 0u, 0u, 0u);
    if (i < NPIECE && r < nrows)
      px[u] = reinterpret_cast<const uint4*>(images + (int64_t)(row0 + r) * K)[i - r * Q16];
  }
  float4 w[N][KJ];
  load_w_regs(W, w);
  lut[tid] = pdm_normalize((uint32_t)tid);
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = tid + 256 * u, r = i / Q16;
    if (i < NPIECE) put_pixels(xs[r], i - r * Q16, px[u], lut);
  }
  __syncthreads();
  const int rows[4] = {wave, wave + 4, wave + 8, wave + 12};
  float lg[4][N];
  wave_logits<4>(xs, rows, w, bias, lg);
  if (lane < 4) {
    const int r = rows[lane];
    float l[N], lp[N];
#pragma unroll
    for (int n = 0; n < N; ++n)
      l[n] = lane == 0 ? lg[0][n] : lane == 1 ? lg[1][n] : lane == 2 ? lg[2][n] : lg[3][n];
    float loss = 0.f;
    int correct = 0;
    if (r < nrows) {
      const int y = labels != nullptr ? labels[row0 + r] : 0;
      const int am = row_logp<N>(l, y, lp, loss);
      float* out = logp + (int64_t)(row0 + r) * N;
#pragma unroll
      for (int n = 0; n < N; ++n) out[n] = lp[n];
      pred[row0 + r] = am;
      if (confusion != nullptr) count_confusion<N>(confusion, y, am);
      correct = (am == y);
    }
    red[r][0] = loss;
    red[r][1] = (float)correct;
  }
  if (metrics == nullptr) return;      // (kernel-uniform)
  __syncthreads();
  if (tid == 0) {
    double l = 0.0, c = 0.0;
    for (int r = 0; r < EROWS; ++r) { l += red[r][0]; c += red[r][1]; }
    atomicAdd(&metrics[0], l);
    atomicAdd(&metrics[1], c);
    atomicAdd(&metrics[2], (double)nrows);
  }
}

}  // namespace

void launch_cnn_predict_head(const float* part, int splitk, int B, const float* bf1,
                             const float* wf2, const float* bf2, const int32_t* ylab, float* logp,
                             int32_t* pred, int64_t* confusion, double* metrics, hipStream_t st) {
  const int nblk = cnn_head_blocks((B + CNN_HEAD_ROWS - 1) / CNN_HEAD_ROWS);
  cnn_predict_head_kernel<<<nblk, 256, 0, st>>>(part, splitk, B, bf1, wf2, bf2, ylab, logp, pred,
                                                confusion, metrics);
}

void launch_lin_predict(const uint8_t* images, const int32_t* labels, int n_total, const float* W,
                        const float* b, float* logp, int32_t* pred, int64_t* confusion,
                        double* metrics, hipStream_t st) {
  const int nblk = (n_total + LIN_EVAL_ROWS - 1) / LIN_EVAL_ROWS;
  lin_predict_kernel<<<nblk, 256, 0, st>>>(images, labels, n_total, W, b, logp, pred, confusion,
                                           metrics);
}
