// Prediction heads: the inference twins of the evaluation heads (cnn_head<eval> in
// cnn_head.hip, lin_eval in linear.hip).  Where those fold a row's logits into three fp64 sums,
// these write what the model said about every row:
//   logp      fp32  [B][10]   log-softmax of the logits
//   pred      int32 [B]       first maximum (torch.argmax; row_xent's `correct` rule)
//   confusion int64 [10][10]  confusion[y][pred] += 1 (labels given; integer atomics, so the
//                             counts do not depend on the order rows arrive in)
//   metrics   fp64  [3]       optionally the evaluation head's (loss sum, correct, count)
// The logits are computed with the evaluation heads' operations in their order (split-K
// partials summed in split order after the bias, the same DPP wave sum, the same expf / logf
// calls), so argmax(logp) is the prediction the printed accuracy counted and -logp[y] is the
// row loss the printed loss summed, bit for bit.
#include "cnn_common.h"
#include "lin_common.h"

namespace {

constexpr int NC = CNN_NCLS;
static_assert(CNN_NCLS == LIN_N, "both models classify 10 digits");

// Log-softmax of one row's logits (every lane of the wave holds the same lg): lp = lg - lse
// with row_xent's max / expf / logf sequence; returns the first maximal index and the row
// loss lse - lg[y] as row_xent forms it.
__device__ __forceinline__ int row_logp(const float (&lg)[NC], int y, float (&lp)[NC],
                                        float& loss) {
  float m = lg[0];
  int am = 0;
#pragma unroll
  for (int n = 1; n < NC; ++n)
    if (lg[n] > m) { m = lg[n]; am = n; }
  float s = 0.f;
#pragma unroll
  for (int n = 0; n < NC; ++n) s += expf(lg[n] - m);
  const float lse = m + logf(s);
#pragma unroll
  for (int n = 0; n < NC; ++n) lp[n] = lg[n] - lse;
  float ly = lg[0];
#pragma unroll
  for (int n = 1; n < NC; ++n) ly = (n == y) ? lg[n] : ly;
  loss = lse - ly;
  return am;
}

// confusion[y][am] += 1; a label outside [0, 10) counts nowhere (and writes nowhere)
__device__ __forceinline__ void count_confusion(int64_t* __restrict__ confusion, int y, int am) {
  if ((unsigned)y < (unsigned)NC)
    atomicAdd(reinterpret_cast<unsigned long long*>(confusion) + y * NC + am, 1ull);
}

// ---- CNN: fc1 split-K reduce + bias + ReLU, fc2, log-softmax, argmax ----
// head_body<false>'s layout: one wave per row (4 rows per workgroup), lane j owns hidden units
// 2j, 2j + 1, a grid-stride over the row groups on at most CNN_HEAD_MAX_BLOCKS workgroups.
// Lane c < 10 stores logp[row][c] (one 40-B segment per wave), lane 0 stores pred and counts.
__global__ __launch_bounds__(256) void cnn_predict_head_kernel(
    const float* __restrict__ part, int S, int B, const float* __restrict__ bf1,
    const float* __restrict__ wf2, const float* __restrict__ bf2, const int32_t* __restrict__ ylab,
    float* __restrict__ logp, int32_t* __restrict__ pred, int64_t* __restrict__ confusion,
    double* __restrict__ metrics) {
  using namespace cnn;
  static_assert(HEAD_ROWS == 4, "one wave per row, 4 waves");
  __shared__ float red[HEAD_ROWS][2];
  const int tid = threadIdx.x, r = tid >> 6, j = tid & 63;
  const int ngroups = (B + HEAD_ROWS - 1) / HEAD_ROWS;
  double el = 0.0, ec = 0.0;                  // eval metrics (thread 0)
  int en = 0;
  const float2 bias = reinterpret_cast<const float2*>(bf1)[j];
  float2 w2v[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) w2v[c] = reinterpret_cast<const float2*>(wf2 + c * HID)[j];
  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int row = grp * HEAD_ROWS + r;
    const bool valid = row < B;
    const int y = (valid && ylab != nullptr) ? ylab[row] : 0;
    float2 h = bias;
    const int rc = min(row, B - 1);
    if (S == 32) {
      // every partial load in flight at once (head_body's S == 32 path)
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
      // batches of 16 loads in flight (clamped addresses + selects), summed in split order
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

    float lg[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) lg[c] = wave_sum_dpp(fmaf(h.y, w2v[c].y, h.x * w2v[c].x)) + bf2[c];
    float lp[NC], loss;
    const int am = row_logp(lg, y, lp, loss);
    // lane c's own class (selects, not a register-array index: that would go to scratch)
    float mine = lp[0];
#pragma unroll
    for (int c = 1; c < NC; ++c) mine = (j == c) ? lp[c] : mine;
    if (valid && j < NC) logp[(int64_t)row * NC + j] = mine;
    if (valid && j == 0) {
      pred[row] = am;
      if (confusion != nullptr) count_confusion(confusion, y, am);
    }
    if (metrics != nullptr) {        // (kernel-uniform) the evaluation head's sums, its way
      if (j == 0) {
        red[r][0] = valid ? loss : 0.f;
        red[r][1] = valid ? (float)(am == y) : 0.f;
      }
      __syncthreads();
      if (tid == 0) {
        for (int i = 0; i < HEAD_ROWS; ++i) {
          el += red[i][0];
          ec += red[i][1];
          en += (grp * HEAD_ROWS + i < B);
        }
      }
      __syncthreads();   // red is rewritten by the next row group
    }
  }
  if (metrics != nullptr && tid == 0) {
    atomicAdd(&metrics[0], el);
    atomicAdd(&metrics[1], ec);
    atomicAdd(&metrics[2], (double)en);
  }
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
      const int am = row_logp(l, y, lp, loss);
      float* out = logp + (int64_t)(row0 + r) * N;
#pragma unroll
      for (int n = 0; n < N; ++n) out[n] = lp[n];
      pred[row0 + r] = am;
      if (confusion != nullptr) count_confusion(confusion, y, am);
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
