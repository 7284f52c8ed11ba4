// Test-time augmentation (--tta V): the reduction that combines the V per-view log-softmax rows
// of every image into the log of the mean probability (docs/kernels.md "Test-time
// augmentation").  The views themselves come from the augmenting gathers (augment.hip) and the
// per-view rows from the prediction heads (predict.hip), both unchanged; this is the only new
// arithmetic.  Per row and class c, in fp32, with l[v][c] the views' rows:
//   m      = max_v l[v][c]
//   s      = sum over v = 0..V-1, ascending, of expf(l[v][c] - m)
//   out[c] = (m + logf(s)) - lnV                  lnV = float32(log(float64(V))), from the host
// and then what the prediction heads write about a row:
//   logp      fp32  [n][10]   out
//   pred      int32 [n]       first maximum of out as stored (torch.argmax)
//   confusion int64 [10][10]  confusion[y][pred] += 1 (labels given; integer atomics; a label
//                             outside 0..9 counts nowhere)
//   metrics   fp64  [3]       (sum of -out[y], sum of [pred == y], rows): a row whose label is
//                             outside 0..9 adds to the row count only
// At V = 1 out is the input, bit for bit: expf(0) = 1, logf(1) = 0, lnV = 0.
//
// Layout: one thread per row, one wave per workgroup.  A row is 40 B, read as five 8-B words
// per view; the V rows of one image are n * 40 B apart.  The views are read twice (maxima,
// then sums): the second pass hits L2, and an online rescaling would not be the specified
// arithmetic.  The ten maxima and the ten sums live in registers, indexed by unrolled
// constants only (no scratch); no LDS: the metric sums cross the wave by shuffles and leave
// as one fp64 atomicAdd triple per workgroup, as the prediction heads' do.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int NC = 10;               // classes (CNN_NCLS, LIN_N)
constexpr int TTA_ROWS = 64;         // rows per workgroup: one wave

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(TTA_ROWS) void tta_reduce_kernel(
    const float* __restrict__ views, int V, int n, float lnV, const int32_t* __restrict__ labels,
    float* __restrict__ logp, int32_t* __restrict__ pred, int64_t* __restrict__ confusion,
    double* __restrict__ metrics) {
  const int row = blockIdx.x * TTA_ROWS + threadIdx.x;
  const bool valid = row < n;
  double loss = 0.0, correct = 0.0;
  if (valid) {
    const int64_t vstride = (int64_t)n * NC;          // floats between two views of a row
    const float* __restrict__ src = views + (int64_t)row * NC;
    float m[NC], s[NC];
#pragma unroll
    for (int c = 0; c < NC; c += 2) {
      const float2 u = *reinterpret_cast<const float2*>(src + c);
      m[c] = u.x;
      m[c + 1] = u.y;
    }
    for (int v = 1; v < V; ++v) {
      const float* __restrict__ p = src + v * vstride;
#pragma unroll
      for (int c = 0; c < NC; c += 2) {
        const float2 u = *reinterpret_cast<const float2*>(p + c);
        m[c] = fmaxf(m[c], u.x);
        m[c + 1] = fmaxf(m[c + 1], u.y);
      }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) s[c] = 0.f;
    for (int v = 0; v < V; ++v) {
      const float* __restrict__ p = src + v * vstride;
#pragma unroll
      for (int c = 0; c < NC; c += 2) {
        const float2 u = *reinterpret_cast<const float2*>(p + c);
        s[c] += expf(u.x - m[c]);
        s[c + 1] += expf(u.y - m[c + 1]);
      }
    }
    float out[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) out[c] = (m[c] + logf(s[c])) - lnV;
    float best = out[0];
    int am = 0;
#pragma unroll
    for (int c = 1; c < NC; ++c)
      if (out[c] > best) { best = out[c]; am = c; }
    float* __restrict__ dst = logp + (int64_t)row * NC;
#pragma unroll
    for (int c = 0; c < NC; c += 2)
      *reinterpret_cast<float2*>(dst + c) = make_float2(out[c], out[c + 1]);
    pred[row] = am;
    if (labels != nullptr) {
      const int y = labels[row];
      if ((unsigned)y < (unsigned)NC) {
        if (confusion != nullptr)
          atomicAdd(reinterpret_cast<unsigned long long*>(confusion) + y * NC + am, 1ull);
        // out[y] by selects, not a register-array index: that would go to scratch
        float oy = out[0];
#pragma unroll
        for (int c = 1; c < NC; ++c) oy = (c == y) ? out[c] : oy;
        loss = (double)(-oy);
        correct = (am == y) ? 1.0 : 0.0;
      }
    }
  }
  if (metrics == nullptr) return;                      // (kernel-uniform)
  loss = wave_sum_f64(loss);
  correct = wave_sum_f64(correct);
  if (threadIdx.x == 0) {
    atomicAdd(&metrics[0], loss);
    atomicAdd(&metrics[1], correct);
    atomicAdd(&metrics[2], (double)min(TTA_ROWS, n - blockIdx.x * TTA_ROWS));
  }
}

}  // namespace

void launch_tta_reduce(const float* logp_views, int V, int n, float lnV, const int32_t* labels,
                       float* logp, int32_t* pred, int64_t* confusion, double* metrics,
                       hipStream_t st) {
  if (n <= 0) return;
  const int nblk = (n + TTA_ROWS - 1) / TTA_ROWS;
  tta_reduce_kernel<<<nblk, TTA_ROWS, 0, st>>>(logp_views, V, n, lnV, labels, logp, pred,
                                               confusion, metrics);
}
