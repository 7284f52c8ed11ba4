// Device helpers shared by the Linear-model kernels (linear.hip, predict.hip): the register
// image of W, the uint8 -> normalised-float row staging, a wave's logits and the row
// log-softmax CE.
#pragma once
#include "../common.h"
#include "../kernels.h"

namespace lin {

constexpr int K = LIN_K;        // 784
constexpr int N = LIN_N;        // 10
constexpr int K4 = K / 4;       // 196 float4 columns
constexpr int KJ = 4;           // 256-feature chunks per row (the last holds 16 features)
constexpr int Q16 = K / 16;     // 49 16-byte pieces per image row

// W[n][4 lane + 256 j .. +3] for every n, j (clamped past the row end: x is zero there)
__device__ __forceinline__ void load_w_regs(const float* __restrict__ W, float4 (&w)[N][KJ]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < KJ; ++j) {
    const int k4 = min(lane + 64 * j, K4 - 1);
#pragma unroll
    for (int n = 0; n < N; ++n) w[n][j] = reinterpret_cast<const float4*>(W + n * K)[k4];
  }
}

// 16 uint8 pixels -> 16 normalised floats (lut = pdm_normalize table) at xrow[16 q ..]
__device__ __forceinline__ void put_pixels(float* xrow, int q, uint4 v, const float* lut) {
  const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float4 f;
    f.x = lut[wd[c] & 0xff];
    f.y = lut[(wd[c] >> 8) & 0xff];
    f.z = lut[(wd[c] >> 16) & 0xff];
    f.w = lut[wd[c] >> 24];
    *reinterpret_cast<float4*>(xrow + 16 * q + 4 * c) = f;
  }
}

// One wave: the 10 logits of R rows (xs rows rows[0..R)), W in registers; every lane
// holds the results after the reduce.
template <int R>
__device__ __forceinline__ void wave_logits(const float (*xs)[K], const int (&rows)[R],
                                            const float4 (&w)[N][KJ],
                                            const float* __restrict__ bias, float (&lg)[R][N]) {
  const int lane = threadIdx.x & 63;
  float acc[R][N];
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int n = 0; n < N; ++n) acc[i][n] = 0.f;
#pragma unroll
  for (int j = 0; j < KJ; ++j) {
    const int k4 = lane + 64 * j;
    const bool on = k4 < K4;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (on) x = reinterpret_cast<const float4*>(xs[rows[i]])[k4];
#pragma unroll
      for (int n = 0; n < N; ++n) {
        float a = acc[i][n];
        a = fmaf(x.x, w[n][j].x, a);
        a = fmaf(x.y, w[n][j].y, a);
        a = fmaf(x.z, w[n][j].z, a);
        a = fmaf(x.w, w[n][j].w, a);
        acc[i][n] = a;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int n = 0; n < N; ++n) lg[i][n] = wave_sum_dpp(acc[i][n]) + bias[n];
}

// log-softmax CE on one row's logits; returns loss, writes softmax probs, sets
// `correct` with torch.argmax tie-breaking (first maximal index).
__device__ __forceinline__ float row_xent(const float (&lg)[N], int y, float (&p)[N], int& correct) {
  float m = lg[0];
  int am = 0;
#pragma unroll
  for (int n = 1; n < N; ++n) {
    if (lg[n] > m) { m = lg[n]; am = n; }
  }
  float s = 0.f;
#pragma unroll
  for (int n = 0; n < N; ++n) { p[n] = expf(lg[n] - m); s += p[n]; }
  const float lse = m + logf(s);
  const float inv = 1.f / s;
#pragma unroll
  for (int n = 0; n < N; ++n) p[n] *= inv;
  correct = (am == y);
  float ly = lg[0];
#pragma unroll
  for (int n = 1; n < N; ++n) ly = (n == y) ? lg[n] : ly;
  return lse - ly;
}

}  // namespace lin
