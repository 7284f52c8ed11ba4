// Exponential moving average of the weights (--ema-decay D) -- the last launch of a step.
//
// One launch sweeps the flat fp32 parameter arena once:  e <- e + w (p - e),  w = float(1 - d_k).
//   * Three separately rounded fp32 operations, never contracted into an fma, so that NumPy
//     float32 (and the CPU path's torch ops) reproduce every bit.  HIP's __fsub_rn / __fmul_rn /
//     __fadd_rn are the plain operators on this target, and hipcc contracts across them by
//     default, so the arithmetic sits under `#pragma clang fp contract(off)` instead of
//     relying on the intrinsics or on an -ffp-contract flag of the build.
//   * Without warmup d_k = D and the host passes w.  With warmup d_k = min(D, (1 + k) / (10 + k))
//     for the 1-based update index k, evaluated here in fp64 (division correctly rounded) and
//     rounded to fp32 once -- optim/ema.py ema_weight is the same expression on the host.
//   * k = the optimizer-step word + a host offset.  The step's head launch has advanced the
//     word (the optimizer read it as *a.step); every workgroup here only reads it and the
//     kernel writes no counter, so no workgroup races another and a captured graph replays
//     across epochs with no host involvement.
// Geometry: optim.hip's plain segment -- 256 threads, two float4 per thread (2048 elements per
// workgroup), a scalar tail for n % 4, no address formed past n.
// e is read and written by this kernel only, p is read again by the next step's kernels:
// NT = true streams e with nontemporal loads and stores (p always with plain loads).
#include "common.h"
#include "kernels.h"

namespace {

constexpr int EMA_CHUNK = 2048;  // elements per workgroup (256 thr x 8)

__device__ __forceinline__ float ema_one(float e, float p, float w) {
#pragma clang fp contract(off)
  const float d = p - e;     // __fsub_rn
  const float s = w * d;     // __fmul_rn
  return e + s;              // __fadd_rn
}

__device__ __forceinline__ float ema_weight(const EmaArgs& a) {
#pragma clang fp contract(off)
  if (!a.warmup) return a.w;
  int64_t k = *a.step + a.offset;
  k = k < 1 ? 1 : k;         // backstop: the host never runs an update before the first step
  const double r = __ddiv_rn(1.0 + (double)k, 10.0 + (double)k);
  const double d = r < a.decay ? r : a.decay;
  return (float)(1.0 - d);
}

template <bool NT>
__device__ __forceinline__ float4 ema_load4(const float* q) {
  if constexpr (NT) {
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(q));
    return make_float4(v[0], v[1], v[2], v[3]);
  } else {
    return *reinterpret_cast<const float4*>(q);
  }
}

template <bool NT>
__device__ __forceinline__ void ema_store4(float* q, float4 v) {
  if constexpr (NT) {
    const f32x4 t = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(t, reinterpret_cast<f32x4*>(q));
  } else {
    *reinterpret_cast<float4*>(q) = v;
  }
}

template <bool NT>
__global__ __launch_bounds__(256) void ema_kernel(EmaArgs a) {
  const float* __restrict__ P = a.p;
  float* __restrict__ E = a.e;
  const int64_t n = a.n;
  // this workgroup lies inside the arena's block range
  PDM_CHECK((int64_t)blockIdx.x * EMA_CHUNK < n, "ema block range", blockIdx.x, n);
  const float w = ema_weight(a);
  const int64_t e0 = (int64_t)blockIdx.x * EMA_CHUNK + threadIdx.x * 8;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int64_t i = e0 + q * 4;
    if (i + 4 <= n) {
      const float4 p = *reinterpret_cast<const float4*>(P + i);
      float4 e = ema_load4<NT>(E + i);
      e.x = ema_one(e.x, p.x, w);
      e.y = ema_one(e.y, p.y, w);
      e.z = ema_one(e.z, p.z, w);
      e.w = ema_one(e.w, p.w, w);
      ema_store4<NT>(E + i, e);
    } else {
      for (int64_t j = i; j < n && j < i + 4; ++j) E[j] = ema_one(E[j], P[j], w);
    }
  }
}

}  // namespace

void launch_ema_update(const EmaArgs& a, bool nt, hipStream_t st) {
  if (a.n <= 0) return;
  const int blocks = (int)((a.n + EMA_CHUNK - 1) / EMA_CHUNK);
  if (nt)
    ema_kernel<true><<<blocks, 256, 0, st>>>(a);
  else
    ema_kernel<false><<<blocks, 256, 0, st>>>(a);
}
