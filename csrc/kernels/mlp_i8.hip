// int8 post-training quantised evaluation of the MLPs' first layer (--quantize int8; docs/kernels.md
// "int8 evaluation") on gfx950's integer matrix cores, v_mfma_i32_16x16x64_i8.
//
// fc1's image operand is a raw byte already: u8 ^ 0x80 is u8 - 128 as an int8, so the activation
// is quantised without error, and only the weight is: per hidden unit n, s1[n] = max_k |W1[n][k]|
// / 127 and q1[n][k] = clamp(rint(W1[n][k] / s1[n]), -127, 127).  With W = s1 q1 the existing
// fold  pre = alpha sum_k W u8 - beta sum_k W + b1  becomes
//
//   pre[b][n] = c1[n] I[b][n] + d1[n],    I[b][n] = sum_k q1[n][k] (u8[b][k] - 128)    (int32)
//   c1[n] = alpha s1[n],   d1[n] = b1[n] + (s1[n] (float)r1[n]) gamma,   r1[n] = sum_k q1[n][k]
//
// with gamma = 128 alpha - beta.  |I| <= 127 * 128 * 784 < 2^24: exact in int32 and as a float.
//
//   mlp_quant_w1  one workgroup per hidden unit, once per weight set: 196 lanes hold four
//                 consecutive weights each (one 16-B load); the row's absmax and the integer row
//                 sum are reduced on the DPP network per wave and across the four waves through
//                 four LDS words; the int8 row goes out as packed dwords, padded with zeros to
//                 832 = 13 x 64 columns, so the forward's last k-step needs no weight mask.
//   mlp_fwd_i8    (m-tile of 16 rows, split s of S) workgroups, 4 waves x 32 hidden units, as
//                 mlp_fwd.  The 784 pixels are 13 k-steps of 64, S in {1, 13}.  Lane (g, i16)
//                 loads 16 B of row i16 at k0 + 16 g (a 16-lane group: one 64-B line piece per
//                 row), flips the four sign bits of each dword with one XOR, and 16 B of each of
//                 its two weight rows: two MFMAs per k-step share the image fragment.  Both
//                 operands take their bytes from the same (g, j) -> k0 + 16 g + j map, so the
//                 sum does not depend on how the instruction orders k inside a lane.  All loads of
//                 a workgroup are issued before its first MFMA.  The last k-step covers k = 768 ..
//                 831: the weights there are zero and integers have no NaN, so whatever bytes the
//                 image lanes g >= 1 read (the next row's) multiply to exactly 0; their address is
//                 clamped to the last 16 B of the image buffer.  Straight-from-memory fragments:
//                 no LDS.  No atomics, a fixed order: bit-reproducible.
//
// Every fp32 operation here is rounded on its own, so NumPy float32 reproduces the bits
// (runtime/cpu_step.py quantize_fc1).  hipcc contracts a * b + c into an fma by default, also
// across HIP's __fmul_rn / __fadd_rn (plain operators on this target), so the one place with a
// product feeding a sum, d1, sits under `#pragma clang fp contract(off)`, as ema.hip's update.
#include "cnn_f32_common.h"

namespace {

using namespace cnn;

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int MQ_K = MLP_IN;                        // 784 pixels
constexpr int MQ_STEPS = MLP_I8_KPAD / 64;          // 13 k-steps
constexpr float MQ_ALPHA = (float)(1.0 / (255.0 * 0.3081));
constexpr float MQ_GAMMA = (float)(128.0 / (255.0 * 0.3081) - 0.1307 / 0.3081);
static_assert(MLP_I8_KPAD % 64 == 0 && MLP_I8_KPAD >= MQ_K && MQ_STEPS == 13 && MQ_K % 16 == 0 &&
              HID == 128, "int8 fc1 geometry");

__device__ __forceinline__ int wave_sum_dpp_i32(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);    // quad_perm [1,0,3,2]
  v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);    // quad_perm [2,3,0,1]
  v += __builtin_amdgcn_update_dpp(0, v, 0x124, 0xf, 0xf, false);   // row_ror:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, false);   // row_ror:8
  return (__builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16)) +
         (__builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48));
}

// the maximum of non-negative floats: their bit patterns order as integers
__device__ __forceinline__ float wave_max_dpp_nonneg(float f) {
  int v = __float_as_int(f);
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x124, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, false));
  return __int_as_float(max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
                            max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48))));
}

// d1 = b1 + (s1 r1) gamma in three roundings (the pragma: see the header)
__device__ __forceinline__ float fold_bias(float b, float s, int r) {
#pragma clang fp contract(off)
  const float sr = s * (float)r;
  const float t = sr * MQ_GAMMA;
  return b + t;
}

// ------------------------------------------------------------------ mlp_quant_w1
__global__ __launch_bounds__(256) void mlp_quant_w1_kernel(
    const float* __restrict__ w1, const float* __restrict__ b1, int8_t* __restrict__ q1,
    float* __restrict__ s1, int32_t* __restrict__ r1, float* __restrict__ c1,
    float* __restrict__ d1) {
  __shared__ float smax[4];
  __shared__ int ssum[4];
  const int n = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
  // lane t < 196: weights 4 t .. 4 t + 3 of the row; 196 .. 207: a dword of the zero padding
  const bool has = tid < MQ_K / 4;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  const f32x4 w = has ? *reinterpret_cast<const f32x4*>(w1 + (int64_t)n * MQ_K + 4 * tid) : z;
  const float mloc = fmaxf(fmaxf(fabsf(w[0]), fabsf(w[1])), fmaxf(fabsf(w[2]), fabsf(w[3])));
  const float mw = wave_max_dpp_nonneg(mloc);
  if ((tid & 63) == 0) smax[wave] = mw;
  __syncthreads();
  const float m = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
  // (HIP's default fp32 division is correctly rounded: common.h pdm_normalize)
  const float s = m == 0.f ? 1.f : m / 127.f;
  int sum = 0;
  uint32_t word = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = (int)fminf(fmaxf(rintf(w[j] / s), -127.f), 127.f);
    sum += q;
    word |= (uint32_t)(q & 0xff) << (8 * j);
  }
  if (tid < MLP_I8_KPAD / 4)
    *reinterpret_cast<uint32_t*>(q1 + (int64_t)n * MLP_I8_KPAD + 4 * tid) = word;
  const int sw = wave_sum_dpp_i32(sum);
  if ((tid & 63) == 0) ssum[wave] = sw;
  __syncthreads();
  if (tid == 0) {
    const int r = (ssum[0] + ssum[1]) + (ssum[2] + ssum[3]);
    s1[n] = s;
    r1[n] = r;
    c1[n] = MQ_ALPHA * s;
    d1[n] = fold_bias(b1[n], s, r);
  }
}

// ------------------------------------------------------------------ mlp_fwd_i8
// KPER = 13 / S k-steps per workgroup, every load issued before the first MFMA
template <int KPER>
__global__ __launch_bounds__(256) void mlp_fwd_i8_kernel(
    const uint8_t* __restrict__ images, const int32_t* __restrict__ labels, int64_t nrow, int B,
    const int8_t* __restrict__ q1, const float* __restrict__ c1, float* __restrict__ part,
    int32_t* __restrict__ ylab) {
  const int mtiles = (B + 15) / 16;
  const int mtile = blockIdx.x % mtiles, sidx = blockIdx.x / mtiles;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i16 = lane & 15;
  // rows >= B read a clamped valid row and store nothing
  const int b = min(mtile * 16 + i16, B - 1);
  if (sidx == 0 && wave == 0 && g == 0 && mtile * 16 + i16 < B) ylab[b] = labels[b];
  const int64_t xo = (int64_t)b * MQ_K + 16 * g;
  const int64_t xlast = nrow * MQ_K - 16;           // the last 16 B of the buffer (16-B aligned)
  const int8_t* wrow = q1 + (int64_t)(wave * 32 + i16) * MLP_I8_KPAD + 16 * g;
  i32x4 xv[KPER], wv[KPER][2];
#pragma unroll
  for (int s = 0; s < KPER; ++s) {
    const int k = (sidx * KPER + s) * 64;
    // k + 16 g >= 784 (the last step's lanes g >= 1): any in-bounds bytes, the weights are zero
    xv[s] = *reinterpret_cast<const i32x4*>(images + min(xo + k, xlast));
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
      wv[s][nt] = *reinterpret_cast<const i32x4*>(wrow + nt * 16 * MLP_I8_KPAD + k);
  }
  i32x4 acc[2] = {i32x4{0, 0, 0, 0}, i32x4{0, 0, 0, 0}};
#pragma unroll
  for (int s = 0; s < KPER; ++s) {
    const i32x4 a = xv[s] ^ (int)0x80808080u;        // u8 - 128 as int8, byte by byte
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
      acc[nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, wv[s][nt], acc[nt], 0, 0, 0);
  }
  float* out = part + (int64_t)sidx * B * HID;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int n = wave * 32 + nt * 16 + i16;        // the D fragment's column
    const float c = c1[n];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rowi = mtile * 16 + 4 * g + r;
      if (rowi < B) out[(int64_t)rowi * HID + n] = c * (float)acc[nt][r];
    }
  }
}

}  // namespace

void launch_mlp_quant_w1(const float* w1, const float* b1, int8_t* q1, float* s1, int32_t* r1,
                         float* c1, float* d1, hipStream_t st) {
  mlp_quant_w1_kernel<<<HID, 256, 0, st>>>(w1, b1, q1, s1, r1, c1, d1);
}

void launch_mlp_fwd_i8(const uint8_t* images, const int32_t* labels, int64_t nrow, int B,
                       const int8_t* q1, const float* c1, float* part, int32_t* ylab, int splitk,
                       hipStream_t st) {
  const int grid = (B + 15) / 16 * splitk;
  if (splitk == MQ_STEPS)
    mlp_fwd_i8_kernel<1><<<grid, 256, 0, st>>>(images, labels, nrow, B, q1, c1, part, ylab);
  else
    mlp_fwd_i8_kernel<MQ_STEPS><<<grid, 256, 0, st>>>(images, labels, nrow, B, q1, c1, part, ylab);
}
