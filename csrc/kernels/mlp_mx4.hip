// MXFP4 post-training quantised evaluation of the MLPs' first layer (--quantize mxfp4;
// docs/kernels.md "MXFP4 evaluation") on gfx950's block-scaled matrix instruction,
// v_mfma_scale_f32_16x16x128_f8f6f4 with an fp8 (E4M3) A operand and an fp4 (E2M1) B operand.
//
// Weights, OCP MX v1.0: each row of fc1.weight [128][784] is cut into blocks of 32 consecutive k
// (24 full ones, one of 16 real weights; padded with zeros to 896 = 7 x 128 columns = 28 blocks).
// A block with m = max |w| > 0 has the scale byte e8 = clamp(floor(log2 m) - 2 + 127, 0, 254),
// X = 2^(e8 - 127), and its elements are v = w / X (exact) rounded to nearest on the E2M1 grid
// {0, .5, 1, 1.5, 2, 3, 4, 6}, ties to the code with mantissa bit 0, above 6 to 6; the code is
// sign << 3 | magnitude code with no negative zero.  m = 0: e8 = 127, codes 0.  Two codes per
// byte, even k in the low nibble: 448 B per row, scales uint8 [128][28].
//
// Pixels are exact: u8 = 16 hi + lo, and 16 hi and lo are E4M3 numbers, so the image goes in as
// two fp8 operands and each (n-tile, k-step) takes two MFMAs.  With Wq the dequantised weights,
//
//   pre[b][n] = alpha I[b][n] + d1[n],   I = sum_k Wq[n][k] u8[b][k],   d1 = b1 - beta R,
//   R[n] = sum_k Wq[n][k]: the block sums (exact in fp32) added in block order 0 .. 24.
//
//   mlp_quant_mx4  one workgroup per hidden unit, once per weight set: lane t < 196 holds weights
//                  4 t .. 4 t + 3 (one 16-B load), lanes 196 .. 223 the zero padding; a block is
//                  8 lanes, its maximum and its sum go over the DPP network (two quad_perms and
//                  row_half_mirror); the exponent comes from the maximum's exponent field, the
//                  grid rounding is seven comparisons.  Each lane stores its 4 codes (2 B), each
//                  block's first lane the scale byte and the block sum into LDS; thread 0 adds
//                  the 25 sums in order and writes d1.
//   mlp_fwd_mx4    (m-tile of 16 rows, split s of S) workgroups, 4 waves x 32 hidden units, as
//                  mlp_fwd_i8.  896 columns are 7 k-steps of 128, S in {1, 7}.  The instruction's
//                  operand maps, as measured on the device (docs/kernels.md): the fp4 B operand
//                  of lane (g, i16) is column i16's k0 + 32 g .. k0 + 32 g + 31 in nibble order,
//                  exactly one MX block, and the lane's scale byte (byte op_sel of its scale
//                  register) is that block's; the fp8 A operand's 32 bytes are row i16's k0 +
//                  16 g .. + 15 (registers 0 - 3) and k0 + 64 + 16 g .. + 15 (registers 4 - 7).
//                  So a lane loads those two 16-B pieces of image row i16 and, for each of its
//                  two weight rows, 16 B of codes and the block's scale byte.  The pixel bytes
//                  become E4M3 bytes of their high (16 n) and low (n) nibbles through a 16-entry
//                  table applied with v_perm_b32 (two 8-byte pools picked by the nibble's bit
//                  3).  The last k-step covers k = 768 .. 895: the codes there are zero and the
//                  table gives finite values only, so whatever bytes the image lanes read past
//                  column 783 multiply to exactly 0; every 16-B piece's address is clamped to
//                  the last 16 B of the image buffer.  No LDS, no atomics, a fixed order:
//                  bit-reproducible.  part = alpha acc, one rounding.
//
// d1's product feeds a difference, so it sits under `#pragma clang fp contract(off)` as
// mlp_i8.hip's fold_bias; NumPy float32 reproduces every bit (runtime/cpu_step.py
// quantize_fc1_mxfp4).
#include "cnn_f32_common.h"

namespace {

using namespace cnn;

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int MX_K = MLP_IN;                        // 784 pixels
constexpr int MX_STEPS = MLP_MX4_KPAD / 128;        // 7 k-steps
constexpr int MX_PITCH = MLP_MX4_KPAD / 2;          // 448 B of codes per row
constexpr int MX_BLOCKS = MLP_MX4_KPAD / 32;        // 28 scale bytes per row
constexpr int MX_REAL_BLOCKS = (MX_K + 31) / 32;    // 25 of them hold weights
constexpr float MX_ALPHA = (float)(1.0 / (255.0 * 0.3081));
constexpr float MX_BETA = (float)(0.1307 / 0.3081);
static_assert(MLP_MX4_KPAD % 128 == 0 && MLP_MX4_KPAD >= MX_K && MX_STEPS == 7 && MX_K % 16 == 0 &&
              MX_BLOCKS % 4 == 0 && HID == 128, "MXFP4 fc1 geometry");

// ------------------------------------------------------------------ mlp_quant_mx4
// the maximum of non-negative floats (as integers) / the sum over the 8 lanes of a block
__device__ __forceinline__ float block_max_dpp_nonneg(float f) {
  int v = __float_as_int(f);
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false));   // row_half_mirror
  return __int_as_float(v);
}

__device__ __forceinline__ float block_sum_dpp(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, false));
  return v;
}

// d1 = b1 - beta R in two roundings (the pragma: see the header)
__device__ __forceinline__ float fold_bias_mx4(float b, float r) {
#pragma clang fp contract(off)
  const float t = MX_BETA * r;
  return b - t;
}

__global__ __launch_bounds__(256) void mlp_quant_mx4_kernel(
    const float* __restrict__ w1, const float* __restrict__ b1, uint8_t* __restrict__ codes,
    uint8_t* __restrict__ scales, float* __restrict__ d1) {
  __shared__ float bsum[MX_BLOCKS];
  const int n = blockIdx.x, tid = threadIdx.x;
  const bool has = tid < MX_K / 4;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  const f32x4 w = has ? *reinterpret_cast<const f32x4*>(w1 + (int64_t)n * MX_K + 4 * tid) : z;
  const float m = block_max_dpp_nonneg(
      fmaxf(fmaxf(fabsf(w[0]), fabsf(w[1])), fmaxf(fabsf(w[2]), fabsf(w[3]))));
  // floor(log2 m) - 2 + 127 from the exponent field; subnormal maxima clamp to 0 as they should
  const int e8 = m == 0.f ? 127 : max((int)((__float_as_uint(m) >> 23) & 0xff) - 2, 0);
  uint32_t nib = 0;
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float a = fabsf(ldexpf(w[j], 127 - e8));     // |w / X|, exact
    const int c = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) +
                  (a >= 3.5f) + (a > 5.f);
    // the grid value of code c: c / 2 up to 2, then 3, 4, 6
    const float q = c <= 4 ? 0.5f * (float)c : (c == 5 ? 3.f : (c == 6 ? 4.f : 6.f));
    const bool neg = w[j] < 0.f && c != 0;
    sum += ldexpf(neg ? -q : q, e8 - 127);             // exact: <= 2 bits on the block's scale
    nib |= (uint32_t)(c | (neg ? 8 : 0)) << (4 * j);
  }
  const float bs = block_sum_dpp(sum);                 // exact too: 32 such values
  if (tid < MLP_MX4_KPAD / 4) {
    *reinterpret_cast<uint16_t*>(codes + (int64_t)n * MX_PITCH + 2 * tid) = (uint16_t)nib;
    if ((tid & 7) == 0) {
      scales[n * MX_BLOCKS + (tid >> 3)] = (uint8_t)e8;
      bsum[tid >> 3] = bs;
    }
  }
  __syncthreads();
  if (tid == 0) {
    float r = bsum[0];
    for (int k = 1; k < MX_REAL_BLOCKS; ++k) r += bsum[k];
    d1[n] = fold_bias_mx4(b1[n], r);
  }
}

// ------------------------------------------------------------------ mlp_fwd_mx4
// E4M3 bytes of n and of 16 n, n = 0 .. 15, as two 8-byte pools each (entry e = byte e of HI:LO):
// 0 -> 0x00, 1 -> 0x38, 2 -> 0x40, 3 -> 0x44, 4 .. 7 -> 0x48 + 2 (n - 4), 8 .. 15 -> 0x50 + (n - 8);
// times 16 is + 4 in the exponent field, + 0x20 (240 = 0x77 is below E4M3's maximum 448)
constexpr uint32_t LO0_L = 0x44403800u, LO0_H = 0x4E4C4A48u, LO1_L = 0x53525150u, LO1_H = 0x57565554u;
constexpr uint32_t HI0_L = 0x64605800u, HI0_H = 0x6E6C6A68u, HI1_L = 0x73727170u, HI1_H = 0x77767574u;

// the table entries of the four nibbles nb (one per byte, 0 .. 15): v_perm_b32's selectors 0 .. 3
// take the bytes of its second source, 4 .. 7 those of its first
template <bool HIGH>
__device__ __forceinline__ int e4m3_of_nibbles(uint32_t nb) {
  const uint32_t sel = nb & 0x07070707u;
  const uint32_t p0 = __builtin_amdgcn_perm(HIGH ? HI0_H : LO0_H, HIGH ? HI0_L : LO0_L, sel);
  const uint32_t p1 = __builtin_amdgcn_perm(HIGH ? HI1_H : LO1_H, HIGH ? HI1_L : LO1_L, sel);
  const uint32_t m = ((nb >> 3) & 0x01010101u) * 0xffu;     // 0xff in the bytes with bit 3 set
  return (int)((p1 & m) | (p0 & ~m));
}

// KPER = 7 / S k-steps per workgroup, every load issued before the first MFMA
template <int KPER>
__global__ __launch_bounds__(256) void mlp_fwd_mx4_kernel(
    const uint8_t* __restrict__ images, const int32_t* __restrict__ labels, int64_t nrow, int B,
    const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales,
    float* __restrict__ part, int32_t* __restrict__ ylab) {
  const int mtiles = (B + 15) / 16;
  const int mtile = blockIdx.x % mtiles, sidx = blockIdx.x / mtiles;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i16 = lane & 15;
  // rows >= B read a clamped valid row and store nothing
  const int b = min(mtile * 16 + i16, B - 1);
  if (sidx == 0 && wave == 0 && g == 0 && mtile * 16 + i16 < B) ylab[b] = labels[b];
  const int64_t xo = (int64_t)b * MX_K + 16 * g;    // A: k0 + 16 g and k0 + 64 + 16 g
  const int64_t xlast = nrow * MX_K - 16;           // the last 16 B of the buffer (16-B aligned)
  const int nrow0 = wave * 32 + i16;                // this lane's B rows: nrow0 and nrow0 + 16
  const uint8_t* crow = codes + (int64_t)nrow0 * MX_PITCH + 16 * g;
  const uint8_t* srow = scales + nrow0 * MX_BLOCKS + g;
  u32x4 xv[KPER][2];
  i32x4 wv[KPER][2];
  uint32_t sc[KPER][2];
#pragma unroll
  for (int s = 0; s < KPER; ++s) {
    const int k = (sidx * KPER + s) * 128;
    // a piece past column 783 (the last step's, all but lane group 0's first): any in-bounds
    // bytes, the codes there are zero
#pragma unroll
    for (int h = 0; h < 2; ++h)
      xv[s][h] = *reinterpret_cast<const u32x4*>(images + min(xo + k + 64 * h, xlast));
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      wv[s][nt] = *reinterpret_cast<const i32x4*>(crow + nt * 16 * MX_PITCH + k / 2);
      sc[s][nt] = srow[nt * 16 * MX_BLOCKS + k / 32];
    }
  }
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int s = 0; s < KPER; ++s) {
    i32x8 ahi, alo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t x = xv[s][j >> 2][j & 3];
      ahi[j] = e4m3_of_nibbles<true>((x >> 4) & 0x0f0f0f0fu);
      alo[j] = e4m3_of_nibbles<false>(x & 0x0f0f0f0fu);
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const i32x8 bq = {wv[s][nt][0], wv[s][nt][1], wv[s][nt][2], wv[s][nt][3], 0, 0, 0, 0};
      const int sb = (int)sc[s][nt];                // op_sel 0 reads byte 0 of the scale operand
      // A: fp8 E4M3 (cbsz 0) at scale 2^0 (127), B: fp4 E2M1 (blgp 4) at the block's scale
      acc[nt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(ahi, bq, acc[nt], 0, 4, 0,
                                                                 0x7f7f7f7f, 0, sb);
      acc[nt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(alo, bq, acc[nt], 0, 4, 0,
                                                                 0x7f7f7f7f, 0, sb);
    }
  }
  float* out = part + (int64_t)sidx * B * HID;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int n = wave * 32 + nt * 16 + i16;        // the D fragment's column
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rowi = mtile * 16 + 4 * g + r;
      if (rowi < B) out[(int64_t)rowi * HID + n] = MX_ALPHA * acc[nt][r];
    }
  }
}

}  // namespace

void launch_mlp_quant_mx4(const float* w1, const float* b1, uint8_t* codes, uint8_t* scales,
                          float* d1, hipStream_t st) {
  mlp_quant_mx4_kernel<<<HID, 256, 0, st>>>(w1, b1, codes, scales, d1);
}

void launch_mlp_fwd_mx4(const uint8_t* images, const int32_t* labels, int64_t nrow, int B,
                        const uint8_t* codes, const uint8_t* scales, float* part, int32_t* ylab,
                        int splitk, hipStream_t st) {
  const int grid = (B + 15) / 16 * splitk;
  if (splitk == MX_STEPS)
    mlp_fwd_mx4_kernel<1><<<grid, 256, 0, st>>>(images, labels, nrow, B, codes, scales, part, ylab);
  else
    mlp_fwd_mx4_kernel<MX_STEPS><<<grid, 256, 0, st>>>(images, labels, nrow, B, codes, scales, part,
                                                       ylab);
}
