// The hidden-layer MLP (--arch mlp: 784 -> fc1 128 -> ReLU -> fc2 10) on gfx950: its first
// layer, forward and weight gradient.  Everything behind fc1's pre-activation -- bias + ReLU,
// fc2, the loss, dlogits, dh, the head slabs -- is the CNN programs' head (cnn_head*.hip,
// predict.hip), which reads the [S][B][128] split-K partials this file's forward writes.
//
// Both GEMMs take the RAW uint8 IMAGE as one operand.  A byte 0..255 has 8 significant bits,
// so it is exact in bf16: it goes into v_mfma_f32_16x16x32_bf16 converted in registers, and
// only the other operand is split: W1 into hi = bf16(w), lo = bf16(w - hi) planes, two MFMAs
// per tile and not the three of cnn_f32x3.hip; dh, split in registers anyway, into three parts
// (hi, mid, lo: all 24 bits), because a batch of one row has nothing to average two planes'
// 2^-17 |dh| remainder over (docs/kernels.md "MLP": the error bound).  The normalisation
// x = (u8 / 255 - 0.1307) / 0.3081 = alpha u8 - beta is affine and folded out of the GEMMs:
//
//   pre[b][n] = alpha sum_k W[n][k] u8[b][k] - beta sum_k W[n][k]        (+ b1[n]: the head)
//   dW1[n][k] = alpha sum_b dh[b][n] u8[b][k] - beta sum_b dh[b][n]
//
// and the second sums come from the fragments a lane holds anyway (VALU adds, then the xor-16
// / xor-32 lane swaps): with the non-image operand as the MFMA's B operand, lane (g, i16)
// holds 8 k-values of column i16, and the D fragment it ends up with is of column i16 too.
//
//   mlp_fwd  (m-tile of 16 rows, split s of S) workgroups, 4 waves x 32 hidden units.  The 784
//            pixels are 25 k-steps of 32 (the last one half: lanes g >= 2 take zero weights),
//            S in {1, 5, 25} splits of 25 / S steps.  Lane (g, i16) loads 8 bytes of row i16
//            (a 16-lane group and its 4 g's: 16 rows x one 32-B line piece) and 16 B of each
//            weight plane; every load of up to 5 steps is in flight before the first MFMA.
//   mlp_bwd  blocks 0..48: dW1 tiles of 16 pixels x 128 hidden units, K = the batch in rounds
//            of 128 rows: the round's [128 rows][16 pixels] bytes go through LDS transposed
//            ([pixel][row], 144-B pitch, double-buffered: one barrier per round), so a lane
//            reads the 8 consecutive rows of its pixel as one ds_read_b64; dh32 comes straight
//            from memory (16 lanes: one 64-B piece of a row) and is split in registers (3 parts).
//            Blocks 49..71: the head-slab reduction (cnn_f32_common.h head_slab_reduce).
//            Fixed round and step order: the gradient is bit-reproducible.
//
// LDS bank model (tools/lds_bank_model.py mlp_bwd): the transposed byte writes (a wave: 64
// consecutive bytes of one pixel row) and the b64 fragment reads (pitch 144 B = 36 dwords:
// the 16 pixels' 4-dword windows tile the 64 banks) both take the conflict-free pass count.
#include "cnn_f32_common.h"

namespace {

using namespace cnn;

constexpr int MLP_K = MLP_IN;                       // 784 pixels
constexpr int MF_STEPS = (MLP_K + 31) / 32;         // 25 k-steps, the last half empty
constexpr float MLP_ALPHA = (float)(1.0 / (255.0 * 0.3081));
constexpr float MLP_BETA = (float)(0.1307 / 0.3081);
constexpr int MB_PX = 16, MB_TILES = MLP_K / MB_PX;            // 49 dW1 tiles
constexpr int MB_ROUND = 128, MB_PITCH = 144, MB_BUF = MB_PX * MB_PITCH;
static_assert(MLP_K % MB_PX == 0 && MF_STEPS == 25 && HID == 128, "mlp geometry");
static_assert(2 * MB_BUF >= 256 * 4 + 256 * 8, "head_slab_reduce's scratch fits the tile's LDS");

// 8 bytes -> 8 bf16, exact: a float of an integer < 256 has nothing below its top 16 bits
__device__ __forceinline__ bf16x8 u8x8_bf16(uint2 v) {
  u32x4 w;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t word = j < 2 ? v.x : v.y;
    const int sh = 16 * (j & 1);
    const float f0 = (float)((word >> sh) & 0xffu), f1 = (float)((word >> (sh + 8)) & 0xffu);
    w[j] = (__float_as_uint(f0) >> 16) | (__float_as_uint(f1) & 0xffff0000u);
  }
  return __builtin_bit_cast(bf16x8, w);
}

__device__ __forceinline__ f32x4 mfma2(bf16x8 a, bf16x8 bh, bf16x8 bl, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bl, c, 0, 0, 0);   // small terms first
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bh, c, 0, 0, 0);
}

// ------------------------------------------------------------------ mlp_fwd
// KPER = 25 / S k-steps per workgroup, taken in chunks of CH = min(KPER, 5) whose loads are
// all issued first.
template <int KPER>
__global__ __launch_bounds__(256) void mlp_fwd_kernel(
    const uint8_t* __restrict__ images, const int32_t* __restrict__ labels, int64_t nrow,
    const int64_t* __restrict__ ctr, StepRows sr, int B, const bf16* __restrict__ whi,
    const bf16* __restrict__ wlo, float* __restrict__ part, int32_t* __restrict__ ylab) {
  constexpr int CH = KPER < 5 ? KPER : 5;
  const int mtiles = (B + 15) / 16;
  const int mtile = blockIdx.x % mtiles, sidx = blockIdx.x / mtiles;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i16 = lane & 15;
  // rows >= B read a clamped valid row and store nothing; a counter driven past the epoch
  // reads a valid row (as cnn_fwd)
  const int b = min(mtile * 16 + i16, B - 1);
  const int64_t row = max(min(ctr ? step_row(sr, nrow, *ctr, b) : (int64_t)b, nrow - 1), (int64_t)0);
  if (sidx == 0 && wave == 0 && g == 0 && mtile * 16 + i16 < B) ylab[b] = labels[row];
  const uint8_t* xrow = images + row * MLP_K + 8 * g;
  const int64_t wo = (int64_t)(wave * 32 + i16) * MLP_K + 8 * g;
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  float ws[2] = {0.f, 0.f};
  for (int s0 = 0; s0 < KPER; s0 += CH) {
    uint2 xv[CH];
    bf16x8 bh[CH][2], bl[CH][2];
    bool on[CH];
#pragma unroll
    for (int s = 0; s < CH; ++s) {
      const int k = (sidx * KPER + s0 + s) * 32;
      on[s] = k + 8 * g < MLP_K;                    // the half step: lanes g >= 2 are past the row
      const int ko = on[s] ? k : 0;
      xv[s] = *reinterpret_cast<const uint2*>(xrow + ko);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        bh[s][nt] = *reinterpret_cast<const bf16x8*>(whi + wo + nt * 16 * MLP_K + ko);
        bl[s][nt] = *reinterpret_cast<const bf16x8*>(wlo + wo + nt * 16 * MLP_K + ko);
      }
    }
#pragma unroll
    for (int s = 0; s < CH; ++s) {
      const bf16x8 a = u8x8_bf16(xv[s]);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const u32x4 z = {0u, 0u, 0u, 0u};
        const bf16x8 h = on[s] ? bh[s][nt] : __builtin_bit_cast(bf16x8, z);
        const bf16x8 l = on[s] ? bl[s][nt] : __builtin_bit_cast(bf16x8, z);
        float t = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) t += from_bf16(h[j]) + from_bf16(l[j]);
        ws[nt] += t;
        acc[nt] = mfma2(a, h, l, acc[nt]);
      }
    }
  }
  float* out = part + (int64_t)sidx * B * HID;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    // this split's share of sum_k W[n][k], n = the D fragment's column
    const float fold = MLP_BETA * sum_xor32(sum_xor16(ws[nt]));
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rowi = mtile * 16 + 4 * g + r;
      if (rowi < B) out[(int64_t)rowi * HID + wave * 32 + nt * 16 + i16] = fmaf(MLP_ALPHA, acc[nt][r], -fold);
    }
  }
}

// ------------------------------------------------------------------ mlp_bwd
// COLSUM (--arch mlp2): tile 0 also stores the column sums of dh that the fold is made of
template <bool COLSUM>
__global__ __launch_bounds__(256) void mlp_bwd_kernel(
    const uint8_t* __restrict__ images, int64_t nrow, const int64_t* __restrict__ ctr, int64_t cback,
    StepRows sr, int B, const float* __restrict__ dh, float* __restrict__ gw1,
    const float* __restrict__ head_slab, int head_blocks, float* __restrict__ gwf2,
    float* __restrict__ gbf2, float* __restrict__ gbf1, double* __restrict__ metrics,
    float* __restrict__ dh_colsum) {
  __shared__ __attribute__((aligned(16))) char sm[2 * MB_BUF];
  const int bid = blockIdx.x;
  if (bid >= MB_TILES) {
    head_slab_reduce(reinterpret_cast<float*>(sm), bid - MB_TILES, head_slab, head_blocks, B, gwf2,
                     gbf2, gbf1, metrics);
    return;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i16 = lane & 15;
  const int px0 = bid * MB_PX;
  // the step's rows: the forward's (the head in between has advanced the counter: cback = 1)
  const int64_t c = ctr ? *ctr - cback : 0;
  // staging role: row tid & 127 of the round, pixels 8 (tid >> 7) .. + 7 of the tile
  const int srow = tid & (MB_ROUND - 1), shalf = tid >> 7;
  auto xload = [&](int r0) __attribute__((always_inline)) {
    const int b = min(r0 + srow, B - 1);
    const int64_t row = max(min(ctr ? step_row(sr, nrow, c, b) : (int64_t)b, nrow - 1), (int64_t)0);
    return *reinterpret_cast<const uint2*>(images + row * MLP_K + px0 + 8 * shalf);
  };
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  float rs[2] = {0.f, 0.f};
  uint2 xv = xload(0);
  for (int r0 = 0, rd = 0; r0 < B; r0 += MB_ROUND, ++rd) {
    // the round's dh rows (k = 8 g + j of each 32-row step; rows >= B are zero), hidden unit
    // 32 wave + 16 nt + i16: in flight across the staging and the barrier
    float v[4][2][8];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int rb = r0 + 32 * ks + 8 * g + j;
        const float* p = dh + (int64_t)min(rb, B - 1) * HID + wave * 32 + i16;
        v[ks][0][j] = p[0];
        v[ks][1][j] = p[16];
      }
    char* buf = sm + (rd & 1) * MB_BUF;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      buf[(8 * shalf + j) * MB_PITCH + srow] = (char)((j < 4 ? xv.x : xv.y) >> (8 * (j & 3)));
    __syncthreads();   // (the other buffer's readers passed the previous round's barrier)
    if (r0 + MB_ROUND < B) xv = xload(r0 + MB_ROUND);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const bf16x8 a = u8x8_bf16(*reinterpret_cast<const uint2*>(buf + i16 * MB_PITCH + 32 * ks + 8 * g));
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        bf16x8 h, m, l;
        float t = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float x = (r0 + 32 * ks + 8 * g + j < B) ? v[ks][nt][j] : 0.f;
          h[j] = to_bf16(x);
          const float r1 = x - from_bf16(h[j]);      // (both remainders are exact in fp32)
          m[j] = to_bf16(r1);
          l[j] = to_bf16(r1 - from_bf16(m[j]));
          t += x;
        }
        rs[nt] += t;
        acc[nt] = mfma2(a, m, l, acc[nt]);
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, h, acc[nt], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    // sum_b dh[b][n], n = the D fragment's column; the lane's rows are pixels 4 g .. 4 g + 3
    const float cs = sum_xor32(sum_xor16(rs[nt]));
    if constexpr (COLSUM) {
      if (bid == 0 && g == 0) dh_colsum[wave * 32 + nt * 16 + i16] = cs;
    }
    const float fold = MLP_BETA * cs;
    const f32x4 o = {fmaf(MLP_ALPHA, acc[nt][0], -fold), fmaf(MLP_ALPHA, acc[nt][1], -fold),
                     fmaf(MLP_ALPHA, acc[nt][2], -fold), fmaf(MLP_ALPHA, acc[nt][3], -fold)};
    *reinterpret_cast<f32x4*>(gw1 + (int64_t)(wave * 32 + nt * 16 + i16) * MLP_K + px0 + 4 * g) = o;
  }
}

}  // namespace

void launch_mlp_fwd(const uint8_t* images, const int32_t* labels, int64_t nrow, const int64_t* ctr,
                    StepRows sr, int B, const __bf16* whi, const __bf16* wlo, float* part,
                    int32_t* ylab, int splitk, hipStream_t st) {
  const int grid = (B + 15) / 16 * splitk;
  if (splitk == 25)
    mlp_fwd_kernel<1><<<grid, 256, 0, st>>>(images, labels, nrow, ctr, sr, B, whi, wlo, part, ylab);
  else if (splitk == 5)
    mlp_fwd_kernel<5><<<grid, 256, 0, st>>>(images, labels, nrow, ctr, sr, B, whi, wlo, part, ylab);
  else
    mlp_fwd_kernel<25><<<grid, 256, 0, st>>>(images, labels, nrow, ctr, sr, B, whi, wlo, part, ylab);
}

void launch_mlp_bwd(const uint8_t* images, int64_t nrow, const int64_t* ctr, int64_t cback,
                    StepRows sr, int B, const float* dh32, float* gw1, const float* head_slab,
                    int head_blocks, float* gwf2, float* gbf2, float* gbf1, double* metrics,
                    hipStream_t st, float* dh_colsum) {
  if (dh_colsum != nullptr)
    mlp_bwd_kernel<true><<<MB_TILES + HRB, 256, 0, st>>>(images, nrow, ctr, cback, sr, B, dh32, gw1,
                                                         head_slab, head_blocks, gwf2, gbf2, gbf1,
                                                         metrics, dh_colsum);
  else
    mlp_bwd_kernel<false><<<MB_TILES + HRB, 256, 0, st>>>(images, nrow, ctr, cback, sr, B, dh32, gw1,
                                                          head_slab, head_blocks, gwf2, gbf2, gbf1,
                                                          metrics, nullptr);
}
