// 2:4 sparse evaluation of the MLPs' first layer (--quantize sparse24; docs/kernels.md "2:4 sparse
// evaluation") on gfx950's structured-sparsity matrix cores, v_smfmac_f32_16x16x64_bf16: the A
// operand holds 2 of every 4 consecutive k, an index register says which two.
//
// Pruning: a row of fc1.weight [128][784] is 196 groups of 4 consecutive columns; a group keeps
// the two entries that rank first by (|w| descending, column ascending), with their fp32 bits,
// and the other two become zero.  (An all-zero group keeps columns 0 and 1; weights are finite.)
// The kept columns of a group are two 2-bit positions p0 < p1.  With Wp the pruned matrix,
//
//   pre[b][n] = alpha sum_k Wp[n][k] u8[b][k] + d1[n],   d1[n] = b1[n] - beta sum_k Wp[n][k]
//
// and the weights keep fp32 semantics as in mlp.hip: two bf16 planes, hi = bf16(w) and
// lo = bf16(w - hi), of the kept entries only.  The pixels are the exact bytes.
//
//   mlp_prune_24   one workgroup per hidden unit, once per weight set: lane t < 196 holds group t
//                  (one 16-B load), ranks its four entries by six comparisons and stores the two
//                  survivors' hi and lo bf16 pairs (4 B each) into the compressed planes
//                  [128][416] (832 / 2 columns: lanes 196 .. 207 store the zero padding).  The
//                  group's nibble p0 | p1 << 2 is packed across lanes in registers: an OR over the
//                  quad on the DPP network gives 16 bits (four groups = the 16 dense columns of
//                  one lane of the forward), the lane 16 further on supplies the next k-step's 16
//                  bits, and every 32nd lane's quads store a word: index [128][7][4] uint32,
//                  word (kp, g) = k-step 2 kp in its low half and 2 kp + 1 in its high half, of
//                  lane group g.  The row sum goes over the DPP network per wave and through four
//                  LDS words across the waves, in a fixed order.
//   mlp_fwd_sp24   (m-tile of 16 batch rows, split s of S) workgroups, 4 waves x 32 hidden units,
//                  as mlp_fwd.  The sparse operand is A, so the weights are A and the image is B.
//                  832 columns are 13 k-steps of 64, S in {1, 13}.  The instruction's operand
//                  maps, as measured on the device (docs/kernels.md: the probe), differ: the A
//                  lane (g, i16) holds the 8 survivors of row i16's 16 consecutive columns k0 +
//                  16 g .. + 15, element e placed by bits 2 e, 2 e + 1 of the half of the index
//                  register that abid names; the B lane (g, i16) holds column i16's k0 + 8 g ..
//                  + 7 (elements 0 .. 7) and k0 + 32 + 8 g .. + 7 (elements 8 .. 15).  So a lane
//                  loads those two 8-B pieces of image row i16 and widens them in registers to
//                  16 exact bf16; for each of its two unit tiles it loads 16 B of each plane and
//                  the index word (one word serves two k-steps); four sparse MFMAs per k-step
//                  share the image fragment, the low plane first.  The D fragment of lane (g,
//                  i16) is units 4 g .. 4 g + 3 of batch row i16: one 16-B store per tile into
//                  mlp_fwd's [S][B][128] partials.  The last k-step covers k = 768 .. 831: the
//                  planes are zero from 784 on and a widened byte is finite, so whatever bytes
//                  the pieces past column 783 read multiply to exactly 0; every piece's address
//                  is clamped to the last 8 B of the image buffer.  No LDS, no atomics, a fixed
//                  order: bit-reproducible.  part = alpha acc, one rounding.
//
// d1's product feeds a difference, so it sits under `#pragma clang fp contract(off)` as
// mlp_i8.hip's fold_bias.  runtime/cpu_step.py prune_fc1_24 is the same definition in NumPy.
#include "cnn_f32_common.h"

namespace {

using namespace cnn;

typedef __bf16 bf16x16 __attribute__((ext_vector_type(16)));

constexpr int SP_K = MLP_IN;                        // 784 pixels
constexpr int SP_GROUPS = SP_K / 4;                 // 196 groups of a row
constexpr int SP_STEPS = MLP_SP24_KPAD / 64;        // 13 k-steps
constexpr int SP_PITCH = MLP_SP24_KPAD / 2;         // 416 bf16 of a compressed row
constexpr int SP_WORDS = (SP_STEPS + 1) / 2 * 4;    // 28 index words of a row
constexpr float SP_ALPHA = (float)(1.0 / (255.0 * 0.3081));
constexpr float SP_BETA = (float)(0.1307 / 0.3081);
static_assert(MLP_SP24_KPAD % 64 == 0 && MLP_SP24_KPAD >= SP_K && SP_STEPS == 13 && SP_K % 16 == 0 &&
              SP_WORDS == 28 && HID == 128, "sparse fc1 geometry");

// ------------------------------------------------------------------ mlp_prune_24
__device__ __forceinline__ float wave_sum_dpp_f32(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124, 0xf, 0xf, false));  // row_ror:4
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xf, 0xf, false));  // row_ror:8
  const int i = __float_as_int(v);
  return (__int_as_float(__builtin_amdgcn_readlane(i, 0)) + __int_as_float(__builtin_amdgcn_readlane(i, 16))) +
         (__int_as_float(__builtin_amdgcn_readlane(i, 32)) + __int_as_float(__builtin_amdgcn_readlane(i, 48)));
}

// d1 = b1 - beta R in two roundings (the pragma: see the header)
__device__ __forceinline__ float fold_bias_sp24(float b, float r) {
#pragma clang fp contract(off)
  const float t = SP_BETA * r;
  return b - t;
}

// the low plane's element of a survivor: the remainder is exact in fp32
__device__ __forceinline__ bf16 lo_bf16(float w) { return to_bf16(w - from_bf16(to_bf16(w))); }

__global__ __launch_bounds__(256) void mlp_prune_24_kernel(
    const float* __restrict__ w1, const float* __restrict__ b1, bf16* __restrict__ whi,
    bf16* __restrict__ wlo, uint32_t* __restrict__ index, float* __restrict__ d1) {
  __shared__ float ssum[4];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool has = tid < SP_GROUPS;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  const f32x4 w = has ? *reinterpret_cast<const f32x4*>(w1 + (int64_t)n * SP_K + 4 * tid) : z;
  // entry j survives if fewer than two entries rank before it: a larger magnitude, or an equal
  // one in a lower column
  const float a[4] = {fabsf(w[0]), fabsf(w[1]), fabsf(w[2]), fabsf(w[3])};
  int before[4] = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = i + 1; j < 4; ++j) {
      const bool first = a[i] >= a[j];              // i < j: a tie goes to i
      before[j] += first;
      before[i] += !first;
    }
  // p0 = the lowest surviving column, p1 = the highest
  const int p0 = before[0] < 2 ? 0 : (before[1] < 2 ? 1 : 2);
  const int p1 = before[3] < 2 ? 3 : (before[2] < 2 ? 2 : 1);
  const float c0 = p0 == 0 ? w[0] : (p0 == 1 ? w[1] : w[2]);
  const float c1 = p1 == 3 ? w[3] : (p1 == 2 ? w[2] : w[1]);
  if (tid < SP_PITCH / 2) {
    const bf16x2 h = {to_bf16(c0), to_bf16(c1)}, l = {lo_bf16(c0), lo_bf16(c1)};
    *reinterpret_cast<bf16x2*>(whi + (int64_t)n * SP_PITCH + 2 * tid) = h;
    *reinterpret_cast<bf16x2*>(wlo + (int64_t)n * SP_PITCH + 2 * tid) = l;
  }
  // group t = 32 kp + 16 h + 4 g + q: nibble q of half h of word (kp, g)
  int v = has ? (p0 | (p1 << 2)) << (4 * (tid & 3)) : 0;
  v |= __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);    // quad_perm [1,0,3,2]
  v |= __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);    // quad_perm [2,3,0,1]
  const int up = __builtin_amdgcn_ds_bpermute(((lane + 16) & 63) << 2, v);   // lane + 16's 16 bits
  if ((tid & 0x13) == 0 && tid < 8 * SP_WORDS)
    index[n * SP_WORDS + (tid >> 5) * 4 + ((tid >> 2) & 3)] = (uint32_t)v | ((uint32_t)up << 16);
  const float sw = wave_sum_dpp_f32(c0 + c1);
  if (lane == 0) ssum[wave] = sw;
  __syncthreads();
  if (tid == 0) d1[n] = fold_bias_sp24(b1[n], (ssum[0] + ssum[1]) + (ssum[2] + ssum[3]));
}

// ------------------------------------------------------------------ mlp_fwd_sp24
// two 8-byte pieces -> 16 bf16, exact: a float of an integer < 256 has nothing below its top 16
// bits
__device__ __forceinline__ bf16x16 u8x16_bf16(uint2 p0, uint2 p1) {
  const uint32_t v[4] = {p0.x, p0.y, p1.x, p1.y};
  uint32_t w[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint32_t word = v[j >> 1];
    const int sh = 16 * (j & 1);
    const float f0 = (float)((word >> sh) & 0xffu), f1 = (float)((word >> (sh + 8)) & 0xffu);
    // the high halves of f1 : f0
    w[j] = __builtin_amdgcn_perm(__float_as_uint(f1), __float_as_uint(f0), 0x07060302u);
  }
  return __builtin_bit_cast(bf16x16, w);
}

// one k-step of one unit tile: the low plane first (small terms first, as mlp.hip's mfma2); HALF
// = which 16 bits of the index word are this k-step's (the instruction's abid)
template <int HALF>
__device__ __forceinline__ f32x4 smfma2(bf16x8 ah, bf16x8 al, bf16x16 b, int idx, f32x4 c) {
  c = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(al, b, c, idx, 0, HALF);
  return __builtin_amdgcn_smfmac_f32_16x16x64_bf16(ah, b, c, idx, 0, HALF);
}

// KPER = 13 / S k-steps per workgroup, every load issued before the first MFMA
template <int KPER>
__global__ __launch_bounds__(256) void mlp_fwd_sp24_kernel(
    const uint8_t* __restrict__ images, const int32_t* __restrict__ labels, int64_t nrow, int B,
    const bf16* __restrict__ whi, const bf16* __restrict__ wlo, const uint32_t* __restrict__ index,
    float* __restrict__ part, int32_t* __restrict__ ylab) {
  const int mtiles = (B + 15) / 16;
  const int mtile = blockIdx.x % mtiles, sidx = blockIdx.x / mtiles;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i16 = lane & 15;
  // rows >= B read a clamped valid row and store nothing
  const int b = min(mtile * 16 + i16, B - 1);
  if (sidx == 0 && wave == 0 && g == 0 && mtile * 16 + i16 < B) ylab[b] = labels[b];
  const int64_t xo = (int64_t)b * SP_K + 8 * g;     // B: k0 + 8 g and k0 + 32 + 8 g
  const int64_t xlast = nrow * SP_K - 8;            // the last 8 B of the buffer (8-B aligned)
  const int unit = wave * 32 + i16;                 // this lane's A rows: unit and unit + 16
  const int64_t wo = (int64_t)unit * SP_PITCH + 8 * g;
  const uint32_t* irow = index + unit * SP_WORDS + g;
  constexpr int NW = (KPER + 1) / 2;
  uint2 xv[KPER][2];
  bf16x8 ah[KPER][2], al[KPER][2];
  uint32_t iw[NW][2];
#pragma unroll
  for (int s = 0; s < KPER; ++s) {
    const int ks = sidx * KPER + s;
    // a piece past column 783 (the last step's, all but lane groups 0 and 1's first): any
    // in-bounds bytes, the planes are zero there
#pragma unroll
    for (int h = 0; h < 2; ++h)
      xv[s][h] = *reinterpret_cast<const uint2*>(images + min(xo + 64 * ks + 32 * h, xlast));
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      ah[s][nt] = *reinterpret_cast<const bf16x8*>(whi + wo + nt * 16 * SP_PITCH + 32 * ks);
      al[s][nt] = *reinterpret_cast<const bf16x8*>(wlo + wo + nt * 16 * SP_PITCH + 32 * ks);
      if ((s & 1) == 0) iw[s >> 1][nt] = irow[nt * 16 * SP_WORDS + (ks >> 1) * 4];
    }
  }
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int s = 0; s < KPER; ++s) {
    const bf16x16 x = u8x16_bf16(xv[s][0], xv[s][1]);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      if (KPER == 1)      // a split's one k-step: its half of the word, moved down
        acc[nt] = smfma2<0>(ah[s][nt], al[s][nt], x, (int)(iw[0][nt] >> (16 * (sidx & 1))), acc[nt]);
      else if (s & 1)
        acc[nt] = smfma2<1>(ah[s][nt], al[s][nt], x, (int)iw[s >> 1][nt], acc[nt]);
      else
        acc[nt] = smfma2<0>(ah[s][nt], al[s][nt], x, (int)iw[s >> 1][nt], acc[nt]);
    }
  }
  // the D fragment: units 4 g .. 4 g + 3 of the tile, batch row i16
  if (mtile * 16 + i16 < B) {
    float* out = part + ((int64_t)sidx * B + b) * HID + wave * 32 + 4 * g;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
      *reinterpret_cast<f32x4*>(out + nt * 16) = SP_ALPHA * acc[nt];
  }
}

}  // namespace

void launch_mlp_prune_24(const float* w1, const float* b1, __bf16* whi, __bf16* wlo, uint32_t* index,
                         float* d1, hipStream_t st) {
  mlp_prune_24_kernel<<<HID, 256, 0, st>>>(w1, b1, whi, wlo, index, d1);
}

void launch_mlp_fwd_sp24(const uint8_t* images, const int32_t* labels, int64_t nrow, int B,
                         const __bf16* whi, const __bf16* wlo, const uint32_t* index, float* part,
                         int32_t* ylab, int splitk, hipStream_t st) {
  const int grid = (B + 15) / 16 * splitk;
  if (splitk == SP_STEPS)
    mlp_fwd_sp24_kernel<1><<<grid, 256, 0, st>>>(images, labels, nrow, B, whi, wlo, index, part, ylab);
  else
    mlp_fwd_sp24_kernel<SP_STEPS><<<grid, 256, 0, st>>>(images, labels, nrow, B, whi, wlo, index, part,
                                                        ylab);
}
