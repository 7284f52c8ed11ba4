// The hidden-to-hidden layer of the two-hidden-layer MLP (--arch mlp2: 784 -> fc1 128 -> ReLU ->
// fc2 128 -> ReLU -> fc3 10) on gfx950, forward and backward.  It sits between mlp_fwd /
// mlp_bwd (mlp.hip), which keep the first layer, and the CNN programs' head (cnn_head*.hip,
// predict.hip), which takes fc2's bias + ReLU and fc3 as its "fc1 bias" and "fc2".
//
// Both operands of every product here are genuine fp32 arrays (activations, dh, the fp32 master
// weight), so the products run on v_mfma_f32_16x16x4_f32 (mfma4, cnn_f32_common.h: lane l =
// 16 g + i holds A[m = i][k = g], B[k = g][n = i], D[m = 4 g + r][n = i]): exact fp32
// products, fp32 accumulation, no planes to keep current.  The MFMA sums over k, so which k a
// (step, lane group g) pair stands for is free as long as A and B agree; each GEMM picks the
// assignment that makes its loads wide.
//
//   mlp_hid_fwd  (m-tile of 16 rows, group of 64 NT output units) workgroups, 4 waves x NT
//                n-tiles.  Phase 1: thread t owns row t >> 4 and the float2's 2 (t & 15) + 32 j
//                of it, sums b1 + the S split-K partials in split order (the head's convention;
//                5 splits = 20 loads in flight), applies the ReLU, stores h1 (the first unit
//                group's workgroup only) and keeps the tile in LDS, [16][136] fp32.  Phase 2:
//                k = 16 q + 4 g + c for step 4 q + c, so a lane's 32 weights of row n are eight
//                16-B loads whose four g-lanes share one 64-B piece (issued before phase 1: they
//                land under the partial sums) and its 32 A values are eight ds_read_b128 of
//                one LDS row; 32 MFMAs per n-tile.
//   mlp_hid_bwd  blocks 0 .. 2 mtiles - 1: dh1 (m-tile of 16 rows, 64 columns k), one 16-column
//                tile per wave.  A = dh2 rows straight from memory (n = 16 q + 4 g + c: eight
//                16-B loads of the lane's row), B = W2[n][k0 + i16] (16 lanes: one 64-B piece of
//                row n), the ReLU mask of h1 applied to the D fragment in registers.
//                The next 64 blocks: the 16 x 16 tiles of dW2, K = the batch in rounds of 128
//                rows; row r0 + 16 step + 4 wave + g goes to wave `wave`, both operands read
//                [b][.] with 16 lanes on a 64-B row piece, the next round's loads in flight
//                ahead of this round's MFMAs; the four waves' fragments meet in LDS and are
//                added in wave order.  Fixed round, step and wave order: bit-reproducible.
//                Rows >= B of h1 and dh are never read (clamped addresses) and enter as zeros.
//
// (k = 32 g + step, 128 contiguous bytes per lane, put the 64 lanes of every weight load on 64
// different cache lines: 16 such loads per wave cost g = 1 about 1.4 us at B = 256.)
//
// LDS bank model (tools/lds_bank_model.py mlp_hid_fwd): pitch 136 dwords (8 mod 64) puts the 16
// lanes of every ds_read_b128 group on the 64 banks once each (8 i16 + 4 g), and the phase-1
// ds_write_b64 of 16 lanes cover 32 consecutive dwords.
#include "cnn_f32_common.h"

namespace {

using namespace cnn;

constexpr int HF_PITCH = 136;            // dwords per LDS row of the h1 tile
constexpr int HB_ROUND = MLP_HID_ROUND;  // dW2: batch rows per round (32 per wave)
constexpr int HB_DW = (HID / 16) * (HID / 16);   // 64 dW2 tiles
static_assert(HID == 128 && HB_ROUND == 128, "mlp_hid geometry");

// ------------------------------------------------------------------ mlp_hid_fwd
// HF_CH: split-K partials in flight per batch (1: mlp_fwd's one split of the large batches)
template <int NT, int HF_CH>
__global__ __launch_bounds__(256) void mlp_hid_fwd_kernel(
    const float* __restrict__ part, int S, int B, const float* __restrict__ b1,
    const float* __restrict__ w2, float* __restrict__ h1, float* __restrict__ pre2) {
  __shared__ __attribute__((aligned(16))) float tile[16 * HF_PITCH];
  constexpr int NGRP = 2 / NT;                     // unit groups of 64 NT per m-tile
  const int mtile = blockIdx.x / NGRP, ngrp = blockIdx.x % NGRP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i16 = lane & 15;
  const int n0 = ngrp * 64 * NT + wave * 16 * NT;
  // the lane's 32 weights of row n (k = 16 q + 4 g + c) per n-tile
  f32x4 wv[NT][8];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int q = 0; q < 8; ++q)
      wv[nt][q] = *reinterpret_cast<const f32x4*>(w2 + (int64_t)(n0 + nt * 16 + i16) * HID + 16 * q + 4 * g);
  // phase 1: rows >= B read a clamped valid row and store nothing
  const int prow = tid >> 4, pc = tid & 15;
  const int row = mtile * 16 + prow;
  const float* prt = part + (int64_t)min(row, B - 1) * HID + 2 * pc;
  float2 h[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) h[j] = *reinterpret_cast<const float2*>(b1 + 2 * pc + 32 * j);
  for (int s0 = 0; s0 < S; s0 += HF_CH) {
    float2 u[HF_CH][4];
#pragma unroll
    for (int q = 0; q < HF_CH; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        u[q][j] = *reinterpret_cast<const float2*>(prt + (int64_t)min(s0 + q, S - 1) * B * HID + 32 * j);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < HF_CH; ++q) {
      const bool on = s0 + q < S;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        h[j].x += on ? u[q][j].x : 0.f;
        h[j].y += on ? u[q][j].y : 0.f;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    h[j].x = fmaxf(h[j].x, 0.f);
    h[j].y = fmaxf(h[j].y, 0.f);
    *reinterpret_cast<float2*>(tile + prow * HF_PITCH + 2 * pc + 32 * j) = h[j];
    if (h1 != nullptr && ngrp == 0 && row < B)
      st_ho<8>(reinterpret_cast<float2*>(h1 + (int64_t)row * HID + 2 * pc + 32 * j), h[j]);
  }
  __syncthreads();
  // phase 2
  f32x4 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* arow = tile + i16 * HF_PITCH + 4 * g;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(arow + 16 * q);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[nt] = mfma4(a[c], wv[nt][q][c], acc[nt]);
  }
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = mtile * 16 + 4 * g + r;
      if (orow < B) st_ho<8>(pre2 + (int64_t)orow * HID + n0 + nt * 16 + i16, acc[nt][r]);
    }
}

// ------------------------------------------------------------------ mlp_hid_bwd
__global__ __launch_bounds__(256) void mlp_hid_bwd_kernel(
    const float* __restrict__ dh2, const float* __restrict__ h1, const float* __restrict__ w2, int B,
    float* __restrict__ dh1, float* __restrict__ gw2) {
  __shared__ f32x4 red[4][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i16 = lane & 15;
  const int ndx = 2 * ((B + 15) / 16);
  const int bid = blockIdx.x;
  if (bid < ndx) {
    // ---- dh1[b][k] = [h1[b][k] > 0] sum_n dh2[b][n] W2[n][k]
    const int mtile = bid >> 1, k0 = (bid & 1) * 64 + wave * 16;
    const int arow = mtile * 16 + i16;
    const bool aon = arow < B;
    f32x4 av[8];
    const float* ap = dh2 + (int64_t)min(arow, B - 1) * HID + 4 * g;
#pragma unroll
    for (int q = 0; q < 8; ++q) av[q] = *reinterpret_cast<const f32x4*>(ap + 16 * q);
    float bv[32];      // step s = 4 q + c: n = 16 q + 4 g + c
#pragma unroll
    for (int s = 0; s < 32; ++s) bv[s] = w2[(int64_t)(16 * (s >> 2) + 4 * g + (s & 3)) * HID + k0 + i16];
    float hm[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      hm[r] = h1[(int64_t)min(mtile * 16 + 4 * g + r, B - 1) * HID + k0 + i16];
    __builtin_amdgcn_sched_barrier(0);   // every load is in flight before the first MFMA
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 32; ++s) acc = mfma4(aon ? av[s >> 2][s & 3] : 0.f, bv[s], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = mtile * 16 + 4 * g + r;
      if (orow < B) st_ho<8>(dh1 + (int64_t)orow * HID + k0 + i16, hm[r] > 0.f ? acc[r] : 0.f);
    }
    return;
  }
  // ---- dW2[n][k] = sum_b dh2[b][n] h1[b][k], tile (n0, k0)
  const int t = bid - ndx;
  const int n0 = (t >> 3) * 16, k0 = (t & 7) * 16;
  const float* pa = dh2 + n0 + i16;
  const float* pb = h1 + k0 + i16;
  float a[8], b[8];
  auto load = [&](int r0) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int64_t rb = min(r0 + 16 * s + 4 * wave + g, B - 1);
      a[s] = pa[rb * HID];
      b[s] = pb[rb * HID];
    }
  };
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  load(0);
  for (int r0 = 0; r0 < B; r0 += HB_ROUND) {
    float ca[8], cb[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const bool on = r0 + 16 * s + 4 * wave + g < B;
      ca[s] = on ? a[s] : 0.f;
      cb[s] = on ? b[s] : 0.f;
    }
    if (r0 + HB_ROUND < B) load(r0 + HB_ROUND);
#pragma unroll
    for (int s = 0; s < 8; ++s)
      if (r0 + 16 * s < B) acc = mfma4(ca[s], cb[s], acc);     // (workgroup-uniform)
  }
  red[wave][lane] = acc;
  __syncthreads();
  if (wave == 0) {
    const f32x4 o = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
#pragma unroll
    for (int r = 0; r < 4; ++r) gw2[(int64_t)(n0 + 4 * g + r) * HID + k0 + i16] = o[r];
  }
}

}  // namespace

void launch_mlp_hid_fwd(const float* part, int splitk, int B, const float* b1, const float* w2,
                        float* h1, float* pre2, int ngroups, hipStream_t st) {
  const int mtiles = (B + 15) / 16;
#define PDM_HID_FWD(NT, CH) \
  mlp_hid_fwd_kernel<NT, CH><<<mtiles * (2 / NT), 256, 0, st>>>(part, splitk, B, b1, w2, h1, pre2)
  if (ngroups == 2) {
    if (splitk == 1) PDM_HID_FWD(1, 1);
    else PDM_HID_FWD(1, 5);
  } else {
    if (splitk == 1) PDM_HID_FWD(2, 1);
    else PDM_HID_FWD(2, 5);
  }
#undef PDM_HID_FWD
}

void launch_mlp_hid_bwd(const float* dh2, const float* h1, const float* w2, int B, float* dh1,
                        float* gw2, hipStream_t st) {
  mlp_hid_bwd_kernel<<<2 * ((B + 15) / 16) + HB_DW, 256, 0, st>>>(dh2, h1, w2, B, dh1, gw2);
}
