// Adversarial evaluation of the hidden-layer MLP (--arch mlp, --attack-eps): one FGSM / PGD step
// on the raw uint8 image, the backward direction of fc1 that training never needs,
//
//   g[b][px] = d(-log_softmax(logits(x_b))[y_b]) / d(normalised pixel) = sum_n dh[b][n] W1[n][px]
//   out      = clamp(x + alpha sign(g), max(0, x0 - eps), min(255, x0 + eps))       sign(0) = 0
//
// in grey levels (the normalisation a u8 - b has a > 0: the sign with respect to the byte is the
// sign above).  One iteration is mlp_fwd on the iterate x, then this kernel on its [S][B][128]
// partials.  Workgroup = (m-tile of 16 rows, pixel block), 4 waves, two phases:
//
//   1  the head's arithmetic for the 16 rows without any of its side effects (no counters, no
//      metrics, no schedule cursor): wave w takes rows w, w + 4, w + 8, w + 12, lane j hidden
//      units 2 j, 2 j + 1 as cnn_head_body.h does -- h = relu(b1 + sum_s part[s]) with the bias
//      first and the splits in order (the ReLU mask is the one predict() sees), the logits as
//      DPP wave sums, softmax, dl = p - onehot(y) (per sample, no 1 / B) and dh = [h > 0] dl . W2
//      into an LDS tile [16][136] fp32.  Every wave then takes ALL of dh as its MFMA B operand,
//      split in registers into three bf16 parts (hi, mid, lo: all 24 bits, as mlp_bwd).
//   2  dX = dh . W1 on v_mfma_f32_16x16x32_bf16 with k = hidden unit.  W1's two bf16 planes are
//      [128][784], laid out for the forward (k = pixel): here the 8 k-values of one pixel lie
//      1568 B apart.  A round's [128 units][112 pixels] of both planes are therefore copied to
//      LDS as they are (16-B pieces, 14 per thread, in flight across phase 1; the LDS image is
//      contiguous: pitch 224 B) and the A fragments come out of ds_read_b64_tr_b16, which hands
//      lane i16 column i16 of four rows: W1 is the A operand with m = pixel, dh the B operand
//      with n = image row, so a lane's D fragment is 4 consecutive pixels of one image and the
//      epilogue is one 4-B load of x and x0, the integer rule and one 4-B store (and, asked for,
//      one 16-B store of the fp32 gradient).  The seven 16-pixel tiles of a round go to waves
//      t % 4; a workgroup walks `rounds` rounds (1: seven pixel blocks per m-tile, 7: one).
//
// k assignment (free as long as A and B agree): slot j of lane group g in step ks is hidden unit
// 32 ks + 4 g + j (j < 4) and 32 ks + 16 + 4 g + j - 4, so the 32 lanes of one LDS pass read
// eight CONSECUTIVE rows.  tools/lds_bank_model.py mlp_attack: at pitch 224 B = 56 dwords (-8 mod
// 64) their 8-dword windows tile the 64 banks, 1.00; the usual 8 g + j rows give 2.00 at every
// 16-B pitch (rows 0 and 8 are 8 * 56 dwords apart: the same banks).  The dh tile's b128 reads
// are 1.00 at pitch 136 dwords (mlp_hid_fwd's layout).
//
// Six MFMAs per k-step: (hi, mid, lo of dh) x (hi, lo of W1), smallest terms first; every
// product is exact, the accumulation is in a fixed order, there are no atomics: the output is
// bit-reproducible.  Rows >= B read clamped addresses, enter as zeros and store nothing.
#include "cnn_common.h"

namespace {

using namespace cnn;

constexpr int AT_K = MLP_IN;                           // 784 pixels
constexpr int AT_TILES = 7, AT_PX = 16 * AT_TILES;     // a round: 7 tiles of 16 pixels
constexpr int AT_ROUNDS = AT_K / AT_PX;                // 7 rounds cover the image
constexpr int AT_PITCH = 2 * AT_PX;                    // 224 B: a hidden unit's pixels of a round
constexpr int AT_PLANE = HID * AT_PITCH;               // 28672 B per plane
constexpr int AT_ROW16 = AT_PITCH / 16;                // 14 16-B pieces per row
constexpr int AT_PIECES = 2 * AT_PLANE / 16 / 256;     // 14 pieces per thread
constexpr int AT_DHP = 136;                            // dh tile pitch, dwords
static_assert(AT_ROUNDS * AT_PX == AT_K && AT_PIECES * 256 * 16 == 2 * AT_PLANE && HID == 128,
              "mlp_attack geometry");
static_assert(16 * AT_DHP * 4 <= 2 * AT_PLANE, "the dh tile lives where the W1 tile goes later");

__device__ __forceinline__ f32x4 mfma(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

template <int S>
__global__ __launch_bounds__(256) void mlp_attack_kernel(
    const float* __restrict__ part, int B, const int32_t* __restrict__ ylab,
    const float* __restrict__ bf1, const float* __restrict__ wf2, const float* __restrict__ bf2,
    const bf16* __restrict__ whi, const bf16* __restrict__ wlo, const uint8_t* __restrict__ x0,
    const uint8_t* __restrict__ x, uint8_t* __restrict__ out, float* __restrict__ grad, int eps,
    int alpha, int rounds) {
  constexpr int CH = S < 5 ? S : 5;                    // partial loads in flight per batch
  __shared__ __attribute__((aligned(16))) char sm[2 * AT_PLANE];
  float* dhs = reinterpret_cast<float*>(sm);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i16 = lane & 15, q = i16 >> 2, pq = i16 & 3;
  const int mtiles = (B + 15) / 16;
  const int mtile = blockIdx.x % mtiles, pb = blockIdx.x / mtiles;

  // a round's W1 tile: piece i = tid + 256 u of [plane][unit][14 pieces], LDS byte 16 i
  u32x4 wv[AT_PIECES];
  auto wload = [&](int rd) __attribute__((always_inline)) {
    const int col = (pb * rounds + rd) * AT_PX;
    static_for<AT_PIECES>([&](auto U) __attribute__((always_inline)) {
      constexpr int u = decltype(U)::value;
      const int i = tid + 256 * u;
      const int lo = i >= HID * AT_ROW16, rem = i - lo * HID * AT_ROW16;
      const int n = rem / AT_ROW16, c = rem - n * AT_ROW16;
      wv[u] = *reinterpret_cast<const u32x4*>((lo ? wlo : whi) + n * AT_K + col + 8 * c);
    });
  };
  wload(0);

  // ---- phase 1: dh of the m-tile's 16 rows (cnn_head_body.h's operations in their order) ----
  {
    const float2 bias = reinterpret_cast<const float2*>(bf1)[lane];
    float2 w2v[NCLS];
#pragma unroll
    for (int c = 0; c < NCLS; ++c) w2v[c] = reinterpret_cast<const float2*>(wf2 + c * HID)[lane];
    for (int i = 0; i < 4; ++i) {
      const int rl = wave + 4 * i, row = mtile * 16 + rl;
      const bool valid = row < B;
      const int rc = min(row, B - 1);
      const int y = ylab[rc];
      float2 h = bias;
#pragma unroll
      for (int s0 = 0; s0 < S; s0 += CH) {
        float2 u[CH];
#pragma unroll
        for (int k = 0; k < CH; ++k)
          u[k] = *reinterpret_cast<const float2*>(part + ((int64_t)(s0 + k) * B + rc) * HID + 2 * lane);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < CH; ++k) {
          h.x += u[k].x;
          h.y += u[k].y;
        }
      }
      h.x = valid ? fmaxf(h.x, 0.f) : 0.f;
      h.y = valid ? fmaxf(h.y, 0.f) : 0.f;
      float lg[NCLS], prob[NCLS];
#pragma unroll
      for (int c = 0; c < NCLS; ++c) lg[c] = wave_sum_dpp(fmaf(h.y, w2v[c].y, h.x * w2v[c].x)) + bf2[c];
      int correct;
      row_xent<NCLS>(lg, y, prob, correct);
      float2 dhv = make_float2(0.f, 0.f);
#pragma unroll
      for (int c = 0; c < NCLS; ++c) {
        const float dl = prob[c] - (c == y ? 1.f : 0.f);
        dhv.x = fmaf(dl, w2v[c].x, dhv.x);
        dhv.y = fmaf(dl, w2v[c].y, dhv.y);
      }
      dhv.x = h.x > 0.f ? dhv.x : 0.f;     // (h is 0 in rows >= B)
      dhv.y = h.y > 0.f ? dhv.y : 0.f;
      reinterpret_cast<float2*>(dhs + rl * AT_DHP)[lane] = dhv;
    }
  }
  __syncthreads();
  // the B fragments of all four k-steps: image row i16, the lane group's 8 hidden units
  bf16x8 bh[4], bm[4], bl[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const float* p = dhs + i16 * AT_DHP + 32 * ks + 4 * g;
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(p), v1 = *reinterpret_cast<const f32x4*>(p + 16);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = j < 4 ? v0[j & 3] : v1[j & 3];
      bh[ks][j] = to_bf16(v);
      const float r1 = v - from_bf16(bh[ks][j]);       // (both remainders are exact in fp32)
      bm[ks][j] = to_bf16(r1);
      bl[ks][j] = to_bf16(r1 - from_bf16(bm[ks][j]));
    }
  }

  // ---- phase 2: the rounds of 112 pixels ----
  const int b = mtile * 16 + i16;
  for (int rd = 0; rd < rounds; ++rd) {
    __syncthreads();   // the dh tile / the previous round's W1 tile has been read
    static_for<AT_PIECES>([&](auto U) __attribute__((always_inline)) {
      constexpr int u = decltype(U)::value;
      *reinterpret_cast<u32x4*>(sm + 16 * (tid + 256 * u)) = wv[u];
    });
    __syncthreads();
    if (rd + 1 < rounds) wload(rd + 1);
    const int col = (pb * rounds + rd) * AT_PX;
    for (int t = wave; t < AT_TILES; t += 4) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        // lane 4 q + pq of a group: row (unit) 32 ks + 4 g + q, pixels 16 t + 4 pq .. + 3
        const char* a0 = sm + (32 * ks + 4 * g + q) * AT_PITCH + 32 * t + 8 * pq;
        const bf16x8 ah = cat_tr(lds_tr16(a0), lds_tr16(a0 + 16 * AT_PITCH));
        const bf16x8 al = cat_tr(lds_tr16(a0 + AT_PLANE), lds_tr16(a0 + AT_PLANE + 16 * AT_PITCH));
        acc = mfma(al, bl[ks], acc);   // small terms first
        acc = mfma(ah, bl[ks], acc);
        acc = mfma(al, bm[ks], acc);
        acc = mfma(ah, bm[ks], acc);
        acc = mfma(al, bh[ks], acc);
        acc = mfma(ah, bh[ks], acc);
      }
      // pixels col + 16 t + 4 g .. + 3 of image row b
      if (b < B) {
        const int64_t o = (int64_t)b * AT_K + col + 16 * t + 4 * g;
        const uint32_t xv = *reinterpret_cast<const uint32_t*>(x + o);
        const uint32_t cv = *reinterpret_cast<const uint32_t*>(x0 + o);
        uint32_t ov = 0u;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int xi = (int)((xv >> (8 * r)) & 0xffu), ci = (int)((cv >> (8 * r)) & 0xffu);
          const int sg = (acc[r] > 0.f) - (acc[r] < 0.f);
          const int v = min(max(xi + alpha * sg, max(ci - eps, 0)), min(ci + eps, 255));
          ov |= (uint32_t)v << (8 * r);
        }
        *reinterpret_cast<uint32_t*>(out + o) = ov;
        if (grad != nullptr) *reinterpret_cast<f32x4*>(grad + o) = acc;
      }
    }
  }
}

}  // namespace

void launch_mlp_attack(const float* part, int splitk, int B, const int32_t* ylab, const float* bf1,
                       const float* wf2, const float* bf2, const __bf16* whi, const __bf16* wlo,
                       const uint8_t* x0, const uint8_t* x, uint8_t* out, float* grad, int eps,
                       int alpha, int px_blocks, hipStream_t st) {
  if (px_blocks == 0) px_blocks = MLP_ATTACK_PX_BLOCKS;
  const int rounds = AT_ROUNDS / px_blocks;
  const int grid = (B + 15) / 16 * px_blocks;
  if (splitk == 25)
    mlp_attack_kernel<25><<<grid, 256, 0, st>>>(part, B, ylab, bf1, wf2, bf2, whi, wlo, x0, x, out,
                                                grad, eps, alpha, rounds);
  else if (splitk == 5)
    mlp_attack_kernel<5><<<grid, 256, 0, st>>>(part, B, ylab, bf1, wf2, bf2, whi, wlo, x0, x, out,
                                               grad, eps, alpha, rounds);
  else
    mlp_attack_kernel<1><<<grid, 256, 0, st>>>(part, B, ylab, bf1, wf2, bf2, whi, wlo, x0, x, out,
                                               grad, eps, alpha, rounds);
}
