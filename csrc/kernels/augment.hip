// Train-time augmentation inside the epoch gather: gather_epoch (data.hip) with every image
// shifted, rotated and zoomed on its way into the epoch buffer.  The step kernels read the
// buffer as before, so augmentation adds nothing to the step chain.
//
// The transform is integer-only (docs/kernels.md "Augmenting gather"; the CPU twin and oracle
// is data/augment.py): a sample's draw depends on (seed, epoch, dataset index) alone --
// Philox4x32-10, counter (index, epoch, 0, 0), key (seed lo, seed hi) -- the angle and zoom
// levels index Q14 tables the host computed in fp64, and the inverse map and the bilinear
// blend are exact int32 arithmetic, so GPU and CPU agree bit for bit.
//
// Layout: a wave owns 16 rows of a 64-row workgroup pass.  Its lanes 0..15 read the rows'
// sampler indices (in place from the pinned host buffer, as gather_epoch), copy the labels
// and do the per-image work once: the Philox draw, the three table reads, A, B, dx, dy.  The
// wave then takes the images one at a time, the parameters broadcast by lane reads (scalars),
// lane c < 49 producing the 16 output pixels of chunk c and storing them as 16 bytes.
// No LDS at all: cnn_bwd leaves 640 of a CU's 163,840 LDS bytes, so any staging carve would
// keep cnn_bwd off the CU while a gather workgroup is resident; the four source bytes of a
// pixel are read through L1 instead (one image's 784 bytes are 7 or 8 cache lines, shared
// by the wave's 49 lanes).  The waves never synchronise with each other.
#include "common.h"
#include "kernels.h"
#include "philox.h"

namespace {

constexpr int AR = 64;                 // rows per workgroup pass (gather_epoch's GR)
constexpr int AW = AR / 4;             // rows per wave
constexpr int A_CHUNKS = 784 / 16;     // 49 16-B chunks per image

__global__ __launch_bounds__(256) void gather_epoch_augment_kernel(
    const uint8_t* __restrict__ images, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ idx, int n, int nimg, uint8_t* __restrict__ out_images,
    int32_t* __restrict__ out_labels, int64_t* __restrict__ ctr, int nctr,
    int64_t* __restrict__ step, int64_t step_value, const int32_t* __restrict__ cosq,
    const int32_t* __restrict__ sinq, const int32_t* __restrict__ invz, int shift, uint32_t epoch,
    uint32_t key0, uint32_t key1) {
  if (blockIdx.x == 0 && threadIdx.x < nctr) ctr[threadIdx.x] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0 && step != nullptr) *step = step_value;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t span = 2u * (uint32_t)shift + 1u;
  // a grid smaller than the row count strides over the rest
  for (int r0 = blockIdx.x * AR + wave * AW; r0 < n; r0 += gridDim.x * AR) {
    const int nr = min(AW, n - r0);
    // per-image work, once: lane i < nr holds image r0 + i's source row and transform
    int p_src = 0, p_a = 16384, p_b = 0, p_ox = 3456, p_oy = 3456;
    if (lane < nr) {
      const int src_u = idx[r0 + lane];
      PDM_CHECK(src_u >= 0 && src_u < nimg, "gather_epoch_augment index", src_u, nimg);
      p_src = min(max(src_u, 0), nimg - 1);   // (a bad host index reads a valid row)
      out_labels[r0 + lane] = labels[p_src];
      uint32_t r[4];
      philox4x32_10((uint32_t)p_src, epoch, 0u, 0u, key0, key1, r);
      const int k = (int)(r[0] >> 22), j = (int)(r[1] >> 26);
      const int iz = invz[j];
      p_a = (cosq[k] * iz + 8192) >> 14;
      p_b = (sinq[k] * iz + 8192) >> 14;
      p_ox = 3456 - 256 * ((int)(r[2] % span) - shift);
      p_oy = 3456 - 256 * ((int)(r[3] % span) - shift);
    }
    for (int i = 0; i < nr; ++i) {
      const int src = __builtin_amdgcn_readlane(p_src, i);
      const int A = __builtin_amdgcn_readlane(p_a, i), B = __builtin_amdgcn_readlane(p_b, i);
      const int ox = __builtin_amdgcn_readlane(p_ox, i), oy = __builtin_amdgcn_readlane(p_oy, i);
      if (lane < A_CHUNKS) {
        const uint8_t* __restrict__ img = images + (int64_t)src * 784;
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          uint32_t word = 0;
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const int pix = 16 * lane + 4 * q + b, y = pix / 28, x = pix - 28 * y;
            const int u = 2 * x - 27, v = 2 * y - 27;
            const int sx = ((A * u + B * v + 64) >> 7) + ox;     // source x, 1/256 px
            const int sy = ((-B * u + A * v + 64) >> 7) + oy;
            const int x0 = sx >> 8, fx = sx & 255, y0 = sy >> 8, fy = sy & 255;
            // zero outside the image: the load is clamped to a valid byte and masked
            const bool cx0 = (unsigned)x0 < 28u, cx1 = (unsigned)(x0 + 1) < 28u;
            const bool cy0 = (unsigned)y0 < 28u, cy1 = (unsigned)(y0 + 1) < 28u;
            const int xa = cx0 ? x0 : 0, xb = cx1 ? x0 + 1 : 0;
            const int ya = cy0 ? y0 * 28 : 0, yb = cy1 ? (y0 + 1) * 28 : 0;
            const int p00 = (cx0 && cy0) ? (int)img[ya + xa] : 0;
            const int p10 = (cx1 && cy0) ? (int)img[ya + xb] : 0;
            const int p01 = (cx0 && cy1) ? (int)img[yb + xa] : 0;
            const int p11 = (cx1 && cy1) ? (int)img[yb + xb] : 0;
            const int o = ((256 - fx) * (256 - fy) * p00 + fx * (256 - fy) * p10 +
                           (256 - fx) * fy * p01 + fx * fy * p11 + 32768) >> 16;
            word |= (uint32_t)o << (8 * b);
          }
          w[q] = word;
        }
        reinterpret_cast<uint4*>(out_images + (int64_t)(r0 + i) * 784)[lane] =
            make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
  }
}

}  // namespace

void launch_gather_epoch_augment(const uint8_t* images, const int32_t* labels, const int32_t* idx,
                                 int n, int nimg, uint8_t* out_images, int32_t* out_labels,
                                 int64_t* ctr, int nctr, int64_t* step, int64_t step_value,
                                 int max_wgs, const int32_t* cosq, const int32_t* sinq,
                                 const int32_t* invz, int shift, uint32_t epoch, uint64_t seed,
                                 hipStream_t st) {
  if (n <= 0 && nctr == 0 && step == nullptr) return;
  int grid = max((n + AR - 1) / AR, 1);
  if (max_wgs > 0 && grid > max_wgs) grid = max_wgs;
  gather_epoch_augment_kernel<<<grid, 256, 0, st>>>(
      images, labels, idx, n, nimg, out_images, out_labels, ctr, nctr, step, step_value, cosq,
      sinq, invz, shift, epoch, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
}
