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
//
// gather_epoch_elastic_kernel, further down, is the same gather with an elastic distortion
// added to the inverse map (--aug-elastic); gather_epoch_mixup_kernel, below that, is the
// elastic gather reading every source byte as a blend of two images (--mixup).
#include "common.h"
#include "kernels.h"
#include "philox.h"
#include "mixup.h"

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

// The elastic twin (--aug-elastic): the kernel above with a smooth per-image displacement
// (ex, ey) added to the source coordinate -- a uniform quadratic B-spline over a 6 x 6 grid of
// control displacements at a spacing of 8 pixels, exact in integers (docs/kernels.md "Elastic
// gather").  It is a twin and not a template instance so that the kernel above compiles to
// exactly what it did before this one existed; the lines they share are kept identical.
//
// A blurred per-pixel field would need LDS staging, which the zero-LDS rule at the top of the
// file rules out.  Instead, per image, lane q < 36 draws control point q = 6 cy + cx (Philox
// counter (index, epoch, 2, q)) into one register, (gx, gy) as two int16, and the pixel lanes
// fetch their 3 x 3 neighbourhood across lanes with ds_bpermute: the source lane depends on the
// reading lane's pixel, which neither DPP's fixed patterns nor a scalar lane read can express;
// the instruction goes through the LDS crossbar but allocates no LDS.  elastic_q is the
// displacements' range in 1/256 px (0..768); 0 reproduces the kernel above bit for bit.
constexpr int ELASTIC_POINTS = 36;

__global__ __launch_bounds__(256) void gather_epoch_elastic_kernel(
    const uint8_t* __restrict__ images, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ idx, int n, int nimg, uint8_t* __restrict__ out_images,
    int32_t* __restrict__ out_labels, int64_t* __restrict__ ctr, int nctr,
    int64_t* __restrict__ step, int64_t step_value, const int32_t* __restrict__ cosq,
    const int32_t* __restrict__ sinq, const int32_t* __restrict__ invz, int shift, uint32_t epoch,
    uint32_t key0, uint32_t key1, int elastic_q) {
  if (blockIdx.x == 0 && threadIdx.x < nctr) ctr[threadIdx.x] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0 && step != nullptr) *step = step_value;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t span = 2u * (uint32_t)shift + 1u;
  const uint32_t span_e = 2u * (uint32_t)elastic_q + 1u;
  // a grid smaller than the row count strides over the rest
  for (int r0 = blockIdx.x * AR + wave * AW; r0 < n; r0 += gridDim.x * AR) {
    const int nr = min(AW, n - r0);
    // per-image work, once: lane i < nr holds image r0 + i's source row and transform
    int p_src = 0, p_a = 16384, p_b = 0, p_ox = 3456, p_oy = 3456;
    if (lane < nr) {
      const int src_u = idx[r0 + lane];
      PDM_CHECK(src_u >= 0 && src_u < nimg, "gather_epoch_elastic index", src_u, nimg);
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
      // the image's control displacements: lane q draws point q, one Philox call each.  Every
      // lane of the wave runs this (lanes 36..63 hold words that nobody reads).
      uint32_t rc[4];
      philox4x32_10((uint32_t)src, epoch, 2u, (uint32_t)lane, key0, key1, rc);
      const int gx = (int)(((rc[0] >> 16) * span_e) >> 16) - elastic_q;
      const int gy = (int)(((rc[1] >> 16) * span_e) >> 16) - elastic_q;
      const int ctl = (gx & 0xffff) | (gy << 16);
      if (lane < A_CHUNKS) {
        const uint8_t* __restrict__ img = images + (int64_t)src * 784;
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          uint32_t word = 0;
          // The four pixels of a group lie in one image row and one 8-pixel cell (28 and 8 are
          // multiples of 4), so they share their 3 x 3 control points: 9 cross-lane reads per
          // group, and the y-weights are applied once per group,
          // vx[a] = sum_b wy[b] gx[6 (cy0 + b) + cx0 + a]   (|vx| <= 512 * 768).
          // A cross-lane read of an inactive lane returns 0, not that lane's value.  The source
          // lanes 0..35 are active here because this branch holds lanes 0..48 (asserted
          // below): keep these reads inside it or outside any branch, never under a narrower
          // one.
          static_assert(ELASTIC_POINTS <= A_CHUNKS, "the control lanes must be active here");
          const int pix0 = 16 * lane + 4 * q, yq = pix0 / 28, xq = pix0 - 28 * yq;
          const int g = 2 * (yq & 7) + 1, f0 = 2 * (xq & 7) + 1;
          const int base = 6 * (yq >> 3) + (xq >> 3);        // <= 21: base + 14 <= 35
          const int wy[3] = {(16 - g) * (16 - g), 256 + 32 * g - 2 * g * g, g * g};
          int vx[3] = {0, 0, 0}, vy[3] = {0, 0, 0};
#pragma unroll
          for (int bb = 0; bb < 3; ++bb) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
              const int c = __builtin_amdgcn_ds_bpermute(4 * (base + 6 * bb + a), ctl);
              vx[a] += wy[bb] * ((c << 16) >> 16);
              vy[a] += wy[bb] * (c >> 16);
            }
          }
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const int pix = 16 * lane + 4 * q + b, y = pix / 28, x = pix - 28 * y;
            const int u = 2 * x - 27, v = 2 * y - 27;
            const int f = f0 + 2 * b;                            // 2 (x & 7) + 1
            const int wx0 = (16 - f) * (16 - f), wx1 = 256 + 32 * f - 2 * f * f, wx2 = f * f;
            const int ex = (wx0 * vx[0] + wx1 * vx[1] + wx2 * vx[2] + (1 << 17)) >> 18;
            const int ey = (wx0 * vy[0] + wx1 * vy[1] + wx2 * vy[2] + (1 << 17)) >> 18;
            const int sx = ((A * u + B * v + 64) >> 7) + ox + ex;     // source x, 1/256 px
            const int sy = ((-B * u + A * v + 64) >> 7) + oy + ey;
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

// The mixup twin (--mixup): the elastic kernel above with every source byte replaced by the
// blend m = (q a + (256 - q) b + 128) >> 8 of image `src` (a) and its partner j (b), both read at
// the same tap; the geometric transform is src's (docs/kernels.md "Mixup"; data/mixup.py).  Lanes
// < nr draw (j, q) with their other per-image work (kernels/mixup.h: Philox counter (index,
// epoch, 3, 0), key (mk0, mk1)); both are broadcast by lane reads, like p_src.  A twin again, not a
// template instance, and the shared lines kept identical.  QT == 256 everywhere reproduces the
// elastic kernel bit for bit ((256 a + 128) >> 8 = a); zero ranges and elastic_q = 0 give the
// plain mixed gather.  ntrain (1..nimg) is the number of samples a partner is drawn from.
__global__ __launch_bounds__(256) void gather_epoch_mixup_kernel(
    const uint8_t* __restrict__ images, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ idx, int n, int nimg, uint8_t* __restrict__ out_images,
    int32_t* __restrict__ out_labels, int64_t* __restrict__ ctr, int nctr,
    int64_t* __restrict__ step, int64_t step_value, const int32_t* __restrict__ cosq,
    const int32_t* __restrict__ sinq, const int32_t* __restrict__ invz, int shift, uint32_t epoch,
    uint32_t key0, uint32_t key1, int elastic_q, const int32_t* __restrict__ qt, uint32_t ntrain,
    uint32_t mk0, uint32_t mk1) {
  if (blockIdx.x == 0 && threadIdx.x < nctr) ctr[threadIdx.x] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0 && step != nullptr) *step = step_value;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t span = 2u * (uint32_t)shift + 1u;
  const uint32_t span_e = 2u * (uint32_t)elastic_q + 1u;
  // a grid smaller than the row count strides over the rest
  for (int r0 = blockIdx.x * AR + wave * AW; r0 < n; r0 += gridDim.x * AR) {
    const int nr = min(AW, n - r0);
    // per-image work, once: lane i < nr holds image r0 + i's source row and transform
    int p_src = 0, p_a = 16384, p_b = 0, p_ox = 3456, p_oy = 3456;
    int p_j = 0, p_q = 256;               // and its partner's row and the blend weight
    if (lane < nr) {
      const int src_u = idx[r0 + lane];
      PDM_CHECK(src_u >= 0 && src_u < nimg, "gather_epoch_mixup index", src_u, nimg);
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
      mixup_draw((uint32_t)p_src, epoch, mk0, mk1, ntrain, qt, p_j, p_q);
      p_j = min(p_j, nimg - 1);               // (j < ntrain <= nimg: a backstop, as p_src's)
    }
    for (int i = 0; i < nr; ++i) {
      const int src = __builtin_amdgcn_readlane(p_src, i);
      const int A = __builtin_amdgcn_readlane(p_a, i), B = __builtin_amdgcn_readlane(p_b, i);
      const int ox = __builtin_amdgcn_readlane(p_ox, i), oy = __builtin_amdgcn_readlane(p_oy, i);
      const int src2 = __builtin_amdgcn_readlane(p_j, i);
      const int mq = __builtin_amdgcn_readlane(p_q, i), mr = 256 - mq;
      // the image's control displacements: lane q draws point q, one Philox call each.  Every
      // lane of the wave runs this (lanes 36..63 hold words that nobody reads).
      uint32_t rc[4];
      philox4x32_10((uint32_t)src, epoch, 2u, (uint32_t)lane, key0, key1, rc);
      const int gx = (int)(((rc[0] >> 16) * span_e) >> 16) - elastic_q;
      const int gy = (int)(((rc[1] >> 16) * span_e) >> 16) - elastic_q;
      const int ctl = (gx & 0xffff) | (gy << 16);
      if (lane < A_CHUNKS) {
        const uint8_t* __restrict__ img = images + (int64_t)src * 784;
        const uint8_t* __restrict__ img2 = images + (int64_t)src2 * 784;
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          uint32_t word = 0;
          // (the elastic kernel's group scheme: 9 cross-lane reads per group of four pixels;
          // the source lanes 0..35 are active because this branch holds lanes 0..48)
          const int pix0 = 16 * lane + 4 * q, yq = pix0 / 28, xq = pix0 - 28 * yq;
          const int g = 2 * (yq & 7) + 1, f0 = 2 * (xq & 7) + 1;
          const int base = 6 * (yq >> 3) + (xq >> 3);        // <= 21: base + 14 <= 35
          const int wy[3] = {(16 - g) * (16 - g), 256 + 32 * g - 2 * g * g, g * g};
          int vx[3] = {0, 0, 0}, vy[3] = {0, 0, 0};
#pragma unroll
          for (int bb = 0; bb < 3; ++bb) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
              const int c = __builtin_amdgcn_ds_bpermute(4 * (base + 6 * bb + a), ctl);
              vx[a] += wy[bb] * ((c << 16) >> 16);
              vy[a] += wy[bb] * (c >> 16);
            }
          }
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const int pix = 16 * lane + 4 * q + b, y = pix / 28, x = pix - 28 * y;
            const int u = 2 * x - 27, v = 2 * y - 27;
            const int f = f0 + 2 * b;                            // 2 (x & 7) + 1
            const int wx0 = (16 - f) * (16 - f), wx1 = 256 + 32 * f - 2 * f * f, wx2 = f * f;
            const int ex = (wx0 * vx[0] + wx1 * vx[1] + wx2 * vx[2] + (1 << 17)) >> 18;
            const int ey = (wx0 * vy[0] + wx1 * vy[1] + wx2 * vy[2] + (1 << 17)) >> 18;
            const int sx = ((A * u + B * v + 64) >> 7) + ox + ex;     // source x, 1/256 px
            const int sy = ((-B * u + A * v + 64) >> 7) + oy + ey;
            const int x0 = sx >> 8, fx = sx & 255, y0 = sy >> 8, fy = sy & 255;
            // zero outside the image: the load is clamped to a valid byte and masked
            const bool cx0 = (unsigned)x0 < 28u, cx1 = (unsigned)(x0 + 1) < 28u;
            const bool cy0 = (unsigned)y0 < 28u, cy1 = (unsigned)(y0 + 1) < 28u;
            const int xa = cx0 ? x0 : 0, xb = cx1 ? x0 + 1 : 0;
            const int ya = cy0 ? y0 * 28 : 0, yb = cy1 ? (y0 + 1) * 28 : 0;
            // each tap: two bytes, blended (at most (256 * 255 + 128) >> 8 = 255)
            const int p00 = (cx0 && cy0) ? (mq * (int)img[ya + xa] + mr * (int)img2[ya + xa] + 128) >> 8 : 0;
            const int p10 = (cx1 && cy0) ? (mq * (int)img[ya + xb] + mr * (int)img2[ya + xb] + 128) >> 8 : 0;
            const int p01 = (cx0 && cy1) ? (mq * (int)img[yb + xa] + mr * (int)img2[yb + xa] + 128) >> 8 : 0;
            const int p11 = (cx1 && cy1) ? (mq * (int)img[yb + xb] + mr * (int)img2[yb + xb] + 128) >> 8 : 0;
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

void launch_gather_epoch_mixup(const uint8_t* images, const int32_t* labels, const int32_t* idx,
                               int n, int nimg, uint8_t* out_images, int32_t* out_labels,
                               int64_t* ctr, int nctr, int64_t* step, int64_t step_value,
                               int max_wgs, const int32_t* cosq, const int32_t* sinq,
                               const int32_t* invz, int shift, uint32_t epoch, uint64_t seed,
                               int elastic_q, const int32_t* qt, int ntrain, uint64_t mixup_seed,
                               hipStream_t st) {
  if (n <= 0 && nctr == 0 && step == nullptr) return;
  int grid = max((n + AR - 1) / AR, 1);
  if (max_wgs > 0 && grid > max_wgs) grid = max_wgs;
  gather_epoch_mixup_kernel<<<grid, 256, 0, st>>>(
      images, labels, idx, n, nimg, out_images, out_labels, ctr, nctr, step, step_value, cosq,
      sinq, invz, shift, epoch, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32),
      elastic_q, qt, (uint32_t)ntrain, (uint32_t)(mixup_seed & 0xffffffffu),
      (uint32_t)(mixup_seed >> 32));
}

void launch_gather_epoch_elastic(const uint8_t* images, const int32_t* labels, const int32_t* idx,
                                 int n, int nimg, uint8_t* out_images, int32_t* out_labels,
                                 int64_t* ctr, int nctr, int64_t* step, int64_t step_value,
                                 int max_wgs, const int32_t* cosq, const int32_t* sinq,
                                 const int32_t* invz, int shift, uint32_t epoch, uint64_t seed,
                                 int elastic_q, hipStream_t st) {
  if (n <= 0 && nctr == 0 && step == nullptr) return;
  int grid = max((n + AR - 1) / AR, 1);
  if (max_wgs > 0 && grid > max_wgs) grid = max_wgs;
  gather_epoch_elastic_kernel<<<grid, 256, 0, st>>>(
      images, labels, idx, n, nimg, out_images, out_labels, ctr, nctr, step, step_value, cosq,
      sinq, invz, shift, epoch, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32),
      elastic_q);
}

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
