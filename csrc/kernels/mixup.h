// The mixup draw (--mixup; docs/kernels.md "Mixup"; the CPU twin and oracle is data/mixup.py):
// for the sample with dataset index i in epoch e, Philox4x32-10 with counter (i, e, 3, 0) and
// key (mixup seed lo, hi) gives the partner j = (r0 * N) >> 32 (any of the N training samples)
// and the blend weight q = QT[r1 >> 22] (QT int32 [1024], 128..256; lambda = q / 256).  One
// device function for the epoch gather (augment.hip), the head and the observer
// (cnn_head_mix.hip), so the image and its target are mixed by the same pair.
#pragma once
#include "philox.h"

// N >= 1.  j < N by construction; the caller guarantees that N rows can be read.
__device__ __forceinline__ void mixup_draw(uint32_t index, uint32_t epoch, uint32_t k0, uint32_t k1,
                                           uint32_t N, const int32_t* __restrict__ QT, int& j,
                                           int& q) {
  uint32_t r[4];
  philox4x32_10(index, epoch, 3u, 0u, k0, k1, r);
  j = (int)__umulhi(r[0], N);
  q = QT[r[1] >> 22];
}
