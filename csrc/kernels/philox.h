// Philox4x32-10 (Salmon et al., Random123): the counter-based generator behind every random
// draw of the device code -- the augmenting gather (augment.hip, counter (index, epoch, 0, 0)),
// the dropout head (cnn_head_drop.hip, counter (index, epoch, 1, unit >> 3)), the elastic
// gather's control points (augment.hip, counter (index, epoch, 2, point)) and the mixup pairs
// (kernels/mixup.h, counter (index, epoch, 3, 0)).  The CPU twin
// is data/augment.py philox4x32_10; tests/test_augment_cpu.py pins it to the Random123 vectors.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t (&r)[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}
