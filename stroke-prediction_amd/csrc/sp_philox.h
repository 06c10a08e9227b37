// Philox4x32-10, the counter-based generator of the batch augmentation: shared by the uniform noise of the elastic deformation
// (sp_augment.hip) and the normal noise of the intensity augmentation (sp_intensity.hip) -- both must run the very same rounds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Salmon et al., "Parallel random numbers: as easy as 1, 2, 3" (SC11).  Counter (c0, c1, c2, c3), key (k0, k1) -> four words.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
