// Exact squared Euclidean distance transform, separable: g <- min_j g[.., j, ..] + (i - j)^2 along each axis in turn.  Shared by
// the surface distances of the batch metrics (sp_transform.hip) and the signed distance maps of the SDM baseline (sp_sdm.hip).
// Seeds are 0 (background) and SP_SD_BIG; every squared distance is an exact integer in fp32 for extents below 2^12.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SP_SD_BIG 1.0e30f

// one axis: element (o, i, k) of an (outer, n, inner) view; the outer index may run over several volumes stored back to back
__device__ __forceinline__ void sp_edt_axis(const float* __restrict__ src, float* __restrict__ dst, int64_t total, int n,
                                            int64_t inner) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t k = idx % inner, oi = idx / inner;
  const int i = (int)(oi % n);
  const float* line = src + (oi - i) * inner + k;
  float best = SP_SD_BIG;
  for (int j = 0; j < n; ++j) {
    const float dj = (float)(i - j);
    best = fminf(best, fmaf(dj, dj, line[(int64_t)j * inner]));
  }
  dst[idx] = best;
}
