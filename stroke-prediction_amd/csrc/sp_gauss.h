// Weights of scipy.ndimage.gaussian_filter, shared by the per-volume filter (sp_transform.hip) and the batched one
// (sp_augment.hip): both must multiply by the very same floats for their results to be equal bit for bit.
#pragma once
#include <math.h>

#define SP_GAUSS_MAX_RADIUS 64

struct GaussW {
  float w[2 * SP_GAUSS_MAX_RADIUS + 1];
};

// radius = int(truncate * sigma + 0.5); weights exp(-x^2 / (2 sigma^2)) normalised to sum 1, computed in double.
// Returns the radius (the caller checks it against SP_GAUSS_MAX_RADIUS BEFORE calling).
static inline int sp_gauss_radius(float sigma, float truncate) { return (int)(truncate * sigma + 0.5f); }
static inline void sp_gauss_weights(float sigma, int radius, GaussW* gw) {
  double sum = 0.0, wd[2 * SP_GAUSS_MAX_RADIUS + 1];
  for (int t = -radius; t <= radius; ++t) { wd[t + radius] = exp(-0.5 * (double)t * t / ((double)sigma * sigma)); sum += wd[t + radius]; }
  for (int t = 0; t <= 2 * radius; ++t) gw->w[t] = (float)(wd[t] / sum);
}
