// The fused optimiser family (include/stroke_amd.h): Adam, AdamW, SGD with momentum and SGD-Nesterov on flat fp32 buffers, with
// global-norm gradient clipping folded into the update.
//   * sp_grad_sqnorm_partials: stage 1 of the norm -- workgroup b leaves the sum of g[i]^2 over its grid-stride slice in partials[b]
//     as a double (the square of an fp32 value is exact in a double).  No atomics; the order inside a workgroup is fixed: per-thread
//     serial, wave sum, the four waves in order through LDS.  So the norm has the same bits on every run (README "Reproducibility").
//   * sp_optim_step_flat: the update.  Hyper-parameters and the step count are read from device memory as adam_hyp_kernel
//     (sp_elem.hip) reads them, so a captured step follows the schedulers.  With clipping on, EVERY wave adds the npartials doubles in
//     one fixed order (all waves of all workgroups get the same bits), forms torch's coefficient min(1, max_norm / (norm + 1e-6)) and
//     folds it into the gradient scale: clipping costs one launch (stage 1) more than the unclipped step and no host read.
// The step is memory-bound (and launch-bound at the U-Net's 355 k parameters): 16-byte loads and stores where all the pointers are
// 16-byte aligned, an element path otherwise -- the per-tensor route of the optimisers passes pointers at arbitrary 4-byte offsets.
// The existing sp_adam_step_flat* kernels (sp_elem.hip) are untouched; kind SP_OPT_ADAM with clipping off repeats adam_hyp_kernel's
// roundings and gives its bits (opt_elem).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sp_common.h"

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define OPT_MAX_BLOCKS 2048         // workgroups of an update launch at most (8 per CU); the grid-stride loop takes the rest
#define OPT_MAX_PARTIALS 256        // workgroups of the norm's stage 1 at most

// ------------------------------------------------------------------------------------------------ squared norm, stage 1
template <bool VEC>
__global__ __launch_bounds__(256) void sqnorm_partials_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ partials,
                                                              int accumulate) {
  double s = 0.0;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, T = (int64_t)gridDim.x * 256;
  if (VEC) {
    const int64_t n4 = n >> 2;
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    for (int64_t i = t; i < n4; i += T) {
      const f32x4 a = g4[i];
      s += (double)a[0] * (double)a[0];
      s += (double)a[1] * (double)a[1];
      s += (double)a[2] * (double)a[2];
      s += (double)a[3] * (double)a[3];
    }
    const int64_t i = (n4 << 2) + t;      // the up to three elements behind the last whole vector
    if (i < n) s += (double)g[i] * (double)g[i];
  } else {
    for (int64_t i = t; i < n; i += T) s += (double)g[i] * (double)g[i];
  }
  __shared__ double red[4];
  const double w = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double b = ((red[0] + red[1]) + red[2]) + red[3];
    partials[blockIdx.x] = accumulate ? partials[blockIdx.x] + b : b;
  }
}

extern "C" int sp_grad_sqnorm_partials(const float* g, int64_t n, double* partials, int32_t npartials, int32_t accumulate,
                                       sp_stream_t stream) {
  SP_CHECK_ARG(g && partials && n > 0 && npartials >= 1 && npartials <= OPT_MAX_PARTIALS, "sp_grad_sqnorm_partials: bad arguments");
  // one workgroup per partial, also where n is small: every slot is (re)written by every call
  if (((uintptr_t)g & 15) == 0)
    hipLaunchKernelGGL(sqnorm_partials_kernel<true>, dim3(npartials), dim3(256), 0, ST(stream), g, n, partials, (int)accumulate);
  else
    hipLaunchKernelGGL(sqnorm_partials_kernel<false>, dim3(npartials), dim3(256), 0, ST(stream), g, n, partials, (int)accumulate);
  SP_CHECK_LAUNCH("sp_grad_sqnorm_partials");
  return SP_OK;
}

// ------------------------------------------------------------------------------------------------ the update
// hyper = {lr, beta1, beta2, eps, weight_decay, max_norm, momentum, -}
struct OptCoef {
  float scale;                                   // grad_scale * clip coefficient
  float lr, wd, momentum;
  float beta1, beta2, eps, lr_over_bc1, inv_sqrt_bc2;
  float decay;                                   // AdamW: 1 - lr * wd
};

// One element.  Contraction is switched off and every fused multiply-add is written out: the element path, the 16-byte path and
// the tail then round alike (hipcc contracts them differently when left to itself), and the Adam moments repeat what
// adam_hyp_kernel (sp_elem.hip) compiles to -- gi and m as one fma each, v and the final division unfused -- which is what makes
// kind ADAM with clipping off equal sp_adam_step_flat_hyp bit for bit (tests/test_gpu_optim.py holds the two against each other).
template <int KIND>
__device__ __forceinline__ void opt_elem(float& p, const float g, float& m, float& v, const OptCoef& c) {
#pragma clang fp contract(off)
  if (KIND == SP_OPT_ADAM || KIND == SP_OPT_ADAMW) {
    // ADAM: gi += wd * p (torch.optim.Adam); ADAMW: p *= 1 - lr * wd first, then Adam without the L2 term (torch.optim.AdamW)
    const float pi = KIND == SP_OPT_ADAMW ? p * c.decay : p;
    const float gi = KIND == SP_OPT_ADAMW ? g * c.scale : __builtin_fmaf(c.wd, pi, g * c.scale);
    const float mi = __builtin_fmaf(1.f - c.beta1, gi, c.beta1 * m);
    const float vi = c.beta2 * v + ((1.f - c.beta2) * gi) * gi;
    m = mi; v = vi;
    p = pi - (c.lr_over_bc1 * mi) / __builtin_fmaf(sqrtf(vi), c.inv_sqrt_bc2, c.eps);
  } else {                                       // torch.optim.SGD at dampening 0 (a zero buffer is its first-step rule)
    const float pi = p;
    const float gi = __builtin_fmaf(c.wd, pi, g * c.scale);
    const float bi = __builtin_fmaf(c.momentum, m, gi);
    m = bi;
    p = __builtin_fmaf(-c.lr, KIND == SP_OPT_SGD_NESTEROV ? __builtin_fmaf(c.momentum, bi, gi) : bi, pi);
  }
}

template <int KIND, bool VEC>
__global__ __launch_bounds__(256) void optim_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, int64_t n, const float* __restrict__ hyper,
                                                    const int32_t* __restrict__ step_ptr, float grad_scale,
                                                    const double* __restrict__ partials, int npartials, float* __restrict__ norm_out) {
  constexpr bool ADAMS = KIND == SP_OPT_ADAM || KIND == SP_OPT_ADAMW;
  OptCoef c;
  c.lr = hyper[0]; c.beta1 = hyper[1]; c.beta2 = hyper[2]; c.eps = hyper[3]; c.wd = hyper[4]; c.momentum = hyper[6];
  const float max_norm = hyper[5];
  c.scale = grad_scale;
  if (partials != nullptr && max_norm > 0.f) {
    // every wave adds the partials alike (lane l: l, l+64, l+128, l+192 in this order, then the xor butterfly, whose sums are the
    // same bits in every lane): no LDS, no barrier, and one coefficient for the whole grid
    const int lane = threadIdx.x & 63;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < OPT_MAX_PARTIALS / 64; ++k) s += (lane + 64 * k < npartials) ? partials[lane + 64 * k] : 0.0;
    s = wave_sum_d(s);
    const float norm = (float)((double)grad_scale * sqrt(s));      // fp32 sums of squares overflow from |g| ~ 1e19 on: the root is taken in double
    const float q = max_norm / (norm + 1e-6f);
    const float coef = q > 1.f ? 1.f : q;                           // clamp(max=1): a NaN norm stays a NaN coefficient, as in torch
    c.scale = grad_scale * coef;
    if (blockIdx.x == 0 && threadIdx.x == 0) *norm_out = norm;
  }
  c.lr_over_bc1 = 0.f; c.inv_sqrt_bc2 = 0.f; c.decay = 1.f;
  if (ADAMS) {
    const float step = (float)(*step_ptr);
    const float bc1 = 1.f - powf(c.beta1, step), bc2 = 1.f - powf(c.beta2, step);
    c.lr_over_bc1 = c.lr / bc1; c.inv_sqrt_bc2 = rsqrtf(bc2);
    c.decay = __builtin_fmaf(-c.lr, c.wd, 1.f);
  }
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, T = (int64_t)gridDim.x * 256;
  float unused = 0.f;
  if (VEC) {
    const int64_t n4 = n >> 2;
    f32x4* p4 = reinterpret_cast<f32x4*>(p);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    f32x4* m4 = reinterpret_cast<f32x4*>(m);
    f32x4* v4 = reinterpret_cast<f32x4*>(v);
    for (int64_t i = t; i < n4; i += T) {
      f32x4 pv = p4[i], mv = m4[i], vv = {0.f, 0.f, 0.f, 0.f};
      const f32x4 gv = g4[i];
      if (ADAMS) vv = v4[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float pk = pv[k], mk = mv[k], vk = vv[k];
        opt_elem<KIND>(pk, gv[k], mk, vk, c);
        pv[k] = pk; mv[k] = mk; vv[k] = vk;
      }
      p4[i] = pv; m4[i] = mv;
      if (ADAMS) v4[i] = vv;
    }
    const int64_t i = (n4 << 2) + t;      // the up to three elements behind the last whole vector
    if (i < n) {
      if (ADAMS) opt_elem<KIND>(p[i], g[i], m[i], v[i], c);
      else opt_elem<KIND>(p[i], g[i], m[i], unused, c);
    }
  } else {
    for (int64_t i = t; i < n; i += T) {
      if (ADAMS) opt_elem<KIND>(p[i], g[i], m[i], v[i], c);
      else opt_elem<KIND>(p[i], g[i], m[i], unused, c);
    }
  }
}

template <int KIND>
static void optim_launch(bool vec, unsigned grid, hipStream_t st, float* p, const float* g, float* m, float* v, int64_t n,
                         const float* hyper, const int32_t* step, float grad_scale, const double* partials, int npartials,
                         float* norm_out) {
  if (vec) hipLaunchKernelGGL((optim_kernel<KIND, true>), dim3(grid), dim3(256), 0, st, p, g, m, v, n, hyper, step, grad_scale, partials, npartials, norm_out);
  else hipLaunchKernelGGL((optim_kernel<KIND, false>), dim3(grid), dim3(256), 0, st, p, g, m, v, n, hyper, step, grad_scale, partials, npartials, norm_out);
}

extern "C" int sp_optim_step_flat(int32_t kind, float* p, const float* g, float* m, float* v, int64_t n, const float* hyper_dev,
                                  const int32_t* step_dev, float grad_scale, const double* partials, int32_t npartials,
                                  float* norm_dev, sp_stream_t stream) {
  const bool adams = kind == SP_OPT_ADAM || kind == SP_OPT_ADAMW;
  SP_CHECK_ARG(kind >= SP_OPT_ADAM && kind <= SP_OPT_SGD_NESTEROV, "sp_optim_step_flat: unknown kind %d", (int)kind);
  SP_CHECK_ARG(p && g && m && n > 0 && hyper_dev && (!adams || (v && step_dev)), "sp_optim_step_flat: bad arguments");
  SP_CHECK_ARG(!partials || (npartials >= 1 && npartials <= OPT_MAX_PARTIALS && norm_dev),
               "sp_optim_step_flat: clipping needs 1..%d partials and a norm scalar", OPT_MAX_PARTIALS);
  // the 16-byte path needs every buffer it touches on a 16-byte boundary (the per-tensor route passes views at any 4-byte offset)
  const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (adams ? (uintptr_t)v : 0)) & 15) == 0;
  const int64_t work = vec ? (n + 3) / 4 : n;
  const unsigned grid = (unsigned)((work + 255) / 256 > OPT_MAX_BLOCKS ? OPT_MAX_BLOCKS : (work + 255) / 256);
  hipStream_t st = ST(stream);
  switch (kind) {
    case SP_OPT_ADAM: optim_launch<SP_OPT_ADAM>(vec, grid, st, p, g, m, v, n, hyper_dev, step_dev, grad_scale, partials, npartials, norm_dev); break;
    case SP_OPT_ADAMW: optim_launch<SP_OPT_ADAMW>(vec, grid, st, p, g, m, v, n, hyper_dev, step_dev, grad_scale, partials, npartials, norm_dev); break;
    case SP_OPT_SGD: optim_launch<SP_OPT_SGD>(vec, grid, st, p, g, m, v, n, hyper_dev, step_dev, grad_scale, partials, npartials, norm_dev); break;
    default: optim_launch<SP_OPT_SGD_NESTEROV>(vec, grid, st, p, g, m, v, n, hyper_dev, step_dev, grad_scale, partials, npartials, norm_dev); break;
  }
  SP_CHECK_LAUNCH("sp_optim_step_flat");
  return SP_OK;
}
