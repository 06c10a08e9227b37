// The training criteria (include/stroke_amd.h), each as sums -> finalize -> backward with the scalar algebra on the device:
//   * sp_dice_*: BatchDiceLoss (metrics.py:16-28), three moments per channel -- the headline training step's path;
//   * sp_vloss_* / sp_bloss_* / sp_tloss_*: ONE per-channel family of four moments, the three region columns holding second or first
//     moments, the fourth nothing, sum bce, sum o*phi or the focal cross-entropy sum;
//   * sp_cae_loss_* / sp_cae_loss_crit_*: the CAE reconstruction loss (CaeReconstructionLearner.py:52-70), ONE kernel set.
// Every sums kernel reduces alike: per-thread fp32, wave sum, the four waves in order (sp_cols_sum), one fp64 atomic per workgroup and
// column into a replica row.  All of it is bandwidth- or latency-bound elementwise work on fp32; nothing here depends on the 16-bit
// storage type.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sp_common.h"

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define LOSS_MAX_BLOCKS 4096      // workgroups of a backward launch at most

// ------------------------------------------------------------------------------------------------ BatchDiceLoss
// These kernels are NOT instances of the four-moment family below: three columns, a flat backward grid and element loads.  Routing them
// through the 16-byte-load kernels would regroup the fp32 partial sums of the headline training step -- a change of its bits.
// sums[c] = (sum o*t, sum o*o, sum t*t) over batch and volume.
// o / t are (B, C, DHW) with an arbitrary BATCH stride (elements): dto.outputs.core / .penu are channel slices of one
// (B, 2, DHW) tensor and are read in place.
__global__ __launch_bounds__(256) void dice_sums_kernel(const float* __restrict__ o, int64_t obs, const float* __restrict__ t,
                                                         int64_t tbs, int C, int64_t DHW, double* __restrict__ sums) {
  // grid.y = b*C + c ; grid.x strides over the volume
  const int bc = blockIdx.y, c = bc % C, b = bc / C;
  const float* op = o + (int64_t)b * obs + (int64_t)c * DHW;
  const float* tp = t + (int64_t)b * tbs + (int64_t)c * DHW;
  float s[3] = {0.f, 0.f, 0.f};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < DHW; i += (int64_t)gridDim.x * 256) {
    const float a = op[i], bb = tp[i];
    s[0] += a * bb; s[1] += a * a; s[2] += bb * bb;
  }
  __shared__ float red[4 * 3];      // [wave][moment], added up in wave order (sp_cols_sum)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float w = wave_sum(s[k]);
    if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * 3 + k] = w;
  }
  __syncthreads();
  // replica row per workgroup (rows 128 bytes or more apart): 1024 same-line fp64 atomics cost ~20 us at the tail
  if (threadIdx.x < 3)
    atomicAdd(&sums[(size_t)((blockIdx.x + blockIdx.y) % SP_REDUCE_ROWS) * SP_DICE_PITCH(C) + c * 3 + threadIdx.x], (double)sp_cols_sum(red, 3, 4, threadIdx.x));
}
extern "C" int sp_dice_sums(const float* o, int64_t o_bstride, const float* t, int64_t t_bstride, int32_t B, int32_t C,
                            int64_t DHW, double* sums, sp_stream_t stream) {
  SP_CHECK_ARG(o && t && sums && B >= 1 && C >= 1 && o_bstride >= C * DHW && t_bstride >= C * DHW, "sp_dice_sums: bad arguments");
  int64_t gx = (DHW + 256 * 8 - 1) / (256 * 8);
  if (gx > 256) gx = 256;
  hipLaunchKernelGGL(dice_sums_kernel, dim3((unsigned)gx, B * C), dim3(256), 0, ST(stream), o, o_bstride, t, t_bstride, C, DHW, sums);
  SP_CHECK_LAUNCH("sp_dice_sums");
  return SP_OK;
}
// loss = 1 - sum_c w_c (2 I_c + eps) / (O_c + T_c + eps);  coef[c] = (ca, cb) with d loss / d o = ca*t + cb*o:
// ca = -2 w / den, cb = 2 w num / den^2.  One launch instead of a dozen one-element torch kernels.
// clear != NULL (= sums): the replica rows are zeroed again once they are read -- the caller keeps ONE accumulator and needs no fill
// launch in front of the next sp_dice_sums (4.9 us of a training step's dependent chain)
__global__ void dice_finalize_kernel(const double* __restrict__ sums, const float* __restrict__ w, double eps, int C,
                                     float* __restrict__ loss, float* __restrict__ coef, double* __restrict__ clear) {
  const int pitch = SP_DICE_PITCH(C);
  if (threadIdx.x == 0) {
    double acc = 0.0;
    for (int c = 0; c < C; ++c) {
      const double num = 2.0 * sp_rows_sum(sums, c * 3, pitch) + eps;
      const double den = sp_rows_sum(sums, c * 3 + 1, pitch) + sp_rows_sum(sums, c * 3 + 2, pitch) + eps;
      acc += (double)w[c] * num / den;
      coef[2 * c] = (float)(-2.0 * w[c] / den);
      coef[2 * c + 1] = (float)(2.0 * w[c] * num / (den * den));
    }
    *loss = (float)(1.0 - acc);
  }
  if (clear) {
    __syncthreads();
    for (int k = threadIdx.x; k < SP_REDUCE_ROWS * pitch; k += blockDim.x) clear[k] = 0.0;
  }
}
extern "C" int sp_dice_finalize(const double* sums, const float* weights, double eps, int32_t C, float* loss, float* coef,
                                sp_stream_t stream) {
  SP_CHECK_ARG(sums && weights && loss && coef && C >= 1, "sp_dice_finalize: bad arguments");
  hipLaunchKernelGGL(dice_finalize_kernel, dim3(1), dim3(64), 0, ST(stream), sums, weights, eps, C, loss, coef, (double*)nullptr);
  SP_CHECK_LAUNCH("sp_dice_finalize");
  return SP_OK;
}
extern "C" int sp_dice_finalize_clear(double* sums, const float* weights, double eps, int32_t C, float* loss, float* coef,
                                      sp_stream_t stream) {
  SP_CHECK_ARG(sums && weights && loss && coef && C >= 1, "sp_dice_finalize_clear: bad arguments");
  hipLaunchKernelGGL(dice_finalize_kernel, dim3(1), dim3(64), 0, ST(stream), sums, weights, eps, C, loss, coef, sums);
  SP_CHECK_LAUNCH("sp_dice_finalize_clear");
  return SP_OK;
}
// do[b,c,v] = up * (ca[c]*t + cb[c]*o), up = *upstream (the scalar gradient of the loss, read on the device)
__global__ void dice_bwd_kernel(const float* __restrict__ o, int64_t obs, const float* __restrict__ t, int64_t tbs,
                                const float* __restrict__ coef, const float* __restrict__ upstream, int C, int64_t DHW,
                                int64_t total, float* __restrict__ d) {
  const float up = upstream ? *upstream : 1.f;
  const int64_t per_b = (int64_t)C * DHW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / per_b, r = i - b * per_b;
    const int c = (int)(r / DHW);
    d[i] = up * (coef[2 * c] * t[b * tbs + r] + coef[2 * c + 1] * o[b * obs + r]);
  }
}
extern "C" int sp_dice_bwd(const float* o, int64_t o_bstride, const float* t, int64_t t_bstride, const float* coef,
                           const float* upstream, int32_t B, int32_t C, int64_t DHW, float* dout, sp_stream_t stream) {
  SP_CHECK_ARG(o && t && coef && dout, "sp_dice_bwd: null pointer");
  const int64_t total = (int64_t)B * C * DHW;
  const unsigned grid = (unsigned)((total + 255) / 256 > LOSS_MAX_BLOCKS ? LOSS_MAX_BLOCKS : (total + 255) / 256);
  hipLaunchKernelGGL(dice_bwd_kernel, dim3(grid), dim3(256), 0, ST(stream), o, o_bstride, t, t_bstride, coef, upstream, C, DHW,
                     total, dout);
  SP_CHECK_LAUNCH("sp_dice_bwd");
  return SP_OK;
}

// ------------------------------------------------------------------------------------------------ the four-moment family
// sums[c] = (sum o*t, sum o*o, sum t*t, X) over batch and volume, the first three present with DICE, X chosen by X4: nothing, sum bce
// (sp_vloss_*: torch.nn.BCELoss semantics, finite at a saturated sigmoid, o = 0 or 1) or sum o*phi (sp_bloss_*: phi a third input,
// dense (B, C, DHW)).  d loss / d o = ca*t + cb*o + c3*X'.
// FIRST (sp_tloss_*: Tversky and focal criteria): the region columns hold first moments, (sum o*t, sum o, sum t), X is the focal cross
// entropy sum fl(o, t) and d loss / d o = ca*t + cb + c3*fl'.  The focal exponent: X4_FOCAL2 is gamma == 2 at compile time (the default
// of the criteria: multiplies only); X4_FOCAL reads gamma from the arguments and branches, uniformly over the launch, between 0, 1
// (multiplies again) and the general x^gamma = expf(gamma log x) on the two logarithms the term has anyway.
enum { X4_NONE = 0, X4_BCE = 1, X4_PHI = 2, X4_FOCAL2 = 3, X4_FOCAL = 4 };
__device__ __forceinline__ float bce_term(float o, float t) {
  return -(t * fmaxf(logf(o), -100.f) + (1.f - t) * fmaxf(logf(1.f - o), -100.f));
}
// d bce / d o: (o - t) / max(o (1 - o), 1e-12)
__device__ __forceinline__ float bce_grad(float o, float t) { return (o - t) / fmaxf(o * (1.f - o), 1e-12f); }
// fl(o, t) = -al t (1 - o)^g lo - (1 - al) (1 - t) o^g l1 with the logarithms clamped as bce_term clamps them: o = 0 and o = 1 give
// finite values (the clamped logarithm stands in the exponent too: 0^g = expf(-100 g), 1 at g = 0 as pow has it)
template <int X4> __device__ __forceinline__ float focal_term(float o, float t, float g, float al) {
  const float q = 1.f - o, lo = fmaxf(logf(o), -100.f), l1 = fmaxf(logf(q), -100.f);
  float pq, po;
  if (X4 == X4_FOCAL2) { pq = q * q; po = o * o; }
  else if (g == 0.f) { pq = 1.f; po = 1.f; }
  else if (g == 1.f) { pq = q; po = o; }
  else { pq = expf(g * l1); po = expf(g * lo); }
  return -(al * t * pq * lo) - (1.f - al) * (1.f - t) * po * l1;
}
// d fl / d o = al t [g (1 - o)^(g-1) lo - (1 - o)^g / max(o, 1e-12)] + (1 - al) (1 - t) [-g o^(g-1) l1 + o^g / max(1 - o, 1e-12)]; the
// g x^(g-1) terms are absent at g = 0.  x^g = x * x^(g-1): two expf for a general g.  Finite for every o in [0, 1].
template <int X4> __device__ __forceinline__ float focal_grad(float o, float t, float g, float al) {
  const float q = 1.f - o, lo = fmaxf(logf(o), -100.f), l1 = fmaxf(logf(q), -100.f);
  const float ro = 1.f / fmaxf(o, 1e-12f), rq = 1.f / fmaxf(q, 1e-12f);
  float A, Bq;      // the bracket of the t = 1 side / of the t = 0 side
  if (X4 == X4_FOCAL2) { A = 2.f * q * lo - q * q * ro; Bq = o * o * rq - 2.f * o * l1; }
  else if (g == 0.f) { A = -ro; Bq = rq; }
  else if (g == 1.f) { A = lo - q * ro; Bq = o * rq - l1; }
  else {
    const float pq = expf((g - 1.f) * l1), po = expf((g - 1.f) * lo);      // (1 - o)^(g-1), o^(g-1)
    A = g * pq * lo - pq * q * ro; Bq = po * o * rq - g * po * l1;
  }
  return al * t * A + (1.f - al) * (1.f - t) * Bq;
}
template <bool DICE, int X4, bool FIRST = false>
__device__ __forceinline__ void crit_acc(float a, float b, float p, float (&s)[4], float fg = 0.f, float fa = 0.f) {
  if (DICE && !FIRST) { s[0] += a * b; s[1] += a * a; s[2] += b * b; }
  if (DICE && FIRST) { s[0] += a * b; s[1] += a; s[2] += b; }
  if (X4 == X4_BCE) s[3] += bce_term(a, b);
  if (X4 == X4_PHI) s[3] += a * p;
  if (X4 == X4_FOCAL2 || X4 == X4_FOCAL) s[3] += focal_term<X4>(a, b, fg, fa);
}
template <int X4, bool FIRST = false>
__device__ __forceinline__ float crit_grad(float a, float b, float p, float ca, float cb, float c3, float fg = 0.f, float fa = 0.f) {
  const float g = FIRST ? ca * b + cb : ca * b + cb * a;
  if (X4 == X4_FOCAL2 || X4 == X4_FOCAL) return g + c3 * focal_grad<X4>(a, b, fg, fa);
  return X4 == X4_BCE ? g + c3 * bce_grad(a, b) : (X4 == X4_PHI ? g + c3 * p : g);
}
// The layout and the reduction order of dice_sums_kernel; an operand no moment needs (t without DICE and BCE, phi without X4_PHI) is
// not loaded, a column whose term is absent is neither reduced nor added.
// VEC: DHW % 4 == 0 and every row base 16-byte aligned (checked by the launcher) -> one 16-byte load per lane and operand.
// FIRST: first moments in the region columns; fg / fa: the focal exponent and alpha (read by the focal instances only).
template <bool DICE, int X4, bool VEC, bool FIRST = false>
__global__ __launch_bounds__(256) void crit_sums_kernel(const float* __restrict__ o, int64_t obs, const float* __restrict__ t, int64_t tbs,
                                                        const float* __restrict__ phi, int C, int64_t DHW, double* __restrict__ sums,
                                                        float fg, float fa) {
  constexpr bool T = DICE || X4 == X4_BCE || X4 == X4_FOCAL2 || X4 == X4_FOCAL, PHI = X4 == X4_PHI;
  // grid.y = b*C + c ; grid.x strides over the volume
  const int bc = blockIdx.y, c = bc % C, b = bc / C;
  const float* op = o + (int64_t)b * obs + (int64_t)c * DHW;
  const float* tp = t + (int64_t)b * tbs + (int64_t)c * DHW;
  const float* pp = PHI ? phi + (int64_t)bc * DHW : nullptr;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if (VEC) {
    const float4* o4 = reinterpret_cast<const float4*>(op);
    const float4* t4 = reinterpret_cast<const float4*>(tp);
    const float4* p4 = reinterpret_cast<const float4*>(pp);
    const int64_t n4 = DHW >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
      const float4 a = o4[i];
      float4 bb = make_float4(0.f, 0.f, 0.f, 0.f), p = bb;
      if (PHI) p = p4[i];
      if (T) bb = t4[i];
      crit_acc<DICE, X4, FIRST>(a.x, bb.x, p.x, s, fg, fa); crit_acc<DICE, X4, FIRST>(a.y, bb.y, p.y, s, fg, fa);
      crit_acc<DICE, X4, FIRST>(a.z, bb.z, p.z, s, fg, fa); crit_acc<DICE, X4, FIRST>(a.w, bb.w, p.w, s, fg, fa);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < DHW; i += (int64_t)gridDim.x * 256)
      crit_acc<DICE, X4, FIRST>(op[i], T ? tp[i] : 0.f, PHI ? pp[i] : 0.f, s, fg, fa);
  }
  __shared__ float red[4 * 4];      // [wave][moment], added up in wave order (sp_cols_sum)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < 3 ? !DICE : X4 == X4_NONE) continue;
    const float w = wave_sum(s[k]);
    if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * 4 + k] = w;
  }
  __syncthreads();
  if (threadIdx.x < 4 && (threadIdx.x < 3 ? DICE : X4 != X4_NONE))
    atomicAdd(&sums[(size_t)((blockIdx.x + blockIdx.y) % SP_REDUCE_ROWS) * SP_VLOSS_PITCH(C) + c * 4 + threadIdx.x], (double)sp_cols_sum(red, 4, 4, threadIdx.x));
}
static inline bool crit_vec_ok(const void* p, int64_t bstride, int B, int64_t DHW) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && DHW % 4 == 0 && (B == 1 || bstride % 4 == 0);
}
static inline bool crit_args_ok(const float* o, int64_t obs, const float* t, int64_t tbs, int32_t B, int32_t C, int64_t DHW) {
  return o && t && B >= 1 && C >= 1 && DHW >= 1 && (int64_t)B * C <= 65535 && obs >= C * DHW && tbs >= C * DHW;
}
// phi != NULL: the fourth moment is sum o*phi, and phi takes part in the choice of the load width; first: first moments (sp_tloss_*)
static void crit_sums_launch(const float* o, int64_t obs, const float* t, int64_t tbs, const float* phi, int32_t B, int32_t C, int64_t DHW,
                             bool dice, int x4, double* sums, sp_stream_t stream, bool first = false, float fg = 0.f, float fa = 0.f) {
  int64_t gx = (DHW + 256 * 8 - 1) / (256 * 8);
  if (gx > 256) gx = 256;
  const bool vec = crit_vec_ok(o, obs, B, DHW) && crit_vec_ok(t, tbs, B, DHW) && (!phi || crit_vec_ok(phi, 0, 1, DHW));
#define SP_CRIT_SUMS(D_, X_, F_)                                                                                                        \
  do {                                                                                                                                  \
    if (vec) hipLaunchKernelGGL((crit_sums_kernel<D_, X_, true, F_>), dim3((unsigned)gx, B * C), dim3(256), 0, ST(stream), o, obs, t, tbs, phi, C, DHW, sums, fg, fa); \
    else hipLaunchKernelGGL((crit_sums_kernel<D_, X_, false, F_>), dim3((unsigned)gx, B * C), dim3(256), 0, ST(stream), o, obs, t, tbs, phi, C, DHW, sums, fg, fa);   \
  } while (0)
  if (first) {
    if (x4 == X4_FOCAL2) { if (dice) SP_CRIT_SUMS(true, X4_FOCAL2, true); else SP_CRIT_SUMS(false, X4_FOCAL2, true); }
    else if (x4 == X4_FOCAL) { if (dice) SP_CRIT_SUMS(true, X4_FOCAL, true); else SP_CRIT_SUMS(false, X4_FOCAL, true); }
    else SP_CRIT_SUMS(true, X4_NONE, true);
  }
  else if (x4 == X4_PHI) { if (dice) SP_CRIT_SUMS(true, X4_PHI, false); else SP_CRIT_SUMS(false, X4_PHI, false); }
  else if (x4 == X4_BCE) { if (dice) SP_CRIT_SUMS(true, X4_BCE, false); else SP_CRIT_SUMS(false, X4_BCE, false); }
  else SP_CRIT_SUMS(true, X4_NONE, false);
#undef SP_CRIT_SUMS
}
extern "C" int sp_vloss_sums(const float* o, int64_t o_bstride, const float* t, int64_t t_bstride, int32_t B, int32_t C, int64_t DHW,
                             int32_t terms, double* sums, sp_stream_t stream) {
  SP_CHECK_ARG(crit_args_ok(o, o_bstride, t, t_bstride, B, C, DHW) && sums && terms >= 1 && terms <= (SP_VLOSS_DICE | SP_VLOSS_BCE),
               "sp_vloss_sums: bad arguments");
  crit_sums_launch(o, o_bstride, t, t_bstride, nullptr, B, C, DHW, terms & SP_VLOSS_DICE, terms & SP_VLOSS_BCE ? X4_BCE : X4_NONE, sums, stream);
  SP_CHECK_LAUNCH("sp_vloss_sums");
  return SP_OK;
}
extern "C" int sp_bloss_sums(const float* o, int64_t o_bstride, const float* t, int64_t t_bstride, const float* phi, int32_t B, int32_t C,
                             int64_t DHW, int32_t dice, double* sums, sp_stream_t stream) {
  SP_CHECK_ARG(crit_args_ok(o, o_bstride, t, t_bstride, B, C, DHW) && phi && sums && (dice == 0 || dice == 1), "sp_bloss_sums: bad arguments");
  crit_sums_launch(o, o_bstride, t, t_bstride, phi, B, C, DHW, dice, X4_PHI, sums, stream);
  SP_CHECK_LAUNCH("sp_bloss_sums");
  return SP_OK;
}
// one thread: the loss and the backward's coefficients (ca, cb, c3) per channel; then all threads zero the replica rows again.
// wd / w4: the weights of the Dice term / of the fourth moment, NULL = the term is absent; scale: one float on the device that
// multiplies w4 (the boundary weight: a captured step follows its schedule), NULL = 1
// FIRST (sp_tloss_*): the region term is the (focal) Tversky loss on first moments, wd its weights: with TP = sum o*t, N = TP + eps,
// D = TP + fpw (sum o - TP) + fnw (sum t - TP) + eps and base = 1 - N / D it is wd max(base, 1e-12)^(1 / tg), and (ca, cb) are the
// coefficients of d / d o = ca*t + cb.  Below the clamp the gradient is zero, as torch's clamp_min has it: a perfectly predicted or an
// empty channel has base = 0, where base^(1/tg - 1) is 0^(negative).
template <bool FIRST>
__global__ void crit_finalize_kernel(double* __restrict__ sums, const float* __restrict__ wd, const float* __restrict__ w4,
                                     const float* __restrict__ scale, double eps, double count, int C, float* __restrict__ loss,
                                     float* __restrict__ coef, double fpw, double fnw, double tg) {
  const int pitch = SP_VLOSS_PITCH(C);
  if (threadIdx.x == 0) {
    const double sc = scale ? (double)scale[0] : 1.0;
    double dice = 0.0, x = 0.0;
    for (int c = 0; c < C; ++c) {
      float ca = 0.f, cb = 0.f, c3 = 0.f;
      if (FIRST && wd) {
        const double tp = sp_rows_sum(sums, c * 4, pitch);
        const double N = tp + eps;
        const double D = tp + fpw * (sp_rows_sum(sums, c * 4 + 1, pitch) - tp) + fnw * (sp_rows_sum(sums, c * 4 + 2, pitch) - tp) + eps;
        const double base = 1.0 - N / D;
        dice += (double)wd[c] * pow(fmax(base, 1e-12), 1.0 / tg);
        const double k = base >= 1e-12 ? -((double)wd[c] / tg) * pow(base, 1.0 / tg - 1.0) : 0.0;
        ca = (float)(k * (1.0 / D - N * (1.0 - fpw - fnw) / (D * D)));
        cb = (float)(-k * N * fpw / (D * D));
      }
      if (!FIRST && wd) {
        const double num = 2.0 * sp_rows_sum(sums, c * 4, pitch) + eps;
        const double den = sp_rows_sum(sums, c * 4 + 1, pitch) + sp_rows_sum(sums, c * 4 + 2, pitch) + eps;
        dice += (double)wd[c] * num / den;
        ca = (float)(-2.0 * wd[c] / den);
        cb = (float)(2.0 * wd[c] * num / (den * den));
      }
      if (w4) {
        const double w = (double)w4[c] * sc;
        x += w * sp_rows_sum(sums, c * 4 + 3, pitch) / count;
        c3 = (float)(w / count);
      }
      coef[3 * c] = ca; coef[3 * c + 1] = cb; coef[3 * c + 2] = c3;
    }
    *loss = (float)((wd ? (FIRST ? dice : 1.0 - dice) : 0.0) + x);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < SP_REDUCE_ROWS * pitch; k += blockDim.x) sums[k] = 0.0;
}
extern "C" int sp_vloss_finalize_clear(double* sums, const float* w_dice, const float* w_bce, double eps, double count, int32_t C,
                                       float* loss, float* coef, sp_stream_t stream) {
  SP_CHECK_ARG(sums && (w_dice || w_bce) && loss && coef && C >= 1 && count > 0.0, "sp_vloss_finalize_clear: bad arguments");
  hipLaunchKernelGGL(crit_finalize_kernel<false>, dim3(1), dim3(64), 0, ST(stream), sums, w_dice, w_bce, (const float*)nullptr, eps, count, C, loss, coef,
                     0.0, 0.0, 1.0);
  SP_CHECK_LAUNCH("sp_vloss_finalize_clear");
  return SP_OK;
}
extern "C" int sp_bloss_finalize_clear(double* sums, const float* w_dice, const float* w_boundary, const float* scale, double eps, double count,
                                       int32_t C, float* loss, float* coef, sp_stream_t stream) {
  SP_CHECK_ARG(sums && w_boundary && scale && loss && coef && C >= 1 && count > 0.0, "sp_bloss_finalize_clear: bad arguments");
  hipLaunchKernelGGL(crit_finalize_kernel<false>, dim3(1), dim3(64), 0, ST(stream), sums, w_dice, w_boundary, scale, eps, count, C, loss, coef,
                     0.0, 0.0, 1.0);
  SP_CHECK_LAUNCH("sp_bloss_finalize_clear");
  return SP_OK;
}
// do[b,c,v] = up * (ca[c]*t + cb[c]*o + c3[c]*X'), X' = phi (PHI) or (o - t)/max(o(1 - o), 1e-12); grid as crit_sums_kernel: the
// coefficients are uniform over a workgroup.  Without phi a channel that has no BCE term (c3 == 0) takes the loop without the division.
// X: X4_BCE (sp_vloss_*), X4_PHI (sp_bloss_*) or, with first moments -- up * (ca*t + cb + c3*fl') --, X4_FOCAL2 / X4_FOCAL (sp_tloss_*:
// a channel without a focal term takes the loop without the logarithms).
template <int X, bool VEC>
__global__ __launch_bounds__(256) void crit_bwd_kernel(const float* __restrict__ o, int64_t obs, const float* __restrict__ t, int64_t tbs,
                                                       const float* __restrict__ phi, const float* __restrict__ coef,
                                                       const float* __restrict__ upstream, int C, int64_t DHW, float* __restrict__ d,
                                                       float fg, float fa) {
  constexpr bool PHI = X == X4_PHI, FIRST = X == X4_FOCAL2 || X == X4_FOCAL;
  constexpr int XA = X, XB = PHI ? X4_PHI : X4_NONE;      // the loop with c3 != 0 / with c3 == 0
  const int bc = blockIdx.y, c = bc % C, b = bc / C;
  const float up = upstream ? *upstream : 1.f;
  const float ca = up * coef[3 * c], cb = up * coef[3 * c + 1], c3 = up * coef[3 * c + 2];
  const bool xa = PHI || coef[3 * c + 2] != 0.f;
  const float* op = o + (int64_t)b * obs + (int64_t)c * DHW;
  const float* tp = t + (int64_t)b * tbs + (int64_t)c * DHW;
  const float* pp = PHI ? phi + (int64_t)bc * DHW : nullptr;
  float* dp = d + (int64_t)bc * DHW;
  if (VEC) {
    const float4* o4 = reinterpret_cast<const float4*>(op);
    const float4* t4 = reinterpret_cast<const float4*>(tp);
    const float4* p4 = reinterpret_cast<const float4*>(pp);
    float4* d4 = reinterpret_cast<float4*>(dp);
    const int64_t n4 = DHW >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
      const float4 a = o4[i], bb = t4[i];
      float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
      if (PHI) p = p4[i];
      d4[i] = xa ? make_float4(crit_grad<XA, FIRST>(a.x, bb.x, p.x, ca, cb, c3, fg, fa), crit_grad<XA, FIRST>(a.y, bb.y, p.y, ca, cb, c3, fg, fa),
                               crit_grad<XA, FIRST>(a.z, bb.z, p.z, ca, cb, c3, fg, fa), crit_grad<XA, FIRST>(a.w, bb.w, p.w, ca, cb, c3, fg, fa))
                 : make_float4(crit_grad<XB, FIRST>(a.x, bb.x, p.x, ca, cb, c3), crit_grad<XB, FIRST>(a.y, bb.y, p.y, ca, cb, c3),
                               crit_grad<XB, FIRST>(a.z, bb.z, p.z, ca, cb, c3), crit_grad<XB, FIRST>(a.w, bb.w, p.w, ca, cb, c3));
    }
  } else if (PHI) {      // written out, t loaded first: the order of the loads decides which of the products the compiler fuses
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < DHW; i += (int64_t)gridDim.x * 256) dp[i] = ca * tp[i] + cb * op[i] + c3 * pp[i];
  } else if (xa) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < DHW; i += (int64_t)gridDim.x * 256) dp[i] = crit_grad<XA, FIRST>(op[i], tp[i], 0.f, ca, cb, c3, fg, fa);
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < DHW; i += (int64_t)gridDim.x * 256) dp[i] = crit_grad<XB, FIRST>(op[i], tp[i], 0.f, ca, cb, c3);
  }
}
// x: X4_BCE, X4_FOCAL2 or X4_FOCAL without phi
static void crit_bwd_launch(const float* o, int64_t obs, const float* t, int64_t tbs, const float* phi, const float* coef, const float* upstream,
                            int32_t B, int32_t C, int64_t DHW, float* dout, sp_stream_t stream, int x = X4_BCE, float fg = 0.f, float fa = 0.f) {
  const bool vec = crit_vec_ok(o, obs, B, DHW) && crit_vec_ok(t, tbs, B, DHW) && (!phi || crit_vec_ok(phi, 0, 1, DHW)) && crit_vec_ok(dout, 0, 1, DHW);
  const int64_t per = vec ? 256 * 4 : 256;                                  // elements per workgroup and trip
  int64_t gx = (DHW + per - 1) / per, cap = LOSS_MAX_BLOCKS / ((int64_t)B * C);
  if (cap < 1) cap = 1;
  if (gx > cap) gx = cap;
#define SP_CRIT_BWD(X_, V_) hipLaunchKernelGGL((crit_bwd_kernel<X_, V_>), dim3((unsigned)gx, B * C), dim3(256), 0, ST(stream), o, obs, t, tbs, phi, coef, upstream, C, DHW, dout, fg, fa)
  if (phi) { if (vec) SP_CRIT_BWD(X4_PHI, true); else SP_CRIT_BWD(X4_PHI, false); }
  else if (x == X4_FOCAL2) { if (vec) SP_CRIT_BWD(X4_FOCAL2, true); else SP_CRIT_BWD(X4_FOCAL2, false); }
  else if (x == X4_FOCAL) { if (vec) SP_CRIT_BWD(X4_FOCAL, true); else SP_CRIT_BWD(X4_FOCAL, false); }
  else { if (vec) SP_CRIT_BWD(X4_BCE, true); else SP_CRIT_BWD(X4_BCE, false); }
#undef SP_CRIT_BWD
}
extern "C" int sp_vloss_bwd(const float* o, int64_t o_bstride, const float* t, int64_t t_bstride, const float* coef, const float* upstream,
                            int32_t B, int32_t C, int64_t DHW, float* dout, sp_stream_t stream) {
  SP_CHECK_ARG(crit_args_ok(o, o_bstride, t, t_bstride, B, C, DHW) && coef && dout, "sp_vloss_bwd: bad arguments");
  crit_bwd_launch(o, o_bstride, t, t_bstride, nullptr, coef, upstream, B, C, DHW, dout, stream);
  SP_CHECK_LAUNCH("sp_vloss_bwd");
  return SP_OK;
}
extern "C" int sp_bloss_bwd(const float* o, int64_t o_bstride, const float* t, int64_t t_bstride, const float* phi, const float* coef,
                            const float* upstream, int32_t B, int32_t C, int64_t DHW, float* dout, sp_stream_t stream) {
  SP_CHECK_ARG(crit_args_ok(o, o_bstride, t, t_bstride, B, C, DHW) && phi && coef && dout, "sp_bloss_bwd: bad arguments");
  crit_bwd_launch(o, o_bstride, t, t_bstride, phi, coef, upstream, B, C, DHW, dout, stream);
  SP_CHECK_LAUNCH("sp_bloss_bwd");
  return SP_OK;
}
// the Tversky / focal entry points: first moments in the region columns, the focal cross entropy in the fourth
static inline bool focal_args_ok(float g, float al) { return (g == 0.f || g >= 1.f) && al >= 0.f && al <= 1.f; }
extern "C" int sp_tloss_sums(const float* o, int64_t o_bstride, const float* t, int64_t t_bstride, int32_t B, int32_t C, int64_t DHW,
                             int32_t terms, float focal_gamma, float focal_alpha, double* sums, sp_stream_t stream) {
  SP_CHECK_ARG(crit_args_ok(o, o_bstride, t, t_bstride, B, C, DHW) && sums && terms >= 1 && terms <= (SP_TLOSS_TVERSKY | SP_TLOSS_FOCAL) &&
               (!(terms & SP_TLOSS_FOCAL) || focal_args_ok(focal_gamma, focal_alpha)), "sp_tloss_sums: bad arguments");
  crit_sums_launch(o, o_bstride, t, t_bstride, nullptr, B, C, DHW, terms & SP_TLOSS_TVERSKY,
                   terms & SP_TLOSS_FOCAL ? (focal_gamma == 2.f ? X4_FOCAL2 : X4_FOCAL) : X4_NONE, sums, stream, true, focal_gamma, focal_alpha);
  SP_CHECK_LAUNCH("sp_tloss_sums");
  return SP_OK;
}
extern "C" int sp_tloss_finalize_clear(double* sums, const float* w_tversky, const float* w_focal, double fp_weight, double fn_weight,
                                       double tversky_gamma, double eps, double count, int32_t C, float* loss, float* coef, sp_stream_t stream) {
  SP_CHECK_ARG(sums && (w_tversky || w_focal) && loss && coef && C >= 1 && count > 0.0 && fp_weight >= 0.0 && fn_weight >= 0.0 && tversky_gamma >= 1.0,
               "sp_tloss_finalize_clear: bad arguments");
  hipLaunchKernelGGL(crit_finalize_kernel<true>, dim3(1), dim3(64), 0, ST(stream), sums, w_tversky, w_focal, (const float*)nullptr, eps, count, C, loss,
                     coef, fp_weight, fn_weight, tversky_gamma);
  SP_CHECK_LAUNCH("sp_tloss_finalize_clear");
  return SP_OK;
}
extern "C" int sp_tloss_bwd(const float* o, int64_t o_bstride, const float* t, int64_t t_bstride, const float* coef, const float* upstream,
                            float focal_gamma, float focal_alpha, int32_t B, int32_t C, int64_t DHW, float* dout, sp_stream_t stream) {
  SP_CHECK_ARG(crit_args_ok(o, o_bstride, t, t_bstride, B, C, DHW) && coef && dout && focal_args_ok(focal_gamma, focal_alpha), "sp_tloss_bwd: bad arguments");
  crit_bwd_launch(o, o_bstride, t, t_bstride, nullptr, coef, upstream, B, C, DHW, dout, stream, focal_gamma == 2.f ? X4_FOCAL2 : X4_FOCAL, focal_gamma,
                  focal_alpha);
  SP_CHECK_LAUNCH("sp_tloss_bwd");
  return SP_OK;
}

// ------------------------------------------------------------------------------------------------ the CAE reconstruction loss
// Three launches (CaeReconstructionLearner.py:52-70), each of the three criterion terms chosen by TERMS (SP_VLOSS_DICE | SP_VLOSS_BCE):
//   [ mean(|p - i| - (p - i)) + mean(|p - c| - (p - c)) + crit(c, tc) + crit(p, tp) + crit(l, tl) + f mean|zi - zl| ] / (5 + f)
// c, p, l, i = the four reconstructions (B, 1, D, H, W), t* the ground truths, z* the latents.  Composed of torch operators and three
// criterion calls it is ~60 kernels between the forward and the backward of a step (0.3 ms of a 6.5 ms step).
// sums (replica rows of 16 doubles): 0 hinge(p, i), 1 hinge(p, c), 2-4 Dice(c), 5-7 Dice(p), 8-10 Dice(l), 11 sum |zi - zl|,
// 12-14 the BCE sums of c, p, l
template <int TERMS>
__global__ __launch_bounds__(256) void cae_crit_sums_kernel(const float* __restrict__ c, int64_t cbs, const float* __restrict__ p, int64_t pbs,
                                                            const float* __restrict__ l, int64_t lbs, const float* __restrict__ ii, int64_t ibs,
                                                            const float* __restrict__ tc, int64_t tcbs, const float* __restrict__ tp, int64_t tpbs,
                                                            const float* __restrict__ tl, int64_t tlbs, int64_t DHW, double* __restrict__ sums,
                                                            int B, const float* __restrict__ zi, const float* __restrict__ zl, int64_t nlat) {
  constexpr bool DICE = (TERMS & SP_VLOSS_DICE) != 0;
  constexpr int X4 = TERMS & SP_VLOSS_BCE ? X4_BCE : X4_NONE;
  __shared__ float red[4 * 16];      // [wave][column of the accumulator row], added up in wave order (sp_cols_sum)
  if ((int)blockIdx.y == B) {        // the latent term: sum |zi - zl| -> column 11
    float t = 0.f;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < nlat; k += (int64_t)gridDim.x * 256) t += fabsf(zi[k] - zl[k]);
    t = wave_sum(t);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&sums[(size_t)(blockIdx.x % SP_REDUCE_ROWS) * 16 + 11], (double)((red[0] + red[1]) + (red[2] + red[3])));
    return;
  }
  const int b = blockIdx.y;
  c += b * cbs; p += b * pbs; l += b * lbs; ii += b * ibs; tc += b * tcbs; tp += b * tpbs; tl += b * tlbs;
  float h[2] = {0.f, 0.f}, sc[4] = {0.f, 0.f, 0.f, 0.f}, sp[4] = {0.f, 0.f, 0.f, 0.f}, sl[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < DHW; v += (int64_t)gridDim.x * 256) {
    const float vc = c[v], vp = p[v], vl = l[v], vi = ii[v];
    const float d1 = vp - vi, d2 = vp - vc;
    h[0] += fabsf(d1) - d1; h[1] += fabsf(d2) - d2;
    crit_acc<DICE, X4>(vc, tc[v], 0.f, sc); crit_acc<DICE, X4>(vp, tp[v], 0.f, sp); crit_acc<DICE, X4>(vl, tl[v], 0.f, sl);
  }
  // accumulator column -> this thread's partial (a column whose term is absent is neither reduced nor added)
  const float col[16] = {h[0], h[1], sc[0], sc[1], sc[2], sp[0], sp[1], sp[2], sl[0], sl[1], sl[2], 0.f, sc[3], sp[3], sl[3], 0.f};
#pragma unroll
  for (int k = 0; k < 15; ++k) {
    if (k == 11 || (k >= 2 && k <= 10 && !DICE) || (k >= 12 && X4 == X4_NONE)) continue;
    const float w = wave_sum(col[k]);
    if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * 16 + k] = w;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < 15 && k != 11 && !(k >= 2 && k <= 10 && !DICE) && !(k >= 12 && X4 == X4_NONE))
    atomicAdd(&sums[(size_t)((blockIdx.x + blockIdx.y) % SP_REDUCE_ROWS) * 16 + k], (double)sp_cols_sum(red, 16, 4, k));
}
// one thread: the loss and the backward's coefficients
//   coef: 0 hinge scale 1 / (N (5 + f)); (1, 2) (3, 4) (5, 6) Dice (ca, cb) / (5 + f) of c, p, l (0 without a Dice term); 7 latent scale
//   f / (nlat (5 + f)); and, only when the caller's buffer holds ncoef = 11 floats, 8-10 = bce_weight / (N (5 + f)) (0 without BCE)
__global__ void cae_crit_finalize_kernel(const double* __restrict__ sums, int64_t nlat, double N, float w, float wb, int terms, int ncoef,
                                         double eps, float factor, float* __restrict__ loss, float* __restrict__ coef) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double lat = nlat > 0 ? sp_rows_sum(sums, 11, 16) / (double)nlat : 0.0;
  const double den0 = 5.0 + (double)factor;
  double acc = sp_rows_sum(sums, 0, 16) / N + sp_rows_sum(sums, 1, 16) / N;
  for (int k = 0; k < 3; ++k) {
    float ca = 0.f, cb = 0.f, cc = 0.f;
    if (terms & SP_VLOSS_DICE) {
      const double num = 2.0 * sp_rows_sum(sums, 2 + 3 * k, 16) + eps;
      const double den = sp_rows_sum(sums, 3 + 3 * k, 16) + sp_rows_sum(sums, 4 + 3 * k, 16) + eps;
      acc += 1.0 - (double)w * num / den;
      ca = (float)(-2.0 * w / den / den0);
      cb = (float)(2.0 * w * num / (den * den) / den0);
    }
    if (terms & SP_VLOSS_BCE) {
      acc += (double)wb * sp_rows_sum(sums, 12 + k, 16) / N;
      cc = (float)((double)wb / (N * den0));
    }
    coef[1 + 2 * k] = ca; coef[2 + 2 * k] = cb;
    if (ncoef == 11) coef[8 + k] = cc;
  }
  acc += (double)factor * lat;
  *loss = (float)(acc / den0);
  coef[0] = (float)(1.0 / (N * den0));
  coef[7] = nlat > 0 ? (float)((double)factor / ((double)nlat * den0)) : 0.f;
}
// gradients of the four reconstructions (dense (B, DHW) each, at dc / dp / dl / di) and of the two latents; up: dL/dloss on the device.
// BCE: coef[8..10] hold a BCE term -- read from the coefficients (the backward's argument list carries no terms), uniform over the
// launch; the Dice-only loop pays no division and reads no coefficient past coef[7]
template <bool BCE>
__device__ __forceinline__ void cae_crit_bwd_loop(const float* __restrict__ c, const float* __restrict__ p, const float* __restrict__ l,
                                                  const float* __restrict__ ii, const float* __restrict__ tc, const float* __restrict__ tp,
                                                  const float* __restrict__ tl, int64_t DHW, const float* __restrict__ coef, float go,
                                                  float* __restrict__ dc, float* __restrict__ dp, float* __restrict__ dl, float* __restrict__ di) {
  constexpr int X4 = BCE ? X4_BCE : X4_NONE;
  const float hs = coef[0] * go;
  const float cac = coef[1] * go, cbc = coef[2] * go, cap = coef[3] * go, cbp = coef[4] * go, cal = coef[5] * go, cbl = coef[6] * go;
  const float ccc = BCE ? coef[8] * go : 0.f, ccp = BCE ? coef[9] * go : 0.f, ccl = BCE ? coef[10] * go : 0.f;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < DHW; v += (int64_t)gridDim.x * 256) {
    const float vc = c[v], vp = p[v], vl = l[v], vi = ii[v];
    const float d1 = vp - vi, d2 = vp - vc;
    const float g1 = ((d1 > 0.f ? 1.f : (d1 < 0.f ? -1.f : 0.f)) - 1.f) * hs;      // d/dd (|d| - d), sign(0) = 0 as torch.abs
    const float g2 = ((d2 > 0.f ? 1.f : (d2 < 0.f ? -1.f : 0.f)) - 1.f) * hs;
    dp[v] = g1 + g2 + crit_grad<X4>(vp, tp[v], 0.f, cap, cbp, ccp);
    di[v] = -g1;
    dc[v] = -g2 + crit_grad<X4>(vc, tc[v], 0.f, cac, cbc, ccc);
    dl[v] = crit_grad<X4>(vl, tl[v], 0.f, cal, cbl, ccl);
  }
}
__global__ __launch_bounds__(256) void cae_crit_bwd_kernel(const float* __restrict__ c, int64_t cbs, const float* __restrict__ p, int64_t pbs,
                                                           const float* __restrict__ l, int64_t lbs, const float* __restrict__ ii, int64_t ibs,
                                                           const float* __restrict__ tc, int64_t tcbs, const float* __restrict__ tp, int64_t tpbs,
                                                           const float* __restrict__ tl, int64_t tlbs, int64_t DHW, int B, const float* __restrict__ coef,
                                                           int ncoef, const float* __restrict__ up, float* __restrict__ dc, float* __restrict__ dp,
                                                           float* __restrict__ dl, float* __restrict__ di, const float* __restrict__ zi,
                                                           const float* __restrict__ zl, int64_t nlat, float* __restrict__ dzi, float* __restrict__ dzl) {
  const float go = up[0];
  if ((int)blockIdx.y == B) {      // the latents
    const float ls = coef[7] * go;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < nlat; k += (int64_t)gridDim.x * 256) {
      const float d = zi[k] - zl[k];
      const float g = d > 0.f ? ls : (d < 0.f ? -ls : 0.f);
      dzi[k] = g; dzl[k] = -g;
    }
    return;
  }
  const int b = blockIdx.y;
  c += b * cbs; p += b * pbs; l += b * lbs; ii += b * ibs; tc += b * tcbs; tp += b * tpbs; tl += b * tlbs;
  dc += (int64_t)b * DHW; dp += (int64_t)b * DHW; dl += (int64_t)b * DHW; di += (int64_t)b * DHW;
  if (ncoef == 11 && coef[8] != 0.f) cae_crit_bwd_loop<true>(c, p, l, ii, tc, tp, tl, DHW, coef, go, dc, dp, dl, di);
  else cae_crit_bwd_loop<false>(c, p, l, ii, tc, tp, tl, DHW, coef, go, dc, dp, dl, di);
}
// ncoef: the floats the entry point's coef buffer holds -- 8 behind sp_cae_loss_fwd / _bwd, 11 behind sp_cae_loss_crit_fwd / _bwd
static int cae_loss_fwd_impl(const char* who, const float* c, int64_t cbs, const float* p, int64_t pbs, const float* l, int64_t lbs, const float* i,
                             int64_t ibs, const float* tc, int64_t tcbs, const float* tp, int64_t tpbs, const float* tl, int64_t tlbs, int32_t B,
                             int64_t DHW, const float* zi, const float* zl, int64_t nlat, float dice_weight, float bce_weight, int32_t terms,
                             int ncoef, double eps, float factor, double* sums, float* loss, float* coef, sp_stream_t stream) {
  SP_CHECK_ARG(c && p && l && i && tc && tp && tl && sums && loss && coef && B >= 1 && B <= 65534 && DHW >= 1 && (nlat == 0 || (zi && zl)) &&
               terms >= 1 && terms <= (SP_VLOSS_DICE | SP_VLOSS_BCE), "%s: bad arguments", who);
  int64_t gx = (DHW + 256 * 8 - 1) / (256 * 8);
  if (gx > 256) gx = 256;
#define SP_CAE_CRIT_SUMS(T) hipLaunchKernelGGL(cae_crit_sums_kernel<T>, dim3((unsigned)gx, B + (nlat > 0 ? 1 : 0)), dim3(256), 0, ST(stream), c, cbs, p, pbs, l, lbs, i, ibs, \
                                               tc, tcbs, tp, tpbs, tl, tlbs, DHW, sums, B, zi, zl, nlat)
  if (terms == 1) SP_CAE_CRIT_SUMS(1);
  else if (terms == 2) SP_CAE_CRIT_SUMS(2);
  else SP_CAE_CRIT_SUMS(3);
#undef SP_CAE_CRIT_SUMS
  hipLaunchKernelGGL(cae_crit_finalize_kernel, dim3(1), dim3(64), 0, ST(stream), sums, nlat, (double)B * (double)DHW, dice_weight, bce_weight, terms, ncoef,
                     eps, factor, loss, coef);
  SP_CHECK_LAUNCH(who);
  return SP_OK;
}
static int cae_loss_bwd_impl(const char* who, const float* c, int64_t cbs, const float* p, int64_t pbs, const float* l, int64_t lbs, const float* i,
                             int64_t ibs, const float* tc, int64_t tcbs, const float* tp, int64_t tpbs, const float* tl, int64_t tlbs, int32_t B,
                             int64_t DHW, const float* coef, int ncoef, const float* up, float* dc, float* dp, float* dl, float* di, const float* zi,
                             const float* zl, int64_t nlat, float* dzi, float* dzl, sp_stream_t stream) {
  SP_CHECK_ARG(c && p && l && i && tc && tp && tl && coef && up && dc && dp && dl && di && B >= 1 && B <= 65534 && DHW >= 1 && (nlat == 0 || (zi && zl && dzi && dzl)),
               "%s: bad arguments", who);
  int64_t gx = (DHW + 256 * 8 - 1) / (256 * 8);
  if (gx > 256) gx = 256;
  hipLaunchKernelGGL(cae_crit_bwd_kernel, dim3((unsigned)gx, B + (nlat > 0 ? 1 : 0)), dim3(256), 0, ST(stream), c, cbs, p, pbs, l, lbs, i, ibs, tc, tcbs, tp, tpbs,
                     tl, tlbs, DHW, B, coef, ncoef, up, dc, dp, dl, di, zi, zl, nlat, dzi, dzl);
  SP_CHECK_LAUNCH(who);
  return SP_OK;
}
extern "C" int sp_cae_loss_fwd(const float* c, int64_t cbs, const float* p, int64_t pbs, const float* l, int64_t lbs, const float* i, int64_t ibs,
                               const float* tc, int64_t tcbs, const float* tp, int64_t tpbs, const float* tl, int64_t tlbs, int32_t B, int64_t DHW,
                               const float* zi, const float* zl, int64_t nlat, float dice_weight, double eps, float factor, double* sums,
                               float* loss, float* coef, sp_stream_t stream) {
  return cae_loss_fwd_impl("sp_cae_loss_fwd", c, cbs, p, pbs, l, lbs, i, ibs, tc, tcbs, tp, tpbs, tl, tlbs, B, DHW, zi, zl, nlat, dice_weight, 0.f,
                           SP_VLOSS_DICE, 8, eps, factor, sums, loss, coef, stream);
}
extern "C" int sp_cae_loss_bwd(const float* c, int64_t cbs, const float* p, int64_t pbs, const float* l, int64_t lbs, const float* i, int64_t ibs,
                               const float* tc, int64_t tcbs, const float* tp, int64_t tpbs, const float* tl, int64_t tlbs, int32_t B, int64_t DHW,
                               const float* coef, const float* up, float* dc, float* dp, float* dl, float* di, const float* zi, const float* zl,
                               int64_t nlat, float* dzi, float* dzl, sp_stream_t stream) {
  return cae_loss_bwd_impl("sp_cae_loss_bwd", c, cbs, p, pbs, l, lbs, i, ibs, tc, tcbs, tp, tpbs, tl, tlbs, B, DHW, coef, 8, up, dc, dp, dl, di, zi, zl,
                           nlat, dzi, dzl, stream);
}
extern "C" int sp_cae_loss_crit_fwd(const float* c, int64_t cbs, const float* p, int64_t pbs, const float* l, int64_t lbs, const float* i, int64_t ibs,
                                    const float* tc, int64_t tcbs, const float* tp, int64_t tpbs, const float* tl, int64_t tlbs, int32_t B, int64_t DHW,
                                    const float* zi, const float* zl, int64_t nlat, float dice_weight, float bce_weight, int32_t terms, double eps,
                                    float factor, double* sums, float* loss, float* coef, sp_stream_t stream) {
  return cae_loss_fwd_impl("sp_cae_loss_crit_fwd", c, cbs, p, pbs, l, lbs, i, ibs, tc, tcbs, tp, tpbs, tl, tlbs, B, DHW, zi, zl, nlat, dice_weight,
                           bce_weight, terms, 11, eps, factor, sums, loss, coef, stream);
}
extern "C" int sp_cae_loss_crit_bwd(const float* c, int64_t cbs, const float* p, int64_t pbs, const float* l, int64_t lbs, const float* i, int64_t ibs,
                                    const float* tc, int64_t tcbs, const float* tp, int64_t tpbs, const float* tl, int64_t tlbs, int32_t B, int64_t DHW,
                                    const float* coef, const float* up, float* dc, float* dp, float* dl, float* di, const float* zi, const float* zl,
                                    int64_t nlat, float* dzi, float* dzl, sp_stream_t stream) {
  return cae_loss_bwd_impl("sp_cae_loss_crit_bwd", c, cbs, p, pbs, l, lbs, i, ibs, tc, tcbs, tp, tpbs, tl, tlbs, B, DHW, coef, 11, up, dc, dp, dl, di, zi,
                           zl, nlat, dzi, dzl, stream);
}
