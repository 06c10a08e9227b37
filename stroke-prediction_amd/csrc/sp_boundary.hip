// The boundary (signed-distance) criteria (include/stroke_amd.h; Kervadec et al., MIDL 2019: loss = mean(o * phi(t))):
//   * sp_signed_distance_batch: phi of every (sample, channel) volume of a label batch -- outside the mask the Euclidean distance to
//     it, inside -(distance to the background - 1), zero for an empty or a full mask -- on the exact separable transform of sp_edt.h.
//     The two transforms of all B * C volumes are one (2 B C D, H, W) stack: a seed launch, a launch per axis, a launch for the roots;
//   * sp_bloss_sums / _finalize_clear / _bwd: the sp_vloss_* triple (sp_elem.hip) with phi as a third input and sum o*phi as the
//     fourth moment; the boundary weight's scalar is read from device memory, so a captured step follows its schedule.
// All of it is bandwidth- or latency-bound elementwise work; nothing here depends on the 16-bit storage type.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sp_common.h"
#include "sp_edt.h"

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define BD_PARTS 64          // seed workgroups per volume at most: one count each, added up by one wave of the roots' launch
#define BD_MAX_BLOCKS 4096

// ------------------------------------------------------------------------------------------------ signed distance
// g[0][bc][v] = 0 on the mask (the transform gives the distance TO the mask), g[1][bc][v] = 0 off the mask (the distance to the
// background); SP_SD_BIG elsewhere.  grid.y = b*C + c, grid.x strides over the volume; part[bc][blockIdx.x] = voxels of the mask this
// workgroup saw: written, not added -- no zeroing, no atomics, and an integer total does not depend on the order
__global__ __launch_bounds__(256) void bd_seed_kernel(const float* __restrict__ t, int64_t tbs, int C, int64_t DHW, int64_t N,
                                                      float* __restrict__ g, unsigned int* __restrict__ part) {
  const int bc = blockIdx.y, c = bc % C, b = bc / C;
  const float* tp = t + (int64_t)b * tbs + (int64_t)c * DHW;
  float* g0 = g + (int64_t)bc * DHW;
  float* g1 = g0 + N;
  unsigned int n = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < DHW; i += (int64_t)gridDim.x * 256) {
    const bool m = tp[i] > 0.5f;
    g0[i] = m ? 0.f : SP_SD_BIG;
    g1[i] = m ? SP_SD_BIG : 0.f;
    n += m;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  __shared__ unsigned int red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) part[(int64_t)bc * BD_PARTS + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void bd_edt_axis_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t total, int n,
                                                          int64_t inner) {
  sp_edt_axis(src, dst, total, n, inner);
}

// phi = mask ? 0 - (sqrt(g1) - 1) : sqrt(g0), in fp64 and rounded once (the squares are exact integers); 0 for a volume whose mask
// holds none or all of its voxels.  The first wave adds the volume's nparts counts; the mask is read off the targets again.
__global__ __launch_bounds__(256) void bd_phi_kernel(const float* __restrict__ t, int64_t tbs, const float* __restrict__ g, int C, int64_t DHW,
                                                     int64_t N, const unsigned int* __restrict__ part, int nparts, float* __restrict__ phi) {
  const int bc = blockIdx.y, c = bc % C, b = bc / C;
  __shared__ unsigned long long tot;
  if (threadIdx.x < 64) {
    unsigned long long n = (int)threadIdx.x < nparts ? part[(int64_t)bc * BD_PARTS + threadIdx.x] : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (threadIdx.x == 0) tot = n;
  }
  __syncthreads();
  const bool degenerate = tot == 0ull || tot == (unsigned long long)DHW;
  const float* tp = t + (int64_t)b * tbs + (int64_t)c * DHW;
  const float* g0 = g + (int64_t)bc * DHW;
  const float* g1 = g0 + N;
  float* pp = phi + (int64_t)bc * DHW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < DHW; i += (int64_t)gridDim.x * 256) {
    float v = 0.f;
    if (!degenerate) v = tp[i] > 0.5f ? (float)(0.0 - (sqrt((double)g1[i]) - 1.0)) : (float)sqrt((double)g0[i]);
    pp[i] = v;
  }
}

static int bd_check_extents(int32_t B, int32_t C, int32_t D, int32_t H, int32_t W, const char* who) {
  SP_CHECK_ARG(B >= 1 && C >= 1 && D >= 1 && H >= 1 && W >= 1, "%s: bad sizes B=%d C=%d (D, H, W)=(%d, %d, %d)", who, B, C, D, H, W);
  SP_CHECK_ARG(D < 4096 && H < 4096 && W < 4096, "%s: extent of 4096 or more", who);
  SP_CHECK_ARG((int64_t)B * C <= 65535, "%s: B * C = %lld > 65535", who, (long long)B * C);
  SP_CHECK_ARG((int64_t)D * H * W < (1ll << 31) && (int64_t)B * C * D * H * W < (1ll << 36), "%s: batch too large", who);
  return SP_OK;
}

extern "C" int sp_signed_distance_batch_workspace(int32_t B, int32_t C, int32_t D, int32_t H, int32_t W, int64_t* floats) {
  SP_CHECK_ARG(floats, "sp_signed_distance_batch_workspace: null pointer");
  const int rc = bd_check_extents(B, C, D, H, W, "sp_signed_distance_batch_workspace");
  if (rc) return rc;
  *floats = 4 * (int64_t)B * C * D * H * W + (int64_t)BD_PARTS * B * C;
  return SP_OK;
}

extern "C" int sp_signed_distance_batch(const float* t, int64_t t_bstride, int32_t B, int32_t C, int32_t D, int32_t H, int32_t W, float* phi,
                                        float* ws, int64_t ws_floats, sp_stream_t stream) {
  SP_CHECK_ARG(t && phi && ws, "sp_signed_distance_batch: null pointer");
  const int rc = bd_check_extents(B, C, D, H, W, "sp_signed_distance_batch");
  if (rc) return rc;
  const int64_t dhw = (int64_t)D * H * W, N = (int64_t)B * C * dhw, need = 4 * N + (int64_t)BD_PARTS * B * C;
  SP_CHECK_ARG(B == 1 || t_bstride >= C * dhw, "sp_signed_distance_batch: batch stride %lld below C * D * H * W = %lld", (long long)t_bstride,
               (long long)(C * dhw));
  SP_CHECK_ARG(ws_floats >= need, "sp_signed_distance_batch: workspace of %lld floats, %lld needed", (long long)ws_floats, (long long)need);
  hipStream_t st = ST(stream);
  float* a = ws;
  float* b = ws + 2 * N;
  unsigned int* part = reinterpret_cast<unsigned int*>(ws + 4 * N);
  int64_t nparts = (dhw + 256 * 8 - 1) / (256 * 8);
  if (nparts > BD_PARTS) nparts = BD_PARTS;
  hipLaunchKernelGGL(bd_seed_kernel, dim3((unsigned)nparts, B * C), dim3(256), 0, st, t, t_bstride, C, dhw, N, a, part);
  // (2 B C D, H, W) scanned along W, H, then D: the volume index is part of the outer index, no line crosses into the next volume
  const int ext[3] = {D, H, W};
  const unsigned grid2 = (unsigned)((2 * N + 255) / 256);
  int64_t inner = 1;
  for (int ax = 2; ax >= 0; --ax) {
    if (ext[ax] > 1) {
      hipLaunchKernelGGL(bd_edt_axis_kernel, dim3(grid2), dim3(256), 0, st, (const float*)a, b, 2 * N, ext[ax], inner);
      float* s = a; a = b; b = s;
    }
    inner *= ext[ax];
  }
  int64_t gx = (dhw + 255) / 256, cap = BD_MAX_BLOCKS / ((int64_t)B * C);
  if (cap < 1) cap = 1;
  if (gx > cap) gx = cap;
  hipLaunchKernelGGL(bd_phi_kernel, dim3((unsigned)gx, B * C), dim3(256), 0, st, t, t_bstride, (const float*)a, C, dhw, N,
                     (const unsigned int*)part, (int)nparts, phi);
  SP_CHECK_LAUNCH("sp_signed_distance_batch");
  return SP_OK;
}

// ------------------------------------------------------------------------------------------------ sums, finalize, backward
template <bool DICE> __device__ __forceinline__ void bloss_acc(float a, float b, float p, float (&s)[4]) {
  if (DICE) { s[0] += a * b; s[1] += a * a; s[2] += b * b; }
  s[3] += a * p;
}
// sums[c] = (sum o*t, sum o*o, sum t*t, sum o*phi) over batch and volume; the grid, the layout and the reduction order of
// vloss_sums_kernel: per-thread fp32, wave sum, the four waves in order, one fp64 atomic per workgroup and column into a replica row.
// VEC: DHW % 4 == 0 and every row base 16-byte aligned (checked by the launcher) -> one 16-byte load per lane and operand.
template <bool DICE, bool VEC>
__global__ __launch_bounds__(256) void bloss_sums_kernel(const float* __restrict__ o, int64_t obs, const float* __restrict__ t, int64_t tbs,
                                                         const float* __restrict__ phi, int C, int64_t DHW, double* __restrict__ sums) {
  const int bc = blockIdx.y, c = bc % C, b = bc / C;
  const float* op = o + (int64_t)b * obs + (int64_t)c * DHW;
  const float* tp = t + (int64_t)b * tbs + (int64_t)c * DHW;
  const float* pp = phi + (int64_t)bc * DHW;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if (VEC) {
    const float4* o4 = reinterpret_cast<const float4*>(op);
    const float4* t4 = reinterpret_cast<const float4*>(tp);
    const float4* p4 = reinterpret_cast<const float4*>(pp);
    const int64_t n4 = DHW >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
      const float4 a = o4[i], p = p4[i];
      float4 bb = make_float4(0.f, 0.f, 0.f, 0.f);
      if (DICE) bb = t4[i];
      bloss_acc<DICE>(a.x, bb.x, p.x, s); bloss_acc<DICE>(a.y, bb.y, p.y, s); bloss_acc<DICE>(a.z, bb.z, p.z, s); bloss_acc<DICE>(a.w, bb.w, p.w, s);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < DHW; i += (int64_t)gridDim.x * 256)
      bloss_acc<DICE>(op[i], DICE ? tp[i] : 0.f, pp[i], s);
  }
  __shared__ float red[4 * 4];      // [wave][moment], added up in wave order (sp_cols_sum)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!DICE && k < 3) continue;
    const float w = wave_sum(s[k]);
    if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * 4 + k] = w;
  }
  __syncthreads();
  if (threadIdx.x < 4 && (DICE || threadIdx.x == 3))
    atomicAdd(&sums[(size_t)((blockIdx.x + blockIdx.y) % SP_REDUCE_ROWS) * SP_BLOSS_PITCH(C) + c * 4 + threadIdx.x], (double)sp_cols_sum(red, 4, 4, threadIdx.x));
}
static inline bool bloss_vec_ok(const void* p, int64_t bstride, int B, int64_t DHW) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && DHW % 4 == 0 && (B == 1 || bstride % 4 == 0);
}
static inline bool bloss_args_ok(const float* o, int64_t obs, const float* t, int64_t tbs, const float* phi, int32_t B, int32_t C, int64_t DHW) {
  return o && t && phi && B >= 1 && C >= 1 && DHW >= 1 && (int64_t)B * C <= 65535 && obs >= C * DHW && tbs >= C * DHW;
}
extern "C" int sp_bloss_sums(const float* o, int64_t o_bstride, const float* t, int64_t t_bstride, const float* phi, int32_t B, int32_t C,
                             int64_t DHW, int32_t dice, double* sums, sp_stream_t stream) {
  SP_CHECK_ARG(bloss_args_ok(o, o_bstride, t, t_bstride, phi, B, C, DHW) && sums && (dice == 0 || dice == 1), "sp_bloss_sums: bad arguments");
  int64_t gx = (DHW + 256 * 8 - 1) / (256 * 8);
  if (gx > 256) gx = 256;
  const bool vec = bloss_vec_ok(o, o_bstride, B, DHW) && bloss_vec_ok(t, t_bstride, B, DHW) && bloss_vec_ok(phi, 0, 1, DHW);
#define SP_BLOSS_SUMS(D_, V_) hipLaunchKernelGGL((bloss_sums_kernel<D_, V_>), dim3((unsigned)gx, B * C), dim3(256), 0, ST(stream), o, o_bstride, t, t_bstride, phi, C, DHW, sums)
  if (dice) { if (vec) SP_BLOSS_SUMS(true, true); else SP_BLOSS_SUMS(true, false); }
  else { if (vec) SP_BLOSS_SUMS(false, true); else SP_BLOSS_SUMS(false, false); }
#undef SP_BLOSS_SUMS
  SP_CHECK_LAUNCH("sp_bloss_sums");
  return SP_OK;
}
// one thread: the loss and the backward's coefficients (ca, cb, cd) per channel; then all threads zero the replica rows again
__global__ void bloss_finalize_kernel(double* __restrict__ sums, const float* __restrict__ wd, const float* __restrict__ wb,
                                      const float* __restrict__ scale, double eps, double count, int C, float* __restrict__ loss,
                                      float* __restrict__ coef) {
  const int pitch = SP_BLOSS_PITCH(C);
  if (threadIdx.x == 0) {
    const double sc = (double)scale[0];
    double dice = 0.0, bnd = 0.0;
    for (int c = 0; c < C; ++c) {
      float ca = 0.f, cb = 0.f;
      if (wd) {
        const double num = 2.0 * sp_rows_sum(sums, c * 4, pitch) + eps;
        const double den = sp_rows_sum(sums, c * 4 + 1, pitch) + sp_rows_sum(sums, c * 4 + 2, pitch) + eps;
        dice += (double)wd[c] * num / den;
        ca = (float)(-2.0 * wd[c] / den);
        cb = (float)(2.0 * wd[c] * num / (den * den));
      }
      const double w = (double)wb[c] * sc;
      bnd += w * sp_rows_sum(sums, c * 4 + 3, pitch) / count;
      coef[3 * c] = ca; coef[3 * c + 1] = cb; coef[3 * c + 2] = (float)(w / count);
    }
    *loss = (float)((wd ? 1.0 - dice : 0.0) + bnd);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < SP_REDUCE_ROWS * pitch; k += blockDim.x) sums[k] = 0.0;
}
extern "C" int sp_bloss_finalize_clear(double* sums, const float* w_dice, const float* w_boundary, const float* scale, double eps, double count,
                                       int32_t C, float* loss, float* coef, sp_stream_t stream) {
  SP_CHECK_ARG(sums && w_boundary && scale && loss && coef && C >= 1 && count > 0.0, "sp_bloss_finalize_clear: bad arguments");
  hipLaunchKernelGGL(bloss_finalize_kernel, dim3(1), dim3(64), 0, ST(stream), sums, w_dice, w_boundary, scale, eps, count, C, loss, coef);
  SP_CHECK_LAUNCH("sp_bloss_finalize_clear");
  return SP_OK;
}
// do[b,c,v] = up * (ca[c]*t + cb[c]*o + cd[c]*phi); grid as bloss_sums_kernel: the coefficients are uniform over a workgroup
template <bool VEC>
__global__ __launch_bounds__(256) void bloss_bwd_kernel(const float* __restrict__ o, int64_t obs, const float* __restrict__ t, int64_t tbs,
                                                        const float* __restrict__ phi, const float* __restrict__ coef,
                                                        const float* __restrict__ upstream, int C, int64_t DHW, float* __restrict__ d) {
  const int bc = blockIdx.y, c = bc % C, b = bc / C;
  const float up = upstream ? *upstream : 1.f;
  const float ca = up * coef[3 * c], cb = up * coef[3 * c + 1], cd = up * coef[3 * c + 2];
  const float* op = o + (int64_t)b * obs + (int64_t)c * DHW;
  const float* tp = t + (int64_t)b * tbs + (int64_t)c * DHW;
  const float* pp = phi + (int64_t)bc * DHW;
  float* dp = d + (int64_t)bc * DHW;
  if (VEC) {
    const float4* o4 = reinterpret_cast<const float4*>(op);
    const float4* t4 = reinterpret_cast<const float4*>(tp);
    const float4* p4 = reinterpret_cast<const float4*>(pp);
    float4* d4 = reinterpret_cast<float4*>(dp);
    const int64_t n4 = DHW >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
      const float4 a = o4[i], bb = t4[i], p = p4[i];
      d4[i] = make_float4(ca * bb.x + cb * a.x + cd * p.x, ca * bb.y + cb * a.y + cd * p.y, ca * bb.z + cb * a.z + cd * p.z,
                          ca * bb.w + cb * a.w + cd * p.w);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < DHW; i += (int64_t)gridDim.x * 256) dp[i] = ca * tp[i] + cb * op[i] + cd * pp[i];
  }
}
extern "C" int sp_bloss_bwd(const float* o, int64_t o_bstride, const float* t, int64_t t_bstride, const float* phi, const float* coef,
                            const float* upstream, int32_t B, int32_t C, int64_t DHW, float* dout, sp_stream_t stream) {
  SP_CHECK_ARG(bloss_args_ok(o, o_bstride, t, t_bstride, phi, B, C, DHW) && coef && dout, "sp_bloss_bwd: bad arguments");
  const bool vec = bloss_vec_ok(o, o_bstride, B, DHW) && bloss_vec_ok(t, t_bstride, B, DHW) && bloss_vec_ok(phi, 0, 1, DHW) && bloss_vec_ok(dout, 0, 1, DHW);
  const int64_t per = vec ? 256 * 4 : 256;                                  // elements per workgroup and trip
  int64_t gx = (DHW + per - 1) / per, cap = BD_MAX_BLOCKS / ((int64_t)B * C);
  if (cap < 1) cap = 1;
  if (gx > cap) gx = cap;
  if (vec) hipLaunchKernelGGL(bloss_bwd_kernel<true>, dim3((unsigned)gx, B * C), dim3(256), 0, ST(stream), o, o_bstride, t, t_bstride, phi, coef, upstream, C, DHW, dout);
  else hipLaunchKernelGGL(bloss_bwd_kernel<false>, dim3((unsigned)gx, B * C), dim3(256), 0, ST(stream), o, o_bstride, t, t_bstride, phi, coef, upstream, C, DHW, dout);
  SP_CHECK_LAUNCH("sp_bloss_bwd");
  return SP_OK;
}
