// Batch-level elastic deformation (common/data.py:BatchElasticDeform): what ElasticDeform does once per sample and channel
// with nine filter launches, a warp and an uploaded noise field each, done for a whole collated batch in five launches:
//   sp_rng_uniform_pm1           one launch   counter-based Philox4x32-10 noise in [-1, 1) for every field
//   sp_gaussian_filter3d_batch   three        scipy.ndimage.gaussian_filter(mode="constant") of all fields, one launch per axis
//   sp_elastic_warp_batch        one          trilinear warp of every channel volume by its three fields, optional x mirror
// Volumes are stored as the collated batch holds them: (Z, Y, X) fp32, X contiguous.  "Voxel (x, y, z)" is what the
// per-sample path (sp_transform.hip) holds at [x, y, z] of its (n0, n1, n2) array: its axis 0 is X here, its axis 2 is Z.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sp_common.h"
#include "sp_gauss.h"
#include "sp_philox.h"

#define ST(s) reinterpret_cast<hipStream_t>(s)

// ------------------------------------------------------------------------------------------------ Philox4x32-10
// Philox4x32-10 (sp_philox.h).  Key (seed lo, seed hi); counter (e >> 2, field, call lo, call hi); element e takes word e & 3 of
// its block: the value depends on (seed, call, field, e) alone, never on the launch.
// one thread per Philox block = four consecutive elements of one field; grid (blocks per field, fields)
__global__ __launch_bounds__(256) void rng_uniform_pm1_kernel(float* __restrict__ dst, int64_t per_field, uint32_t k0, uint32_t k1,
                                                              uint32_t call_lo, uint32_t call_hi, int vec4) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t e0 = q * 4;
  if (e0 >= per_field) return;
  const uint32_t field = blockIdx.y;
  uint32_t w[4];
  philox4x32_10((uint32_t)q, field, call_lo, call_hi, k0, k1, w);
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = 2.f * ((float)(w[i] >> 8) * 5.9604644775390625e-08f) - 1.f;      // u = 24 bits * 2^-24: all exact
  float* p = dst + (int64_t)field * per_field + e0;
  if (vec4) {      // per_field a multiple of 4 and dst 16-byte aligned: every block of every field is one aligned float4
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (e0 + i < per_field) p[i] = v[i];
  }
}

extern "C" int sp_rng_uniform_pm1(float* dst, int32_t nfields, int64_t per_field, int64_t seed_bits, int64_t call_bits, sp_stream_t stream) {
  const uint64_t seed = (uint64_t)seed_bits, call = (uint64_t)call_bits;      // the ABI carries the 64 bits as int64_t
  SP_CHECK_ARG(dst && nfields >= 1 && nfields <= 65535 && per_field >= 1 && per_field < (1ll << 31),
               "sp_rng_uniform_pm1: bad arguments (1 <= nfields <= 65535, 1 <= per_field < 2^31)");
  const int64_t blocks = (per_field + 3) / 4;
  const int vec4 = (per_field % 4 == 0) && (reinterpret_cast<uintptr_t>(dst) % 16 == 0);
  hipLaunchKernelGGL(rng_uniform_pm1_kernel, dim3((unsigned)((blocks + 255) / 256), (unsigned)nfields), dim3(256), 0, ST(stream), dst,
                     per_field, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), (uint32_t)(call & 0xffffffffu),
                     (uint32_t)(call >> 32), vec4);
  SP_CHECK_LAUNCH("sp_rng_uniform_pm1");
  return SP_OK;
}

// ------------------------------------------------------------------------------------------------ batched Gaussian filter
// Each pass stages its input tile plus a halo of `radius` in LDS, so an input element is fetched once per tile instead of once
// per tap.  Whatever lies outside the line (the volume's border -- and with it the neighbouring field, because a line never
// leaves its field) is staged as 0: fmaf(w, 0, acc) == acc, so summing ALL 2 radius + 1 taps lowest to highest gives the very
// bits of gauss1d_kernel's clipped loop.  The lanes of a wave read consecutive LDS words for every tap: no bank conflicts.
#define GX_TX 128      // x pass: outputs per row of a tile (a thread owns one column of every second row)
#define GX_ROWS 8      // x pass: rows per tile
#define GS_TL 32       // strided pass: outputs along the filtered axis per tile
#define GS_TI 64       // strided pass: contiguous elements per tile row (one wave's width)

// pass along X, the contiguous axis: `rows` lines of X elements (rows = nfields * Z * Y); grid (row tiles, x tiles)
__global__ __launch_bounds__(256) void gauss_x_batch_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t rows, int X,
                                                            int radius, GaussW gw) {
  extern __shared__ float s[];
  const int pitch = GX_TX + 2 * radius;
  const int64_t row0 = (int64_t)blockIdx.x * GX_ROWS;
  const int x0 = blockIdx.y * GX_TX;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = wave; r < GX_ROWS; r += 4) {
    const int64_t row = row0 + r;
    for (int c = lane; c < pitch; c += 64) {
      const int x = x0 - radius + c;
      s[r * pitch + c] = (row < rows && x >= 0 && x < X) ? src[row * X + x] : 0.f;
    }
  }
  __syncthreads();
  const int tx = threadIdx.x & (GX_TX - 1), ty = threadIdx.x >> 7;
  if (x0 + tx >= X) return;
  for (int r = ty; r < GX_ROWS; r += 2) {
    const int64_t row = row0 + r;
    if (row >= rows) break;
    const float* p = s + r * pitch + tx;      // tap t of output tx sits at p[t + radius]
    float acc = 0.f;
    for (int t = 0; t <= 2 * radius; ++t) acc = fmaf(gw.w[t], p[t], acc);
    dst[row * X + x0 + tx] = acc;
  }
}

// pass along an axis of extent `len` and stride `inner` > 1 in an (outer, len, inner) view: Y (outer = nfields * Z, inner = X)
// or Z (outer = nfields, inner = Y * X).  grid (outer * inner tiles, len tiles)
__global__ __launch_bounds__(256) void gauss_strided_batch_kernel(const float* __restrict__ src, float* __restrict__ dst, int len,
                                                                  int64_t inner, int n_itiles, int radius, GaussW gw) {
  extern __shared__ float s[];
  const int64_t o = blockIdx.x / n_itiles;
  const int it = blockIdx.x - (int)(o * n_itiles);
  const int l0 = blockIdx.y * GS_TL;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = (int64_t)it * GS_TI + lane;
  const bool live = i < inner;
  const int64_t base = o * len * inner + i;
  for (int l = wave; l < GS_TL + 2 * radius; l += 4) {
    const int L = l0 - radius + l;
    s[l * GS_TI + lane] = (live && L >= 0 && L < len) ? src[base + L * inner] : 0.f;
  }
  __syncthreads();
  if (!live) return;
  for (int l = wave; l < GS_TL; l += 4) {
    const int L = l0 + l;
    if (L >= len) break;
    const float* p = s + l * GS_TI + lane;      // tap t of output l sits in row l + t
    float acc = 0.f;
    for (int t = 0; t <= 2 * radius; ++t) acc = fmaf(gw.w[t], p[t * GS_TI], acc);
    dst[base + L * inner] = acc;
  }
}

extern "C" int sp_gaussian_filter3d_batch(const float* src, float* dst, float* tmp, int32_t nfields, int32_t Z, int32_t Y, int32_t X,
                                          float sigma, float truncate, sp_stream_t stream) {
  SP_CHECK_ARG(src && dst && tmp && tmp != src && tmp != dst && src != dst && nfields >= 1 && Z >= 1 && Y >= 1 && X >= 1 && sigma > 0.f &&
                   truncate > 0.f,
               "sp_gaussian_filter3d_batch: bad arguments");
  const int radius = sp_gauss_radius(sigma, truncate);
  SP_CHECK_ARG(radius <= SP_GAUSS_MAX_RADIUS, "sp_gaussian_filter3d_batch: radius %d above %d", radius, SP_GAUSS_MAX_RADIUS);
  GaussW gw;
  sp_gauss_weights(sigma, radius, &gw);
  const int64_t plane = (int64_t)Y * X, rows = (int64_t)nfields * Z * Y;
  hipStream_t st = ST(stream);
  // x: src -> dst
  const int64_t gx = (rows + GX_ROWS - 1) / GX_ROWS, gxt = (X + GX_TX - 1) / GX_TX;
  // y: dst -> tmp, lines of one (field, z) plane; z: tmp -> dst, lines of one field
  const int64_t yt = (X + GS_TI - 1) / GS_TI, zt = (plane + GS_TI - 1) / GS_TI;
  const int64_t gy = (int64_t)nfields * Z * yt, gz = (int64_t)nfields * zt;
  const int64_t gyl = (Y + GS_TL - 1) / GS_TL, gzl = (Z + GS_TL - 1) / GS_TL;
  SP_CHECK_ARG(gx < (1ll << 31) && gy < (1ll << 31) && gz < (1ll << 31) && gxt <= 65535 && gyl <= 65535 && gzl <= 65535 && yt < (1ll << 31) &&
                   zt < (1ll << 31),
               "sp_gaussian_filter3d_batch: batch too large for one launch per axis");
  const size_t lds_x = (size_t)GX_ROWS * (GX_TX + 2 * radius) * sizeof(float);      // <= 8 KB
  const size_t lds_s = (size_t)(GS_TL + 2 * radius) * GS_TI * sizeof(float);       // <= 40 KB
  hipLaunchKernelGGL(gauss_x_batch_kernel, dim3((unsigned)gx, (unsigned)gxt), dim3(256), lds_x, st, src, dst, rows, X, radius, gw);
  hipLaunchKernelGGL(gauss_strided_batch_kernel, dim3((unsigned)gy, (unsigned)gyl), dim3(256), lds_s, st, (const float*)dst, tmp, Y,
                     (int64_t)X, (int)yt, radius, gw);
  hipLaunchKernelGGL(gauss_strided_batch_kernel, dim3((unsigned)gz, (unsigned)gzl), dim3(256), lds_s, st, (const float*)tmp, dst, Z, plane,
                     (int)zt, radius, gw);
  SP_CHECK_LAUNCH("sp_gaussian_filter3d_batch");
  return SP_OK;
}

// ------------------------------------------------------------------------------------------------ batched warp
// Volume v = sample b, channel c (v = b * (C0 + C1) + c): channels c < C0 live in src0 / dst0 (B, C0, Z, Y, X), the others in
// src1 / dst1 (B, C1, Z, Y, X).  Its fields dx, dy, dz are fields[3 v], [3 v + 1], [3 v + 2].  The coordinate, border and
// interpolation expressions are those of warp_linear_kernel (sp_transform.hip) with (i, j, k) = (x, y, z) and
// (d0, d1, d2) = (dy, dx, dz): the reference displaces axis 0 by the SECOND field (data.py:336-337).  flip[b] != 0 reads the
// source mirrored along x: HemisphericFlip followed by ElasticDeform.  grid (blocks per volume, volumes)
__global__ __launch_bounds__(256) void elastic_warp_batch_kernel(const float* __restrict__ src0, float* __restrict__ dst0, int C0,
                                                                 const float* __restrict__ src1, float* __restrict__ dst1, int C1,
                                                                 const float* __restrict__ fields, const int32_t* __restrict__ flip,
                                                                 float s0, float s1, float s2, int n2, int n1, int n0) {
  const int64_t total = (int64_t)n0 * n1 * n2;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int v = blockIdx.y, Ct = C0 + C1;
  const int b = v / Ct, c = v - b * Ct;
  const float* __restrict__ img = c < C0 ? src0 + ((int64_t)b * C0 + c) * total : src1 + ((int64_t)b * C1 + (c - C0)) * total;
  float* __restrict__ out = c < C0 ? dst0 + ((int64_t)b * C0 + c) * total : dst1 + ((int64_t)b * C1 + (c - C0)) * total;
  const float* __restrict__ d1 = fields + (int64_t)v * 3 * total;      // dx displaces y
  const float* __restrict__ d0 = d1 + total;                           // dy displaces x
  const float* __restrict__ d2 = d0 + total;
  const bool mirror = flip != nullptr && flip[b] != 0;
  const int i = (int)(idx % n0);
  const int64_t r = idx / n0;
  const int j = (int)(r % n1), k = (int)(r / n1);
  const float c0 = (float)i + s0 * d0[idx], c1 = (float)j + s1 * d1[idx], c2 = (float)k + s2 * d2[idx];
  if (!(c0 >= 0.f && c0 <= (float)(n0 - 1) && c1 >= 0.f && c1 <= (float)(n1 - 1) && c2 >= 0.f && c2 <= (float)(n2 - 1))) {
    out[idx] = 0.f;
    return;
  }
  const float f0 = floorf(c0), f1 = floorf(c1), f2 = floorf(c2);
  const float t0 = c0 - f0, t1 = c1 - f1, t2 = c2 - f2;
  const int a0 = (int)f0, a1 = (int)f1, a2 = (int)f2;
  const int b0 = min(a0 + 1, n0 - 1), b1 = min(a1 + 1, n1 - 1), b2 = min(a2 + 1, n2 - 1);     // weight 0 when clamped
  const int xa = mirror ? n0 - 1 - a0 : a0, xb = mirror ? n0 - 1 - b0 : b0;
  const int64_t pa0 = ((int64_t)a2 * n1 + a1) * n0, pa1 = ((int64_t)a2 * n1 + b1) * n0;      // (z, y) rows at z = a2
  const int64_t pb0 = ((int64_t)b2 * n1 + a1) * n0, pb1 = ((int64_t)b2 * n1 + b1) * n0;      // and at z = b2
  const float v000 = img[pa0 + xa], v001 = img[pb0 + xa], v010 = img[pa1 + xa], v011 = img[pb1 + xa];
  const float v100 = img[pa0 + xb], v101 = img[pb0 + xb], v110 = img[pa1 + xb], v111 = img[pb1 + xb];
  const float u0 = 1.f - t0, u1 = 1.f - t1, u2 = 1.f - t2;
  out[idx] = u0 * (u1 * (u2 * v000 + t2 * v001) + t1 * (u2 * v010 + t2 * v011)) +
             t0 * (u1 * (u2 * v100 + t2 * v101) + t1 * (u2 * v110 + t2 * v111));
}

extern "C" int sp_elastic_warp_batch(const float* src0, float* dst0, int32_t C0, const float* src1, float* dst1, int32_t C1,
                                     const float* fields, const int32_t* flip, int32_t B, int32_t Z, int32_t Y, int32_t X, float alpha,
                                     float alpha_z, sp_stream_t stream) {
  SP_CHECK_ARG(fields && B >= 1 && C0 >= 0 && C1 >= 0 && C0 + C1 >= 1 && Z >= 1 && Y >= 1 && X >= 1, "sp_elastic_warp_batch: bad arguments");
  SP_CHECK_ARG((C0 == 0 || (src0 && dst0 && src0 != dst0)) && (C1 == 0 || (src1 && dst1 && src1 != dst1)),
               "sp_elastic_warp_batch: source and destination must be two buffers");
  const int64_t total = (int64_t)Z * Y * X, volumes = (int64_t)B * (C0 + C1);
  SP_CHECK_ARG(total < (1ll << 31) && volumes <= 65535, "sp_elastic_warp_batch: 2^31 voxels per volume or more than 65535 volumes");
  hipLaunchKernelGGL(elastic_warp_batch_kernel, dim3((unsigned)((total + 255) / 256), (unsigned)volumes), dim3(256), 0, ST(stream), src0,
                     dst0, C0, src1, dst1, C1, fields, flip, alpha, alpha, alpha_z, Z, Y, X);
  SP_CHECK_LAUNCH("sp_elastic_warp_batch");
  return SP_OK;
}
