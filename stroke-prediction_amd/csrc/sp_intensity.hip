// Batch-level intensity augmentation (common/data.py:IntensityAugment): Gaussian blur, Gaussian noise, brightness, contrast and
// gamma of every (sample, image channel) field of a collated batch, two launches without blur and five with it:
//   sp_blur3d_reflect_batch      three   scipy.ndimage.gaussian_filter(mode="reflect") with one weights row per field, a launch per axis
//   sp_intensity_stats_partials  one     min, max and sum of the noisy field in 64 fixed chunks (the noise is regenerated, not stored)
//   sp_intensity_apply_batch     one     noise, gain, contrast about the mean, gamma: four voxels = one Philox block per work item
// A field is one (b, c) volume of per_field = Z * Y * X fp32 voxels, X contiguous; its row of 8 floats is [sigma_n, gain,
// contrast, gamma, invert, 0, 0, 0].  A stage whose parameter is neutral is skipped by a workgroup-uniform branch, so a field
// with an all-neutral row leaves bit-equal.  Every expression below is evaluated as written: no contraction into fma.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sp_common.h"
#include "sp_gauss.h"
#include "sp_philox.h"

#pragma clang fp contract(off)

#define ST(s) reinterpret_cast<hipStream_t>(s)

// ------------------------------------------------------------------------------------------------ blur, reflected border
// The tiling of sp_gaussian_filter3d_batch (sp_augment.hip): the input tile plus a halo of `radius` is staged in LDS, the taps are
// summed lowest to highest with fmaf.  Two differences: the halo is filled through the mirrored index (scipy's "reflect":
// d c b a | a b c d | d c b a) instead of 0, and the weights are a row per field, staged in LDS once per workgroup -- which is
// why a workgroup never leaves its field (grid z).  A field whose row is the delta kernel is copied: bit-equal, -0 included.
#define BX_TX 128      // x pass: outputs per row of a tile
#define BX_ROWS 8      // x pass: rows per tile
#define BS_TL 32       // strided pass: outputs along the filtered axis per tile
#define BS_TI 64       // strided pass: contiguous elements per tile row (one wave's width)

// index i of a line of n elements, -radius <= i < n + radius and radius <= n, mirrored into [0, n); -1 when i is further out
// (the part of the last tile's halo that no output of the line reads)
__device__ __forceinline__ int mirror_index(int i, int n) {
  const int m = i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i);
  return (m >= 0 && m < n) ? m : -1;
}

// pass along X: a field holds rows_pf = Z * Y lines of X elements; grid (row tiles of a field, x tiles, fields)
__global__ __launch_bounds__(256) void blur_x_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                     const float* __restrict__ weights, int rows_pf, int X, int radius) {
  extern __shared__ float s[];
  const int taps = 2 * radius + 1, wpad = (taps + 3) & ~3;
  float* sw = s;
  float* st = s + wpad;
  const int pitch = BX_TX + 2 * radius;
  const int field = blockIdx.z;
  const int row0 = blockIdx.x * BX_ROWS, x0 = blockIdx.y * BX_TX;
  const int64_t base = (int64_t)field * rows_pf * X;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int t = threadIdx.x; t < taps; t += 256) sw[t] = weights[(int64_t)field * taps + t];
  for (int r = wave; r < BX_ROWS; r += 4) {
    const int row = row0 + r;
    for (int c = lane; c < pitch; c += 64) {
      const int x = mirror_index(x0 - radius + c, X);
      st[r * pitch + c] = (row < rows_pf && x >= 0) ? src[base + (int64_t)row * X + x] : 0.f;
    }
  }
  __syncthreads();
  const bool delta = sw[radius] == 1.f;
  const int tx = threadIdx.x & (BX_TX - 1), ty = threadIdx.x >> 7;
  if (x0 + tx >= X) return;
  for (int r = ty; r < BX_ROWS; r += 2) {
    const int row = row0 + r;
    if (row >= rows_pf) break;
    const float* p = st + r * pitch + tx;      // tap t of output tx sits at p[t]
    float acc = p[radius];
    if (!delta) {
      acc = 0.f;
      for (int t = 0; t < taps; ++t) acc = fmaf(sw[t], p[t], acc);
    }
    dst[base + (int64_t)row * X + x0 + tx] = acc;
  }
}

// pass along an axis of extent `len` and stride `inner` in the (outer_pf, len, inner) view of a field: Y (outer_pf = Z, inner = X)
// or Z (outer_pf = 1, inner = Y * X).  grid (outer_pf * inner tiles, len tiles, fields)
__global__ __launch_bounds__(256) void blur_strided_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                           const float* __restrict__ weights, int outer_pf, int len, int inner,
                                                           int n_itiles, int radius) {
  extern __shared__ float s[];
  const int taps = 2 * radius + 1, wpad = (taps + 3) & ~3;
  float* sw = s;
  float* st = s + wpad;
  const int field = blockIdx.z;
  const int o = blockIdx.x / n_itiles, it = blockIdx.x - o * n_itiles;
  const int l0 = blockIdx.y * BS_TL;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = it * BS_TI + lane;
  const bool live = i < inner;
  const int64_t base = ((int64_t)field * outer_pf + o) * len * inner + i;
  for (int t = threadIdx.x; t < taps; t += 256) sw[t] = weights[(int64_t)field * taps + t];
  for (int l = wave; l < BS_TL + 2 * radius; l += 4) {
    const int L = mirror_index(l0 - radius + l, len);
    st[l * BS_TI + lane] = (live && L >= 0) ? src[base + (int64_t)L * inner] : 0.f;
  }
  __syncthreads();
  const bool delta = sw[radius] == 1.f;
  if (!live) return;
  for (int l = wave; l < BS_TL; l += 4) {
    const int L = l0 + l;
    if (L >= len) break;
    const float* p = st + l * BS_TI + lane;      // tap t of output l sits in row l + t
    float acc = p[radius * BS_TI];
    if (!delta) {
      acc = 0.f;
      for (int t = 0; t < taps; ++t) acc = fmaf(sw[t], p[t * BS_TI], acc);
    }
    dst[base + (int64_t)L * inner] = acc;
  }
}

extern "C" int sp_blur3d_reflect_batch(const float* src, float* dst, float* tmp, const float* weights, int32_t nfields, int32_t Z, int32_t Y,
                                       int32_t X, int32_t radius, sp_stream_t stream) {
  SP_CHECK_ARG(src && dst && tmp && weights, "sp_blur3d_reflect_batch: src, dst, tmp and weights must not be NULL");
  SP_CHECK_ARG(tmp != src && tmp != dst && src != dst, "sp_blur3d_reflect_batch: src, dst and tmp are three different buffers");
  SP_CHECK_ARG(nfields >= 1 && nfields <= 65535, "sp_blur3d_reflect_batch: 1 <= nfields <= 65535, got %d", nfields);
  SP_CHECK_ARG(radius >= 0 && radius <= SP_GAUSS_MAX_RADIUS, "sp_blur3d_reflect_batch: 0 <= radius <= %d, got %d", SP_GAUSS_MAX_RADIUS, radius);
  SP_CHECK_ARG(Z >= 1 && Y >= 1 && X >= 1 && Z >= radius && Y >= radius && X >= radius,
               "sp_blur3d_reflect_batch: every extent of (%d, %d, %d) must be >= 1 and >= the radius %d (one reflection)", Z, Y, X, radius);
  const int64_t plane = (int64_t)Y * X, per_field = plane * Z;
  SP_CHECK_ARG(per_field < (1ll << 31), "sp_blur3d_reflect_batch: a field holds 2^31 voxels or more");
  const int64_t rows_pf = (int64_t)Z * Y;
  const int64_t gx = (rows_pf + BX_ROWS - 1) / BX_ROWS, gxt = (X + BX_TX - 1) / BX_TX;
  const int64_t yt = (X + BS_TI - 1) / BS_TI, zt = (plane + BS_TI - 1) / BS_TI;
  const int64_t gy = (int64_t)Z * yt, gz = zt;
  const int64_t gyl = (Y + BS_TL - 1) / BS_TL, gzl = (Z + BS_TL - 1) / BS_TL;
  SP_CHECK_ARG(gxt <= 65535 && gyl <= 65535 && gzl <= 65535, "sp_blur3d_reflect_batch: an extent of (%d, %d, %d) is too large for one launch per axis",
               Z, Y, X);
  const int wpad = (2 * radius + 1 + 3) & ~3;
  const size_t lds_x = (size_t)(wpad + BX_ROWS * (BX_TX + 2 * radius)) * sizeof(float);      // <= 8.5 KB
  const size_t lds_s = (size_t)(wpad + (BS_TL + 2 * radius) * BS_TI) * sizeof(float);       // <= 40.5 KB
  hipStream_t st = ST(stream);
  // x: src -> dst; y: dst -> tmp; z: tmp -> dst
  hipLaunchKernelGGL(blur_x_kernel, dim3((unsigned)gx, (unsigned)gxt, (unsigned)nfields), dim3(256), lds_x, st, src, dst, weights, (int)rows_pf,
                     X, radius);
  hipLaunchKernelGGL(blur_strided_kernel, dim3((unsigned)gy, (unsigned)gyl, (unsigned)nfields), dim3(256), lds_s, st, (const float*)dst, tmp,
                     weights, Z, Y, X, (int)yt, radius);
  hipLaunchKernelGGL(blur_strided_kernel, dim3((unsigned)gz, (unsigned)gzl, (unsigned)nfields), dim3(256), lds_s, st, (const float*)tmp, dst,
                     weights, 1, Z, (int)plane, (int)zt, radius);
  SP_CHECK_LAUNCH("sp_blur3d_reflect_batch");
  return SP_OK;
}

// ------------------------------------------------------------------------------------------------ noise
// Standard normals by Box-Muller from Philox4x32-10: key (seed lo, seed hi), counter (q, 0x80000000 | field, call lo, call hi)
// for the block q = e >> 2 of four consecutive elements.  The high bit of the field word keeps the stream apart from
// sp_rng_uniform_pm1's (field < 65536) under one seed.  Words (w0, w1) give elements 4q and 4q + 1, (w2, w3) give 4q + 2 and
// 4q + 3: u1 = ((w >> 8) + 1) 2^-24 in (0, 1], u2 = (w' >> 8) 2^-24 in [0, 1), r = sqrt(-2 ln u1); the even element takes
// r cos(2 pi u2), the odd one r sin(2 pi u2).  A function of (seed, call, field, e) alone.
struct NoiseKey {
  uint32_t k0, k1, call_lo, call_hi;
};

__device__ __forceinline__ void normals4(uint32_t q, uint32_t field, const NoiseKey& key, float n[4]) {
  uint32_t w[4];
  philox4x32_10(q, 0x80000000u | field, key.call_lo, key.call_hi, key.k0, key.k1, w);
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float u1 = (float)((w[2 * p] >> 8) + 1u) * 5.9604644775390625e-08f;      // 24 bits * 2^-24: exact
    const float u2 = (float)(w[2 * p + 1] >> 8) * 5.9604644775390625e-08f;
    const float r = sqrtf(-2.f * logf(u1));
    const float a = 6.2831853071795864769f * u2;
    n[2 * p] = r * cosf(a);
    n[2 * p + 1] = r * sinf(a);
  }
}

// the four elements of block q of a field (f points at the field), after the noise stage; elements at or behind `end` are not read
__device__ __forceinline__ void load_noisy4(const float* f, int64_t e0, int64_t end, int vec4, float sn, uint32_t field,
                                            const NoiseKey& key, float v[4]) {
  if (vec4) {      // per_field a multiple of 4 and the buffer 16-byte aligned: every block of every field is one aligned float4
    const float4 t = *reinterpret_cast<const float4*>(f + e0);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = e0 + i < end ? f[e0 + i] : 0.f;
  }
  if (sn != 0.f) {
    float n[4];
    normals4((uint32_t)(e0 >> 2), field, key, n);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = v[i] + sn * n[i];
  }
}

// ------------------------------------------------------------------------------------------------ statistics
// partials[field][c] = (min, max, sum, 0) of y1 over chunk c of the field: SP_INTENSITY_CHUNKS contiguous chunks of `chunk`
// elements (a multiple of 4: a Philox block never straddles two).  One workgroup per chunk: a thread adds up the blocks
// threadIdx.x, threadIdx.x + 256, ... of its chunk in element order, the 64 lanes of a wave combine by shuffles at the fixed
// offsets 32, 16, ..., 1, thread 0 combines the four waves in index order.  No atomics: the same inputs give the same bits.
#define SP_INTENSITY_CHUNKS 64

__global__ __launch_bounds__(256) void intensity_stats_kernel(const float* __restrict__ src, const float* __restrict__ params,
                                                              float* __restrict__ partials, int64_t per_field, int64_t chunk, NoiseKey key,
                                                              int vec4) {
  __shared__ float red[3][4];
  const uint32_t field = blockIdx.y;
  const float sn = params[(int64_t)field * 8];
  const float* __restrict__ f = src + (int64_t)field * per_field;
  const int64_t lo = (int64_t)blockIdx.x * chunk;
  const int64_t hi = lo + chunk < per_field ? lo + chunk : per_field;
  float mn = INFINITY, mx = -INFINITY, sum = 0.f;
  for (int64_t e0 = lo + 4 * (int64_t)threadIdx.x; e0 < hi; e0 += 4 * 256) {
    float v[4];
    load_noisy4(f, e0, hi, vec4, sn, field, key, v);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (e0 + i < hi) {
        mn = fminf(mn, v[i]);
        mx = fmaxf(mx, v[i]);
        sum = sum + v[i];
      }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    mn = fminf(mn, __shfl_down(mn, off));
    mx = fmaxf(mx, __shfl_down(mx, off));
    sum = sum + __shfl_down(sum, off);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wave] = mn;
    red[1][wave] = mx;
    red[2][wave] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    mn = red[0][0]; mx = red[1][0]; sum = red[2][0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      mn = fminf(mn, red[0][w]);
      mx = fmaxf(mx, red[1][w]);
      sum = sum + red[2][w];
    }
    reinterpret_cast<float4*>(partials)[(int64_t)field * SP_INTENSITY_CHUNKS + blockIdx.x] = make_float4(mn, mx, sum, 0.f);
  }
}

static int64_t intensity_chunk(int64_t per_field) {
  const int64_t c = (per_field + SP_INTENSITY_CHUNKS - 1) / SP_INTENSITY_CHUNKS;
  return (c + 3) / 4 * 4;
}

static NoiseKey noise_key(int64_t seed_bits, int64_t call_bits) {
  const uint64_t seed = (uint64_t)seed_bits, call = (uint64_t)call_bits;      // the ABI carries the 64 bits as int64_t
  NoiseKey k;
  k.k0 = (uint32_t)(seed & 0xffffffffu);
  k.k1 = (uint32_t)(seed >> 32);
  k.call_lo = (uint32_t)(call & 0xffffffffu);
  k.call_hi = (uint32_t)(call >> 32);
  return k;
}

extern "C" int sp_intensity_stats_partials(const float* src, const float* params, float* partials, int32_t nfields, int64_t per_field,
                                           int64_t seed, int64_t call, sp_stream_t stream) {
  SP_CHECK_ARG(src && params && partials, "sp_intensity_stats_partials: src, params and partials must not be NULL");
  SP_CHECK_ARG(reinterpret_cast<uintptr_t>(partials) % 16 == 0, "sp_intensity_stats_partials: partials must be 16-byte aligned");
  SP_CHECK_ARG(nfields >= 1 && nfields <= 65535 && per_field >= 1 && per_field < (1ll << 31),
               "sp_intensity_stats_partials: bad arguments (1 <= nfields <= 65535, 1 <= per_field < 2^31)");
  const int vec4 = (per_field % 4 == 0) && (reinterpret_cast<uintptr_t>(src) % 16 == 0);
  hipLaunchKernelGGL(intensity_stats_kernel, dim3(SP_INTENSITY_CHUNKS, (unsigned)nfields), dim3(256), 0, ST(stream), src, params, partials,
                     per_field, intensity_chunk(per_field), noise_key(seed, call), vec4);
  SP_CHECK_LAUNCH("sp_intensity_stats_partials");
  return SP_OK;
}

// ------------------------------------------------------------------------------------------------ apply
// what the later stages need of a field, derived once per workgroup from its 64 partials
struct FieldRange {
  float m2, min2, max2, min3, max3, R, den;
};

__device__ __forceinline__ float contrast_map(float y2, float k, const FieldRange& fr) {
  return fminf(fmaxf(fmaf(y2 - fr.m2, k, fr.m2), fr.min2), fr.max2);
}

// grid (blocks of 256 Philox blocks per field, fields); a work item = four consecutive voxels
__global__ __launch_bounds__(256) void intensity_apply_kernel(const float* src, float* dst, const float* __restrict__ params,
                                                              const float* __restrict__ partials, int64_t per_field, NoiseKey key, int vec4) {
  __shared__ float4 part[SP_INTENSITY_CHUNKS];
  const uint32_t field = blockIdx.y;
  const float* __restrict__ row = params + (int64_t)field * 8;
  const float sn = row[0], g = row[1], k = row[2], gm = row[3];
  const bool invert = row[4] != 0.f;
  const bool do_gain = g != 1.f, do_contrast = k != 1.f, do_gamma = gm != 1.f || invert;
  FieldRange fr = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 1.f};
  if (do_contrast || do_gamma) {      // uniform over the workgroup: the row is the field's
    if (threadIdx.x < SP_INTENSITY_CHUNKS)
      part[threadIdx.x] = reinterpret_cast<const float4*>(partials)[(int64_t)field * SP_INTENSITY_CHUNKS + threadIdx.x];
    __syncthreads();
    float mn = part[0].x, mx = part[0].y;
    double sum = (double)part[0].z;
    for (int c = 1; c < SP_INTENSITY_CHUNKS; ++c) {      // index order, every thread the same
      mn = fminf(mn, part[c].x);
      mx = fmaxf(mx, part[c].y);
      sum = sum + (double)part[c].z;
    }
    const float mean1 = (float)(sum / (double)per_field);
    fr.m2 = g * mean1;
    fr.min2 = g * mn;      // exact: a multiply by g > 0 is monotone
    fr.max2 = g * mx;
    fr.min3 = do_contrast ? contrast_map(fr.min2, k, fr) : fr.min2;
    fr.max3 = do_contrast ? contrast_map(fr.max2, k, fr) : fr.max2;
    fr.R = fr.max3 - fr.min3;
    fr.den = fr.R + 1e-7f;
  }
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t e0 = q * 4;
  if (e0 >= per_field) return;
  const int64_t off = (int64_t)field * per_field;
  float v[4];
  load_noisy4(src + off, e0, per_field, vec4, sn, field, key, v);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float y = v[i];
    if (do_gain) y = g * y;
    if (do_contrast) y = contrast_map(y, k, fr);
    if (do_gamma) {
      if (invert) {
        const float t = fmaxf((fr.max3 - y) / fr.den, 0.f);
        y = fr.max3 - powf(t, gm) * fr.R;
      } else {
        const float t = fmaxf((y - fr.min3) / fr.den, 0.f);
        y = powf(t, gm) * fr.R + fr.min3;
      }
    }
    v[i] = y;
  }
  float* p = dst + off + e0;
  if (vec4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (e0 + i < per_field) p[i] = v[i];
  }
}

extern "C" int sp_intensity_apply_batch(const float* src, float* dst, const float* params, const float* partials, int32_t nfields,
                                        int64_t per_field, int64_t seed, int64_t call, sp_stream_t stream) {
  SP_CHECK_ARG(src && dst && params && partials, "sp_intensity_apply_batch: src, dst, params and partials must not be NULL");
  SP_CHECK_ARG(reinterpret_cast<uintptr_t>(partials) % 16 == 0, "sp_intensity_apply_batch: partials must be 16-byte aligned");
  SP_CHECK_ARG(nfields >= 1 && nfields <= 65535 && per_field >= 1 && per_field < (1ll << 31),
               "sp_intensity_apply_batch: bad arguments (1 <= nfields <= 65535, 1 <= per_field < 2^31)");
  const int vec4 = (per_field % 4 == 0) && (reinterpret_cast<uintptr_t>(src) % 16 == 0) && (reinterpret_cast<uintptr_t>(dst) % 16 == 0);
  const int64_t blocks = (per_field + 3) / 4;
  hipLaunchKernelGGL(intensity_apply_kernel, dim3((unsigned)((blocks + 255) / 256), (unsigned)nfields), dim3(256), 0, ST(stream), src, dst,
                     params, partials, per_field, noise_key(seed, call), vec4);
  SP_CHECK_LAUNCH("sp_intensity_apply_batch");
  return SP_OK;
}
