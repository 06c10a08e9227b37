// Augmenting patch sampler for the device-resident case cache (common/data.py: PatchAugment / CachedBatchLoader): the batched gather
// of sp_gather.hip read through a per-sample transform.  Sample b still names its case, its patch origin (in group 0's PADDED
// coordinates) and its flip flag in one table row; in addition a row of `xform` holds an output -> source affine map about the patch
// centre, `fields` an optional displacement triple on group 0's output grid shared by every channel of both groups, `intensity` an
// optional (gain, bias) per image channel.  For group t and output voxel v:
//   p = v + (pad0 - pad_t)                        patch-frame position (group 0: p = v)
//   c = (ext0 - 1) / 2                            patch centre
//   q = (o - pad0) + c + M (p - c) + t + (alpha_xy fx, alpha_xy fy, alpha_z fz)[b, p]      source position, unpadded coordinates
//   flip: q.x <- (X - 1) - q.x
// and the value is the trilinear sum over the corners floor(q) + {0, 1}^3, a corner outside the volume contributing the pad value:
// S = sum of w_k src_k and W = sum of w_k over the corners inside; group 0 writes gain S + bias W + padval0 (1 - W), group 1 (pad 0)
// writes S, or S >= thresh1 as 1.0 / 0.0.  The sum above is evaluated left to right in fp32: integer and half-integer terms are
// exact, weights 1 and 0 reproduce the source value, so the identity map equals sp_patch_gather_batch bit for bit.
// One work item per output voxel (or per four consecutive x with one 16-byte store); no LDS, no atomics.  The field reads are
// coalesced; the corner reads are scattered over one ~7 MB case, which sits in L2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sp_common.h"

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define SAMPLE_THREADS 256

struct SampleGroup {
  const float* src;      // (N, C, Z, Y, X)
  float* dst;            // (B, C, d, h, w)
  int32_t C, w, h, d;
  int32_t ax, ay, az;    // pad0 - pad_t: output voxel -> patch-frame position
  float padval;
  float thresh;          // >= 0: write (value >= thresh) as 1.0 / 0.0 (labels)
  int32_t vec;           // 1: a thread writes four consecutive x with one 16-byte store (w % 4 == 0 and dst 16-byte aligned)
  int32_t nblk;          // workgroups per (sample, channel) volume
};

struct SampleFrame {
  int32_t w0, h0, d0;    // group 0's output grid: the frame of the patch centre and of the fields
  int32_t px0, py0, pz0;
};

// S and W of one position: the corners inside the volume with a non-zero weight (a weight of exactly 0 reads nothing, so an
// integer coordinate touches one voxel per axis)
__device__ __forceinline__ void trilinear(const float* __restrict__ vol, float qx, float qy, float qz, int Z, int Y, int X, float& S,
                                          float& W) {
  S = 0.f;
  W = 0.f;
  // a coordinate outside (-1, n) has no corner inside (also catches NaN and keeps the int conversion defined)
  if (!(qx > -1.f && qx < (float)X && qy > -1.f && qy < (float)Y && qz > -1.f && qz < (float)Z)) return;
  const float flx = floorf(qx), fly = floorf(qy), flz = floorf(qz);
  const float fx = qx - flx, fy = qy - fly, fz = qz - flz;
  const int ix = (int)flx, iy = (int)fly, iz = (int)flz;
  const float wx[2] = {1.f - fx, fx}, wy[2] = {1.f - fy, fy}, wz[2] = {1.f - fz, fz};
#pragma unroll
  for (int kz = 0; kz < 2; ++kz) {
    const int sz = iz + kz;
    const bool zin = sz >= 0 && sz < Z;
#pragma unroll
    for (int ky = 0; ky < 2; ++ky) {
      const int sy = iy + ky;
      const bool yin = zin && sy >= 0 && sy < Y;
      const float wzy = wz[kz] * wy[ky];
      const int64_t rowoff = ((int64_t)(yin ? sz : 0) * Y + (yin ? sy : 0)) * X;
#pragma unroll
      for (int kx = 0; kx < 2; ++kx) {
        const int sx = ix + kx;
        const float wk = wzy * wx[kx];
        if (yin && sx >= 0 && sx < X && wk != 0.f) {
          S = fmaf(wk, vol[rowoff + sx], S);
          W += wk;
        }
      }
    }
  }
}

// Workgroup id -> (group, sample, channel, block of the volume), as in patch_gather_batch_kernel.
__global__ __launch_bounds__(SAMPLE_THREADS) void patch_sample_batch_kernel(SampleGroup g0, SampleGroup g1, SampleFrame fr,
                                                                            const int32_t* __restrict__ table,
                                                                            const float* __restrict__ xform,
                                                                            const float* __restrict__ fields,
                                                                            const float* __restrict__ intensity, uint32_t blocks0, int N,
                                                                            int Z, int Y, int X) {
  uint32_t bid = blockIdx.x;
  const bool second = bid >= blocks0;
  if (second) bid -= blocks0;
  const float* __restrict__ src = second ? g1.src : g0.src;
  float* __restrict__ dst = second ? g1.dst : g0.dst;
  const int C = second ? g1.C : g0.C, w = second ? g1.w : g0.w, h = second ? g1.h : g0.h, d = second ? g1.d : g0.d;
  const int ax = second ? g1.ax : g0.ax, ay = second ? g1.ay : g0.ay, az = second ? g1.az : g0.az;
  const float padval = second ? g1.padval : g0.padval;
  const float thresh = second ? g1.thresh : g0.thresh;
  const int vec = second ? g1.vec : g0.vec;
  const uint32_t nblk = (uint32_t)(second ? g1.nblk : g0.nblk);
  const uint32_t vol = bid / nblk, blk = bid - vol * nblk;
  const int b = (int)(vol / (uint32_t)C), c = (int)(vol - (uint32_t)b * (uint32_t)C);
  const int32_t* __restrict__ row = table + (int64_t)b * 5;
  const int cs = row[0];
  const bool mirror = row[4] != 0;
  const float* __restrict__ xf = xform + (int64_t)b * 16;
  const float m00 = xf[0], m01 = xf[1], m02 = xf[2], m10 = xf[3], m11 = xf[4], m12 = xf[5], m20 = xf[6], m21 = xf[7], m22 = xf[8];
  const float tx = xf[9], ty = xf[10], tz = xf[11], axy = xf[12], alz = xf[13];
  // patch centre and (o - pad0) + c: integers and half-integers, exact
  const float cx = 0.5f * (float)(fr.w0 - 1), cy = 0.5f * (float)(fr.h0 - 1), cz = 0.5f * (float)(fr.d0 - 1);
  const float bx = (float)(row[1] - fr.px0) + cx, by = (float)(row[2] - fr.py0) + cy, bz = (float)(row[3] - fr.pz0) + cz;
  float gain = 1.f, bias = 0.f;
  if (!second && intensity) {
    gain = intensity[((int64_t)b * C + c) * 2];
    bias = intensity[((int64_t)b * C + c) * 2 + 1];
  }
  const int wq = vec ? w >> 2 : w;                                   // work items per output row
  const int64_t i = (int64_t)blk * SAMPLE_THREADS + threadIdx.x;
  if (i >= (int64_t)wq * h * d) return;
  const int xq = (int)(i % wq);
  const int64_t r = i / wq;
  const int y = (int)(r % h), z = (int)(r / h);
  const bool live = cs >= 0 && cs < N;
  const float* __restrict__ volume = src + ((int64_t)(live ? cs : 0) * C + c) * ((int64_t)Z * Y * X);
  float* __restrict__ out = dst + (((int64_t)vol * d + z) * h + y) * w;
  const int py = y + ay, pz = z + az;
  const float dy = (float)py - cy, dz = (float)pz - cz;
  // the field row of this output row: fields (B, 3, d0, h0, w0), components fx, fy, fz
  const int64_t fplane = (int64_t)fr.d0 * fr.h0 * fr.w0;
  const float* __restrict__ frow = fields ? fields + (int64_t)b * 3 * fplane + ((int64_t)pz * fr.h0 + py) * fr.w0 : nullptr;
  const int nx = vec ? 4 : 1;
  const int x0 = vec ? xq << 2 : xq;
  const int px0 = x0 + ax;
  float f[3][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  if (frow) {
    if (vec && ((reinterpret_cast<uintptr_t>(frow + px0) | (uintptr_t)(fplane * 4)) & 15) == 0) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float4 t = *reinterpret_cast<const float4*>(frow + a * fplane + px0);
        f[a][0] = t.x; f[a][1] = t.y; f[a][2] = t.z; f[a][3] = t.w;
      }
    } else {
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < nx) f[a][k] = frow[a * fplane + px0 + k];
    }
  }
  float res[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    res[k] = padval;
    if (k >= nx) continue;
    const float dx = (float)(px0 + k) - cx;
    // q = (o - pad0) + c + M (p - c) + t + alpha f, left to right
    float qx = bx + fmaf(m02, dz, fmaf(m01, dy, m00 * dx)) + tx;
    float qy = by + fmaf(m12, dz, fmaf(m11, dy, m10 * dx)) + ty;
    float qz = bz + fmaf(m22, dz, fmaf(m21, dy, m20 * dx)) + tz;
    if (frow) {
      qx += axy * f[0][k];
      qy += axy * f[1][k];
      qz += alz * f[2][k];
    }
    if (mirror) qx = (float)(X - 1) - qx;
    float S = 0.f, W = 0.f;
    if (live) trilinear(volume, qx, qy, qz, Z, Y, X, S, W);
    float val = second ? S : fmaf(gain, S, fmaf(bias, W, padval * (1.f - W)));
    if (thresh >= 0.f) val = val >= thresh ? 1.f : 0.f;
    res[k] = val;
  }
  if (vec)
    *reinterpret_cast<float4*>(out + x0) = make_float4(res[0], res[1], res[2], res[3]);
  else
    out[x0] = res[0];
}

static int sample_group(SampleGroup* g, const char* which, const float* src, float* dst, int32_t C, const int32_t* ext, const int32_t* pad,
                        const int32_t* pad0, float padval, float thresh) {
  g->src = src; g->dst = dst; g->C = C; g->padval = padval; g->thresh = thresh;
  g->w = g->h = g->d = 1; g->ax = g->ay = g->az = 0; g->vec = 0; g->nblk = 1;
  if (C == 0) return SP_OK;
  SP_CHECK_ARG(ext && pad, "sp_patch_sample_batch: group %s has %d channels but no extents / padding", which, C);
  // the extents first: an output without elements has no address to check
  SP_CHECK_ARG(ext[0] >= 1 && ext[1] >= 1 && ext[2] >= 1, "sp_patch_sample_batch: group %s extents (%d, %d, %d) must be positive", which,
               ext[0], ext[1], ext[2]);
  SP_CHECK_ARG(src && dst, "sp_patch_sample_batch: group %s has %d channels but a NULL pointer", which, C);
  const int64_t total = (int64_t)ext[0] * ext[1] * ext[2];
  SP_CHECK_ARG(total < (1ll << 31), "sp_patch_sample_batch: group %s: 2^31 or more output voxels per volume", which);
  g->w = ext[0]; g->h = ext[1]; g->d = ext[2];
  g->ax = pad0[0] - pad[0]; g->ay = pad0[1] - pad[1]; g->az = pad0[2] - pad[2];
  // every output row starts 16-byte aligned when the base does and w is a multiple of 4 (a volume then is one too)
  g->vec = (ext[0] % 4 == 0) && (reinterpret_cast<uintptr_t>(dst) % 16 == 0);
  const int64_t items = g->vec ? total / 4 : total;
  g->nblk = (int32_t)((items + SAMPLE_THREADS - 1) / SAMPLE_THREADS);
  return SP_OK;
}

extern "C" int sp_patch_sample_batch(const float* src0, float* dst0, int32_t C0, const int32_t* ext0, const int32_t* pad0, float padval0,
                                     const float* src1, float* dst1, int32_t C1, const int32_t* ext1, const int32_t* pad1, float thresh1,
                                     const int32_t* table, const float* xform, const float* fields, const float* intensity, int32_t N,
                                     int32_t B, int32_t Z, int32_t Y, int32_t X, sp_stream_t stream) {
  SP_CHECK_ARG(table && B >= 1 && N >= 1 && Z >= 1 && Y >= 1 && X >= 1 && C0 >= 0 && C1 >= 0,
               "sp_patch_sample_batch: bad arguments (table, B >= 1, N >= 1, Z, Y, X >= 1, C0, C1 >= 0)");
  SP_CHECK_ARG(C0 + C1 >= 1, "sp_patch_sample_batch: both groups are empty (C0 = C1 = 0)");
  SP_CHECK_ARG((int64_t)Z * Y * X < (1ll << 31), "sp_patch_sample_batch: 2^31 or more voxels per cached volume");
  SP_CHECK_ARG(xform, "sp_patch_sample_batch: xform is NULL (one row of 16 floats per sample is required)");
  SP_CHECK_ARG(!(intensity && C0 == 0), "sp_patch_sample_batch: intensity given but group 0 is empty (C0 = 0)");
  // group 0's grid is the frame of the patch centre, of the origins and of the fields, also when group 0 has no channels
  SP_CHECK_ARG(ext0 && pad0, "sp_patch_sample_batch: ext0 / pad0 are NULL (they define the patch frame of both groups)");
  SP_CHECK_ARG(ext0[0] >= 1 && ext0[1] >= 1 && ext0[2] >= 1, "sp_patch_sample_batch: group 0 extents (%d, %d, %d) must be positive", ext0[0],
               ext0[1], ext0[2]);
  SampleGroup g0, g1;
  int rc = sample_group(&g0, "0", src0, dst0, C0, ext0, pad0, pad0, padval0, -1.f);
  if (rc != SP_OK) return rc;
  rc = sample_group(&g1, "1", src1, dst1, C1, ext1, pad1, pad0, 0.f, thresh1 >= 0.f ? thresh1 : -1.f);
  if (rc != SP_OK) return rc;
  if (fields && C1 > 0) {
    // the kernel indexes the fields at p = v + (pad0 - pad1): every voxel of group 1 must fall on group 0's grid
    SP_CHECK_ARG(g1.ax >= 0 && g1.ay >= 0 && g1.az >= 0 && g1.w + g1.ax <= ext0[0] && g1.h + g1.ay <= ext0[1] && g1.d + g1.az <= ext0[2],
                 "sp_patch_sample_batch: fields given but group 1 (ext1 (%d, %d, %d), pad0 - pad1 (%d, %d, %d)) leaves group 0's grid "
                 "(%d, %d, %d)", g1.w, g1.h, g1.d, g1.ax, g1.ay, g1.az, ext0[0], ext0[1], ext0[2]);
  }
  SampleFrame fr = {ext0[0], ext0[1], ext0[2], pad0[0], pad0[1], pad0[2]};
  const int64_t blocks0 = (int64_t)B * C0 * g0.nblk, blocks1 = (int64_t)B * C1 * g1.nblk;
  SP_CHECK_ARG(blocks0 + blocks1 < (1ll << 31), "sp_patch_sample_batch: B = %d needs %lld workgroups, above the grid limit of 2^31 - 1", B,
               (long long)(blocks0 + blocks1));
  hipLaunchKernelGGL(patch_sample_batch_kernel, dim3((unsigned)(blocks0 + blocks1)), dim3(SAMPLE_THREADS), 0, ST(stream), g0, g1, fr, table,
                     xform, fields, intensity, (uint32_t)blocks0, N, Z, Y, X);
  SP_CHECK_LAUNCH("sp_patch_sample_batch");
  return SP_OK;
}
