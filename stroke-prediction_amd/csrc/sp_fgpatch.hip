// Foreground-oversampled patch origins for the device-resident case cache (common/data.py: ForegroundOversample / CachedBatchLoader).
// The loader draws every patch origin uniformly; for a share of each batch the origin is replaced, ON THE DEVICE, by one that puts a
// uniformly drawn foreground voxel of the sample's case at a drawn position of the label patch.  The labels already live in device
// memory, so nothing is read back and the host never walks a volume.
//   sp_fg_row_index     (once per cache / channel mask / threshold): the exclusive prefix sum of the per-x-row foreground counts of
//                       every case -- the index that turns "foreground voxel number k" into a row by bisection.
//   sp_patch_origins_fg (every batch, between the table upload and the gather): one wave per sample bisects the index, walks the one
//                       row the voxel lies in with ballots and rewrites the origin words of the sample's table row.
// Foreground voxels are numbered in the cache's C order (z, y, x): number k is numpy.flatnonzero(mask[n])[k].  All counts are
// integers, there are no atomics, and no result depends on how the waves are scheduled.  Latency-bound bookkeeping: no LDS beyond the
// scan's wave totals, no tuning beyond coalesced row reads and one wave per sample.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sp_common.h"

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define FG_THREADS 256
#define FG_WAVES (FG_THREADS / SP_WAVE)

// is voxel x of the x row at `line` (channel 0 of the case; cstride floats between channels) foreground?  x < X is the caller's.
__device__ __forceinline__ bool fg_voxel(const float* __restrict__ line, int64_t cstride, int C1, uint32_t chanmask, float thr, int x) {
  bool fg = false;
  for (int c = 0; c < C1; ++c)
    if ((chanmask >> c) & 1u) fg = fg || line[(int64_t)c * cstride + x] > thr;
  return fg;
}

// One wave per x row (row id = n * R + r, R = Z * Y): lanes along x, a ballot per 64 voxels.  The count goes to prefix[n][r + 1]; the
// scan below turns the counts into the prefix sums in place.
__global__ __launch_bounds__(FG_THREADS) void fg_row_count_kernel(const float* __restrict__ labels, int32_t* __restrict__ prefix, int64_t rows,
                                                                 int R, int C1, int X, uint32_t chanmask, float thr) {
  const int lane = threadIdx.x & (SP_WAVE - 1);
  const int64_t row = (int64_t)blockIdx.x * FG_WAVES + (threadIdx.x >> 6);      // wave-uniform
  if (row >= rows) return;
  const int64_t n = row / R, r = row - n * R;
  const int64_t cstride = (int64_t)R * X;
  const float* __restrict__ line = labels + (n * C1 * R + r) * X;
  int count = 0;
  for (int x0 = 0; x0 < X; x0 += SP_WAVE) {
    const int x = x0 + lane;
    const bool fg = x < X && fg_voxel(line, cstride, C1, chanmask, thr, x);
    count += __popcll(__ballot(fg));
  }
  if (lane == 0) prefix[n * (R + 1) + r + 1] = count;
}

// One workgroup per case: prefix[n][0] = 0 and an inclusive scan of the counts at prefix[n][1 .. R], FG_THREADS at a time with a
// running carry (any R; the last chunk may be partial).  Inside a chunk: a shuffle scan per wave, the wave totals through LDS.
__global__ __launch_bounds__(FG_THREADS) void fg_row_scan_kernel(int32_t* __restrict__ prefix, int R) {
  __shared__ int32_t wave_total[FG_WAVES];
  int32_t* __restrict__ p = prefix + (int64_t)blockIdx.x * (R + 1);
  const int t = threadIdx.x, lane = t & (SP_WAVE - 1), wave = t >> 6;
  if (t == 0) p[0] = 0;
  int32_t carry = 0;
  for (int base = 0; base < R; base += FG_THREADS) {
    const int i = base + t;
    int32_t v = i < R ? p[i + 1] : 0;
#pragma unroll
    for (int o = 1; o < SP_WAVE; o <<= 1) {
      const int32_t up = __shfl_up(v, o, SP_WAVE);
      if (lane >= o) v += up;
    }
    if (lane == SP_WAVE - 1) wave_total[wave] = v;
    __syncthreads();
    int32_t before = carry, chunk = 0;
#pragma unroll
    for (int w = 0; w < FG_WAVES; ++w) {
      if (w < wave) before += wave_total[w];
      chunk += wave_total[w];
    }
    if (i < R) p[i + 1] = before + v;
    carry += chunk;
    __syncthreads();      // wave_total is rewritten by the next chunk
  }
}

struct FgOrigins {
  int32_t w1, h1, d1;      // label patch extents
  int32_t mx, my, mz;      // largest legal origin
};

// One 64-lane wave (= one workgroup) per sample.  Everything up to the row walk is computed by all lanes alike (wave-uniform values);
// the walk puts lane l on voxel x0 + l.  Lane 0 stores.
__global__ __launch_bounds__(SP_WAVE) void patch_origins_fg_kernel(const float* __restrict__ labels, const int32_t* __restrict__ prefix,
                                                                  const int32_t* __restrict__ draws, int32_t* __restrict__ table,
                                                                  int32_t* __restrict__ picked, FgOrigins g, int N, int C1, int Z, int Y,
                                                                  int X, uint32_t chanmask, float thr) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int32_t* __restrict__ row = table + (int64_t)b * 5;
  const int32_t* __restrict__ dr = draws + (int64_t)b * 5;
  const int slot = row[0];
  const bool mirror = row[4] != 0;
  const int R = Z * Y;
  int32_t k = -1, fx = -1, fy = -1, fz = -1;
  if (dr[0] != 0 && slot >= 0 && slot < N) {
    const int32_t* __restrict__ p = prefix + (int64_t)slot * (R + 1);
    const int32_t total = p[R];
    if (total > 0) {
      const uint32_t want = (uint32_t)(((uint64_t)(uint32_t)dr[1] * (uint64_t)(uint32_t)total) >> 32);      // < total
      // the row r with p[r] <= want < p[r + 1]: p[lo] <= want < p[hi] holds from (0, R) on; R < 2^31 needs at most 31 halvings
      int lo = 0, hi = R;
      for (int step = 0; step < 32 && hi - lo > 1; ++step) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((uint32_t)p[mid] <= want) lo = mid; else hi = mid;
      }
      uint32_t rem = want - (uint32_t)p[lo];
      const int64_t cstride = (int64_t)R * X;
      const float* __restrict__ line = labels + ((int64_t)slot * C1 * R + lo) * X;
      for (int x0 = 0; x0 < X; x0 += SP_WAVE) {
        const int x = x0 + lane;
        const bool fg = x < X && fg_voxel(line, cstride, C1, chanmask, thr, x);
        const unsigned long long m = __ballot(fg);
        const uint32_t c = (uint32_t)__popcll(m);
        if (rem < c) {
          // the lane with `rem` set lanes below it
          const unsigned long long below = m & ((1ull << lane) - 1ull);
          const unsigned long long sel = __ballot(fg && (uint32_t)__popcll(below) == rem);
          fx = x0 + (__ffsll((long long)sel) - 1);
          fy = lo % Y;
          fz = lo / Y;
          k = (int32_t)want;
          break;
        }
        rem -= c;
      }
      // not found: the index says the row holds the voxel and the labels say it does not -- the row stays as the host drew it
    }
  }
  if (lane != 0) return;
  if (k >= 0) {
    const int jx = min(max(dr[2], 0), g.w1 - 1), jy = min(max(dr[3], 0), g.h1 - 1), jz = min(max(dr[4], 0), g.d1 - 1);
    const int lx = mirror ? X - 1 - fx : fx;
    row[1] = min(max(lx - jx, 0), g.mx);
    row[2] = min(max(fy - jy, 0), g.my);
    row[3] = min(max(fz - jz, 0), g.mz);
  }
  if (picked) {
    int32_t* __restrict__ o = picked + (int64_t)b * 4;
    o[0] = k; o[1] = fx; o[2] = fy; o[3] = fz;
  }
}

static int fg_check(const char* who, const float* labels, const int32_t* prefix, int32_t N, int32_t C1, int32_t Z, int32_t Y, int32_t X,
                    int32_t chanmask) {
  SP_CHECK_ARG(labels && prefix, "%s: NULL labels or prefix", who);
  SP_CHECK_ARG(N >= 1 && Z >= 1 && Y >= 1 && X >= 1, "%s: N, Z, Y, X must be positive, got %d, %d, %d, %d", who, N, Z, Y, X);
  SP_CHECK_ARG(C1 >= 1 && C1 <= 32, "%s: C1 = %d, the channel mask has 32 bits", who, C1);
  const uint32_t usable = C1 == 32 ? 0xffffffffu : ((1u << C1) - 1u);
  SP_CHECK_ARG(((uint32_t)chanmask & usable) != 0, "%s: chanmask 0x%x selects no channel below C1 = %d", who, (unsigned)chanmask, C1);
  SP_CHECK_ARG((int64_t)Z * Y * X < (1ll << 31), "%s: 2^31 or more voxels per case", who);
  SP_CHECK_ARG((int64_t)N * Z * Y < (1ll << 31), "%s: 2^31 or more x rows over all cases", who);
  return SP_OK;
}

extern "C" int sp_fg_row_index(const float* labels, int32_t N, int32_t C1, int32_t Z, int32_t Y, int32_t X, int32_t chanmask, float threshold,
                               int32_t* prefix, sp_stream_t stream) {
  const int rc = fg_check("sp_fg_row_index", labels, prefix, N, C1, Z, Y, X, chanmask);
  if (rc != SP_OK) return rc;
  const int R = Z * Y;
  const int64_t rows = (int64_t)N * R;
  hipLaunchKernelGGL(fg_row_count_kernel, dim3((unsigned)((rows + FG_WAVES - 1) / FG_WAVES)), dim3(FG_THREADS), 0, ST(stream), labels, prefix,
                     rows, R, C1, X, (uint32_t)chanmask, threshold);
  SP_CHECK_LAUNCH("sp_fg_row_index (count)");
  hipLaunchKernelGGL(fg_row_scan_kernel, dim3((unsigned)N), dim3(FG_THREADS), 0, ST(stream), prefix, R);
  SP_CHECK_LAUNCH("sp_fg_row_index (scan)");
  return SP_OK;
}

extern "C" int sp_patch_origins_fg(const float* labels, const int32_t* prefix, int32_t N, int32_t C1, int32_t Z, int32_t Y, int32_t X,
                                   int32_t chanmask, float threshold, const int32_t* draws, const int32_t* ext1, const int32_t* omax,
                                   int32_t* table, int32_t* picked, int32_t B, sp_stream_t stream) {
  const int rc = fg_check("sp_patch_origins_fg", labels, prefix, N, C1, Z, Y, X, chanmask);
  if (rc != SP_OK) return rc;
  SP_CHECK_ARG(draws && ext1 && omax && table && B >= 1, "sp_patch_origins_fg: bad arguments (draws, ext1, omax, table, B >= 1)");
  SP_CHECK_ARG(ext1[0] >= 1 && ext1[1] >= 1 && ext1[2] >= 1, "sp_patch_origins_fg: ext1 (%d, %d, %d) must be positive", ext1[0], ext1[1],
               ext1[2]);
  SP_CHECK_ARG(omax[0] >= 0 && omax[1] >= 0 && omax[2] >= 0, "sp_patch_origins_fg: omax (%d, %d, %d) must not be negative", omax[0], omax[1],
               omax[2]);
  FgOrigins g;
  g.w1 = ext1[0]; g.h1 = ext1[1]; g.d1 = ext1[2];
  g.mx = omax[0]; g.my = omax[1]; g.mz = omax[2];
  hipLaunchKernelGGL(patch_origins_fg_kernel, dim3((unsigned)B), dim3(SP_WAVE), 0, ST(stream), labels, prefix, draws, table, picked, g, N, C1,
                     Z, Y, X, (uint32_t)chanmask, threshold);
  SP_CHECK_LAUNCH("sp_patch_origins_fg");
  return SP_OK;
}
