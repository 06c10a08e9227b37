// The signed-distance-map (SDM) interpolation baseline (reference test_sdm_resampling.py:15-52) on the device:
//   * sp_sdm_signed_fields: penu_dist = edt(penu > thr) - edt(penu < thr), core_dist = edt(1 - core_bin) - edt(core > thr) with
//     scipy.ndimage.distance_transform_edt semantics (unit spacing), including the artificial core of an empty core mask
//     (center_of_mass of the penumbra mask, truncated, dilated to the L1 ball of radius `dilate`), decided on the device;
//   * sp_sdm_zoom: scipy.ndimage.zoom(x, factors) with order 3, mode "constant", grid_mode False (the cubic B-spline prefilter
//     with mirror boundaries, then a separable 4-tap evaluation with mirrored coefficient indices), an output crop and a
//     leading batch axis, fp64 / int8 inputs and fp64 / int8 / fp32-sign-mask outputs;
//   * sp_sdm_blend: latent_penu * t - latent_core * (1 - t) for T values of t in one launch, in fp64 without contraction.
// Volumes are small (<= 28 x 132 x 132, exports 28 x 256 x 256): these are latency / L2-bound scans and gathers.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sp_common.h"
#include "sp_edt.h"

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define SDM_MAXDIM 3
#define SDM_LINES 64                  // lines per workgroup of the LDS-staged prefilter (one per lane)
#define SDM_LDS_PITCH (SDM_LINES + 1) // doubles per line position in LDS (odd pitch: the staging stores spread over the banks)
#define SDM_MAX_LDS_LINE 256          // longest contiguous line the LDS-staged prefilter takes (128 KiB of LDS)

enum { SDM_CNT_CORE = 0, SDM_CNT_PENU_GT = 1, SDM_CNT_PENU_LT = 2, SDM_SUM_D = 3, SDM_SUM_H = 4, SDM_SUM_W = 5, SDM_NCNT = 6 };
#define SDM_SEED_BLOCKS 1024                                      // workgroups of the seed pass: one partial record each
static const int64_t kCountersBytes = SDM_SEED_BLOCKS * SDM_NCNT * 8;   // uint64 partials at the front of the workspace

// ------------------------------------------------------------------------------------------------ signed fields
// g[4][N] seeds of the four transforms: 0 where the transform's input is zero, SP_SD_BIG elsewhere
//   0: penu > thr   1: penu < thr   2: 1 - core_bin (zero on the core; the artificial core is stamped later)   3: core > thr
// and per workgroup the exact counts / index sums the artificial core needs, written (not added) to part[block][6]: no atomics,
// no zeroing, and the totals do not depend on the order of arrival
__global__ __launch_bounds__(256) void sdm_seed_kernel(const float* __restrict__ core, const float* __restrict__ penu, float thr, int H,
                                                       int W, int64_t n, float* __restrict__ g, unsigned long long* __restrict__ part) {
  unsigned long long c[SDM_NCNT] = {0, 0, 0, 0, 0, 0};
  const int64_t hw = (int64_t)H * W;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256) {
    const float p = penu[idx], q = core[idx];
    const bool pg = p > thr, pl = p < thr, cg = q > thr;
    g[idx] = pg ? SP_SD_BIG : 0.f;
    g[n + idx] = pl ? SP_SD_BIG : 0.f;
    g[2 * n + idx] = cg ? 0.f : SP_SD_BIG;
    g[3 * n + idx] = cg ? SP_SD_BIG : 0.f;
    c[SDM_CNT_CORE] += cg;
    c[SDM_CNT_PENU_LT] += pl;
    if (pg) {
      c[SDM_CNT_PENU_GT] += 1;
      c[SDM_SUM_D] += (unsigned long long)(idx / hw);
      c[SDM_SUM_H] += (unsigned long long)((idx % hw) / W);
      c[SDM_SUM_W] += (unsigned long long)(idx % W);
    }
  }
  __shared__ unsigned long long red[4][SDM_NCNT];
#pragma unroll
  for (int j = 0; j < SDM_NCNT; ++j) {
    unsigned long long v = c[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < SDM_NCNT)
    part[(int64_t)blockIdx.x * SDM_NCNT + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// the artificial core (test_sdm_resampling.py:26-30) and the info record; one workgroup, which first adds the seed pass's
// partials.  Exact integer sums, divided in double and truncated like int(center_of_mass); the dilation of one voxel by
// `dilate` iterations of the rank-3 cross is the L1 ball of that radius, clipped to the volume
__global__ __launch_bounds__(256) void sdm_stamp_kernel(const unsigned long long* __restrict__ part, int nparts, int D, int H, int W, int r,
                                                        float* __restrict__ g2, int32_t* __restrict__ info) {
  __shared__ unsigned long long tot[4][SDM_NCNT];
  unsigned long long c[SDM_NCNT] = {0, 0, 0, 0, 0, 0};
  for (int b = threadIdx.x; b < nparts; b += blockDim.x) {
#pragma unroll
    for (int j = 0; j < SDM_NCNT; ++j) c[j] += part[(int64_t)b * SDM_NCNT + j];
  }
#pragma unroll
  for (int j = 0; j < SDM_NCNT; ++j) {
    unsigned long long v = c[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) tot[threadIdx.x >> 6][j] = v;
  }
  __syncthreads();
  unsigned long long cnt[SDM_NCNT];
#pragma unroll
  for (int j = 0; j < SDM_NCNT; ++j) cnt[j] = tot[0][j] + tot[1][j] + tot[2][j] + tot[3][j];
  const unsigned long long n = (unsigned long long)D * H * W;
  const unsigned long long nc = cnt[SDM_CNT_CORE], npg = cnt[SDM_CNT_PENU_GT], npl = cnt[SDM_CNT_PENU_LT];
  const bool art = nc == 0 && npg > 0;
  int cog[3] = {-1, -1, -1};
  if (art) {
    cog[0] = (int)((double)cnt[SDM_SUM_D] / (double)npg);
    cog[1] = (int)((double)cnt[SDM_SUM_H] / (double)npg);
    cog[2] = (int)((double)cnt[SDM_SUM_W] / (double)npg);
    const int side = 2 * r + 1;
    for (int e = threadIdx.x; e < side * side * side; e += blockDim.x) {
      const int a = e / (side * side) - r, b = (e / side) % side - r, c = e % side - r;
      const int d = cog[0] + a, h = cog[1] + b, w = cog[2] + c;
      if (abs(a) + abs(b) + abs(c) <= r && d >= 0 && d < D && h >= 0 && h < H && w >= 0 && w < W)
        g2[((int64_t)d * H + h) * W + w] = 0.f;
    }
  }
  if (threadIdx.x == 0) {
    const int bits = (npg == n ? 1 : 0) | (npl == n ? 2 : 0) | (nc == 0 && npg == 0 ? 4 : 0) | (nc == n ? 8 : 0);
    info[SP_SDM_INFO_ARTIFICIAL] = art ? 1 : 0;
    info[SP_SDM_INFO_COG + 0] = cog[0];
    info[SP_SDM_INFO_COG + 1] = cog[1];
    info[SP_SDM_INFO_COG + 2] = cog[2];
    info[SP_SDM_INFO_DEGENERATE] = bits;
    info[5] = 0; info[6] = 0; info[7] = 0;
  }
}

__global__ __launch_bounds__(256) void sdm_edt_axis_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t total, int n,
                                                           int64_t inner) {
  sp_edt_axis(src, dst, total, n, inner);
}

// fields[0] = core_dist, fields[1] = penu_dist (squared distances are exact integers: the roots in fp64, as scipy takes them)
__global__ __launch_bounds__(256) void sdm_fields_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ core_dist,
                                                         double* __restrict__ penu_dist) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  penu_dist[idx] = sqrt((double)g[idx]) - sqrt((double)g[n + idx]);
  core_dist[idx] = sqrt((double)g[2 * n + idx]) - sqrt((double)g[3 * n + idx]);
}

static int64_t fields_ws_bytes(int64_t n) { return kCountersBytes + 2 * 4 * n * (int64_t)sizeof(float); }

extern "C" int sp_sdm_signed_fields(const float* core, const float* penu, int32_t D, int32_t H, int32_t W, float threshold,
                                    int32_t dilate, double* core_dist, double* penu_dist, int32_t* info, void* ws, int64_t ws_bytes,
                                    sp_stream_t stream) {
  SP_CHECK_ARG(core && penu && core_dist && penu_dist && info && ws, "sp_sdm_signed_fields: null pointer");
  SP_CHECK_ARG(D >= 1 && H >= 1 && W >= 1 && dilate >= 1, "sp_sdm_signed_fields: bad extents (%d, %d, %d) or dilate %d", D, H, W, dilate);
  SP_CHECK_ARG(D < 4096 && H < 4096 && W < 4096, "sp_sdm_signed_fields: extent of 4096 or more");
  const int64_t n = (int64_t)D * H * W;
  SP_CHECK_ARG(4 * n < (1ll << 31), "sp_sdm_signed_fields: volume too large");
  SP_CHECK_ARG(ws_bytes >= fields_ws_bytes(n), "sp_sdm_signed_fields: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
               (long long)fields_ws_bytes(n));
  hipStream_t st = ST(stream);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(ws);
  float* g0 = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + kCountersBytes);
  float* g1 = g0 + 4 * n;
  const unsigned grid = (unsigned)((n + 255) / 256), grid4 = (unsigned)((4 * n + 255) / 256);
  const int nseed = grid < SDM_SEED_BLOCKS ? (int)grid : SDM_SEED_BLOCKS;
  hipLaunchKernelGGL(sdm_seed_kernel, dim3(nseed), dim3(256), 0, st, core, penu, threshold, H, W, n, g0, cnt);
  hipLaunchKernelGGL(sdm_stamp_kernel, dim3(1), dim3(256), 0, st, (const unsigned long long*)cnt, nseed, D, H, W, dilate, g0 + 2 * n, info);
  // the four transforms in the same three launches: a (4 D, H, W) stack scanned along W, H, then D (4 D = 4 x D: the D scan's
  // lines never cross from one volume into the next)
  const int ext[3] = {D, H, W};
  float* a = g0; float* b = g1;
  int64_t inner = 1;
  for (int ax = 2; ax >= 0; --ax) {
    if (ext[ax] > 1) {
      hipLaunchKernelGGL(sdm_edt_axis_kernel, dim3(grid4), dim3(256), 0, st, (const float*)a, b, 4 * n, ext[ax], inner);
      float* t = a; a = b; b = t;
    }
    inner *= ext[ax];
  }
  hipLaunchKernelGGL(sdm_fields_kernel, dim3(grid), dim3(256), 0, st, (const float*)a, n, core_dist, penu_dist);
  SP_CHECK_LAUNCH("sp_sdm_signed_fields");
  return SP_OK;
}

// ------------------------------------------------------------------------------------------------ cubic-spline zoom
__device__ __forceinline__ double sdm_load(const void* p, int64_t i, int dtype) {
  switch (dtype) {
    case SP_SDM_I8: return (double)reinterpret_cast<const int8_t*>(p)[i];
    case SP_SDM_F32_AS_I8: return (double)(int8_t)reinterpret_cast<const float*>(p)[i];     // numpy astype(int8): truncation
    default: return reinterpret_cast<const double*>(p)[i];
  }
}
__device__ __forceinline__ void sdm_store(void* p, int64_t i, int dtype, double v) {
  switch (dtype) {
    case SP_SDM_I8: {    // scipy's integer output: round half away from zero, then the C conversion
      const double r = v > 0.0 ? v + 0.5 : v - 0.5;
      reinterpret_cast<int8_t*>(p)[i] = (int8_t)(int)r;
      break;
    }
    case SP_SDM_MASK_GT0: reinterpret_cast<float*>(p)[i] = v > 0.0 ? 1.f : 0.f; break;
    case SP_SDM_MASK_LT0: reinterpret_cast<float*>(p)[i] = v < 0.0 ? 1.f : 0.f; break;
    default: reinterpret_cast<double*>(p)[i] = v;
  }
}

// scipy ni_splines.c, order 3, mirror boundaries: gain, causal init (full mirrored sum), causal pass, anticausal init and pass.
// LD(i) reads x[i] of the line (any dtype), C(i) is the fp64 coefficient slot; both may alias (in place)
#define SDM_PREFILTER(LD, C, n, z, zn1)                                                  \
  do {                                                                                   \
    const double gain_ = (1.0 - (z)) * (1.0 - 1.0 / (z));                                \
    double c0_ = LD(0) * gain_ + (zn1) * (LD((n) - 1) * gain_);                          \
    double zi_ = (z);                                                                    \
    for (int i_ = 1; i_ < (n) - 1; ++i_) {                                               \
      c0_ += zi_ * (LD(i_) * gain_ + (zn1) * (LD((n) - 1 - i_) * gain_));                \
      zi_ *= (z);                                                                        \
    }                                                                                    \
    double prev_ = c0_ / (1.0 - (zn1) * (zn1));                                          \
    C(0) = prev_;                                                                        \
    for (int i_ = 1; i_ < (n); ++i_) { prev_ = LD(i_) * gain_ + (z) * prev_; C(i_) = prev_; } \
    double nxt_ = ((z) * C((n) - 2) + prev_) * (z) / ((z) * (z) - 1.0);                  \
    C((n) - 1) = nxt_;                                                                   \
    for (int i_ = (n) - 2; i_ >= 0; --i_) { nxt_ = (z) * (nxt_ - C(i_)); C(i_) = nxt_; } \
  } while (0)

// lines along a strided axis (inner > 1): one thread per line, each recurrence step a coalesced row access across the lanes
__global__ __launch_bounds__(256) void sdm_prefilter_strided_kernel(const void* __restrict__ src, int src_dtype, double* __restrict__ dst,
                                                                    int64_t lines, int n, int64_t inner, double z, double zn1) {
  const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (l >= lines) return;
  const int64_t base = (l / inner) * n * inner + l % inner;
#define LD_(i) sdm_load(src, base + (int64_t)(i) * inner, src_dtype)
#define C_(i) dst[base + (int64_t)(i) * inner]
  SDM_PREFILTER(LD_, C_, n, z, zn1);
#undef LD_
#undef C_
}

// lines along the contiguous axis: SDM_LINES consecutive rows staged in LDS with coalesced loads, one lane per line
__global__ __launch_bounds__(SDM_LINES) void sdm_prefilter_rows_kernel(const void* __restrict__ src, int src_dtype, double* __restrict__ dst,
                                                                       int64_t lines, int n, double z, double zn1) {
  extern __shared__ double lds[];
  const int64_t l0 = (int64_t)blockIdx.x * SDM_LINES;
  const int nl = (int)min((int64_t)SDM_LINES, lines - l0);
  const int64_t off = l0 * n;
  for (int e = threadIdx.x; e < nl * n; e += SDM_LINES) {
    const int line = e / n, i = e - line * n;
    lds[i * SDM_LDS_PITCH + line] = sdm_load(src, off + e, src_dtype);
  }
  __syncthreads();
  if ((int)threadIdx.x < nl) {
    double* c = lds + threadIdx.x;
#define LD_(i) c[(i) * SDM_LDS_PITCH]
#define C_(i) c[(i) * SDM_LDS_PITCH]
    SDM_PREFILTER(LD_, C_, n, z, zn1);
#undef LD_
#undef C_
  }
  __syncthreads();
  for (int e = threadIdx.x; e < nl * n; e += SDM_LINES) {
    const int line = e / n, i = e - line * n;
    dst[off + e] = lds[i * SDM_LDS_PITCH + line];
  }
}

__device__ __forceinline__ int sdm_mirror(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  i = abs(i) % p;
  return i >= n ? p - i : i;
}

// one axis of the separable evaluation: (outer, n_in, inner) -> (outer, n_out, inner), output index o reads the spline at
// coordinate (lo + o) * scale (scale = (n_in - 1) / (n_full - 1)), taps floor - 1 .. floor + 2 with mirrored indices
__global__ __launch_bounds__(256) void sdm_resample_kernel(const double* __restrict__ c, void* __restrict__ out, int out_dtype, int64_t total,
                                                           int n_in, int n_out, int64_t inner, int lo, double scale) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t k = idx % inner, r = idx / inner;
  const int o = (int)(r % n_out);
  const int64_t outer = r / n_out;
  const double cc = (double)(lo + o) * scale;
  const double f = floor(cc), y = cc - f, zz = 1.0 - y;
  double w[4];
  w[0] = zz * zz * zz / 6.0;
  w[1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
  w[2] = (zz * zz * (zz - 2.0) * 3.0 + 4.0) / 6.0;
  w[3] = 1.0 - w[0] - w[1] - w[2];
  const int s = (int)f - 1;
  const double* line = c + outer * n_in * inner + k;
  double acc = 0.0;
#pragma unroll
  for (int t = 0; t < 4; ++t) acc += w[t] * line[(int64_t)sdm_mirror(s + t, n_in) * inner];
  sdm_store(out, idx, out_dtype, acc);
}

struct ZoomPlan {
  int nd, batch;
  int in[SDM_MAXDIM], full[SDM_MAXDIM];
  int64_t ws_bytes;
};

static int zoom_plan(int32_t ndim, const int32_t* in_dims, const int32_t* full_dims, int32_t batch, ZoomPlan* p, const char* who) {
  SP_CHECK_ARG(ndim >= 1 && ndim <= SDM_MAXDIM && batch >= 1, "%s: rank %d (1..3) or batch %d", who, ndim, batch);
  p->nd = ndim;
  p->batch = batch;
  int64_t nin = 1, nmax = 1;
  bool any = false;
  for (int a = 0; a < ndim; ++a) {
    p->in[a] = in_dims[a];
    p->full[a] = full_dims[a];
    SP_CHECK_ARG(in_dims[a] >= 1 && full_dims[a] >= 1 && in_dims[a] < (1 << 20) && full_dims[a] < (1 << 20), "%s: bad extent on axis %d", who, a);
    nin *= in_dims[a];
    nmax *= in_dims[a] > full_dims[a] ? in_dims[a] : full_dims[a];
    any = any || in_dims[a] != full_dims[a];
  }
  SP_CHECK_ARG(any, "%s: no axis changes its extent", who);
  SP_CHECK_ARG(batch * nmax < (1ll << 31), "%s: volume too large", who);
  p->ws_bytes = (int64_t)sizeof(double) * batch * (nin + 2 * nmax);
  return SP_OK;
}

static int full_extents(int32_t ndim, const int32_t* in_dims, const double* factors, int32_t* full, const char* who) {
  SP_CHECK_ARG(ndim >= 1 && ndim <= SDM_MAXDIM, "%s: rank %d (1..3)", who, ndim);
  for (int a = 0; a < ndim; ++a) {
    SP_CHECK_ARG(factors[a] > 0.0 && in_dims[a] >= 1, "%s: bad factor or extent on axis %d", who, a);
    full[a] = (int32_t)nearbyint((double)in_dims[a] * factors[a]);     // Python's round(n * f): half to even
    SP_CHECK_ARG(full[a] >= 1, "%s: axis %d zooms to an empty extent", who, a);
  }
  return SP_OK;
}

extern "C" int sp_sdm_zoom_plan(int32_t ndim, const int32_t* in_dims, const double* factors, int32_t batch, int32_t* full_dims,
                                int64_t* ws_bytes) {
  SP_CHECK_ARG(in_dims && factors && full_dims && ws_bytes, "sp_sdm_zoom_plan: null pointer");
  int rc = full_extents(ndim, in_dims, factors, full_dims, "sp_sdm_zoom_plan");
  if (rc) return rc;
  ZoomPlan p;
  rc = zoom_plan(ndim, in_dims, full_dims, batch, &p, "sp_sdm_zoom_plan");
  if (rc) return rc;
  *ws_bytes = p.ws_bytes;
  return SP_OK;
}

extern "C" int sp_sdm_zoom(const void* src, int32_t src_dtype, void* dst, int32_t dst_dtype, int32_t batch, int32_t ndim,
                           const int32_t* in_dims, const int32_t* full_dims, const int32_t* crop_lo, const int32_t* crop_n, void* ws,
                           int64_t ws_bytes, sp_stream_t stream) {
  SP_CHECK_ARG(src && dst && in_dims && full_dims && ws, "sp_sdm_zoom: null pointer");
  SP_CHECK_ARG(src_dtype == SP_SDM_F64 || src_dtype == SP_SDM_I8 || src_dtype == SP_SDM_F32_AS_I8, "sp_sdm_zoom: source dtype %d", src_dtype);
  SP_CHECK_ARG(dst_dtype == SP_SDM_F64 || dst_dtype == SP_SDM_I8 || dst_dtype == SP_SDM_MASK_GT0 || dst_dtype == SP_SDM_MASK_LT0,
               "sp_sdm_zoom: output dtype %d", dst_dtype);
  ZoomPlan p;
  int rc = zoom_plan(ndim, in_dims, full_dims, batch, &p, "sp_sdm_zoom");
  if (rc) return rc;
  SP_CHECK_ARG(ws_bytes >= p.ws_bytes, "sp_sdm_zoom: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)p.ws_bytes);
  int lo[SDM_MAXDIM], cn[SDM_MAXDIM];
  for (int a = 0; a < ndim; ++a) {
    lo[a] = crop_lo ? crop_lo[a] : 0;
    cn[a] = crop_n ? crop_n[a] : p.full[a];
    SP_CHECK_ARG(lo[a] >= 0 && cn[a] >= 1 && lo[a] + cn[a] <= p.full[a], "sp_sdm_zoom: crop [%d, %d) outside axis %d of extent %d", lo[a],
                 lo[a] + cn[a], a, p.full[a]);
    SP_CHECK_ARG(p.in[a] != p.full[a] || (lo[a] == 0 && cn[a] == p.full[a]), "sp_sdm_zoom: crop on axis %d, which keeps its extent", a);
    SP_CHECK_ARG(p.in[a] == p.full[a] || p.in[a] == 1 || a < ndim - 1 || p.in[a] <= SDM_MAX_LDS_LINE,
                 "sp_sdm_zoom: contiguous axis of %d > %d samples", p.in[a], SDM_MAX_LDS_LINE);
  }
  hipStream_t st = ST(stream);
  int64_t nin = 1, nmax = 1;
  for (int a = 0; a < ndim; ++a) { nin *= p.in[a]; nmax *= p.in[a] > p.full[a] ? p.in[a] : p.full[a]; }
  double* coef = reinterpret_cast<double*>(ws);
  double* tmp[2] = {coef + (int64_t)batch * nin, coef + (int64_t)batch * (nin + nmax)};
  const double z = sqrt(3.0) - 2.0;
  // prefilter every axis that changes extent (an axis of factor 1 is evaluated at the knots, where the spline reproduces the data)
  const void* cur = src;
  int cur_dtype = src_dtype;
  for (int a = 0; a < ndim; ++a) {
    if (p.in[a] == p.full[a] || p.in[a] == 1) continue;
    int64_t inner = 1, lines = batch;
    for (int b = 0; b < ndim; ++b) {
      if (b > a) inner *= p.in[b];
      if (b != a) lines *= p.in[b];
    }
    const double zn1 = pow(z, (double)(p.in[a] - 1));
    if (inner > 1) {
      hipLaunchKernelGGL(sdm_prefilter_strided_kernel, dim3((unsigned)((lines + 255) / 256)), dim3(256), 0, st, cur, cur_dtype, coef, lines,
                         p.in[a], inner, z, zn1);
    } else {
      const int lds = SDM_LDS_PITCH * p.in[a] * (int)sizeof(double);
      SP_ENSURE_LDS(sdm_prefilter_rows_kernel, lds, "sp_sdm_zoom");
      hipLaunchKernelGGL(sdm_prefilter_rows_kernel, dim3((unsigned)((lines + SDM_LINES - 1) / SDM_LINES)), dim3(SDM_LINES), lds, st, cur,
                         cur_dtype, coef, lines, p.in[a], z, zn1);
    }
    cur = coef;
    cur_dtype = SP_SDM_F64;
  }
  if (cur == src) {      // only axes of extent 1 change: no filter, the data are the coefficients
    SP_CHECK_ARG(src_dtype == SP_SDM_F64, "sp_sdm_zoom: an integer source needs a filtered axis");
  }
  // separable evaluation, axis by axis; the last pass writes dst in its dtype
  int dims[SDM_MAXDIM];
  for (int a = 0; a < ndim; ++a) dims[a] = p.in[a];
  int last = -1;
  for (int a = 0; a < ndim; ++a) if (p.in[a] != p.full[a]) last = a;
  int pp = 0;
  for (int a = 0; a < ndim; ++a) {
    if (p.in[a] == p.full[a]) continue;
    int64_t inner = 1, outer = batch;
    for (int b = 0; b < ndim; ++b) {
      if (b > a) inner *= dims[b];
      if (b < a) outer *= dims[b];
    }
    const double scale = p.full[a] > 1 ? (double)(p.in[a] - 1) / (double)(p.full[a] - 1) : 1.0;
    const int64_t total = outer * cn[a] * inner;
    void* out = a == last ? dst : (void*)tmp[pp];
    hipLaunchKernelGGL(sdm_resample_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const double*)cur, out,
                       a == last ? dst_dtype : (int)SP_SDM_F64, total, dims[a], cn[a], inner, lo[a], scale);
    dims[a] = cn[a];
    cur = out;
    pp ^= 1;
  }
  SP_CHECK_LAUNCH("sp_sdm_zoom");
  return SP_OK;
}

// ------------------------------------------------------------------------------------------------ blend and masks
// v[k][i] = penu[i] * t_k - core[i] * (1 - t_k) in fp64 without contraction: two rounded products, one rounded difference, as
// numpy computes it.  (1 - t_k) is rounded in the dtype of t: numpy keeps `1 - t` in float32 for a float32 scalar t.
__global__ __launch_bounds__(256) void sdm_blend_kernel(const double* __restrict__ penu, const double* __restrict__ core, const void* __restrict__ t,
                                                        int t_dtype, int T, int64_t n, const double* __restrict__ intp_in,
                                                        double* __restrict__ intp_out, float* __restrict__ masks) {
#pragma clang fp contract(off)
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)T * n) return;
  const int k = (int)(idx / n);
  const int64_t i = idx - (int64_t)k * n;
  double v;
  if (intp_in) {
    v = intp_in[idx];
  } else {
    double tk, uk;
    if (t_dtype == SP_SDM_F32) {
      const float tf = reinterpret_cast<const float*>(t)[k];
      tk = (double)tf;
      uk = (double)(1.0f - tf);
    } else {
      tk = reinterpret_cast<const double*>(t)[k];
      uk = 1.0 - tk;
    }
    const double a = penu[i] * tk;
    const double b = core[i] * uk;
    v = a - b;
  }
  if (intp_out) intp_out[idx] = v;
  if (masks) {
    masks[idx] = v > 0.0 ? 1.f : 0.f;
    if (k == 0) {
      masks[(int64_t)T * n + i] = core[i] < 0.0 ? 1.f : 0.f;
      masks[(int64_t)(T + 1) * n + i] = penu[i] > 0.0 ? 1.f : 0.f;
    }
  }
}

extern "C" int sp_sdm_blend(const double* penu, const double* core, const void* t, int32_t t_dtype, int32_t T, int64_t n,
                            const double* intp_in, double* intp_out, float* masks, sp_stream_t stream) {
  SP_CHECK_ARG(penu && core, "sp_sdm_blend: null field");
  SP_CHECK_ARG((intp_in != nullptr) != (intp_out != nullptr), "sp_sdm_blend: exactly one of intp_in / intp_out");
  SP_CHECK_ARG(intp_in || t, "sp_sdm_blend: null t");
  SP_CHECK_ARG(intp_out || masks, "sp_sdm_blend: nothing to write");
  SP_CHECK_ARG(t_dtype == SP_SDM_F64 || t_dtype == SP_SDM_F32, "sp_sdm_blend: t dtype %d", t_dtype);
  SP_CHECK_ARG(T >= 1 && n >= 1 && (int64_t)T * n < (1ll << 31), "sp_sdm_blend: bad sizes T=%d n=%lld", T, (long long)n);
  const int64_t total = (int64_t)T * n;
  hipLaunchKernelGGL(sdm_blend_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ST(stream), penu, core, t, t_dtype, T, n, intp_in,
                     intp_out, masks);
  SP_CHECK_LAUNCH("sp_sdm_blend");
  return SP_OK;
}

// ------------------------------------------------------------------------------------------------ planning (host only)
extern "C" int sp_sdm_plan(int32_t D, int32_t H, int32_t W, double zoom, int32_t resample, int32_t T, int32_t* ext, int64_t* ws_bytes) {
  SP_CHECK_ARG(ext && ws_bytes, "sp_sdm_plan: null pointer");
  SP_CHECK_ARG(D >= 1 && H >= 1 && W >= 1 && D < 4096 && H < 4096 && W < 4096 && zoom > 0.0 && T >= 1,
               "sp_sdm_plan: bad arguments D=%d H=%d W=%d zoom=%g T=%d", D, H, W, zoom, T);
  const int32_t in[3] = {D, H, W};
  const double down[3] = {1.0, 1.0 / zoom, 1.0 / zoom};
  int32_t lat[3];
  int rc = full_extents(3, in, down, lat, "sp_sdm_plan");
  if (rc) return rc;
  int64_t need = fields_ws_bytes((int64_t)D * H * W);
  ZoomPlan p;
  if (lat[1] != H || lat[2] != W) {
    rc = zoom_plan(3, in, lat, 2, &p, "sp_sdm_plan");
    if (rc) return rc;
    need = need > p.ws_bytes ? need : p.ws_bytes;
  }
  int32_t rec[3] = {D, H, W};
  if (resample) {
    const double up[3] = {1.0, zoom, zoom};
    int32_t full[3];
    rc = full_extents(3, lat, up, full, "sp_sdm_plan");
    if (rc) return rc;
    // the reference's hard-coded crop [:, 2:130, 2:130] (test_sdm_resampling.py:42-43,50), numpy slice semantics
    for (int a = 1; a < 3; ++a) rec[a] = (full[a] < 130 ? full[a] : 130) - 2;
    SP_CHECK_ARG(rec[1] >= 1 && rec[2] >= 1, "sp_sdm_plan: the [2:130] crop of a %d x %d upsampled plane is empty", full[1], full[2]);
    if (full[1] != lat[1] || full[2] != lat[2]) {
      rc = zoom_plan(3, lat, full, 2 + T, &p, "sp_sdm_plan");
      if (rc) return rc;
      need = need > p.ws_bytes ? need : p.ws_bytes;
    }
  }
  ext[0] = lat[0]; ext[1] = lat[1]; ext[2] = lat[2];
  ext[3] = rec[0]; ext[4] = rec[1]; ext[5] = rec[2];
  *ws_bytes = need;
  return SP_OK;
}
