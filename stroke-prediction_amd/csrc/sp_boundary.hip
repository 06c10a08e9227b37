// The boundary (signed-distance) criteria (include/stroke_amd.h; Kervadec et al., MIDL 2019: loss = mean(o * phi(t))):
//   * sp_signed_distance_batch: phi of every (sample, channel) volume of a label batch -- outside the mask the Euclidean distance to
//     it, inside -(distance to the background - 1), zero for an empty or a full mask -- on the exact separable transform of sp_edt.h.
//     The two transforms of all B * C volumes are one (2 B C D, H, W) stack: a seed launch, a launch per axis, a launch for the roots.
// The criterion that reads phi (sp_bloss_sums / _finalize_clear / _bwd) is in sp_loss.hip.
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
