// Batched patch gather for the device-resident case cache (common/data.py:DeviceCaseCache / CachedBatchLoader): what
// HemisphericFlip -> PadImages -> RandomPatch -> ToTensor -> default_collate do with a flip, a torch.full, a slice assignment, two
// slices and a stack PER SAMPLE, done for a whole batch and both tensors (images and labels) in ONE launch.
// The cache holds every case in the ToTensor layout, (N, C, Z, Y, X) fp32 with X contiguous; sample b of the batch names its case,
// its patch origin (in PADDED coordinates) and its flip flag in one row of a small table.  Output element
//   dst_t[b, c, z, y, x] = src_t[case, c, oz + z - pz_t, oy + y - py_t, flip ? X - 1 - u : u],   u = ox + x - px_t,
// or padval_t when (u, v, s) leaves the volume: flipping and then padding symmetrically equals padding and then flipping, so the
// mirror is applied to the in-range source index alone.  Pure data movement: no LDS, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sp_common.h"

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define GATHER_THREADS 256

struct GatherGroup {
  const float* src;      // (N, C, Z, Y, X)
  float* dst;            // (B, C, d, h, w)
  int32_t C, w, h, d, px, py, pz;
  float padval;
  int32_t vec;           // 1: a thread writes four consecutive x with one 16-byte store (w % 4 == 0 and dst 16-byte aligned)
  int32_t nblk;          // workgroups per (sample, channel) volume
};

// Workgroup id -> (group, sample, channel, block of the volume): group 0's B * C0 * nblk0 workgroups first, then group 1's.
// Consecutive lanes cover consecutive x (or consecutive quads of x) of one output row and run on into the next row.
__global__ __launch_bounds__(GATHER_THREADS) void patch_gather_batch_kernel(GatherGroup g0, GatherGroup g1, const int32_t* __restrict__ table,
                                                                            uint32_t blocks0, int N, int Z, int Y, int X) {
  uint32_t bid = blockIdx.x;
  const bool second = bid >= blocks0;
  if (second) bid -= blocks0;
  const float* __restrict__ src = second ? g1.src : g0.src;
  float* __restrict__ dst = second ? g1.dst : g0.dst;
  const int C = second ? g1.C : g0.C, w = second ? g1.w : g0.w, h = second ? g1.h : g0.h, d = second ? g1.d : g0.d;
  const int px = second ? g1.px : g0.px, py = second ? g1.py : g0.py, pz = second ? g1.pz : g0.pz;
  const float padval = second ? g1.padval : g0.padval;
  const int vec = second ? g1.vec : g0.vec;
  const uint32_t nblk = (uint32_t)(second ? g1.nblk : g0.nblk);
  const uint32_t vol = bid / nblk, blk = bid - vol * nblk;
  const int b = (int)(vol / (uint32_t)C), c = (int)(vol - (uint32_t)b * (uint32_t)C);
  const int32_t* __restrict__ row = table + (int64_t)b * 5;
  const int cs = row[0];
  const int64_t ox = row[1], oy = row[2], oz = row[3];
  const bool mirror = row[4] != 0;
  const int wq = vec ? w >> 2 : w;                                   // work items per output row
  const int64_t i = (int64_t)blk * GATHER_THREADS + threadIdx.x;
  if (i >= (int64_t)wq * h * d) return;
  const int xq = (int)(i % wq);
  const int64_t r = i / wq;
  const int y = (int)(r % h), z = (int)(r / h);
  const int64_t v = oy + y - py, s = oz + z - pz;
  const bool row_in = cs >= 0 && cs < N && v >= 0 && v < Y && s >= 0 && s < Z;
  const float* __restrict__ line = src + ((((int64_t)(row_in ? cs : 0) * C + c) * Z + (row_in ? s : 0)) * Y + (row_in ? v : 0)) * X;
  float* __restrict__ out = dst + (((int64_t)vol * d + z) * h + y) * w;
  if (!vec) {
    const int64_t u = ox + xq - px;
    float val = padval;
    if (row_in && u >= 0 && u < X) val = line[mirror ? X - 1 - u : u];
    out[xq] = val;
    return;
  }
  const int x0 = xq << 2;
  const int64_t u0 = ox + x0 - px;                                   // the quad reads u0 .. u0 + 3
  float q[4];
  // the four sources as they lie in memory: ascending from `lo` (mirrored: the quad read backwards)
  const int64_t lo = mirror ? X - 1 - (u0 + 3) : u0;
  if (row_in && u0 >= 0 && u0 + 3 < X && ((reinterpret_cast<uintptr_t>(line + lo) & 15) == 0)) {
    const float4 t = *reinterpret_cast<const float4*>(line + lo);
    q[0] = mirror ? t.w : t.x;
    q[1] = mirror ? t.z : t.y;
    q[2] = mirror ? t.y : t.z;
    q[3] = mirror ? t.x : t.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t u = u0 + k;
      q[k] = (row_in && u >= 0 && u < X) ? line[mirror ? X - 1 - u : u] : padval;
    }
  }
  *reinterpret_cast<float4*>(out + x0) = make_float4(q[0], q[1], q[2], q[3]);
}

static int gather_group(GatherGroup* g, const char* which, const float* src, float* dst, int32_t C, const int32_t* ext, const int32_t* pad,
                        float padval) {
  g->src = src; g->dst = dst; g->C = C; g->padval = padval;
  g->w = g->h = g->d = 1; g->px = g->py = g->pz = 0; g->vec = 0; g->nblk = 1;
  if (C == 0) return SP_OK;
  SP_CHECK_ARG(ext && pad, "sp_patch_gather_batch: group %s has %d channels but no extents / padding", which, C);
  // the extents first: an output without elements has no address to check
  SP_CHECK_ARG(ext[0] >= 1 && ext[1] >= 1 && ext[2] >= 1, "sp_patch_gather_batch: group %s extents (%d, %d, %d) must be positive", which,
               ext[0], ext[1], ext[2]);
  SP_CHECK_ARG(src && dst, "sp_patch_gather_batch: group %s has %d channels but a NULL pointer", which, C);
  const int64_t total = (int64_t)ext[0] * ext[1] * ext[2];
  SP_CHECK_ARG(total < (1ll << 31), "sp_patch_gather_batch: group %s: 2^31 or more output voxels per volume", which);
  g->w = ext[0]; g->h = ext[1]; g->d = ext[2];
  g->px = pad[0]; g->py = pad[1]; g->pz = pad[2];
  // every output row starts 16-byte aligned when the base does and w is a multiple of 4 (a volume then is one too)
  g->vec = (ext[0] % 4 == 0) && (reinterpret_cast<uintptr_t>(dst) % 16 == 0);
  const int64_t items = g->vec ? total / 4 : total;
  g->nblk = (int32_t)((items + GATHER_THREADS - 1) / GATHER_THREADS);
  return SP_OK;
}

extern "C" int sp_patch_gather_batch(const float* src0, float* dst0, int32_t C0, const int32_t* ext0, const int32_t* pad0, float padval0,
                                     const float* src1, float* dst1, int32_t C1, const int32_t* ext1, const int32_t* pad1, float padval1,
                                     const int32_t* table, int32_t N, int32_t B, int32_t Z, int32_t Y, int32_t X, sp_stream_t stream) {
  SP_CHECK_ARG(table && B >= 1 && N >= 1 && Z >= 1 && Y >= 1 && X >= 1 && C0 >= 0 && C1 >= 0,
               "sp_patch_gather_batch: bad arguments (table, B >= 1, N >= 1, Z, Y, X >= 1, C0, C1 >= 0)");
  SP_CHECK_ARG(C0 + C1 >= 1, "sp_patch_gather_batch: both groups are empty (C0 = C1 = 0)");
  SP_CHECK_ARG((int64_t)Z * Y * X < (1ll << 31), "sp_patch_gather_batch: 2^31 or more voxels per cached volume");
  GatherGroup g0, g1;
  int rc = gather_group(&g0, "0", src0, dst0, C0, ext0, pad0, padval0);
  if (rc != SP_OK) return rc;
  rc = gather_group(&g1, "1", src1, dst1, C1, ext1, pad1, padval1);
  if (rc != SP_OK) return rc;
  const int64_t blocks0 = (int64_t)B * C0 * g0.nblk, blocks1 = (int64_t)B * C1 * g1.nblk;
  SP_CHECK_ARG(blocks0 + blocks1 < (1ll << 31), "sp_patch_gather_batch: B = %d needs %lld workgroups, above the grid limit of 2^31 - 1", B,
               (long long)(blocks0 + blocks1));
  hipLaunchKernelGGL(patch_gather_batch_kernel, dim3((unsigned)(blocks0 + blocks1)), dim3(GATHER_THREADS), 0, ST(stream), g0, g1, table,
                     (uint32_t)blocks0, N, Z, Y, X);
  SP_CHECK_LAUNCH("sp_patch_gather_batch");
  return SP_OK;
}
