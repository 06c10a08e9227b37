// Stack input of the CTP-conditioned CAE encoder (common/model/Cae3D.py Enc3DCtp; reference Cae3D.py:151-165): every pass of
// one encoder call encodes cat(shape label, CBV, TTD), the two perfusion maps cut out of their padded volumes.  One launch
// builds the channels-last stack input of all G passes,
//   x0[g B + b][d][h][w][0..CP) = (label_g, CBV, TTD, 0, ..., 0),
// bit-equal to crop -> torch.cat -> sp_ncdhw_to_cl, and in training adds the per-pass BatchNorm batch statistics of the STORED
// values (bf16-rounded in bf16) into the first layer's accumulator -- the work of three crops, three concatenations, a batch
// concatenation, a layout pass and G sp_bn_stats passes.
//
// One thread = one (spatial voxel, 16-byte chunk of the output voxel); the chunk is the fastest index, so a wave writes 1 KiB
// of contiguous output per store.  Chunk 0 holds channels 0..2 (and zeros), every other chunk is zeros.  The thread of chunk 0
// reads the voxel's CBV / TTD once and the G labels (coalesced along W), and writes the G output voxels.  CBV / TTD are the
// same in all passes: their sums are reduced once and added to every pass's region.  Sums are kept in fp64 per thread (the
// products of fp32 values are exact there), reduced wave -> LDS (in wave order) -> one fp64 atomic per value and workgroup into
// replica row (workgroup % nrep) of each pass's region, as the elementwise kernels do (sp_elem.hip).
#include "sp_common.h"

#define ST(s) reinterpret_cast<hipStream_t>(s)

enum { CTP_MAXG = 4, CTP_NVAL = (CTP_MAXG + 2) * 2 };

struct CtpArgs {
  const float* lab[CTP_MAXG];
  int64_t lab_bs[CTP_MAXG];
  const float* cbv;
  const float* ttd;
  int64_t cbv_bs, ttd_bs;
  void* x0;
  double* sums;
  int64_t gstride;              // doubles per pass region of sums
  int64_t pass_vox;             // B * D * H * W: output voxels of one pass
  uint32_t items;               // B * D * H * W * chunks per voxel
  int32_t G, W, H, DH, Hp, Wp, oD, oH, oW, CP, lnch, nrep;
  FastDiv dW, dH, dDH;
};

template <typename T, bool STATS>
__global__ __launch_bounds__(256) void ctp_stack_input_kernel(CtpArgs a) {
  constexpr int EPC = 16 / sizeof(T);                          // elements per 16-byte chunk
  const uint32_t nch = 1u << a.lnch;
  const uint32_t first = blockIdx.x * 256u + threadIdx.x;
  const uint32_t chunk = first & (nch - 1);                    // fixed over the grid-stride loop (the stride is a multiple of 256)
  double s[CTP_NVAL];                                          // (sum, sum of squares): label of pass 0..MAXG-1, CBV, TTD
#pragma unroll
  for (int k = 0; k < CTP_NVAL; ++k) s[k] = 0.0;
  T* x0 = reinterpret_cast<T*>(a.x0);
  for (uint32_t it = first; it < a.items; it += gridDim.x * 256u) {
    const uint32_t q = it >> a.lnch;                           // spatial voxel of one pass: (b, d, h, w)
    const uint32_t row = fdiv(q, a.dW), w = q - row * (uint32_t)a.W;
    const uint32_t b = fdiv(row, a.dDH), dh = row - b * (uint32_t)a.DH;
    T* dst = x0 + (int64_t)q * a.CP + chunk * EPC;
    if (chunk != 0) {
#pragma unroll
      for (int g = 0; g < CTP_MAXG; ++g)
        if (g < a.G) *reinterpret_cast<uint4*>(dst + g * a.pass_vox * a.CP) = make_uint4(0u, 0u, 0u, 0u);
      continue;
    }
    const uint32_t d = fdiv(dh, a.dH), h = dh - d * (uint32_t)a.H;
    const int64_t src = ((int64_t)(d + a.oD) * a.Hp + (h + a.oH)) * a.Wp + (w + a.oW);
    const float cv = a.cbv[(int64_t)b * a.cbv_bs + src], tv = a.ttd[(int64_t)b * a.ttd_bs + src];
    float lv[CTP_MAXG];
#pragma unroll
    for (int g = 0; g < CTP_MAXG; ++g) lv[g] = g < a.G ? a.lab[g][(int64_t)b * a.lab_bs[g] + (int64_t)dh * a.W + w] : 0.f;
    float cs, ts;                                              // CBV / TTD as stored
    if constexpr (sizeof(T) == 2) {
      const uint32_t ct = sp_pack_bf16x2(cv, tv);
      cs = sp_h2f_lo(ct);
      ts = sp_h2f_hi(ct);
    } else {
      cs = cv;
      ts = tv;
    }
#pragma unroll
    for (int g = 0; g < CTP_MAXG; ++g) {
      if (g < a.G) {
        uint4 word;
        float ls;
        if constexpr (sizeof(T) == 2) {
          const uint32_t w0 = sp_pack_bf16x2(lv[g], cv);
          word = make_uint4(w0, sp_pack_bf16x2(tv, 0.f), 0u, 0u);
          ls = sp_h2f_lo(w0);
        } else {
          word = make_uint4(__float_as_uint(lv[g]), __float_as_uint(cv), __float_as_uint(tv), 0u);
          ls = lv[g];
        }
        *reinterpret_cast<uint4*>(dst + g * a.pass_vox * a.CP) = word;
        if (STATS) {
          s[2 * g] += (double)ls;
          s[2 * g + 1] += (double)ls * (double)ls;
        }
      }
    }
    if (STATS) {
      s[2 * CTP_MAXG] += (double)cs;
      s[2 * CTP_MAXG + 1] += (double)cs * (double)cs;
      s[2 * CTP_MAXG + 2] += (double)ts;
      s[2 * CTP_MAXG + 3] += (double)ts * (double)ts;
    }
  }
  if (STATS) {
    __shared__ double red[4][CTP_NVAL];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < CTP_NVAL; ++k) {
      const double v = wave_sum_d(s[k]);
      if (lane == 0) red[wv][k] = v;
    }
    __syncthreads();
    // threads [0, 2G): the labels' (sum, sum of squares) into their own pass's region; [2G, 6G): the four CBV / TTD values
    // into every pass's region
    const int t = threadIdx.x;
    if (t < 6 * a.G) {
      int g, ch, k;
      if (t < 2 * a.G) {
        g = t >> 1; ch = 0; k = t;
      } else {
        const int u = t - 2 * a.G;
        g = u >> 2; ch = 1 + ((u & 3) >> 1); k = 2 * CTP_MAXG + (u & 3);
      }
      const double v = red[0][k] + red[1][k] + red[2][k] + red[3][k];
      atomicAdd(&a.sums[g * a.gstride + (int64_t)(blockIdx.x % a.nrep) * a.CP * 2 + ch * 2 + (k & 1)], v);
    }
  }
}

extern "C" int sp_ctp_stack_input(const float* const* labels, const int64_t* label_bstride, int32_t G, int32_t B, int32_t D,
                                  int32_t H, int32_t W, const float* cbv, int64_t cbv_bstride, const float* ttd,
                                  int64_t ttd_bstride, int32_t Dp, int32_t Hp, int32_t Wp, int32_t oD, int32_t oH, int32_t oW,
                                  void* x0, int32_t dtype, int32_t CP, double* sums, int64_t sums_gstride, int32_t nrep,
                                  sp_stream_t stream) {
  SP_CHECK_ARG(labels && label_bstride && G >= 1 && G <= CTP_MAXG, "sp_ctp_stack_input: bad arguments (G=%d, at most %d passes)",
               G, (int)CTP_MAXG);
  SP_CHECK_ARG(B >= 1 && D >= 1 && H >= 1 && W >= 1 && cbv && ttd && x0 && ((uintptr_t)x0 & 15) == 0,
               "sp_ctp_stack_input: bad arguments (extents, pointers or a stack input not 16-byte aligned)");
  SP_CHECK_ARG(oD >= 0 && oH >= 0 && oW >= 0 && oD + D <= Dp && oH + H <= Hp && oW + W <= Wp,
               "sp_ctp_stack_input: the crop [%d, %d) x [%d, %d) x [%d, %d) is outside the CTP volume %d x %d x %d", oD, oD + D,
               oH, oH + H, oW, oW + W, Dp, Hp, Wp);
  SP_CHECK_ARG(dtype == SP_BF16 || dtype == SP_F32, "sp_ctp_stack_input: bad arguments (dtype=%d)", dtype);
  const int esz = dtype == SP_BF16 ? 2 : 4;
  const int nch = CP * esz / 16;
  SP_CHECK_ARG(CP >= 8 && CP % 8 == 0 && (nch & (nch - 1)) == 0, "sp_ctp_stack_input: bad arguments (CP=%d)", CP);
  SP_CHECK_ARG(!sums || (nrep >= 1 && sums_gstride >= (int64_t)nrep * CP * 2),
               "sp_ctp_stack_input: bad arguments (nrep=%d, sums_gstride=%lld)", nrep, (long long)sums_gstride);
  const int64_t pass_vox = (int64_t)B * D * H * W;
  SP_CHECK_ARG(pass_vox * nch < ((int64_t)1 << 31), "sp_ctp_stack_input: volume too large (%lld voxels)", (long long)pass_vox);
  CtpArgs a;
  for (int g = 0; g < CTP_MAXG; ++g) {
    a.lab[g] = g < G ? labels[g] : nullptr;
    a.lab_bs[g] = g < G ? label_bstride[g] : 0;
    SP_CHECK_ARG(g >= G || labels[g], "sp_ctp_stack_input: label %d is null", g);
  }
  a.cbv = cbv; a.ttd = ttd; a.cbv_bs = cbv_bstride; a.ttd_bs = ttd_bstride;
  a.x0 = x0; a.sums = sums; a.gstride = sums_gstride; a.pass_vox = pass_vox;
  a.items = (uint32_t)(pass_vox * nch);
  a.G = G; a.W = W; a.H = H; a.DH = D * H; a.Hp = Hp; a.Wp = Wp; a.oD = oD; a.oH = oH; a.oW = oW; a.CP = CP; a.nrep = nrep;
  a.lnch = 0;
  while ((1 << a.lnch) < nch) ++a.lnch;
  a.dW = make_fastdiv(W); a.dH = make_fastdiv(H); a.dDH = make_fastdiv(D * H);
  const int64_t nb = ((int64_t)a.items + 255) / 256;
  const unsigned grid = (unsigned)(nb > 2048 ? 2048 : nb);       // 8 workgroups per CU; the rest by the grid-stride loop
  if (dtype == SP_BF16) {
    if (sums) hipLaunchKernelGGL((ctp_stack_input_kernel<bf16_t, true>), dim3(grid), dim3(256), 0, ST(stream), a);
    else hipLaunchKernelGGL((ctp_stack_input_kernel<bf16_t, false>), dim3(grid), dim3(256), 0, ST(stream), a);
  } else {
    if (sums) hipLaunchKernelGGL((ctp_stack_input_kernel<float, true>), dim3(grid), dim3(256), 0, ST(stream), a);
    else hipLaunchKernelGGL((ctp_stack_input_kernel<float, false>), dim3(grid), dim3(256), 0, ST(stream), a);
  }
  SP_CHECK_LAUNCH("sp_ctp_stack_input");
  return SP_OK;
}
