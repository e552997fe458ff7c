// Time gradient of one conditional layer norm (the input gradient the parameter-gradient kernels of norm_fast.hip cannot give).
//
// Reference: ConditionalLayerNorm.forward (scOT/model.py:143-160): gamma = W_g·t + b_g, beta = W_b·t + b_b, y = gamma·xhat + beta,
// used as out = resid + s_b·y (model.py:570,574 with Swinv2DropPath's per-sample scale).  t enters through gamma and beta only, so
//   d_time[b] += s_b · Σ_{rows r of sample b} Σ_c dout[r,c] · (W_g[c]·xhat[r,c] + W_b[c]),     xhat = (x − mean_r)·rstd_r.
// The backward kernels keep Σ_b t_b·dgamma and Σ_b dgamma: the per-sample sums are gone there, hence this pass of its own.
//
// Memory-bound: dout and x are read once (16-byte loads, a sample's rows taken as one flat run of 8-element chunks so that every
// lane works whatever C is), W_g / W_b sit in LDS.  DETERMINISTIC: a block owns a fixed span of one sample, a thread sums its
// chunks in order, the wave sum is the xor-shuffle tree of common.h, the four waves are added in order by one thread; the blocks of
// a sample meet through `workspace` and a second launch adds them in a fixed order — no floating-point atomics anywhere.
#include "common.h"

constexpr int DT_LDS_C = 2048;     // widths up to this keep W_g / W_b in LDS (16 KB); wider ones read them through the caches
constexpr int DT_UNROLL = 4;       // units a thread has in flight
constexpr int DT_BLOCKS = 1024;    // blocks the plan aims for (4 per CU)

struct ClnDtimeArgs {
  const void* dout; const void* x; const float* mean; const float* rstd; const float* gw_w; const float* bw_w;
  const float* sscale; float* d_time; float* partial;
  int dout_dt, x_dt, rows_per_sample, C;
  unsigned units;     // per sample: 8-element chunks (VEC) or elements
  unsigned per;       // units per block
  int cps;            // blocks per sample
};

template <bool VEC>
__global__ __launch_bounds__(256) void cln_dtime_partial_kernel(ClnDtimeArgs p) {
  __shared__ __attribute__((aligned(16))) float sgw[DT_LDS_C];
  __shared__ __attribute__((aligned(16))) float sbw[DT_LDS_C];
  __shared__ float red[4];
  const int C = p.C;
  const bool in_lds = C <= DT_LDS_C;
  if (in_lds) {
    for (int c = threadIdx.x; c < C; c += 256) { sgw[c] = p.gw_w[c]; sbw[c] = p.bw_w[c]; }
  }
  __syncthreads();
  const int b = blockIdx.x / p.cps, chunk = blockIdx.x % p.cps;
  const unsigned u0 = (unsigned)chunk * p.per;
  const unsigned u1 = p.units - u0 < p.per ? p.units : u0 + p.per;
  const unsigned upr = VEC ? (unsigned)C / 8 : (unsigned)C;          // units per row
  const size_t row0 = (size_t)b * p.rows_per_sample;
  float acc = 0.f;
  for (unsigned u = u0 + threadIdx.x; u < u1; u += 256 * DT_UNROLL) {
    if (VEC) {
      float d[DT_UNROLL][8], xv[DT_UNROLL][8], mu[DT_UNROLL], rs[DT_UNROLL];
      int cc[DT_UNROLL];
#pragma unroll
      for (int i = 0; i < DT_UNROLL; ++i) {
        const unsigned uu = u + 256u * i;
        cc[i] = 0; mu[i] = 0.f; rs[i] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) { d[i][j] = 0.f; xv[i][j] = 0.f; }
        if (uu < u1) {      // (uu cannot wrap: units < 2^31 and the stride is 1024)
          const unsigned r = uu / upr;
          cc[i] = (int)(uu - r * upr) * 8;
          const size_t row = row0 + r;
          ld8(p.dout, p.dout_dt, row * C + cc[i], d[i]);
          ld8(p.x, p.x_dt, row * C + cc[i], xv[i]);
          mu[i] = p.mean[row]; rs[i] = p.rstd[row];
        }
      }
#pragma unroll
      for (int i = 0; i < DT_UNROLL; ++i) {
        float gw[8], bw[8];
        if (in_lds) {
          const float4 g0 = *(const float4*)(sgw + cc[i]), g1 = *(const float4*)(sgw + cc[i] + 4);
          const float4 b0 = *(const float4*)(sbw + cc[i]), b1 = *(const float4*)(sbw + cc[i] + 4);
          gw[0] = g0.x; gw[1] = g0.y; gw[2] = g0.z; gw[3] = g0.w; gw[4] = g1.x; gw[5] = g1.y; gw[6] = g1.z; gw[7] = g1.w;
          bw[0] = b0.x; bw[1] = b0.y; bw[2] = b0.z; bw[3] = b0.w; bw[4] = b1.x; bw[5] = b1.y; bw[6] = b1.z; bw[7] = b1.w;
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) { gw[j] = p.gw_w[cc[i] + j]; bw[j] = p.bw_w[cc[i] + j]; }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += d[i][j] * fmaf(gw[j], (xv[i][j] - mu[i]) * rs[i], bw[j]);      // (an idle slot holds d = 0)
      }
    } else {
#pragma unroll
      for (int i = 0; i < DT_UNROLL; ++i) {
        const unsigned uu = u + 256u * i;
        if (uu < u1) {
          const unsigned r = uu / upr;
          const int c = (int)(uu - r * upr);
          const size_t row = row0 + r;
          const float xh = (ld1(p.x, p.x_dt, row * C + c) - p.mean[row]) * p.rstd[row];
          const float g = in_lds ? sgw[c] : p.gw_w[c], bb = in_lds ? sbw[c] : p.bw_w[c];
          acc += ld1(p.dout, p.dout_dt, row * C + c) * fmaf(g, xh, bb);
        }
      }
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float s = ((red[0] + red[1]) + red[2]) + red[3];
    if (p.cps == 1) p.d_time[b] += (p.sscale ? p.sscale[b] : 1.f) * s;      // the sample's only block: no second launch
    else p.partial[blockIdx.x] = s;
  }
}

// d_time[b] += s_b · Σ_i partial[b][i], one wave per sample: lane l adds i = l, l + 64, … in order, then the shuffle tree
__global__ __launch_bounds__(64) void cln_dtime_finish_kernel(const float* __restrict__ partial, int cps, const float* __restrict__ sscale,
                                                              float* __restrict__ d_time) {
  const int b = blockIdx.x;
  float acc = 0.f;
  for (int i = threadIdx.x; i < cps; i += 64) acc += partial[(size_t)b * cps + i];
  acc = wave_sum(acc);
  if (threadIdx.x == 0) d_time[b] += (sscale ? sscale[b] : 1.f) * acc;
}

// the launch plan, a function of the three sizes alone (so that two calls add in the same order); false = not covered
static bool cln_dtime_plan(int rows, int rows_per_sample, int C, bool vec, unsigned* units, unsigned* per, int* cps) {
  if (rows <= 0 || rows_per_sample <= 0 || C <= 0 || rows % rows_per_sample) return false;
  const size_t elems = (size_t)rows_per_sample * C;
  if (elems >= ((size_t)1 << 31)) return false;
  const size_t u = vec ? elems / 8 : elems;
  const size_t total = u * (size_t)(rows / rows_per_sample);
  const size_t step = 256 * DT_UNROLL;
  size_t pb = (total + DT_BLOCKS - 1) / DT_BLOCKS;
  pb = (pb + step - 1) / step * step;
  const size_t floor_ = vec ? 2 * step : 8 * step;       // at least two (eight scalar) trips per thread: the W_g / W_b fill is amortised
  if (pb < floor_) pb = floor_;
  if (pb >= ((size_t)1 << 31)) return false;
  const size_t n = (u + pb - 1) / pb;
  if (n * (size_t)(rows / rows_per_sample) >= ((size_t)1 << 31)) return false;
  *units = (unsigned)u; *per = (unsigned)pb; *cps = (int)n;
  return true;
}

// (the workspace is sized for the 8-element-chunk plan or the element plan, whichever has more blocks: which of them a call takes
// also depends on the alignment of its pointers)
extern "C" size_t scot_cln_dtime_workspace_bytes(int rows, int rows_per_sample, int C) {
  unsigned units, per;
  int cps_s, cps_v = 0;
  if (!cln_dtime_plan(rows, rows_per_sample, C, false, &units, &per, &cps_s)) return 0;
  if (C % 8 == 0 && !cln_dtime_plan(rows, rows_per_sample, C, true, &units, &per, &cps_v)) return 0;
  return (size_t)(rows / rows_per_sample) * (size_t)(cps_s > cps_v ? cps_s : cps_v) * sizeof(float);
}

extern "C" int scot_cln_dtime(const void* dout, int dout_dt, const void* x, int x_dt, const float* mean, const float* rstd,
                              const float* gw_w, const float* bw_w, const float* sample_scale, float* d_time, int rows,
                              int rows_per_sample, int C, void* workspace, size_t ws_bytes, hipStream_t stream) {
  if (!dout || !x || !mean || !rstd || !gw_w || !bw_w || !d_time) return SCOT_ERR_UNSUPPORTED;
  if ((dout_dt != SCOT_F32 && dout_dt != SCOT_BF16) || (x_dt != SCOT_F32 && x_dt != SCOT_BF16)) return SCOT_ERR_UNSUPPORTED;
  const bool vec = C > 0 && C % 8 == 0 && ((((uintptr_t)dout) | ((uintptr_t)x)) & 15) == 0;
  ClnDtimeArgs a{};
  if (!cln_dtime_plan(rows, rows_per_sample, C, vec, &a.units, &a.per, &a.cps)) return SCOT_ERR_UNSUPPORTED;
  const int batch = rows / rows_per_sample;
  if (a.cps > 1 && (!workspace || (((uintptr_t)workspace) & 3) || ws_bytes < (size_t)batch * a.cps * sizeof(float))) return SCOT_ERR_UNSUPPORTED;
  a.dout = dout; a.x = x; a.mean = mean; a.rstd = rstd; a.gw_w = gw_w; a.bw_w = bw_w; a.sscale = sample_scale; a.d_time = d_time;
  a.partial = (float*)workspace; a.dout_dt = dout_dt; a.x_dt = x_dt; a.rows_per_sample = rows_per_sample; a.C = C;
  if (vec) hipLaunchKernelGGL(cln_dtime_partial_kernel<true>, dim3(batch * a.cps), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(cln_dtime_partial_kernel<false>, dim3(batch * a.cps), dim3(256), 0, stream, a);
  int rc = scot_check_launch();
  if (rc == SCOT_OK && a.cps > 1) {
    hipLaunchKernelGGL(cln_dtime_finish_kernel, dim3(batch), dim3(64), 0, stream, (const float*)workspace, a.cps, sample_scale, d_time);
    rc = scot_check_launch();
  }
  return rc;
}
