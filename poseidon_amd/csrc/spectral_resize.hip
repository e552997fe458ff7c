// spectral_resize — the whole spectral resize of a batch of square planes in ONE launch (reference model.py:1293-1316).
//
//     Y[b] = Pr X[b] Pr^T - Pi X[b] Pi^T          X [nimg, s, s], Pr / Pi [t, s] row-major, Y [nimg, t, t], all fp32
//
// (csrc/misc.hip derives the operator; this kernel takes ANY Pr, Pi.)  The two-launch form — an NT GEMM that writes U = X [Pr; Pi]^T to
// HBM and scot_spectral_apply, a scalar loop over it — stays as it is; this one keeps the intermediate on the chip.
//
// One workgroup (4 waves) owns 16 output rows m0 .. m0+15 of one plane, in three phases separated by barriers:
//   0. the operator rows of the tile, P = [Pr[m0..]; Pi[m0..]]  ([32][s]), go to LDS, zero beyond row t and beyond column s
//   1. W = P X[b]  ([32][s], the panel [2 TM, s]): wave w computes the 16-column tiles w, w+4, ...; A fragments from LDS, B fragments
//      straight from X (a lane reads X[k][n0 + lane&15]: 64 contiguous bytes per 16 lanes), the next fragment loaded ahead of the MFMAs
//      of the current one.  W goes to LDS with its lower half negated: W = [Wr; -Wi]
//   2. Y[b][m0.., :] = Wr Pr^T + (-Wi) Pi^T: wave w computes the 16-column tiles w, w+4, ... of the t output columns in ONE accumulator;
//      A fragments from the panel in LDS, B fragments are rows of Pr / Pi (k-contiguous: two 16-byte loads per lane when s % 4 == 0 —
//      every row is then 16-byte aligned —, scalar loads otherwise)
// Arithmetic: v_mfma_f32_16x16x4_f32 (common.h mma16(Frag<float>)): exact fp32 products, fp32 accumulation in k order.  Every output
// element is ONE chain in a fixed order inside one workgroup — no atomics, no split-K —, and a workgroup sees its own plane only: the
// bits do not depend on nimg, on the run, or on the build's 16-bit operand format.
// The contraction runs over s rounded up to 32 with zeros SUPPLIED (never loaded) beyond s, so nothing outside an extent is read.
// FLOPs 4 t s (s + t) per plane; LDS 2 * 32 * (s32 + 4) floats: 33 KB at s = 128, 66.5 KB at s = 256, 129 KB at s = 512 (< 160 KB / CU).
#include "common.h"

namespace {
constexpr int SR_TM = 16;            // output rows of a workgroup
constexpr int SR_ROWS = 2 * SR_TM;   // rows of the LDS tiles: the Pr half, then the Pi half
constexpr int SR_MAX = 512;

__host__ __device__ inline int sr_pitch(int s) { return (s + 31) / 32 * 32 + 4; }

// B fragment of phase 1: X[kk + 8g + j][n], zero beyond s either way
__device__ __forceinline__ Frag<float> sr_load_x(const float* __restrict__ Xb, int s, int kk, int n, int g) {
  Frag<float> f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = kk + 8 * g + j;
    f.v[j] = (k < s && n < s) ? Xb[(size_t)k * s + n] : 0.f;
  }
  return f;
}

// B fragment of phase 2: P[n][kk + 8g .. + 8), zero beyond row t and beyond column s
template <bool VEC> __device__ __forceinline__ Frag<float> sr_load_p(const float* __restrict__ P, int s, int t, int kk, int n, int g) {
  Frag<float> f;
  const int k0 = kk + 8 * g;
  if (VEC) {      // s % 4 == 0: a float4 lies whole inside the row or whole outside it
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (n < t) {
      const float* p = P + (size_t)n * s + k0;
      if (k0 < s) a = *(const float4*)p;
      if (k0 + 4 < s) b = *(const float4*)(p + 4);
    }
    f.v[0] = a.x; f.v[1] = a.y; f.v[2] = a.z; f.v[3] = a.w; f.v[4] = b.x; f.v[5] = b.y; f.v[6] = b.z; f.v[7] = b.w;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) f.v[j] = (n < t && k0 + j < s) ? P[(size_t)n * s + k0 + j] : 0.f;
  }
  return f;
}

template <bool VEC>
__global__ __launch_bounds__(256) void spectral_resize_kernel(const float* __restrict__ X, const float* __restrict__ Pr,
                                                              const float* __restrict__ Pi, float* __restrict__ Y, int s, int t, int mtiles) {
  extern __shared__ __attribute__((aligned(16))) float sr_lds[];      // P [32][pitch], then W [32][pitch]
  const int pitch = sr_pitch(s), s32 = pitch - 4;
  float* Pt = sr_lds;
  float* Wt = sr_lds + SR_ROWS * pitch;
  const int b = blockIdx.x / mtiles, m0 = (blockIdx.x % mtiles) * SR_TM;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const float* Xb = X + (size_t)b * s * s;
  float* Yb = Y + (size_t)b * t * t;

  // 0. the tile's operator rows
  for (int i = threadIdx.x; i < SR_ROWS * s32; i += 256) {
    const int r = i / s32, k = i - r * s32, m = m0 + (r & (SR_TM - 1));
    const float* P = r < SR_TM ? Pr : Pi;
    Pt[r * pitch + k] = (m < t && k < s) ? P[(size_t)m * s + k] : 0.f;
  }
  __syncthreads();

  // 1. W = P X
  for (int nt = wave; nt < s32 / 16; nt += 4) {
    const int n = nt * 16 + c;
    f32x4_t ar = {0.f, 0.f, 0.f, 0.f}, ai = ar;
    Frag<float> xb = sr_load_x(Xb, s, 0, n, g);
    for (int kk = 0; kk < s32; kk += 32) {
      const Frag<float> cur = xb;
      if (kk + 32 < s32) xb = sr_load_x(Xb, s, kk + 32, n, g);
      mma16(ar, lds_frag_kc(Pt, pitch, 0, kk, lane), cur);
      mma16(ai, lds_frag_kc(Pt, pitch, SR_TM, kk, lane), cur);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      Wt[(4 * g + i) * pitch + n] = ar[i];
      Wt[(SR_TM + 4 * g + i) * pitch + n] = -ai[i];
    }
  }
  __syncthreads();

  // 2. Y = Wr Pr^T + (-Wi) Pi^T
  for (int nt = wave; nt < (t + 15) / 16; nt += 4) {
    const int n = nt * 16 + c;
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    Frag<float> pr = sr_load_p<VEC>(Pr, s, t, 0, n, g), pi = sr_load_p<VEC>(Pi, s, t, 0, n, g);
    for (int kk = 0; kk < s32; kk += 32) {
      const Frag<float> cr = pr, ci = pi;
      if (kk + 32 < s32) {
        pr = sr_load_p<VEC>(Pr, s, t, kk + 32, n, g);
        pi = sr_load_p<VEC>(Pi, s, t, kk + 32, n, g);
      }
      mma16(acc, lds_frag_kc(Wt, pitch, 0, kk, lane), cr);
      mma16(acc, lds_frag_kc(Wt, pitch, SR_TM, kk, lane), ci);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + 4 * g + i;
      if (m < t && n < t) Yb[(size_t)m * t + n] = acc[i];
    }
  }
}

template <bool VEC> int sr_launch(const float* X, const float* Pr, const float* Pi, float* Y, int nimg, int s, int t, hipStream_t st) {
  const size_t sh = (size_t)2 * SR_ROWS * sr_pitch(s) * sizeof(float);
  // (more than 64 KB of dynamic LDS needs the attribute: set once per kernel, to the largest request there is)
  static const hipError_t raised = hipFuncSetAttribute((const void*)spectral_resize_kernel<VEC>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       (int)((size_t)2 * SR_ROWS * sr_pitch(SR_MAX) * sizeof(float)));
  (void)raised;
  const int mtiles = (t + SR_TM - 1) / SR_TM;
  hipLaunchKernelGGL(spectral_resize_kernel<VEC>, dim3((unsigned)((size_t)nimg * mtiles)), dim3(256), sh, st, X, Pr, Pi, Y, s, t, mtiles);
  return scot_check_launch();
}
}  // namespace

extern "C" int scot_spectral_resize(const float* X, const float* Pr, const float* Pi, float* Y, int nimg, int s, int t, hipStream_t st) {
  if (!X || !Pr || !Pi || !Y || nimg < 1 || s < 1 || t < 1 || Y == X) return SCOT_ERR_SHAPE;
  if ((((uintptr_t)X | (uintptr_t)Pr | (uintptr_t)Pi | (uintptr_t)Y) & 15) != 0) return SCOT_ERR_SHAPE;
  if (s > SR_MAX || t > SR_MAX) return SCOT_ERR_UNSUPPORTED;
  if ((size_t)nimg * ((t + SR_TM - 1) / SR_TM) > 0x7fffffffu) return SCOT_ERR_UNSUPPORTED;
  return s % 4 == 0 ? sr_launch<true>(X, Pr, Pi, Y, nimg, s, t, st) : sr_launch<false>(X, Pr, Pi, Y, nimg, s, t, st);
}
