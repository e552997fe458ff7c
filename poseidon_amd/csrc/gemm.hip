// scot_gemm — the dense contractions of the scOT hot path (52 % MLP + 19.5 % QKV + 6.5 % out-proj + ConvNeXt
// pointwise + merge/unmerge + patch embed/recovery) and their dgrad / wgrad forms.
//
//   layout NT : C[M,N] = A[M,K] · B[N,K]^T     forward of every nn.Linear (weights are [out,in]; reference
//                                              HF:545-561, HF:389-410, model.py:709,747,760)
//   layout NN : C[M,N] = A[M,K] · B[K,N]       dgrad (dX = dY · W) and the ConvTranspose2d of model.py:616-621
//   layout TN : C[M,N] += A[K,M]^T · B[K,N]    wgrad (dW = dY^T · X), split over K
//
// scot_gemm (bottom of this file) validates the arguments once, writes them into a GemmCall (gemm_call.h) and offers it to four kernel
// families, most specialised first; the first that does not answer SCOT_ERR_UNSUPPORTED has run the call:
//   1. gemm_panel  weights resident in LDS, no barriers: 16-bit NT / NN with K = 96 / 192 and M >= 4096 (stages 0 / 1), where a tiled
//                  kernel has 2-3 K-tiles per workgroup and is latency-bound.  First, because every shape it takes would also fit 3.
//   2. gemm_wide   128 x 128 tiles: 16-bit NT with M, N multiples of 128 where that grid still fills the chip (policy in gemm_wide.hip).
//                  Before 3, which takes all of these shapes at twice the L2 -> LDS bytes per flop.
//   3. gemm_fast   the production tiled kernel (64 x 64, 64 x 96, 96 x 96; table and policy in gemm_fast.hip): operands in the compute
//                  type, 16-byte aligned, leading dimensions whole vectors, no GELU on load; TN splits K through the workspace.
//   4. the kernel below: any alignment and leading dimension, mixed operand dtypes, GELU on load, column sums by a second launch
//                  (scot_colsum), TN with fp32 atomics.  What it declines is what scot_gemm answers.
// Each family keeps its own decline conditions (the panel wants an aligned bias, the wide kernel does not; only 4 converts operands);
// one that accepts a call launches it or reports the launch error: there is no other route.
//
// The kernel of this file: one workgroup = 256 threads = 4 waves (2x2) computing a BMxBN tile with 16x16 MFMA fragments, BK = 32.
// Operands are staged HBM → registers (coalesced 16-byte loads along the contiguous dimension, optional GELU,
// convert to the compute type) → LDS.  An operand whose contiguous dimension is NOT the contraction (B of NN,
// both of TN) stays in its source orientation in LDS and is read with the transposing fragment read
// (ds_read_b64_tr_b16 for bf16) — no transposed copies of activations or weights are ever written to HBM.
// Epilogue (fused): + bias[n], * colscale[n], * gelu'(aux[m,n]), + resid[m,n], store f32/bf16 or atomicAdd (TN).
#include "gemm_call.h"

struct GemmArgs {
  const void* A; const void* B; void* C;
  const float* bias; const float* colscale; const void* aux; const void* resid;
  int M, N, K;
  int lda, ldb, ldc, ldaux, ldres;
  int a_dt, b_dt, c_dt, aux_dt, res_dt;
  int a_gelu, b_gelu, aux_gelu_grad, atomic;
  int ksplit;   // K elements per blockIdx.z (multiple of 32)
  int a_vec, b_vec;  // 16-byte vector loads legal
  int use_tr;
  void* C2; int aux_mul;
};

constexpr int BK = 32;

template <typename CT, int R, bool KC> struct TileShape {
  // KC: [R][BK+kpad]  else: [BK][R+8]
  static constexpr int pitch = KC ? (BK + ct_traits<CT>::kpad) : (R + 8);
  static constexpr int elems = KC ? R * pitch : BK * pitch;
  static constexpr int nchunk = (R * (BK / 8) + 255) / 256;  // 8-element chunks per thread
};

// Load this thread's chunks of one operand tile into registers (as f32).
template <int R, bool KC>
__device__ __forceinline__ void stage_load(float (&st)[(R * 4 + 255) / 256][8], const void* src, int dt, int ld, int vec,
                                           int row0, int rmax, int k0, int kend, int tid, bool gelu) {
  constexpr int NCH = (R * 4 + 255) / 256;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = tid + i * 256;
    float* v = st[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    if (c < R * 4) {
      if (KC) {
        const int row = row0 + (c >> 2), k = k0 + (c & 3) * 8;
        if (row < rmax && k < kend) {
          const size_t idx = (size_t)row * ld + k;
          if (vec && k + 8 <= kend) ld8(src, dt, idx, v);
          else {
#pragma unroll
            for (int j = 0; j < 8; ++j) if (k + j < kend) v[j] = ld1(src, dt, idx + j);
          }
        }
      } else {
        constexpr int CPR = R / 8;  // chunks per k-row
        const int k = k0 + c / CPR, r = row0 + (c % CPR) * 8;
        if (k < kend && r < rmax) {
          const size_t idx = (size_t)k * ld + r;
          if (vec && r + 8 <= rmax) ld8(src, dt, idx, v);
          else {
#pragma unroll
            for (int j = 0; j < 8; ++j) if (r + j < rmax) v[j] = ld1(src, dt, idx + j);
          }
        }
      }
      if (gelu) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = gelu_f(v[j]);
      }
    }
  }
}

template <typename CT> __device__ __forceinline__ void lds_store8(CT* p, const float v[8]);
template <> __device__ __forceinline__ void lds_store8<float>(float* p, const float v[8]) {
  *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
  *(float4*)(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
template <> __device__ __forceinline__ void lds_store8<bf16_t>(bf16_t* p, const float v[8]) {
  *(uint4*)p = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
}

template <typename CT, int R, bool KC>
__device__ __forceinline__ void stage_store(CT* tile, const float (&st)[(R * 4 + 255) / 256][8], int tid) {
  constexpr int NCH = (R * 4 + 255) / 256;
  constexpr int pitch = TileShape<CT, R, KC>::pitch;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = tid + i * 256;
    if (c < R * 4) {
      if (KC) lds_store8<CT>(tile + (c >> 2) * pitch + (c & 3) * 8, st[i]);
      else { constexpr int CPR = R / 8; lds_store8<CT>(tile + (c / CPR) * pitch + (c % CPR) * 8, st[i]); }
    }
  }
}

template <typename CT, int BM, int BN, int LAYOUT>
__global__ __launch_bounds__(256) void gemm_kernel(GemmArgs p) {
  constexpr bool A_KC = (LAYOUT != LAYOUT_TN);
  constexpr bool B_KC = (LAYOUT == LAYOUT_NT);
  using TA = TileShape<CT, BM, A_KC>;
  using TB = TileShape<CT, BN, B_KC>;
  constexpr int MI = BM / 32, NI = BN / 32;
  __shared__ __attribute__((aligned(16))) CT lds[TA::elems + TB::elems];
  CT* As = lds;
  CT* Bs = lds + TA::elems;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int kbeg = blockIdx.z * p.ksplit;
  const int kend = min(p.K, kbeg + p.ksplit);

  f32x4_t acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  float sa[TA::nchunk][8], sb[TB::nchunk][8];
  stage_load<BM, A_KC>(sa, p.A, p.a_dt, p.lda, p.a_vec, m0, p.M, kbeg, kend, tid, p.a_gelu != 0);
  stage_load<BN, B_KC>(sb, p.B, p.b_dt, p.ldb, p.b_vec, n0, p.N, kbeg, kend, tid, p.b_gelu != 0);

  for (int k0 = kbeg; k0 < kend; k0 += BK) {
    __syncthreads();  // previous tile's fragment reads are done
    stage_store<CT, BM, A_KC>(As, sa, tid);
    stage_store<CT, BN, B_KC>(Bs, sb, tid);
    __syncthreads();
    if (k0 + BK < kend) {  // prefetch next tile into registers while the MFMAs run
      stage_load<BM, A_KC>(sa, p.A, p.a_dt, p.lda, p.a_vec, m0, p.M, k0 + BK, kend, tid, p.a_gelu != 0);
      stage_load<BN, B_KC>(sb, p.B, p.b_dt, p.ldb, p.b_vec, n0, p.N, k0 + BK, kend, tid, p.b_gelu != 0);
    }
    Frag<CT> fa[MI], fb[NI];
    const int g = lane >> 4;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int r0 = wr * (BM / 2) + i * 16;
      if (A_KC) fa[i] = lds_frag_kc(As, TA::pitch, r0, 0, lane);
      else fa[i] = lds_frag_ks(As, TA::pitch, r0, g * 8, g * 8 + 4, lane, p.use_tr);
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int c0 = wc * (BN / 2) + j * 16;
      if (B_KC) fb[j] = lds_frag_kc(Bs, TB::pitch, c0, 0, lane);
      else fb[j] = lds_frag_ks(Bs, TB::pitch, c0, g * 8, g * 8 + 4, lane, p.use_tr);
    }
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j) mma16(acc[i][j], fa[i], fb[j]);
  }

  // epilogue
  const int colbase = n0 + wc * (BN / 2) + (lane & 15);
  const int rowbase = m0 + wr * (BM / 2) + (lane >> 4) * 4;
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int col = colbase + j * 16;
    if (col >= p.N) continue;
    const float bv = (p.bias && blockIdx.z == 0) ? p.bias[col] : 0.f;
    const float cs = p.colscale ? p.colscale[col] : 1.f;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rowbase + i * 16 + r;
        if (row >= p.M) continue;
        float v = (acc[i][j][r] + bv) * cs;
        if (p.aux_gelu_grad) {
          const float x = ld1(p.aux, p.aux_dt, (size_t)row * p.ldaux + col);
          v *= p.aux_mul ? x : gelu_grad_f(x);
        }
        if (p.resid) v += ld1(p.resid, p.res_dt, (size_t)row * p.ldres + col);
        const size_t ci = (size_t)row * p.ldc + col;
        if (p.atomic) atomicAdd((float*)p.C + ci, v);
        else if (p.C2) { st1(p.C, p.c_dt, ci, gelu_f(v)); if (p.C2 != p.C) st1(p.C2, p.c_dt, ci, gelu_grad_f(v)); }
        else st1(p.C, p.c_dt, ci, v);
      }
    }
  }
}

template <typename CT, int BM, int BN>
static int launch_layout(const GemmArgs& a, int layout, int nsplit, hipStream_t s) {
  dim3 grid((a.N + BN - 1) / BN, (a.M + BM - 1) / BM, nsplit), block(256);
  switch (layout) {
    case LAYOUT_NT: hipLaunchKernelGGL((gemm_kernel<CT, BM, BN, LAYOUT_NT>), grid, block, 0, s, a); break;
    case LAYOUT_NN: hipLaunchKernelGGL((gemm_kernel<CT, BM, BN, LAYOUT_NN>), grid, block, 0, s, a); break;
    case LAYOUT_TN: hipLaunchKernelGGL((gemm_kernel<CT, BM, BN, LAYOUT_TN>), grid, block, 0, s, a); break;
    default: return SCOT_ERR_UNSUPPORTED;
  }
  return scot_check_launch();
}

extern "C" int scot_colsum(const void* x, int x_dt, const void* y, int y_dt, float* out, int M, int N, int ld, hipStream_t s);

// The last candidate: one 64 x 64 tile shape, any alignment, mixed operand dtypes, GELU on load.  Pure: SCOT_OK and the K slices, or the
// status scot_gemm answers for a call that no family takes.
int plan_generic(const GemmCall& c, GenericPlan& p) {
  if (c.C2 && c.layout == LAYOUT_TN) return SCOT_ERR_UNSUPPORTED;
  p.nsplit = 1;
  p.atomic = 0;
  p.ksplit = ((c.K + 31) / 32) * 32;
  if (c.layout == LAYOUT_TN) {
    // wgrad: tiny output, huge K (= tokens) → split K so that >= ~512 workgroups exist; fp32 atomics into C.
    if (c.c_dt != SCOT_F32) return SCOT_ERR_DTYPE;
    const long tiles = (long)((c.M + 127) / 128) * ((c.N + 95) / 96);
    long want = (768 + tiles - 1) / tiles;
    long maxsplit = (c.K + 255) / 256;
    int nsplit = (int)(want < 1 ? 1 : (want > maxsplit ? maxsplit : want));
    int per = (c.K + nsplit - 1) / nsplit;
    per = ((per + 31) / 32) * 32;
    p.ksplit = per;
    p.nsplit = (c.K + per - 1) / per;
    p.atomic = 1;
    if (!c.accumulate) return SCOT_ERR_UNSUPPORTED;  // caller zeroes C (gradient arena semantics: +=)
  }
  return SCOT_OK;
}

int scot_gemm_generic(const GemmCall& c, const GenericPlan& p, hipStream_t stream) {
  GemmArgs a;
  a.A = c.A; a.B = c.B; a.C = c.C; a.bias = c.bias; a.colscale = c.colscale; a.aux = c.aux; a.resid = c.resid;
  a.M = c.M; a.N = c.N; a.K = c.K; a.lda = c.lda; a.ldb = c.ldb; a.ldc = c.ldc; a.ldaux = c.ldaux; a.ldres = c.ldres;
  a.a_dt = c.a_dt; a.b_dt = c.b_dt; a.c_dt = c.c_dt; a.aux_dt = c.aux_dt; a.res_dt = c.res_dt;
  a.a_gelu = c.a_gelu; a.b_gelu = c.b_gelu; a.aux_gelu_grad = c.aux != nullptr; a.use_tr = g_scot_use_tr;
  a.C2 = c.C2; a.aux_mul = c.aux_mul;
  a.a_vec = aligned16(c.A) && c.lda % 8 == 0;
  a.b_vec = aligned16(c.B) && c.ldb % 8 == 0;
  a.atomic = p.atomic;
  a.ksplit = p.ksplit;
  if (c.layout != LAYOUT_TN) {
    const GemmResid r = gemm_resid(c);
    a.resid = r.p; a.res_dt = r.dt; a.ldres = r.ld;
  }
  int rc = c.compute == SCOT_BF16 ? launch_layout<bf16_t, 64, 64>(a, c.layout, p.nsplit, stream) : launch_layout<float, 64, 64>(a, c.layout, p.nsplit, stream);
  if (rc == SCOT_OK && c.colsum_out) {   // this kernel has no column sums of its own: a second launch
    if (c.layout == LAYOUT_TN) rc = scot_colsum(c.A, c.a_dt, nullptr, 0, c.colsum_out, c.K, c.M, c.lda, stream);  // Σ_k A[k][m]
    else rc = scot_colsum(c.C, c.c_dt, nullptr, 0, c.colsum_out, c.M, c.N, c.ldc, stream);
  }
  return rc;
}

// The arguments of scot_gemm as a GemmCall, validated: SCOT_OK, or the status the call gets before any family is asked.
#define SCOT_GEMM_PARAMS                                                                                                        \
  int layout, int compute, int M, int N, int K, const void *A, int a_dt, int lda, int a_gelu, const void *B, int b_dt, int ldb, \
      int b_gelu, void *C, int c_dt, int ldc, const float *bias, const float *colscale, const void *aux, int aux_dt, int ldaux,  \
      const void *resid, int res_dt, int ldres, int accumulate, float *colsum_out, void *workspace, size_t ws_bytes, int aux_mul, \
      void *C2
#define SCOT_GEMM_ARGS                                                                                                            \
  layout, compute, M, N, K, A, a_dt, lda, a_gelu, B, b_dt, ldb, b_gelu, C, c_dt, ldc, bias, colscale, aux, aux_dt, ldaux, resid, \
      res_dt, ldres, accumulate, colsum_out, workspace, ws_bytes, aux_mul, C2
static int gemm_call(SCOT_GEMM_PARAMS, GemmCall& c) {
  if (M <= 0 || N <= 0 || K <= 0) return SCOT_ERR_SHAPE;
  if (layout < 0 || layout > 2 || compute < 0 || compute > SCOT_BF16X3) return SCOT_ERR_UNSUPPORTED;
  if ((a_dt | b_dt | c_dt) & ~1) return SCOT_ERR_DTYPE;
  if (compute == SCOT_BF16X3 && (a_dt != SCOT_F32 || b_dt != SCOT_F32)) return SCOT_ERR_DTYPE;   // bf16x3 splits fp32 operands
  // C += result is "the residual is C" in every NT / NN kernel (gemm_resid), so a call that names a residual as well has no kernel
  if (layout != LAYOUT_TN && accumulate && resid != nullptr) return SCOT_ERR_UNSUPPORTED;
  c = GemmCall{SCOT_GEMM_ARGS};
  return SCOT_OK;
}

// Which family runs a call, and its plan: the first of the four whose planner accepts.  `family` < 0: the status scot_gemm answers.
struct GemmPlan { int family; PanelPlan panel; WidePlan wide; FastPlan fast; GenericPlan generic; };
static GemmPlan plan_gemm(const GemmCall& c) {
  GemmPlan g = {};
  if (plan_panel(c, g.panel)) g.family = SCOT_ROUTE_PANEL;
  else if (plan_wide(c, g.wide)) g.family = SCOT_ROUTE_WIDE;
  else if (plan_fast_call(c, g.fast)) g.family = SCOT_ROUTE_FAST;
  else { const int rc = plan_generic(c, g.generic); g.family = rc == SCOT_OK ? SCOT_ROUTE_GENERIC : rc; }
  return g;
}

extern "C" int scot_gemm(SCOT_GEMM_PARAMS, hipStream_t stream) {
  GemmCall c;
  const int rc = gemm_call(SCOT_GEMM_ARGS, c);
  if (rc != SCOT_OK) return rc;
  const GemmPlan g = plan_gemm(c);
  switch (g.family) {
    case SCOT_ROUTE_PANEL: return scot_gemm_panel(c, g.panel, stream);
    case SCOT_ROUTE_WIDE: return scot_gemm_wide(c, g.wide, stream);
    case SCOT_ROUTE_FAST: return scot_gemm_fast(c, g.fast, stream);
    case SCOT_ROUTE_GENERIC: return scot_gemm_generic(c, g.generic, stream);
    default: return g.family;
  }
}

// include/scot_hip.h: scot_gemm_route — plan_gemm's answer for the same arguments; nothing is launched, no pointer is read.
extern "C" int scot_gemm_route(SCOT_GEMM_PARAMS, int* route) {
  if (!route) return SCOT_ERR_SHAPE;
  for (int i = 0; i < SCOT_ROUTE_INTS; ++i) route[i] = 0;
  GemmCall c;
  const int rc = gemm_call(SCOT_GEMM_ARGS, c);
  if (rc != SCOT_OK) { route[0] = rc; return SCOT_OK; }
  const GemmPlan g = plan_gemm(c);
  route[0] = g.family;
  route[5] = 1;
  switch (g.family) {
    case SCOT_ROUTE_PANEL:      // a wave walks 32-row groups against a resident panel of nf 16-column fragments, 96 K elements per chunk
      route[1] = g.panel.nf; route[2] = 32; route[3] = 16 * g.panel.nf; route[4] = 96; route[6] = COMMIT_EPILOGUE; break;
    case SCOT_ROUTE_WIDE:
      route[1] = g.wide.variant; route[2] = 128; route[3] = 128; route[4] = 64; route[6] = COMMIT_EPILOGUE; route[7] = g.wide.epi; break;
    case SCOT_ROUTE_FAST:
      fast_tile_of(g.fast, &route[1], &route[2], &route[3], &route[4]);
      route[5] = g.fast.nsplit; route[6] = g.fast.commit; route[8] = g.fast.zl; break;
    case SCOT_ROUTE_GENERIC:    // row: 0 = the 16-bit MFMA instantiation, 1 = the fp32 one (fp32 and bf16x3 compute)
      route[1] = c.compute == SCOT_BF16 ? 0 : 1; route[2] = 64; route[3] = 64; route[4] = BK;
      route[5] = g.generic.nsplit; route[6] = g.generic.atomic ? COMMIT_ATOMIC : COMMIT_EPILOGUE; break;
    default: break;
  }
  return SCOT_OK;
}

// include/scot_hip.h: scot_route_table — the rows a route can name, so that a test can hold every one of them to a case
extern "C" int scot_route_table(int table, int row, int* route) {
  if (!route) return SCOT_ERR_SHAPE;
  for (int i = 0; i < SCOT_ROUTE_INTS; ++i) route[i] = 0;
  bool ok = false;
  switch (table) {
    case 0: ok = fast_table_row(row, route); break;
    case 1: ok = tail_table_row(row, route); break;
    case 2: ok = row >= 0 && row < 3; break;      // gemm_wide.hip's instantiations (WIDE_V_*), also the grouped 128 x 128 kernel's
    case 3: ok = row >= 0 && row < 4; break;      // the grouped weight-gradient kernels (GROUP_*)
    default: break;
  }
  route[0] = ok ? 1 : 0;
  return SCOT_OK;
}
