// One scot_gemm call as a value.  scot_gemm (gemm.hip) validates the arguments, fills a GemmCall and offers it to the four kernel
// families in turn; each of them reads what it needs from here instead of receiving the ~30 arguments again.
#pragma once
#include "common.h"

constexpr int LAYOUT_NT = 0;   // C[M,N] = A[M,K] · B[N,K]^T
constexpr int LAYOUT_NN = 1;   // C[M,N] = A[M,K] · B[K,N]
constexpr int LAYOUT_TN = 2;   // C[M,N] += A[K,M]^T · B[K,N]

// The arguments of scot_gemm (include/scot_hip.h), unchanged.
struct GemmCall {
  int layout, compute, M, N, K;
  const void* A; int a_dt, lda, a_gelu;
  const void* B; int b_dt, ldb, b_gelu;
  void* C; int c_dt, ldc;
  const float* bias; const float* colscale;
  const void* aux; int aux_dt, ldaux;
  const void* resid; int res_dt, ldres;
  int accumulate;
  float* colsum_out;
  void* workspace; size_t ws_bytes;
  int aux_mul;
  void* C2;
};

// The residual operand the NT / NN epilogues read.  `accumulate` (C += result) IS "the residual is C itself"; scot_gemm has already
// refused an NT / NN call that asks for both.  (TN accumulates by construction and its kernels read no residual.)
struct GemmResid { const void* p; int dt, ld; };
inline GemmResid gemm_resid(const GemmCall& c) {
  return c.accumulate ? GemmResid{c.C, c.c_dt, c.ldc} : GemmResid{c.resid, c.res_dt, c.ldres};
}

// all of these pointers on 16-byte boundaries (NULL counts as aligned)
template <typename... P> inline bool aligned16(const P*... p) { return ((... | (uintptr_t)p) & 15) == 0; }
// leading dimensions in whole 16-byte vectors: lda / ldb multiples of `epc` (operand elements per 16 bytes), ldc / ldaux / ldres of 8
inline bool ld_vectors(const GemmCall& c, int epc) {
  return c.lda % epc == 0 && c.ldb % epc == 0 && c.ldc % 8 == 0 && !(c.aux && c.ldaux % 8) && !(c.resid && c.ldres % 8);
}

// The candidates, in the order scot_gemm asks them (gemm.hip says why).  SCOT_ERR_UNSUPPORTED = "not mine, ask the next".
int scot_gemm_panel(const GemmCall& c, hipStream_t stream);     // gemm_panel.hip
int scot_gemm_wide(const GemmCall& c, hipStream_t stream);      // gemm_wide.hip
int scot_gemm_fast(const GemmCall& c, hipStream_t stream);      // gemm_fast.hip
int scot_gemm_generic(const GemmCall& c, hipStream_t stream);   // gemm.hip
int scot_gemm_wide_mode(int* variant);   // gemm_wide.hip: scot_gemm_wide_config's state (the grouped weight gradients' planner reads it)
extern int g_scot_use_tr;
