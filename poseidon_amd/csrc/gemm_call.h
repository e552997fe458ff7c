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

// The candidates, in the order plan_gemm (gemm.hip) asks them.  Every family has a pure planner — shapes, dtypes, flags, which operands are
// present and how their pointers are aligned; no pointer is read, nothing is launched — and a launcher that takes the plan.  A planner that
// declines says "not mine, ask the next"; scot_gemm_route reports the same plan the launch would run.
struct PanelPlan { int nf; };                      // 16-column fragments per resident panel: 3 (48 columns) or 6 (96)
struct WidePlan { int variant, epi; };             // WIDE_V_* instantiation, WIDE_EPI_* epilogue class
struct FastTile;
// How a workgroup's accumulator tile meets C — EPILOGUE: NT / NN unsplit, the fused epilogue stores it; OWNER: TN unsplit, C += acc by the
// tile's only owner; WORKSPACE: TN split, partial tiles + one reduce pass with zl lanes per 8 results; ATOMIC: split without a usable
// workspace (TN) or by scot_gemm_splitk_config (NT), and every TN product of the generic kernel: fp32 atomics into C.
enum { COMMIT_EPILOGUE, COMMIT_OWNER, COMMIT_WORKSPACE, COMMIT_ATOMIC };
struct FastPlan {
  const FastTile* tile;
  int nsplit, ksplit, commit, zl;   // K slices; K elements per slice
  size_t ws_used;                   // bytes of workspace the launch writes
};
struct GenericPlan { int nsplit, ksplit, atomic; };   // K slices (TN only), K elements per slice, fp32 atomics into C
bool plan_panel(const GemmCall& c, PanelPlan& p);       // gemm_panel.hip
bool plan_wide(const GemmCall& c, WidePlan& p);         // gemm_wide.hip
bool plan_fast_call(const GemmCall& c, FastPlan& p);    // gemm_fast.hip: plan_fast with the call's own workspace and alignment
int plan_generic(const GemmCall& c, GenericPlan& p);    // gemm.hip: SCOT_OK, or what scot_gemm answers for a call nobody takes
void fast_tile_of(const FastPlan& p, int* row, int* bm, int* bn, int* bk);   // gemm_fast.hip: the plan's row of kFastTiles
bool fast_table_row(int row, int* route);   // gemm_fast.hip / mlp_fused.hip: one row of kFastTiles / kTailShapes for scot_route_table
bool tail_table_row(int row, int* route);
int scot_gemm_panel(const GemmCall& c, const PanelPlan& p, hipStream_t stream);
int scot_gemm_wide(const GemmCall& c, const WidePlan& p, hipStream_t stream);
int scot_gemm_fast(const GemmCall& c, const FastPlan& p, hipStream_t stream);
int scot_gemm_generic(const GemmCall& c, const GenericPlan& p, hipStream_t stream);
int scot_gemm_wide_mode(int* variant);   // gemm_wide.hip: scot_gemm_wide_config's state (the grouped weight gradients' planner reads it)
extern int g_scot_use_tr;
