"""One guarded case per kernel ROUTE: which kernel a call reaches is asked, not assumed.

`scot_gemm`, `scot_wgrad_group` and the fused layer tails choose their kernel from shapes, dtypes, epilogue operands, pointer alignment and
policy thresholds.  tests/route_census.py lists the route KEY of every call the engine issues for the presets (on the CPU, nothing
launched); ROUTE_CASES below holds, for every such key and for every row of the kernels' tables that only the C ABI reaches, the SMALLEST
call that takes it — the route's threshold shape, never the workload's — ragged in M and N where the route allows it.  Every case

  * asserts that `scot_*_route` on its OWN guarded arguments (real library, real alignment) answers the key it declares;
  * runs inside guard bands, strided (pad 8) and dense, and applies the four checks of tests/test_kernels_guarded_gpu.py: bands intact,
    results finite, `gemm_excess <= 1` against the fp64 product of the operands as the MFMA sees them (the epilogue's addends and factors
    enter `mag` / `nadd` / `abs_extra` as gemm_epilogues_guarded derives them: no stored tolerance), bit-equality with the unguarded
    launch where the route is deterministic (TN products and colsum_out keep the tolerance of test_kernels_gpu.py).

The fused-tail and grouped weight-gradient keys reuse block_tail_*_guarded / fused_halves_*_guarded / wgrad_group_guarded with the key's
shape.  tests/test_kernel_routes_cpu.py holds the closure test (census keys are a subset of these keys), runs the small cases on the
emulated kernels and asserts that no table row is without a case."""
import math
from typing import NamedTuple

import pytest
import torch

import kernel_checks as kc
import route_census as RC
import test_kernels_gpu as G
import test_kernels_guarded_gpu as GG
from poseidon_amd import ops

F32 = torch.float32
NT, NN, TN = ops.NT, ops.NN, ops.TN
F32C, BF16, X3 = ops.F32, ops.BF16, ops.X3
PANEL, WIDE, FAST, GENERIC = ops.ROUTE_PANEL, ops.ROUTE_WIDE, ops.ROUTE_FAST, ops.ROUTE_GENERIC
(T_64x64, T_64x64_GLDS, T_64x64_BK32, T_64x64_DEEP, T_64x96, T_96x96, T_F32_64x64, T_X3_64x64, T_X3_64x96, T_X3_96x96) = range(10)      # kFastTiles
GROUP_64x64, GROUP_64x64_KG2, GROUP_96x96, GROUP_WIDE = range(4)
EMU_MAX_MACS = 16 << 20      # cases up to this many multiply-adds (and below the panel's 4096 rows) also run on the emulated kernels


def gk(layout, compute, family, row, dts, commit=0, split=0, zl=None, wide_epi=0, bias=0, colscale=0, aux=0, resid=0, accumulate=0, C2=0,
       colsum_out=0, a_gelu=0, b_gelu=0):
    """a scot_gemm route key (tests/route_census.py).  dts: the dtypes of A, B, C and, where present, aux and resid in that order, "f" = fp32,
    "h" = the 16-bit operand format; aux: 1 = gelu'(aux), 2 = aux as is; C2: 1 = gelu / gelu' dual store, 2 = C2 == C."""
    t = [int(c == "h") for c in dts]
    extra = t[3:]
    aux_dt = extra.pop(0) if aux else 0
    res_dt = extra.pop(0) if resid else 0
    assert not extra, dts
    zl = (1 if family == FAST else 0) if zl is None else zl
    return ("scot_gemm", layout, compute, family, row, commit, split, zl, wide_epi, t[0], t[1], t[2], bias, colscale, aux, aux_dt, resid, res_dt,
            accumulate, C2, colsum_out, a_gelu, b_gelu)


def tail_key(entry, C, HC, TT, qkv=0, pro=0, recomp=0):
    return (entry, 0, C, HC, TT, qkv, pro, recomp)


def wg_key(kernel, split, zl, variant=-1):
    return ("scot_wgrad_group", 0, kernel, variant, split, zl)


# (key, M, N, K): the smallest ragged call that takes the key, found by sweeping scot_gemm_route over shapes with the key's operands
# (M >= 130 or, for TN, 136: three 64-row tiles, the last ragged; N >= 72; K >= 72 and past the route's own threshold; the panel from its
# 4096 rows on, the 128 x 128 tiles by policy from 129 tiles on and, with one workgroup per CU, at 128 tiles).  "table row": a row of
# kFastTiles x layout that no preset reaches but the C ABI does.
GEMM_ROUTES = [
    (gk(NT, X3, FAST, T_X3_64x96, "fff", bias=1), 130, 96, 72),
    (gk(NT, BF16, PANEL, 6, "hhh", bias=1), 4100, 192, 192),
    (gk(NT, X3, FAST, T_X3_64x64, "fff"), 130, 72, 72),
    (gk(NT, BF16, WIDE, 2, "hhh", bias=1), 16512, 256, 384),
    (gk(NT, BF16, FAST, T_64x64_GLDS, "hhf", bias=1), 130, 72, 192),
    (gk(NT, BF16, WIDE, 2, "hhh", bias=1, C2=1), 16512, 256, 384),
    (gk(NT, BF16, FAST, T_64x64_GLDS, "hhh", bias=1), 130, 72, 192),
    (gk(NT, BF16, FAST, T_64x64_GLDS, "hhh", bias=1, C2=1), 130, 72, 192),
    (gk(NT, BF16, PANEL, 6, "hhh", bias=1, C2=1), 4100, 192, 192),
    (gk(NT, BF16, FAST, T_64x96, "hhf", bias=1), 130, 96, 72),
    (gk(NT, X3, FAST, T_X3_64x96, "fff"), 130, 96, 72),
    (gk(NN, X3, FAST, T_X3_64x64, "fff"), 130, 72, 72),
    (gk(TN, X3, FAST, T_X3_64x64, "fff", commit=2, split=1, accumulate=1, zl=32), 136, 72, 16384),
    (gk(NT, BF16, FAST, T_64x96, "hhf", accumulate=1), 130, 96, 72),
    (gk(NN, X3, FAST, T_X3_64x96, "fff"), 130, 96, 72),
    (gk(NT, BF16, FAST, T_64x64_GLDS, "hhf", accumulate=1), 130, 72, 192),
    (gk(TN, X3, FAST, T_X3_96x96, "fff", commit=2, split=1, accumulate=1, zl=32), 192, 96, 16384),
    (gk(NT, BF16, WIDE, 1, "hhhh", wide_epi=1, aux=2), 16512, 256, 384),
    (gk(NT, BF16, FAST, T_64x64_GLDS, "hhh"), 130, 72, 192),
    (gk(TN, X3, FAST, T_X3_64x64, "fff", commit=2, split=1, accumulate=1, zl=4), 136, 72, 1024),
    (gk(NT, BF16, WIDE, 0, "hhhh", wide_epi=1, aux=2), 1024, 2048, 384),
    (gk(TN, X3, FAST, T_X3_64x64, "fff", commit=2, split=1, accumulate=1), 136, 72, 264),
    (gk(NT, BF16, PANEL, 6, "hhhh", aux=2), 4100, 192, 192),
    (gk(NT, BF16, FAST, T_64x96, "hhh"), 130, 96, 72),
    (gk(TN, X3, FAST, T_X3_64x64, "fff", commit=2, split=1, accumulate=1, colsum_out=1, zl=32), 136, 72, 16384),
    (gk(NT, X3, FAST, T_X3_64x64, "fff", bias=1), 130, 72, 72),
    (gk(NT, BF16, FAST, T_64x64_BK32, "hhh", bias=1), 130, 72, 72),
    (gk(NT, BF16, FAST, T_64x64_BK32, "hhh", bias=1, C2=1), 130, 72, 72),
    (gk(NT, BF16, PANEL, 3, "hhf", bias=1), 4100, 144, 192),
    (gk(NT, BF16, FAST, T_64x64_BK32, "hhhh", aux=2), 130, 72, 72),
    (gk(NT, BF16, PANEL, 3, "hhf", accumulate=1), 4100, 144, 192),
    (gk(NT, BF16, FAST, T_64x64_BK32, "hhh"), 130, 72, 72),
    (gk(NT, BF16, FAST, T_64x64, "hhf", accumulate=1), 130, 72, 136),
    (gk(TN, X3, FAST, T_X3_96x96, "fff", commit=2, split=1, accumulate=1, zl=8), 192, 96, 8192),
    (gk(NT, BF16, FAST, T_64x64_GLDS, "hhhh", aux=2), 130, 72, 192),
    (gk(NT, BF16, PANEL, 3, "hhh"), 4100, 144, 192),
    (gk(NT, BF16, WIDE, 2, "hhf", bias=1), 16512, 256, 384),
    (gk(NT, BF16, WIDE, 0, "hhf", bias=1), 1024, 2048, 3072),
    (gk(NT, BF16, WIDE, 1, "hhf", wide_epi=2, accumulate=1), 16512, 256, 384),
    (gk(NT, BF16, WIDE, 2, "hhh"), 16512, 256, 384),
    (gk(TN, X3, FAST, T_X3_96x96, "fff", commit=2, split=1, accumulate=1, zl=4), 288, 1152, 8192),
    (gk(NT, BF16, WIDE, 0, "hhf", wide_epi=2, accumulate=1), 1024, 2048, 3072),
    (gk(TN, X3, FAST, T_X3_64x64, "fff", commit=1, accumulate=1), 136, 72, 72),
    (gk(NT, F32C, FAST, T_F32_64x64, "fff", bias=1), 130, 72, 72),
    (gk(NT, F32C, FAST, T_F32_64x64, "fff"), 130, 72, 72),
    (gk(NN, F32C, FAST, T_F32_64x64, "fff"), 130, 72, 72),
    (gk(TN, F32C, FAST, T_F32_64x64, "fff", commit=2, split=1, accumulate=1, zl=8), 136, 72, 4096),
    (gk(TN, F32C, FAST, T_F32_64x64, "fff", commit=2, split=1, accumulate=1, zl=4), 136, 72, 1024),
    (gk(TN, F32C, FAST, T_F32_64x64, "fff", commit=2, split=1, accumulate=1), 136, 72, 264),
    (gk(TN, F32C, FAST, T_F32_64x64, "fff", commit=1, accumulate=1), 136, 72, 72),
    (gk(TN, F32C, FAST, T_F32_64x64, "fff", commit=2, split=1, accumulate=1, colsum_out=1, zl=8), 136, 72, 4096),
    (gk(NT, F32C, FAST, T_F32_64x64, "fff", bias=1, C2=1), 130, 72, 72),
    (gk(NN, F32C, FAST, T_F32_64x64, "ffff", aux=2), 130, 72, 72),
    (gk(NN, F32C, FAST, T_F32_64x64, "fff", accumulate=1), 130, 72, 72),
    (gk(TN, F32C, FAST, T_F32_64x64, "fff", commit=2, split=1, accumulate=1, colsum_out=1, zl=4), 136, 72, 1024),
    (gk(TN, F32C, FAST, T_F32_64x64, "fff", commit=2, split=1, accumulate=1, colsum_out=1), 136, 72, 264),
    (gk(TN, F32C, FAST, T_F32_64x64, "fff", commit=1, accumulate=1, colsum_out=1), 136, 72, 72),
    (gk(NT, X3, FAST, T_X3_64x64, "fff", bias=1, C2=1), 130, 72, 72),
    (gk(NN, X3, FAST, T_X3_64x64, "ffff", aux=2), 130, 72, 72),
    (gk(NN, X3, FAST, T_X3_64x96, "fff", accumulate=1), 130, 96, 72),
    (gk(TN, X3, FAST, T_X3_96x96, "fff", commit=2, split=1, accumulate=1, colsum_out=1, zl=8), 192, 96, 8192),
    (gk(NN, X3, FAST, T_X3_64x64, "fff", accumulate=1), 130, 72, 72),
    (gk(TN, X3, FAST, T_X3_64x64, "fff", commit=2, split=1, accumulate=1, colsum_out=1, zl=4), 136, 72, 1024),
    (gk(TN, X3, FAST, T_X3_64x64, "fff", commit=2, split=1, accumulate=1, colsum_out=1), 136, 72, 264),
    (gk(TN, X3, FAST, T_X3_64x64, "fff", commit=1, accumulate=1, colsum_out=1), 136, 72, 72),
    (gk(NN, BF16, FAST, T_64x64, "hhh", bias=1), 130, 72, 136),      # table row
    (gk(TN, BF16, FAST, T_64x64, "hhf", commit=2, split=1, accumulate=1, colsum_out=1, zl=4), 136, 72, 2048),      # table row
    (gk(NN, BF16, FAST, T_64x64_BK32, "hhhh", aux=1), 130, 72, 72),      # table row
    (gk(NT, BF16, FAST, T_64x64_DEEP, "hhh", bias=1, C2=1), 130, 72, 2312),      # table row
    (gk(NT, BF16, FAST, T_64x64_DEEP, "hhf", accumulate=1), 130, 72, 2312),      # table row
    (gk(NN, BF16, FAST, T_64x64_DEEP, "hhhh", aux=2), 130, 72, 2304),      # table row
    (gk(NN, BF16, FAST, T_64x96, "hhff", bias=1, resid=1), 130, 96, 72),      # table row
    (gk(TN, BF16, FAST, T_64x96, "hhf", commit=2, split=1, accumulate=1, zl=4), 136, 96, 2048),      # table row
    (gk(TN, BF16, FAST, T_96x96, "hhf", commit=2, split=1, accumulate=1, colsum_out=1, zl=8), 192, 96, 8192),      # table row
    (gk(TN, X3, FAST, T_X3_64x96, "fff", commit=2, split=1, accumulate=1, zl=4), 136, 96, 1024),      # table row
]


class Case(NamedTuple):
    keys: tuple      # the route keys the case's launches take (the two fused halves: one per entry point)
    body: str        # which guarded body runs it
    args: tuple
    emu: bool        # small enough for the emulated kernels


def _gemm_case(key, M, N, K):
    d = dict(zip(RC.GEMM_KEY_FIELDS, key[1:]))
    kind = "f16" if d["compute"] == BF16 else "bf16"      # the engine's default build for 16-bit operands; fp32 / split operands: either
    return Case((key,), "gemm", (kind, key, M, N, K), M < 4096 and M * N * K <= EMU_MAX_MACS)


_FWD, _BWD = "scot_block_tail_fwd", "scot_block_tail_bwd"
_HALVES_FWD, _HALVES_BWD = ("scot_proj_cln_fwd", "scot_mlp_block_fwd"), ("scot_proj_cln_bwd", "scot_mlp_block_bwd")
ROUTE_CASES = [_gemm_case(*c) for c in GEMM_ROUTES] + [
    # fused layer tails (kind, C, B, L, ...): 64-row workgroups at three ragged samples, 128-row ones (TT = 2) from 65536 rows of C = 96 on
    Case((tail_key(_FWD, 48, 192, 1, qkv=1),), "tail_fwd", ("f16", 48, 3, 200, True, True, True, False), True),
    Case((tail_key(_FWD, 48, 192, 1),), "tail_fwd", ("f16", 48, 3, 200, True, True, False, False), True),
    Case((tail_key(_FWD, 96, 64, 1, qkv=1),), "tail_fwd", ("f16", 96, 3, 200, True, True, True, True), True),
    Case((tail_key(_FWD, 96, 64, 1),), "tail_fwd", ("f16", 96, 3, 200, True, True, False, True), True),
    Case((tail_key(_FWD, 192, 64, 1, qkv=1),), "tail_fwd", ("f16", 192, 3, 72, True, True, True, True), True),
    Case((tail_key(_FWD, 192, 64, 1),), "tail_fwd", ("f16", 192, 3, 72, True, True, False, True), True),
    Case((tail_key(_FWD, 96, 64, 2, qkv=1),), "tail_fwd", ("f16", 96, 64, 1024, True, True, True, True), False),
    Case((tail_key(_FWD, 96, 64, 2),), "tail_fwd", ("f16", 96, 64, 1024, True, True, False, True), False),
    Case((tail_key(_BWD, 96, 64, 1),), "tail_bwd", ("f16", 96, 3, 192, True, "stored"), True),
    Case((tail_key(_BWD, 96, 64, 1, pro=1),), "tail_bwd", ("f16", 96, 3, 192, True, "prologue"), True),
    Case((tail_key(_BWD, 192, 64, 1),), "tail_bwd", ("f16", 192, 3, 64, True, "stored"), True),
    Case((tail_key(_BWD, 96, 64, 2),), "tail_bwd", ("f16", 96, 64, 1024, True, "stored"), False),
    Case((tail_key(_BWD, 96, 64, 2, pro=1),), "tail_bwd", ("f16", 96, 64, 1024, True, "prologue"), False),
    # ... rows and template forms of the tails' table that the presets do not reach
    Case((tail_key(_BWD, 48, 192, 1),), "tail_bwd", ("f16", 48, 3, 192, True, "stored"), True),
    Case((tail_key(_BWD, 96, 64, 1, recomp=1),), "tail_bwd", ("f16", 96, 3, 192, True, "lean"), True),
    Case((tail_key(_BWD, 192, 64, 1, recomp=1),), "tail_bwd", ("f16", 192, 3, 64, True, "lean"), True),
    Case((tail_key(_BWD, 192, 64, 1, pro=1),), "tail_bwd", ("f16", 192, 3, 64, True, "prologue"), True),
    Case(tuple(tail_key(e, 96, 64, 1) for e in _HALVES_FWD), "halves_fwd", (96, 3, 200, True, True), True),
    Case(tuple(tail_key(e, 192, 64, 1) for e in _HALVES_FWD), "halves_fwd", (192, 3, 72, True, True), True),
    Case(tuple(tail_key(e, 96, 64, 2) for e in _HALVES_FWD), "halves_fwd", (96, 64, 1024, True, True), False),
    Case(tuple(tail_key(e, 96, 64, 1) for e in _HALVES_BWD), "halves_bwd", (96, 3, 192, True), True),
    Case(tuple(tail_key(e, 192, 64, 1) for e in _HALVES_BWD), "halves_bwd", (192, 3, 64, True), True),
    Case(tuple(tail_key(e, 96, 64, 2) for e in _HALVES_BWD), "halves_bwd", (96, 64, 1024, True), False),
    # grouped weight gradients (kind, K, dims [(M_i, N_i)], forced, scaled): the kernel, whether K is split and the lanes of the reduce pass
    # follow from the tile count and K — 64 x 64: 12 / 6 tiles; two K groups: unsplit from 4 K-tiles; 96 x 96: whole 96-tiles over >= 8192
    # tokens; 128 x 128: 256 tiles unsplit, 64 tiles over 8192 tokens split
    Case((wg_key(GROUP_64x64, 1, 1),), "wgroup", ("f16", 1024, ((72, 136), (136, 72)), -1, False), True),
    Case((wg_key(GROUP_64x64, 1, 4),), "wgroup", ("f16", 2048, ((72, 136), (136, 72)), -1, True), False),
    Case((wg_key(GROUP_64x64, 1, 8),), "wgroup", ("f16", 16384, ((48, 192), (192, 48)), -1, True), False),
    Case((wg_key(GROUP_64x64_KG2, 0, 1),), "wgroup", ("f16", 256, ((72, 136), (136, 72)), -1, True), True),
    Case((wg_key(GROUP_96x96, 1, 4),), "wgroup", ("f16", 8192, ((96, 96), (288, 96)), -1, False), False),
    Case((wg_key(GROUP_96x96, 1, 8),), "wgroup", ("f16", 16384, ((96, 96), (288, 96)), -1, True), False),
    Case((wg_key(GROUP_WIDE, 0, 1, variant=1),), "wgroup", ("f16", 128, ((1024, 2048), (2048, 1024)), -1, True), False),
    Case((wg_key(GROUP_WIDE, 1, 4, variant=1),), "wgroup", ("f16", 8192, ((512, 1024), (1024, 512)), -1, False), False),
]
CASE_IDS = [f"{i}-{c.body}-" + ("x".join(str(a) for a in c.args[2:]) if c.body == "gemm" else "-".join(str(a) for a in c.args if not isinstance(a, tuple)))
            for i, c in enumerate(ROUTE_CASES)]

# rows of the kernels' tables that no call can select in this process, with the reason (tests/test_kernel_routes_cpu.py holds each as a
# strict expected failure)
UNREACHABLE_ROWS = {
    ("scot_mlp_block_fwd", 192, 64, 2): "C = 192 with 128-row workgroups (256 VGPRs + spills) is selected by the SCOT_MLP_TT=2 override only, which the library reads once per process",
    ("scot_mlp_block_bwd", 192, 64, 2): "C = 192 with 128-row workgroups (256 VGPRs + spills) is selected by the SCOT_MLP_TT=2 override only, which the library reads once per process",
}


# ------------------------------------------------------------------------------------------------------------------ the GEMM body
def _call_key(layout, compute, M, N, K, A, lda, B, ldb, C, ldc, bias=None, colscale=None, aux=None, ldaux=0, resid=None, ldres=0, a_gelu=False,
              b_gelu=False, accumulate=False, colsum_out=None, aux_mul=False, gelu_deriv_out=None):
    """the route key of ops.gemm(...) with these arguments, from the library the launch would go to"""
    args = ops._gemm_args(layout, compute, M, N, K, A, lda, B, ldb, C, ldc, bias, colscale, aux, ldaux, resid, ldres, a_gelu, b_gelu, accumulate,
                          colsum_out, aux_mul, gelu_deriv_out)
    return RC.key_of(ops._raw(), "scot_gemm", args + (None,))


def gemm_route_guarded(kind, key, M, N, K, dry=False):
    """One scot_gemm call built from the flags of `key`, at M x N x K, under the library's default policy (as the engine's calls).  dry:
    only build the arguments (torch.empty) and assert the route, launch nothing."""
    d = dict(zip(RC.GEMM_KEY_FIELDS, key[1:]))
    lay, compute, tn = d["layout"], d["compute"], d["layout"] == TN
    if d["colscale"] and tn or d["colsum_out"] and not tn or (d["a_gelu"] or d["b_gelu"]) and compute == X3:
        raise NotImplementedError(f"no reference for this form yet: {RC.describe_key(key)}")
    prev = ops.use(kind)
    try:
        hd = ops.half_dtype()
        DT = (F32, hd)
        ua = kc.U32 if compute == F32C else GG.U_MFMA16
        u_op = kc.UNIT[hd] if compute == BF16 else 0.0
        make = (lambda *s, dtype=F32, **kw: torch.empty(*s, dtype=dtype, device=G.DEV)) if dry else G.rnd
        A = make(*((K, M) if tn else (M, K)), dtype=DT[d["a_dt"]])
        B = make(*((N, K) if lay == NT else (K, N)), dtype=DT[d["b_dt"]], scale=K ** -0.5, seed=1)
        bias = make(N, seed=2) if d["bias"] else None
        cs = make(N, seed=5) if d["colscale"] else None
        aux = make(M, N, dtype=DT[d["aux_dt"]], seed=8) if d["aux"] else None
        res = make(M, N, dtype=DT[d["res_dt"]], seed=6) if d["resid"] else None
        C0 = make(M, N, dtype=DT[d["c_dt"]], seed=9) if d["accumulate"] else None
        ncs = M if tn else N
        cdt = DT[d["c_dt"]]

        def launch(pad, guarded):
            """-> (C, C2, colsum, guards) of one launch; the route is asserted on these very arguments first"""
            gd = GG.Guards()
            op = (lambda t, p, name: gd.op(t, p, name)) if guarded else (lambda t, p, name: t)
            out = (lambda shape, dt_, p, src, name: gd.out(shape, dt_, p, src=src, name=name)) if guarded else \
                  (lambda shape, dt_, p, src, name: src.clone() if src is not None else GG.nan_like(shape, dt_))
            Ag, Bg = op(A, pad, "A"), op(B, pad, "B")
            Cg = out((M, N), cdt, pad, C0, "C")
            C2g = None if not d["C2"] else (Cg if d["C2"] == 2 else out((M, N), cdt, pad, None, "C2"))
            csum = None
            if d["colsum_out"]:
                csum = gd.out((ncs,), F32, fill=0.0, name="colsum_out") if guarded else torch.zeros(ncs, device=G.DEV)
            kw = dict(bias=op(bias, 0, "bias"), colscale=op(cs, 0, "colscale"), aux=op(aux, pad, "aux"), ldaux=N + pad if d["aux"] else 0,
                      resid=op(res, pad, "resid"), ldres=N + pad if d["resid"] else 0, a_gelu=bool(d["a_gelu"]), b_gelu=bool(d["b_gelu"]),
                      accumulate=bool(d["accumulate"]), colsum_out=csum, aux_mul=d["aux"] == 2, gelu_deriv_out=C2g)
            pos = (lay, compute, M, N, K, Ag, A.shape[1] + pad, Bg, B.shape[1] + pad, Cg, N + pad)
            got = _call_key(*pos, **kw)
            assert got == key, f"the case no longer takes its route (pad {pad}, guarded {guarded}):\n  declared {RC.describe_key(key)}\n  takes    {RC.describe_key(got)}"
            if not dry:
                ops.gemm(*pos, **kw)
            return Cg, C2g, csum, gd

        if dry:
            for pad in (8, 0):
                launch(pad, True)
            return
        # ---- the fp64 reference on the operands as the MFMA sees them (gemm_layouts_guarded / gemm_epilogues_guarded)
        mm = (lambda X, Y: X @ Y.t()) if lay == NT else (lambda X, Y: X @ Y) if lay == NN else (lambda X, Y: X.t() @ Y)

        def operand(X, gelu):      # (value, magnitude, deviation of what the MFMA sees from the value) — GELU on load is evaluated in fp32
            if not gelu:
                x = (X.to(hd) if compute == BF16 else X).double()
                return x, x.abs(), None
            x64 = X.double()
            e, g = GG.gelu_operand_err(x64, u_op), GG._gelu64(x64)
            return g, g.abs() + e, e
        Ae, Aabs, EA = operand(A, d["a_gelu"])
        Be, Babs, EB = operand(B, d["b_gelu"])
        v, mag = mm(Ae, Be), mm(Aabs, Babs)
        ae = torch.zeros_like(v)
        if EA is not None:
            ae = ae + mm(EA, Babs)
        if EB is not None:
            ae = ae + mm(Ae.abs(), EB)
        # fp32 roundings on an element's path: K products; TN: + the partial sums of the K slices (each at least 32 deep) + the add into C;
        # bf16x3: three products per term and the split's operand error (~2^-17 per product) as a multiple of the same |A| |B| term
        nadd = K + (K // 32 + 2 if tn else 0)
        if compute == X3:
            nadd = 3 * K + K // 32 + 2 + math.ceil(3 * 2.0 ** -17 / GG.U_MFMA16)
        if d["bias"]:
            v, mag, nadd = v + bias.double(), mag + bias.double().abs(), nadd + 1
        if d["colscale"]:
            v, mag, ae, nadd = v * cs.double(), mag * cs.double().abs(), ae * cs.double().abs(), nadd + 1
        if d["aux"] == 2:
            v, mag, ae, nadd = v * aux.double(), mag * aux.double().abs(), ae * aux.double().abs(), nadd + 1
        elif d["aux"] == 1:      # the factor gelu'(aux) carries its evaluation error (aux is a stored operand: no error of its own)
            gg = GG._gelu_grad64(aux.double())
            ae = ae * gg.abs() + (v.abs() + nadd * ua * mag + ae) * GG.gelu_eval_err(aux.double())[1]
            v, mag, nadd = v * gg, mag * gg.abs(), nadd + 1
        addend = res if d["resid"] else C0
        if addend is not None:
            v, mag = v + addend.double(), mag + addend.double().abs()
            nadd += 0 if tn else 1
        what = f"{RC.describe_key(key)} at {M}x{N}x{K}"
        Cp, C2p, csp, _ = launch(0, False)
        for pad in (8, 0):
            Cg, C2g, csg, gd = launch(pad, True)
            GG.sync()
            gd.check()
            assert GG.finite(Cg) and (C2g is None or GG.finite(C2g)) and (csg is None or GG.finite(csg))
            if d["C2"]:      # gelu(v) and gelu'(v) of the fp32 value v: gemm_epilogues_guarded's dual store
                dv = nadd * ua * mag + ae
                ev_g, ev_gp = GG.gelu_eval_err(v)
                zero = torch.zeros_like(v)
                GG.assert_excess(f"{what} pad {pad} gelu(v)", Cg, GG._gelu64(v), zero, 0, ua, abs_extra=GG.LIP_GELU * dv + ev_g + GG.D_CDF * dv)
                if d["C2"] == 1:
                    GG.assert_excess(f"{what} pad {pad} gelu'(v)", C2g, GG._gelu_grad64(v), zero, 0, ua, abs_extra=GG.LIP_GELU_GRAD * dv + ev_gp)
                    assert GG.same(C2g, C2p), kc.describe_worst(C2g, C2p.double())
            else:
                GG.assert_excess(f"{what} pad {pad}", Cg, v, mag, nadd, ua, abs_extra=ae)
            if tn:      # split K, partial tiles or one owner; colsum_out by atomics: the tolerances of test_gemm_layouts
                tol = 2e-3 if compute == BF16 else 2e-5
                assert G.rel(Cg, v) < tol and G.rel(Cg, Cp) < 2e-6
                if csg is not None:
                    assert G.rel(csg, A.double().sum(0)) < 1e-4
            else:
                assert GG.same(Cg, Cp), kc.describe_worst(Cg, Cp.double())
    finally:
        ops.use(prev)


# -------------------------------------------------------------------------------------------------------- routes of the reused bodies
def shape_keys(case, lib):
    """the route keys of a fused-tail / grouped weight-gradient case from its shapes alone (aligned operands, a workspace of the size the
    library asks for): what the CPU suite compares with the declared keys"""
    import ctypes
    route = (ctypes.c_int * 12)()
    if case.body == "wgroup":
        kind, K, dims, forced, scaled = case.args
        n = len(dims)
        VP, IA = ctypes.c_void_p * n, ctypes.c_int * n
        p = VP(*[0x10000] * n)
        Ms, Ns = IA(*[m for m, _ in dims]), IA(*[nn for _, nn in dims])
        need = int(lib.scot_wgrad_group_workspace_bytes(n, K, Ms, Ns))
        args = (BF16, n, K, p, p, p, p, Ms, Ns, 0x10000, max(need, 8 << 20), None, None, None)
        return {RC.key_of(lib, "scot_wgrad_group", args)}
    if case.body in ("tail_fwd", "tail_bwd"):
        kind, C, B, L = case.args[:4]
        if case.body == "tail_fwd":
            q = (ops.TAIL_FWD, C, B * L, L, 4 * C, int(case.args[6]), 0, 0)
        else:
            q = (ops.TAIL_BWD, C, B * L, L, 4 * C, 0, int(case.args[5] == "prologue"), int(case.args[5] == "lean"))
        assert lib.scot_block_tail_route(*q, route) == 0
        return {(_FWD if case.body == "tail_fwd" else _BWD, route[0], route[1], route[2], route[3], route[5], route[6], route[7])}
    C, B, L = case.args[:3]
    out = set()
    for entry, fam, hid in zip(_HALVES_FWD if case.body == "halves_fwd" else _HALVES_BWD,
                               (ops.TAIL_PROJ_FWD, ops.TAIL_MLP_FWD) if case.body == "halves_fwd" else (ops.TAIL_PROJ_BWD, ops.TAIL_MLP_BWD), (-1, 4 * C)):
        assert lib.scot_block_tail_route(fam, C, B * L, L, hid, 0, 0, 0, route) == 0
        out.add((entry, route[0], route[1], route[2], route[3], route[5], route[6], route[7]))
    return out


def run_case(case, dry=False):
    """run one case's guarded body; the launches of the reused bodies are recorded (ops.set_recorder, as the step tape does) and every
    routed one must have taken a key the case declares"""
    if case.body == "gemm":
        return gemm_route_guarded(*case.args, dry=dry)
    body = {"tail_fwd": GG.block_tail_fwd_guarded, "tail_bwd": GG.block_tail_bwd_guarded, "halves_fwd": GG.fused_halves_fwd_guarded,
            "halves_bwd": GG.fused_halves_bwd_guarded, "wgroup": GG.wgrad_group_guarded}[case.body]
    args = case.args
    if case.body == "wgroup":
        args = (args[0], args[1], list(args[2]), args[3], args[4])
    log = []
    prev_kind = ops.use("f16") if case.body.startswith("halves") else None      # (the two halves' bodies run in the active build)
    prev = ops.set_recorder(log)
    try:
        body(*args)
    finally:
        ops.set_recorder(prev)
        if prev_kind is not None:
            ops.use(prev_kind)
    took = {RC.key_of(ops._raw(), fn.__name__, a) for fn, a in log if fn.__name__ in RC.ROUTED}
    assert took == set(case.keys), "the case no longer takes its route:\n  declared " + "; ".join(RC.describe_key(k) for k in case.keys) + \
        "\n  took     " + "; ".join(RC.describe_key(k) for k in sorted(took, key=str))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ROUTE_CASES, ids=CASE_IDS)
def test_route_case(case):
    run_case(case)


# ---------------------------------------------------------------------------------------------- the census against a recorded step
@pytest.mark.gpu
def test_recorded_step_takes_the_census_keys(monkeypatch):
    """One real training step of Poseidon-T (fp16, batch 32) recorded the way the step tape records it, against the dry census of the same
    configuration run here against the real library: the two key sets are equal.  Pins the proxy (what it answers, which entry points it
    forwards) and the alignment the dry run's CPU buffers stand in for."""
    from poseidon_amd import lib as scot_lib
    from poseidon_amd.synth import synth_inputs
    import test_model_gpu as TM
    tag, size, channels, batch, compute, igr = RC.CONFIGS[1]
    assert (tag, compute) == ("T", "fp16")
    monkeypatch.setenv("SCOT_TAPE", "0")      # the engine's own tape would replay instead of calling: every launch goes through the wrappers
    model = TM._preset_model(tag, size, channels, compute)[2]
    pv, t, lab = synth_inputs(batch, channels, channels, size, "smooth")
    pv, t, lab = pv.cuda(), t.cuda(), lab.cuda()
    model(pixel_values=pv, time=t, labels=lab).loss.backward()      # first use: workspace growth, lazy plans
    model.zero_grad()
    log = []
    prev = ops.set_recorder(log)
    try:
        model(pixel_values=pv, time=t, labels=lab).loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.set_recorder(prev)
    real = scot_lib.load()
    recorded = RC.keys_of([(fn.__name__, args, "recorded step") for fn, args in log], lib=real)
    with pytest.MonkeyPatch.context() as mp:
        dry = RC.keys_of(RC.census(mp, tag, size, channels, batch, compute, igr, load=lambda kind: scot_lib.load(kind=kind)), lib=real)
    only_real = [RC.describe_key(k) for k in recorded if k not in dry]
    only_dry = [RC.describe_key(k) + " | " + RC.describe_call(*dry[k]) for k in dry if k not in recorded]
    assert not only_real and not only_dry, "recorded step only:\n  " + "\n  ".join(only_real) + "\ndry census only:\n  " + "\n  ".join(only_dry)
