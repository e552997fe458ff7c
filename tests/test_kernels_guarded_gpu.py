"""The hot-path kernels inside poisoned guard bands, judged per element (tests/kernel_checks.py).

Every operand and every result of a case is a view inside a larger allocation whose surroundings hold NaN of one fixed bit pattern
(`kernel_checks.guarded`); the kernel is launched once on those views and once on plain tensors with the same contents.  Then
  (a) every band, row gap and padding is intact bit for bit            — no store outside the extent the call was given;
  (b) every result is finite                                          — no load outside it reached an MFMA or a sum (0 * NaN = NaN);
  (c) the LOCAL bound of the family holds: `gemm_excess <= 1` for products (no stored tolerance: the componentwise bound of an
      fp32-accumulated inner product plus one rounding), a per-row comparison against a rounding model for attention and the conditional
      layer norm, an exact or single-rounding compare for data movement;
  (d) the result is BIT-IDENTICAL to the plain launch wherever the entry point is deterministic — an answer that depends on what lies
      beside the operands is wrong even when both answers are within tolerance.  Results the header documents as order-dependent (fp32
      atomics: TN products, K slices, colsum_out, bias gradients, attention's dbias_table / dlogit_scale, the norms' parameter gradients)
      take the tolerance of their existing test in test_kernels_gpu.py instead.
References, shape lists and tolerances come from test_kernels_gpu (imported as G; G.DEV is read at call time, so the CPU emulation's patch
of that name reaches every allocation here).  The bodies take their shapes as arguments: tests/test_kernels_emu_cpu.py calls them with
small ragged shapes on the emulated kernels."""
import math

import pytest
import torch

import kernel_checks as kc
import test_kernels_gpu as G
from poseidon_amd import ops

pytestmark = pytest.mark.gpu

F32 = torch.float32
U_MFMA16 = 2.0 ** -23      # per-add roundoff assumed for the 16-bit MFMAs' internal sum (see kernel_checks.gemm_excess)
NAN = float("nan")


class Guards:
    """The guarded tensors of one case."""

    def __init__(self):
        self.items = []

    def op(self, t, pad=0, name="operand"):
        """guarded copy of an operand; pad > 0: row stride = row width + pad"""
        if t is None:
            return None
        v, g = kc.guarded(tuple(t.shape), t.dtype, G.DEV, src=t, ld=(t.shape[-1] + pad) if pad else None, name=name)
        self.items.append(g)
        return v

    def out(self, shape, dtype, pad=0, src=None, fill=None, name="result"):
        """guarded result: NaN body unless the op accumulates (src / fill)"""
        v, g = kc.guarded(tuple(shape), dtype, G.DEV, src=src, fill=fill, ld=(shape[-1] + pad) if pad else None, name=name)
        self.items.append(g)
        return v

    def group(self, shapes, dtype, srcs=None, fills=None, name="group"):
        vs, g = kc.guarded_group(shapes, dtype, G.DEV, srcs=srcs, fills=fills, name=name)
        self.items.append(g)
        return vs

    def check(self):
        kc.check_all(self.items)


def sync():
    torch.cuda.synchronize()


def nan_like(shape, dtype):
    return torch.full(tuple(shape), NAN, device=G.DEV, dtype=dtype)


def finite(t):
    """(b): True, or an AssertionError that says how much of the result is not finite and where"""
    bad = ~torch.isfinite(t.float() if t.dtype != torch.float64 else t)
    if bool(bad.any()):
        idx = bad.nonzero()
        rows = bad.reshape(-1, bad.shape[-1]).any(-1).nonzero().flatten()
        raise AssertionError(f"non-finite result (an over-read reached an MFMA or a sum?): {int(bad.sum())} of {bad.numel()} element(s) of a {tuple(t.shape)} "
                             f"tensor, first at {idx[0].tolist()}, last at {idx[-1].tolist()}; {rows.numel()} row(s) affected, first {int(rows[0])}, last {int(rows[-1])}")
    return True


def same(a, b):
    """bit-identical (torch.equal treats NaN as unequal: a NaN result fails here as well)"""
    return a.shape == b.shape and torch.equal(a.contiguous(), b.contiguous())


def u_add(compute):
    return kc.U32 if compute == ops.F32 else U_MFMA16


def assert_excess(what, got, ref, mag, nadd, uadd, extra=0.0, tile=None, abs_extra=None):
    """(c) for products.  `mag` is the magnitude sum of everything that enters an element in fp32 before the single rounding — |A| |B| plus
    the absolute values of the epilogue's addends, times the absolute values of its factors — and `nadd` the number of fp32 roundings on
    that path: K for the contraction, one more per epilogue operation.  Every one of them is at most u * (a partial magnitude) <= u * mag."""
    worst, idx = kc.gemm_excess(got, ref, mag, nadd, kc.UNIT[got.dtype], extra=extra, u_add=uadd, abs_extra=abs_extra)
    print(f"worst excess {what}: {worst:.3f} at {idx}")
    assert worst <= 1.0, f"{what}: element {idx} is {worst:.2f} x its bound; {kc.describe_worst(got, ref, tile=tile)}"
    return worst


# =========================================================================================================================== GEMM
def _operands(layout, compute, mixed, M, N, K):
    adt = F32 if compute in (ops.F32, ops.X3) else ops.half_dtype()
    bdt = F32 if mixed else adt
    if layout == ops.NT:
        return G.rnd(M, K, dtype=adt), G.rnd(N, K, dtype=bdt, scale=K ** -0.5, seed=1)
    if layout == ops.NN:
        return G.rnd(M, K, dtype=adt), G.rnd(K, N, dtype=bdt, scale=K ** -0.5, seed=1)
    return G.rnd(K, M, dtype=adt), G.rnd(K, N, dtype=bdt, scale=K ** -0.5, seed=1)


def _product64(layout, compute, A, B):
    """fp64 product and |A| |B| on the operands as the MFMA sees them (a fp32 B beside a 16-bit A is rounded while it is staged)"""
    Aq = A.double()
    Bq = (B.to(ops.half_dtype()) if compute == ops.BF16 else B).double()
    if layout == ops.NT:
        return Aq @ Bq.t(), Aq.abs() @ Bq.abs().t()
    if layout == ops.NN:
        return Aq @ Bq, Aq.abs() @ Bq.abs()
    return Aq.t() @ Bq, Aq.abs().t() @ Bq.abs()


class _gemm_config:
    """library-wide tile / K-slice policy for one case, restored afterwards"""

    def __init__(self, wide=None, splitk=(-1, 0)):
        self.wide, self.splitk = wide, splitk

    def __enter__(self):
        lib = ops.L()
        if self.wide is not None:
            lib.scot_gemm_wide_config(*self.wide)
        lib.scot_gemm_splitk_config(*self.splitk)
        return lib

    def __exit__(self, *exc):
        lib = ops.L()
        lib.scot_gemm_wide_config(1, 0)
        lib.scot_gemm_splitk_config(0, 1)


GEMM_PADS = [(c, 0) for c in G.GEMM_CASES] + [(c, 8) for c in G.GEMM_CASES] + \
            [(c, 3) for c in G.GEMM_CASES if c[3:] in ((257, 130, 72), (520, 64, 40))]       # 3: rows off every vector alignment (scalar loaders)


@pytest.mark.parametrize("case,pad", GEMM_PADS, ids=lambda v: "-".join(str(int(x)) for x in v) if isinstance(v, tuple) else f"pad{v}")
def test_gemm_layouts_guarded(case, pad):
    gemm_layouts_guarded(*case, pad)


def gemm_layouts_guarded(compute, layout, mixed, M, N, K, pad):
    """scot_gemm NT / NN / TN, operands in the compute type (gemm_fast; gemm_panel for the bias + residual call of the 4096-row NT / NN
    shapes only: the calls in front of it pass colsum_out, which the panel and the 128 x 128 tiles decline) and fp32 B beside 16-bit A (the
    generic kernel), fp32 and 16-bit results, with `lda / ldb / ldc / ldres` = width + pad.  K slices with atomics are off here (their own
    test below), so NT / NN are deterministic; TN (split K, atomics or partial tiles) and colsum_out are order-dependent.  Which kernel a
    shape reaches is asked, not assumed, in tests/test_kernel_routes_gpu.py: one case per route and epilogue form."""
    A, B = _operands(layout, compute, mixed, M, N, K)
    ref, ab = _product64(layout, compute, A, B)
    tn = layout == ops.TN
    ua = u_add(compute)
    with _gemm_config():
        gd = Guards()
        Ag, Bg = gd.op(A, pad, "A"), gd.op(B, pad, "B")
        lda, ldb = A.shape[1] + pad, B.shape[1] + pad
        tol = 2e-5 if compute == ops.F32 else 2e-3
        for cdt in ([F32] if tn or compute != ops.BF16 else [F32, ops.half_dtype()]):
            C0 = G.rnd(M, N, seed=9) if tn else None
            Cg = gd.out((M, N), cdt, pad, src=C0, name="C")
            Cp = C0.clone() if tn else nan_like((M, N), cdt)
            ncs = M if tn else N
            csg, csp = gd.out((ncs,), F32, fill=0.0, name="colsum_out"), torch.zeros(ncs, device=G.DEV)
            ops.gemm(layout, compute, M, N, K, Ag, lda, Bg, ldb, Cg, N + pad, accumulate=tn, colsum_out=csg)
            ops.gemm(layout, compute, M, N, K, A, A.shape[1], B, B.shape[1], Cp, N, accumulate=tn, colsum_out=csp)
            sync()
            gd.check()
            assert finite(Cg) and finite(csg)
            if tn:      # C0 + sum of K products, in slices: at most K + (number of slices) + 1 additions, a slice is at least 32 deep
                assert_excess(f"gemm TN {M}x{N}x{K} compute {compute}", Cg, C0.double() + ref, ab + C0.double().abs(), K + K // 32 + 2, ua)
                assert G.rel(Cg, C0.double() + ref) < tol and G.rel(Cg, Cp) < 2e-6
                assert G.rel(csg, A.double().sum(0)) < 1e-4
            else:
                assert_excess(f"gemm layout {layout} {M}x{N}x{K} compute {compute} mixed {mixed} -> {cdt}", Cg, ref, ab, K, ua)
                assert same(Cg, Cp), kc.describe_worst(Cg, Cp.double())
                # fp32 C: sums of the stored result.  16-bit C (include/scot_hip.h): the tiled kernels (csrc/gemm_fast.hip: operands in the
                # compute type, N, K and the leading dimensions multiples of 8) sum the fp32 values BEFORE the store rounds them, the generic
                # kernel (csrc/gemm.hip: everything else) sums what it stored
                tiled = not mixed and pad % 8 == 0 and N % 8 == 0 and K % 8 == 0 and (layout == ops.NT or N >= 8)
                assert G.rel(csg, ref.sum(0) if (cdt != F32 and tiled) else Cg.double().sum(0)) < 1e-4
        if not tn:      # bias + residual (strided too), no column sums: small grids take the split-K + epilogue-pass route
            bias, res = G.rnd(N, seed=5), G.rnd(M, N, seed=6)
            bg, rg = gd.op(bias, name="bias"), gd.op(res, pad, "resid")
            C2g, C2p = gd.out((M, N), F32, pad, name="C (bias + resid)"), nan_like((M, N), F32)
            ops.gemm(layout, compute, M, N, K, Ag, lda, Bg, ldb, C2g, N + pad, bias=bg, resid=rg, ldres=N + pad)
            ops.gemm(layout, compute, M, N, K, A, A.shape[1], B, B.shape[1], C2p, N, bias=bias, resid=res, ldres=N)
            sync()
            gd.check()
            assert finite(C2g)
            assert_excess(f"gemm layout {layout} {M}x{N}x{K} compute {compute} mixed {mixed} + bias + resid", C2g, ref + bias.double() + res.double(),
                          ab + bias.double().abs() + res.double().abs(), K + 2, ua)
            assert same(C2g, C2p), kc.describe_worst(C2g, C2p.double())


def _gelu64(u):
    return torch.nn.functional.gelu(u)


def _gelu_grad64(u):
    return 0.5 * (1 + torch.erf(u / math.sqrt(2))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)


# The library's GELU (csrc/common.h, gelu_terms): Phi(x) = 0.5 + sign(x) (0.5 - poly(t) e), t = rcp(1 + p z), e = exp2(-z^2 log2 e), z = |x| / sqrt 2,
# Abramowitz-Stegun 7.1.26, for which the source states |abs err of erf| <= 1.5e-7, i.e. 0.75e-7 on Phi.  On top of that its evaluation in fp32:
# every quantity of the chain lies in [0, 1]; v_rcp_f32 and v_exp_f32 are 1-ulp instructions, the argument of the exponential carries two
# roundings and x e^-x <= 0.37, the five Horner steps, the two fused multiply-adds and the final add one rounding each on values <= 1 — twelve
# roundings of at most 2^-24 in all, taken at full size.  The Gaussian term e alone: its instruction, and its argument's two roundings: 4 x 2^-24.
D_CDF = 0.75e-7 + 12 * kc.U32
D_EXP = 4 * kc.U32
INV_SQRT_2PI = 0.3989422804014327


def gelu_eval_err(v64):
    """absolute error of the library's gelu(v) and gelu'(v) evaluated in fp32 AT the fp32 value v: (|v| dPhi + one product rounding,
    dPhi + |v| c dE + two product roundings and an add)"""
    g, gp = _gelu64(v64), _gelu_grad64(v64)
    gauss = v64.abs() * INV_SQRT_2PI * torch.exp(-0.5 * v64 * v64)
    return v64.abs() * D_CDF + kc.U32 * g.abs(), D_CDF + v64.abs() * INV_SQRT_2PI * D_EXP + 2 * kc.U32 * gauss + kc.U32 * gp.abs()


# |gelu'| <= 1.13 and |gelu''| = |(2 - x^2) phi(x)| <= 2 phi(0) < 0.8: how an error dv of the epilogue's fp32 value v moves gelu(v) and gelu'(v)
LIP_GELU, LIP_GELU_GRAD = 1.13, 0.8


def gelu_operand_err(u64, u_op):
    """elementwise bound on |operand the MFMA sees - gelu64(u)| when gelu(u) is evaluated on load and rounded to an operand format of unit
    roundoff u_op (0 for fp32 operands): the evaluation error, then one rounding of a value within that error of gelu64(u)"""
    ev, _ = gelu_eval_err(u64)
    return ev + u_op * (_gelu64(u64).abs() + ev)


@pytest.mark.parametrize("pad", [0, 8, 16])
@pytest.mark.parametrize("compute", [ops.F32, ops.BF16])
def test_gemm_epilogues_guarded(compute, pad):
    gemm_epilogues_guarded(compute, 520, 192, 96, pad)


def gemm_epilogues_guarded(compute, M, N, K, pad):
    """The epilogue forms of test_gemm_epilogues with every operand guarded and strided: bias -> 16-bit u; GELU-on-load + bias + colscale +
    residual; gelu' multiply from aux; aux_mul; accumulate; TN with GELU on the B operand + colsum_out; the gelu / gelu' dual store.
    (c): gemm_excess on every form.  Where the epilogue evaluates erf / exp (GELU on load, gelu', the dual store) the bound takes the
    library's own statement on its erf approximation (csrc/common.h: |abs err| <= 1.5e-7) plus its fp32 evaluation (D_CDF, D_EXP above) as
    an absolute term: gelu / gelu' move by at most 1.13 / 0.8 times the error of the fp32 value they are taken of, plus their own
    evaluation error; an operand that is gelu(u) evaluated on load differs from gelu64(u) by gelu_operand_err, which enters as E |B|."""
    cdt = F32 if compute == ops.F32 else ops.half_dtype()
    tol = 2e-5 if compute == ops.F32 else 1e-2
    ua = u_add(compute)
    u_op = 0.0 if compute == ops.F32 else kc.UNIT[cdt]
    x, w, b = G.rnd(M, K, dtype=cdt), G.rnd(N, K, dtype=cdt, scale=0.1, seed=1), G.rnd(N, seed=2)
    with _gemm_config():
        gd = Guards()
        xg, wg, bg = gd.op(x, pad, "x"), gd.op(w, pad, "w"), gd.op(b, name="bias")
        # fc1: u = x w^T + b in the compute type
        ug, up = gd.out((M, N), cdt, pad, name="u"), nan_like((M, N), cdt)
        ops.gemm(ops.NT, compute, M, N, K, xg, K + pad, wg, K + pad, ug, N + pad, bias=bg)
        ops.gemm(ops.NT, compute, M, N, K, x, K, w, K, up, N, bias=b)
        sync()
        gd.check()
        ref_u = x.double() @ w.double().t() + b.double()
        assert finite(ug) and same(ug, up)
        assert_excess(f"epilogue bias compute {compute}", ug, ref_u, x.double().abs() @ w.double().abs().t() + b.double().abs(), K + 1, ua)
        # fc2 with GELU on load: y = (gelu(u) w2^T + b2) * cs + res
        w2, b2, cs, res = G.rnd(K, N, dtype=cdt, scale=0.1, seed=3), G.rnd(K, seed=4), G.rnd(K, seed=5), G.rnd(M, K, seed=6)
        w2g, b2g, csg, resg = gd.op(w2, pad, "w2"), gd.op(b2, name="b2"), gd.op(cs, name="colscale"), gd.op(res, pad, "resid")
        yg, yp = gd.out((M, K), F32, pad, name="y"), nan_like((M, K), F32)
        ops.gemm(ops.NT, compute, M, K, N, ug, N + pad, w2g, N + pad, yg, K + pad, bias=b2g, colscale=csg, resid=resg, ldres=K + pad, a_gelu=True)
        ops.gemm(ops.NT, compute, M, K, N, up, N, w2, N, yp, K, bias=b2, colscale=cs, resid=res, ldres=K, a_gelu=True)
        sync()
        gd.check()
        g64 = _gelu64(up.double())
        assert finite(yg) and same(yg, yp)
        assert G.rel(yg, (g64 @ w2.double().t() + b2.double()) * cs.double() + res.double()) < tol
        e_a = gelu_operand_err(up.double(), u_op)            # the A operand as the MFMA sees it against gelu64 of the stored u
        assert_excess(f"epilogue GELU on load, bias * colscale + resid compute {compute}", yg, (g64 @ w2.double().t() + b2.double()) * cs.double() + res.double(),
                      ((g64.abs() + e_a) @ w2.double().abs().t() + b2.double().abs()) * cs.double().abs() + res.double().abs(), N + 3, ua,
                      abs_extra=(e_a @ w2.double().abs().t()) * cs.double().abs())
        # the rational part of the same epilogue without GELU on load: per element
        y2g, y2p = gd.out((M, K), F32, pad, name="y2"), nan_like((M, K), F32)
        ops.gemm(ops.NT, compute, M, K, N, ug, N + pad, w2g, N + pad, y2g, K + pad, bias=b2g, colscale=csg, resid=resg, ldres=K + pad)
        ops.gemm(ops.NT, compute, M, K, N, up, N, w2, N, y2p, K, bias=b2, colscale=cs, resid=res, ldres=K)
        sync()
        gd.check()
        u64 = up.double()
        assert finite(y2g) and same(y2g, y2p)
        assert_excess(f"epilogue bias * colscale + resid compute {compute}", y2g, (u64 @ w2.double().t() + b2.double()) * cs.double() + res.double(),
                      (u64.abs() @ w2.double().abs().t() + b2.double().abs()) * cs.double().abs() + res.double().abs(), N + 3, ua)
        # dgrad (NN): du = (dy w2) * gelu'(u); * aux as is; accumulate
        dy = G.rnd(M, K, dtype=cdt, seed=7)
        dyg = gd.op(dy, pad, "dy")
        dug, dup = gd.out((M, N), cdt, pad, name="du"), nan_like((M, N), cdt)
        ops.gemm(ops.NN, compute, M, N, K, dyg, K + pad, w2g, N + pad, dug, N + pad, aux=ug, ldaux=N + pad)
        ops.gemm(ops.NN, compute, M, N, K, dy, K, w2, N, dup, N, aux=up, ldaux=N)
        sync()
        gd.check()
        prod, aprod = dy.double() @ w2.double(), dy.double().abs() @ w2.double().abs()
        assert finite(dug) and same(dug, dup) and G.rel(dug, prod * _gelu_grad64(u64)) < tol
        # v = acc * gelu'(aux): the factor carries its evaluation error (aux is a stored operand: no error of its own), then one product rounding
        assert_excess(f"epilogue * gelu'(aux) compute {compute}", dug, prod * _gelu_grad64(u64), aprod * _gelu_grad64(u64).abs(), K + 1, ua,
                      abs_extra=(prod.abs() + K * ua * aprod) * gelu_eval_err(u64)[1])
        aux = G.rnd(M, N, dtype=cdt, seed=8)
        auxg = gd.op(aux, pad, "aux")
        dmg, dmp = gd.out((M, N), cdt, pad, name="du (aux_mul)"), nan_like((M, N), cdt)
        ops.gemm(ops.NN, compute, M, N, K, dyg, K + pad, w2g, N + pad, dmg, N + pad, aux=auxg, ldaux=N + pad, aux_mul=True)
        ops.gemm(ops.NN, compute, M, N, K, dy, K, w2, N, dmp, N, aux=aux, ldaux=N, aux_mul=True)
        sync()
        gd.check()
        assert finite(dmg) and same(dmg, dmp)
        assert_excess(f"epilogue aux_mul compute {compute}", dmg, prod * aux.double(), aprod * aux.double().abs(), K + 1, ua)
        acc0 = G.rnd(M, N, seed=9)
        ag, ap = gd.out((M, N), F32, pad, src=acc0, name="accumulated"), acc0.clone()
        ops.gemm(ops.NN, compute, M, N, K, dyg, K + pad, w2g, N + pad, ag, N + pad, accumulate=True)
        ops.gemm(ops.NN, compute, M, N, K, dy, K, w2, N, ap, N, accumulate=True)
        sync()
        gd.check()
        assert finite(ag) and same(ag, ap)
        assert_excess(f"epilogue accumulate compute {compute}", ag, acc0.double() + prod, aprod + acc0.double().abs(), K + 1, ua)
        # wgrad (TN) with GELU on the B operand + bias gradient
        dw0, db0 = G.rnd(K, N, seed=10), G.rnd(K, seed=11)
        dwg, dbg = gd.out((K, N), F32, pad, src=dw0, name="dw"), gd.out((K,), F32, src=db0, name="dbias")
        ops.gemm(ops.TN, compute, K, N, M, dyg, K + pad, ug, N + pad, dwg, N + pad, b_gelu=True, accumulate=True, colsum_out=dbg)
        sync()
        gd.check()
        assert finite(dwg) and G.rel(dwg - dw0, dy.double().t() @ g64) < tol and G.rel(dbg - db0, dy.double().sum(0)) < 1e-4
        assert_excess(f"epilogue TN with GELU on the B operand compute {compute}", dwg, dw0.double() + dy.double().t() @ g64,
                      dy.double().abs().t() @ (g64.abs() + e_a) + dw0.double().abs(), M + M // 32 + 2, ua, abs_extra=dy.double().abs().t() @ e_a)
        # the fc1 form: gelu(v) and gelu'(v) from one pass
        a_g, gp_g = gd.out((M, N), cdt, pad, name="gelu(u)"), gd.out((M, N), cdt, pad, name="gelu'(u)")
        a_p, gp_p = nan_like((M, N), cdt), nan_like((M, N), cdt)
        ops.gemm(ops.NT, compute, M, N, K, xg, K + pad, wg, K + pad, a_g, N + pad, bias=bg, gelu_deriv_out=gp_g)
        ops.gemm(ops.NT, compute, M, N, K, x, K, w, K, a_p, N, bias=b, gelu_deriv_out=gp_p)
        sync()
        gd.check()
        assert finite(a_g) and finite(gp_g) and same(a_g, a_p) and same(gp_g, gp_p)
        assert G.rel(a_g, _gelu64(ref_u)) < tol and G.rel(gp_g, _gelu_grad64(ref_u)) < tol
        dv = (K + 1) * ua * (x.double().abs() @ w.double().abs().t() + b.double().abs())       # error of the fp32 value v the two are taken of
        ev_g, ev_gp = gelu_eval_err(ref_u)
        zero = torch.zeros_like(ref_u)
        assert_excess(f"epilogue gelu(v) of the dual store compute {compute}", a_g, _gelu64(ref_u), zero, 0, ua, abs_extra=LIP_GELU * dv + ev_g + D_CDF * dv)
        assert_excess(f"epilogue gelu'(v) of the dual store compute {compute}", gp_g, _gelu_grad64(ref_u), zero, 0, ua, abs_extra=LIP_GELU_GRAD * dv + ev_gp)


WIDE_GUARDED = G.WIDE_CASES + [(384, 256, 192, 0), (384, 256, 192, 1), (384, 256, 192, 2)]      # + three tile rows / two tile columns per variant


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("M,N,K,variant", WIDE_GUARDED)
def test_gemm_wide_tiles_guarded(kind, M, N, K, variant, pad):
    gemm_wide_tiles_guarded(kind, M, N, K, variant, pad)


def gemm_wide_tiles_guarded(kind, M, N, K, variant, pad):
    """csrc/gemm_wide.hip (128 x 128 tiles; the three instantiations forced as test_gemm_wide_tiles does, -1 = the library's policy): the
    engine's forms — bias to fp32 and to 16 bits, the gelu / gelu' dual store, the data gradient times aux, the accumulating data gradient —
    guarded and strided.  16-bit results are where one global norm is blind: here every element is held to its own bound."""
    prev = ops.use(kind)
    try:
        hd = ops.half_dtype()
        tol16 = 1.2e-3 if kind == "f16" else 6e-3
        x, w, b = G.rnd(M, K, dtype=hd), G.rnd(N, K, dtype=hd, scale=K ** -0.5, seed=1), G.rnd(N, seed=2)
        u = x.double() @ w.double().t() + b.double()
        mag = x.double().abs() @ w.double().abs().t() + b.double().abs()
        with _gemm_config(wide=(1 if variant < 0 else 2, max(variant, 0))):
            gd = Guards()
            xg, wg, bg = gd.op(x, pad, "x"), gd.op(w, pad, "w"), gd.op(b, name="bias")
            for odt in (F32, hd):
                yg, yp = gd.out((M, N), odt, pad, name=f"y {odt}"), nan_like((M, N), odt)
                ops.gemm(ops.NT, ops.BF16, M, N, K, xg, K + pad, wg, K + pad, yg, N + pad, bias=bg)
                ops.gemm(ops.NT, ops.BF16, M, N, K, x, K, w, K, yp, N, bias=b)
                sync()
                gd.check()
                assert finite(yg) and same(yg, yp), kc.describe_worst(yg, yp.double(), tile=128)
                assert_excess(f"gemm_wide {kind} {M}x{N}x{K} variant {variant} -> {odt}", yg, u, mag, K + 1, U_MFMA16, tile=128)
            gvg, gdg = gd.out((M, N), hd, pad, name="gelu"), gd.out((M, N), hd, pad, name="gelu'")
            gvp, gdp = nan_like((M, N), hd), nan_like((M, N), hd)
            ops.gemm(ops.NT, ops.BF16, M, N, K, xg, K + pad, wg, K + pad, gvg, N + pad, bias=bg, gelu_deriv_out=gdg)
            ops.gemm(ops.NT, ops.BF16, M, N, K, x, K, w, K, gvp, N, bias=b, gelu_deriv_out=gdp)
            sync()
            gd.check()
            assert finite(gvg) and finite(gdg) and same(gvg, gvp) and same(gdg, gdp)
            assert G.rel(gvg, _gelu64(u)) < tol16 and G.rel(gdg, _gelu_grad64(u)) < tol16
            dv = (K + 1) * U_MFMA16 * mag                     # error of the fp32 value v = x w^T + b that gelu and gelu' are taken of
            ev_g, ev_gp = gelu_eval_err(u)
            zero = torch.zeros_like(u)
            assert_excess(f"gemm_wide {kind} {M}x{N}x{K} variant {variant} gelu(v)", gvg, _gelu64(u), zero, 0, U_MFMA16, tile=128,
                          abs_extra=LIP_GELU * dv + ev_g + D_CDF * dv)
            assert_excess(f"gemm_wide {kind} {M}x{N}x{K} variant {variant} gelu'(v)", gdg, _gelu_grad64(u), zero, 0, U_MFMA16, tile=128,
                          abs_extra=LIP_GELU_GRAD * dv + ev_gp)
            if K % 128 == 0 and N % 64 == 0:      # data gradients dx[M, K] = dy[M, N] w[N, K]: an NT product on the transposed copy
                dy, wt, aux = G.rnd(M, N, dtype=hd, seed=3), w.t().contiguous(), G.rnd(M, K, dtype=hd, seed=4)
                dyg, wtg, auxg = gd.op(dy, pad, "dy"), gd.op(wt, pad, "wt"), gd.op(aux, pad, "aux")
                prod, aprod = dy.double() @ w.double(), dy.double().abs() @ w.double().abs()
                dxg, dxp = gd.out((M, K), hd, pad, name="dx"), nan_like((M, K), hd)
                ops.gemm(ops.NT, ops.BF16, M, K, N, dyg, N + pad, wtg, N + pad, dxg, K + pad, aux=auxg, ldaux=K + pad, aux_mul=True)
                ops.gemm(ops.NT, ops.BF16, M, K, N, dy, N, wt, N, dxp, K, aux=aux, ldaux=K, aux_mul=True)
                g0 = G.rnd(M, K, seed=5)
                gg, gp = gd.out((M, K), F32, pad, src=g0, name="g (accumulated)"), g0.clone()
                ops.gemm(ops.NT, ops.BF16, M, K, N, dyg, N + pad, wtg, N + pad, gg, K + pad, accumulate=True)
                ops.gemm(ops.NT, ops.BF16, M, K, N, dy, N, wt, N, gp, K, accumulate=True)
                sync()
                gd.check()
                assert finite(dxg) and finite(gg) and same(dxg, dxp) and same(gg, gp)
                assert_excess(f"gemm_wide {kind} dgrad * aux {M}x{K}x{N} variant {variant}", dxg, prod * aux.double(), aprod * aux.double().abs(), N + 1,
                              U_MFMA16, tile=128)
                assert_excess(f"gemm_wide {kind} dgrad accumulate {M}x{K}x{N} variant {variant}", gg, g0.double() + prod, aprod + g0.double().abs(), N + 1,
                              U_MFMA16, tile=128)
    finally:
        ops.use(prev)


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("M,N,K,S", [(1024, 768, 3072, 2), (1024, 768, 2304, 3), (4096, 384, 1536, 4), (1000, 200, 1088, 2)])
def test_gemm_split_k_atomic_guarded(kind, M, N, K, S, pad):
    gemm_split_k_atomic_guarded(kind, M, N, K, S, pad)


def gemm_split_k_atomic_guarded(kind, M, N, K, S, pad):
    """K slices adding into an fp32 result with atomics (csrc/gemm_fast.hip): the zeroed forward form and the accumulating data-gradient form.
    Order-dependent, so no bit compare; but the componentwise bound holds in ANY order: K products + S partial sums + bias / C0."""
    prev = ops.use(kind)
    try:
        hd = ops.half_dtype()
        x, w, b = G.rnd(M, K, dtype=hd), G.rnd(N, K, dtype=hd, scale=K ** -0.5, seed=1), G.rnd(N, seed=2)
        prod, aprod = x.double() @ w.double().t(), x.double().abs() @ w.double().abs().t()
        with _gemm_config(wide=(0, 0), splitk=(S, 1)):
            gd = Guards()
            xg, wg, bg = gd.op(x, pad, "x"), gd.op(w, pad, "w"), gd.op(b, name="bias")
            yg = gd.out((M, N), F32, pad, name="y (zeroed by the launcher)")
            ops.gemm(ops.NT, ops.BF16, M, N, K, xg, K + pad, wg, K + pad, yg, N + pad, bias=bg)
            g0 = G.rnd(M, N, seed=5)
            gg = gd.out((M, N), F32, pad, src=g0, name="g (accumulated)")
            ops.gemm(ops.NT, ops.BF16, M, N, K, xg, K + pad, wg, K + pad, gg, N + pad, accumulate=True)
            sync()
            gd.check()
            assert finite(yg) and finite(gg)
            assert_excess(f"split-K {kind} {M}x{N}x{K} S={S} forward", yg, prod + b.double(), aprod + b.double().abs(), K + S + 1, U_MFMA16)
            assert_excess(f"split-K {kind} {M}x{N}x{K} S={S} accumulate", gg, g0.double() + prod, aprod + g0.double().abs(), K + S + 1, U_MFMA16)
            assert G.rel(yg, prod + b.double()) < 2e-6 and G.rel(gg, g0.double() + prod) < 1e-6
    finally:
        ops.use(prev)


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("layout,M,N,K", [(ops.NT, 4096, 288, 96), (ops.NN, 1000, 384, 96), (ops.TN, 96, 288, 4100 // 4 * 4), (ops.NT, 300, 72, 40),
                                          (ops.TN, 64, 96, 136), (ops.TN, 96, 96, 8192)])      # (the 64 x 96 and 96 x 96 tiles in TN)
def test_gemm_bf16x3_guarded(layout, M, N, K, pad):
    gemm_bf16x3_guarded(layout, M, N, K, pad)


def gemm_bf16x3_guarded(layout, M, N, K, pad):
    """compute = bf16x3 (fp32 operands split into hi + lo while staged).  Its operand error (~2^-17 per product) is a property of
    the split, not of the accumulation, so the per-element bound is the fp32 one with that operand term added: 3 * 2^-17 |A| |B| (hi·lo,
    lo·hi kept, lo·lo dropped, two operand roundings)."""
    A, B = _operands(layout, ops.X3, False, M, N, K)
    ref, ab = _product64(layout, ops.X3, A, B)
    tn = layout == ops.TN
    with _gemm_config():
        gd = Guards()
        Ag, Bg = gd.op(A, pad, "A"), gd.op(B, pad, "B")
        C0 = G.rnd(M, N, seed=9) if tn else None
        Cg, Cp = gd.out((M, N), F32, pad, src=C0, name="C"), (C0.clone() if tn else nan_like((M, N), F32))
        bias = None if tn else G.rnd(N, seed=2)
        ops.gemm(layout, ops.X3, M, N, K, Ag, A.shape[1] + pad, Bg, B.shape[1] + pad, Cg, N + pad, bias=gd.op(bias, name="bias"), accumulate=tn)
        ops.gemm(layout, ops.X3, M, N, K, A, A.shape[1], B, B.shape[1], Cp, N, bias=bias, accumulate=tn)
        sync()
        gd.check()
        full = ref + (C0.double() if tn else bias.double())
        mag = ab + (C0.double().abs() if tn else bias.double().abs())
        assert finite(Cg) and G.rel(Cg, full) < 2e-5
        # K * u_add * mag covers the accumulation; the split's operand error enters as a multiple of the same |A| |B| term
        nadd = 3 * K + K // 32 + 2 + math.ceil(3 * 2.0 ** -17 / U_MFMA16)
        assert_excess(f"bf16x3 layout {layout} {M}x{N}x{K}", Cg, full, mag, nadd, U_MFMA16)
        if not tn:
            assert same(Cg, Cp)


NAN_CASES = [("generic (fp32 B beside 16-bit A)", ops.NT, True, 257, 130, 72), ("gemm_fast 64 x 64", ops.NT, False, 520, 64, 40),
             ("gemm_fast NN", ops.NN, False, 520, 64, 40), ("gemm_panel", ops.NT, False, 4096, 384, 96), ("gemm_wide", ops.NT, False, 384, 256, 192)]
NAN_FAMILY = {"generic": ops.ROUTE_GENERIC, "gemm_fast": ops.ROUTE_FAST, "gemm_panel": ops.ROUTE_PANEL, "gemm_wide": ops.ROUTE_WIDE}


@pytest.mark.parametrize("what,layout,mixed,M,N,K", NAN_CASES, ids=[c[0] for c in NAN_CASES])
def test_gemm_nan_stays_in_its_row_and_column(what, layout, mixed, M, N, K):
    gemm_nan_stays_in_its_row_and_column(layout, mixed, M, N, K, wide=(2, 0) if what == "gemm_wide" else None, family=NAN_FAMILY[what.split()[0]])


def gemm_nan_stays_in_its_row_and_column(layout, mixed, M, N, K, wide=None, family=None):
    """A NaN inside one row of A makes exactly that row of C non-finite and leaves every other element bit-equal to the clean run; likewise
    one column through B.  (Shapes chosen so that each kernel file of scot_gemm's dispatch takes one: `family`, where given, is asserted
    through scot_gemm_route on the very arguments of the launch.)"""
    A, B = _operands(layout, ops.BF16, mixed, M, N, K)
    with _gemm_config(wide=wide):
        def run(A_, B_):
            gd = Guards()
            C = gd.out((M, N), F32, name="C")
            args = (layout, ops.BF16, M, N, K, gd.op(A_, name="A"), A_.shape[1], gd.op(B_, name="B"), B_.shape[1], C, N)
            assert family is None or ops.gemm_route(*args)[0] == family, f"the case reaches kernel family {ops.gemm_route(*args)[0]}, not {family}"
            ops.gemm(*args)
            sync()
            gd.check()
            return C
        clean = run(A, B)
        assert finite(clean)
        r, c = M - 2, N // 2 + 1
        An = A.clone()
        An[r, K // 3] = NAN
        got = run(An, B)
        keep = torch.ones(M, dtype=torch.bool, device=G.DEV)
        keep[r] = False
        assert not bool(torch.isfinite(got[r]).any()), "the poisoned row must be non-finite in every column"
        assert torch.equal(got[keep], clean[keep]), "a NaN in one row of A changed other rows"
        Bn = B.clone()
        if layout == ops.NT:
            Bn[c, K // 2] = NAN
        else:
            Bn[K // 2, c] = NAN
        got = run(A, Bn)
        keepc = torch.ones(N, dtype=torch.bool, device=G.DEV)
        keepc[c] = False
        assert not bool(torch.isfinite(got[:, c]).any())
        assert torch.equal(got[:, keepc], clean[:, keepc]), "a NaN in one column of B changed other columns"


@pytest.mark.parametrize("M,N,K", [(257, 136, 72), (512, 256, 128)])
def test_gemm_operands_near_binary16_maximum(M, N, K):
    gemm_operands_near_binary16_maximum(M, N, K)


def gemm_operands_near_binary16_maximum(M, N, K):
    """binary16 build, operands up to the format's largest finite value (65504) and an fp32 result: products reach 4e9 and sums 1e11, all
    inside fp32 — the result is finite and within the per-element bound (nothing is formed in 16 bits on the way)."""
    prev = ops.use("f16")
    try:
        hd = ops.half_dtype()
        g = torch.Generator().manual_seed(M + N + K)
        big = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) * 65504.0).to(G.DEV).to(hd)
        A, B = big(M, K), big(N, K)
        A[0, :], B[0, :] = 65504.0, 65504.0                # the extreme corner: K * 65504^2
        A[1, :] = -65504.0
        assert finite(A) and finite(B)
        ref, ab = _product64(ops.NT, ops.BF16, A, B)
        with _gemm_config():
            gd = Guards()
            C = gd.out((M, N), F32, name="C")
            ops.gemm(ops.NT, ops.BF16, M, N, K, gd.op(A, name="A"), K, gd.op(B, name="B"), K, C, N)
            sync()
            gd.check()
        assert finite(C)
        assert_excess(f"binary16-maximum operands {M}x{N}x{K}", C, ref, ab, K, U_MFMA16)
    finally:
        ops.use(prev)


# ======================================================================================================= grouped weight gradients
def _wgroup_dims(C):
    return [(C, 4 * C), (4 * C, C), (C, C), (3 * C, C)]            # (M_i, N_i) of fc2, fc1, proj, qkv: dW_i [M_i, N_i]


WGROUP_GUARDED = [(K, C, -1, False) for K, C in G.WGROUP_CASES] + [(K, C, -1, True) for K, C in G.WGROUP_CASES if C % 8 == 0 and K % 8 == 0] + \
                 [(1024, 768, 0, False), (1024, 768, 2, True), (4096, 384, 1 | (4 << 4), True), (4096, 384, 2 | (2 << 4), False), (512, 128, 1, True),
                  (192, 256, 0 | (3 << 4), True), (2048, 1536, -1, False), (8192, 768, -1, True)]


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("K,C,forced,scaled", WGROUP_GUARDED)
def test_wgrad_group_guarded(kind, K, C, forced, scaled):
    wgrad_group_guarded(kind, K, _wgroup_dims(C), forced, scaled)


def wgrad_group_guarded(kind, K, dims, forced, scaled):
    """scot_wgrad_group with the dW of a layer BACK TO BACK in one guarded flat buffer at the gradient arena's 64-float alignment, the bias
    gradients likewise; the padding between neighbours is checked like a band.  forced: -1 = the library's tile policy, else kernel
    instantiation | K slices << 4 of the 128 x 128 tiles (scot_gemm_wide_config mode 2).  scaled: the modes of the lazy zero-grad —
    GRAD_STORE_SCALED writes over NaN (what the arena holds beside a first writer), GRAD_ADD_SCALED, GRAD_ADD.
    (c): gemm_excess with K = the token count (loose for fp32 at K = 65536, so the existing rel() < 1e-6 stays beside it)."""
    prev = ops.use(kind)
    try:
        hd = ops.half_dtype()
        n = len(dims)
        modes = [(ops.GRAD_STORE_SCALED, ops.GRAD_ADD_SCALED, ops.GRAD_ADD)[i % 3] for i in range(n)] if scaled else [ops.GRAD_ADD] * n
        sval = 2.0 ** -7 if scaled else 1.0
        s = torch.tensor([sval], device=G.DEV) if scaled else None
        dys = [G.rnd(K, m, dtype=hd, scale=0.5, seed=10 + i) for i, (m, _) in enumerate(dims)]
        xs = [G.rnd(K, nn, dtype=hd, seed=20 + i) for i, (_, nn) in enumerate(dims)]
        dws0 = [G.rnd(m, nn, seed=30 + i) for i, (m, nn) in enumerate(dims)]
        dbs0 = [G.rnd(m, seed=40 + i) for i, (m, _) in enumerate(dims)]
        covered = all(m % 8 == 0 and nn % 8 == 0 for m, nn in dims) and K % 8 == 0
        with _gemm_config(wide=(2, forced) if forced >= 0 else None, splitk=(0, 1)) as lib:
            gd = Guards()
            dyg, xg = [gd.op(t, name=f"dY{i}") for i, t in enumerate(dys)], [gd.op(t, name=f"X{i}") for i, t in enumerate(xs)]
            store = [md == ops.GRAD_STORE_SCALED for md in modes]
            dwg = gd.group([tuple(t.shape) for t in dws0], F32, srcs=[None if st else t for t, st in zip(dws0, store)], name="dW arena")
            dbg = gd.group([tuple(t.shape) for t in dbs0], F32, srcs=dbs0, name="dbias arena")
            dwp = [nan_like(t.shape, F32) if st else t.clone() for t, st in zip(dws0, store)]
            dbp = [t.clone() for t in dbs0]
            sg = gd.op(s, name="grad_scale")
            ok = ops.wgrad_group(ops.BF16, list(zip(dyg, xg, dwg, dbg)), modes if scaled else None, sg)
            assert ok == covered
            if not ok:      # shapes the grouped kernel declines go through the per-problem path (same contract), guarded as well
                for dy, x, dw, db in zip(dyg, xg, dwg, dbg):
                    ops.linear_wgrad(ops.BF16, dy, x, dw, dbias=db)
            else:
                assert ops.wgrad_group(ops.BF16, list(zip(dys, xs, dwp, dbp)), modes if scaled else None, s)
            sync()
            gd.check()
        worst = 0.0
        for i, (dy, x, dw0, dw, db0, db, md) in enumerate(zip(dys, xs, dws0, dwg, dbs0, dbg, modes)):
            prod, aprod = dy.double().t() @ x.double(), dy.double().abs().t() @ x.double().abs()
            base = 0.0 if md == ops.GRAD_STORE_SCALED else dw0.double()
            sv = 1.0 if md == ops.GRAD_ADD else sval                    # the plain accumulation takes no scale
            ref = base + sv * prod
            mag = (0.0 if md == ops.GRAD_STORE_SCALED else dw0.double().abs()) + sv * aprod
            assert finite(dw) and finite(db), i
            # K products, the partial sums of the K slices (each at least 32 tokens deep), the scale and the add into the arena
            worst = max(worst, assert_excess(f"wgrad_group {kind} K={K} dW{i} {tuple(dw.shape)} mode {md} forced {forced}", dw, ref, mag, K + K // 32 + 3,
                                             U_MFMA16))
            assert G.rel(dw.double() - base, sv * prod) < 1e-6, (K, i, md)
            assert G.rel(db.double() - db0.double(), dy.double().sum(0)) < 2e-6
            if ok:      # the weight gradients are deterministic (partial tiles + one grouped pass); the bias gradients are atomics
                assert same(dw, dwp[i]), (i, kc.describe_worst(dw, dwp[i].double()))
        print(f"worst excess wgrad_group {kind} K={K} forced {forced} scaled {scaled}: {worst:.3f}")
    finally:
        ops.use(prev)


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("mode", [ops.GRAD_ADD, ops.GRAD_STORE_SCALED, ops.GRAD_ADD_SCALED])
@pytest.mark.parametrize("M,C", [(2048, 96), (4096, 96), (1000, 96), (1024, 192), (2056, 192)])
def test_wgrad_mlp_guarded(kind, M, C, mode):
    wgrad_mlp_guarded(kind, M, C, mode)


def wgrad_mlp_guarded(kind, M, C, mode):
    """scot_wgrad_mlp (fc1 / fc2 weight + bias gradients with gelu(u), gelu'(u), du recomputed on the fly) writing dW1 | db1 | dW2 | db2 into ONE
    guarded contiguous range — the gradient arena's layout for these four — with bands on both sides.
    Reference: the chain restated in fp64 on the operands as stored (csrc/wgrad_mlp.hip's header):
        u = h16 W1^T + b1,   act = gelu(u),   D = dz W2,   du = D ⊙ gelu'(u),   dW1 = du^T h16,  db1 = Σ du,  dW2 = dz^T act,  db2 = Σ dz
    (c): gemm_excess with K = the token count on dW1 and dW2.  act and du never exist in HBM: the kernel forms them in fp32 from its own
    accumulators and rounds them ONCE to the operand format as MFMA operands.  Their deviation from the fp64 act / du is bounded elementwise —
      u and D carry the roundoff of a C-term (hid-term) fp32 contraction: du_acc = (C + 1) u_add (|h| |W1| + |b1|),  dD = hid u_add |dz| |W2|;
      act:  1.13 du_acc + gelu's evaluation error + one operand rounding;
      du:   |gelu'| dD + (|D| + dD) (0.8 du_acc + gelu' evaluation error) + one product rounding + one operand rounding —
    and enters the bound as an operand term E^T |h| resp. |dz|^T E, as the hi + lo split's does for bf16x3.  The bias gradients are sums of the
    same du / dz over the tokens and are held to the same kind of bound.  (d): the whole range bit-identical to the plain launch."""
    prev = ops.use(kind)
    try:
        hd = ops.half_dtype()
        hid = 4 * C
        h16, dz = G.rnd(M, C, dtype=hd, seed=1), G.rnd(M, C, dtype=hd, scale=0.5, seed=2)
        w1, b1 = G.rnd(hid, C, scale=C ** -0.5, seed=3).to(hd), G.rnd(hid, seed=4, scale=0.2)
        w2 = G.rnd(C, hid, scale=hid ** -0.5, seed=5).to(hd)
        w2t = w2.t().contiguous()
        sizes = [hid * C, hid, C * hid, C]
        tot = sum(sizes)
        sval = 2.0 ** -7 if mode != ops.GRAD_ADD else 1.0
        s = torch.tensor([sval], device=G.DEV) if mode != ops.GRAD_ADD else None
        flat0 = G.rnd(tot, seed=6)

        def views(flat):
            o, out = 0, []
            for sz in sizes:
                out.append(flat[o:o + sz])
                o += sz
            return out[0].view(hid, C), out[1], out[2].view(C, hid), out[3]

        def start(flat):
            dW1, db1, dW2, db2 = views(flat)
            if mode == ops.GRAD_STORE_SCALED:      # what zero_grad leaves for a storing first writer
                dW1.fill_(NAN)
                dW2.fill_(NAN)
            return dW1, db1, dW2, db2
        gd = Guards()
        fg = gd.out((tot,), F32, src=flat0, name="dW1|db1|dW2|db2")
        fp = flat0.clone()
        outs_g, outs_p = start(fg), start(fp)
        args = [gd.op(h16, name="h16"), gd.op(dz, name="dz"), gd.op(w1, name="w1"), gd.op(b1, name="b1"), gd.op(w2t, name="w2t")]
        assert ops.wgrad_mlp(*args, *outs_g, mode=mode, grad_scale=gd.op(s, name="grad_scale"))
        assert ops.wgrad_mlp(h16, dz, w1, b1, w2t, *outs_p, mode=mode, grad_scale=s)
        sync()
        gd.check()
        assert finite(fg)
        assert same(fg, fp)      # partial planes + one flat reduce: deterministic, bias gradients included
        # ---- the fp64 restatement and the operands' deviation from it
        D64 = torch.float64
        h, z, W1, W2, B1 = h16.to(D64), dz.to(D64), w1.to(D64), w2.to(D64), b1.to(D64)
        uop = kc.UNIT[hd]
        u = h @ W1.t() + B1
        du_acc = (C + 1) * U_MFMA16 * (h.abs() @ W1.abs().t() + B1.abs())
        act, gp = _gelu64(u), _gelu_grad64(u)
        ev_g, ev_gp = gelu_eval_err(u)
        e_act32 = LIP_GELU * du_acc + ev_g + D_CDF * du_acc                       # the fp32 value before the operand rounding
        e_act = e_act32 + uop * (act.abs() + e_act32)
        Dm = z @ W2
        dD = hid * U_MFMA16 * (z.abs() @ W2.abs())
        du = Dm * gp
        e_du32 = gp.abs() * dD + (Dm.abs() + dD) * (LIP_GELU_GRAD * du_acc + ev_gp) + kc.U32 * du.abs()
        e_du = e_du32 + uop * (du.abs() + e_du32)
        base = [t.double() for t in views(flat0.clone())]
        wscale = sval                                                             # mode 0: plain +=; 1: store s * acc; 2: += s * acc
        if mode == ops.GRAD_STORE_SCALED:
            base[0], base[2] = torch.zeros_like(base[0]), torch.zeros_like(base[2])
        nadd = M + M // 32 + 3       # M products, the partial sums of the token slices (each at least 32 rows), the scale, the add into the arena
        for name, got, ref, mag, ex, b0 in (
                ("dW1", outs_g[0], du.t() @ h, (du.abs() + e_du).t() @ h.abs(), e_du.t() @ h.abs(), base[0]),
                ("dW2", outs_g[2], z.t() @ act, z.abs().t() @ (act.abs() + e_act), z.abs().t() @ e_act, base[2])):
            assert_excess(f"wgrad_mlp {kind} M={M} C={C} mode {mode} {name}", got, b0 + wscale * ref, b0.abs() + wscale * mag, nadd, U_MFMA16,
                          abs_extra=wscale * ex)
        # bias gradients (always a plain accumulation): sums over the tokens of the same du / dz
        for name, got, col, ecol, b0 in (("db1", outs_g[1], du, e_du, base[1]), ("db2", outs_g[3], z, torch.zeros_like(z), base[3])):
            ref = b0 + col.sum(0)
            within(got, ref, nadd * kc.U32 * (col.abs().sum(0) + ecol.sum(0) + b0.abs()) + ecol.sum(0) + kc.U32 * ref.abs(), f"wgrad_mlp {name}")
        # beside it, as for the grouped gradients: the global norm against the same restatement on the operands the kernel rounds (16-bit act / du)
        act16, du16 = act.to(hd).to(D64), du.to(hd).to(D64)
        tol = 4e-3 if kind == "bf16" else 6e-4      # act / du are rounded to 16 bits at possibly different last places than the fp64 values
        assert G.rel(outs_g[0].double() - base[0], wscale * (du16.t() @ h)) < tol and G.rel(outs_g[2].double() - base[2], wscale * (z.t() @ act16)) < tol
    finally:
        ops.use(prev)


# ====================================================================================== rounding models (attention, conditional layer norm)
# A rigorous bound through a softmax or a normalisation is not practical.  Instead the test computes, on its own inputs, a ROUNDING MODEL: the
# fp64 restatement with a rounding at the points the kernels document (attention: normalised q and k, P, dS and the stored result in the
# operand format — test_kernels_gpu.py's comment on its 16-bit tolerances, csrc/attention*.hip; CLN: the stored result and, for 16-bit x,
# the input, which already is 16-bit).  Its per-row error against the exact fp64 result is e_model[row]; every row of the kernel's result must
# satisfy  e_kernel[row] <= MARGIN * max(e_model[row], median(e_model))  (kernel_checks.row_model_excess; no row left out).
# MARGIN covers what the model leaves out — fp32 accumulation order, the hardware's exp / rsqrt — and is measured against the REFERENCE,
# never against a kernel:  python tests/test_kernels_guarded_gpu.py --measure-margins  runs the model on the CPU over ATTN_CASES and the CLN
# shapes with its arithmetic in fp32 instead of fp64, in two summation orders, and prints the worst per-row ratio of those runs to the fp64
# model per class; MARGIN is twice that ratio (the factor two: the hardware's transcendental error is not in the model either).
# (run from the repository root with PYTHONPATH=.; numbers beside MARGIN below and in DESIGN.md §4)
class _RoundST(torch.autograd.Function):
    """round in the forward, pass the gradient through: the kernels differentiate the unrounded expression"""

    @staticmethod
    def forward(ctx, x, fn):
        return fn(x)

    @staticmethod
    def backward(ctx, g):
        return g, None


class _RoundGrad(torch.autograd.Function):
    """identity in the forward, round the gradient (dS)"""

    @staticmethod
    def forward(ctx, x, fn):
        ctx.fn = fn
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return ctx.fn(g), None


def _round_bits(x, bits):
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(m * 2.0 ** bits) / 2.0 ** bits, e)


def _rounders(klass, half):
    """(operand rounding, result dtype) of a compute class: "f32" exact fp32 MFMA, "x3" hi + lo split (~2^-17), "16" the operand format"""
    if klass == "16":
        return (lambda x: x.to(half).to(x.dtype)), half
    if klass == "x3":
        return (lambda x: _round_bits(x, 17)), F32
    return (lambda x: x.to(F32).to(x.dtype)), F32


def _to_windows(x, Hp, Wp, ws, shift):
    """[B, Hp*Wp, heads] per token -> [B*nW, heads, N] in G._attn_ref's window layout (roll, partition)"""
    B, heads = x.shape[0], x.shape[-1]
    x = x.view(B, Hp, Wp, heads)
    if shift:
        x = torch.roll(x, (-shift, -shift), (1, 2))
    return x.view(B, Hp // ws, ws, Wp // ws, ws, heads).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, heads).transpose(1, 2)


def attn_model(qkv, table, ls, dout, case, klass, half, dtype=torch.float64, reverse=False, exact=False, out_fwd=None):
    """(out, dqkv) in fp64 of G._attn_ref evaluated in `dtype`, with the class's roundings (exact: without any): normalised q and k, P and
    dS in the operand format, out and dqkv in the result type.  One more point that the sources state: every backward kernel takes the
    softmax backward's row term delta = rowsum(dO ∘ O) from the STORED, rounded forward output (csrc/attention.hip: "delta = rowsum(dO ∘ O)
    comes from the forward output"; csrc/attention_w16.hip: "dS uses delta from the stored (rounded) forward output").  With 16-bit
    results this is the largest single contribution to the error of dq / dk where the attention is peaked: P (dP - delta) cancels and the
    rounding of O does not.
    With delta = sum_k P dP (what the softmax backward subtracts) the kernel's dS is P (dP - delta) - P (delta~ - delta); the
    second term is the gradient of -(delta~ - delta) · logsumexp(s) and is added to the model's backward in that form.  out_fwd: the stored
    forward output the backward is given (an OPERAND of scot_window_attn_bwd); default: the model's own rounded output."""
    B, Hp, Wp, C, heads, ws, shift = case
    rop, rdt = _rounders(klass, half)
    rres = lambda x: x.to(rdt).to(x.dtype)
    stash = {}

    def hook(name, t):
        if exact:
            return t
        if name == "s":
            stash["s"] = t = _RoundGrad.apply(t, rop)
            return t
        r = _RoundST.apply(t, rres if name == "out" else rop)
        if name == "p":
            stash["p"], stash["p_r"] = t.detach(), r
        return r
    q = qkv.detach().to(dtype).clone().requires_grad_(True)
    out = G._attn_ref(q, table.to(dtype), ls.to(dtype), B, Hp, Wp, C, heads, ws, shift, hook=hook, reverse=reverse)
    loss = (out * dout.to(dtype)).sum()
    if not exact:
        stored = out.detach() if out_fwd is None else out_fwd.to(dtype)
        delta_k = _to_windows((stored * dout.to(dtype)).view(B, Hp * Wp, heads, C // heads).sum(-1), Hp, Wp, ws, shift)
        (dP,) = torch.autograd.grad(loss, stash["p_r"], retain_graph=True)
        delta = (stash["p"] * dP).sum(-1)                   # what autograd's softmax backward subtracts
        loss = loss - ((delta_k - delta) * torch.logsumexp(stash["s"], -1)).sum()
    loss.backward()
    return out.detach().double(), (q.grad if exact else rres(q.grad)).double()


def cln_model(x, res, t, gw_w, gw_b, bw_w, bw_b, sc, dout, cond, klass_dt, dtype=torch.float64, reverse=False, exact=False):
    """(out, dx) in fp64 of the conditional layer norm restated as in test_cln_fwd_bwd, evaluated in `dtype`; the model rounds the stored
    results: out to fp32, dx to x's type."""
    B, L, C = x.shape
    fl = (lambda v: v.flip(-1)) if reverse else (lambda v: v)
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    xs = fl(xx)
    mu = xs.mean(-1, keepdim=True)
    xh = (xx - mu) / torch.sqrt(((xs - mu) ** 2).mean(-1, keepdim=True) + 1e-5)
    tt = t.to(dtype).view(B, 1, 1)
    g = tt * gw_w.to(dtype) + gw_b.to(dtype) if cond else gw_b.to(dtype)
    b = tt * bw_w.to(dtype) + bw_b.to(dtype) if cond else bw_b.to(dtype)
    y = g * xh + b
    out = res.to(dtype) + (sc.to(dtype).view(B, 1, 1) * y if sc is not None else y)
    out.backward(dout.to(dtype))
    if exact:
        return out.detach().double(), xx.grad.double()
    return out.detach().to(F32).double(), xx.grad.to(klass_dt).double()


# class -> MARGIN = 2 x the worst per-row ratio printed by --measure-margins (fp32 model, plain and reversed order, against the fp64 model)
# worst ratios measured: 16-bit operands 1.65 (a rounding that falls the other way), hi + lo split 3.33, exact fp32 MFMA 40.10 (the model's
# only rounding there is the stored result's, so fp32 arithmetic IS the error), conditional layer norm 6.61
MARGIN = {"attn16": 2 * 1.65, "attnx3": 2 * 3.33, "attnf32": 2 * 40.10, "cln": 2 * 6.61}


def _attn_inputs(case, cdt):
    B, Hp, Wp, C, heads, ws, shift = case
    L, TS = Hp * Wp, (2 * ws - 1) ** 2
    qkv = G.rnd(B, L, 3 * C, dtype=cdt)
    table = (16 * torch.sigmoid(G.rnd(heads, TS, seed=1))).contiguous()
    ls = torch.linspace(math.log(3.0), math.log(20.0), heads, device=G.DEV)
    dout = G.rnd(B, L, C, dtype=cdt, seed=2)
    return qkv, table, ls, dout


@pytest.mark.parametrize("compute", [ops.F32, ops.BF16, ops.X3, "f16"])
@pytest.mark.parametrize("case", G.ATTN_CASES)
def test_window_attention_guarded(compute, case):
    f16 = compute == "f16"
    window_attention_guarded("f16" if f16 else "bf16", ops.BF16 if f16 else compute, case)


def window_attention_guarded(kind, compute, case):
    """scot_window_attn_fwd / bwd / bwd_rep + scot_replica_reduce / scot_window_attn_probs with every tensor guarded: (a), (b), the per-row bound
    against the rounding model for out and dqkv, (d) for out, lse, dqkv and the probabilities; dbias_table / dlogit_scale (atomics) at
    the tolerances of test_window_attention_fwd_bwd."""
    prev = ops.use(kind)
    try:
        half = ops.half_dtype()
        B, Hp, Wp, C, heads, ws, shift = case
        klass = "16" if compute == ops.BF16 else "x3" if compute == ops.X3 else "f32"
        cdt = half if compute == ops.BF16 else F32
        L, TS, N = Hp * Wp, (2 * ws - 1) ** 2, ws * ws
        nW = (Hp // ws) * (Wp // ws)
        qkv, table, ls, dout = _attn_inputs(case, cdt)
        gd = Guards()
        qg, tg, lg, dg = gd.op(qkv, name="qkv"), gd.op(table, name="bias_table"), gd.op(ls, name="logit_scale"), gd.op(dout, name="dout")
        og, lseg = gd.out((B, L, C), cdt, name="out"), gd.out((B * nW, heads, N), F32, name="lse")
        dqg, dtg, dlg = gd.out((B, L, 3 * C), cdt, name="dqkv"), gd.out((heads, TS), F32, fill=0.0, name="dbias_table"), \
            gd.out((heads,), F32, fill=0.0, name="dlogit_scale")
        ops.window_attn_fwd(compute, qg, og, lseg, tg, lg, B, Hp, Wp, C, heads, ws, shift)
        ops.window_attn_bwd(compute, qg, og, dg, lseg, tg, lg, dqg, dtg, dlg, B, Hp, Wp, C, heads, ws, shift)
        op_, lsep, dqp = nan_like((B, L, C), cdt), nan_like((B * nW, heads, N), F32), nan_like((B, L, 3 * C), cdt)
        dtp, dlp = torch.zeros(heads, TS, device=G.DEV), torch.zeros(heads, device=G.DEV)
        ops.window_attn_fwd(compute, qkv, op_, lsep, table, ls, B, Hp, Wp, C, heads, ws, shift)
        ops.window_attn_bwd(compute, qkv, op_, dout, lsep, table, ls, dqp, dtp, dlp, B, Hp, Wp, C, heads, ws, shift)
        # the replica entry + the fold, replicas and destination guarded (strides with odd padding, as in the existing test)
        R, pad = 3, 5
        st, sl = heads * TS + pad, heads + pad
        rtg, rlg = gd.out((R * st,), F32, fill=0.0, name="table replicas"), gd.out((R * sl,), F32, fill=0.0, name="logit-scale replicas")
        dq2g = gd.out((B, L, 3 * C), cdt, name="dqkv (replica entry)")
        ops.window_attn_bwd_rep(compute, qg, og, dg, lseg, tg, lg, dq2g, rtg, rlg, B, Hp, Wp, C, heads, ws, shift, R, st, sl)
        dstg = gd.out((heads + 2,), F32, fill=0.0, name="replica_reduce dst")
        d1 = gd.op(torch.tensor([0, 0, heads * TS], dtype=torch.int32, device=G.DEV), name="desc")
        d2 = gd.op(torch.tensor([0, 2, heads], dtype=torch.int32, device=G.DEV), name="desc")
        ops.replica_reduce(rtg, 1, R, st, d1, 1, heads * TS, rtg)
        ops.replica_reduce(rlg, 0, R, sl, d2, 1, heads, dstg)
        sync()
        gd.check()
        for name, t in (("out", og), ("lse", lseg), ("dqkv", dqg), ("dbias_table", dtg), ("dlogit_scale", dlg), ("dqkv rep", dq2g), ("rt", rtg), ("dst", dstg)):
            assert finite(t), name
        assert same(og, op_) and same(lseg, lsep) and same(dqg, dqp) and same(dq2g, dqg)
        # (c) per row against the rounding model
        ex_out, ex_dq = attn_model(qkv, table, ls, dout, case, klass, half, exact=True)
        mo_out, mo_dq = attn_model(qkv, table, ls, dout, case, klass, half, out_fwd=og)
        margin = MARGIN["attn" + klass]
        r_out, row_o = kc.row_model_excess(og.reshape(-1, C), ex_out.reshape(-1, C), mo_out.reshape(-1, C), margin)
        r_dq, row_d = kc.row_model_excess(dqg.reshape(-1, 3 * C), ex_dq.reshape(-1, 3 * C), mo_dq.reshape(-1, 3 * C), margin)
        print(f"worst ratio attention {kind} compute {compute} {case}: out {r_out * margin:.2f} x model (row {row_o}), dqkv {r_dq * margin:.2f} x model "
              f"(row {row_d}); margin {margin:.1f}")
        assert r_out <= 1.0, f"out row {row_o} (window row {row_o // Wp}): {r_out * margin:.2f} x the model's error; {kc.describe_worst(og, ex_out)}"
        assert r_dq <= 1.0, f"dqkv row {row_d}: {r_dq * margin:.2f} x the model's error; {kc.describe_worst(dqg, ex_dq)}"
        # the same against the model run on its OWN rounded forward output (nothing of the kernel enters the reference): a forward / backward
        # pair that is wrong in a self-consistent way cannot pass this one
        _, mo_dq0 = attn_model(qkv, table, ls, dout, case, klass, half)
        r_dq0, row_d0 = kc.row_model_excess(dqg.reshape(-1, 3 * C), ex_dq.reshape(-1, 3 * C), mo_dq0.reshape(-1, 3 * C), margin)
        print(f"worst ratio attention {kind} compute {compute} {case}: dqkv against the model on its own forward output {r_dq0 * margin:.2f} x model (row {row_d0})")
        assert r_dq0 <= 1.0, f"dqkv row {row_d0}: {r_dq0 * margin:.2f} x the independent model's error; {kc.describe_worst(dqg, ex_dq)}"
        # order-dependent sums: the tolerances of test_window_attention_fwd_bwd
        q64, t64, l64 = qkv.double().requires_grad_(True), table.double().requires_grad_(True), ls.double().requires_grad_(True)
        exact_p = {}
        keep_p = lambda name, v: (exact_p.__setitem__("p", v.detach()) if name == "p" else None, v)[1]
        G._attn_ref(q64, t64, l64, B, Hp, Wp, C, heads, ws, shift, hook=keep_p).backward(dout.double())
        t16 = ((1.2e-3, 2e-3), 2e-2) if half == torch.float16 else ((8e-3, 1.2e-2), 0.1)
        tol_g = 5e-5 if compute == ops.F32 else 2e-4 if compute == ops.X3 else t16[0][1]
        tol_ls = 2e-4 if compute == ops.F32 else 2e-3 if compute == ops.X3 else t16[1]
        assert G.rel(dtg, t64.grad) < tol_g and G.rel(dlg, l64.grad) < tol_ls
        assert G.rel(dtg, dtp) < 1e-5 and G.rel(dlg, dlp) < 5e-4
        assert G.rel(rtg[:heads * TS].view(heads, TS), dtg) < 1e-5 and G.rel(dstg[2:], dlg) < 5e-4 and bool(torch.all(dstg[:2] == 0))
        # the probabilities (output_attentions), where the entry covers the shape
        d = C // heads
        if d <= 64 and N * d * 4 <= 65536:
            pg, pp = gd.out((B * nW, heads, N, N), F32, name="probs"), nan_like((B * nW, heads, N, N), F32)
            ops.window_attn_probs(qg, lseg, tg, lg, pg, B, Hp, Wp, C, heads, ws, shift)
            ops.window_attn_probs(qkv, lsep, table, ls, pp, B, Hp, Wp, C, heads, ws, shift)
            sync()
            gd.check()
            assert finite(pg) and same(pg, pp)
            # per element: P = exp(s - lse).  With 16-bit operands every cosine carries two operand roundings (|cos| <= 1), so a logit is
            # off by at most 2 * scale * u and the forward's lse — a log-sum-exp of such logits — by as much: P is within exp(+-4 scale u) of
            # the exact value (+ 1e-5 for the fp32 arithmetic and the hardware exp).  Rows then sum to 1 within the same factor.
            uop = kc.UNIT[half] if klass == "16" else 2.0 ** -17 if klass == "x3" else kc.U32
            fac = math.expm1(4 * float(torch.exp(ls.max())) * uop) + 1e-5
            pe = exact_p["p"]
            bad = (pg.double() - pe).abs() > fac * pe + 1e-30
            assert not bool(bad.any()), f"{int(bad.sum())} probabilities beyond exp(4 scale u) of the reference; first at {bad.nonzero()[0].tolist()}"
            assert float((pg.double().sum(-1) - 1).abs().max()) <= fac
    finally:
        ops.use(prev)


@pytest.mark.parametrize("kind,compute", [("bf16", ops.F32), ("bf16", ops.BF16), ("f16", ops.BF16), ("bf16", ops.X3)])
@pytest.mark.parametrize("case", [(1, 32, 32, 96, 3, 16, 8), (2, 8, 8, 32, 2, 4, 2), (1, 14, 14, 32, 1, 7, 3)])
def test_window_attention_zero_token(kind, compute, case):
    window_attention_zero_token(kind, compute, case)


def window_attention_zero_token(kind, compute, case):
    """A token whose q and k are exactly zero (a padded position): F.normalize's clamp_min(1e-12) path.  Forward: the zero query attends by
    the bias table alone, the zero key scores cos = 0 — against the fp64 restatement, which states the reference's semantics.  Backward: the
    reference's gradient of a clamped row is g / eps; the fp32 kernels store that, the 16-bit kernels store 0 for a clamped row (g / eps
    overflows binary16, and the row's input is zero — csrc/attention.hip): pinned as documented.  Every other row is held to
    the tolerance of test_window_attention_fwd_bwd."""
    prev = ops.use(kind)
    try:
        half = ops.half_dtype()
        B, Hp, Wp, C, heads, ws, shift = case
        cdt = half if compute == ops.BF16 else F32
        L, TS, N = Hp * Wp, (2 * ws - 1) ** 2, ws * ws
        nW = (Hp // ws) * (Wp // ws)
        qkv, table, ls, dout = _attn_inputs(case, cdt)
        zt = [(0, 0), (B - 1, L - 1), (0, L // 2 + 1)]
        for b, tok in zt:
            qkv[b, tok, :2 * C] = 0
        gd = Guards()
        qg, tg, lg, dg = gd.op(qkv, name="qkv"), gd.op(table, name="bias_table"), gd.op(ls, name="logit_scale"), gd.op(dout, name="dout")
        og, lseg = gd.out((B, L, C), cdt, name="out"), gd.out((B * nW, heads, N), F32, name="lse")
        dqg, dtg, dlg = gd.out((B, L, 3 * C), cdt, name="dqkv"), gd.out((heads, TS), F32, fill=0.0), gd.out((heads,), F32, fill=0.0)
        ops.window_attn_fwd(compute, qg, og, lseg, tg, lg, B, Hp, Wp, C, heads, ws, shift)
        ops.window_attn_bwd(compute, qg, og, dg, lseg, tg, lg, dqg, dtg, dlg, B, Hp, Wp, C, heads, ws, shift)
        sync()
        gd.check()
        q64 = qkv.double().requires_grad_(True)
        ref = G._attn_ref(q64, table.double(), ls.double(), B, Hp, Wp, C, heads, ws, shift)
        ref.backward(dout.double())
        t16 = (1.2e-3, 2e-3) if half == torch.float16 else (8e-3, 1.2e-2)
        tol_o, tol_g = (2e-5, 5e-5) if compute == ops.F32 else (5e-5, 2e-4) if compute == ops.X3 else t16
        assert finite(og) and G.rel(og, ref.detach()) < tol_o
        zrow = torch.zeros(B, L, dtype=torch.bool, device=G.DEV)
        for b, tok in zt:
            zrow[b, tok] = True
            assert G.rel(og[b, tok], ref.detach()[b, tok]) < 4 * tol_o, "the zero token's own output row"
        gref = q64.grad.clone()
        got = dqg.double()
        # v's gradient of the zero token is an ordinary one; its q / k gradient is the clamped row
        if compute == ops.BF16:
            assert bool((got[zrow][:, :2 * C] == 0).all()), "16-bit build: a clamped row's gradient is stored as 0 (documented)"
            gref[zrow, :2 * C] = 0
        else:
            assert finite(dqg)
            assert G.rel(got[zrow][:, :2 * C], gref[zrow][:, :2 * C]) < 10 * tol_g, "fp32 results: g / eps, the reference's value"
            gref[zrow, :2 * C] = 0
            got[zrow, :2 * C] = 0        # (1e12-sized entries would drown every other row in one norm)
        assert bool(torch.isfinite(got).all()) and G.rel(got, gref) < tol_g
    finally:
        ops.use(prev)


# ----------------------------------------------------------------------------------------------------------- conditional layer norm
CLN_SHAPES = [(3, 64, 96), (2, 16, 768), (2, 9, 20), (2, 300, 48), (2, 1024, 192), (2, 5, 1536), (3, 33, 16), (64, 16, 768), (64, 64, 384), (5, 6, 128)]


def _cln_inputs(xdt, B, L, C):
    x, res, t = G.rnd(B, L, C, dtype=xdt), G.rnd(B, L, C, seed=1), torch.rand(B, generator=torch.Generator().manual_seed(B + L + C)).to(G.DEV)
    ps = [G.rnd(C, seed=2, scale=0.3), 1 + G.rnd(C, seed=3, scale=0.1), G.rnd(C, seed=4, scale=0.1), G.rnd(C, seed=5, scale=0.1)]
    return x, res, t, ps, G.rnd(B, L, C, seed=6)


@pytest.mark.parametrize("cond", [True, False])
@pytest.mark.parametrize("xdt", [F32, torch.bfloat16])
@pytest.mark.parametrize("B,L,C", CLN_SHAPES)
def test_cln_guarded(cond, xdt, B, L, C):
    cln_guarded(cond, xdt, B, L, C)


def cln_guarded(cond, xdt, B, L, C, constant_row=False):
    """scot_cln_fwd / bwd / bwd_finish with every tensor guarded — the four parameter gradients and d_xbias back to back at the arena's
    alignment.  (c): out and dx per row against the rounding model; mean / rstd against fp64 at one fp32 rounding each plus the sum's
    roundoff (C * 2^-24 relative to the row's magnitude); the parameter gradients (atomics) at the tolerances of test_cln_fwd_bwd.
    constant_row: one row of x is constant (variance exactly 0: rstd = 1 / sqrt(eps), x-hat = 0, out = resid + beta)."""
    x, res, t, ps, dout = _cln_inputs(xdt, B, L, C)
    if constant_row:
        x[0, L // 2, :] = 1.75
        x[B - 1, 0, :] = 0.0
    tt = t if cond else None
    gd = Guards()
    xg, rg, tg, dog = gd.op(x, name="x"), gd.op(res, name="resid"), gd.op(tt, name="time"), gd.op(dout, name="dout")
    pg = [gd.op(p, name=f"param{i}") if (cond or i in (1, 3)) else None for i, p in enumerate(ps)]
    pp = [p if (cond or i in (1, 3)) else None for i, p in enumerate(ps)]
    og, o16g = gd.out((B, L, C), F32, name="out"), gd.out((B, L, C), torch.bfloat16, name="out2")
    mg, sg = gd.out((B * L,), F32, name="mean"), gd.out((B * L,), F32, name="rstd")
    ops.cln_fwd(xg, rg, og, mg, sg, tg, pg[0], pg[1], pg[2], pg[3], B * L, L, C, 1e-5, out2=o16g)
    dxg = gd.out((B, L, C), xdt, name="dx")
    gr = gd.group([(C,)] * 5, F32, fills=[0.0] * 5, name="d_gw_w|d_gw_b|d_bw_w|d_bw_b|d_xbias")
    ops.cln_bwd(dog, xg, mg, sg, tg, pg[0], pg[1], dxg, gr[0], gr[1], gr[2], gr[3], B * L, L, C, d_xbias=gr[4])
    op_, o16p, mp, sp, dxp = nan_like((B, L, C), F32), nan_like((B, L, C), torch.bfloat16), nan_like((B * L,), F32), nan_like((B * L,), F32), \
        nan_like((B, L, C), xdt)
    grp = [torch.zeros(C, device=G.DEV) for _ in range(5)]
    ops.cln_fwd(x, res, op_, mp, sp, tt, pp[0], pp[1], pp[2], pp[3], B * L, L, C, 1e-5, out2=o16p)
    ops.cln_bwd(dout, x, mp, sp, tt, pp[0], pp[1], dxp, grp[0], grp[1], grp[2], grp[3], B * L, L, C, d_xbias=grp[4])
    sync()
    gd.check()
    for name, v in (("out", og), ("out2", o16g), ("mean", mg), ("rstd", sg), ("dx", dxg), ("grads", torch.cat(gr))):
        assert finite(v), name
    assert same(og, op_) and same(o16g, o16p) and same(mg, mp) and same(sg, sp) and same(dxg, dxp)
    assert same(o16g, og.to(torch.bfloat16))
    args = (x, res, t, ps[0], ps[1], ps[2], ps[3], None, dout, cond, xdt)
    ex_out, ex_dx = cln_model(*args, exact=True)
    mo_out, mo_dx = cln_model(*args)
    margin = MARGIN["cln"]
    r_out, row_o = kc.row_model_excess(og.reshape(-1, C), ex_out.reshape(-1, C), mo_out.reshape(-1, C), margin)
    r_dx, row_d = kc.row_model_excess(dxg.reshape(-1, C), ex_dx.reshape(-1, C), mo_dx.reshape(-1, C), margin)
    print(f"worst ratio cln cond {cond} {xdt} {(B, L, C)}: out {r_out * margin:.2f} x model (row {row_o}), dx {r_dx * margin:.2f} x model (row {row_d}); "
          f"margin {margin:.1f}")
    assert r_out <= 1.0, f"out row {row_o}: {r_out * margin:.2f} x the model's error; {kc.describe_worst(og, ex_out)}"
    assert r_dx <= 1.0, f"dx row {row_d}: {r_dx * margin:.2f} x the model's error; {kc.describe_worst(dxg, ex_dx)}"
    x64 = x.double().reshape(-1, C)
    mu64 = x64.mean(-1)
    var64 = ((x64 - mu64.unsqueeze(1)) ** 2).mean(-1)
    amean = x64.abs().mean(-1)
    assert bool(((mg.double() - mu64).abs() <= (C + 2) * kc.U32 * amean + 1e-37).all()), "mean: beyond the roundoff of a C-term fp32 sum"
    rs64 = 1.0 / torch.sqrt(var64 + 1e-5)
    assert G.rel(sg, rs64) < 1e-5
    if constant_row:
        for b, l in ((0, L // 2), (B - 1, 0)):
            r = b * L + l
            assert float(mg[r]) == float(x[b, l, 0]) and abs(float(sg[r]) / (1e-5 ** -0.5) - 1) < 1e-6
            beta = (float(t[b]) * ps[2].double() + ps[3].double()) if cond else ps[3].double()
            assert float((og[b, l].double() - (res[b, l].double() + beta)).abs().max()) < 1e-6, "constant row: out = resid + beta"
    # parameter gradients: atomics — the tolerances of test_cln_fwd_bwd
    xr = x.double().requires_grad_(True)
    p64 = [p.double().requires_grad_(True) for p in ps]
    mu = xr.mean(-1, keepdim=True)
    xh = (xr - mu) / torch.sqrt((xr * xr).mean(-1, keepdim=True) - mu * mu + 1e-5)
    g_ = t.double().view(B, 1, 1) * p64[0] + p64[1] if cond else p64[1]
    b_ = t.double().view(B, 1, 1) * p64[2] + p64[3] if cond else p64[3]
    (res.double() + g_ * xh + b_).backward(dout.double())
    if not constant_row:
        assert G.rel(gr[4], xr.grad.sum((0, 1))) < (2e-3 if xdt == F32 else 5e-2)
        for i in ([0, 1, 2, 3] if cond else [1, 3]):
            assert G.rel(gr[i], p64[i].grad) < 1e-4 and G.rel(gr[i], grp[i]) < 1e-5, i
    # mode 3: dx + per-block partial sums (the header sizes the scratch: scot_cln_bwd_workspace_bytes), finished into contiguous gradients
    nf = ops.cln_bwd_partial_floats(B * L, L, C, cond)
    if nf:
        part = gd.out((nf,), F32, name="mode-3 partial sums")
        dx3 = gd.out((B, L, C), xdt, name="dx (mode 3)")
        g3 = gd.group([(C,)] * 4, F32, fills=[0.25] * 4, name="mode-3 gradients")
        sel = g3 if cond else [None, g3[0], None, g3[1]]
        ops.cln_bwd(dog, xg, mg, sg, tg, pg[0], pg[1], dx3, None, None, None, None, B * L, L, C, sample_scale=None, mode=3, partial=part)
        ops.cln_bwd_finish(part, B * L, L, C, sel[0], sel[1], sel[2], sel[3])
        sync()
        gd.check()
        assert finite(dx3) and (same(dx3, dxg) or G.rel(dx3, dxg) < 1e-6)
        if not constant_row:
            for i in ([0, 1, 2, 3] if cond else [1, 3]):
                assert G.rel(sel[i] - 0.25, p64[i].grad) < 1e-4, i


@pytest.mark.parametrize("xdt", [F32, torch.bfloat16])
@pytest.mark.parametrize("B,L,C", [(3, 64, 96), (2, 9, 20), (2, 16, 768)])
def test_cln_constant_row(xdt, B, L, C):
    cln_guarded(True, xdt, B, L, C, constant_row=True)


# ================================================================================================================ fused layer tails
TAIL_CASES = [(kind, C, B, L) for kind in ("bf16", "f16") for C, B, L in ((48, 3, 200), (48, 2, 1024), (96, 3, 200), (96, 2, 1024), (192, 5, 72), (192, 2, 256))]
# C = 96 from 65536 rows on runs 128-row workgroups: M at that threshold, and M = 65664 with L % 128 != 0, where the forward runs 128-row
# workgroups and the backward 64-row ones with partial-sum matrices sized by scot_block_tail_workgroups
TAIL_CASES_128 = [(kind, 96, B, L) for kind in ("bf16", "f16") for B, L in ((64, 1024), (342, 192))]


def _tail_inputs(C, B, L, cond, hd):
    M, hid = B * L, 4 * C
    d = dict(a=G.rnd(M, C, seed=11).to(hd), x=G.rnd(M, C, seed=12),
             wo=G.rnd(C, C, scale=C ** -0.5, seed=13).to(hd), bo=G.rnd(C, seed=14, scale=0.2),
             w1=G.rnd(hid, C, scale=C ** -0.5, seed=2).to(hd), b1=G.rnd(hid, seed=3, scale=0.2),
             w2=G.rnd(C, hid, scale=hid ** -0.5, seed=4).to(hd), b2=G.rnd(C, seed=5, scale=0.2),
             wq=G.rnd(3 * C, C, scale=C ** -0.5, seed=41).to(hd), bq=G.rnd(3 * C, seed=42, scale=0.2),
             t=torch.rand(B, generator=torch.Generator().manual_seed(1)).to(G.DEV) if cond else None,
             s1=((torch.rand(B, generator=torch.Generator().manual_seed(2)) > 0.3).float() / 0.7).to(G.DEV),
             s2=((torch.rand(B, generator=torch.Generator().manual_seed(3)) > 0.3).float() / 0.7).to(G.DEV))
    for i, (sd, sc, one) in enumerate(((20, 0.3, 0), (21, 0.1, 1), (22, 0.1, 0), (23, 0.1, 0))):
        d[f"n1_{i}"] = (one + G.rnd(C, seed=sd, scale=sc)) if (cond or i in (1, 3)) else None
    for i, (sd, sc, one) in enumerate(((6, 0.3, 0), (7, 0.1, 1), (8, 0.1, 0), (9, 0.1, 0))):
        d[f"n2_{i}"] = (one + G.rnd(C, seed=sd, scale=sc)) if (cond or i in (1, 3)) else None
    return d


# the lean form (16-bit z, no 4C-wide saves) is a training form of C = 96 / 192
TAIL_FWD = [(*c, train, cond, nq, lean) for c in TAIL_CASES for train, cond, nq in ((True, True, True), (True, False, False), (False, True, False), (False, False, True))
            for lean in (False, True) if not (lean and (c[1] == 48 or not train))]
TAIL_FWD += [(*c, True, True, True, lean) for c in TAIL_CASES_128 for lean in (False, True)]


@pytest.mark.parametrize("kind,C,B,L,train,cond,next_qkv,lean", TAIL_FWD)
def test_block_tail_fwd_guarded(kind, C, B, L, train, cond, next_qkv, lean):
    block_tail_fwd_guarded(kind, C, B, L, train, cond, next_qkv, lean)


def block_tail_fwd_guarded(kind, C, B, L, train, cond, next_qkv, lean):
    """scot_block_tail_fwd (+ the next layer's q/k/v epilogue) at C = 48 / 96 / 192 with ragged L.  Its arithmetic is already pinned by
    torch.equal against the unfused chain; here every tensor it reads lies in NaN bands and every tensor it writes — h, h16, z, mean,
    rstd, gelu(u), gelu'(u), out, the 16-bit copies, qkv — is held to (a), (b) and (d).  lean: 16-bit z1 / z2 and no 4C-wide saves."""
    prev = ops.use(kind)
    try:
        hd = ops.half_dtype()
        M, hid = B * L, 4 * C
        d = _tail_inputs(C, B, L, cond, hd)
        gd = Guards()
        gi = {k: gd.op(v, name=k) for k, v in d.items()}
        zdt = hd if lean else F32
        shapes = dict(h=((M, C), F32), h16=((M, C), hd), out=((M, C), F32), out16=((M, C), hd))
        if train:
            shapes.update(z1=((M, C), zdt), m1=((M,), F32), r1=((M,), F32), z2=((M, C), zdt), m2=((M,), F32), r2=((M,), F32))
            if not lean:
                shapes.update(u=((M, hid), hd), gp=((M, hid), hd))
        if next_qkv:
            shapes["q"] = ((M, 3 * C), hd)
        og = {k: gd.out(sh, dt_, name=k) for k, (sh, dt_) in shapes.items()}
        op_ = {k: nan_like(sh, dt_) for k, (sh, dt_) in shapes.items()}

        def run(i, o):
            g = o.get
            return ops.block_tail_fwd((i["a"], i["wo"], i["bo"], i["x"], o["h"], o["h16"], g("z1"), g("m1"), g("r1"), i["n1_0"], i["n1_1"], i["n1_2"],
                                       i["n1_3"], i["s1"]),
                                      (i["w1"], i["b1"], i["w2"], i["b2"], o["out"], o["out16"], g("u"), g("gp"), g("z2"), g("m2"), g("r2"), i["n2_0"],
                                       i["n2_1"], i["n2_2"], i["n2_3"], i["s2"]),
                                      i["t"], M, L, C, hid, 1e-5, *((i["wq"], i["bq"], o["q"]) if next_qkv else ()), z16=lean)
        assert run(gi, og) and run(d, op_)
        sync()
        gd.check()
        for k in shapes:
            assert finite(og[k]), k
            assert same(og[k], op_[k]), (k, kc.describe_worst(og[k].reshape(M, -1), op_[k].double().reshape(M, -1), tile=64))
        return d, op_
    finally:
        ops.use(prev)


# samples of whole 64-row tiles: guarded launches of the backward.  C = 48 has the stored-gelu' form only.
TAIL_BWD = [(*c, cond, form) for c in [t for t in TAIL_CASES if t[3] % 64 == 0] + [(k, C, 3, 192) for k in ("bf16", "f16") for C in (48, 96, 192)]
            for cond in (True, False) for form in ("stored", "prologue", "lean") if not (c[1] == 48 and form != "stored")]
TAIL_BWD += [(*c, True, form) for c in TAIL_CASES_128 for form in ("stored", "lean")]
# ragged samples (L = 200, 72): NOT launches of the backward — the entry point must decline them (-3) and write nothing anywhere
TAIL_BWD_DECLINED = [(*c, True, "stored") for c in TAIL_CASES if c[3] % 64]


@pytest.mark.parametrize("kind,C,B,L,cond,form", TAIL_BWD)
def test_block_tail_bwd_guarded(kind, C, B, L, cond, form):
    block_tail_bwd_guarded(kind, C, B, L, cond, form)


@pytest.mark.parametrize("kind,C,B,L,cond,form", TAIL_BWD_DECLINED)
def test_block_tail_bwd_declines_ragged_samples(kind, C, B, L, cond, form):
    block_tail_bwd_guarded(kind, C, B, L, cond, form)


def block_tail_bwd_guarded(kind, C, B, L, cond, form, upstream=None):
    """scot_block_tail_bwd: stored gelu'(u) and atomics; with the qkv data-gradient prologue in place; the lean form (gelu'(u) recomputed from
    h16 / b1, no du, 16-bit z, per-workgroup partial sums finished by scot_partial_colsum).  The norms' eight parameter gradients lie
    back to back in one guarded buffer at the arena's alignment, the partial-sum matrices are guarded to the size the header gives
    ([scot_block_tail_workgroups, (4 | 2) x C rounded up to 64])."""
    prev = ops.use(kind)
    try:
        hd = ops.half_dtype()
        M, hid = B * L, 4 * C
        lean, prologue = form == "lean", form == "prologue"
        d = _tail_inputs(C, B, L, cond, hd)
        g0 = G.rnd(M, C, seed=31)
        if upstream is not None:      # the non-finite section below: its upstream gradient, the guarded launch only, its own checks
            g0 = upstream(g0)
            for s in ("s1", "s2"):        # both branches kept in every sample: a dropped one (sample scale 0) is a mask that closes the path
                d[s] = torch.full_like(d[s], 1.0 / 0.7)
        z2, z1 = G.rnd(M, C, seed=32), G.rnd(M, C, seed=33)
        st = lambda z: (z.mean(-1).contiguous(), (1.0 / torch.sqrt(z.var(-1, unbiased=False) + 1e-5)).contiguous())
        (m2, r2), (m1, r1) = st(z2), st(z1)
        if lean:
            z2, z1 = z2.to(hd), z1.to(hd)
        extra = dict(g0=g0, z2=z2, z1=z1, m2=m2, r2=r2, m1=m1, r1=r1, gp=G.rnd(M, hid, seed=34).to(hd), h16=G.rnd(M, C, seed=35).to(hd),
                     dqkv=G.rnd(M, 3 * C, seed=41).to(hd) if prologue else None,
                     wqkv=G.rnd(3 * C, C, scale=(3 * C) ** -0.5, seed=42).to(hd) if prologue else None)
        d.update(extra)
        gd = Guards()
        gi = {k: gd.op(v, name=k) for k, v in d.items()}
        shapes = dict(dz2=((M, C), hd), dz1=((M, C), hd), da=((M, C), hd))
        if not lean:
            shapes["du"] = ((M, hid), hd)
        Cp = (C + 63) // 64 * 64
        nwg = ops.tail_workgroups(M, L, C)
        ncol = (4 if cond else 2) * Cp

        def run(i, guarded):
            o = {k: (gd.out(sh, dt_, name=k) if guarded else nan_like(sh, dt_)) for k, (sh, dt_) in shapes.items()}
            if prologue:      # in place: g is read, added to and overwritten
                o["g"] = gd.out((M, C), F32, src=g0, name="g (in place)") if guarded else g0.clone()
                gin = o["g"]
            else:
                o["g"] = gd.out((M, C), F32, name="g_out") if guarded else nan_like((M, C), F32)
                gin = i["g0"]
            if guarded:
                flat2 = gd.group([(C,)] * 4, F32, fills=[0.0] * 4, name="norm-2 parameter gradients")
                flat1 = gd.group([(C,)] * 4, F32, fills=[0.0] * 4, name="norm-1 parameter gradients")
            else:
                flat2, flat1 = [torch.zeros(C, device=G.DEV) for _ in range(4)], [torch.zeros(C, device=G.DEV) for _ in range(4)]
            p2 = flat2 if cond else [None, flat2[1], None, flat2[3]]
            p1 = flat1 if cond else [None, flat1[1], None, flat1[3]]
            part2 = part1 = None
            if lean:
                part2 = gd.out((nwg, ncol), F32, name="partial2") if guarded else nan_like((nwg, ncol), F32)
                part1 = gd.out((nwg, ncol), F32, name="partial1") if guarded else nan_like((nwg, ncol), F32)
            o["ok"] = ops.block_tail_bwd(gin, o["g"], (i["z2"], i["m2"], i["r2"], i["n2_0"], i["n2_1"], i["s2"], None if lean else i["gp"], i["w1"], i["w2"],
                                                    o["dz2"], o.get("du"), p2[0], p2[1], p2[2], p2[3]),
                                      (i["z1"], i["m1"], i["r1"], i["n1_0"], i["n1_1"], i["s1"], i["wo"], o["dz1"], o["da"], p1[0], p1[1], p1[2], p1[3]),
                                      i["t"], M, L, C, hid, dqkv=i["dqkv"], wqkv=i["wqkv"], h16=i["h16"] if lean else None, b1=i["b1"] if lean else None,
                                      z16=lean, partial2=part2, partial1=part1)
            o["p2"], o["p1"], o["part2"], o["part1"] = p2, p1, part2, part1
            return o
        og = run(gi, True)
        if L % 64:      # samples that are not whole 64-row tiles are declined (-3): nothing may have been written anywhere
            sync()
            gd.check()
            assert not og["ok"] and all(bool(torch.isnan(og[k].float()).all()) for k in shapes)
            return
        if upstream is not None:
            assert og["ok"]
            sync()
            gd.check()
            og["inputs"] = d
            return og
        op_ = run(d, False)
        assert og["ok"] and op_["ok"]
        sync()
        gd.check()
        for k in list(shapes) + ["g"]:
            assert finite(og[k]), k
            assert same(og[k], op_[k]), (k, kc.describe_worst(og[k].reshape(M, -1), op_[k].double().reshape(M, -1), tile=64))
        if lean:      # the written part of the partial-sum rows: [nwg, (4 | 2) blocks of Cp] of which C columns each carry sums
            for part_g, part_p in ((og["part2"], op_["part2"]), (og["part1"], op_["part1"])):
                pgv, ppv = part_g.view(nwg, -1, Cp)[:, :, :C], part_p.view(nwg, -1, Cp)[:, :, :C]
                assert finite(pgv) and same(pgv, ppv)
        else:         # atomics: the tolerance of test_block_tail_bwd_fused
            for a_, b_ in zip(og["p2"] + og["p1"], op_["p2"] + op_["p1"]):
                if a_ is not None:
                    assert finite(a_) and G.rel(a_, b_) < 1e-4
    finally:
        ops.use(prev)


@pytest.mark.parametrize("train,cond", [(True, True), (False, False)])
@pytest.mark.parametrize("C,B,L", [(96, 3, 200), (96, 2, 1024), (192, 5, 72), (192, 2, 256)])
def test_fused_halves_fwd_guarded(C, B, L, train, cond):
    fused_halves_fwd_guarded(C, B, L, train, cond)


def fused_halves_fwd_guarded(C, B, L, train, cond):
    """scot_proj_cln_fwd and scot_mlp_block_fwd on their own (the two launches the block tail replaces): (a), (b), (d) on every tensor."""
    hd = ops.half_dtype()
    M, hid = B * L, 4 * C
    d = _tail_inputs(C, B, L, cond, hd)
    d["h"], d["h16"] = G.rnd(M, C, seed=50), G.rnd(M, C, seed=50).to(hd)
    gd = Guards()
    gi = {k: gd.op(v, name=k) for k, v in d.items()}
    shapes = dict(po=((M, C), F32), po16=((M, C), hd), mo=((M, C), F32), mo16=((M, C), hd))
    if train:
        shapes.update(z1=((M, C), F32), m1=((M,), F32), r1=((M,), F32), z2=((M, C), F32), m2=((M,), F32), r2=((M,), F32), u=((M, hid), hd), gp=((M, hid), hd))
    og = {k: gd.out(sh, dt_, name=k) for k, (sh, dt_) in shapes.items()}
    op_ = {k: nan_like(sh, dt_) for k, (sh, dt_) in shapes.items()}

    def run(i, o):
        g = o.get
        assert ops.proj_cln_fwd(i["a"], i["wo"], i["bo"], i["x"], o["po"], o["po16"], g("z1"), g("m1"), g("r1"), i["t"], i["n1_0"], i["n1_1"], i["n1_2"],
                                i["n1_3"], i["s1"], M, L, C, 1e-5)
        assert ops.mlp_block_fwd(i["h16"], i["h"], i["w1"], i["b1"], i["w2"], i["b2"], o["mo"], o["mo16"], g("u"), g("gp"), g("z2"), g("m2"), g("r2"), i["t"],
                                 i["n2_0"], i["n2_1"], i["n2_2"], i["n2_3"], i["s2"], M, L, C, hid, 1e-5)
    run(gi, og)
    run(d, op_)
    sync()
    gd.check()
    for k in shapes:
        assert finite(og[k]), k
        assert same(og[k], op_[k]), (k, kc.describe_worst(og[k].reshape(M, -1), op_[k].double().reshape(M, -1), tile=64))


@pytest.mark.parametrize("cond", [True, False])
@pytest.mark.parametrize("C,B,L", [(96, 3, 192), (96, 2, 1024), (192, 5, 64), (192, 2, 256)])
def test_fused_halves_bwd_guarded(C, B, L, cond):
    fused_halves_bwd_guarded(C, B, L, cond)


def fused_halves_bwd_guarded(C, B, L, cond, upstream=None):
    """scot_proj_cln_bwd and scot_mlp_block_bwd (out of place) on their own: data tensors (a), (b), (d); the norm-parameter gradients
    (atomics) back to back at the arena's alignment, at the tolerance of test_proj_cln_bwd_fused / test_mlp_block_bwd_fused."""
    hd = ops.half_dtype()
    M, hid = B * L, 4 * C
    d = _tail_inputs(C, B, L, cond, hd)
    z = G.rnd(M, C, seed=2, scale=1.5) + 0.3
    d.update(g=G.rnd(M, C, seed=1), z=z, mean=z.mean(-1).contiguous(), rstd=(1.0 / torch.sqrt(z.var(-1, unbiased=False) + 1e-5)).contiguous(),
             gp=G.rnd(M, hid, seed=3, scale=0.5).to(hd))
    if upstream is not None:
        d["g"] = upstream(d["g"])
        for s in ("s1", "s2"):        # both branches kept in every sample: a dropped one (sample scale 0) is a mask that closes the path
            d[s] = torch.full_like(d[s], 1.0 / 0.7)
    gd = Guards()
    gi = {k: gd.op(v, name=k) for k, v in d.items()}
    shapes = dict(pdz=((M, C), hd), pda=((M, C), hd), mdz=((M, C), hd), mdu=((M, hid), hd), mg=((M, C), F32))

    def run(i, guarded):
        o = {k: (gd.out(sh, dt_, name=k) if guarded else nan_like(sh, dt_)) for k, (sh, dt_) in shapes.items()}
        if guarded:
            fp, fm = gd.group([(C,)] * 4, F32, fills=[0.0] * 4, name="proj norm gradients"), gd.group([(C,)] * 4, F32, fills=[0.0] * 4, name="mlp norm gradients")
        else:
            fp, fm = [torch.zeros(C, device=G.DEV) for _ in range(4)], [torch.zeros(C, device=G.DEV) for _ in range(4)]
        sel = lambda f: f if cond else [None, f[1], None, f[3]]
        pp, pm = sel(fp), sel(fm)
        assert ops.proj_cln_bwd(i["g"], i["z"], i["mean"], i["rstd"], i["t"], i["n1_0"], i["n1_1"], i["s1"], i["wo"], o["pdz"], o["pda"], pp[0], pp[1], pp[2], pp[3],
                                M, L, C)
        assert ops.mlp_block_bwd(i["g"], o["mg"], i["z"], i["mean"], i["rstd"], i["t"], i["n2_0"], i["n2_1"], i["s2"], i["gp"], i["w1"], i["w2"], o["mdz"], o["mdu"],
                                 pm[0], pm[1], pm[2], pm[3], M, L, C, hid)
        o["grads"] = [t for t in pp + pm if t is not None]
        return o
    if upstream is not None:
        og = run(gi, True)
        sync()
        gd.check()
        og["inputs"] = d
        return og
    og, op_ = run(gi, True), run(d, False)
    sync()
    gd.check()
    for k in shapes:
        assert finite(og[k]), k
        assert same(og[k], op_[k]), (k, kc.describe_worst(og[k].reshape(M, -1), op_[k].double().reshape(M, -1), tile=64))
    for a_, b_ in zip(og["grads"], op_["grads"]):
        assert finite(a_) and G.rel(a_, b_) < 1e-4


# ===================================================================================================== data movement and small ops
def within(got, exact64, bound64, what):
    """every element within its own bound of the fp64 value (a NaN fails)"""
    bad = ~((got.double() - exact64).abs() <= bound64)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} element(s) beyond their bound, first at {bad.nonzero()[0].tolist()}"


SMALL_SIZES = [1000 * 4 + 3, 8192]          # one odd size (scalar tails), one multiple of every vector width


@pytest.mark.parametrize("n", SMALL_SIZES)
def test_flat_ops_guarded(n):
    flat_ops_guarded(n)


def flat_ops_guarded(n):
    """scot_scale_inplace(_dev), scot_segments_scale, scot_axpy_dev, scot_pow2_rescale, scot_dp_pack / unpack, scot_add, the cast form of
    scot_scale_residual: flat fp32 ranges the way the arenas hold them, in NaN bands.  A product or a conversion is ONE rounding, so
    the compare is exact against torch's fp32 arithmetic; fmaf(a, x, y) is held to one rounding of the fp64 value."""
    gd = Guards()
    x0 = G.rnd(n, seed=1)
    # x *= scale (host factor), non-finite results counted per wave
    xg, cnt = gd.out((n,), F32, src=x0, name="x"), gd.out((1,), torch.int32, fill=0, name="nonfinite")
    ops.scale_inplace(xg, 0.375, cnt)
    sync()
    gd.check()
    assert torch.equal(xg, x0 * 0.375) and int(cnt) == 0
    # the factor read from the device; one Inf makes one wave report
    sdev = gd.op(torch.tensor([4.0], device=G.DEV), name="scale_dev")
    xg[n // 2] = float("inf")
    ops.scale_inplace_dev(xg, sdev, cnt)
    sync()
    gd.check()
    ref = x0 * 0.375 * 4.0
    ref[n // 2] = float("inf")
    assert torch.equal(xg, ref) and int(cnt) == 1
    # a list of pieces: offsets multiples of 4, the last piece ends inside a 4-float group and at the range's very end
    segs = [(0, 64), (128, min(4096, n // 2 // 4 * 4)), (n - 61 - (n - 61) % 4, 61 + (n - 61) % 4)]
    chunks = gd.op(torch.tensor(segs, dtype=torch.int64, device=G.DEV), name="chunks")
    yg = gd.out((n,), F32, src=x0, name="x (segments)")
    cnt2 = gd.out((1,), torch.int32, fill=0, name="nonfinite")
    ops.segments_scale(yg, chunks, len(segs), sdev, cnt2)
    sync()
    gd.check()
    ref = x0.clone()
    for o, c in segs:
        ref[o:o + c] *= 4.0
    assert torch.equal(yg, ref) and int(cnt2) == 0
    ops.segments_scale(yg, chunks, len(segs), None)
    sync()
    gd.check()
    for o, c in segs:
        ref[o:o + c] = 0.0
    assert torch.equal(yg, ref)
    # dst += alpha * src, src cleared in the same pass
    d0, s0 = G.rnd(n, seed=2), G.rnd(n, seed=3)
    dg, sg, al = gd.out((n,), F32, src=d0, name="dst"), gd.out((n,), F32, src=s0, name="src"), gd.op(torch.tensor([0.3], device=G.DEV), name="alpha")
    ops.axpy_dev(dg, sg, al, clear_src=True)
    sync()
    gd.check()
    exact = d0.double() + float(al[0]) * s0.double()
    within(dg, exact, kc.U32 * exact.abs() + 1e-45, "axpy_dev (one fmaf)")
    assert bool((sg == 0).all())
    # power-of-two rescale: c = 2^k, k >= 0, with max|v| * c in [1/2, 1) (never scaled down), out2[1] = 1 / c
    for vmax in (3e-5, 0.5, 0.7, 1.0, 6.0):
        v = x0[:n].clone()
        v = v / v.abs().max() * vmax
        o2 = gd.out((2,), F32, name="pow2 out")
        ops.pow2_rescale(gd.op(v, name="v"), o2)
        sync()
        gd.check()
        m = float(v.abs().max())
        c, ci = float(o2[0]), float(o2[1])
        assert c >= 1.0 and math.log2(c) == int(math.log2(c)) and c * ci == 1.0
        assert (0.5 <= m * c < 1.0) if m < 1.0 else c == 1.0, (m, c)
    # the wire format of the data-parallel exchange: bfloat16 in both builds
    wire = gd.out((n,), torch.bfloat16, name="wire")
    srcg = gd.op(x0, name="src")
    ops.dp_pack(srcg, wire, 0.25)
    sync()
    gd.check()
    assert torch.equal(wire, (x0 * 0.25).to(torch.bfloat16))
    back = gd.out((n,), F32, name="unpacked")
    ops.dp_unpack(wire, back, 4.0)
    sync()
    gd.check()
    assert torch.equal(back, wire.float() * 4.0)
    # conversions and the periodic add
    hd = ops.half_dtype()
    c16, c32 = gd.out((n,), hd, name="cast to 16 bits"), gd.out((n,), F32, name="cast back")
    ops.cast(srcg, c16)
    ops.cast(c16, c32)
    sync()
    gd.check()
    assert torch.equal(c16, x0.to(hd)) and torch.equal(c32, x0.to(hd).float())
    per = next(q for q in (96, 61, 48, 13, 8, 7, 3, 1) if n % q == 0)
    pe = G.rnd(per, seed=4)
    ag = gd.out((n,), F32, name="a + periodic b")
    ops.add(srcg, gd.op(pe, name="b"), ag, period=per)
    sync()
    gd.check()
    assert torch.equal(ag, x0 + pe.repeat(n // per))


@pytest.mark.parametrize("rows,C", [(37, 24), (128, 96)])
def test_column_ops_guarded(rows, C):
    column_ops_guarded(rows, C)


def column_ops_guarded(rows, C):
    """scot_colscale_dev (C % 8 == 0), scot_mask_tokens(_bwd), scot_batch_sum, scot_partial_colsum(_batch), scot_colsum with a row stride."""
    gd = Guards()
    hd = ops.half_dtype()
    g, gamma, mul = G.rnd(rows, C, seed=1), G.rnd(C, seed=2, scale=1e-3), torch.tensor([64.0], device=G.DEV)
    gg, gag, mg = gd.op(g, name="g"), gd.op(gamma, name="gamma"), gd.op(mul, name="mul")
    exact = g.double() * gamma.double() * 64.0
    for odt in (F32, hd):      # two fp32 products, then one rounding to the result format
        out = gd.out((rows, C), odt, name=f"colscale {odt}")
        ops.colscale_dev(gg, gag, mg, out, rows, C)
        sync()
        gd.check()
        within(out, exact, ((kc.UNIT[odt] if odt != F32 else 0.0) + 2.5 * kc.U32) * exact.abs() + kc.SUBNORMAL_HALF_ULP[kc.UNIT[odt]], f"colscale_dev -> {odt}")
    # mask tokens, in place; backward: d_token += sum of masked rows (atomics over 64-row blocks), masked rows zeroed
    x0, tok = G.rnd(rows, C, seed=3), G.rnd(C, seed=4)
    mask = (torch.arange(rows) % 3 == 1).to(torch.uint8).to(G.DEV)
    mask[rows - 1] = 1
    xg, mk, tg = gd.out((rows, C), F32, src=x0, name="x"), gd.op(mask, name="mask"), gd.op(tok, name="token")
    ops.mask_tokens(xg, mk, tg, rows, C)
    sync()
    gd.check()
    assert torch.equal(xg, torch.where(mask.bool().unsqueeze(1), tok.unsqueeze(0), x0))
    g0, dt0 = G.rnd(rows, C, seed=5), G.rnd(C, seed=6)
    gg2, dtg = gd.out((rows, C), F32, src=g0, name="g"), gd.out((C,), F32, src=dt0, name="d_token")
    ops.mask_tokens_bwd(gg2, mk, dtg, rows, C)
    sync()
    gd.check()
    assert torch.equal(gg2, torch.where(mask.bool().unsqueeze(1), torch.zeros_like(g0), g0))
    msum, mabs = (g0.double() * mask.double().unsqueeze(1)).sum(0), (g0.double().abs() * mask.double().unsqueeze(1)).sum(0)
    within(dtg, dt0.double() + msum, (rows + 2) * kc.U32 * (mabs + dt0.double().abs()) + 1e-45, "mask_tokens_bwd")
    # column / batch sums: a sum of n terms in fp32 in any order is within n * u * sum|x| of the exact one
    for dt_ in (F32, hd):
        xs = G.rnd(rows, C, seed=7, dtype=dt_)
        o0 = G.rnd(C, seed=8)
        o = gd.out((C,), F32, src=o0, name="batch_sum out (+=)")
        ops.batch_sum(gd.op(xs, name="x"), o, rows, C)
        sync()
        gd.check()
        within(o, o0.double() + xs.double().sum(0), (rows + 1) * kc.U32 * (xs.double().abs().sum(0) + o0.double().abs()) + 1e-45, f"batch_sum {dt_}")
        o2, xs_s = gd.out((C,), F32, src=o0, name="colsum out"), gd.op(xs, pad=8, name="x (strided)")
        lib_rc = ops.L().scot_colsum(ops.ptr(xs_s), ops.dt(xs_s), None, 0, ops.ptr(o2), rows, C, C + 8, ops.stream())
        assert lib_rc == 0
        sync()
        gd.check()
        within(o2, o0.double() + xs.double().sum(0), (rows + 1) * kc.U32 * (xs.double().abs().sum(0) + o0.double().abs()) + 1e-45, f"colsum ld {dt_}")
    part, o0 = G.rnd(rows, C, seed=9), G.rnd(C, seed=10)
    pg, og = gd.op(part, name="partial"), gd.out((C,), F32, src=o0, name="out")
    ops.partial_colsum(pg, rows, C, og)
    items = []
    for j, (nb, nc) in enumerate(((rows, C), (5, 3 * C), (1, 8))):
        pj, oj = G.rnd(nb, nc, seed=20 + j), G.rnd(nc, seed=30 + j)
        items.append((gd.op(pj, name=f"partial{j}"), nb, nc, gd.out((nc,), F32, src=oj, name=f"out{j}"), pj, oj))
    ops.partial_colsum_batch([it[:4] for it in items])
    sync()
    gd.check()
    within(og, o0.double() + part.double().sum(0), (rows + 1) * kc.U32 * (part.double().abs().sum(0) + o0.double().abs()) + 1e-45, "partial_colsum")
    for pjg, nb, nc, ojg, pj, oj in items:
        within(ojg, oj.double() + pj.double().sum(0), (nb + 1) * kc.U32 * (pj.double().abs().sum(0) + oj.double().abs()) + 1e-45, "partial_colsum_batch")


@pytest.mark.parametrize("H,W,transpose", [(12, 12, True), (9, 13, False), (16, 16, False)])
def test_gather_guarded(H, W, transpose):
    gather_guarded(H, W, transpose)


def gather_guarded(H, W, transpose):
    """scot_gather_pairs / scot_gather_planes: out = fmaf(a[c], plane, b[c]) with the plane picked per (sample, channel); constant channels
    (src = -1), fixed planes (src <= -2, never transposed), the transposed read of square planes."""
    n, T, nsrc, B, C = 3, 4, 3, 4, 5
    gd = Guards()
    data = G.rnd(n, T, nsrc, H, W, seed=1)
    it = torch.tensor([[2, 0, 1, 2], [0, 1, 3, 2], [1, 3, 0, 3]], dtype=torch.int32, device=G.DEV)
    src = torch.tensor([1, -1, 0, 2, 1], dtype=torch.int32, device=G.DEV)
    a, b = G.rnd(C, seed=2), G.rnd(C, seed=3)
    dg, ig, sg, ag, bg = gd.op(data, name="data"), gd.op(it, name="it"), gd.op(src, name="src"), gd.op(a, name="a"), gd.op(b, name="b")
    pv, lab = gd.out((B, C, H, W), F32, name="pv"), gd.out((B, C, H, W), F32, name="lab")
    ops.gather_pairs(dg, ig, sg, ag, bg, pv, lab, T, nsrc, H, W, transpose)
    sync()
    gd.check()

    def ref(tidx_row, src_list, planes=None):
        out = torch.empty(B, C, H, W, dtype=torch.float64, device=G.DEV)
        mag = torch.empty_like(out)
        for bi in range(B):
            for c in range(C):
                sc = int(src_list[c])
                if sc == -1:
                    out[bi, c], mag[bi, c] = b[c].double(), b[c].double().abs()
                    continue
                P = data[int(it[0, bi]), int(tidx_row[bi]), sc].double() if sc >= 0 else planes[-2 - sc].double()
                if transpose and sc >= 0:
                    P = P.t()
                out[bi, c] = a[c].double() * P + b[c].double()
                mag[bi, c] = out[bi, c].abs()
        return out, mag
    for got, row in ((pv, it[1]), (lab, it[2])):
        r, m = ref(row, src)
        within(got, r, kc.U32 * m + 1e-45, "gather_pairs (one fmaf)")
    planes = G.rnd(2, H, W, seed=4)
    src2 = torch.tensor([1, -1, -2, 2, -3], dtype=torch.int32, device=G.DEV)
    out = gd.out((B, C, H, W), F32, name="out")
    ops.gather_planes(dg, gd.op(it[0].contiguous(), name="traj"), gd.op(it[1].contiguous(), name="tidx"), gd.op(src2, name="src"), ag, bg,
                      gd.op(planes, name="planes"), out, T, nsrc, H, W, transpose)
    sync()
    gd.check()
    r, m = ref(it[1], src2, planes)
    within(out, r, kc.U32 * m + 1e-45, "gather_planes (one fmaf)")


def test_data_movement_guarded():
    data_movement_guarded()


def data_movement_guarded():
    """scot_copy2d, scot_space_to_depth / depth_to_space, scot_patchify / unpatchify and scot_transpose_cast (rows, cols multiples of 8: its
    documented precondition) on guarded tensors: exact compares, matrices of the transposed arena back to back WITHOUT slack."""
    gd = Guards()
    hd = ops.half_dtype()
    B, H, W, C = 2, 5, 7, 12
    x = G.rnd(B, H, W, C)
    xg = gd.op(x, name="x")
    pad, crop = gd.out((B, 8, 8, C), F32, name="padded"), gd.out((B, 4, 6, C), F32, name="cropped")
    ops.copy2d(xg, pad, B, H, W, 8, 8, C)
    ops.copy2d(xg, crop, B, H, W, 4, 6, C)
    sync()
    gd.check()
    assert torch.equal(pad, torch.nn.functional.pad(x, (0, 0, 0, 1, 0, 3))) and torch.equal(crop, x[:, :4, :6])
    for (H, W), C in (((9, 5), 6), ((9, 5), 16), ((8, 8), 96)):      # 6: element-wise kernel; multiples of 8: eight channels per thread
        a, b = G.rnd(B, H, W, C), G.rnd(B, H, W, C, seed=1)
        H2, W2 = (H + 1) // 2, (W + 1) // 2
        co = gd.out((B, H2, W2, 4 * C), F32, name="coarse")
        ops.space_to_depth(gd.op(a, name="fine"), gd.op(b, name="fine2"), co, B, H, W, C, 0)
        s_ = torch.nn.functional.pad(a + b, (0, 0, 0, W % 2, 0, H % 2))
        fine = gd.out((B, H, W, C), F32, name="fine back")
        ops.depth_to_space(co, fine, B, H, W, H2, W2, C, 0)
        z = G.rnd(B, H2, W2, 4 * C, seed=2)
        fine2 = gd.out((B, H, W, C), F32, name="pixel shuffle")
        ops.depth_to_space(gd.op(z, name="z"), fine2, B, H, W, H2, W2, C, 1)
        sync()
        gd.check()
        assert torch.equal(co, torch.cat([s_[:, 0::2, 0::2], s_[:, 1::2, 0::2], s_[:, 0::2, 1::2], s_[:, 1::2, 1::2]], -1))
        assert torch.equal(fine, a + b)
        assert torch.equal(fine2, z.view(B, H2, W2, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H2, 2 * W2, C)[:, :H, :W])
    for H, W, Cc, cdt in ((18, 14, 3, F32), (16, 16, 3, F32), (64, 32, 5, hd)):
        p = 4
        img = G.rnd(B, Cc, H, W)
        gh, gw = (H + p - 1) // p, (W + p - 1) // p
        cols = gd.out((B * gh * gw, Cc * p * p), cdt, name="cols")
        imgg = gd.op(img, name="img")
        ops.patchify(imgg, cols, B, Cc, H, W, p)
        sync()
        gd.check()
        padded = torch.nn.functional.pad(img, (0, gw * p - W, 0, gh * p - H))
        assert torch.equal(cols, padded.view(B, Cc, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, Cc * p * p).to(cdt))
        if cdt == F32:
            bias = G.rnd(Cc, seed=1)
            back = gd.out((B, Cc, H, W), F32, name="unpatchified")
            ops.unpatchify(cols, gd.op(bias, name="bias"), back, B, Cc, H, W, gh, gw, p)
            sync()
            gd.check()
            assert torch.equal(back, img + bias.view(1, -1, 1, 1))
    mats = [(96, 288), (288, 96), (40, 72), (8, 8), (72, 200)]
    offs, cur = [], 0
    for r, c in mats:
        offs.append(cur)
        cur += (r * c + 63) // 64 * 64                    # the arena's alignment, nothing more
    cur = offs[-1] + mats[-1][0] * mats[-1][1]             # the last matrix ends the range
    arena = G.rnd(cur, seed=3)
    desc, tile = [], 0
    for (r, c), o in zip(mats, offs):
        desc.append((o, r, c, tile))
        tile += ((r + 63) // 64) * ((c + 63) // 64)
    wt = gd.out((cur,), hd, name="transposed copies")
    ops.transpose_cast(gd.op(arena, name="fp32 arena"), wt, gd.op(torch.tensor(desc, dtype=torch.int32, device=G.DEV), name="desc"), len(mats), tile)
    sync()
    gd.check()
    for (r, c), o in zip(mats, offs):
        assert torch.equal(wt[o:o + r * c].view(c, r), arena[o:o + r * c].view(r, c).to(hd).t()), (r, c)


# =============================================================== second ring: stencils, head and loss, position-bias MLP, spectral apply, optimizer
# csrc/misc.hip and csrc/optim.hip: entry points of every training step that the older suite judges by one global rel() on two to five shapes.
# Same four assertions as above.  The local bounds: a stencil is an inner product over its taps (gemm_excess, K = the taps + the bias); a sum
# that meets in atomicAdd is an inner product in ANY order over everything added; an elementwise formula is held to the number of fp32
# roundings on its path, counted and stated at the call site, each at most u times the magnitude sum of the expression it sits in.
class _build:
    """route the wrappers to one build of the library for the length of a case"""

    def __init__(self, kind):
        self.kind = kind

    def __enter__(self):
        self.prev = ops.use(self.kind)
        return ops.half_dtype()

    def __exit__(self, *exc):
        ops.use(self.prev)


def still_poison(t):
    """a result that a declined call must not touch: every element still the band's NaN, bit for bit"""
    idt, poison = kc._POISON[t.dtype]
    return bool((t.contiguous().view(idt) == poison).all())


def off_by_one(gd, t, name):
    """(guarded copy of t whose first element lies ONE element behind a 256-byte boundary, plain copy at the same misalignment): the view is
    taken from the inside of a guarded allocation, the element in front of it keeps the band's NaN (asserted by the caller's finite check:
    a loader that reads it poisons the result).  What the entry points do with it: the 16-byte vector loaders are not taken."""
    v = gd.out((t.numel() + 1,), t.dtype, name=name)
    v[1:].copy_(t.reshape(-1))
    p = torch.empty(t.numel() + 64, dtype=t.dtype, device=G.DEV)
    o = 1 + ((-p.data_ptr()) % 16) // p.element_size()
    p[o:o + t.numel()].copy_(t.reshape(-1))
    gv, pv = v[1:].view(t.shape), p[o:o + t.numel()].view(t.shape)
    assert gv.data_ptr() % 16 == t.element_size() and pv.data_ptr() % 16 == t.element_size()
    return gv, pv


# ------------------------------------------------------------------------------------------------------------------------ depthwise 7 x 7
def _dwconv64(x64, w64, b64, flip):
    """NHWC depthwise 7 x 7, padding 3; flip: the data gradient's form, conv(dy, flip(w))"""
    ww = w64.flip(-1, -2) if flip else w64
    return torch.nn.functional.conv2d(x64.permute(0, 3, 1, 2), ww, b64, padding=3, groups=x64.shape[-1]).permute(0, 2, 3, 1).contiguous()


def _dwconv_wgrad64(dy64, x64):
    B, H, W, C = x64.shape
    xp = torch.nn.functional.pad(x64, (0, 0, 3, 3, 3, 3))
    dw = torch.empty(C, 1, 7, 7, dtype=torch.float64, device=x64.device)
    for ki in range(7):
        for kj in range(7):
            dw[:, 0, ki, kj] = (dy64 * xp[:, ki:ki + H, kj:kj + W, :]).sum((0, 1, 2))
    return dw


# (B, H, W, C).  The loaders of dwconv7_tiled_kernel / dwconv7_wgrad_tiled_kernel: VEC = false for C % 4 != 0 (6 and 30: one channel block,
# C < 32; 33: a second block with ONE live channel), VEC = true for C % 4 == 0 (24, 40: not multiples of 32; 96).  H != W, H and W below the
# 7-wide stencil, H and W off the 8 x 8 tile.  Last: stage 0 of the timed model.
DW_SHAPES = [(2, 5, 9, 6), (1, 13, 6, 30), (2, 9, 11, 33), (2, 12, 20, 24), (3, 3, 4, 40), (2, 64, 64, 96)]
DW_IDS = lambda v: "x".join(str(i) for i in v) if isinstance(v, tuple) else None


@pytest.mark.parametrize("y16", [False, True], ids=["y_f32", "y_16"])
@pytest.mark.parametrize("x16", [False, True], ids=["x_f32", "x_16"])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("shape", DW_SHAPES, ids=DW_IDS)
def test_dwconv7_guarded(shape, kind, x16, y16):
    dwconv7_guarded(kind, *shape, x16, y16)


@pytest.mark.parametrize("x16", [False, True], ids=["x_f32", "x_16"])
@pytest.mark.parametrize("shape", [(2, 10, 7, 24), (1, 11, 8, 64)], ids=DW_IDS)
def test_dwconv7_guarded_misaligned_base_falls_back_from_vec(shape, x16):
    dwconv7_guarded("bf16", *shape, x16, False, misaligned=True)


def dwconv7_guarded(kind, B, H, W, C, x16, y16, misaligned=False):
    """scot_dwconv7, forward (bias) and flip = 1 (the data gradient, no bias), x_dt x y_dt in {fp32, 16 bit}; misaligned: C % 4 == 0 with a
    base one element off 16-byte alignment, the fallback from VEC.  (c): an inner product over 49 taps and the bias, K = 50, accumulated in
    fp32, one rounding to the result format.  gridDim.z = B, gridDim.y = ceil(C / 32): both above 1 in most shapes."""
    with _build(kind) as hd:
        xdt, ydt = (hd if x16 else F32), (hd if y16 else F32)
        gd = Guards()
        x, dy = G.rnd(B, H, W, C, dtype=xdt), G.rnd(B, H, W, C, seed=3, dtype=xdt)
        w, bias = G.rnd(C, 1, 7, 7, seed=1, scale=0.2), G.rnd(C, seed=2)
        wg, bg = gd.op(w, name="w"), gd.op(bias, name="bias")
        for flip, src, b_, b_g in ((False, x, bias, bg), (True, dy, None, None)):
            sg, sp = off_by_one(gd, src, "x (misaligned)") if misaligned else (gd.op(src, name="x"), src)
            yg, yp = gd.out((B, H, W, C), ydt, name="y"), nan_like((B, H, W, C), ydt)
            ops.dwconv7(sg, wg, b_g, yg, B, H, W, C, flip=flip)
            ops.dwconv7(sp, w, b_, yp, B, H, W, C, flip=flip)
            sync()
            gd.check()
            ref = _dwconv64(src.double(), w.double(), None if b_ is None else b_.double(), flip)
            mag = _dwconv64(src.double().abs(), w.double().abs(), None if b_ is None else b_.double().abs(), flip)
            assert finite(yg) and same(yg, yp), kc.describe_worst(yg, yp.double())
            assert_excess(f"dwconv7 {kind} {(B, H, W, C)} flip {flip} x {xdt} -> {ydt} misaligned {misaligned}", yg, ref, mag, 50, kc.U32)


@pytest.mark.parametrize("x16", [False, True], ids=["x_f32", "x_16"])
@pytest.mark.parametrize("g16", [False, True], ids=["dy_f32", "dy_16"])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("shape", DW_SHAPES, ids=DW_IDS)
def test_dwconv7_wgrad_guarded(shape, kind, g16, x16):
    dwconv7_wgrad_guarded(kind, *shape, g16, x16)


@pytest.mark.parametrize("g16,x16", [(False, False), (True, False)])
def test_dwconv7_wgrad_guarded_misaligned_base_falls_back_from_vec(g16, x16):
    dwconv7_wgrad_guarded("bf16", 2, 10, 7, 24, g16, x16, misaligned=True)


def dwconv7_wgrad_guarded(kind, B, H, W, C, g16, x16, misaligned=False):
    """scot_dwconv7_wgrad, all four dy_dt x x_dt pairs: dw += sum dy x (49 taps), db += sum dy, into an arena group that already holds values
    (the entry point accumulates).  Sums of B H W products that meet in atomicAdd: gemm_excess with K = B H W + 1 and the prior value in the
    magnitude; no bit-identity, rel() < 1e-5 stays beside the bound.  (The entry point fixes its tile groups at one: gridDim.z = 1 always.)"""
    with _build(kind) as hd:
        gd = Guards()
        x, dy = G.rnd(B, H, W, C, dtype=hd if x16 else F32), G.rnd(B, H, W, C, seed=3, dtype=hd if g16 else F32)
        dw0, db0 = G.rnd(C, 1, 7, 7, seed=4), G.rnd(C, seed=5)
        if misaligned:
            (xg, _), (dyg, _) = off_by_one(gd, x, "x (misaligned)"), off_by_one(gd, dy, "dy (misaligned)")
        else:
            xg, dyg = gd.op(x, name="x"), gd.op(dy, name="dy")
        dwg, dbg = gd.group([(C, 1, 7, 7), (C,)], F32, srcs=[dw0, db0], name="dw | db")
        ops.dwconv7_wgrad(dyg, xg, dwg, dbg, B, H, W, C)
        sync()
        gd.check()
        assert finite(dwg) and finite(dbg)
        n = B * H * W
        ref_w = dw0.double() + _dwconv_wgrad64(dy.double(), x.double())
        mag_w = dw0.double().abs() + _dwconv_wgrad64(dy.double().abs(), x.double().abs())
        ref_b, mag_b = db0.double() + dy.double().sum((0, 1, 2)), db0.double().abs() + dy.double().abs().sum((0, 1, 2))
        what = f"dwconv7_wgrad {kind} {(B, H, W, C)} dy 16-bit {g16} x 16-bit {x16} misaligned {misaligned}"
        assert_excess(what + " dw", dwg.view(C, 49), ref_w.view(C, 49), mag_w.view(C, 49), n + 1, kc.U32)
        assert_excess(what + " db", dbg, ref_b, mag_b, n + 1, kc.U32)
        assert G.rel(dwg, ref_w) < 1e-5 and G.rel(dbg, ref_b) < 1e-5


# ------------------------------------------------------------------------------------------------------------------------------ 5 x 5 mixup
def _conv5_wgrad64(dy64, x64):
    B, Cc, H, W = x64.shape
    xp = torch.nn.functional.pad(x64, (2, 2, 2, 2))
    dw = torch.empty(Cc, Cc, 5, 5, dtype=torch.float64, device=x64.device)
    for ki in range(5):
        for kj in range(5):
            dw[:, :, ki, kj] = torch.einsum("boyx,biyx->oi", dy64, xp[:, :, ki:ki + H, kj:kj + W])
    return dw


# (Cc, H, W, B): conv5_tiled_kernel<1..5> (133 and 131: two column tiles, the second one ragged and W % 4 != 0: the scalar column store;
# H % 8 != 0: ragged row tiles), conv5_kernel (per pixel) at Cc = 6 and 8
CONV5_SHAPES = [(1, 13, 133, 2), (2, 9, 10, 2), (3, 20, 131, 1), (4, 32, 32, 2), (4, 17, 136, 1), (5, 13, 10, 3), (6, 9, 9, 2), (8, 7, 13, 2)]


@pytest.mark.parametrize("shape", CONV5_SHAPES, ids=DW_IDS)
def test_conv5_guarded(shape):
    conv5_guarded(*shape)


@pytest.mark.parametrize("shape", [(4, 9, 14, 2), (2, 5, 133, 1)], ids=DW_IDS)
def test_conv5_guarded_misaligned_base_takes_the_per_pixel_kernel(shape):
    conv5_guarded(*shape, misaligned=True)


def conv5_guarded(Cc, H, W, B, misaligned=False):
    """scot_conv5 (transpose off and on) and scot_conv5_wgrad.  misaligned: `in` one element off 16-byte alignment at Cc <= 5, the alignment
    fallback to conv5_kernel.  (c): K = 25 Cc for the products, K = B H W + 1 for the weight gradient (atomics, prior values)."""
    gd = Guards()
    x, w, dy = G.rnd(B, Cc, H, W), G.rnd(Cc, Cc, 5, 5, seed=1, scale=0.2), G.rnd(B, Cc, H, W, seed=2)
    wg = gd.op(w, name="w")
    held = {}
    for transpose, src in ((False, x), (True, dy)):
        sg, sp = off_by_one(gd, src, "in (misaligned)") if misaligned else (gd.op(src, name="in"), src)
        held[transpose] = sg
        yg, yp = gd.out((B, Cc, H, W), F32, name="out"), nan_like((B, Cc, H, W), F32)
        ops.conv5(sg, wg, yg, B, Cc, H, W, transpose=transpose)
        ops.conv5(sp, w, yp, B, Cc, H, W, transpose=transpose)
        sync()
        gd.check()
        f = torch.nn.functional.conv_transpose2d if transpose else torch.nn.functional.conv2d
        ref, mag = f(src.double(), w.double(), None, padding=2), f(src.double().abs(), w.double().abs(), None, padding=2)
        assert finite(yg) and same(yg, yp), kc.describe_worst(yg, yp.double())
        assert_excess(f"conv5 Cc {Cc} {(B, H, W)} transpose {transpose} misaligned {misaligned}", yg, ref, mag, 25 * Cc, kc.U32)
    dw0 = G.rnd(Cc, Cc, 5, 5, seed=3)
    dwg = gd.out((Cc, Cc, 5, 5), F32, src=dw0, name="dw")
    ops.conv5_wgrad(held[True], held[False], dwg, B, Cc, H, W)
    sync()
    gd.check()
    ref = dw0.double() + _conv5_wgrad64(dy.double(), x.double())
    mag = dw0.double().abs() + _conv5_wgrad64(dy.double().abs(), x.double().abs())
    assert finite(dwg)
    assert_excess(f"conv5_wgrad Cc {Cc} {(B, H, W)}", dwg.view(Cc * Cc, 25), ref.view(Cc * Cc, 25), mag.view(Cc * Cc, 25), B * H * W + 1, kc.U32)
    assert G.rel(dwg, ref) < 1e-5


def test_conv5_declines_leave_the_result_untouched():
    conv5_declines()


def conv5_declines():
    """Cc = 9 (scot_conv5, scot_conv5_wgrad) and a W whose two LDS strips exceed 64 KB (scot_conv5_wgrad: Cc (12 W + 32) floats; Cc = 8,
    W = 172) return -3 on the host, before any launch, and leave the result's NaN intact."""
    gd = Guards()
    lib = ops.L()
    for Cc, H, W, fwd in ((9, 4, 8, True), (8, 4, 172, False)):
        x, w, dy = G.rnd(1, Cc, H, W), G.rnd(Cc, Cc, 5, 5, seed=1), G.rnd(1, Cc, H, W, seed=2)
        xg, wg, dyg = gd.op(x, name="in"), gd.op(w, name="w"), gd.op(dy, name="dout")
        out, dw = gd.out((1, Cc, H, W), F32, name="out"), gd.out((Cc, Cc, 5, 5), F32, name="dw")
        if fwd:
            for tr in (0, 1):
                assert lib.scot_conv5(ops.ptr(xg), ops.ptr(wg), ops.ptr(out), 1, Cc, H, W, tr, ops.stream()) == -3
        assert lib.scot_conv5_wgrad(ops.ptr(dyg), ops.ptr(xg), ops.ptr(dw), 1, Cc, H, W, ops.stream()) == -3
        sync()
        gd.check()
        assert still_poison(out) and still_poison(dw)


# ------------------------------------------------------------------------------------------------------- head, loss, input-gradient helpers
EPS_LOSS = float(torch.tensor(1e-10, dtype=F32))       # the 1e-10f of loss_finish_kernel / loss_bwd_kernel as the kernels see it

# p x mask x HW is the full matrix; the residual, the channel groups (a -1 channel: in no group) and `normalized` alternate over it so
# that both settings of each meet both p and every mask form.  HW: 256 = one workgroup per plane with idle lanes of the last stride,
# 4097 = two workgroups, the second with ONE element, 16384 = the timed problem: four workgroups per plane meeting in atomicAdd.
HEAD_CASES = [(p, mk, HW, (i + j + k) % 2 == 0, [0, 0, -1, 1] if (i + k) % 2 == 0 else ([0, 0, 0, 0] if j == 0 else [1, 0, 2, -1]), (j + k) % 2 == 0)
              for i, p in enumerate((1, 2)) for j, mk in enumerate(("none", "plane", "pixel")) for k, HW in enumerate((256, 4097, 16384))]


@pytest.mark.parametrize("p,mk,HW,resid,goc,normalized", HEAD_CASES,
                         ids=[f"p{c[0]}-mask_{c[1]}-HW{c[2]}-resid{int(c[3])}-groups{'_'.join(str(g) for g in c[4])}-norm{int(c[5])}" for c in HEAD_CASES])
def test_head_loss_guarded(p, mk, HW, resid, goc, normalized):
    head_loss_guarded(p, mk, HW, resid, goc, normalized)


def head_loss_guarded(p, mk, HW, resid, goc, normalized, B=2):
    """scot_head_finalize (labels given, and NULL: inference), scot_loss_finish, scot_loss_bwd (dloss NULL and a device scalar),
    scot_zero_masked, scot_add_channels (dst_ch == Cc and > Cc).  mk: "none", "plane" (mask_full = 0: one byte per (b, c)), "pixel"
    (mask_full = 1: one byte per element)."""
    u = kc.U32
    Cc, pv_ch = len(goc), len(goc) + 1
    ngroups = max(goc) + 1
    gd = Guards()
    pred0, lab, pv = G.rnd(B, Cc, HW), G.rnd(B, Cc, HW, seed=1), G.rnd(B, pv_ch, HW, seed=2)
    full = mk == "pixel"
    if mk == "plane":
        m = torch.zeros(B, Cc, dtype=torch.uint8, device=G.DEV)
        m[:, -1] = 1
        m[0, 0] = 1
        mexp = m.bool().view(B, Cc, 1).expand(B, Cc, HW)
    elif full:
        m = (G.rnd(B, Cc, HW, seed=3) > 0.3).to(torch.uint8)
        m[B - 1, Cc - 1, HW - 1] = 1          # the last element of all: the tail of the last workgroup
        mexp = m.bool()
    else:
        m, mexp = None, torch.zeros(B, Cc, HW, dtype=torch.bool, device=G.DEV)
    gt = torch.tensor(goc, dtype=torch.int32, device=G.DEV)
    cnt = torch.tensor([B * goc.count(g) * HW for g in range(ngroups)], dtype=F32, device=G.DEV)
    sums0 = G.rnd(2 * ngroups, seed=4).abs()
    labg, pvg, mg, gg, cg = gd.op(lab, name="labels"), gd.op(pv, name="pixel_values"), gd.op(m, name="mask"), gd.op(gt, name="groups"), gd.op(cnt, name="counts")
    predg, predp = gd.out((B, Cc, HW), F32, src=pred0, name="pred"), pred0.clone()
    sumsg, sumsp = gd.out((2 * ngroups,), F32, src=sums0, name="sums"), sums0.clone()
    ops.head_finalize(predg, pvg if resid else None, pv_ch, labg, mg, full, gg, sumsg, B, Cc, HW, p)
    ops.head_finalize(predp, pv if resid else None, pv_ch, lab, m, full, gt, sumsp, B, Cc, HW, p)
    sync()
    gd.check()
    # pred: v = pred + pv is ONE fp32 addition (no residual: unchanged), a masked element IS the label
    v64 = pred0.double() + (pv[:, :Cc].double() if resid else 0.0)
    ev = torch.where(mexp, 0.0, u * v64.abs() if resid else torch.zeros_like(v64))
    vq = torch.where(mexp, lab.double(), v64)
    assert finite(predg) and same(predg, predp)
    within(predg, vq, ev, f"head_finalize pred (p {p}, mask {mk}, HW {HW}, residual {resid})")
    assert torch.equal(predg[mexp], lab[mexp])
    # sums[g] += sum over the group of |d|^p and |y|^p, d = fl(v - y): partial sums per lane, wave, workgroup, then atomicAdd — any order, K =
    # the group's element count + the prior value.  The roundings INSIDE a term are not relative to it (v ~ y: d is small, v's rounding is
    # not), so they enter as an absolute term: d carries ev (the rounding of v) and u |d| (its own); |d| passes that on; d d squares it
    # ((2 |d| + ed) ed) and rounds once more; y y rounds once.  A masked element has d = 0 exactly.
    lab64 = lab.double()
    d = vq - lab64
    ed = torch.where(mexp, 0.0, ev + u * (d.abs() + ev))
    if p == 1:
        t1, e1, t2, e2 = d.abs(), ed, lab64.abs(), torch.zeros_like(d)
    else:
        t1, e1, t2, e2 = d * d, (2 * d.abs() + ed) * ed + u * (d.abs() + ed) ** 2, lab64 * lab64, u * lab64 * lab64
    assert finite(sumsg)
    for g in range(ngroups):
        sel = [c for c in range(Cc) if goc[c] == g]
        for k, (t_, e_) in enumerate(((t1, e1), (t2, e2))):
            s0 = sums0[2 * g + k].double()
            assert_excess(f"head_finalize sums[{g}][{k}] (p {p}, mask {mk}, HW {HW})", sumsg[2 * g + k].view(1), (s0 + t_[:, sel].sum()).view(1),
                          (s0.abs() + t_[:, sel].sum()).view(1), B * len(sel) * HW + 1, u, abs_extra=e_[:, sel].sum().view(1))
    # labels = NULL (inference): pred is updated, sums are not touched
    p2, s2 = gd.out((B, Cc, HW), F32, src=pred0, name="pred (inference)"), gd.out((2 * ngroups,), F32, src=sums0, name="sums (inference)")
    ops.head_finalize(p2, pvg, pv_ch, None, None, False, gg, s2, B, Cc, HW, p)
    sync()
    gd.check()
    vi = pred0.double() + pv[:, :Cc].double()
    within(p2, vi, u * vi.abs(), "head_finalize without labels")
    assert torch.equal(s2, sums0)
    # loss = (1 / G) sum_g num_g [/ (den_g + 1e-10)] from the sums as stored (operands of this entry point).  Roundings on a term's path:
    # num = s / c (1); normalized: den = s / c (1), + 1e-10f (1), the quotient (1); then at most G additions and the division by G (1):
    # G + 2, normalized G + 5.  Every term is positive: the magnitude sum is the loss itself.
    s64, c64 = sumsg.double(), cnt.double()
    terms = s64[0::2] / c64
    if normalized:
        terms = terms / (s64[1::2] / c64 + EPS_LOSS)
    loss64 = (terms.sum() / ngroups).view(1)
    lossg = gd.out((1,), F32, name="loss")
    ops.loss_finish(sumsg, cg, ngroups, normalized, lossg)
    sync()
    gd.check()
    within(lossg, loss64, (ngroups + (5 if normalized else 2)) * u * 1.01 * loss64, f"loss_finish (G {ngroups}, normalized {normalized})")
    # dpred = dloss * coef * (sign(diff) | 2 diff), exact zeros where masked or in no group.  Roundings of coef = dloss / (G c) [/ (s / c + 1e-10f)]:
    # the product G c (1), the quotient (1), normalized: s / c (1), + 1e-10f (1), the second quotient (1) -> 2, normalized 5.  p = 2 adds
    # diff = fl(pred - y) (1) and the product with coef (1; the factor 2 is exact) -> 4, normalized 7.  p = 1: the sign of an fp32
    # subtraction is the sign of the exact difference — equality, not a tolerance.
    goc_e = gt.long().view(1, Cc, 1).expand(B, Cc, HW)
    live = (goc_e >= 0) & ~mexp
    gsafe = goc_e.clamp_min(0)
    coef = 1.0 / (ngroups * c64[gsafe])
    if normalized:
        coef = coef / (s64[1::2][gsafe] / c64[gsafe] + EPS_LOSS)
    diff = predg.double() - lab64
    nround = (2 if p == 1 else 4) + (3 if normalized else 0)
    sums_plain = sumsg.clone()
    for dl in (None, torch.tensor([0.37], device=G.DEV)):
        dpg, dpp = gd.out((B, Cc, HW), F32, name="dpred"), nan_like((B, Cc, HW), F32)
        ops.loss_bwd(predg, labg, mg, full, gg, sumsg, cg, ngroups, normalized, gd.op(dl, name="dloss"), dpg, B, Cc, HW, p)
        ops.loss_bwd(predp, lab, m, full, gt, sums_plain, cnt, ngroups, normalized, dl, dpp, B, Cc, HW, p)
        sync()
        gd.check()
        gl = 1.0 if dl is None else float(dl[0])
        exact = torch.where(live, gl * coef * (torch.sign(diff) if p == 1 else 2.0 * diff), 0.0)
        assert finite(dpg) and same(dpg, dpp)
        within(dpg, exact, nround * u * 1.01 * exact.abs() + 1e-45, f"loss_bwd (p {p}, mask {mk}, HW {HW}, normalized {normalized}, dloss {dl is not None})")
        assert bool((dpg[~live] == 0).all())
        if p == 1:
            assert torch.equal(torch.sign(dpg).double(), torch.where(live, torch.sign(diff), 0.0))
    # the head's part of the input gradient: exact data movement / one fp32 addition, against torch
    g0 = G.rnd(B, Cc, HW, seed=6)
    if m is not None:
        zg = gd.out((B, Cc, HW), F32, src=g0, name="g (zero_masked)")
        ops.zero_masked(zg, mg, full, B, Cc, HW)
        sync()
        gd.check()
        assert torch.equal(zg, torch.where(mexp, torch.zeros_like(g0), g0))
    srcg = gd.op(g0, name="src")
    for dst_ch in (Cc, Cc + 2):
        d0 = G.rnd(B, dst_ch, HW, seed=7)
        dg = gd.out((B, dst_ch, HW), F32, src=d0, name=f"dst ({dst_ch} channels)")
        ops.add_channels(dg, dst_ch, srcg, B, Cc, HW)
        sync()
        gd.check()
        want = d0.clone()
        want[:, :Cc] += g0
        assert torch.equal(dg, want)


@pytest.mark.parametrize("B,Cc,HW", [(3, 4, 1000), (2, 5, 4097), (1, 3, 255), (4, 1, 16384)])
def test_nchw_channel_sum_guarded(B, Cc, HW):
    nchw_channel_sum_guarded(B, Cc, HW)


def nchw_channel_sum_guarded(B, Cc, HW):
    """scot_nchw_channel_sum: out[c] += sum over (b, i) — one workgroup per plane, B atomics per channel: any order, K = B HW + 1"""
    gd = Guards()
    x, o0 = G.rnd(B, Cc, HW), G.rnd(Cc, seed=1)
    og = gd.out((Cc,), F32, src=o0, name="out")
    ops.nchw_channel_sum(gd.op(x, name="x"), og, B, Cc, HW)
    sync()
    gd.check()
    assert finite(og)
    ref, mag = o0.double() + x.double().sum((0, 2)), o0.double().abs() + x.double().abs().sum((0, 2))
    assert_excess(f"nchw_channel_sum {(B, Cc, HW)}", og, ref, mag, B * HW + 1, kc.U32)
    assert G.rel(og, ref) < 1e-5


# ------------------------------------------------------------------------------------------------------------------------ position-bias MLP
# table[h][e] = 16 sigmoid(z[e][h]), z = relu(coords W0^T + b0) W2^T (512 hidden units).  z is a product and gets the product bound.  The
# sigmoid is `16.0f / (1.0f + __expf(-z))`, and __expf is v_exp_f32 of the argument times log2(e) (clang's __clang_hip_math.h).  Neither the
# ROCm headers nor any document shipped with them states an accuracy for that instruction, so the table gets no derived bound: it is held
# per row (= per head) to a ROUNDING MODEL, the way attention and the conditional layer norm are — the fp64 restatement with a rounding
# where the kernel rounds (the scaled argument, the exponential, 1 + e, the quotient; for the whole chain also the three operations of
# a hidden unit and the stored z), MARGIN = twice the worst per-row ratio of that model evaluated in fp32 (two summation orders) to the
# model evaluated in fp64, measured on the CPU by --measure-margins.  The table is judged twice: against the fp64 sigmoid of the kernel's
# OWN stored z (an operand of that last step: isolates the exponential and the division), and against the exact chain with a model into
# which nothing of the kernel enters.
LOG2E_F32 = float(torch.tensor(1.4426950408889634, dtype=F32))         # 0x1.715476p+0
CPB_LAYERS = [(16, 3), (16, 6), (8, 12), (4, 24), (7, 2)]              # (window, heads) of test_cpb_batched_layers
# worst ratios measured over CPB_LAYERS + (16, 24) with the inputs of the cases below and with a six times wider z: the last step 1.11 (the
# model's exponential is correctly rounded, fp32 libm's is not quite), the whole chain 6.81 (the model rounds z once, fp32 arithmetic sums
# 512 products)
MARGIN.update({"cpb_sigmoid": 2 * 1.11, "cpb_chain": 2 * 6.81})


def _r32(x):
    return x.to(F32).to(x.dtype)


def _cpb_coords(ws):
    r = torch.arange(-(ws - 1), ws, dtype=F32)
    tab = torch.stack(torch.meshgrid(r, r, indexing="ij"), -1) / max(ws - 1, 1) * 8
    return (torch.sign(tab) * torch.log2(tab.abs() + 1) / 3).reshape(-1, 2).to(G.DEV)


def cpb_sigmoid_model(z, dtype=torch.float64, exact=False):
    """16 / (1 + exp2(-z log2 e)) evaluated in `dtype` with a rounding to fp32 where cpb_fwd_kernel rounds; exact: 16 sigmoid(z) in fp64"""
    if exact:
        return 16.0 * torch.sigmoid(z.double())
    zz = z.to(dtype)
    e = _r32(torch.exp2(_r32(-zz * LOG2E_F32)))
    return _r32(16.0 / _r32(1.0 + e)).double()


def cpb_chain_model(coords, w0, b0, w2, dtype=torch.float64, reverse=False, exact=False):
    """(z [TS, heads], table [heads, TS]) of the whole chain in `dtype`; roundings: the two products and two additions of a hidden unit, the
    stored z, then cpb_sigmoid_model's"""
    r = (lambda v: v) if exact else _r32
    c, w0_, b0_, w2_ = (t.to(torch.float64 if exact else dtype) for t in (coords, w0, b0, w2))
    hid = torch.relu(r(r(r(c[:, 0:1] * w0_[:, 0]) + r(c[:, 1:2] * w0_[:, 1])) + b0_))
    z = r(hid.flip(-1) @ w2_.flip(-1).t() if reverse else hid @ w2_.t())
    return z.double(), cpb_sigmoid_model(z, dtype, exact).t()


def _cpb_fwd64(coords, w0, b0, w2):
    """(pre, e_pre, hid, z) in fp64.  e_pre: a hidden unit is w0y cy + w0x cx + b0 in at most three roundings (fewer where the compiler
    contracts), each at most u times the magnitude sum; relu passes the deviation on unchanged."""
    c = coords.double()
    pre = c @ w0.double().t() + b0.double()
    e_pre = 3 * kc.U32 * (c.abs() @ w0.double().abs().t() + b0.double().abs())
    hid = torch.relu(pre)
    return pre, e_pre, hid, hid @ w2.double().t()


def _cpb_check_fwd(what, coords, w0, b0, w2, zg, tg):
    """zg [TS, heads], tg [heads, TS] as the kernels stored them"""
    _, e_pre, hid, z64 = _cpb_fwd64(coords, w0, b0, w2)
    aw2 = w2.double().abs().t()
    assert finite(zg) and finite(tg)
    # z: 512 products accumulated in fp32 (per lane, wave, workgroup: any order); the hidden units enter with their deviation as E |W2|
    assert_excess(what + " z", zg, z64, (hid + e_pre) @ aw2, 512, kc.U32, abs_extra=e_pre @ aw2)
    ex1, m1 = cpb_sigmoid_model(zg, exact=True).t(), cpb_sigmoid_model(zg).t()
    r1, row1 = kc.row_model_excess(tg, ex1, m1, MARGIN["cpb_sigmoid"])
    ex2, m2 = cpb_chain_model(coords, w0, b0, w2, exact=True)[1], cpb_chain_model(coords, w0, b0, w2)[1]
    r2, row2 = kc.row_model_excess(tg, ex2, m2, MARGIN["cpb_chain"])
    print(f"worst ratio {what} table: sigmoid of the stored z {r1 * MARGIN['cpb_sigmoid']:.2f} (head {row1}), whole chain {r2 * MARGIN['cpb_chain']:.2f} (head {row2})")
    assert r1 <= 1.0, f"{what}: table head {row1} is {r1:.2f} x its allowance against the sigmoid of the stored z; {kc.describe_worst(tg, ex1)}"
    assert r2 <= 1.0, f"{what}: table head {row2} is {r2:.2f} x its allowance against the exact chain; {kc.describe_worst(tg, ex2)}"


def _cpb_check_bwd(what, coords, w0, b0, w2, z, dtab, prior, got):
    """prior / got: (dw0 [512, 2], db0 [512], dw2 [heads, 512]) before and after `+=`.  z [TS, heads] is the STORED operand, dtab [heads, TS].
    dz = dtable 16 s (1 - s), s = 1 / (1 + exp2(-z log2 e)): the deviation of the kernel's dz from the fp64 value takes the exponential as
    a 1-ulp (= 2 u) instruction, the assumption D_CDF above makes for the same v_exp_f32 — it enters the bound only through this
    second-order operand term.  e = exp(-z): its argument's rounding and the fp32 log2 e move it by 2 |z| u, the instruction by 2 u; s:
    the sum and the quotient, one rounding each, and the error of e times de s / s = (1 - s); 1 - s: the error of s and one rounding;
    dz: two more products.  dh = dz W2 (`heads` terms); dpre = dh where pre > 0 — where the fp64 pre lies within e_pre of zero the kernel may
    decide either way, and the whole of |dh| is allowed there.  Then sums over the TS table entries + the prior value, in any order."""
    u = kc.U32
    TS, heads = z.shape
    pre, e_pre, hid, _ = _cpb_fwd64(coords, w0, b0, w2)
    z64, dt64, w264, c = z.double(), dtab.double().t(), w2.double(), coords.double()
    sg, om = torch.sigmoid(z64), torch.sigmoid(-z64)
    d_sg = sg * ((2 * z64.abs() + 2) * u * om + 2 * u)
    d_om = d_sg + u * om
    dz = dt64 * 16.0 * sg * om
    e_dz = 1.01 * (dt64.abs() * 16.0 * (d_sg * om + sg * d_om) + 2 * u * dz.abs())
    dh = dz @ w264
    e_dh = 1.01 * (heads * u * (dz.abs() @ w264.abs()) + e_dz @ w264.abs())
    livep = pre > 0
    dpre = torch.where(livep, dh, 0.0)
    e_dpre = torch.where(livep, e_dh, 0.0) + torch.where(pre.abs() <= e_pre, dh.abs() + e_dh, 0.0)
    refs = (dpre.t() @ c, dpre.sum(0), dz.t() @ hid)
    mags = (dpre.abs().t() @ c.abs(), dpre.abs().sum(0), dz.abs().t() @ (hid + e_pre))
    extras = (e_dpre.t() @ c.abs(), e_dpre.sum(0), e_dz.t() @ (hid + e_pre) + dz.abs().t() @ e_pre)
    for name, g0, g1, ref, mag, ex in zip(("dw0", "db0", "dw2"), prior, got, refs, mags, extras):
        assert finite(g1)
        assert_excess(f"{what} {name}", g1, g0.double() + ref, g0.double().abs() + mag, TS + 1, u, abs_extra=ex)
        assert G.rel(g1.double() - g0.double(), ref) < 1e-4


@pytest.mark.parametrize("ws,heads", [(16, 3), (8, 12), (4, 24), (7, 2)])
def test_cpb_guarded(ws, heads):
    cpb_guarded(ws, heads)


def cpb_guarded(ws, heads):
    """scot_cpb_fwd / scot_cpb_bwd (one layer): deterministic by design (a workgroup owns its hidden units' gradients, no atomics) — two
    launches and the plain launch agree bit for bit"""
    TS = (2 * ws - 1) ** 2
    gd = Guards()
    coords = _cpb_coords(ws)
    w0, b0, w2 = G.rnd(512, 2), G.rnd(512, seed=1, scale=0.5), G.rnd(heads, 512, seed=2, scale=0.05)
    cg, w0g, b0g, w2g = gd.op(coords, name="coords"), gd.op(w0, name="w0"), gd.op(b0, name="b0"), gd.op(w2, name="w2")
    tg, zg = gd.out((heads, TS), F32, name="table"), gd.out((TS, heads), F32, name="z")
    tp, zp = nan_like((heads, TS), F32), nan_like((TS, heads), F32)
    ops.cpb_fwd(cg, w0g, b0g, w2g, tg, zg, ws, heads)
    ops.cpb_fwd(coords, w0, b0, w2, tp, zp, ws, heads)
    sync()
    gd.check()
    assert same(tg, tp) and same(zg, zp)
    _cpb_check_fwd(f"cpb_fwd ws {ws} heads {heads}", coords, w0, b0, w2, zg, tg)
    dtab = G.rnd(heads, TS, seed=3)
    dtg = gd.op(dtab, name="dtable")
    prior = (G.rnd(512, 2, seed=4, scale=0.1), G.rnd(512, seed=5, scale=0.1), G.rnd(heads, 512, seed=6, scale=0.1))
    runs = []
    for k in range(2):
        gs = gd.group([(512, 2), (512,), (heads, 512)], F32, srcs=list(prior), name=f"dw0 | db0 | dw2 (launch {k})")
        ops.cpb_bwd(cg, w0g, b0g, w2g, zg, dtg, gs[0], gs[1], gs[2], ws, heads)
        runs.append(gs)
    plain = [t.clone() for t in prior]
    ops.cpb_bwd(coords, w0, b0, w2, zp, dtab, plain[0], plain[1], plain[2], ws, heads)
    sync()
    gd.check()
    for a, b, c in zip(runs[0], runs[1], plain):
        assert same(a, b) and same(a, c)
    _cpb_check_bwd(f"cpb_bwd ws {ws} heads {heads}", coords, w0, b0, w2, zg, dtab, prior, runs[0])


@pytest.mark.parametrize("first", [0, 1, 3])
def test_cpb_batched_guarded(first):
    cpb_batched_guarded(CPB_LAYERS, first)


def cpb_batched_guarded(layers, first, upstream=None):
    """scot_cpb_fwd_batched over all layers, scot_cpb_bwd_batched over layers first.. of the list.  Parameters and gradients lie the way the
    arenas hold them: a layer's w0 | b0 | w2 back to back, a neighbour that is no CPB parameter (100 floats + padding to 64) behind every
    layer.  The gradients hold prior values; layers in front of `first`, every neighbour and all padding must come back bit-unchanged."""
    gd = Guards()
    wss = sorted({w for w, _ in layers})
    coff, cur, cl = {}, 0, []
    for ws in wss:
        coff[ws] = cur
        cl.append(_cpb_coords(ws).reshape(-1))
        cur += cl[-1].numel()
    coords = torch.cat(cl)
    shapes, srcs_p, srcs_g = [], [], []
    for li, (ws, heads) in enumerate(layers):
        shapes += [(1536 + heads * 512,), (100,)]
        lp = torch.cat([G.rnd(1024, seed=10 * li), G.rnd(512, seed=10 * li + 1, scale=0.5), G.rnd(heads * 512, seed=10 * li + 2, scale=0.05)])
        srcs_p += [lp, G.rnd(100, seed=10 * li + 3)]
        srcs_g += [G.rnd(1536 + heads * 512, seed=10 * li + 4, scale=0.1), G.rnd(100, seed=10 * li + 5)]
    pviews = gd.group(shapes, F32, srcs=srcs_p, name="parameter arena")
    offs = [(v.data_ptr() - pviews[0].data_ptr()) // 4 for v in pviews]
    span = offs[-1] + 100
    desc, toff = [], 0
    for li, (ws, heads) in enumerate(layers):
        o = offs[2 * li]
        desc += [o, o + 1024, o + 1536, coff[ws], ws, heads, toff, toff]
        toff += heads * (2 * ws - 1) ** 2
    d = torch.tensor(desc, dtype=torch.int32, device=G.DEV)
    dtab = G.rnd(toff, seed=5)
    if upstream is not None:      # the non-finite section below: its upstream gradient, one guarded launch, its own checks
        dtab = upstream(dtab, desc)
    cg, dg, dtg = gd.op(coords, name="coords"), gd.op(d, name="desc"), gd.op(dtab, name="dtables")
    tabg, zg = gd.out((toff,), F32, name="tables"), gd.out((toff,), F32, name="z")
    pplain = torch.zeros(span, device=G.DEV)
    for v, o in zip(srcs_p, offs):
        pplain[o:o + v.numel()] = v
    tabp, zp = nan_like((toff,), F32), nan_like((toff,), F32)
    max_ws, max_heads = max(w for w, _ in layers), max(h for _, h in layers)
    ops.cpb_fwd_batched(pviews[0], dg, len(layers), max_ws, cg, tabg, zg)
    ops.cpb_fwd_batched(pplain, d, len(layers), max_ws, coords, tabp, zp)
    sync()
    gd.check()
    assert same(tabg, tabp) and same(zg, zp)
    if upstream is not None:
        gv = gd.group(shapes, F32, srcs=srcs_g, name="gradient arena")
        ops.cpb_bwd_batched(pviews[0], dg, first, len(layers) - first, max_ws, max_heads, cg, zg, dtg, gv[0])
        sync()
        gd.check()
        return gv, srcs_p, coords, coff
    runs = []
    for k in range(2):
        gv = gd.group(shapes, F32, srcs=srcs_g, name=f"gradient arena (launch {k})")
        assert [(v.data_ptr() - gv[0].data_ptr()) // 4 for v in gv] == offs
        ops.cpb_bwd_batched(pviews[0], dg, first, len(layers) - first, max_ws, max_heads, cg, zg, dtg, gv[0])
        runs.append(gv)
    gplain = torch.zeros(span, device=G.DEV)
    for v, o in zip(srcs_g, offs):
        gplain[o:o + v.numel()] = v
    ops.cpb_bwd_batched(pplain, d, first, len(layers) - first, max_ws, max_heads, coords, zp, dtab, gplain)
    sync()
    gd.check()
    for i, (a, b, o) in enumerate(zip(runs[0], runs[1], offs)):
        assert same(a, b) and same(a, gplain[o:o + a.numel()]), f"arena member {i}"
        if i % 2 == 1 or i // 2 < first:
            assert same(a, srcs_g[i]), f"arena member {i} lies outside the range and was changed"
    for li, (ws, heads) in enumerate(layers):
        ts = (2 * ws - 1) ** 2
        lp, t0 = srcs_p[2 * li], desc[8 * li + 6]
        w0, b0, w2 = lp[:1024].view(512, 2), lp[1024:1536], lp[1536:].view(heads, 512)
        cs = coords[coff[ws]:coff[ws] + 2 * ts].view(ts, 2)
        zl, tl = zg[t0:t0 + heads * ts].view(ts, heads), tabg[t0:t0 + heads * ts].view(heads, ts)
        _cpb_check_fwd(f"cpb_fwd_batched layer {li} (ws {ws}, heads {heads})", cs, w0, b0, w2, zl, tl)
        if li >= first:
            g0, g1 = srcs_g[2 * li], runs[0][2 * li]
            cut = lambda g: (g[:1024].view(512, 2), g[1024:1536], g[1536:].view(heads, 512))
            _cpb_check_bwd(f"cpb_bwd_batched first {first} layer {li} (ws {ws}, heads {heads})", cs, w0, b0, w2, zl, dtab[t0:t0 + heads * ts].view(heads, ts),
                           cut(g0), cut(g1))


# ---------------------------------------------------------------------------------------------------------------------------- spectral apply
@pytest.mark.parametrize("nimg", [1, 5])
@pytest.mark.parametrize("s,t", [(32, 64), (64, 32), (24, 40), (128, 128)])
def test_spectral_apply_guarded(s, t, nimg):
    spectral_apply_guarded(s, t, nimg)


def spectral_apply_guarded(s, t, nimg):
    """scot_spectral_apply at kernel level: Y[b] = Pr U_r[b] - Pi U_i[b], one chain of 2 s fused multiply-adds per element: K = 2 s.
    (24, 40): t off the 16-row / 16-column tile, clamped rows of Pr / Pi and clamped columns of U."""
    gd = Guards()
    U, Pr, Pi = G.rnd(nimg * s, 2 * t), G.rnd(t, s, seed=1, scale=s ** -0.5), G.rnd(t, s, seed=2, scale=s ** -0.5)
    Yg, Yp = gd.out((nimg, t, t), F32, name="Y"), nan_like((nimg, t, t), F32)
    ops.spectral_apply(gd.op(U, name="U"), gd.op(Pr, name="Pr"), gd.op(Pi, name="Pi"), Yg, nimg, s, t)
    ops.spectral_apply(U, Pr, Pi, Yp, nimg, s, t)
    sync()
    gd.check()
    U3 = U.double().view(nimg, s, 2 * t)
    ref = Pr.double() @ U3[:, :, :t] - Pi.double() @ U3[:, :, t:]
    mag = Pr.double().abs() @ U3[:, :, :t].abs() + Pi.double().abs() @ U3[:, :, t:].abs()
    assert finite(Yg) and same(Yg, Yp)
    assert_excess(f"spectral_apply s {s} t {t} nimg {nimg}", Yg, ref, mag, 2 * s, kc.U32)


def test_spectral_apply_declines_s_513():
    spectral_apply_declines()


def spectral_apply_declines():
    """s = 513: the two 16 x s strips of Pr and Pi exceed 64 KB of LDS — -3 from the host, nothing launched, Y untouched"""
    gd = Guards()
    s, t = 513, 16
    U, Pr, Pi = G.rnd(s, 2 * t), G.rnd(t, s, seed=1), G.rnd(t, s, seed=2)
    Y = gd.out((1, t, t), F32, name="Y")
    rc = ops.L().scot_spectral_apply(ops.ptr(gd.op(U, name="U")), ops.ptr(gd.op(Pr, name="Pr")), ops.ptr(gd.op(Pi, name="Pi")), ops.ptr(Y), 1, s, t, ops.stream())
    sync()
    gd.check()
    assert rc == -3 and still_poison(Y)


# --------------------------------------------------------------------------------------------------------------------------------- optimizer
def _opt_group(gd, sizes, dtype, srcs=None, fills=None, name="arena"):
    """an arena group with a 4096-element band (the default band is 128 rows of the widest member: 128 x 8 M elements here)"""
    vs, g = kc.guarded_group([(s,) for s in sizes], dtype, G.DEV, srcs=srcs, fills=fills, band=kc.MIN_BAND, name=name)
    gd.items.append(g)
    return vs


# (size, parameter group) of the arena's members; sizes are multiples of 8 and not of 64, so every member is followed by padding
OPT_SMALL = [(1000, 0), (24, 1), (2056, 0), (40, 2)]
OPT_LARGE = [(1000, 0), (8400000, 1), (24, 2), (4104, 0)]            # > 4096 x 256 x 8 elements: the grid-stride loops of both kernels iterate


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("members", [OPT_SMALL, OPT_LARGE], ids=["small", "grid_stride"])
def test_optimizer_guarded(members, kind):
    optimizer_guarded(kind, members)


def optimizer_guarded(kind, members):
    """scot_grad_sqnorm, scot_clip_coef, scot_adamw_step, scot_optim_finish on the device.  params, grads, exp_avg, exp_avg_sq and the 16-bit
    copy are arena groups whose padding is marked 255 in map8 and holds the poison NaN — in the gradient too, the state the lazy
    zero-grad leaves.  Three steps: clipped (coefficient below 1, Adam's clock read from the device), unclipped (clip = NULL, the host's
    step number), and a step whose norm is not finite, which must change nothing."""
    import ctypes
    u = kc.U32
    with _build(kind) as hd:
        lib, st = ops.L(), ops.stream()
        gd = Guards()
        sizes = [s for s, _ in members]
        lr_, wd_ = [1e-2, 3e-3, 1e-3], [0.1, 0.0, 0.05]
        lr32, wd32 = (ctypes.c_float * 3)(*lr_), (ctypes.c_float * 3)(*wd_)
        beta1, beta2, eps = (float(torch.tensor(v, dtype=F32)) for v in (0.9, 0.999, 1e-8))
        p0 = [G.rnd(s, seed=i) for i, s in enumerate(sizes)]
        g0 = [G.rnd(s, seed=10 + i, scale=0.5) for i, s in enumerate(sizes)]
        m0 = [G.rnd(s, seed=20 + i, scale=0.1) for i, s in enumerate(sizes)]
        v0 = [G.rnd(s, seed=30 + i, scale=0.3) ** 2 for i, s in enumerate(sizes)]
        P, Gr, M, V = (_opt_group(gd, sizes, F32, srcs=src, name=nm) for src, nm in ((p0, "params"), (g0, "grads"), (m0, "exp_avg"), (v0, "exp_avg_sq")))
        S = _opt_group(gd, sizes, hd, fills=[-7.0] * len(sizes), name="shadow16")
        offs = [(v.data_ptr() - P[0].data_ptr()) // 4 for v in P]
        for grp in (Gr, M, V):
            assert [(v.data_ptr() - grp[0].data_ptr()) // 4 for v in grp] == offs
        assert [(v.data_ptr() - S[0].data_ptr()) // 2 for v in S] == offs
        n = offs[-1] + sizes[-1]
        assert n % 8 == 0 and all(o % 8 == 0 for o in offs)
        map8 = torch.full((n // 8,), 255, dtype=torch.uint8)
        for (s, gi), o in zip(members, offs):
            map8[o // 8:(o + s) // 8] = gi
        mapg = gd.op(map8.to(G.DEV), name="map8")
        nblk = int(lib.scot_optim_blocks(n))
        partial, clip = gd.out((nblk,), F32, name="partial"), gd.out((3,), F32, src=torch.tensor([1.0, 0.0, 0.0], device=G.DEV), name="clip")
        state = gd.out((2,), torch.int32, src=torch.tensor([4, 0], dtype=torch.int32, device=G.DEV), name="step_state")
        nlive = sum(sizes)

        def norm_step(max_norm):
            assert lib.scot_grad_sqnorm(ops.ptr(Gr[0]), ops.ptr(mapg), n, ops.ptr(partial), st) == 0
            assert lib.scot_clip_coef(ops.ptr(partial), nblk, max_norm, ops.ptr(clip), st) == 0
            sync()
            gd.check()

        def adam(clip_t, state_t, host_step):
            assert lib.scot_adamw_step(ops.ptr(P[0]), ops.ptr(Gr[0]), ops.ptr(M[0]), ops.ptr(V[0]), ops.ptr(mapg), n, ctypes.cast(lr32, ctypes.c_void_p),
                                       ctypes.cast(wd32, ctypes.c_void_p), 3, beta1, beta2, eps, host_step, ops.ptr(clip_t), ops.ptr(state_t), ops.ptr(S[0]), st) == 0
            sync()
            gd.check()          # the padding of all five arrays, bit for bit

        def check_update(before, cc, t, what):
            """p, m, v per element against the update of csrc/optim.hip's header comment in fp64 on the operands as the kernel receives them
            (lr, wd, the betas and eps as fp32 values, cc = the stored clip coefficient).  Roundings, each at most u times the magnitude sum
            of the expression it sits in:
              m' = m + (g cc - m)(1 - b1): g cc, the difference, 1 - b1, the product, the sum — 5, on |m| + (|g cc| + |m|)(1 - b1);
              v' = b2 v + (1 - b2)(g cc)^2: g cc (twice), 1 - b2, two products, b2 v, the sum — 7, all terms positive: on v';
              p' = p (1 - lr wd) - (lr / bc1) m' / (sqrt(v') rsqrt_bc2 + eps): lr wd, the difference, the product — 3 on |p (1 - lr wd)|;
                   denominator: half of v's 7, the square root, rsqrt_bc2 (rounded to fp32), the product, + eps — 7.5, positive terms;
                   bc1 (rounded to fp32), lr / bc1, the quotient, the product — 4; together 11.5, taken as 12, on |update|; the carried
                   error of m' times step / denominator; the final subtraction — 1 on |p'|."""
            bc1, rbc2 = 1.0 - beta1 ** t, 1.0 / math.sqrt(1.0 - beta2 ** t)
            for i, ((s, gi), o) in enumerate(zip(members, offs)):
                pb, mb, vb = (x[i].double() for x in before)
                lr, wd = float(lr32[gi]), float(wd32[gi])
                gj = Gr[i].double() * cc
                m1 = mb + (gj - mb) * (1.0 - beta1)
                e_m = 5 * u * 1.01 * (mb.abs() + (gj.abs() + mb.abs()) * (1.0 - beta1))
                v1 = beta2 * vb + (1.0 - beta2) * gj * gj
                den = torch.sqrt(v1) * rbc2 + eps
                step = lr / bc1
                upd = step * m1 / den
                pd = pb * (1.0 - lr * wd)
                p1 = pd - upd
                e_p = 1.01 * (u * p1.abs() + 3 * u * pd.abs() + 12 * u * upd.abs() + step * e_m / den)
                assert finite(P[i]) and finite(M[i]) and finite(V[i])
                within(M[i], m1, e_m + 1e-45, f"{what}: exp_avg of member {i}")
                within(V[i], v1, 7 * u * 1.01 * v1 + 1e-45, f"{what}: exp_avg_sq of member {i}")
                within(P[i], p1, e_p + 1e-45, f"{what}: params of member {i}")
                assert torch.equal(S[i], P[i].to(hd)), f"{what}: shadow16 of member {i} is not the round-to-nearest conversion of the stored p"

        snapshot = lambda: tuple([t.clone() for t in grp] for grp in (P, M, V))
        # ---- step 1: clipped.  norm^2 = sum of nlive squares: per-workgroup partial sums in fp32 in any order (K = n), their sum in fp64, the
        # square root halves the relative error, the conversion to fp32 rounds once
        g64 = torch.cat([g.double() for g in Gr])
        exact_norm = g64.norm()
        norm_step(float(exact_norm) * 0.5)
        c = clip.double()
        assert finite(clip) and float(c[2]) == 0.0
        within(clip[1:2], exact_norm.view(1), ((nlive + 1) * u / 2 * 1.01 + u) * exact_norm.view(1), "gradient norm (any order, K = n)")
        print(f"gradient norm: relative error {abs(float(c[1]) - float(exact_norm)) / float(exact_norm):.2e} of an allowance of {(nlive + 1) * u / 2 + u:.2e}")
        # coef = max_norm / (norm + 1e-6f) from the STORED norm: the sum and the quotient, 2 roundings
        mx = float(torch.tensor(float(exact_norm) * 0.5, dtype=F32))
        coef = mx / (float(c[1]) + float(torch.tensor(1e-6, dtype=F32)))
        assert coef < 1.0 and abs(float(c[0]) - coef) <= 2 * u * 1.01 * coef
        before = snapshot()
        adam(clip, state, 99)                   # the host's step number is ignored when the device clock is given: t = step_state[0] + 1 = 5
        check_update(before, float(c[0]), 5, "clipped step")
        assert lib.scot_optim_finish(ops.ptr(state), ops.ptr(clip), None, 2.0, 0.5, 0, float(2 ** 20), st) == 0
        sync()
        gd.check()
        assert state.tolist() == [5, 0]
        # ---- step 2: clip = NULL, step_state = NULL: no clipping, no skip, the bias corrections of the host's step number
        before = snapshot()
        adam(None, None, 3)
        check_update(before, 1.0, 3, "unclipped step")
        # ---- step 3: one Inf in a live gradient: the norm is not finite, and the step changes NOTHING — p, m, v, the 16-bit copy, bit for bit
        Gr[1][sizes[1] // 2] = float("inf")
        norm_step(1.0)
        assert float(clip[2]) == 1.0
        before, sbefore = snapshot(), [t.clone() for t in S]
        adam(clip, state, 1)
        for grp, old in zip((P, M, V), before):
            for a, b in zip(grp, old):
                assert same(a, b)
        for a, b in zip(S, sbefore):
            assert same(a, b)
        assert lib.scot_optim_finish(ops.ptr(state), ops.ptr(clip), None, 2.0, 0.5, 0, float(2 ** 20), st) == 0
        sync()
        gd.check()
        assert state.tolist() == [5, 1]


# (size, parameter group): 64-float spacing as in the flat arenas; 1003 is no multiple of 8, so its last 8-element chunk is shared with
# five floats of (zero) alignment padding; the 64 floats behind the first member are a gradient-carrying non-parameter region (the key-bias
# slot of the fused qkv bias: map8 == 255)
VERDICT_MEMBERS = [(1000, 0), (1003, 1), (24, 2), (4104, 0)]
VERDICT_FREE = (1024, 64)       # (offset, size) of the non-parameter region
INF = float("inf")


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_optimizer_verdicts(kind):
    optimizer_verdicts(kind)


def optimizer_verdicts(kind):
    """What makes scot_clip_coef flag a step (clip[2] = 1), through the four launches of FusedAdamW.step on one guarded arena laid out like
    the product's (64-float spacing, ZERO padding, map8 from the rule of poseidon_amd.optim.group_map8).  A flagged step changes nothing
    but the skip counter and halves the scale; a step that is not flagged equals the clean step bit for bit (no atomics in these kernels):
      NaN only, -Inf only, +Inf only, in a live chunk                                  -> skipped
      the same in the last, partly padded chunk of the 1003-element member             -> skipped
      all three in a region mapped 255 (not a parameter)                               -> applied, bit-identical to the clean step
      one FINITE element of 2e19, whose square overflows fp32                          -> skipped (pinned; include/scot_hip.h says so)
      one finite element of 1e19 (square 1e38)                                         -> applied: the boundary is the square's overflow"""
    import ctypes
    with _build(kind) as hd:
        lib, st = ops.L(), ops.stream()
        gd = Guards()
        offs, o = [], 0
        for s, _ in VERDICT_MEMBERS:
            offs.append(o)
            o = (o + s + 63) // 64 * 64
            if o == VERDICT_FREE[0]:
                o += VERDICT_FREE[1]
        n = o
        assert n % 8 == 0 and offs[1] == VERDICT_FREE[0] + VERDICT_FREE[1]
        live = torch.zeros(n, dtype=torch.bool)
        map8 = torch.full((n // 8,), 255, dtype=torch.uint8)
        for (s, gi), o in zip(VERDICT_MEMBERS, offs):
            live[o:o + s] = True
            map8[o // 8:(o + s + 7) // 8] = gi
        live = live.to(G.DEV)
        lr32, wd32 = (ctypes.c_float * 3)(1e-2, 3e-3, 1e-3), (ctypes.c_float * 3)(0.1, 0.0, 0.05)
        init = [G.rnd(n, seed=1) * live, G.rnd(n, seed=2, scale=0.5) * live, G.rnd(n, seed=3, scale=0.1) * live, (G.rnd(n, seed=4, scale=0.3) * live) ** 2]
        init[1][VERDICT_FREE[0]:VERDICT_FREE[0] + VERDICT_FREE[1]] = 0.25       # the key-bias slot carries a gradient
        P, Gr, M, V = (gd.out((n,), F32, src=t, name=nm) for t, nm in zip(init, ("params", "grads", "exp_avg", "exp_avg_sq")))
        S = gd.out((n,), hd, src=init[0].to(hd), name="shadow16")
        mapg = gd.op(map8.to(G.DEV), name="map8")
        nblk = int(lib.scot_optim_blocks(n))
        partial, clip = gd.out((nblk,), F32, name="partial"), gd.out((3,), F32, fill=0.0, name="clip")
        state, scale = gd.out((2,), torch.int32, fill=0, name="step_state"), gd.out((4,), F32, fill=0.0, name="scale_state")
        max_norm = 0.5 * float((init[1].double() * live).norm())       # (clipping on: the coefficient comes from the same norm)

        def step(plants):
            """from the same initial state every time -> (flagged, [p, m, v, shadow16, clip, step_state, scale_state])"""
            for t, src in zip((P, Gr, M, V), init):
                t.copy_(src)
            S.copy_(init[0].to(hd))
            for i, v in plants:
                Gr[i] = v
            clip.copy_(torch.tensor([1.0, 0.0, 0.0]))
            state.copy_(torch.tensor([4, 7], dtype=torch.int32))
            scale.copy_(torch.tensor([1024.0, 1.0 / 1024.0, 0.0, 0.0]))
            assert lib.scot_grad_sqnorm(ops.ptr(Gr), ops.ptr(mapg), n, ops.ptr(partial), st) == 0
            assert lib.scot_clip_coef(ops.ptr(partial), nblk, max_norm, ops.ptr(clip), st) == 0
            assert lib.scot_adamw_step(ops.ptr(P), ops.ptr(Gr), ops.ptr(M), ops.ptr(V), ops.ptr(mapg), n, ctypes.cast(lr32, ctypes.c_void_p),
                                       ctypes.cast(wd32, ctypes.c_void_p), 3, 0.9, 0.999, 1e-8, 1, ops.ptr(clip), ops.ptr(state), ops.ptr(S), st) == 0
            assert lib.scot_optim_finish(ops.ptr(state), ops.ptr(clip), ops.ptr(scale), 2.0, 0.5, 2000, float(2 ** 30), st) == 0
            sync()
            gd.check()
            assert float(clip[2]) in (0.0, 1.0)
            return float(clip[2]) == 1.0, [t.clone() for t in (P, M, V, S, clip, state, scale)]

        def skipped(res, what):
            flagged, (p, m, v, s16, c, stt, sc) = res
            assert flagged, f"{what}: not flagged"
            for nm, a, b in zip(("params", "exp_avg", "exp_avg_sq"), (p, m, v), (init[0], init[2], init[3])):
                assert same(a, b), f"{what}: a flagged step changed {nm}"
            assert same(s16, init[0].to(hd)), f"{what}: a flagged step changed the 16-bit copy"
            assert stt.tolist() == [4, 8] and sc.tolist() == [512.0, 1.0 / 512.0, 0.0, 0.0], (what, stt.tolist(), sc.tolist())

        clean = step([])
        assert not clean[0] and clean[1][5].tolist() == [5, 7] and clean[1][6].tolist() == [1024.0, 1.0 / 1024.0, 1.0, 0.0]
        assert finite(clean[1][0]) and not same(clean[1][0], init[0]) and 0.0 < float(clean[1][4][0]) < 1.0
        mid, last = offs[0] + 500, offs[1] + VERDICT_MEMBERS[1][0] - 1           # (the last live element of the partly padded chunk)
        assert last % 8 == 2 and int(map8[last // 8]) == 1 and not bool(live[last + 1])
        for name, v in (("NaN", NAN), ("-Inf", -INF), ("+Inf", INF)):
            skipped(step([(mid, v)]), f"{name} only, in a live chunk")
            skipped(step([(last, v)]), f"{name} only, in the last, partly padded chunk of a {VERDICT_MEMBERS[1][0]}-element tensor")
        f0 = VERDICT_FREE[0]
        free = step([(f0, NAN), (f0 + 9, INF), (f0 + VERDICT_FREE[1] - 1, -INF)])
        assert not free[0], "a non-finite value outside every parameter (map8 == 255) flagged the step"
        for nm, a, b in zip(("params", "exp_avg", "exp_avg_sq", "shadow16", "clip", "step_state", "scale_state"), free[1], clean[1]):
            assert same(a, b), f"non-finite values where map8 == 255 changed {nm}"
        skipped(step([(mid, 2e19)]), "a finite gradient whose square overflows fp32 (2e19)")
        skipped(step([(last, -2e19)]), "a finite gradient whose square overflows fp32 (-2e19)")
        edge = step([(mid, 1e19)])
        assert not edge[0] and float(edge[1][4][1]) >= float(torch.tensor(1e19, dtype=F32)) and finite(edge[1][0]) and finite(edge[1][1]) and finite(edge[1][2])


# ====================================================================================== non-finite in, non-finite out; overflow stores Inf
# The fp16 backward runs under a gradient scale that grows until something overflows, and training is right only if that overflow is SEEN:
# an Inf or NaN in a kernel's upstream gradient has to come out of it as Inf / NaN (a clamping convert, a max / med3 that drops a NaN or
# a "safe" epilogue would hide it from scot_clip_coef), and a result beyond binary16's range has to be stored as Inf.  Per kernel:
#   arrival     +Inf, NaN and -Inf, one element each, in row 0, a row of an inner tile and the last row of the upstream gradient: every
#               data-gradient output is non-finite in EVERY element of those rows (all of these kernels contract over, or normalise, the
#               row), and every reduction over rows (parameter gradients, partial sums, column sums) holds a non-finite element;
#   locality    all other rows are bit-identical to the clean launch, where the header documents the output as deterministic;
#   saturation  (f16 build, 16-bit outputs) three upstream rows scaled so that the fp64 reference leaves binary16's range: beyond
#               65520 (1 + b) the stored value is +-Inf with the reference's sign, below 65504 (1 - b) it is finite and within the bound.
#               In a fused chain this is claimed for the FIRST 16-bit store; what contracts over that row afterwards meets Inf of both
#               signs, so there the claim is non-finite in every element (Inf - Inf = NaN is legitimate), stated per output;
# and the guard bands are checked after every launch, as everywhere in this file.
def plant_rows(M):
    return (0, 64 + 5 if M > 128 else M // 2, M - 1)


def plant(g):
    """+Inf, NaN, -Inf in three rows of a [M, W] upstream gradient (columns 1, W // 2, W - 1)"""
    g = g.clone()
    M, W = g.shape
    for r, c, v in zip(plant_rows(M), (1, W // 2, W - 1), (INF, NAN, -INF)):
        g[r, c] = v
    return g


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def arrived(what, clean, dirty, M, rows=None, deterministic=True):
    """arrival and locality of one row-local output (rows of `dirty` that hold a planted upstream element: all of it non-finite)"""
    rows = plant_rows(M) if rows is None else rows
    c, d = clean.reshape(M, -1), dirty.reshape(M, -1)
    assert finite(c), what
    nf = ~torch.isfinite(d.float())
    for r in rows:
        assert bool(nf[r].all()), f"{what}: row {r} holds a planted non-finite upstream element, yet {int((~nf[r]).sum())} of {nf.shape[1]} elements are finite"
    keep = torch.ones(M, dtype=torch.bool, device=d.device)
    keep[list(rows)] = False
    assert not bool(nf[keep].any()), f"{what}: non-finite values in {int(nf[keep].any(-1).sum())} row(s) that depend on no planted element"
    if deterministic:
        assert torch.equal(bits(d[keep]), bits(c[keep])), f"{what}: rows that depend on no planted element differ from the clean launch"


def reduced(what, clean, dirty):
    """a reduction over rows: finite in the clean launch, non-finite somewhere once a row holds a planted element"""
    assert finite(clean), what
    assert bool((~torch.isfinite(dirty.float())).any()), f"{what}: a sum over rows with planted Inf / NaN is finite everywhere"


def scale_rows(k, rows=None):
    """the upstream gradient with three rows (default: plant_rows) times 2^k (exact: a power of two on fp32 or fp64 data)"""
    def up(g):
        g = g.clone()
        g[list(plant_rows(g.shape[0]) if rows is None else rows)] *= 2.0 ** k
        return g
    return up


def saturated(what, got, ref, room, rows, b, row_band=None):
    """saturation of one 16-bit [M, n] output whose `rows` were scaled out of binary16's range; ref in fp64, room: the absolute part of the
    bound (roundoff of cancelling sums), b its relative part.  On the reference ALONE: at least 90 % of the scaled rows' elements lie
    beyond 65520 (1 + b), at most 1 % between the two classes, every other row is in range.  Then: beyond 65520 (1 + b) the stored value
    is Inf of the reference's sign; below 65504 (1 - b) it is finite and, in the scaled rows, within b |ref| + room (the other rows are
    held to locality by the caller)."""
    M = ref.shape[0]
    got = got.reshape(M, -1)
    big = torch.zeros(M, dtype=torch.bool, device=ref.device)
    big[list(rows)] = True
    if row_band is None:
        must_inf, must_fin = ref.abs() > 65520.0 * (1 + b), ref.abs() < 65504.0 * (1 - b)
    else:       # a case whose existing bound is one absolute figure per row (a bound on the row's error norm bounds each element's)
        must_inf, must_fin = ref.abs() > 65520.0 + row_band, ref.abs() < 65504.0 - row_band
    share_inf, share_band = float(must_inf[big].float().mean()), float((~must_inf & ~must_fin)[big].float().mean())
    print(f"saturation {what}: {share_inf:.3f} of the scaled rows' elements must be Inf, {share_band:.4f} undecided")
    assert bool(must_fin[~big].all()), what
    if row_band is None:
        assert share_inf >= 0.9 and share_band <= 0.01, (what, share_inf, share_band)      # (the reference alone)
    else:
        assert share_inf > 0.5, (what, share_inf)             # (see the caller: the shares above are out of reach of a per-row bound)
    g64 = got.double()
    assert bool((torch.isinf(g64) & (torch.sign(g64) == torch.sign(ref)))[must_inf].all()), \
        f"{what}: {int((~(torch.isinf(g64) & (torch.sign(g64) == torch.sign(ref))))[must_inf].sum())} element(s) beyond binary16's range were not stored as Inf of the reference's sign"
    assert bool(torch.isfinite(g64)[must_fin].all()), f"{what}: Inf / NaN stored for a reference inside binary16's range"
    inside = must_fin & big.unsqueeze(1)
    bad = inside & ~((g64 - ref).abs() <= b * ref.abs() + room)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} in-range element(s) of the scaled rows beyond the bound; first at {bad.nonzero()[0].tolist()}"


def all_nonfinite(what, got, M, rows):
    """an output BEHIND a 16-bit tensor that overflowed: a contraction over a row that holds +Inf and -Inf is Inf - Inf = NaN, legitimately,
    so the claim for the scaled rows is non-finite in every element, and finite everywhere else"""
    nf = ~torch.isfinite(got.reshape(M, -1).float())
    keep = torch.ones(M, dtype=torch.bool, device=nf.device)
    keep[list(rows)] = False
    assert bool(nf[~keep].all()), f"{what}: {int((~nf[~keep]).sum())} finite element(s) in rows whose 16-bit upstream overflowed"
    assert not bool(nf[keep].any()), f"{what}: non-finite values in rows that were not scaled"


def _ln_bwd64(g, z, mean, rstd, t, gw_w, gw_b, sc, L, cond):
    """(dz, the same expression over absolute values) in fp64 of the conditional layer norm's data gradient from SAVED statistics, as
    test_mlp_block_bwd_fused restates it: dz = rstd (d - mean(d) - xhat mean(d xhat)), d = g s gamma"""
    M = g.shape[0]
    per_row = lambda v: v.double().repeat_interleave(L).view(M, 1)
    gam = (per_row(t) * gw_w.double() + gw_b.double()) if cond else gw_b.double()
    xh = (z.double() - mean.double().view(M, 1)) * rstd.double().view(M, 1)
    d = g.double() * per_row(sc) * gam
    r = rstd.double().view(M, 1)
    dz = r * (d - d.mean(-1, keepdim=True) - xh * (d * xh).mean(-1, keepdim=True))
    mag = r * (d.abs() + d.abs().mean(-1, keepdim=True) + xh.abs() * (d * xh).abs().mean(-1, keepdim=True))
    return dz, mag


B_LN16 = 2.0 ** -9       # a 16-bit layer-norm gradient: the store's 2^-11 and the fp32 arithmetic of two C-term means (the absolute term
                         # (C + 8) 2^-24 mag covers their cancellation; next to 65504 in a row scaled to ~2^21 it is below 2^-11 |ref| too)
K_SAT = 22               # g ~ N(0, 1) times 2^22 against 65504 < 2^16: |dz| / 65520 > 1 for all but the few per cent of |N(0, 1)| below 2^-5


NF_TAIL = [(kind, C, 2, 64, cond, form) for kind, cond in (("f16", True), ("bf16", False)) for C, form in ((96, "stored"), (96, "prologue"), (96, "lean"), (192, "lean"), (48, "stored"))]


@pytest.mark.parametrize("kind,C,B,L,cond,form", NF_TAIL)
def test_block_tail_bwd_nonfinite(kind, C, B, L, cond, form):
    block_tail_bwd_nonfinite(kind, C, B, L, cond, form)


def block_tail_bwd_nonfinite(kind, C, B, L, cond, form):
    """scot_block_tail_bwd in its three forms: g (upstream) -> dz2, du, dz1, da and the gradient handed to the layer below, row by row;
    the norms' parameter gradients (atomics) or the lean form's partial-sum matrices over rows."""
    M = B * L
    clean = block_tail_bwd_guarded(kind, C, B, L, cond, form, upstream=lambda g: g)
    dirty = block_tail_bwd_guarded(kind, C, B, L, cond, form, upstream=plant)
    for k in ("dz2", "dz1", "da", "g") + (() if form == "lean" else ("du",)):
        arrived(f"block_tail_bwd {form} C {C}: {k}", clean[k], dirty[k], M)
    if form == "lean":
        for k in ("part2", "part1"):
            reduced(f"block_tail_bwd lean C {C}: {k}", clean[k].view(clean[k].shape[0], -1, (C + 63) // 64 * 64)[:, :, :C],
                    dirty[k].view(dirty[k].shape[0], -1, (C + 63) // 64 * 64)[:, :, :C])
    else:
        for k in ("p2", "p1"):
            for i, (a, b) in enumerate(zip(clean[k], dirty[k])):
                if a is not None:
                    reduced(f"block_tail_bwd {form} C {C}: {k}[{i}]", a, b)
    if kind != "f16":
        return
    # saturation.  dz2 is the chain's first 16-bit store: beyond binary16's range it holds Inf of the reference's sign.  Everything behind it
    # (du, the gradient handed on, dz1, da) contracts over a row of dz2 that now holds Inf of both signs: NaN is legitimate there.
    sat = block_tail_bwd_guarded(kind, C, B, L, cond, form, upstream=scale_rows(K_SAT))
    i, rows = sat["inputs"], plant_rows(M)
    gin = i["g0"].double() + (i["dqkv"].double() @ i["wqkv"].double() if form == "prologue" else 0.0)
    ref, mag = _ln_bwd64(gin, i["z2"], i["m2"], i["r2"], i["t"], i["n2_0"], i["n2_1"], i["s2"], L, cond)
    saturated(f"block_tail_bwd {form} C {C}: dz2", sat["dz2"], ref, (C + 8) * kc.U32 * mag, rows, B_LN16)
    keep = [r for r in range(M) if r not in rows]
    assert torch.equal(bits(sat["dz2"][keep]), bits(clean["dz2"][keep])), "dz2: rows that were not scaled differ from the clean launch"
    for k in ("dz1", "da", "g") + (() if form == "lean" else ("du",)):
        all_nonfinite(f"block_tail_bwd {form} C {C} behind an overflowed dz2: {k}", sat[k], M, rows)
        assert torch.equal(bits(sat[k].reshape(M, -1)[keep]), bits(clean[k].reshape(M, -1)[keep])), f"{k}: rows that were not scaled differ from the clean launch"


@pytest.mark.parametrize("kind,C,cond", [("f16", 96, True), ("bf16", 192, False)])
def test_fused_halves_bwd_nonfinite(kind, C, cond):
    fused_halves_bwd_nonfinite(kind, C, 2, 64, cond)


def fused_halves_bwd_nonfinite(kind, C, B, L, cond):
    """scot_proj_cln_bwd and scot_mlp_block_bwd on their own"""
    with _build(kind):
        M = B * L
        clean = fused_halves_bwd_guarded(C, B, L, cond, upstream=lambda g: g)
        dirty = fused_halves_bwd_guarded(C, B, L, cond, upstream=plant)
        for k in ("pdz", "pda", "mdz", "mdu", "mg"):
            arrived(f"fused halves bwd C {C}: {k}", clean[k], dirty[k], M)
        for i, (a, b) in enumerate(zip(clean["grads"], dirty["grads"])):
            reduced(f"fused halves bwd C {C}: parameter gradient {i}", a, b)
        if kind != "f16":
            return
        # saturation: each kernel's first 16-bit store (its layer-norm gradient) holds Inf of the reference's sign; what contracts over
        # that row (proj_cln_bwd's da; mlp_block_bwd's du and the gradient handed on) sees Inf of both signs: NaN is legitimate there
        sat = fused_halves_bwd_guarded(C, B, L, cond, upstream=scale_rows(K_SAT))
        i, rows = sat["inputs"], plant_rows(M)
        keep = [r for r in range(M) if r not in rows]
        for out, n, s, behind in (("pdz", "n1", "s1", ("pda",)), ("mdz", "n2", "s2", ("mdu", "mg"))):
            ref, mag = _ln_bwd64(i["g"], i["z"], i["mean"], i["rstd"], i["t"], i[n + "_0"], i[n + "_1"], i[s], L, cond)
            saturated(f"fused halves bwd C {C}: {out}", sat[out], ref, (C + 8) * kc.U32 * mag, rows, B_LN16)
            for k in behind:
                all_nonfinite(f"fused halves bwd C {C} behind an overflowed {out}: {k}", sat[k], M, rows)
            for k in (out,) + behind:
                assert torch.equal(bits(sat[k].reshape(M, -1)[keep]), bits(clean[k].reshape(M, -1)[keep])), f"{k}: rows that were not scaled differ from the clean launch"


@pytest.mark.parametrize("kind,cond,x16,B,L,C", [("f16", True, True, 2, 72, 96), ("f16", False, False, 3, 43, 20), ("f16", True, True, 2, 1024, 192),
                                                 ("f16", False, True, 3, 43, 20), ("bf16", True, True, 2, 72, 96)])
def test_cln_bwd_nonfinite(kind, cond, x16, B, L, C):
    cln_bwd_nonfinite(kind, cond, x16, B, L, C)


def cln_bwd_nonfinite(kind, cond, x16, B, L, C):
    """scot_cln_bwd (atomics) and its mode 3 with scot_cln_bwd_finish: dout -> dx row by row, parameter gradients and d_xbias over rows.
    x16: x and dx in the build's 16-bit type.  Saturation (f16 build, 16-bit dx): three rows of dout times 2^22 against cln_model's fp64 dx;
    dx is the kernel's only 16-bit store, so Inf of the reference's sign is the claim for both entry points."""
    with _build(kind) as hd:
        _cln_bwd_nonfinite(kind, cond, hd if x16 else F32, B, L, C)


def _cln_bwd_nonfinite(kind, cond, xdt, B, L, C):
    x, res, t, ps, dout = _cln_inputs(xdt, B, L, C)
    M = B * L
    tt = t if cond else None
    out = {}
    ups = [("clean", dout), ("dirty", plant(dout.reshape(M, C)).reshape(dout.shape))]
    if kind == "f16" and xdt != F32:
        ups.append(("scaled", scale_rows(K_SAT)(dout.reshape(M, C)).reshape(dout.shape)))
    for name, up in ups:
        gd = Guards()
        xg, rg, tg, dog = gd.op(x, name="x"), gd.op(res, name="resid"), gd.op(tt, name="time"), gd.op(up, name="dout")
        pg = [gd.op(p, name=f"param{i}") if (cond or i in (1, 3)) else None for i, p in enumerate(ps)]
        og, mg, sg = gd.out((B, L, C), F32, name="out"), gd.out((M,), F32, name="mean"), gd.out((M,), F32, name="rstd")
        ops.cln_fwd(xg, rg, og, mg, sg, tg, pg[0], pg[1], pg[2], pg[3], M, L, C, 1e-5)
        dxg = gd.out((B, L, C), xdt, name="dx")
        gr = gd.group([(C,)] * 5, F32, fills=[0.0] * 5, name="d_gw_w|d_gw_b|d_bw_w|d_bw_b|d_xbias")
        ops.cln_bwd(dog, xg, mg, sg, tg, pg[0], pg[1], dxg, gr[0], gr[1], gr[2], gr[3], M, L, C, d_xbias=gr[4])
        o = dict(dx=dxg, grads=[gr[i] for i in ([0, 1, 2, 3] if cond else [1, 3])] + [gr[4]])
        nf = ops.cln_bwd_partial_floats(M, L, C, cond)
        if nf:
            part, dx3 = gd.out((nf,), F32, name="mode-3 partial sums"), gd.out((B, L, C), xdt, name="dx (mode 3)")
            g3 = gd.group([(C,)] * 4, F32, fills=[0.0] * 4, name="mode-3 gradients")
            sel = g3 if cond else [None, g3[0], None, g3[1]]
            ops.cln_bwd(dog, xg, mg, sg, tg, pg[0], pg[1], dx3, None, None, None, None, M, L, C, sample_scale=None, mode=3, partial=part)
            ops.cln_bwd_finish(part, M, L, C, sel[0], sel[1], sel[2], sel[3])
            o.update(dx3=dx3, grads3=[g_ for g_ in sel if g_ is not None])
        sync()
        gd.check()
        out[name] = o
    c, d = out["clean"], out["dirty"]
    arrived(f"cln_bwd {(B, L, C)}: dx", c["dx"], d["dx"], M)
    for i, (a, b) in enumerate(zip(c["grads"], d["grads"])):
        reduced(f"cln_bwd {(B, L, C)}: gradient {i}", a, b)
    if "dx3" in c:
        arrived(f"cln_bwd mode 3 {(B, L, C)}: dx", c["dx3"], d["dx3"], M)
        for i, (a, b) in enumerate(zip(c["grads3"], d["grads3"])):
            reduced(f"cln_bwd_finish {(B, L, C)}: gradient {i}", a, b)
    if "scaled" not in out:
        return
    s, rows = out["scaled"], plant_rows(M)
    ref = cln_model(x, res, t, ps[0], ps[1], ps[2], ps[3], None, ups[2][1], cond, xdt, exact=True)[1].reshape(M, C)
    # the same expression over absolute values, from fp64 statistics (biased variance, eps = 1e-5)
    x64 = x.double().reshape(M, C)
    xc = x64 - x64.mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + 1e-5)
    gam = (t.double().repeat_interleave(L).view(M, 1) * ps[0].double() + ps[1].double()) if cond else ps[1].double()
    dd, xh = ups[2][1].double().reshape(M, C) * gam, xc * rs
    mag = rs * (dd.abs() + dd.abs().mean(-1, keepdim=True) + xh.abs() * (dd * xh).abs().mean(-1, keepdim=True))
    keep = [r for r in range(M) if r not in rows]
    for k in ("dx", "dx3") if "dx3" in s else ("dx",):
        saturated(f"cln_bwd {(B, L, C)}: {k}", s[k], ref, (C + 8) * kc.U32 * mag, rows, B_LN16)
        assert torch.equal(bits(s[k].reshape(M, C)[keep]), bits(c[k].reshape(M, C)[keep])), f"{k}: rows that were not scaled differ from the clean launch"


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("what,layout,mixed,M,N,K", NAN_CASES, ids=[c[0] for c in NAN_CASES])
def test_gemm_16bit_result_nonfinite(kind, what, layout, mixed, M, N, K):
    gemm_16bit_result_nonfinite(kind, layout, mixed, M, N, K, wide=(2, 0) if what == "gemm_wide" else None, family=NAN_FAMILY[what.split()[0]])


def gemm_16bit_result_nonfinite(kind, layout, mixed, M, N, K, wide=None, family=None):
    """scot_gemm with a 16-bit C (the data gradients dX = dY W of the backward), one case per kernel family: arrival and locality for
    planted rows of A, and — f16 build — saturation: three rows of A times 2^12 and B times 2^8 put the fp64 reference of those rows
    around 2^20, all else stays in range.  b = 2e-3, this file's bound for 16-bit products."""
    with _build(kind) as hd:
        with _gemm_config(wide=wide):
            A, B = _operands(layout, ops.BF16, mixed, M, N, K)
            rows = plant_rows(M)

            def launch(A_, B_):
                gd = Guards()
                Ag, Bg, Cg = gd.op(A_, 8, "A"), gd.op(B_, 8, "B"), gd.out((M, N), hd, 8, name="C")
                args = (layout, ops.BF16, M, N, K, Ag, A_.shape[1] + 8, Bg, B_.shape[1] + 8, Cg, N + 8)
                assert family is None or ops.gemm_route(*args)[0] == family, f"the case reaches kernel family {ops.gemm_route(*args)[0]}, not {family}"
                ops.gemm(*args)
                sync()
                gd.check()
                return Cg
            clean = launch(A, B)
            arrived(f"gemm layout {layout} {M}x{N}x{K} -> 16-bit C", clean, launch(plant(A), B), M)
            if kind != "f16":
                return
            b = 2e-3
            As, Bs = A.clone(), (B.float() * 256.0).to(B.dtype)
            As[list(rows)] = (As[list(rows)].float() * 4096.0).to(A.dtype)
            assert finite(As) and finite(Bs)
            ref, ab = _product64(layout, ops.BF16, As, Bs)
            big = torch.zeros(M, dtype=torch.bool, device=ref.device)
            big[list(rows)] = True
            must_inf, must_fin = ref.abs() > 65520.0 * (1 + b), ref.abs() < 65504.0 * (1 - b)
            share_inf = float(must_inf[big].float().mean())
            share_band = float((~must_inf & ~must_fin)[big].float().mean())
            print(f"saturation {M}x{N}x{K}: {share_inf:.3f} of the scaled rows' elements must be Inf, {share_band:.4f} undecided")
            assert share_inf >= 0.9 and share_band <= 0.01 and bool(must_fin[~big].all())          # (a condition on the reference alone)
            got = launch(As, Bs)
            g64 = got.double()
            assert bool((torch.isinf(g64) & (torch.sign(g64) == torch.sign(ref)))[must_inf].all()), \
                f"{int((~torch.isinf(g64))[must_inf].sum())} element(s) beyond binary16's range were not stored as Inf of the reference's sign"
            assert bool(torch.isfinite(g64)[must_fin].all()), "Inf / NaN stored for a reference inside binary16's range"
            zero = torch.zeros_like(got)
            assert_excess(f"gemm saturation {M}x{N}x{K}: the elements in range", torch.where(must_fin, got, zero), torch.where(must_fin, ref, zero.double()),
                          torch.where(must_fin, ab, torch.ones_like(ab)), K, U_MFMA16)
            base = launch(A, Bs)                       # the unscaled rows obey locality: identical to the launch without scaled rows
            keep = ~big
            assert torch.equal(bits(got[keep]), bits(base[keep]))


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("rows,C", [(130, 96), (37, 24)])
def test_device_scaled_ops_nonfinite(kind, rows, C):
    device_scaled_ops_nonfinite(kind, rows, C)


def device_scaled_ops_nonfinite(kind, rows, C):
    """scot_colscale_dev (16-bit out: the ConvNeXt branch's upstream gradient under its extra power of two) and scot_axpy_dev (the way the
    branch's scratch gradients — where an overflow of that branch happens — reach the arena); scot_partial_colsum(_batch) and
    scot_replica_reduce (the sums that finish partial matrices and attention's replicas).  Elementwise kernels: the planted ELEMENT is
    non-finite, every other element is bit-identical (the column sums of 64 and more partial rows meet in atomics: those columns agree
    to the roundoff of the sum instead).  Saturation of colscale_dev (f16): the three rows of g times 2^22, every other row as in the clean launch."""
    with _build(kind) as hd:
        g, gamma = G.rnd(rows, C, seed=1), 1.0 + G.rnd(C, seed=2, scale=0.1)
        spots = list(zip(plant_rows(rows), (1, C // 2, C - 1)))

        def elementwise(what, clean, dirty, shape):
            c, d = clean.reshape(shape), dirty.reshape(shape)
            assert finite(c)
            hit = torch.zeros(shape, dtype=torch.bool, device=c.device)
            for r, col in spots:
                hit[r, col] = True
            nf = ~torch.isfinite(d.float())
            assert torch.equal(nf, hit), f"{what}: non-finite exactly where planted expected, found {int(nf.sum())} element(s)"
            assert torch.equal(bits(d[~hit]), bits(c[~hit])), what

        def colscale(g_, mul):
            gd = Guards()
            o = gd.out((rows, C), hd, name="colscale out")
            ops.colscale_dev(gd.op(g_, name="g"), gd.op(gamma, name="gamma"), gd.op(torch.tensor([mul], device=G.DEV), name="mul"), o, rows, C)
            sync()
            gd.check()
            return o
        elementwise("colscale_dev", colscale(g, 4.0), colscale(plant(g), 4.0), (rows, C))
        if kind == "f16":
            b = 2.0 ** -10              # three fp32 roundings and the store's
            gs = scale_rows(K_SAT)(g)                   # the three rows times 2^22, mul = 4 as in the clean launch: all other rows stay in range
            ref = gs.double() * gamma.double() * 4.0
            sat = colscale(gs, 4.0)
            saturated("colscale_dev", sat, ref, 0.0, plant_rows(rows), b)
            keep = [r for r in range(rows) if r not in plant_rows(rows)]
            assert torch.equal(bits(sat[keep]), bits(colscale(g, 4.0)[keep])), "colscale_dev: rows that were not scaled differ from the clean launch"

        def axpy(src_, clear):
            gd = Guards()
            dst, src = gd.out((rows * C,), F32, src=G.rnd(rows * C, seed=3), name="dst"), gd.out((rows * C,), F32, src=src_.reshape(-1), name="src")
            ops.axpy_dev(dst, src, gd.op(torch.tensor([0.25], device=G.DEV), name="alpha"), clear_src=clear)
            sync()
            gd.check()
            if clear:
                assert float(src.abs().max()) == 0.0
            return dst
        for clear in (False, True):
            elementwise(f"axpy_dev clear_src {clear}", axpy(g, clear), axpy(plant(g), clear), (rows, C))

        def colsums(part_):
            gd = Guards()
            pg = gd.op(part_, name="partial")
            o1 = gd.out((C,), F32, fill=0.5, name="partial_colsum out")
            o2 = gd.out((C,), F32, fill=0.5, name="partial_colsum_batch out")
            o3 = gd.out((C,), F32, fill=0.5, name="partial_colsum_batch out (2)")
            ops.partial_colsum(pg, rows, C, o1)
            ops.partial_colsum_batch([(pg, rows, C, o2), (pg, rows - 1, C, o3)])
            rep = gd.out((3, 2 * C), F32, src=torch.stack([part_[r, :C].repeat(2) for r in plant_rows(rows)]), name="replicas")
            desc = gd.op(torch.tensor([[0, 0, C], [C, C, C - 3]], dtype=torch.int32, device=G.DEV), name="desc")
            o4 = gd.out((2 * C,), F32, fill=0.5, name="replica_reduce dst")
            ops.replica_reduce(rep, 0, 3, 2 * C, desc, 2, C, o4)
            sync()
            gd.check()
            return o1, o2, o3, o4
        cols = [c for _, c in spots]
        cl, di = colsums(g), colsums(plant(g))
        for what, c_, d_, planted_cols in (("partial_colsum", cl[0], di[0], cols), ("partial_colsum_batch", cl[1], di[1], cols),
                                           ("partial_colsum_batch (all but the last row)", cl[2], di[2], cols[:2]),
                                           ("replica_reduce", cl[3][:C], di[3][:C], cols), ("replica_reduce (second entry)", cl[3][C:2 * C - 3], di[3][C:2 * C - 3], cols[:2])):
            assert finite(c_), what
            nf = ~torch.isfinite(d_)
            want = torch.zeros_like(nf)
            want[planted_cols] = True
            assert torch.equal(nf, want), f"{what}: non-finite columns {nf.nonzero().flatten().tolist()}, planted {planted_cols}"
            if what.startswith("partial_colsum") and rows >= 64:      # from 64 rows on the sum runs in slices that meet in `out` through atomics
                room = 8 * kc.U32 * (g.double().abs().sum(0) + 0.5)[:d_.numel()]
                assert bool(((d_.double() - c_.double()).abs() <= room)[~want].all()), what
            else:
                assert torch.equal(bits(d_[~want]), bits(c_[~want])), what
        assert float(di[3][2 * C - 3:].min()) == 0.5 and float(di[3][2 * C - 3:].max()) == 0.5      # beyond the entry's count: untouched


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("K,dims", [(200, [(40, 72), (72, 40), (48, 48)]), (2048, [(96, 384), (384, 96), (288, 96)])], ids=["ragged", "C96"])
def test_wgrad_group_nonfinite(kind, K, dims):
    wgrad_group_nonfinite(kind, K, dims)


def wgrad_group_nonfinite(kind, K, dims):
    """scot_wgrad_group (or, for shapes it declines, the per-problem path) in every grad mode — GRAD_STORE_SCALED, GRAD_ADD_SCALED, GRAD_ADD,
    one problem each: dW = dY^T X is a reduction over the tokens, so a planted element of dY in column c makes ROW c of dW non-finite in
    every element and db[c] non-finite; every other row of dW is bit-identical to the clean launch (deterministic), every other bias
    gradient (atomics) stays finite."""
    with _build(kind) as hd:
        modes = [ops.GRAD_STORE_SCALED, ops.GRAD_ADD_SCALED, ops.GRAD_ADD][:len(dims)]
        s = torch.tensor([2.0 ** -7], device=G.DEV)
        dys = [G.rnd(K, m, dtype=hd, scale=0.5, seed=10 + i) for i, (m, _) in enumerate(dims)]
        xs = [G.rnd(K, nn, dtype=hd, seed=20 + i) for i, (_, nn) in enumerate(dims)]
        dws0 = [G.rnd(m, nn, seed=30 + i) for i, (m, nn) in enumerate(dims)]
        dbs0 = [G.rnd(m, seed=40 + i) for i, (m, _) in enumerate(dims)]
        covered = all(m % 8 == 0 and nn % 8 == 0 for m, nn in dims) and K % 8 == 0

        def launch(dys_):
            with _gemm_config(splitk=(0, 1)):
                gd = Guards()
                dyg, xg = [gd.op(t, name=f"dY{i}") for i, t in enumerate(dys_)], [gd.op(t, name=f"X{i}") for i, t in enumerate(xs)]
                dwg = gd.group([tuple(t.shape) for t in dws0], F32, srcs=[None if md == ops.GRAD_STORE_SCALED else t for t, md in zip(dws0, modes)], name="dW arena")
                dbg = gd.group([tuple(t.shape) for t in dbs0], F32, srcs=dbs0, name="dbias arena")
                ok = ops.wgrad_group(ops.BF16, list(zip(dyg, xg, dwg, dbg)), modes, gd.op(s, name="grad_scale"))
                assert ok == covered
                if not ok:
                    for dy, x, dw, db in zip(dyg, xg, dwg, dbg):
                        dw.copy_(dws0[dwg.index(dw)])
                        ops.linear_wgrad(ops.BF16, dy, x, dw, dbias=db)
                sync()
                gd.check()
                return dwg, dbg
        cw, cb = launch(dys)
        dw_, db_ = launch([plant(t.float()).to(hd) for t in dys])
        for i, (m, _) in enumerate(dims):
            cols = (1, m // 2, m - 1)
            arrived(f"wgrad_group K {K} dW{i} mode {modes[i]}", cw[i], dw_[i], m, rows=cols)
            nf = ~torch.isfinite(db_[i])
            want = torch.zeros_like(nf)
            want[list(cols)] = True
            assert finite(cb[i]) and torch.equal(nf, want), f"wgrad_group K {K} db{i}: non-finite at {nf.nonzero().flatten().tolist()}, planted columns {cols}"


@pytest.mark.parametrize("kind,M,C,mode", [("f16", 136, 96, ops.GRAD_ADD), ("f16", 136, 96, ops.GRAD_STORE_SCALED), ("f16", 136, 96, ops.GRAD_ADD_SCALED),
                                           ("bf16", 72, 192, ops.GRAD_STORE_SCALED), ("f16", 1000, 96, ops.GRAD_ADD_SCALED)])
def test_wgrad_mlp_nonfinite(kind, M, C, mode):
    wgrad_mlp_nonfinite(kind, M, C, mode)


def wgrad_mlp_nonfinite(kind, M, C, mode):
    """scot_wgrad_mlp in every grad mode.  dz (upstream) planted at (r, c):  dW2 = dz^T gelu(u): row c non-finite in every element, the other
    rows bit-identical (deterministic), db2[c] non-finite alone;  D = dz W2 is non-finite in all of row r, so du = D gelu'(u) is, and
    dW1 = du^T h16 and db1 = sum du, reductions over the rows, are non-finite in EVERY element."""
    with _build(kind) as hd:
        hid = 4 * C
        h16, dz = G.rnd(M, C, dtype=hd, seed=1), G.rnd(M, C, dtype=hd, scale=0.5, seed=2)
        w1, b1 = G.rnd(hid, C, scale=C ** -0.5, seed=3).to(hd), G.rnd(hid, seed=4, scale=0.2)
        w2t = G.rnd(C, hid, scale=hid ** -0.5, seed=5).to(hd).t().contiguous()
        sizes = [hid * C, hid, C * hid, C]
        s = torch.tensor([2.0 ** -7], device=G.DEV) if mode != ops.GRAD_ADD else None
        flat0 = G.rnd(sum(sizes), seed=6)

        def launch(dz_):
            gd = Guards()
            fg = gd.out((sum(sizes),), F32, src=flat0, name="dW1|db1|dW2|db2")
            o = torch.split(fg, sizes)
            dW1, db1, dW2, db2 = o[0].view(hid, C), o[1], o[2].view(C, hid), o[3]
            if mode == ops.GRAD_STORE_SCALED:
                dW1.fill_(NAN)
                dW2.fill_(NAN)
            assert ops.wgrad_mlp(gd.op(h16, name="h16"), gd.op(dz_, name="dz"), gd.op(w1, name="w1"), gd.op(b1, name="b1"), gd.op(w2t, name="w2t"),
                                 dW1, db1, dW2, db2, mode=mode, grad_scale=gd.op(s, name="grad_scale"))
            sync()
            gd.check()
            return dW1, db1, dW2, db2
        c, d = launch(dz), launch(plant(dz.float()).to(hd))
        cols = (1, C // 2, C - 1)
        assert all(finite(t) for t in c)
        arrived(f"wgrad_mlp M {M} C {C} mode {mode}: dW2", c[2], d[2], C, rows=cols)
        nf = ~torch.isfinite(d[3])
        want = torch.zeros_like(nf)
        want[list(cols)] = True
        assert torch.equal(nf, want) and torch.equal(bits(d[3][~want]), bits(c[3][~want])), "wgrad_mlp: db2"
        assert not bool(torch.isfinite(d[0]).any()), f"wgrad_mlp dW1: {int(torch.isfinite(d[0]).sum())} finite element(s) below rows of du that are not finite"
        assert not bool(torch.isfinite(d[1]).any()), "wgrad_mlp db1"


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("shape", [(2, 9, 11, 33), (2, 12, 20, 24), (1, 17, 16, 96)], ids=DW_IDS)
@pytest.mark.parametrize("x16", [False, True], ids=["x_f32", "x_16"])
def test_dwconv7_data_gradient_nonfinite(kind, shape, x16):
    dwconv7_data_gradient_nonfinite(kind, *shape, x16)


def dwconv7_data_gradient_nonfinite(kind, B, H, W, C, x16):
    """scot_dwconv7 with flip = 1 and a 16-bit result (the ConvNeXt block's data gradient).  A pixel of the result depends on the 7 x 7
    pixels around it in its own image and channel, cropped at the border (zero padding): the dependency mask is the stencil applied to the
    indicator of the planted elements.  Saturation (f16, fp32 upstream): image row H // 2 of sample 0 times 2^22; b = 2^-10 (50 fp32
    additions and the store's rounding)."""
    with _build(kind) as hd:
        xdt = hd if x16 else F32
        dy = G.rnd(B, H, W, C, seed=3, dtype=xdt)
        w = G.rnd(C, 1, 7, 7, seed=1, scale=0.2)

        def launch(dy_):
            gd = Guards()
            y = gd.out((B, H, W, C), hd, name="dx")
            ops.dwconv7(gd.op(dy_, name="dy"), gd.op(w, name="w"), None, y, B, H, W, C, flip=True)
            sync()
            gd.check()
            return y
        clean = launch(dy)
        assert finite(clean)
        hit = torch.zeros(B, H, W, C, dtype=torch.float64, device=G.DEV)
        dirty_in = dy.clone()
        for (b_, h_, w_, c_), v in zip(((0, 0, 1, 1), (B - 1, H // 2, W // 2, C // 2), (B - 1, H - 1, W - 1, C - 1)), (INF, NAN, -INF)):
            dirty_in[b_, h_, w_, c_] = v
            hit[b_, h_, w_, c_] = 1.0
        dep = _dwconv64(hit, torch.ones_like(w, dtype=torch.float64), None, True) > 0
        assert int(dep.sum()) in range(3 * 16, 3 * 49 + 1)
        got = launch(dirty_in)
        nf = ~torch.isfinite(got.float())
        assert torch.equal(nf, dep), f"dwconv7 flip: {int((nf & ~dep).sum())} non-finite element(s) outside the stencil of a planted one, {int((dep & ~nf).sum())} finite inside"
        assert torch.equal(bits(got[~dep]), bits(clean[~dep]))
        if kind != "f16" or x16:
            return
        b = 2.0 ** -10
        big_in = dy.clone()
        big_in[0, H // 2] *= 2.0 ** 22
        ref = _dwconv64(big_in.double(), w.double(), None, True)
        mag = _dwconv64(big_in.double().abs(), w.double().abs(), None, True)
        rows = torch.zeros(B, H, W, C, dtype=torch.bool, device=G.DEV)
        rows[0, H // 2] = True
        near = _dwconv64(rows.double(), torch.ones_like(w, dtype=torch.float64), None, True) > 0
        must_inf, must_fin = ref.abs() > 65520.0 * (1 + b), ref.abs() < 65504.0 * (1 - b)
        share_inf, share_band = float(must_inf[rows].float().mean()), float((~must_inf & ~must_fin)[rows].float().mean())
        print(f"dwconv7 saturation {(B, H, W, C)}: {share_inf:.3f} of the scaled row's elements must be Inf, {share_band:.4f} undecided")
        assert share_inf >= 0.9 and share_band <= 0.01 and bool(must_fin[~near].all())
        got = launch(big_in)
        g64 = got.double()
        assert bool((torch.isinf(g64) & (torch.sign(g64) == torch.sign(ref)))[must_inf].all()), \
            f"{int((~torch.isinf(g64))[must_inf].sum())} element(s) beyond binary16's range were not stored as Inf of the reference's sign"
        assert bool(torch.isfinite(g64)[must_fin].all())
        zero = torch.zeros_like(got)
        assert_excess(f"dwconv7 saturation {(B, H, W, C)}: the elements in range", torch.where(must_fin, got, zero), torch.where(must_fin, ref, zero.double()),
                      torch.where(must_fin, mag, torch.ones_like(mag)), 50, kc.U32)
        assert torch.equal(bits(got[~near]), bits(clean[~near]))


NF_ATTN = [("f16", (2, 8, 8, 32, 2, 4, 2)), ("bf16", (1, 14, 14, 32, 1, 7, 3)), ("f16", (1, 32, 32, 96, 3, 16, 8)), ("bf16", (1, 16, 16, 32, 2, 16, 0))]


@pytest.mark.parametrize("kind,case", NF_ATTN, ids=lambda v: str(v).replace(" ", ""))
def test_window_attention_bwd_nonfinite(kind, case):
    window_attention_bwd_nonfinite(kind, case)


def window_attention_bwd_nonfinite(kind, case):
    """scot_window_attn_bwd (generic and 16 x 16 windows) and scot_window_attn_bwd_rep with 16-bit operands.  dout planted at token r, channel
    ch of head h; within r's (shifted) window W:
      dV = P^T dO     column ch of the value block is non-finite for EVERY token of W (a masked pair has P = 0 and 0 * Inf = NaN);
      dP = dO V^T     row r, so dS row r, so dQ of token r in all of head h's channels, and dK = dS^T Q in all of head h's channels for
                      every token of W (the cosine normalisation's backward keeps NaN);
      dbias_table and dlogit_scale (sums over windows, atomics / replicas) hold a non-finite element for head h.
    Locality: tokens of every other window are bit-identical to the clean launch, and so are, inside W, the columns of the other heads.
    (Inside head h's blocks of W the untouched columns may or may not be identical: not asserted.)"""
    with _build(kind) as half:
        B, Hp, Wp, C, heads, ws, shift = case
        L, TS, N, d = Hp * Wp, (2 * ws - 1) ** 2, ws * ws, C // heads
        nW = (Hp // ws) * (Wp // ws)
        qkv, table, ls, dout = _attn_inputs(case, half)
        R, pad = 3, 5
        st, sl = heads * TS + pad, heads + pad

        def launch(dout_, qkv_=None):
            gd = Guards()
            qg, tg, lg, dg = gd.op(qkv if qkv_ is None else qkv_, name="qkv"), gd.op(table, name="bias_table"), gd.op(ls, name="logit_scale"), gd.op(dout_, name="dout")
            og, lseg = gd.out((B, L, C), half, name="out"), gd.out((B * nW, heads, N), F32, name="lse")
            dqg, dtg, dlg = gd.out((B, L, 3 * C), half, name="dqkv"), gd.out((heads, TS), F32, fill=0.0, name="dbias_table"), \
                gd.out((heads,), F32, fill=0.0, name="dlogit_scale")
            ops.window_attn_fwd(ops.BF16, qg, og, lseg, tg, lg, B, Hp, Wp, C, heads, ws, shift)
            ops.window_attn_bwd(ops.BF16, qg, og, dg, lseg, tg, lg, dqg, dtg, dlg, B, Hp, Wp, C, heads, ws, shift)
            rtg, rlg = gd.out((R * st,), F32, fill=0.0, name="table replicas"), gd.out((R * sl,), F32, fill=0.0, name="logit-scale replicas")
            dq2g = gd.out((B, L, 3 * C), half, name="dqkv (replica entry)")
            ops.window_attn_bwd_rep(ops.BF16, qg, og, dg, lseg, tg, lg, dq2g, rtg, rlg, B, Hp, Wp, C, heads, ws, shift, R, st, sl)
            sync()
            gd.check()
            rt = rtg.view(R, st)[:, :heads * TS].reshape(R, heads, TS)
            return dict(dqkv=dqg, dqkv_rep=dq2g, dtable=dtg, dls=dlg, rt=rt, rl=rlg.view(R, sl)[:, :heads])
        clean = launch(dout)
        assert all(finite(v) for v in clean.values())
        M = B * L
        spots = list(zip(plant_rows(M), (1, C // 2, C - 1)))
        dirty = launch(plant(dout.reshape(M, C).float()).to(half).reshape(B, L, C))
        tok = torch.arange(M, device=G.DEV)
        b_, y_, x_ = tok // L, (tok % L) // Wp, tok % Wp
        win = (b_ * (Hp // ws) + ((y_ - shift) % Hp) // ws) * (Wp // ws) + ((x_ - shift) % Wp) // ws       # window of every token (torch.roll by -shift)
        must = torch.zeros(M, 3 * C, dtype=torch.bool, device=G.DEV)       # has to be non-finite
        free = torch.zeros(M, 3 * C, dtype=torch.bool, device=G.DEV)       # may be either
        hit_heads = set()
        for r, ch in spots:
            h = ch // d
            hit_heads.add(h)
            inw = win == win[r]
            assert int(inw.sum()) == N
            must[inw, 2 * C + ch] = True
            must[inw, C + h * d:C + (h + 1) * d] = True
            must[r, h * d:(h + 1) * d] = True
            for blk in range(3):
                free[inw, blk * C + h * d:blk * C + (h + 1) * d] = True
        for name in ("dqkv", "dqkv_rep"):
            got, ref = dirty[name].reshape(M, 3 * C), clean[name].reshape(M, 3 * C)
            nf = ~torch.isfinite(got.float())
            assert bool(nf[must].all()), f"{name}: {int((~nf)[must].sum())} of {int(must.sum())} elements that depend on a planted dout element are finite"
            assert not bool(nf[~free].any()), f"{name}: {int(nf[~free].sum())} non-finite element(s) in other windows or other heads"
            assert torch.equal(bits(got[~free]), bits(ref[~free])), f"{name}: other windows / other heads differ from the clean launch"
        for h in range(heads):
            for name in ("dtable", "dls", "rt", "rl"):
                t = dirty[name]
                part = t[..., h, :] if name in ("dtable", "rt") else t[..., h]
                if h in hit_heads:
                    assert bool((~torch.isfinite(part)).any()), f"{name}: head {h} saw a planted element, its sum is finite everywhere"
                else:
                    assert bool(torch.isfinite(part).all()), f"{name}: head {h} saw no planted element"
        if kind != "f16":
            return
        # saturation.  dout is a 16-bit OPERAND here, so a scaled row has to stay below 65504 itself: three tokens' rows times 2^A_SAT.
        #   dV = P^T dO is a convex combination of rows of dO: it cannot leave the range, and is asserted finite everywhere.
        #   dq = (dq^ - q^ (q^ . dq^)) / |q| grows with 1 / |q| (cosine attention: the forward does not depend on |q|), so q and k of every
        #   token are given at 2^-Q_SAT of their size; dS = P (dP - delta), the 16-bit operand in between, stays in range (the logit
        #   scale is applied in fp32 behind it), so the q block of the three tokens is a FINAL 16-bit store: Inf of the reference's sign.
        # The bound: this kernel's existing bound is window_attention_guarded's, per ROW: |got - exact| <= MARGIN max(e_model, median) |exact|
        # in the row's 2-norm, e_model the rounding model's relative error (dominated by delta taken from the rounded O).  A bound on the
        # row's error norm bounds each element's, so every element of row r gets the absolute band t_r = that figure, from the model at
        # the unscaled dout (dq of a token is linear in its row of dout; the model itself rounds its scaled result to Inf): beyond
        # 65520 + t_r Inf of the reference's sign, below 65504 - t_r finite and within t_r.  t_r is a fixed fraction of the row's norm, so
        # NO scale brings 90 % of a row beyond it with 1 % in between: on the reference alone the shares are 0.875 / 0.125 ((2,8,8,32,2,4,2))
        # and 0.875 / 0.087 ((1,32,32,96,3,16,8)) here and 0.906 / 0.094, 0.917 / 0.083 at four times the scale.  Asserted instead: more
        # than half of the scaled rows' elements are in the must-be-Inf class.
        A_SAT, Q_SAT = 13, 9
        small = qkv.clone()
        small[..., :2 * C] = (small[..., :2 * C].float() * 2.0 ** -Q_SAT).to(half)
        rows = plant_rows(M)
        dsc = scale_rows(A_SAT)(dout.reshape(M, C).float()).to(half).reshape(B, L, C)
        assert finite(dsc)
        ex = attn_model(small, table, ls, dout, case, "16", half, exact=True)[1].reshape(M, 3 * C)[:, :C]
        mo = attn_model(small, table, ls, dout, case, "16", half)[1].reshape(M, 3 * C)[:, :C]
        e_model = kc.row_errors(mo, ex)
        factor = torch.ones(M, 1, dtype=torch.float64, device=ex.device)
        factor[list(rows)] = 2.0 ** A_SAT
        ref = ex * factor
        band = (MARGIN["attn16"] * torch.maximum(e_model, e_model.median()) * ex.norm(dim=-1)).unsqueeze(1) * factor
        base, sat = launch(dout, small), launch(dsc, small)
        scaled_windows = torch.zeros(M, dtype=torch.bool, device=G.DEV)
        for r in rows:
            scaled_windows |= win == win[r]
        for name in ("dqkv", "dqkv_rep"):
            got = sat[name].reshape(M, 3 * C)
            saturated(f"window attention {case}: the q block of {name}", got[:, :C], ref[:, :C], band, rows, 0.0, row_band=band)
            assert finite(got[:, 2 * C:]), f"{name}: dV, a convex combination of in-range rows of dO, is not finite"
            assert torch.equal(bits(got[~scaled_windows]), bits(base[name].reshape(M, 3 * C)[~scaled_windows])), f"{name}: windows without a scaled token differ from the unscaled launch"


def test_cpb_bwd_batched_nonfinite():
    cpb_bwd_batched_nonfinite(CPB_LAYERS, 1)


def cpb_bwd_batched_nonfinite(layers, first):
    """scot_cpb_bwd_batched: dtable (what the attention backward accumulated) planted at (head h, table entry t) of three layers of the
    range.  The bias MLP is table = 16 sigmoid(w2 relu(w0 c + b0)): the ReLU is a documented mask, so the element is planted where it is
    open and the claim is made for the hidden units that are open at entry t (pre-activation beyond 1e-3 in fp64): dw2[h, unit], dw0[unit, :]
    and db0[unit] are non-finite.  Locality: the other heads' rows of dw2, every other layer, every neighbour in the arena are
    bit-identical to the clean launch (this kernel sums without atomics: asserted by the guarded case above through two launches)."""
    picks = {}

    def planted(dtab, desc):
        dtab = dtab.clone()
        inside = [li for li in range(first, len(layers))]
        for li, v in zip((inside[0], inside[len(inside) // 2], inside[-1]), (INF, NAN, -INF)):
            ws, heads = layers[li]
            ts, t0 = (2 * ws - 1) ** 2, desc[8 * li + 6]
            h, t = heads - 1, ts // 3
            dtab[t0 + h * ts + t] = v
            picks[li] = (h, t)
        return dtab
    clean = cpb_batched_guarded(layers, first, upstream=lambda dtab, desc: dtab)[0]
    dirty, srcs_p, coords, coff = cpb_batched_guarded(layers, first, upstream=planted)
    assert len(picks) == 3
    for li, (ws, heads) in enumerate(layers):
        gc, gdirty = clean[2 * li], dirty[2 * li]
        assert finite(gc) and torch.equal(bits(clean[2 * li + 1]), bits(dirty[2 * li + 1])), f"the neighbour behind layer {li}"
        if li not in picks:
            assert torch.equal(bits(gc), bits(gdirty)), f"layer {li} holds no planted element"
            continue
        h, t = picks[li]
        ts = (2 * ws - 1) ** 2
        lp = srcs_p[2 * li].double()
        w0, b0 = lp[:1024].view(512, 2), lp[1024:1536]
        c = coords[coff[ws]:coff[ws] + 2 * ts].view(ts, 2).double()[t]
        pre = w0 @ c + b0
        opened = pre > 1e-3
        assert int(opened.sum()) > 32
        cut = lambda g: (g[:1024].view(512, 2), g[1024:1536], g[1536:].view(heads, 512))
        (dw0, db0, dw2), (cw0, cb0, cw2) = cut(gdirty), cut(gc)
        nf = lambda x: ~torch.isfinite(x)
        assert bool(nf(dw2[h])[opened].all()), f"layer {li}: dw2[{h}] is finite at {int((~nf(dw2[h]))[opened].sum())} open unit(s)"
        assert bool(nf(dw0)[opened].all()) and bool(nf(db0)[opened].all()), f"layer {li}: dw0 / db0 are finite at open units"
        others = [i for i in range(heads) if i != h]
        assert torch.equal(bits(dw2[others]), bits(cw2[others])), f"layer {li}: rows of dw2 of other heads differ from the clean launch"


def measure_margins():
    """prints, per class, the worst per-row ratio of the fp32-evaluated rounding model (two summation orders) to the fp64-evaluated one"""
    G.DEV = "cpu"
    worst = {}
    for li, (ws, heads) in enumerate(CPB_LAYERS + [(16, 24)]):
        coords = _cpb_coords(ws)
        for src, w2s in (("cpb_guarded", 0.05), ("cpb_batched_guarded", 0.05), ("a wider z", 0.3)):
            if src == "cpb_guarded":
                w0, b0, w2 = G.rnd(512, 2), G.rnd(512, seed=1, scale=0.5), G.rnd(heads, 512, seed=2, scale=w2s)
            else:
                w0, b0 = G.rnd(1024, seed=10 * li).view(512, 2), G.rnd(512, seed=10 * li + 1, scale=0.5)
                w2 = G.rnd(heads * 512, seed=10 * li + 2, scale=w2s).view(heads, 512)
            zex, tex = cpb_chain_model(coords, w0, b0, w2, exact=True)
            z64, t64 = cpb_chain_model(coords, w0, b0, w2)
            zs = _r32(zex)          # a stored z: the last step's operand
            s_ex, s64, s32 = cpb_sigmoid_model(zs, exact=True).t(), cpb_sigmoid_model(zs).t(), cpb_sigmoid_model(zs, dtype=F32).t()
            r, row = kc.row_model_excess(s32, s_ex, s64, 1.0)
            worst["cpb_sigmoid"] = max(worst.get("cpb_sigmoid", 0.0), r)
            print(f"cpb sigmoid ws {ws} heads {heads} inputs of {src}: ratio {r:.2f} (head {row})")
            for rev in (False, True):
                t32 = cpb_chain_model(coords, w0, b0, w2, dtype=F32, reverse=rev)[1]
                r, row = kc.row_model_excess(t32, tex, t64, 1.0)
                worst["cpb_chain"] = max(worst.get("cpb_chain", 0.0), r)
                print(f"cpb chain ws {ws} heads {heads} inputs of {src} reversed {rev}: ratio {r:.2f} (head {row})")
    for klass, half in (("16", torch.bfloat16), ("16", torch.float16), ("x3", None), ("f32", None)):
        cdt = half if klass == "16" else F32
        for case in G.ATTN_CASES:
            qkv, table, ls, dout = _attn_inputs(case, cdt)
            ex = attn_model(qkv, table, ls, dout, case, klass, half, exact=True)
            m64 = attn_model(qkv, table, ls, dout, case, klass, half)
            for rev in (False, True):
                m32 = attn_model(qkv, table, ls, dout, case, klass, half, dtype=F32, reverse=rev)
                for k in (0, 1):
                    n = ex[k].shape[-1]
                    r, row = kc.row_model_excess(m32[k].reshape(-1, n), ex[k].reshape(-1, n), m64[k].reshape(-1, n), 1.0)
                    key = "attn" + klass
                    worst[key] = max(worst.get(key, 0.0), r)
                    print(f"attn {klass} {half} {case} {'dqkv' if k else 'out'} reversed {rev}: ratio {r:.2f} (row {row})")
    for xdt in (F32, torch.bfloat16):
        for cond in (True, False):
            for B, L, C in CLN_SHAPES:
                x, res, t, ps, dout = _cln_inputs(xdt, B, L, C)
                args = (x, res, t, ps[0], ps[1], ps[2], ps[3], None, dout, cond, xdt)
                ex, m64 = cln_model(*args, exact=True), cln_model(*args)
                for rev in (False, True):
                    m32 = cln_model(*args, dtype=F32, reverse=rev)
                    for k in (0, 1):
                        r, row = kc.row_model_excess(m32[k].reshape(-1, C), ex[k].reshape(-1, C), m64[k].reshape(-1, C), 1.0)
                        worst["cln"] = max(worst.get("cln", 0.0), r)
                        print(f"cln {xdt} cond {cond} {(B, L, C)} {'dx' if k else 'out'} reversed {rev}: ratio {r:.2f} (row {row})")
    for k, v in worst.items():
        print(f"WORST {k}: {v:.2f}  -> MARGIN {2 * v:.2f}")


if __name__ == "__main__":
    import sys
    if "--measure-margins" in sys.argv:
        measure_margins()
