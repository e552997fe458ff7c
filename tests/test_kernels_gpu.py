"""GPU parity tests of every C-ABI kernel against a plain PyTorch reference of the same op (fp64 on the GPU).
Run on the MI355X box:  python -m pytest tests -m gpu -q
Tolerances: compute=f32 (exact fp32 MFMA) 2e-5 rel-L2; compute=bf16: operands are rounded to bf16 (2^-9), tolerance
stated per test (the reference is evaluated on the SAME bf16-rounded operands where that isolates kernel error)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from poseidon_amd import ops  # noqa: E402

DEV = "cuda"


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def rnd(*shape, dtype=torch.float32, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


def test_selftest_tr():
    l = ops.L()
    print("use_tr =", l.scot_get_use_tr())
    assert l.scot_get_use_tr() in (0, 1)


# ----------------------------------------------------------------------------------------------- GEMM
GEMM_SHAPES = [(304, 96, 96), (1024, 288, 96), (257, 130, 72), (4096, 384, 96), (64, 64, 3072), (1024, 768, 768), (65536, 96, 384), (520, 64, 40)]
# mixed = False: operands in the compute dtype (gemm_fast); True: fp32 B beside 16-bit A (generic kernel; exists in the 16-bit mode only)
GEMM_CASES = [(c, l, mx, *sh) for c in (ops.F32, ops.BF16) for l in (ops.NT, ops.NN, ops.TN) for mx in (False, True) for sh in GEMM_SHAPES
              if not (mx and (c == ops.F32 or sh[0] > 5000))]
# + the smallest shapes that select the rows of gemm_fast's tile table (csrc/gemm_fast.hip: kFastTiles) which the list above leaves out:
# 96 x 96 (TN, whole 96-tiles over >= 8192 tokens), four register sets in NT (K >= 2304 that is not whole 64-tiles), plain 64 x 64 in NT
GEMM_CASES += [(ops.BF16, ops.TN, False, 96, 96, 8192), (ops.BF16, ops.NT, False, 64, 64, 2312), (ops.BF16, ops.NT, False, 64, 64, 136)]


@pytest.mark.parametrize("compute,layout,mixed,M,N,K", GEMM_CASES)
def test_gemm_layouts(compute, layout, mixed, M, N, K):
    adt = torch.float32 if compute == ops.F32 else torch.bfloat16
    bdt = torch.float32 if mixed else adt
    if layout == ops.NT:
        A, B = rnd(M, K, dtype=adt), rnd(N, K, dtype=bdt, scale=0.1, seed=1)
    elif layout == ops.NN:
        A, B = rnd(M, K, dtype=adt), rnd(K, N, dtype=bdt, scale=0.1, seed=1)
    else:
        A, B = rnd(K, M, dtype=adt), rnd(K, N, dtype=bdt, scale=0.1, seed=1)
    Aq = A.double()
    Bq = (B.to(torch.bfloat16) if compute == ops.BF16 else B).double()  # reference on the operands the MFMA sees
    ref = (Aq @ Bq.t()) if layout == ops.NT else ((Aq @ Bq) if layout == ops.NN else (Aq.t() @ Bq))
    C = torch.zeros(M, N, device=DEV) if layout == ops.TN else torch.full((M, N), float("nan"), device=DEV)
    cs = torch.zeros(M if layout == ops.TN else N, device=DEV)
    ops.gemm(layout, compute, M, N, K, A, A.shape[1], B, B.shape[1], C, N, accumulate=(layout == ops.TN), colsum_out=cs)
    torch.cuda.synchronize()
    tol = 2e-5 if compute == ops.F32 else 2e-3
    assert rel(C, ref) < tol
    cs_ref = Aq.sum(0) if layout == ops.TN else C.double().sum(0)
    assert rel(cs, cs_ref) < 1e-4
    if layout != ops.TN:  # without the column-sum request small grids take the split-K + epilogue-pass route
        bias = rnd(N, seed=5)
        res = rnd(M, N, seed=6)
        C2 = torch.full((M, N), float("nan"), device=DEV)
        ops.gemm(layout, compute, M, N, K, A, A.shape[1], B, B.shape[1], C2, N, bias=bias, resid=res, ldres=N)
        assert rel(C2, ref + bias.double() + res.double()) < tol


# (M, N, K, variant): -1 = the library's own policy for the shape (Poseidon-B's deep stages, Poseidon-L, Poseidon-B at 256 x 256), else forced
WIDE_CASES = [(1024, 3072, 768, -1), (4096, 1536, 384, -1), (1024, 768, 3072, -1), (2048, 6144, 1536, -1), (8192, 768, 3072, -1), (32768, 384, 1536, -1),
              (2048, 1536, 1536, 0), (1024, 768, 768, 1), (256, 128, 64, 2), (128, 128, 1024, 0), (4096, 384, 384, 2)]


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("M,N,K,variant", WIDE_CASES)
def test_gemm_wide_tiles(kind, M, N, K, variant):
    """csrc/gemm_wide.hip: NT products on 128 x 128 tiles (three instantiations: 8 waves x 4 LDS stages, 8 x 2, 4 x 2).  Every epilogue form
    of the engine's calls against fp64 on the rounded operands, and against gemm_fast's 64 x 64 tiles (same products, another summation
    order); repeated launches are bit-identical."""
    prev = ops.use(kind)
    lib = ops.L()
    try:
        hd = ops.half_dtype()
        tol16 = 1.2e-3 if kind == "f16" else 6e-3
        x, w, b = rnd(M, K, dtype=hd), rnd(N, K, dtype=hd, scale=K ** -0.5, seed=1), rnd(N, seed=2)
        u = x.double() @ w.double().t() + b.double()
        lib.scot_gemm_wide_config(0, 0)
        y_fast = torch.empty(M, N, device=DEV)
        ops.linear_fwd(ops.BF16, x, w, y_fast, bias=b)
        lib.scot_gemm_wide_config(1 if variant < 0 else 2, max(variant, 0))
        y32, y16 = torch.full((M, N), float("nan"), device=DEV), torch.empty(M, N, device=DEV, dtype=hd)
        ops.linear_fwd(ops.BF16, x, w, y32, bias=b)
        ops.linear_fwd(ops.BF16, x, w, y16, bias=b)
        assert rel(y32, u) < 1e-5 and rel(y16, u) < tol16 and rel(y32, y_fast) < 2e-6
        for _ in range(5):
            y = torch.full((M, N), float("nan"), device=DEV)
            ops.linear_fwd(ops.BF16, x, w, y, bias=b)
            assert torch.equal(y, y32)
        gv, gd = torch.empty(M, N, device=DEV, dtype=hd), torch.empty(M, N, device=DEV, dtype=hd)
        ops.linear_fwd(ops.BF16, x, w, gv, bias=b, gelu_deriv_out=gd)
        assert rel(gv, torch.nn.functional.gelu(u)) < tol16
        assert rel(gd, 0.5 * (1 + torch.erf(u / math.sqrt(2))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)) < tol16
        if K % 128 == 0 and N % 64 == 0:      # the data gradients: dx[M, K] = dy[M, N] w[N, K] as an NT product on the transposed copy
            dy, wt, aux = rnd(M, N, dtype=hd, seed=3), w.t().contiguous(), rnd(M, K, dtype=hd, seed=4)
            dx = torch.empty(M, K, device=DEV, dtype=hd)
            ops.linear_dgrad(ops.BF16, dy, w, dx, aux=aux, aux_mul=True, wt=wt)
            assert rel(dx, (dy.double() @ w.double()) * aux.double()) < tol16
            g0 = rnd(M, K, seed=5)
            g = g0.clone()
            ops.linear_dgrad(ops.BF16, dy, w, g, accumulate=True, wt=wt)
            assert rel(g, g0.double() + dy.double() @ w.double()) < 1e-5
        torch.cuda.synchronize()
    finally:
        lib.scot_gemm_wide_config(1, 0)
        ops.use(prev)


@pytest.mark.parametrize("compute", [ops.F32, ops.BF16])
def test_gemm_epilogues(compute):
    M, N, K = 520, 192, 96
    cdt = torch.float32 if compute == ops.F32 else torch.bfloat16
    x, w, b = rnd(M, K, dtype=cdt), rnd(N, K, dtype=cdt, scale=0.1, seed=1), rnd(N, seed=2)
    tol = 2e-5 if compute == ops.F32 else 1e-2
    # fc1: u = x w^T + b (stored in compute dtype)
    u = torch.empty(M, N, device=DEV, dtype=cdt)
    ops.linear_fwd(compute, x, w, u, bias=b)
    ref_u = x.double() @ w.double().t() + b.double()
    assert rel(u, ref_u) < tol
    # fc2 with GELU on load: y = gelu(u) w2^T + b2, f32 out, + residual + colscale
    w2, b2, cs, res = rnd(K, N, dtype=cdt, scale=0.1, seed=3), rnd(K, seed=4), rnd(K, seed=5), rnd(M, K, seed=6)
    y = torch.empty(M, K, device=DEV)
    ops.gemm(ops.NT, compute, M, K, N, u, N, w2, N, y, K, bias=b2, colscale=cs, resid=res, ldres=K, a_gelu=True)
    g = torch.nn.functional.gelu(u.double())
    ref_y = (g @ w2.double().t() + b2.double()) * cs.double() + res.double()
    assert rel(y, ref_y) < tol
    # dgrad with gelu' epilogue: du = (dy w2) * gelu'(u); accumulate variant
    dy = rnd(M, K, dtype=cdt, seed=7)
    du = torch.empty(M, N, device=DEV, dtype=cdt)
    ops.linear_dgrad(compute, dy, w2, du, aux=u)
    ud = u.double()
    gp = 0.5 * (1 + torch.erf(ud / math.sqrt(2))) + ud * torch.exp(-0.5 * ud * ud) / math.sqrt(2 * math.pi)
    ref_du = (dy.double() @ w2.double()) * gp
    assert rel(du, ref_du) < tol
    acc = rnd(M, N, seed=8)
    acc0 = acc.clone()
    ops.linear_dgrad(compute, dy, w2, acc, accumulate=True)
    assert rel(acc, acc0.double() + dy.double() @ w2.double()) < tol
    # wgrad with GELU on the B operand: dw2 += dy^T gelu(u);  bias grad via colsum
    dw2 = torch.zeros(K, N, device=DEV)
    db = torch.zeros(K, device=DEV)
    ops.linear_wgrad(compute, dy, u, dw2, b_gelu=True, dbias=db)
    assert rel(dw2, dy.double().t() @ g) < tol
    assert rel(db, dy.double().sum(0)) < 1e-4
    db2 = torch.zeros(K, device=DEV)
    ops.colsum(dy, db2)
    assert rel(db2, dy.double().sum(0)) < 1e-5
    # fc1 with the dual epilogue: a = gelu(u), gp = gelu'(u);  dgrad with aux_mul multiplies by gp as is
    a_ = torch.empty(M, N, device=DEV, dtype=cdt)
    gp_ = torch.empty(M, N, device=DEV, dtype=cdt)
    ops.linear_fwd(compute, x, w, a_, bias=b, gelu_deriv_out=gp_)
    u64 = x.double() @ w.double().t() + b.double()
    gp64 = 0.5 * (1 + torch.erf(u64 / math.sqrt(2))) + u64 * torch.exp(-0.5 * u64 * u64) / math.sqrt(2 * math.pi)
    assert rel(a_, torch.nn.functional.gelu(u64)) < tol
    assert rel(gp_, gp64) < tol
    du2 = torch.empty(M, N, device=DEV, dtype=cdt)
    ops.linear_dgrad(compute, dy, w2, du2, aux=gp_, aux_mul=True)
    assert rel(du2, (dy.double() @ w2.double()) * gp_.double()) < tol


# ----------------------------------------------------------------------------------------------- attention
def _attn_ref(qkv, table, logit_scale, B, Hp, Wp, C, heads, ws, shift, hook=None, reverse=False):
    """fp64 torch restatement on [B, Hp*Wp, 3C] with roll/partition (HF:389-455, ref model.py:522-559).
    hook(name, tensor) -> tensor (optional) is called on the normalised q and k ("qk"), the logits ("s"), the probabilities ("p") and the
    result ("out"): the points where the kernels round (tests/test_kernels_guarded_gpu.py builds its rounding model from them);
    reverse: the three contractions are summed in the opposite order (only differs in finite precision)."""
    hk = hook if hook is not None else (lambda name, t: t)
    fl = (lambda t, dim: t.flip(dim)) if reverse else (lambda t, dim: t)
    N, d = ws * ws, C // heads
    x = qkv.view(B, Hp, Wp, 3 * C)
    if shift:
        x = torch.roll(x, (-shift, -shift), (1, 2))
    xw = x.view(B, Hp // ws, ws, Wp // ws, ws, 3 * C).permute(0, 1, 3, 2, 4, 5).reshape(-1, N, 3 * C)
    q, k, v = [t.reshape(-1, N, heads, d).transpose(1, 2) for t in xw.split(C, dim=-1)]
    qn = hk("qk", q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12))
    kn = hk("qk", k / k.norm(dim=-1, keepdim=True).clamp_min(1e-12))
    s = fl(qn, -1) @ fl(kn, -1).transpose(-1, -2) * torch.exp(torch.clamp(logit_scale, max=math.log(100.0))).view(1, heads, 1, 1)
    yy = torch.arange(ws, device=qkv.device).repeat_interleave(ws)
    xx = torch.arange(ws, device=qkv.device).repeat(ws)
    idx = (yy.view(-1, 1) - yy.view(1, -1) + ws - 1) * (2 * ws - 1) + (xx.view(-1, 1) - xx.view(1, -1) + ws - 1)
    s = s + table[:, idx.reshape(-1)].view(1, heads, N, N)
    if shift:
        ys, xs = torch.arange(Hp, device=qkv.device), torch.arange(Wp, device=qkv.device)
        ry = (ys >= Hp - ws).long() + (ys >= Hp - shift).long()
        rx = (xs >= Wp - ws).long() + (xs >= Wp - shift).long()
        rid = (ry.view(-1, 1) * 3 + rx.view(1, -1)).view(Hp // ws, ws, Wp // ws, ws).permute(0, 2, 1, 3).reshape(-1, N)
        m = (rid.unsqueeze(1) != rid.unsqueeze(2)).to(s.dtype) * (-200.0)
        nW = m.shape[0]
        s = (s.view(B, nW, heads, N, N) + m.view(1, nW, 1, N, N)).view(-1, heads, N, N)
    o = (fl(hk("p", torch.softmax(hk("s", s), -1)), -1) @ fl(v, -2)).transpose(1, 2).reshape(-1, ws, ws, C)
    o = o.view(B, Hp // ws, Wp // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    return hk("out", o.reshape(B, Hp * Wp, C))


ATTN_CASES = [  # B, Hp, Wp, C, heads, ws, shift
    (2, 32, 32, 96, 3, 16, 8),    # Poseidon-B stage 0 (head_dim 32, N=256, shifted)
    (2, 32, 32, 48, 3, 16, 0),    # Poseidon-T stage 0 (head_dim 16)
    (1, 16, 16, 128, 2, 16, 0),   # head_dim 64 (Poseidon-L), N=256
    (1, 32, 32, 96, 3, 16, 0),    # 16x16 fast path, unshifted, 2x2 windows
    (2, 32, 32, 48, 3, 16, 8),    # 16x16 fast path, head_dim 16, shifted
    (1, 48, 32, 96, 3, 16, 8),    # 16x16 fast path, 3x2 windows: interior / last-row / last-column mask regions
    (1, 32, 48, 128, 2, 16, 8),   # 16x16 fast path, head_dim 64, 2x3 windows
    (3, 8, 8, 64, 2, 8, 0),       # N=64
    (2, 8, 8, 32, 2, 4, 2),       # N=16 shifted
    (2, 4, 4, 128, 2, 4, 0),      # N=16, head_dim 64
    (1, 14, 14, 32, 1, 7, 3),     # N=49 (not a multiple of 16) shifted
]


@pytest.mark.parametrize("compute", [ops.F32, ops.BF16, ops.X3, "f16"])
@pytest.mark.parametrize("case", ATTN_CASES)
def test_window_attention_fwd_bwd(compute, case):
    """"f16": the 16-bit kernels in the binary16 build of the library (the product's default operand format)."""
    f16 = compute == "f16"
    prev = ops.use("f16" if f16 else "bf16")
    try:
        _window_attention_fwd_bwd(ops.BF16 if f16 else compute, case, torch.float16 if f16 else torch.bfloat16)
    finally:
        ops.use(prev)


def _window_attention_fwd_bwd(compute, case, half):
    B, Hp, Wp, C, heads, ws, shift = case
    cdt = half if compute == ops.BF16 else torch.float32     # bf16x3 keeps fp32 tensors and splits inside the kernel
    L, TS, N = Hp * Wp, (2 * ws - 1) ** 2, ws * ws
    qkv = rnd(B, L, 3 * C, dtype=cdt)
    table = (16 * torch.sigmoid(rnd(heads, TS, seed=1))).contiguous()
    ls = torch.linspace(math.log(3.0), math.log(20.0), heads, device=DEV)
    dout = rnd(B, L, C, dtype=cdt, seed=2)
    out = torch.full((B, L, C), float("nan"), device=DEV, dtype=cdt)
    nW = (Hp // ws) * (Wp // ws)
    lse = torch.empty(B * nW, heads, N, device=DEV)
    ops.window_attn_fwd(compute, qkv, out, lse, table, ls, B, Hp, Wp, C, heads, ws, shift)
    dqkv = torch.full((B, L, 3 * C), float("nan"), device=DEV, dtype=cdt)
    dtab = torch.zeros(heads, TS, device=DEV)
    dls = torch.zeros(heads, device=DEV)
    ops.window_attn_bwd(compute, qkv, out, dout, lse, table, ls, dqkv, dtab, dls, B, Hp, Wp, C, heads, ws, shift)
    torch.cuda.synchronize()

    q64 = qkv.double().requires_grad_(True)
    t64 = table.double().requires_grad_(True)
    l64 = ls.double().requires_grad_(True)
    ref = _attn_ref(q64, t64, l64, B, Hp, Wp, C, heads, ws, shift)
    ref.backward(dout.double())
    # 16-bit operands: q/k (normalised), P and dS are rounded to the operand format inside the kernel.  Measured over these cases on
    # MI355X (tools/probes/attn_err_probe.py): bf16 out <= 5.3e-3, dqkv <= 7.8e-3, dtab <= 6.4e-3, dls <= 5.9e-2; binary16 out <= 6.4e-4,
    # dqkv <= 1.1e-3, dtab <= 7.8e-4, dls <= 8.4e-3 — bounds at ~1.5-2x of that
    t16 = ((1.2e-3, 2e-3), 2e-2) if half == torch.float16 else ((8e-3, 1.2e-2), 0.1)
    tol_o, tol_g = (2e-5, 5e-5) if compute == ops.F32 else (5e-5, 2e-4) if compute == ops.X3 else t16[0]
    tol_ls = 2e-4 if compute == ops.F32 else 2e-3 if compute == ops.X3 else t16[1]  # Σ_k dS = 0: d logit_scale is a heavily cancelling sum
    assert rel(out, ref.detach()) < tol_o, "out"
    assert rel(dqkv, q64.grad) < tol_g, "dqkv"
    assert rel(dtab, t64.grad) < tol_g, "dbias_table"
    # d logit_scale is a heavily cancelling sum over all (q,k) pairs: bf16 operand rounding shows up amplified
    assert rel(dls, l64.grad) < tol_ls, "dlogit_scale"
    # the replica entry (window w accumulates into replica w % R of both buffers) + the fold: same sums in another order
    R, pad = 3, 5
    st, sl = heads * TS + pad, heads + pad
    rt, rl = torch.zeros(R * st, device=DEV), torch.zeros(R * sl, device=DEV)
    dq2 = torch.empty_like(dqkv)
    ops.window_attn_bwd_rep(compute, qkv, out, dout, lse, table, ls, dq2, rt, rl, B, Hp, Wp, C, heads, ws, shift, R, st, sl)
    assert torch.equal(dq2, dqkv)
    used = {w % R for w in range(B * nW)}
    assert all((rt[r * st:(r + 1) * st].abs().sum() > 0) == (r in used) for r in range(R))
    dst = torch.zeros(heads + 2, device=DEV)
    ops.replica_reduce(rt, 1, R, st, torch.tensor([0, 0, heads * TS], dtype=torch.int32, device=DEV), 1, heads * TS, rt)
    ops.replica_reduce(rl, 0, R, sl, torch.tensor([0, 2, heads], dtype=torch.int32, device=DEV), 1, heads, dst)
    torch.cuda.synchronize()
    assert rel(rt[:heads * TS].view(heads, TS), dtab) < 1e-5 and rel(dst[2:], dls) < 5e-4 and torch.all(dst[:2] == 0)


# ----------------------------------------------------------------------------------------------- CLN
@pytest.mark.parametrize("cond", [True, False])
@pytest.mark.parametrize("xdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,L,C", [(3, 64, 96), (2, 16, 768), (2, 9, 20), (2, 300, 48), (2, 1024, 192), (2, 5, 1536), (3, 33, 16), (64, 16, 768),
                                   (64, 64, 384), (5, 6, 128)])
def test_cln_fwd_bwd(cond, xdt, B, L, C):
    x = rnd(B, L, C, dtype=xdt)
    res = rnd(B, L, C, seed=1)
    t = torch.rand(B, device=DEV)
    gw_w, gw_b, bw_w, bw_b = rnd(C, seed=2, scale=0.3), 1 + rnd(C, seed=3, scale=0.1), rnd(C, seed=4, scale=0.1), rnd(C, seed=5, scale=0.1)
    out = torch.empty(B, L, C, device=DEV)
    out16 = torch.empty(B, L, C, device=DEV, dtype=torch.bfloat16)
    mean, rstd = torch.empty(B * L, device=DEV), torch.empty(B * L, device=DEV)
    ops.cln_fwd(x, res, out, mean, rstd, t if cond else None, gw_w if cond else None, gw_b, bw_w if cond else None, bw_b,
                B * L, L, C, 1e-5, out2=out16)
    dout = rnd(B, L, C, seed=6)
    dx = torch.empty(B, L, C, device=DEV, dtype=xdt)
    grads = [torch.zeros(C, device=DEV) for _ in range(4)]
    dxb = torch.zeros(C, device=DEV)
    ops.cln_bwd(dout, x, mean, rstd, t if cond else None, gw_w if cond else None, gw_b, dx, grads[0], grads[1], grads[2],
                grads[3], B * L, L, C, d_xbias=dxb)
    torch.cuda.synchronize()
    assert torch.equal(out16, out.to(torch.bfloat16))
    x64 = x.double().requires_grad_(True)
    ps = [p.double().requires_grad_(True) for p in (gw_w, gw_b, bw_w, bw_b)]
    mu = x64.mean(-1, keepdim=True)
    var = (x64 * x64).mean(-1, keepdim=True) - mu * mu
    xh = (x64 - mu) / torch.sqrt(var + 1e-5)
    if cond:
        g = t.double().view(B, 1, 1) * ps[0] + ps[1]
        b = t.double().view(B, 1, 1) * ps[2] + ps[3]
    else:
        g, b = ps[1], ps[3]
    ref = res.double() + g * xh + b
    ref.backward(dout.double())
    assert rel(out, ref.detach()) < 1e-5
    assert rel(dx, x64.grad) < (1e-4 if xdt == torch.float32 else 1e-2)
    assert rel(dxb, x64.grad.sum((0, 1))) < (2e-3 if xdt == torch.float32 else 5e-2)
    for i in ([0, 1, 2, 3] if cond else [1, 3]):
        assert rel(grads[i], ps[i].grad) < 1e-4, i

    # mode 3 (the deep stages' form): dx + per-block partial sums, finished into CONTIGUOUS parameter gradients by a second launch
    nf = ops.cln_bwd_partial_floats(B * L, L, C, cond)
    assert (nf > 0) == (C % 64 == 0 and 128 <= C <= 1536 and B * L <= 8192)
    if nf:
        part = torch.full((nf,), float("nan"), device=DEV)
        dx3 = torch.empty(B, L, C, dtype=xdt, device=DEV)
        flat = torch.zeros(4 * C, device=DEV) + 0.25                      # += semantics: starts non-zero
        g3 = [flat[i * C:(i + 1) * C] for i in range(4)] if cond else [None, flat[0:C], None, flat[C:2 * C]]
        ops.cln_bwd(dout, x, mean, rstd, t if cond else None, gw_w if cond else None, gw_b, dx3, None, None, None, None, B * L, L, C,
                    sample_scale=None, mode=3, partial=part)
        ops.cln_bwd_finish(part, B * L, L, C, g3[0], g3[1], g3[2], g3[3])
        torch.cuda.synchronize()
        assert torch.equal(dx3, dx) or rel(dx3, dx) < 1e-6
        for i in ([0, 1, 2, 3] if cond else [1, 3]):
            assert rel(g3[i] - 0.25, ps[i].grad) < 1e-4, i


# ----------------------------------------------------------------------------------------------- fused MLP block (experimental)
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("cond", [True, False])
@pytest.mark.parametrize("B,L,C", [(2, 1024, 96), (3, 200, 96), (64, 1024, 96), (2, 256, 192), (5, 72, 192)])
def test_mlp_block_fused(train, cond, B, L, C):
    """scot_mlp_block_fwd vs the three validated launches it replaces (fc1 + GELU epilogue, fc2, cond-LN + residual) on the
    same operands — both round gelu(u) to bf16 before fc2, so they agree to accumulation order — and vs an fp64 reference."""
    M, hid = B * L, 4 * C
    bf = torch.bfloat16
    h = rnd(M, C, seed=1)
    h16 = h.to(bf)
    w1, b1 = rnd(hid, C, scale=C ** -0.5, seed=2).to(bf), rnd(hid, seed=3, scale=0.2)
    w2, b2 = rnd(C, hid, scale=hid ** -0.5, seed=4).to(bf), rnd(C, seed=5, scale=0.2)
    t = torch.rand(B, device=DEV)
    sc = (torch.rand(B, device=DEV) > 0.3).float() / 0.7
    gw_w, gw_b, bw_w, bw_b = rnd(C, seed=6, scale=0.3), 1 + rnd(C, seed=7, scale=0.1), rnd(C, seed=8, scale=0.1), rnd(C, seed=9, scale=0.1)
    cw = (gw_w, bw_w) if cond else (None, None)
    # three-kernel path
    u = torch.empty(M, hid, device=DEV, dtype=bf)
    gp = torch.empty(M, hid, device=DEV, dtype=bf)
    ops.linear_fwd(ops.BF16, h16, w1, u, bias=b1, gelu_deriv_out=gp if train else u)
    z = torch.empty(M, C, device=DEV)
    ops.linear_fwd(ops.BF16, u, w2, z, bias=b2)
    out, out16 = torch.empty(M, C, device=DEV), torch.empty(M, C, device=DEV, dtype=bf)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    ops.cln_fwd(z, h, out, mean, rstd, t if cond else None, cw[0], gw_b, cw[1], bw_b, M, L, C, 1e-5, out2=out16, sample_scale=sc)
    # fused
    fu = torch.full((M, hid), float("nan"), device=DEV, dtype=bf) if train else None
    fgp = torch.full((M, hid), float("nan"), device=DEV, dtype=bf) if train else None
    fz = torch.full((M, C), float("nan"), device=DEV) if train else None
    fmean = torch.full((M,), float("nan"), device=DEV) if train else None
    frstd = torch.full((M,), float("nan"), device=DEV) if train else None
    fout, fout16 = torch.full((M, C), float("nan"), device=DEV), torch.full((M, C), float("nan"), device=DEV, dtype=bf)
    assert ops.mlp_block_fwd(h16, h, w1, b1, w2, b2, fout, fout16, fu, fgp, fz, fmean, frstd, t if cond else None, cw[0], gw_b, cw[1],
                             bw_b, sc, M, L, C, hid, 1e-5)
    torch.cuda.synchronize()
    assert torch.isfinite(fout).all() and torch.isfinite(fout16.float()).all()
    assert rel(fout, out) < 2e-5
    assert torch.equal(fout16, fout.to(bf))
    if train:
        # same fp32 accumulators up to summation order, then one bf16 rounding: a last-bit flip on a few elements at most
        assert rel(fu.float(), u.float()) < 1e-3 and rel(fgp.float(), gp.float()) < 1e-3
        assert rel(fz, z) < 2e-5 and rel(fmean, mean) < 1e-4 and rel(frstd, rstd) < 1e-4
    # fp64 reference on the same bf16 operands (gelu output rounded to bf16, as both kernel paths do)
    a = torch.nn.functional.gelu(h16.double() @ w1.double().T + b1.double()).to(bf).double()
    zr = a @ w2.double().T + b2.double()
    mu, var = zr.mean(-1, keepdim=True), zr.var(-1, unbiased=False, keepdim=True)
    xh = ((zr - mu) / torch.sqrt(var + 1e-5)).view(B, L, C)
    tt = t.double().view(B, 1, 1)
    g = tt * gw_w.double() + gw_b.double() if cond else gw_b.double()
    b = tt * bw_w.double() + bw_b.double() if cond else bw_b.double()
    ref = h.double().view(B, L, C) + sc.double().view(B, 1, 1) * (g * xh + b)
    assert rel(fout.view(B, L, C), ref) < 2e-3      # bf16 rounding of gelu(u) right at a rounding boundary differs from fp64's


@pytest.mark.parametrize("cond", [True, False])
@pytest.mark.parametrize("B,L,C", [(2, 1024, 96), (3, 192, 96), (64, 1024, 96), (2, 256, 192), (5, 64, 192)])
def test_mlp_block_bwd_fused(cond, B, L, C):
    """scot_mlp_block_bwd vs the three validated launches it replaces (cond-LN backward, dgrad fc2 with the gelu' multiply,
    dgrad fc1 accumulated into g) on the same operands."""
    M, hid = B * L, 4 * C
    bf = torch.bfloat16
    g = rnd(M, C, seed=1)
    z = rnd(M, C, seed=2, scale=1.5) + 0.3
    mean = z.mean(-1)
    rstd = 1.0 / torch.sqrt(z.var(-1, unbiased=False) + 1e-5)
    gp = rnd(M, hid, seed=3, scale=0.5).to(bf)
    w1 = rnd(hid, C, scale=C ** -0.5, seed=4).to(bf)
    w2 = rnd(C, hid, scale=hid ** -0.5, seed=5).to(bf)
    t = torch.rand(B, device=DEV)
    sc = (torch.rand(B, device=DEV) > 0.3).float() / 0.7
    gw_w, gw_b = rnd(C, seed=6, scale=0.3), 1 + rnd(C, seed=7, scale=0.1)
    # three-kernel path
    dz = torch.empty(M, C, device=DEV, dtype=bf)
    grads = [torch.zeros(C, device=DEV) for _ in range(4)]
    ops.cln_bwd(g, z, mean, rstd, t if cond else None, gw_w if cond else None, gw_b, dz, grads[0], grads[1], grads[2], grads[3],
                M, L, C, sample_scale=sc)
    du = torch.empty(M, hid, device=DEV, dtype=bf)
    ops.linear_dgrad(ops.BF16, dz, w2, du, aux=gp, aux_mul=True)
    gh = g.clone()
    ops.linear_dgrad(ops.BF16, du, w1, gh, accumulate=True)
    # fused (out of place, then in place)
    fdz = torch.full((M, C), float("nan"), device=DEV, dtype=bf)
    fdu = torch.full((M, hid), float("nan"), device=DEV, dtype=bf)
    fgh = torch.full((M, C), float("nan"), device=DEV)
    fgr = [torch.zeros(C, device=DEV) for _ in range(4)]
    assert ops.mlp_block_bwd(g, fgh, z, mean, rstd, t if cond else None, gw_w if cond else None, gw_b, sc, gp, w1, w2, fdz, fdu,
                             fgr[0] if cond else None, fgr[1], fgr[2] if cond else None, fgr[3], M, L, C, hid)
    gi = g.clone()
    assert ops.mlp_block_bwd(gi, gi, z, mean, rstd, t if cond else None, gw_w if cond else None, gw_b, sc, gp, w1, w2,
                             torch.empty_like(fdz), torch.empty_like(fdu), None if not cond else torch.zeros(C, device=DEV),
                             torch.zeros(C, device=DEV), None if not cond else torch.zeros(C, device=DEV), torch.zeros(C, device=DEV),
                             M, L, C, hid)
    torch.cuda.synchronize()
    assert torch.isfinite(fgh).all()
    assert rel(fdz.float(), dz.float()) < 1e-3            # one bf16 rounding of values that agree to fp32 summation order
    assert rel(fdu.float(), du.float()) < 5e-3            # du inherits dz's last-bit flips through a K = C contraction
    assert rel(fgh, gh) < 1e-3
    assert torch.equal(gi, fgh)                           # in place == out of place
    for i in ([0, 1, 2, 3] if cond else [1, 3]):
        assert rel(fgr[i], grads[i]) < 1e-4, i
    # fp64 reference of the whole chain on the same operands
    d = (g.double() * sc.double().repeat_interleave(L).view(M, 1))
    gam = (t.double().repeat_interleave(L).view(M, 1) * gw_w.double() + gw_b.double()) if cond else gw_b.double()
    xh = (z.double() - mean.double().view(M, 1)) * rstd.double().view(M, 1)
    gd = d * gam
    rdz = rstd.double().view(M, 1) * (gd - gd.mean(-1, keepdim=True) - xh * (gd * xh).mean(-1, keepdim=True))
    rdu = (rdz @ w2.double()) * gp.double()
    rgh = g.double() + rdu @ w1.double()
    assert rel(fdz.float(), rdz) < 6e-3 and rel(fdu.float(), rdu) < 1e-2 and rel(fgh, rgh) < 5e-3


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("cond", [True, False])
@pytest.mark.parametrize("B,L,C", [(2, 1024, 96), (3, 200, 96), (64, 1024, 96), (2, 256, 192), (5, 72, 192)])
def test_proj_cln_fused(train, cond, B, L, C):
    """scot_proj_cln_fwd vs linear_fwd + cln_fwd on the same operands."""
    M = B * L
    bf = torch.bfloat16
    a = rnd(M, C, seed=1).to(bf)
    x = rnd(M, C, seed=2)
    w, bias = rnd(C, C, scale=C ** -0.5, seed=3).to(bf), rnd(C, seed=4, scale=0.2)
    t = torch.rand(B, device=DEV)
    sc = (torch.rand(B, device=DEV) > 0.3).float() / 0.7
    gw_w, gw_b, bw_w, bw_b = rnd(C, seed=6, scale=0.3), 1 + rnd(C, seed=7, scale=0.1), rnd(C, seed=8, scale=0.1), rnd(C, seed=9, scale=0.1)
    cw = (gw_w, bw_w) if cond else (None, None)
    z = torch.empty(M, C, device=DEV)
    ops.linear_fwd(ops.BF16, a, w, z, bias=bias)
    out, out16 = torch.empty(M, C, device=DEV), torch.empty(M, C, device=DEV, dtype=bf)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    ops.cln_fwd(z, x, out, mean, rstd, t if cond else None, cw[0], gw_b, cw[1], bw_b, M, L, C, 1e-5, out2=out16, sample_scale=sc)
    nan = float("nan")
    fz = torch.full((M, C), nan, device=DEV) if train else None
    fmean = torch.full((M,), nan, device=DEV) if train else None
    frstd = torch.full((M,), nan, device=DEV) if train else None
    fout, fout16 = torch.full((M, C), nan, device=DEV), torch.full((M, C), nan, device=DEV, dtype=bf)
    assert ops.proj_cln_fwd(a, w, bias, x, fout, fout16, fz, fmean, frstd, t if cond else None, cw[0], gw_b, cw[1], bw_b, sc, M, L, C, 1e-5)
    torch.cuda.synchronize()
    assert torch.isfinite(fout).all()
    assert rel(fout, out) < 2e-5 and torch.equal(fout16, fout.to(bf))
    if train:
        assert rel(fz, z) < 2e-5 and rel(fmean, mean) < 1e-4 and rel(frstd, rstd) < 1e-4


@pytest.mark.parametrize("cond", [True, False])
@pytest.mark.parametrize("B,L,C", [(2, 1024, 96), (3, 192, 96), (64, 1024, 96), (2, 256, 192), (5, 64, 192)])
def test_proj_cln_bwd_fused(cond, B, L, C):
    """scot_proj_cln_bwd vs cln_bwd + linear_dgrad on the same operands."""
    M = B * L
    bf = torch.bfloat16
    g = rnd(M, C, seed=1)
    z = rnd(M, C, seed=2, scale=1.5) + 0.3
    mean = z.mean(-1)
    rstd = 1.0 / torch.sqrt(z.var(-1, unbiased=False) + 1e-5)
    w = rnd(C, C, scale=C ** -0.5, seed=4).to(bf)
    t = torch.rand(B, device=DEV)
    sc = (torch.rand(B, device=DEV) > 0.3).float() / 0.7
    gw_w, gw_b = rnd(C, seed=6, scale=0.3), 1 + rnd(C, seed=7, scale=0.1)
    dz = torch.empty(M, C, device=DEV, dtype=bf)
    grads = [torch.zeros(C, device=DEV) for _ in range(4)]
    ops.cln_bwd(g, z, mean, rstd, t if cond else None, gw_w if cond else None, gw_b, dz, grads[0], grads[1], grads[2], grads[3],
                M, L, C, sample_scale=sc)
    da = torch.empty(M, C, device=DEV, dtype=bf)
    ops.linear_dgrad(ops.BF16, dz, w, da)
    fdz = torch.full((M, C), float("nan"), device=DEV, dtype=bf)
    fda = torch.full((M, C), float("nan"), device=DEV, dtype=bf)
    fgr = [torch.zeros(C, device=DEV) for _ in range(4)]
    assert ops.proj_cln_bwd(g, z, mean, rstd, t if cond else None, gw_w if cond else None, gw_b, sc, w, fdz, fda,
                            fgr[0] if cond else None, fgr[1], fgr[2] if cond else None, fgr[3], M, L, C)
    torch.cuda.synchronize()
    assert torch.isfinite(fda.float()).all()
    assert rel(fdz.float(), dz.float()) < 1e-3 and rel(fda.float(), da.float()) < 5e-3
    for i in ([0, 1, 2, 3] if cond else [1, 3]):
        assert rel(fgr[i], grads[i]) < 1e-4, i


# ----------------------------------------------------------------------------------------------- data movement
def test_copy2d_pad_crop():
    B, H, W, C = 2, 5, 7, 12
    x = rnd(B, H, W, C)
    pad = torch.empty(B, 8, 8, C, device=DEV)
    ops.copy2d(x, pad, B, H, W, 8, 8, C)
    ref = torch.nn.functional.pad(x, (0, 0, 0, 1, 0, 3))
    assert torch.equal(pad, ref)
    crop = torch.empty(B, 4, 6, C, device=DEV)
    ops.copy2d(x, crop, B, H, W, 4, 6, C)
    assert torch.equal(crop, x[:, :4, :6].contiguous())


@pytest.mark.parametrize("C", [6, 16, 96])        # 6: element-wise kernel; multiples of 8: eight channels per thread
@pytest.mark.parametrize("H,W", [(8, 8), (9, 5)])
def test_space_depth(H, W, C):
    B = 2
    a, b = rnd(B, H, W, C), rnd(B, H, W, C, seed=1)
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    co = torch.empty(B, H2, W2, 4 * C, device=DEV)
    ops.space_to_depth(a, b, co, B, H, W, C, 0)
    s = torch.nn.functional.pad(a + b, (0, 0, 0, W % 2, 0, H % 2))
    ref = torch.cat([s[:, 0::2, 0::2], s[:, 1::2, 0::2], s[:, 0::2, 1::2], s[:, 1::2, 1::2]], -1)
    assert torch.equal(co, ref)
    # scatter back (gradient of merge): each fine position receives its own slice
    fine = torch.empty(B, H, W, C, device=DEV)
    ops.depth_to_space(co, fine, B, H, W, H2, W2, C, 0)
    assert torch.equal(fine, a + b)
    # order 1 = pixel shuffle of the unmerge (model.py:748-756) incl. crop
    z = rnd(B, H2, W2, 4 * C, seed=2)
    fine2 = torch.empty(B, H, W, C, device=DEV)
    ops.depth_to_space(z, fine2, B, H, W, H2, W2, C, 1)
    ref2 = z.view(B, H2, W2, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H2, 2 * W2, C)[:, :H, :W]
    assert torch.equal(fine2, ref2.contiguous())
    back = torch.empty(B, H2, W2, 4 * C, device=DEV)
    ops.space_to_depth(fine2, None, back, B, H, W, C, 1)
    mask = torch.zeros(B, 2 * H2, 2 * W2, C, device=DEV)
    mask[:, :H, :W] = 1
    mref = (z.view(B, H2, W2, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H2, 2 * W2, C) * mask)
    mref = mref.view(B, H2, 2, W2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H2, W2, 4 * C)
    assert torch.equal(back, mref)


@pytest.mark.parametrize("H,W,Cc,cdt", [(16, 16, 3, torch.float32), (18, 14, 3, torch.float32), (128, 128, 4, torch.float32),
                                        (64, 32, 5, torch.bfloat16)])     # unpadded p = 4 grids take the LDS-staged strip kernel
def test_patchify_unpatchify(H, W, Cc, cdt):
    B, p = 2, 4
    img = rnd(B, Cc, H, W)
    gh, gw = (H + p - 1) // p, (W + p - 1) // p
    cols = torch.full((B * gh * gw, Cc * p * p), float("nan"), device=DEV, dtype=cdt)
    ops.patchify(img, cols, B, Cc, H, W, p)
    padded = torch.nn.functional.pad(img, (0, gw * p - W, 0, gh * p - H))
    ref = padded.view(B, Cc, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, Cc * p * p)
    assert torch.equal(cols, ref.to(cdt))
    if cdt != torch.float32:
        return
    bias = rnd(Cc, seed=1)
    back = torch.empty(B, Cc, H, W, device=DEV)
    ops.unpatchify(cols, bias, back, B, Cc, H, W, gh, gw, p)
    assert torch.allclose(back, img + bias.view(1, -1, 1, 1))


@pytest.mark.parametrize("M,N", [(65536 + 37, 96), (4099, 48), (1024, 768), (300, 2048), (129, 8), (777, 200), (513, 100)])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_colsum_shapes(M, N, dt):
    """`scot_colsum` (bias / layer-scale gradients): the 8-column vector form (N % 8 == 0) and the scalar form, ragged row counts,
    both operand types, with and without the elementwise factor; the result is ADDED to `out`."""
    if DEV == "cpu" and M > 8192:                       # the CPU emulation of the kernels (tests/hipemu)
        M = 2048 + 37
    a, b = rnd(M, N, dtype=dt), rnd(M, N, seed=1, dtype=dt)
    o = torch.ones(N, device=DEV)
    ops.colsum(a, o)
    assert rel(o, 1 + a.double().sum(0)) < 2e-5
    o = torch.zeros(N, device=DEV)
    ops.colsum(a, o, y=b)
    assert rel(o, (a.double() * b.double()).sum(0)) < 2e-5


def test_reductions_and_scale_residual():
    B, Cc, HW = 3, 4, 1000
    x = rnd(B, Cc, HW)
    out = torch.zeros(Cc, device=DEV)
    ops.nchw_channel_sum(x, out, B, Cc, HW)
    assert rel(out, x.double().sum((0, 2))) < 1e-5
    M, N = 777, 200
    a, b = rnd(M, N, dtype=torch.bfloat16), rnd(M, N, seed=1)
    o1 = torch.zeros(N, device=DEV)
    ops.colsum(a, o1)
    assert rel(o1, a.double().sum(0)) < 1e-5
    a32 = a.float()
    o2 = torch.zeros(N, device=DEV)
    ops.colsum(a32, o2, y=b)
    assert rel(o2, (a.double() * b.double()).sum(0)) < 1e-5
    sc = rnd(N, seed=2)
    o3 = torch.empty(M, N, device=DEV)
    ops.scale_residual(a, sc, b, o3, M, N)
    assert rel(o3, b.double() + sc.double() * a.double()) < 1e-6
    pe = rnd(N, seed=3)
    o4 = torch.empty(M, N, device=DEV)
    ops.add(b, pe, o4, period=N)
    assert torch.allclose(o4, b + pe)
    o5 = torch.zeros(HW, device=DEV)
    ops.batch_sum(x.view(B * Cc, HW), o5, B * Cc, HW)
    assert rel(o5, x.double().sum((0, 1))) < 1e-5


# ----------------------------------------------------------------------------------------------- stencils
@pytest.mark.parametrize("H,W,C,B", [(16, 16, 96, 2), (5, 5, 24, 2), (40, 40, 64, 24)])   # last: 25 tiles per sample, all walked by ONE wgrad workgroup per (32 channels, sample) — the entry point fixes its tile groups at one
def test_dwconv7(H, W, C, B):
    x = rnd(B, H, W, C)
    w, bias = rnd(C, 1, 7, 7, seed=1, scale=0.2), rnd(C, seed=2)
    y = torch.empty(B, H, W, C, device=DEV)
    ops.dwconv7(x, w, bias, y, B, H, W, C)
    x64 = x.double().requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), bias.double().requires_grad_(True)
    ref = torch.nn.functional.conv2d(x64.permute(0, 3, 1, 2), w64, b64, padding=3, groups=C).permute(0, 2, 3, 1)
    dy = rnd(B, H, W, C, seed=3)
    ref.backward(dy.double())
    assert rel(y, ref.detach()) < 1e-5
    dx = torch.empty(B, H, W, C, device=DEV)
    ops.dwconv7(dy, w, None, dx, B, H, W, C, flip=True)
    assert rel(dx, x64.grad) < 1e-5
    dw, db = torch.zeros(C, 1, 7, 7, device=DEV), torch.zeros(C, device=DEV)
    ops.dwconv7_wgrad(dy, x, dw, db, B, H, W, C)
    assert rel(dw, w64.grad) < 1e-5
    assert rel(db, b64.grad) < 1e-5


@pytest.mark.parametrize("Cc,H,W", [(4, 32, 32), (5, 13, 10), (4, 128, 128), (1, 20, 132), (6, 9, 9)])   # tiled kernel: Cc <= 5 (ragged tiles, 2 column tiles); 6: per-pixel fallback
def test_conv5(Cc, H, W):
    B = 2
    x, w = rnd(B, Cc, H, W), rnd(Cc, Cc, 5, 5, seed=1, scale=0.2)
    y = torch.empty(B, Cc, H, W, device=DEV)
    ops.conv5(x, w, y, B, Cc, H, W)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    ref = torch.nn.functional.conv2d(x64, w64, None, padding=2)
    dy = rnd(B, Cc, H, W, seed=2)
    ref.backward(dy.double())
    assert rel(y, ref.detach()) < 1e-5
    dx = torch.empty(B, Cc, H, W, device=DEV)
    ops.conv5(dy, w, dx, B, Cc, H, W, transpose=True)
    assert rel(dx, x64.grad) < 1e-5
    dw = torch.zeros(Cc, Cc, 5, 5, device=DEV)
    ops.conv5_wgrad(dy, x, dw, B, Cc, H, W)
    assert rel(dw, w64.grad) < 1e-5


# ----------------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize("p,groups,resid,mask", [(1, [0, 1, 3, 4], False, False), (2, None, False, False),
                                                  (1, [0, 1, 3, 4], True, True), (2, [0, 2, 4], False, True)])
def test_head_finalize_loss(p, groups, resid, mask):
    B, Cc, H, W = 3, 4, 16, 16
    pred0, lab, pv = rnd(B, Cc, H, W), rnd(B, Cc, H, W, seed=1), rnd(B, 5, H, W, seed=2)
    pm = torch.zeros(B, Cc, dtype=torch.bool, device=DEV)
    pm[:, -1] = True
    G = len(groups) - 1 if groups else 1
    goc = torch.full((Cc,), -1, dtype=torch.int32)
    cnt = torch.zeros(G)
    if groups:
        for g in range(G):
            goc[groups[g]:groups[g + 1]] = g
            cnt[g] = B * (groups[g + 1] - groups[g]) * H * W
    else:
        goc[:] = 0
        cnt[0] = B * Cc * H * W
    goc, cnt = goc.to(DEV), cnt.to(DEV)
    pred = pred0.clone()
    sums = torch.zeros(2 * G, device=DEV)
    loss = torch.zeros(1, device=DEV)
    ops.head_finalize(pred, pv if resid else None, 5, lab, pm.to(torch.uint8) if mask else None, False, goc, sums, B, Cc, H * W, p)
    ops.loss_finish(sums, cnt, G, groups is not None, loss)
    dpred = torch.empty_like(pred)
    ops.loss_bwd(pred, lab, pm.to(torch.uint8) if mask else None, False, goc, sums, cnt, G, groups is not None, None, dpred,
                 B, Cc, H * W, p)
    torch.cuda.synchronize()
    p64 = pred0.double().requires_grad_(True)
    q = p64 + (pv[:, :Cc].double() if resid else 0)
    if mask:
        q = torch.where(pm.view(B, Cc, 1, 1).expand_as(q), lab.double(), q)
    fn = (lambda a, b: (a - b).abs().mean()) if p == 1 else (lambda a, b: ((a - b) ** 2).mean())
    if groups:
        ref = torch.stack([fn(q[:, groups[i]:groups[i + 1]], lab[:, groups[i]:groups[i + 1]].double()) /
                           (fn(lab[:, groups[i]:groups[i + 1]].double(), 0 * lab[:, groups[i]:groups[i + 1]].double()) + 1e-10)
                           for i in range(G)]).mean()
    else:
        ref = fn(q, lab.double())
    ref.backward()
    assert rel(pred, q.detach()) < 1e-6
    assert abs(float(loss) - float(ref.detach())) < 1e-5 * abs(float(ref.detach()))
    assert rel(dpred, p64.grad) < 1e-5


# ----------------------------------------------------------------------------------------------- CPB MLP
@pytest.mark.parametrize("ws,heads", [(16, 3), (8, 12), (4, 24), (7, 2)])
def test_cpb(ws, heads):
    TS = (2 * ws - 1) ** 2
    r = torch.arange(-(ws - 1), ws, dtype=torch.float32)
    tab = torch.stack(torch.meshgrid(r, r, indexing="ij"), -1) / max(ws - 1, 1) * 8
    coords = (torch.sign(tab) * torch.log2(tab.abs() + 1) / 3).reshape(-1, 2).to(DEV)
    w0, b0, w2 = rnd(512, 2), rnd(512, seed=1, scale=0.5), rnd(heads, 512, seed=2, scale=0.05)
    table, z = torch.empty(heads, TS, device=DEV), torch.empty(TS, heads, device=DEV)
    ops.cpb_fwd(coords, w0, b0, w2, table, z, ws, heads)
    ps = [t.double().requires_grad_(True) for t in (w0, b0, w2)]
    ref = 16 * torch.sigmoid(torch.relu(coords.double() @ ps[0].t() + ps[1]) @ ps[2].t()).t()
    dt_ = rnd(heads, TS, seed=3)
    ref.backward(dt_.double())
    assert rel(table, ref.detach()) < 1e-5
    g = [torch.zeros_like(t) for t in (w0, b0, w2)]
    ops.cpb_bwd(coords, w0, b0, w2, z, dt_, g[0], g[1], g[2], ws, heads)
    torch.cuda.synchronize()
    for a, b in zip(g, ps):
        assert rel(a, b.grad) < 1e-4


def test_cpb_batched_layers():
    """scot_cpb_fwd_batched / scot_cpb_bwd_batched (all layers of a range in one launch; the backward stages a layer's table-gradient
    tile once per workgroup and owns its hidden units' gradients) against fp64 autograd of HF:376-378, 418-428 per layer, mixed window
    sizes and head counts, `+=` into gradients that already hold values."""
    layers = [(16, 3), (16, 6), (8, 12), (4, 24), (7, 2)]
    coords, coff, cur = [], {}, 0
    for ws in sorted({w for w, _ in layers}):
        r = torch.arange(-(ws - 1), ws, dtype=torch.float32)
        tab = torch.stack(torch.meshgrid(r, r, indexing="ij"), -1) / max(ws - 1, 1) * 8
        c = (torch.sign(tab) * torch.log2(tab.abs() + 1) / 3).reshape(-1)
        coff[ws] = cur
        cur += c.numel()
        coords.append(c)
    coords = torch.cat(coords).to(DEV)
    desc, off, toff = [], 0, 0
    for ws, heads in layers:
        ts = (2 * ws - 1) ** 2
        desc += [off, off + 1024, off + 1536, coff[ws], ws, heads, toff, toff]
        off += 1536 + heads * 512
        toff += heads * ts
    params = rnd(off, scale=0.3)
    dtab = rnd(toff, seed=5)
    tables, z = torch.empty(toff, device=DEV), torch.empty(toff, device=DEV)
    grads = rnd(off, seed=9, scale=0.1)
    g0 = grads.clone()
    d = torch.tensor(desc, dtype=torch.int32).to(DEV)
    ops.cpb_fwd_batched(params, d, len(layers), 16, coords, tables, z)
    ops.cpb_bwd_batched(params, d, 1, len(layers) - 1, 16, 24, coords, z, dtab, grads)       # layers 1.. of the list
    torch.cuda.synchronize()
    assert torch.equal(grads[:desc[8]], g0[:desc[8]])                                          # layer 0 is outside the range
    for li, (ws, heads) in enumerate(layers):
        o, ts = desc[8 * li], (2 * ws - 1) ** 2
        w0 = params[o:o + 1024].view(512, 2).double().requires_grad_(True)
        b0 = params[o + 1024:o + 1536].double().requires_grad_(True)
        w2 = params[o + 1536:o + 1536 + heads * 512].view(heads, 512).double().requires_grad_(True)
        cs = coords[coff[ws]:coff[ws] + 2 * ts].view(ts, 2).double()
        ref = 16 * torch.sigmoid(torch.relu(cs @ w0.t() + b0) @ w2.t()).t()
        t0 = desc[8 * li + 6]
        assert rel(tables[t0:t0 + heads * ts].view(heads, ts), ref.detach()) < 1e-5
        if li == 0:
            continue
        ref.backward(dtab[t0:t0 + heads * ts].view(heads, ts).double())
        got = (grads - g0)[o:o + 1536 + heads * 512]
        want = torch.cat([w0.grad.reshape(-1), b0.grad, w2.grad.reshape(-1)])
        assert rel(got, want) < 1e-4, (ws, heads)


# ----------------------------------------------------------------------------------------------- bf16x3 GEMM
@pytest.mark.parametrize("layout,M,N,K", [(ops.NT, 4096, 288, 96), (ops.NT, 1024, 96, 384), (ops.NN, 2048, 96, 384), (ops.NN, 1000, 384, 96),
                                          (ops.TN, 384, 96, 8192), (ops.TN, 96, 288, 4100 // 4 * 4), (ops.NT, 300, 72, 40),
                                          (ops.TN, 64, 96, 136)])      # (the 64 x 96 tile in TN)
def test_gemm_bf16x3_is_fp32_class(layout, M, N, K):
    """compute = bf16x3: fp32 operands split into hi + lo bf16, three bf16 MFMAs per K-step.  Against an fp64 product the error
    must be in the fp32 class (operand error ~2^-17), two orders of magnitude below plain bf16 operands (2^-9)."""
    if layout == ops.NT:
        A, B = rnd(M, K), rnd(N, K, seed=1)
        ref = A.double() @ B.double().t()
    elif layout == ops.NN:
        A, B = rnd(M, K), rnd(K, N, seed=1)
        ref = A.double() @ B.double()
    else:
        A, B = rnd(K, M), rnd(K, N, seed=1)
        ref = A.double().t() @ B.double()
    C = torch.zeros(M, N, device=DEV)
    bias = rnd(N, seed=2) if layout != ops.TN else None
    ops.gemm(layout, ops.X3, M, N, K, A, A.shape[1], B, B.shape[1], C, N, bias=bias, accumulate=layout == ops.TN)
    torch.cuda.synchronize()
    if bias is not None:
        ref = ref + bias.double()
    e = rel(C, ref)
    assert e < 2e-5, e
    Cb = torch.zeros(M, N, device=DEV)
    ops.gemm(layout, ops.BF16, M, N, K, A.bfloat16(), A.shape[1], B.bfloat16(), B.shape[1], Cb, N, bias=bias, accumulate=layout == ops.TN)
    torch.cuda.synchronize()
    assert rel(Cb, ref) > 20 * e      # what the split buys


# ----------------------------------------------------------------------------------------------- block tail (two halves, one launch)
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("cond", [True, False])
@pytest.mark.parametrize("B,L,C", [(2, 1024, 96), (3, 192, 96), (64, 1024, 96), (2, 256, 192), (5, 64, 192)])
@pytest.mark.parametrize("next_qkv", [False, True])
def test_block_tail_fwd_fused(train, cond, B, L, C, next_qkv):
    """scot_block_tail_fwd == scot_proj_cln_fwd followed by scot_mlp_block_fwd (the two validated launches it replaces): same
    arithmetic in the same order, the MLP half's operand rows only travel through LDS instead of HBM — equal up to nothing.
    next_qkv: the epilogue that produces the following layer's q/k/v projection == the stand-alone GEMM on out16 (fp32 sums to
    accumulation order, then one 16-bit rounding)."""
    M, hid = B * L, 4 * C
    bf = torch.bfloat16
    a = rnd(M, C, seed=11).to(bf)
    x = rnd(M, C, seed=12)
    wo, bo = rnd(C, C, scale=C ** -0.5, seed=13).to(bf), rnd(C, seed=14, scale=0.2)
    w1, b1 = rnd(hid, C, scale=C ** -0.5, seed=2).to(bf), rnd(hid, seed=3, scale=0.2)
    w2, b2 = rnd(C, hid, scale=hid ** -0.5, seed=4).to(bf), rnd(C, seed=5, scale=0.2)
    t = torch.rand(B, device=DEV) if cond else None
    s1 = (torch.rand(B, device=DEV) > 0.3).float() / 0.7
    s2 = (torch.rand(B, device=DEV) > 0.3).float() / 0.7
    n1 = [rnd(C, seed=20, scale=0.3) if cond else None, 1 + rnd(C, seed=21, scale=0.1), rnd(C, seed=22, scale=0.1) if cond else None, rnd(C, seed=23, scale=0.1)]
    n2 = [rnd(C, seed=6, scale=0.3) if cond else None, 1 + rnd(C, seed=7, scale=0.1), rnd(C, seed=8, scale=0.1) if cond else None, rnd(C, seed=9, scale=0.1)]

    def bufs():
        f = lambda *s, dtype=torch.float32: torch.full(s, float("nan"), device=DEV, dtype=dtype)
        d = dict(h=f(M, C), h16=f(M, C, dtype=bf), out=f(M, C), out16=f(M, C, dtype=bf))
        d.update(dict(z1=f(M, C), m1=f(M), r1=f(M), u=f(M, hid, dtype=bf), gp=f(M, hid, dtype=bf), z2=f(M, C), m2=f(M), r2=f(M)) if train else
                 dict(z1=None, m1=None, r1=None, u=None, gp=None, z2=None, m2=None, r2=None))
        return d
    r = bufs()
    assert ops.proj_cln_fwd(a, wo, bo, x, r["h"], r["h16"], r["z1"], r["m1"], r["r1"], t, n1[0], n1[1], n1[2], n1[3], s1, M, L, C, 1e-5)
    assert ops.mlp_block_fwd(r["h16"], r["h"], w1, b1, w2, b2, r["out"], r["out16"], r["u"], r["gp"], r["z2"], r["m2"], r["r2"], t, n2[0], n2[1],
                             n2[2], n2[3], s2, M, L, C, hid, 1e-5)
    f = bufs()
    wq, bq = rnd(3 * C, C, scale=C ** -0.5, seed=41).to(bf), rnd(3 * C, seed=42, scale=0.2)
    q = torch.full((M, 3 * C), float("nan"), device=DEV, dtype=bf) if next_qkv else None
    assert ops.block_tail_fwd((a, wo, bo, x, f["h"], f["h16"], f["z1"], f["m1"], f["r1"], n1[0], n1[1], n1[2], n1[3], s1),
                              (w1, b1, w2, b2, f["out"], f["out16"], f["u"], f["gp"], f["z2"], f["m2"], f["r2"], n2[0], n2[1], n2[2], n2[3], s2),
                              t, M, L, C, hid, 1e-5, *((wq, bq, q) if next_qkv else ()))
    torch.cuda.synchronize()
    for k in r:
        if r[k] is not None:
            assert torch.isfinite(f[k].float()).all(), k
            assert torch.equal(f[k], r[k]), (k, rel(f[k].float(), r[k].float()))
    if next_qkv:
        qr = torch.empty_like(q)
        ops.linear_fwd(ops.BF16, r["out16"], wq, qr, bias=bq)
        torch.cuda.synchronize()
        assert torch.isfinite(q.float()).all()
        ref = r["out16"].float() @ wq.float().t() + bq
        assert rel(q.float(), ref) < 4e-3 and rel(q.float(), qr.float()) < 2e-3, (rel(q.float(), ref), rel(q.float(), qr.float()))
        assert (q != qr).float().mean() < 0.02      # same products, fp32 sums in a different order: rare last-place flips only


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("cond", [True, False])
@pytest.mark.parametrize("B,L", [(2, 1024), (3, 200), (32, 1024)])
@pytest.mark.parametrize("next_qkv", [False, True])
def test_block_tail_fwd_fused_c48(train, cond, B, L, next_qkv):
    """scot_block_tail_fwd at C = 48 (Poseidon-T / -S stage 0, reference train.py:35-47; forward only): the contraction over the 48 channels
    runs as two 32-wide MFMA K-steps whose last 16 columns are zero on both sides, the row layout skips the pieces that do not exist, the
    statistics divide by 48.  There are no stand-alone C = 48 fused halves to compare with, so the reference is the chain restated in torch
    with the kernel's rounding points (16-bit h16 / gelu(u) / out16, fp32 everything else): fp32 tensors to accumulation order, 16-bit
    tensors to rare last-place flips."""
    C, hid = 48, 192
    M = B * L
    hd = ops.half_dtype() if hasattr(ops, "half_dtype") else torch.bfloat16
    a = rnd(M, C, seed=11).to(hd)
    x = rnd(M, C, seed=12)
    wo, bo = rnd(C, C, scale=C ** -0.5, seed=13).to(hd), rnd(C, seed=14, scale=0.2)
    w1, b1 = rnd(hid, C, scale=C ** -0.5, seed=2).to(hd), rnd(hid, seed=3, scale=0.2)
    w2, b2 = rnd(C, hid, scale=hid ** -0.5, seed=4).to(hd), rnd(C, seed=5, scale=0.2)
    t = torch.rand(B, device=DEV) if cond else None
    s1 = (torch.rand(B, device=DEV) > 0.3).float() / 0.7
    s2 = (torch.rand(B, device=DEV) > 0.3).float() / 0.7
    n1 = [rnd(C, seed=20, scale=0.3) if cond else None, 1 + rnd(C, seed=21, scale=0.1), rnd(C, seed=22, scale=0.1) if cond else None, rnd(C, seed=23, scale=0.1)]
    n2 = [rnd(C, seed=6, scale=0.3) if cond else None, 1 + rnd(C, seed=7, scale=0.1), rnd(C, seed=8, scale=0.1) if cond else None, rnd(C, seed=9, scale=0.1)]
    f = lambda *s, dtype=torch.float32: torch.full(s, float("nan"), device=DEV, dtype=dtype)
    o = dict(h=f(M, C), h16=f(M, C, dtype=hd), out=f(M, C), out16=f(M, C, dtype=hd))
    o.update(dict(z1=f(M, C), m1=f(M), r1=f(M), u=f(M, hid, dtype=hd), gp=f(M, hid, dtype=hd), z2=f(M, C), m2=f(M), r2=f(M)) if train else
             dict(z1=None, m1=None, r1=None, u=None, gp=None, z2=None, m2=None, r2=None))
    wq, bq = rnd(3 * C, C, scale=C ** -0.5, seed=41).to(hd), rnd(3 * C, seed=42, scale=0.2)
    q = torch.full((M, 3 * C), float("nan"), device=DEV, dtype=hd) if next_qkv else None
    assert ops.block_tail_fwd((a, wo, bo, x, o["h"], o["h16"], o["z1"], o["m1"], o["r1"], n1[0], n1[1], n1[2], n1[3], s1),
                              (w1, b1, w2, b2, o["out"], o["out16"], o["u"], o["gp"], o["z2"], o["m2"], o["r2"], n2[0], n2[1], n2[2], n2[3], s2),
                              t, M, L, C, hid, 1e-5, *((wq, bq, q) if next_qkv else ()))
    torch.cuda.synchronize()
    D = torch.float64
    per_row = lambda v: v.repeat_interleave(L).unsqueeze(1).to(D)

    def cln(z, n, s, resid):
        mu = z.mean(-1, keepdim=True)
        var = (z * z).mean(-1, keepdim=True) - mu * mu
        rs = 1.0 / torch.sqrt(var + 1e-5)
        ga = n[1].to(D) + (n[0].to(D) * per_row(t) if cond else 0.0)
        be = n[3].to(D) + (n[2].to(D) * per_row(t) if cond else 0.0)
        return resid.to(D) + per_row(s) * (ga * ((z - mu) * rs) + be), mu.squeeze(1), rs.squeeze(1)
    z1 = a.to(D) @ wo.to(D).t() + bo.to(D)
    h, m1, r1 = cln(z1, n1, s1, x)
    h16 = o["h16"]                                     # the kernel's own rounding of h feeds its second half
    assert rel(o["h"], h) < 2e-6 and rel(h16.float(), h) < 3e-3 and (h16 != h.to(torch.float32).to(hd)).float().mean() < 0.02
    u = h16.to(D) @ w1.to(D).t() + b1.to(D)
    act = torch.nn.functional.gelu(u)
    gp = 0.5 * (1 + torch.erf(u / math.sqrt(2))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)
    act16 = o["u"] if train else act.to(torch.float32).to(hd)
    z2 = act16.to(D) @ w2.to(D).t() + b2.to(D)
    out, m2, r2 = cln(z2, n2, s2, o["h"])
    tol16 = 6e-3 if hd == torch.bfloat16 else 1e-3
    assert torch.isfinite(o["out"]).all() and rel(o["out"], out) < (2e-6 if train else tol16), rel(o["out"], out)
    assert rel(o["out16"].float(), o["out"]) < tol16
    if train:
        assert rel(o["z1"], z1) < 2e-6 and rel(o["m1"], m1) < 2e-6 and rel(o["r1"], r1) < 2e-6
        assert rel(o["u"].float(), act) < tol16 and rel(o["gp"].float(), gp) < tol16
        assert rel(o["z2"], z2) < 2e-6 and rel(o["m2"], m2) < 1e-5 and rel(o["r2"], r2) < 2e-6
    if next_qkv:
        ref = o["out16"].to(D) @ wq.to(D).t() + bq.to(D)
        assert torch.isfinite(q.float()).all() and rel(q.float(), ref) < tol16


@pytest.mark.parametrize("cond", [True, False])
@pytest.mark.parametrize("B,L", [(2, 1024), (3, 192), (32, 1024)])
def test_block_tail_bwd_fused_c48(cond, B, L):
    """scot_block_tail_bwd at C = 48 (the stored-gelu' form: Poseidon-T / -S stage 0) against the chain restated in fp64, stage by stage
    from the kernel's own 16-bit intermediates: dz2 = CLN_bwd(s2·g) -> du = (dz2·W2) ⊙ gelu'(u) -> g' = g + du·W1 -> dz1 = CLN_bwd(s1·g')
    -> da = dz1·Wo, and the eight norm-parameter gradients (atomics)."""
    C, hid = 48, 192
    M = B * L
    hd = ops.half_dtype()
    D = torch.float64
    g0 = rnd(M, C, seed=31)
    z2, z1 = rnd(M, C, seed=32), rnd(M, C, seed=33)
    st = lambda z: (z.mean(-1).contiguous(), (1.0 / torch.sqrt(z.var(-1, unbiased=False) + 1e-5)).contiguous())
    (m2, r2), (m1, r1) = st(z2), st(z1)
    gp = rnd(M, hid, seed=34).to(hd)
    w1, w2 = rnd(hid, C, scale=C ** -0.5, seed=2).to(hd), rnd(C, hid, scale=hid ** -0.5, seed=4).to(hd)
    wo = rnd(C, C, scale=C ** -0.5, seed=13).to(hd)
    t = torch.rand(B, device=DEV) if cond else None
    s1 = (torch.rand(B, device=DEV) > 0.3).float() / 0.7
    s2 = (torch.rand(B, device=DEV) > 0.3).float() / 0.7
    gw2 = (rnd(C, seed=6, scale=0.3) if cond else None, 1 + rnd(C, seed=7, scale=0.1))
    gw1 = (rnd(C, seed=20, scale=0.3) if cond else None, 1 + rnd(C, seed=21, scale=0.1))
    f = lambda *s_, dtype=torch.float32: torch.full(s_, float("nan"), device=DEV, dtype=dtype)
    zc = lambda: torch.zeros(C, device=DEV)
    o = dict(g=f(M, C), dz2=f(M, C, dtype=hd), du=f(M, hid, dtype=hd), dz1=f(M, C, dtype=hd), da=f(M, C, dtype=hd))
    p2, p1 = [zc() if cond else None, zc(), zc() if cond else None, zc()], [zc() if cond else None, zc(), zc() if cond else None, zc()]
    assert ops.block_tail_bwd(g0, o["g"], (z2, m2, r2, gw2[0], gw2[1], s2, gp, w1, w2, o["dz2"], o["du"], p2[0], p2[1], p2[2], p2[3]),
                              (z1, m1, r1, gw1[0], gw1[1], s1, wo, o["dz1"], o["da"], p1[0], p1[1], p1[2], p1[3]), t, M, L, C, hid)
    torch.cuda.synchronize()
    per_row = lambda v: v.repeat_interleave(L).unsqueeze(1).to(D)

    def cln_bwd(gin, z, mean, rstd, gw, s):
        dd = gin.to(D) * per_row(s)
        xh = (z.to(D) - mean.to(D).unsqueeze(1)) * rstd.to(D).unsqueeze(1)
        ga = gw[1].to(D) + (gw[0].to(D) * per_row(t) if cond else 0.0)
        d = dd * ga
        m_1, m_2 = d.mean(-1, keepdim=True), (d * xh).mean(-1, keepdim=True)
        dz = rstd.to(D).unsqueeze(1) * (d - m_1 - xh * m_2)
        tt_ = per_row(t) if cond else None
        pg = [(tt_ * dd * xh).sum(0) if cond else None, (dd * xh).sum(0), (tt_ * dd).sum(0) if cond else None, dd.sum(0)]
        return dz, pg
    tol16 = 6e-3 if hd == torch.bfloat16 else 1e-3
    for k in o:
        assert torch.isfinite(o[k].float()).all(), k
    dz2, pg2 = cln_bwd(g0, z2, m2, r2, gw2, s2)
    assert rel(o["dz2"].float(), dz2) < tol16
    du = (o["dz2"].to(D) @ w2.to(D)) * gp.to(D)
    assert rel(o["du"].float(), du) < tol16
    g1 = g0.to(D) + o["du"].to(D) @ w1.to(D)
    assert rel(o["g"], g1) < 2e-6
    dz1, pg1 = cln_bwd(o["g"], z1, m1, r1, gw1, s1)
    assert rel(o["dz1"].float(), dz1) < tol16
    assert rel(o["da"].float(), o["dz1"].to(D) @ wo.to(D)) < tol16
    for got, ref in zip(p2 + p1, pg2 + pg1):
        if got is not None:
            assert rel(got, ref) < 1e-4


@pytest.mark.parametrize("prologue", [False, True])
@pytest.mark.parametrize("cond", [True, False])
@pytest.mark.parametrize("B,L,C", [(2, 1024, 96), (3, 192, 96), (64, 1024, 96), (2, 256, 192), (5, 64, 192)])
def test_block_tail_bwd_fused(cond, B, L, C, prologue):
    """scot_block_tail_bwd == [qkv dgrad into g (prologue)] + scot_mlp_block_bwd + scot_proj_cln_bwd on its g_out: the data tensors
    are equal (the prologue's fp32 sums to accumulation order), the parameter-gradient sums (atomics) equal to accumulation order."""
    M, hid = B * L, 4 * C
    bf = torch.bfloat16
    g0 = rnd(M, C, seed=31)
    z2, z1 = rnd(M, C, seed=32), rnd(M, C, seed=33)
    st = lambda z: (z.mean(-1).contiguous(), (1.0 / torch.sqrt(z.var(-1, unbiased=False) + 1e-5)).contiguous())
    (m2, r2), (m1, r1) = st(z2), st(z1)
    gp = rnd(M, hid, seed=34).to(bf)
    w1, w2 = rnd(hid, C, scale=C ** -0.5, seed=2).to(bf), rnd(C, hid, scale=hid ** -0.5, seed=4).to(bf)
    wo = rnd(C, C, scale=C ** -0.5, seed=13).to(bf)
    t = torch.rand(B, device=DEV) if cond else None
    s1 = (torch.rand(B, device=DEV) > 0.3).float() / 0.7
    s2 = (torch.rand(B, device=DEV) > 0.3).float() / 0.7
    gw2 = (rnd(C, seed=6, scale=0.3) if cond else None, 1 + rnd(C, seed=7, scale=0.1))
    gw1 = (rnd(C, seed=20, scale=0.3) if cond else None, 1 + rnd(C, seed=21, scale=0.1))

    def outs():
        f = lambda *s, dtype=torch.float32: torch.full(s, float("nan"), device=DEV, dtype=dtype)
        z = lambda: torch.zeros(C, device=DEV)
        return dict(g=f(M, C), dz2=f(M, C, dtype=bf), du=f(M, hid, dtype=bf), dz1=f(M, C, dtype=bf), da=f(M, C, dtype=bf)), \
            [z() if cond else None, z(), z() if cond else None, z()], [z() if cond else None, z(), z() if cond else None, z()]
    r, rp2, rp1 = outs()
    dqkv = wqkv = None
    gin_r = gin_f = g0
    if prologue:
        dqkv, wqkv = rnd(M, 3 * C, seed=41).to(bf), rnd(3 * C, C, scale=(3 * C) ** -0.5, seed=42).to(bf)
        gin_r, gin_f = g0.clone(), g0.clone()
        ops.linear_dgrad(ops.BF16, dqkv, wqkv, gin_r, accumulate=True)
        r["g"] = gin_r
    assert ops.mlp_block_bwd(gin_r, r["g"], z2, m2, r2, t, gw2[0], gw2[1], s2, gp, w1, w2, r["dz2"], r["du"], rp2[0], rp2[1], rp2[2], rp2[3], M, L, C,
                             hid)
    assert ops.proj_cln_bwd(r["g"], z1, m1, r1, t, gw1[0], gw1[1], s1, wo, r["dz1"], r["da"], rp1[0], rp1[1], rp1[2], rp1[3], M, L, C)
    f, fp2, fp1 = outs()
    if prologue:
        f["g"] = gin_f                    # in place
    assert ops.block_tail_bwd(gin_f, f["g"], (z2, m2, r2, gw2[0], gw2[1], s2, gp, w1, w2, f["dz2"], f["du"], fp2[0], fp2[1], fp2[2], fp2[3]),
                              (z1, m1, r1, gw1[0], gw1[1], s1, wo, f["dz1"], f["da"], fp1[0], fp1[1], fp1[2], fp1[3]), t, M, L, C, hid,
                              dqkv=dqkv, wqkv=wqkv)
    torch.cuda.synchronize()
    for k in r:
        assert torch.isfinite(f[k].float()).all(), k
        if prologue:      # the stand-alone dgrad GEMM and the prologue sum the same products in a different order
            assert rel(f[k].float(), r[k].float()) < (2e-3 if f[k].dtype == bf else 1e-5), (k, rel(f[k].float(), r[k].float()))
        else:
            assert torch.equal(f[k], r[k]), (k, rel(f[k].float(), r[k].float()))
    for a_, b_ in zip(fp2 + fp1, rp2 + rp1):
        if a_ is not None:
            assert rel(a_, b_) < 1e-4


# ----------------------------------------------------------------------------------------------- transposed weight copies
def test_transpose_cast_and_dgrad_nt():
    """scot_transpose_cast: per-matrix transposes of an fp32 arena in the operand format (ragged 64x64 tiles included); a data
    gradient through the transposed copy (NT product) equals the NN product on the plain copy to fp32 accumulation order."""
    mats = [(96, 288), (288, 96), (384, 1536), (40, 72), (768, 192)]
    offs, cur = [], 0
    for r, c in mats:
        offs.append(cur)
        cur += (r * c + 63) // 64 * 64 + 64
    arena = rnd(cur, seed=3)
    desc, tile = [], 0
    for (r, c), o in zip(mats, offs):
        desc.append((o, r, c, tile))
        tile += ((r + 63) // 64) * ((c + 63) // 64)
    wt = torch.full((cur,), float("nan"), device=DEV, dtype=torch.bfloat16)
    ops.transpose_cast(arena, wt, torch.tensor(desc, dtype=torch.int32, device=DEV), len(mats), tile)
    torch.cuda.synchronize()
    for (r, c), o in zip(mats, offs):
        ref = arena[o:o + r * c].view(r, c).to(torch.bfloat16).t().contiguous()
        assert torch.equal(wt[o:o + r * c].view(c, r), ref), (r, c)
    r, c = mats[2]
    w16 = arena[offs[2]:offs[2] + r * c].view(r, c).to(torch.bfloat16)
    dy = rnd(512, r, seed=5).to(torch.bfloat16)
    a, b = torch.empty(512, c, device=DEV), torch.empty(512, c, device=DEV)
    ops.linear_dgrad(ops.BF16, dy, w16, a)
    ops.linear_dgrad(ops.BF16, dy, w16, b, wt=wt[offs[2]:offs[2] + r * c].view(c, r))
    torch.cuda.synchronize()
    assert rel(b, a) < 1e-6 and rel(b, dy.float() @ w16.float()) < 1e-5


# ----------------------------------------------------------------------------------------------- grouped weight gradients
# scot_wgrad_group is the kernel bench.py's `roofline` is quoted on: pinned here DIRECTLY on the MI355X (round 2 only covered it on the
# CPU emulation and through whole-model gradients): the four weight gradients of a ScOTLayer (fc2, fc1, out-projection, qkv) at every
# Poseidon-B stage shape, a ragged token count, shapes off the 96-tile path, both operand formats; reference = fp64 dY^T X on the
# operands as stored (16-bit), i.e. what is bounded is the kernel's own error (fp32 MFMA accumulation + split-K partial sums).
WGROUP_CASES = [(65536, 96), (16384, 192), (4096, 384), (1024, 768), (2008, 96), (4104, 64), (1000, 40), (1004, 32)]


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("K,C", WGROUP_CASES)
def test_wgrad_group_direct(kind, K, C):
    prev = ops.use(kind)
    try:
        hd = ops.half_dtype()
        dims = [(C, 4 * C), (4 * C, C), (C, C), (3 * C, C)]            # (M_i, N_i) of fc2, fc1, proj, qkv: dW_i [M_i, N_i]
        dys = [rnd(K, m, dtype=hd, scale=0.5, seed=10 + i) for i, (m, _) in enumerate(dims)]
        xs = [rnd(K, n, dtype=hd, seed=20 + i) for i, (_, n) in enumerate(dims)]
        dws0 = [rnd(m, n, seed=30 + i) for i, (m, n) in enumerate(dims)]                       # += semantics: start from non-zero
        dbs0 = [rnd(m, seed=40 + i) for i, (m, _) in enumerate(dims)]
        dws, dbs = [t.clone() for t in dws0], [t.clone() for t in dbs0]
        ok = ops.wgrad_group(ops.BF16, [(dy, x, dw, db) for dy, x, dw, db in zip(dys, xs, dws, dbs)])
        if not ok:     # shapes the grouped kernel declines go through the per-problem path (same contract)
            for dy, x, dw, db in zip(dys, xs, dws, dbs):
                ops.linear_wgrad(ops.BF16, dy, x, dw, dbias=db)
        torch.cuda.synchronize()
        assert ok == (C % 8 == 0 and K % 8 == 0)
        worst = 0.0
        for dy, x, dw0, dw, db0, db in zip(dys, xs, dws0, dws, dbs0, dbs):
            ref = dy.double().t() @ x.double()
            e = rel(dw.double() - dw0.double(), ref)
            worst = max(worst, e)
            assert e < 1e-6, (K, C, tuple(dw.shape), e)               # measured on MI355X (round 3): 9.5e-8 .. 4.1e-7 over all cases
            assert rel(db.double() - db0.double(), dy.double().sum(0)) < 2e-6
        print(f"wgrad_group {kind} K={K} C={C}: worst rel-L2 {worst:.2e}")
    finally:
        ops.use(prev)


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("K,C,forced", [(1024, 768, 0), (1024, 768, 2), (4096, 384, 1 | (4 << 4)), (4096, 384, 2 | (2 << 4)), (2048, 1536, -1), (8192, 768, -1),
                                        (512, 128, 1), (192, 256, 0 | (3 << 4))])
def test_wgrad_group_wide_tiles(kind, K, C, forced):
    """csrc/wgrad_wide.hip (128 x 128 tiles; forced = kernel instantiation | K slices << 4, -1 = the library's policy) against fp64 and against the
    64 x 64-tile grouped kernel, += semantics, bias gradients; repeated launches of the unsplit form are bit-identical."""
    prev = ops.use(kind)
    lib = ops.L()
    try:
        hd = ops.half_dtype()
        dims = [(C, 4 * C), (4 * C, C), (C, C), (3 * C, C)]
        dys = [rnd(K, m, dtype=hd, scale=0.5, seed=10 + i) for i, (m, _) in enumerate(dims)]
        xs = [rnd(K, n, dtype=hd, seed=20 + i) for i, (_, n) in enumerate(dims)]
        dws0 = [rnd(m, n, seed=30 + i) for i, (m, n) in enumerate(dims)]
        dbs0 = [rnd(m, seed=40 + i) for i, (m, _) in enumerate(dims)]
        out = {}
        for mode in ("narrow", "wide", "wide2"):
            lib.scot_gemm_wide_config(0 if mode == "narrow" else (1 if forced < 0 else 2), max(forced, 0))
            dws, dbs = [t.clone() for t in dws0], [t.clone() for t in dbs0]
            assert ops.wgrad_group(ops.BF16, [(dy, x, dw, db) for dy, x, dw, db in zip(dys, xs, dws, dbs)])
            torch.cuda.synchronize()
            out[mode] = (dws, dbs)
        for i, (dy, x) in enumerate(zip(dys, xs)):
            ref = dy.double().t() @ x.double()
            assert rel(out["wide"][0][i].double() - dws0[i].double(), ref) < 1e-6
            assert rel(out["wide"][1][i].double() - dbs0[i].double(), dy.double().sum(0)) < 2e-6
            assert rel(out["wide"][0][i], out["narrow"][0][i]) < 1e-6
            if forced >= 0 and (forced >> 4) == 0:
                assert torch.equal(out["wide"][0][i], out["wide2"][0][i])
    finally:
        lib.scot_gemm_wide_config(1, 0)
        ops.use(prev)


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("K,C,forced", [(65536, 96, -1), (16384, 192, -1), (4096, 384, -1), (1024, 768, -1), (4096, 384, 1 | (4 << 4)), (2008, 96, -1)])
def test_wgrad_group_store_and_scaled_modes(kind, K, C, forced):
    """Round 6 (lazy zero-grad): scot_wgrad_group's `modes` at every Poseidon-B stage shape — 1 = the first writer stores s·acc over a tensor
    full of NaN, 2 = adds s·acc to unscaled contents, 0 = plain accumulation — through every kernel that finishes a grouped weight gradient
    (64 x 64 / 96 x 96 tiles with the grouped split-K reduce, the unsplit single-owner epilogues of the 64 x 64 and 128 x 128 tiles, the
    K-sliced 128 x 128 form); bias gradients always accumulate unscaled.  Reference: fp64 on the operands as stored."""
    prev = ops.use(kind)
    lib = ops.L()
    try:
        hd = ops.half_dtype()
        dims = [(C, 4 * C), (4 * C, C), (C, C), (3 * C, C)]
        modes = [ops.GRAD_STORE_SCALED, ops.GRAD_ADD_SCALED, ops.GRAD_ADD, ops.GRAD_STORE_SCALED]
        s = torch.tensor([2.0 ** -7], device=DEV)
        dys = [rnd(K, m, dtype=hd, scale=0.5, seed=10 + i) for i, (m, _) in enumerate(dims)]
        xs = [rnd(K, n, dtype=hd, seed=20 + i) for i, (_, n) in enumerate(dims)]
        dws0 = [rnd(m, n, seed=30 + i) for i, (m, n) in enumerate(dims)]
        dbs0 = [rnd(m, seed=40 + i) for i, (m, _) in enumerate(dims)]
        dws = [torch.full_like(t, float("nan")) if md == ops.GRAD_STORE_SCALED else t.clone() for t, md in zip(dws0, modes)]
        dbs = [t.clone() for t in dbs0]
        if forced >= 0:
            lib.scot_gemm_wide_config(2, forced)
        assert ops.wgrad_group(ops.BF16, [(dy, x, dw, db) for dy, x, dw, db in zip(dys, xs, dws, dbs)], modes, s)
        torch.cuda.synchronize()
        for dy, x, dw0, dw, db0, db, md in zip(dys, xs, dws0, dws, dbs0, dbs, modes):
            prod = dy.double().t() @ x.double()
            ref = {ops.GRAD_STORE_SCALED: prod * 2.0 ** -7, ops.GRAD_ADD_SCALED: dw0.double() + prod * 2.0 ** -7, ops.GRAD_ADD: dw0.double() + prod}[md]
            assert bool(torch.isfinite(dw).all()) and rel(dw, ref) < 1e-6, (K, C, md)
            assert rel(db.double() - db0.double(), dy.double().sum(0)) < 2e-6
    finally:
        lib.scot_gemm_wide_config(1, 0)
        ops.use(prev)


def test_segments_scale_and_fill():
    """scot_segments_scale: pieces (offset, count <= 4096) of one flat tensor scaled by a device factor — non-finite results counted — or zeroed
    (scale NULL); everything between the pieces untouched."""
    n = 5_000_000
    x0 = rnd(n)
    g = torch.Generator().manual_seed(5)
    segs, o = [], 0
    while o + 8192 < n:
        c = int(torch.randint(1, 1025, (1,), generator=g)) * 4 - int(torch.randint(0, 4, (1,), generator=g))      # (counts need not be multiples of 4)
        segs.append((o, c))
        o += (c + 3) // 4 * 4 + int(torch.randint(0, 4096, (1,), generator=g)) * 4
    chunks = torch.tensor([v for sg in segs for v in sg], dtype=torch.int64, device=DEV).reshape(-1, 2)
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    for o, c in segs:
        mask[o:o + c] = True
    x, cnt = x0.clone(), torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.segments_scale(x, chunks, len(segs), torch.tensor([0.5], device=DEV), cnt)
    assert torch.equal(x, torch.where(mask, x0 * 0.5, x0)) and int(cnt) == 0
    x[segs[3][0] + 1] = float("inf")
    ops.segments_scale(x, chunks, len(segs), torch.tensor([2.0], device=DEV), cnt)
    assert int(cnt) == 1
    ops.segments_scale(x, chunks, len(segs), None)
    assert torch.equal(x, torch.where(mask, torch.zeros_like(x0), x0))


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("M,N,K,S", [(1024, 768, 3072, 2), (1024, 768, 2304, 3), (4096, 384, 1536, 4), (1000, 200, 1088, 2)])
def test_gemm_nt_split_k_atomic(kind, M, N, K, S):
    """csrc/gemm_fast.hip, K slices of the fp32-result NT products adding into the result with fp32 atomics (scot_gemm_splitk_config; the
    library's policy never selects it — profiles/round6/splitk_*): the zeroed forward form and the accumulating data-gradient form against fp64
    and against the unsplit kernel."""
    prev = ops.use(kind)
    lib = ops.L()
    try:
        hd = ops.half_dtype()
        x, w, b = rnd(M, K, dtype=hd), rnd(N, K, dtype=hd, scale=K ** -0.5, seed=1), rnd(N, seed=2)
        u = x.double() @ w.double().t() + b.double()
        lib.scot_gemm_wide_config(0, 0)
        lib.scot_gemm_splitk_config(-1, 0)
        y0 = torch.empty(M, N, device=DEV)
        ops.linear_fwd(ops.BF16, x, w, y0, bias=b)
        lib.scot_gemm_splitk_config(S, 1)
        y = torch.full((M, N), float("nan"), device=DEV)
        ops.linear_fwd(ops.BF16, x, w, y, bias=b)
        g0 = rnd(M, N, seed=5)
        g = g0.clone()
        ops.linear_dgrad(ops.BF16, x, w.t().contiguous(), g, accumulate=True, wt=w)
        torch.cuda.synchronize()
        assert rel(y, u) < 2e-6 and rel(y, y0) < 1e-6
        assert rel(g, g0.double() + x.double() @ w.double().t()) < 1e-6
    finally:
        lib.scot_gemm_splitk_config(0, 1)
        lib.scot_gemm_wide_config(1, 0)
        ops.use(prev)


# ----------------------------------------------------------------------------------------------- the layer tail without 4C-wide tensors in HBM
@pytest.mark.parametrize("prologue", [False, True])
@pytest.mark.parametrize("cond", [True, False])
@pytest.mark.parametrize("B,L,C", [(2, 1024, 96), (3, 192, 96), (64, 1024, 96), (2, 256, 192), (5, 64, 192)])
def test_block_tail_lean_forms(cond, B, L, C, prologue):
    """Round 3: forward tail that stores neither gelu(u) nor gelu'(u) (z1 / z2 as 16-bit), backward tail that RECOMPUTES gelu'(u) from
    h16, does not store du and hands its norms' parameter-gradient column sums over as per-workgroup partial rows, and scot_wgrad_mlp,
    which recomputes gelu(u) / du for the fc1 / fc2 weight gradients — against the round-2 forms of the same entry points (which store
    and re-read those tensors) on the same inputs."""
    M, hid = B * L, 4 * C
    bf = torch.bfloat16
    a, x = rnd(M, C, seed=11).to(bf), rnd(M, C, seed=12)
    wo, bo = rnd(C, C, scale=C ** -0.5, seed=13).to(bf), rnd(C, seed=14, scale=0.2)
    w1, b1 = rnd(hid, C, scale=C ** -0.5, seed=2).to(bf), rnd(hid, seed=3, scale=0.2)
    w2, b2 = rnd(C, hid, scale=hid ** -0.5, seed=4).to(bf), rnd(C, seed=5, scale=0.2)
    t = torch.rand(B, device=DEV) if cond else None
    n1 = [rnd(C, seed=20, scale=0.3) if cond else None, 1 + rnd(C, seed=21, scale=0.1), rnd(C, seed=22, scale=0.1) if cond else None, rnd(C, seed=23, scale=0.1)]
    n2 = [rnd(C, seed=6, scale=0.3) if cond else None, 1 + rnd(C, seed=7, scale=0.1), rnd(C, seed=8, scale=0.1) if cond else None, rnd(C, seed=9, scale=0.1)]
    f = lambda *s, dtype=torch.float32: torch.full(s, float("nan"), device=DEV, dtype=dtype)

    # ---- forward: round-2 form (everything stored, fp32 z) vs lean form
    o = dict(h=f(M, C), h16=f(M, C, dtype=bf), z1=f(M, C), m1=f(M), r1=f(M), out=f(M, C), out16=f(M, C, dtype=bf), act=f(M, hid, dtype=bf),
             dact=f(M, hid, dtype=bf), z2=f(M, C), m2=f(M), r2=f(M))
    assert ops.block_tail_fwd((a, wo, bo, x, o["h"], o["h16"], o["z1"], o["m1"], o["r1"], n1[0], n1[1], n1[2], n1[3], None),
                              (w1, b1, w2, b2, o["out"], o["out16"], o["act"], o["dact"], o["z2"], o["m2"], o["r2"], n2[0], n2[1], n2[2], n2[3], None),
                              t, M, L, C, hid, 1e-5)
    n = dict(h=f(M, C), h16=f(M, C, dtype=bf), z1=f(M, C, dtype=bf), m1=f(M), r1=f(M), out=f(M, C), out16=f(M, C, dtype=bf), z2=f(M, C, dtype=bf),
             m2=f(M), r2=f(M))
    assert ops.block_tail_fwd((a, wo, bo, x, n["h"], n["h16"], n["z1"], n["m1"], n["r1"], n1[0], n1[1], n1[2], n1[3], None),
                              (w1, b1, w2, b2, n["out"], n["out16"], None, None, n["z2"], n["m2"], n["r2"], n2[0], n2[1], n2[2], n2[3], None),
                              t, M, L, C, hid, 1e-5, z16=True)
    torch.cuda.synchronize()
    for k in ("h", "h16", "m1", "r1", "out", "out16", "m2", "r2"):
        assert torch.equal(n[k], o[k]), k
    assert torch.equal(n["z1"], o["z1"].to(bf)) and torch.equal(n["z2"], o["z2"].to(bf))

    # ---- backward: round-2 form (gelu'(u) loaded, du stored, atomics) vs lean forms
    g0 = rnd(M, C, seed=31)
    dqkv = wqkv = None
    if prologue:
        dqkv, wqkv = rnd(M, 3 * C, seed=41).to(bf), rnd(3 * C, C, scale=(3 * C) ** -0.5, seed=42).to(bf)
    zc = lambda: torch.zeros(C, device=DEV)

    def run(lean_z, recomp, partials):
        g = g0.clone()
        outs = dict(dz2=f(M, C, dtype=bf), du=None if recomp else f(M, hid, dtype=bf), dz1=f(M, C, dtype=bf), da=f(M, C, dtype=bf))
        Cp = (C + 63) // 64 * 64      # [gw_w | gw_b | bw_w | bw_b] ([gw_b | bw_b] without conditioning) at the parameter arena's stride
        flat2, flat1 = torch.zeros(4 * Cp, device=DEV), torch.zeros(4 * Cp, device=DEV)
        if cond:
            p2, p1 = [flat2[i * Cp:i * Cp + C] for i in range(4)], [flat1[i * Cp:i * Cp + C] for i in range(4)]
        else:
            p2, p1 = [None, flat2[0:C], None, flat2[Cp:Cp + C]], [None, flat1[0:C], None, flat1[Cp:Cp + C]]
        nwg = ops.tail_workgroups(M, L, C)
        ncol = (4 if cond else 2) * Cp
        part2 = f(nwg, ncol) if partials else None
        part1 = f(nwg, ncol) if partials else None
        z2_, z1_ = (n["z2"], n["z1"]) if lean_z else (o["z2"], o["z1"])
        assert ops.block_tail_bwd(g, g, (z2_, o["m2"], o["r2"], n2[0], n2[1], None, None if recomp else o["dact"], w1, w2, outs["dz2"], outs["du"],
                                         p2[0], p2[1], p2[2], p2[3]),
                                  (z1_, o["m1"], o["r1"], n1[0], n1[1], None, wo, outs["dz1"], outs["da"], p1[0], p1[1], p1[2], p1[3]),
                                  t, M, L, C, hid, dqkv=dqkv, wqkv=wqkv, h16=o["h16"] if recomp else None, b1=b1 if recomp else None, z16=lean_z,
                                  partial2=part2, partial1=part1)
        if partials:
            ops.partial_colsum(part2, nwg, ncol, flat2)
            ops.partial_colsum(part1, nwg, ncol, flat1)
        torch.cuda.synchronize()
        outs["g"] = g
        return outs, flat2, flat1
    assert ops.tail_workgroups(M, L, C) == (M + (128 if (C == 96 and M >= 65536 and L % 128 == 0) else 64) - 1) // (128 if (C == 96 and M >= 65536 and L % 128 == 0) else 64)
    r, r2f, r1f = run(False, False, False)
    # (1) recomputation + partial sums, fp32 z: the same values (the recomputed u is the forward's u bit for bit, gelu' rounded alike)
    c, c2f, c1f = run(False, True, True)
    for k in ("g", "dz2", "dz1", "da"):
        assert torch.isfinite(c[k].float()).all(), k
        assert torch.equal(c[k], r[k]), (k, rel(c[k].float(), r[k].float()))
    assert rel(c2f, r2f) < 1e-4 and rel(c1f, r1f) < 1e-4
    # (2) + 16-bit z1 / z2: x-hat carries one 16-bit rounding (2^-9 bf16 / 2^-12 binary16)
    e, e2f, e1f = run(True, True, True)
    tol = 1.5e-2 if ops.half_dtype() == torch.bfloat16 else 2e-3
    for k in ("g", "dz2", "dz1", "da"):
        assert rel(e[k].float(), r[k].float()) < tol, (k, rel(e[k].float(), r[k].float()))
    assert rel(e2f, r2f) < tol and rel(e1f, r1f) < tol

    # ---- fc1 / fc2 weight gradients with everything recomputed vs the GEMMs on the stored tensors
    gW = torch.zeros(2 * hid * C + hid + C, device=DEV) + 0.125           # [W1 | b1 | W2 | b2] contiguous, += semantics
    dW1, db1, dW2, db2 = gW[:hid * C].view(hid, C), gW[hid * C:hid * C + hid], gW[hid * C + hid:2 * hid * C + hid].view(C, hid), gW[2 * hid * C + hid:]
    w2t = w2.t().contiguous()
    assert ops.wgrad_mlp(o["h16"], r["dz2"], w1, b1, w2t, dW1, db1, dW2, db2)
    torch.cuda.synchronize()
    du, act, dz2, h16 = r["du"].double(), o["act"].double(), r["dz2"].double(), o["h16"].double()
    assert rel(dW1 - 0.125, du.t() @ h16) < 2e-4 and rel(db1 - 0.125, du.sum(0)) < 2e-4
    assert rel(dW2 - 0.125, dz2.t() @ act) < 2e-4 and rel(db2 - 0.125, dz2.sum(0)) < 2e-4
