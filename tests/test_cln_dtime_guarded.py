"""scot_cln_dtime (csrc/cln_dtime.hip) inside NaN guard bands, against a per-sample bound in which no measured number enters.

  d_time[b] += s_b · Σ_{rows r of sample b} Σ_c dout[r,c] · (gw_w[c]·xhat[r,c] + bw_w[c]),   xhat = (x − mean_r)·rstd_r

Every operand, the result and the workspace are views inside poisoned allocations (tests/kernel_checks.py): the bands must be
intact bit for bit, the result finite, bit-identical to the launch on plain tensors and to a second launch (the kernel promises a
fixed summation order), and

  |d_time[b] − fp64| <= (n + 8)·2^-24 · s_b · Σ_{r,c} |dout|·(|gw_w|·|xhat| + |bw_w|),      n = rows_per_sample·C

— the bound of an n-term fp32 sum in ANY order (Higham §3.1/§4.2: (n − 1)u to first order) plus the roundings on the way to a
term: x − mean, ·rstd, the fused multiply-add, ·dout, the final ·s_b and the add into d_time (6 <= 8).  The 16-bit inputs are taken
as the kernel sees them (the reference is computed from the rounded values).

Small shapes run on the CPU emulation (`not gpu`), the full list on the MI355X (`-m gpu`)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
from kernel_checks import U32, check_all, guarded  # noqa: E402
from poseidon_amd import ops  # noqa: E402


def launch(dout, x, mean, rstd, gw, bw, scale, d_time, rows, rps, C, ws):
    """the C ABI call itself, with the caller's workspace (ops.cln_dtime takes the shared one)"""
    return ops.L().scot_cln_dtime(ops.ptr(dout), ops.dt(dout), ops.ptr(x), ops.dt(x), ops.ptr(mean), ops.ptr(rstd), ops.ptr(gw), ops.ptr(bw),
                                  ops.ptr(scale), ops.ptr(d_time), rows, rps, C, ops.ptr(ws), 0 if ws is None else ws.numel() * 4, ops.stream())


def ws_floats(rows, rps, C):
    need = int(ops._raw().scot_cln_dtime_workspace_bytes(rows, rps, C))
    assert need > 0 and need % 4 == 0
    return need // 4


def one_case(C, rps, B, dtype, with_scale, device, seed=0):
    gen = torch.Generator(device=device).manual_seed(1000 * C + 7 * rps + B + seed)
    rows = B * rps
    x32 = torch.randn(rows, C, generator=gen, device=device) * 1.5 + 0.3
    d32 = torch.randn(rows, C, generator=gen, device=device) * (1.0 + torch.arange(C, device=device) % 3)
    xs, ds = x32.to(dtype), d32.to(dtype)            # what the kernel sees
    xf = xs.float()
    mean = xf.mean(-1)
    var = (xf * xf).mean(-1) - mean * mean
    rstd = 1.0 / torch.sqrt(var.clamp_min(0) + 1e-5)
    gw = torch.randn(C, generator=gen, device=device) * 0.7
    bw = torch.randn(C, generator=gen, device=device) * 0.4
    sc = (torch.tensor([0.0, 2.0, 1.25, 4.0 / 3.0])[torch.arange(B) % 4] if B > 1 else torch.tensor([1.6])).to(device) if with_scale else None
    nws = ws_floats(rows, rps, C)

    gx, Gx = guarded((rows, C), dtype, device, src=xs, name="x")
    gd, Gd = guarded((rows, C), dtype, device, src=ds, name="dout")
    gm, Gm = guarded((rows,), torch.float32, device, src=mean, name="mean")
    gr, Gr = guarded((rows,), torch.float32, device, src=rstd, name="rstd")
    ggw, Ggw = guarded((C,), torch.float32, device, src=gw, name="gw_w")
    gbw, Gbw = guarded((C,), torch.float32, device, src=bw, name="bw_w")
    gt, Gt = guarded((B,), torch.float32, device, fill=0.0, name="d_time")
    gws, Gws = guarded((nws,), torch.float32, device, name="workspace")
    guards = [Gx, Gd, Gm, Gr, Ggw, Gbw, Gt, Gws]
    if with_scale:
        gs, Gs = guarded((B,), torch.float32, device, src=sc, name="sample_scale")
        guards.append(Gs)
    else:
        gs = None
    assert launch(gd, gx, gm, gr, ggw, gbw, gs, gt, rows, rps, C, gws) == 0
    got = gt.clone()
    check_all(guards)
    assert torch.isfinite(got).all(), (C, rps, B, dtype, got)

    # the same launch on plain tensors, and a second one: bit for bit
    for _ in range(2):
        pt, pws = torch.zeros(B, device=device), torch.empty(nws, device=device)
        assert launch(ds.clone(), xs.clone(), mean.clone(), rstd.clone(), gw.clone(), bw.clone(), None if sc is None else sc.clone(),
                      pt, rows, rps, C, pws) == 0
        assert torch.equal(pt.view(torch.int32), got.view(torch.int32)), (C, rps, B, dtype, pt, got)

    # fp64 on the operands as the kernel sees them
    xh = (xs.double() - mean.double()[:, None]) * rstd.double()[:, None]
    term = ds.double() * (gw.double() * xh + bw.double())
    absterm = ds.double().abs() * (gw.double().abs() * xh.abs() + bw.double().abs())
    s64 = sc.double() if sc is not None else torch.ones(B, dtype=torch.float64, device=device)
    ref = s64 * term.view(B, -1).sum(-1)
    bound = (rps * C + 8) * U32 * s64.abs() * absterm.view(B, -1).sum(-1)
    err = (got.double() - ref).abs()
    assert bool((err <= bound).all()), (C, rps, B, dtype, with_scale, err.tolist(), bound.tolist())

    # += : a second call onto the first result adds the same amount (one more rounding of the sum)
    assert launch(gd, gx, gm, gr, ggw, gbw, gs, gt, rows, rps, C, gws) == 0
    check_all(guards)
    assert bool(((gt.double() - 2 * got.double()).abs() <= 2 * U32 * got.double().abs()).all())


def declines(device):
    """unsupported arguments: -3, and nothing is written"""
    B, rps, C = 2, 1024, 48
    rows = B * rps
    x, d = torch.randn(rows, C, device=device), torch.randn(rows, C, device=device)
    m, r = torch.zeros(rows, device=device), torch.ones(rows, device=device)
    gw, bw = torch.ones(C, device=device), torch.ones(C, device=device)
    nws = ws_floats(rows, rps, C)
    assert nws > B                                        # (several blocks per sample: the workspace is needed)
    gt, Gt = guarded((B,), torch.float32, device, fill=3.0, name="d_time")
    gws, Gws = guarded((nws,), torch.float32, device, name="workspace")
    lib = ops.L()
    base = [ops.ptr(d), 0, ops.ptr(x), 0, ops.ptr(m), ops.ptr(r), ops.ptr(gw), ops.ptr(bw), None, ops.ptr(gt), rows, rps, C, ops.ptr(gws), nws * 4,
            ops.stream()]

    def call(**kw):
        a = list(base)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.scot_cln_dtime(*a)
    assert call(a1=7) == -3 and call(a3=2) == -3                  # dtype codes
    assert call(a10=rows + 1) == -3 and call(a11=0) == -3 and call(a12=0) == -3     # sizes
    assert call(a14=4) == -3 and call(a13=None) == -3             # workspace
    assert call(a6=None) == -3 and call(a9=None) == -3            # operands
    assert int(ops._raw().scot_cln_dtime_workspace_bytes(rows + 1, rps, C)) == 0
    check_all([Gt, Gws])
    assert float(gt.min()) == 3.0 and float(gt.max()) == 3.0
    assert call() == 0


# ------------------------------------------------------------------------------------------------ CPU emulation (small shapes)
@pytest.fixture()
def emu(monkeypatch):
    import emu_session
    lib = emu_session.load_emu()
    emu_session.patch_ops(monkeypatch, lib)
    return lib


SMALL = [(16, 1), (16, 49), (16, 64), (48, 64), (24, 49), (100, 49), (96, 1), (100, 1)]


@pytest.mark.parametrize("C,rps", SMALL)
def test_cln_dtime_guarded_small(emu, C, rps):
    for B in (1, 3):
        for dtype in (torch.float32, torch.bfloat16):
            for with_scale in (False, True):
                one_case(C, rps, B, dtype, with_scale, torch.device("cpu"))


@pytest.mark.parametrize("C,rps,B", [(48, 1024, 3), (100, 1024, 1), (192, 1024, 1)])
def test_cln_dtime_guarded_several_blocks_per_sample(emu, C, rps, B):
    """a sample split over several blocks: the partial sums meet through the workspace and the finishing launch"""
    assert ws_floats(B * rps, rps, C) > B
    one_case(C, rps, B, torch.float32, True, torch.device("cpu"))
    one_case(C, rps, B, torch.bfloat16, False, torch.device("cpu"))


def test_cln_dtime_f16_build(emu):
    prev = ops.use("f16")
    try:
        one_case(48, 64, 3, torch.float16, True, torch.device("cpu"))
        one_case(100, 49, 1, torch.float16, False, torch.device("cpu"))
    finally:
        ops.use(prev)


def test_cln_dtime_declines_unsupported_arguments(emu):
    declines(torch.device("cpu"))


# ------------------------------------------------------------------------------------------------ MI355X (the full list)
FULL_C = [16, 48, 96, 192, 384, 768, 1536, 24, 100]
FULL_RPS = [1, 49, 64, 1024, 16384]


@pytest.mark.gpu
@pytest.mark.parametrize("rps", FULL_RPS)
@pytest.mark.parametrize("C", FULL_C)
def test_cln_dtime_guarded_gpu(C, rps):
    dev = torch.device("cuda")
    for kind in ("bf16", "f16"):
        prev = ops.use(kind)
        try:
            for B in (1, 3):
                for dtype in ((torch.float32, ops.HALF[kind]) if kind == "bf16" else (ops.HALF[kind],)):
                    for with_scale in (False, True):
                        one_case(C, rps, B, dtype, with_scale, dev)
        finally:
            ops.use(prev)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_cln_dtime_declines_unsupported_arguments_gpu():
    declines(torch.device("cuda"))
    torch.cuda.synchronize()
