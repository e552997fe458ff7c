"""What the two scot_spectral_resize test modules share (tests/test_spectral_resize_emu_cpu.py on the CPU emulation,
tests/test_spectral_resize_gpu.py on the MI355X): the case lists, the guarded launch, the fp64 reference and the bound.  A plain module;
the callers pass a `Ctx`.

  Y[b] = Pr X[b] Pr^T - Pi X[b] Pi^T          X [nimg, s, s], Pr / Pi [t, s], Y [nimg, t, t], fp32 (csrc/spectral_resize.hip)

BOUND (K1, K6).  The kernel forms W = fl(P X) — one length-s contraction per element, fp32 products exact in the MFMA, fp32 accumulation:
|W - P X| <= s u |P||X| to first order (Higham §3.1) — and then ONE chain of 2 s terms Wr Pr^T + (-Wi) Pi^T, whose own rounding is at most
2 s u (|Wr||Pr|^T + |Wi||Pi|^T); the error of W enters through |P|^T once more: s u.  Contracting in the other order (X P^T first, then
two length-s products and a subtraction) gives s u + s u + u.  Either way, per element,

  |Y - Y64| <= (3 s + 4) u (|Pr||X||Pr|^T + |Pi||X||Pi|^T),      u = 2^-24

with Y64 in fp64 from the same fp32 operands (the 4: the subtraction, the fp64 reference's own error and second-order terms, generously).
Derived, not measured.

Every operand and Y are views inside NaN bands (tests/kernel_checks.py): an over-read shows as a NaN in Y — the kernel contracts over s
rounded up to 32 and over row tiles of 16, with zeros SUPPLIED beyond the extents —, a stray store changes a band."""
import torch

import kernel_checks as kc

U32 = 2.0 ** -24
K1_SHAPES = [(16, 32), (32, 16), (20, 12), (12, 20), (17, 33), (33, 17), (64, 48), (1, 5), (5, 1)]
K2_SHAPES = [(32, 64), (32, 16), (64, 32), (24, 40)]
K6_SHAPES = [(256, 128), (128, 256)]      # GPU only, nimg = 8


class Ctx:
    """the library, the binary16 build of it, the device of the operands, the stream handle and the wait"""

    def __init__(self, lib, lib_f16, device, stream=lambda: None, sync=lambda: None):
        self.lib, self.lib_f16, self.device, self.stream, self.sync = lib, lib_f16, device, stream, sync


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def operands(nimg, s, t, seed=0):
    g = torch.Generator().manual_seed(100003 * s + 101 * t + nimg + seed)
    return (torch.randn(nimg, s, s, generator=g), torch.randn(t, s, generator=g) / s ** 0.5, torch.randn(t, s, generator=g) / s ** 0.5)


def reference(X, Pr, Pi):
    """fp64 on the same fp32 operands -> (Y64, the magnitude |Pr||X||Pr|^T + |Pi||X||Pi|^T)"""
    x, pr, pi = X.double(), Pr.double(), Pi.double()
    y = pr @ x @ pr.T - pi @ x @ pi.T
    mag = pr.abs() @ x.abs() @ pr.abs().T + pi.abs() @ x.abs() @ pi.abs().T
    return y, mag


class Launch:
    """X, Pr, Pi and Y as guarded views on ctx.device (Y's body keeps the poison); call() launches and waits"""

    def __init__(self, ctx, X, Pr, Pi):
        self.ctx = ctx
        self.nimg, self.s, self.t = X.shape[0], X.shape[1], Pr.shape[0]
        dev = ctx.device
        self.X, g0 = kc.guarded(tuple(X.shape), torch.float32, dev, src=X.to(dev), name="X")
        self.Pr, g1 = kc.guarded(tuple(Pr.shape), torch.float32, dev, src=Pr.to(dev), name="Pr")
        self.Pi, g2 = kc.guarded(tuple(Pi.shape), torch.float32, dev, src=Pi.to(dev), name="Pi")
        self.Y, g3 = kc.guarded((self.nimg, self.t, self.t), torch.float32, dev, name="Y")
        self.guards, self.poison = [g0, g1, g2, g3], g3.poison

    def call(self, lib=None, **over):
        a = dict(X=self.X.data_ptr(), Pr=self.Pr.data_ptr(), Pi=self.Pi.data_ptr(), Y=self.Y.data_ptr(), nimg=self.nimg, s=self.s, t=self.t)
        a.update(over)
        rc = (lib or self.ctx.lib).scot_spectral_resize(a["X"], a["Pr"], a["Pi"], a["Y"], a["nimg"], a["s"], a["t"], self.ctx.stream())
        self.ctx.sync()
        return rc

    def untouched(self):
        kc.check_all(self.guards)
        return bool((self.Y.view(torch.int32) == self.poison).all())

    def result(self):
        kc.check_all(self.guards)
        return self.Y.cpu().clone()


def check_bound(ctx, nimg, s, t):
    """K1 / K6 -> the result"""
    X, Pr, Pi = operands(nimg, s, t)
    L = Launch(ctx, X, Pr, Pi)
    assert L.call() == 0
    got = L.result()
    ref, mag = reference(X, Pr, Pi)
    assert torch.isfinite(got).all(), f"s {s} t {t} nimg {nimg}: a non-finite output (an operand was read outside its extent)"
    err, bound = (got.double() - ref).abs(), (3 * s + 4) * U32 * mag
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"\n[spectral_resize] s={s} t={t} nimg={nimg}: worst |Y-Y64|/bound = {worst:.3f}")
    assert (err <= bound).all(), (s, t, nimg, worst)
    return got


def check_bits(ctx, s=20, t=12):
    """K3: run to run, a plane alone against the same plane in a batch of 3, both builds"""
    X, Pr, Pi = operands(3, s, t, seed=3)
    L = Launch(ctx, X, Pr, Pi)
    assert L.call() == 0
    first = L.result()
    L.Y.view(torch.int32).fill_(L.poison)
    assert L.call() == 0
    assert torch.equal(L.result().view(torch.int32), first.view(torch.int32))
    for b in range(3):
        one = Launch(ctx, X[b:b + 1], Pr, Pi)
        assert one.call() == 0
        assert torch.equal(one.result().view(torch.int32)[0], first.view(torch.int32)[b]), b
    other = Launch(ctx, X, Pr, Pi)
    assert other.call(lib=ctx.lib_f16) == 0
    assert torch.equal(other.result().view(torch.int32), first.view(torch.int32))


def check_nonfinite(ctx, s=20, t=12):
    """K4: a NaN, and an Inf, in plane 1 of 3"""
    X, Pr, Pi = operands(3, s, t, seed=4)
    base = Launch(ctx, X, Pr, Pi)
    assert base.call() == 0
    want = base.result()
    for bad in (float("nan"), float("inf")):
        Xb = X.clone()
        Xb[1, s // 2, s // 3] = bad
        L = Launch(ctx, Xb, Pr, Pi)
        assert L.call() == 0
        got = L.result()
        # (every output element of the plane depends on every input element through two dense products with non-zero operators)
        assert not torch.isfinite(got[1]).any(), bad
        for b in (0, 2):
            assert torch.equal(got[b].view(torch.int32), want[b].view(torch.int32)), (bad, b)


def check_refusals(ctx):
    """K5: every refusal returns its code, launches nothing: Y keeps its guard fill"""
    X, Pr, Pi = operands(2, 8, 12)
    L = Launch(ctx, X, Pr, Pi)
    bad = [("X NULL", dict(X=None), -1), ("Pr NULL", dict(Pr=None), -1), ("Pi NULL", dict(Pi=None), -1), ("Y NULL", dict(Y=None), -1),
           ("nimg 0", dict(nimg=0), -1), ("nimg -1", dict(nimg=-1), -1), ("s 0", dict(s=0), -1), ("t 0", dict(t=0), -1),
           ("s -3", dict(s=-3), -1), ("X unaligned", dict(X=L.X.data_ptr() + 4), -1), ("Pr unaligned", dict(Pr=L.Pr.data_ptr() + 8), -1),
           ("Pi unaligned", dict(Pi=L.Pi.data_ptr() + 4), -1), ("Y unaligned", dict(Y=L.Y.data_ptr() + 4), -1),
           ("Y == X", dict(Y=L.X.data_ptr()), -1), ("s 513", dict(s=513), -3), ("t 513", dict(t=513), -3)]
    before = L.X.clone()
    for label, over, code in bad:
        assert L.call(**over) == code, label
        assert L.untouched(), label
        assert torch.equal(L.X, before), label
    assert L.call() == 0 and not L.untouched()


def check_real_operators(s, t, device):
    """K2: scOT.model.spectral_resize(..., fused=True) against the reference's fft2 -> crop / pad -> ifft2 (oracle.scot_cpu), forward and
    gradient, within the bound of the two-launch path's test (tests/test_kernels_emu_cpu.py::test_spectral_resize_native)"""
    from oracle.scot_cpu import spectral_resize as ref_resize
    from scOT.model import spectral_resize
    g = torch.Generator().manual_seed(11 * s + t)
    x = torch.randn(2, 3, s, s, generator=g).to(device).requires_grad_(True)
    y = spectral_resize(x, t, fused=True)
    xr = x.detach().cpu().double().requires_grad_(True)
    yr = ref_resize(xr, t)
    assert tuple(y.shape) == (2, 3, t, t) and rel(y.detach().cpu(), yr.detach()) < 2e-6
    gy = torch.randn(2, 3, t, t, generator=g)
    y.backward(gy.to(device))
    yr.backward(gy.double())
    assert rel(x.grad.cpu(), xr.grad) < 2e-6
    plain = spectral_resize(x.detach(), t)
    assert rel(plain.cpu(), y.detach().cpu()) < 2e-6      # (the default path is a different summation order: close, not equal)


def check_declared(lib):
    """K7: header, prototypes and ABI"""
    import os
    import re
    from conftest import ROOT
    from poseidon_amd import lib as scotlib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scot_hip.h")).read(), flags=re.S)
    assert re.search(r"int scot_spectral_resize\(const float\* X, const float\* Pr, const float\* Pi, float\* Y, int nimg, int s, int t, "
                     r"scot_stream_t stream\);", header)
    P, I = scotlib.P, scotlib.I
    assert scotlib.PROTOTYPES["scot_spectral_resize"] == [P, P, P, P, I, I, I, P]
    assert "scot_spectral_apply" in scotlib.PROTOTYPES and "scot_plan_describe_resize" in scotlib.PLAN_PROTOTYPES
    assert scotlib.ABI_VERSION == 8 and lib.scot_abi_version() == 8
