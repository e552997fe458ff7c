"""What the two scot_grad_accumulate test modules share (tests/test_grad_accumulate_emu_cpu.py on the CPU emulation,
tests/test_grad_accumulate_gpu.py on the MI355X): the maps, the guarded launch and the checks.  A plain module; the callers pass a `Ctx`.

  dst[i] = weight * grad[i]  (acc NULL)   or   acc[i] + weight * grad[i]      where map8[i / 8] != 255; every other float of dst keeps its bits

EXPECTATION.  `acc + grad * weight` as two eager fp32 torch operations on the operands' own device, compared with torch.equal: the product
is rounded, then the sum.  A kernel that contracts the two into an FMA rounds once.  Before a case judges the kernel it checks that its inputs
can tell the two apart: the single-rounding model (acc.double() + grad.double() * weight).float() differs from the expectation in at least one
mapped element (SEED is chosen so that this holds at every size, down to n = 8).

dst, acc and grad are views inside NaN bands (tests/kernel_checks.py), the map inside a band of its own; dst is pre-filled with SENTINEL, one
bit pattern no arithmetic on these inputs produces, so a float the kernel must not touch is provably untouched."""
import torch

import kernel_checks as kc

SENTINEL = 0x5EED1234                      # as fp32: 3.4e18
SEED = 3
WEIGHT = float(torch.tensor(1.0 / 3.0, dtype=torch.float32))      # the fp32 the C call receives, exactly
BAND = 4096
SIZES = (8, 8 * 257)                       # one lane; past one workgroup (256 lanes) with an odd tail
MAPS = ("groups", "edges", "none")         # no 255 at all; 255 at the first, last and a middle group; all 255
BLOCK_FLOATS = 8 * 2 * 256                  # floats one workgroup covers per trip (csrc/optim.hip: 256 lanes, two 8-float groups each)


class Ctx:
    """the library (its plan table typed), the device of the operands, the stream handle and the wait"""

    def __init__(self, lib, device, stream=lambda: None, sync=lambda: None):
        self.lib, self.device, self.stream, self.sync = lib, device, stream, sync


def full_sweep_plus_one_group(ctx):
    """one 8-float group more than a full sweep of the largest grid the kernel launches (from its own block rule)"""
    blocks = int(ctx.lib.scot_grad_accumulate_blocks(1 << 40))
    n = blocks * BLOCK_FLOATS + 8
    assert int(ctx.lib.scot_grad_accumulate_blocks(n)) == blocks and int(ctx.lib.scot_grad_accumulate_blocks(8)) == 1
    return n


def make_map(n, kind):
    n8 = n // 8
    if kind == "none":
        return torch.full((n8,), 255, dtype=torch.uint8)
    m = (torch.arange(n8) % 4).to(torch.uint8)
    if kind == "edges":
        m[0] = m[-1] = m[n8 // 2] = 255
    return m


def make_grads(n, steps=3, seed=SEED):
    g = torch.Generator().manual_seed(seed + n)
    return [torch.randn(n, generator=g) * (1.0 + k) for k in range(steps)]


class Launch:
    """one map and one gradient at a time, as guarded views on ctx.device; call() launches and waits"""

    def __init__(self, ctx, n, map_kind):
        self.ctx, self.n = ctx, n
        dev = ctx.device
        self.map, self.gm = kc.guarded((n // 8,), torch.uint8, dev, src=make_map(n, map_kind).to(dev), band=BAND, name="map8")
        self.on = (self.map != 255).repeat_interleave(8)
        self.grad, self.gg = kc.guarded((n,), torch.float32, dev, band=BAND, name="grad")
        self.guards = [self.gm, self.gg]

    def buffer(self, name):
        """a float buffer of n, every float the sentinel"""
        t, g = kc.guarded((self.n,), torch.float32, self.ctx.device, band=BAND, name=name)
        t.view(torch.int32).fill_(SENTINEL)
        self.guards.append(g)
        return t

    def call(self, dst, acc, weight, grad=None, n=None, map8=None):
        P = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())      # noqa: E731
        self.ctx.sync()
        rc = self.ctx.lib.scot_grad_accumulate(P(dst), P(acc), P(self.grad if grad is None else grad), P(self.map if map8 is None else map8),
                                               self.n if n is None else n, weight, self.ctx.stream())
        self.ctx.sync()
        return rc

    def check(self, dst, want):
        """want at the mapped positions, the sentinel everywhere else, every band intact"""
        assert torch.equal(dst[self.on], want[self.on])
        assert bool((dst.view(torch.int32)[~self.on] == SENTINEL).all())
        kc.check_all(self.guards)


def check_three_adds(ctx, n, map_kind, in_place):
    """A0 = w g0 (acc NULL), A1 = A0 + w g1, A2 = A1 + w g2: in place (dst == acc) or each into a fresh buffer"""
    L = Launch(ctx, n, map_kind)
    grads = [g.to(ctx.device) for g in make_grads(n)]
    told_apart = False
    A = want = None
    for k, g in enumerate(grads):
        L.grad.copy_(g)
        prod = L.grad * WEIGHT
        want_k = prod if k == 0 else want + prod
        if k:
            fused = (want.double() + L.grad.double() * WEIGHT).float()
            told_apart |= bool((fused != want_k)[L.on].any())
        dst = L.buffer(f"A{k}") if (k == 0 or not in_place) else A
        assert L.call(dst, None if k == 0 else A, WEIGHT) == 0
        want = want_k      # (its unmapped floats are never compared)
        L.check(dst, want)
        if k and not in_place:
            assert torch.equal(A.view(torch.int32), prev_bits)                    # acc is read only
        A, prev_bits = dst, dst.view(torch.int32).clone()
    assert told_apart or not bool(L.on.any()), "these inputs cannot tell an FMA from two roundings: choose another SEED"


SPECIAL = (-0.0, 0.0, 1e-45, -1e-45, 1.1754942e-38, -5.877e-39, float("inf"), float("-inf"), 1.0, -3.5, 3.4028235e38, 1.17549435e-38)


def check_copy_keeps_bits(ctx, n):
    """weight = 1, acc NULL: a masked copy that keeps -0.0, denormals, +-Inf and ordinary values bit for bit"""
    L = Launch(ctx, n, "edges" if n > 24 else "groups")
    vals = torch.tensor(SPECIAL, dtype=torch.float32).repeat((n + len(SPECIAL) - 1) // len(SPECIAL))[:n]
    assert bool((vals.abs() < 1.1754944e-38).logical_and(vals != 0).any())                    # denormals are among them
    L.grad.copy_(vals.to(ctx.device))
    dst = L.buffer("dst")
    assert L.call(dst, None, 1.0) == 0
    assert torch.equal(dst.view(torch.int32)[L.on], L.grad.view(torch.int32)[L.on])
    assert bool((dst.view(torch.int32)[~L.on] == SENTINEL).all())
    kc.check_all(L.guards)


def check_nonfinite(ctx, n=8 * 257):
    """NaN stays NaN, Inf gives Inf, Inf + (-Inf) gives NaN: each in exactly the element it enters"""
    L = Launch(ctx, n, "groups")
    g = make_grads(n, 1)[0]
    i_nan, i_inf, i_mix = 5, n // 2 + 3, n - 2
    g[i_nan], g[i_inf], g[i_mix] = float("nan"), float("inf"), float("-inf")
    L.grad.copy_(g.to(ctx.device))
    first = L.buffer("first")
    assert L.call(first, None, WEIGHT) == 0
    assert bool(torch.isnan(first[i_nan])) and float(first[i_inf]) == float("inf") and float(first[i_mix]) == float("-inf")
    others = torch.ones(n, dtype=torch.bool, device=ctx.device)
    others[[i_nan, i_inf, i_mix]] = False
    assert bool(torch.isfinite(first[others]).all())
    acc = L.buffer("acc")
    acc.copy_(make_grads(n, 1, seed=SEED + 1)[0].to(ctx.device))
    acc[i_mix] = float("inf")
    out = L.buffer("out")
    assert L.call(out, acc, WEIGHT) == 0
    assert bool(torch.isnan(out[i_nan])) and float(out[i_inf]) == float("inf") and bool(torch.isnan(out[i_mix]))
    assert bool(torch.isfinite(out[others]).all()) and torch.equal(out[others], (acc + L.grad * WEIGHT)[others])
    kc.check_all(L.guards)


def check_refusals(ctx, n=64):
    """every refusal of the header: -1, dst bit-unchanged"""
    L = Launch(ctx, n, "groups")
    L.grad.copy_(make_grads(n, 1)[0].to(ctx.device))
    dst, acc = L.buffer("dst"), L.buffer("acc")
    room = L.buffer("room")      # (a misaligned view needs n floats behind its start)
    cases = {
        "NULL dst": dict(dst=None, acc=acc), "NULL grad": dict(dst=dst, acc=acc, grad=0), "NULL map8": dict(dst=dst, acc=acc, map8=0),      # (address 0)
        "n == 0": dict(dst=dst, acc=acc, n=0), "n % 8 != 0": dict(dst=dst, acc=acc, n=12),
        "dst not 16-byte aligned": dict(dst=room.data_ptr() + 4, acc=None, n=n - 8),
        "acc not 16-byte aligned": dict(dst=dst, acc=room.data_ptr() + 8, n=n - 8),
        "grad not 16-byte aligned": dict(dst=dst, acc=None, grad=L.grad.data_ptr() + 4, n=n - 8),
        "weight inf": dict(dst=dst, acc=acc, weight=float("inf")), "weight nan": dict(dst=dst, acc=acc, weight=float("nan")),
        "dst == grad": dict(dst=L.grad, acc=acc),
    }
    grad_bits = L.grad.view(torch.int32).clone()
    for label, kw in cases.items():
        kw = dict(kw)
        assert L.call(kw.pop("dst"), kw.pop("acc"), kw.pop("weight", WEIGHT), **kw) == -1, label
        for t in (dst, acc, room):
            assert bool((t.view(torch.int32) == SENTINEL).all()), label
        assert torch.equal(L.grad.view(torch.int32), grad_bits), label
    kc.check_all(L.guards)
    assert L.call(dst, None, WEIGHT) == 0      # ... and the same operands are accepted
