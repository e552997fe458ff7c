"""What the two scot_error_sums test modules share (tests/test_error_sums_emu_cpu.py on the CPU emulation, tests/test_error_sums_gpu.py on the
MI355X): the case list, the guarded launch, the fp64 reference and the bound.  A plain module; the callers pass a `Ctx`.

  sums[b][g] = { Σ|p−t|, Σ|t|, Σ(p−t)², Σt² } over the channels of group g and all pixels of sample b, every term and sum in fp64.

BOUND.  All terms are non-negative, so an n-term fp64 sum in ANY order errs by at most (n−1)·2⁻⁵³·Σ to first order (Higham §4.2), and
each term carries at most two roundings (the subtraction of two exactly converted fp32 values, the square); hence per entry

  |got − ref| ≤ 2·(n+2)·2⁻⁵³·ref,        n = (c1−c0)·HW

with the numpy fp64 reference on the same fp32 inputs (whose own error has the same form: the factor 2).  Derived, not measured.

Operands and `sums` are views inside NaN bands (tests/kernel_checks.py): an over-read shows as a NaN sum, a stray store changes a band.
The workspace is 0xff bytes before every launch (as fp64: NaN), inside bands of its own."""
import ctypes

import numpy as np
import torch

import kernel_checks as kc

CHUNK = 4096          # floats of a run one workgroup reduces (csrc/error_sums.hip); test_chunk_constant checks it through the workspace query
U64 = 2.0 ** -53
PINS_SLICES = [0, 1, 3, 4]

# (id, B, C, HW, slices or None, channels filled with NaN, GPU only)
CASES = [
    ("one_element", 1, 1, 1, [0, 1], (), False),
    ("short_odd_scalar", 2, 3, 3, [0, 1, 3], (), False),
    ("vector_length_unaligned_start", 2, 4, 6, [0, 1, 3, 4], (), False),
    ("aligned_vector_pins_shape", 6, 4, 256, [0, 1, 3, 4], (), False),
    ("chunk_minus_1", 1, 1, CHUNK - 1, None, (), False),
    ("chunk", 1, 1, CHUNK, None, (), False),
    ("chunk_plus_1", 1, 1, CHUNK + 1, None, (), False),
    ("two_chunks_plus_5", 2, 1, 2 * CHUNK + 5, None, (), False),
    ("channels_outside_groups_are_nan", 2, 5, 64, [1, 3], (0, 3, 4), False),
    ("preset_plane_128x128", 2, 4, 16384, [0, 1, 3, 4], (), True),
]


class Ctx:
    """the library (its plan table typed), the device of the operands, the stream handle and the wait"""

    def __init__(self, lib, device, stream=lambda: None, sync=lambda: None):
        self.lib, self.device, self.stream, self.sync = lib, device, stream, sync


def int_array(values):
    return ctypes.cast((ctypes.c_int * max(1, len(values)))(*values), ctypes.c_void_p)


def make_inputs(B, C, HW, nan_channels=(), seed=0):
    g = torch.Generator().manual_seed(1000 * C + 7 * HW + B + seed)
    tg = torch.randn(B, C, HW, generator=g) * 1.5 + 0.25
    pr = tg + 0.1 * torch.randn(B, C, HW, generator=g)
    for c in nan_channels:
        pr[:, c] = float("nan")
        tg[:, c] = float("nan")
    return pr, tg


def reference(pr, tg, slices):
    """numpy in fp64 on the same fp32 inputs -> ([B, G, 4], n per group)"""
    p, t = pr.numpy().astype(np.float64), tg.numpy().astype(np.float64)
    sl = slices if slices is not None else [0, pr.shape[1]]
    out = np.empty((pr.shape[0], len(sl) - 1, 4))
    for g, (a, b) in enumerate(zip(sl, sl[1:])):
        d, tt = p[:, a:b] - t[:, a:b], t[:, a:b]
        out[:, g] = np.stack([np.abs(d).sum((1, 2)), np.abs(tt).sum((1, 2)), (d * d).sum((1, 2)), (tt * tt).sum((1, 2))], -1)
    return out, [(b - a) * pr.shape[2] for a, b in zip(sl, sl[1:])]


def workspace_bytes(ctx, B, C, HW, slices, groups=None):
    groups = (1 if slices is None else len(slices) - 1) if groups is None else groups
    return int(ctx.lib.scot_error_sums_workspace_bytes(B, C, HW, None if slices is None else int_array(slices), groups))


class Launch:
    """pred, target, sums and the workspace as guarded views on ctx.device; call() launches (workspace poisoned first) and waits"""

    def __init__(self, ctx, pr, tg, slices, groups=None, ws_bytes=None):
        self.ctx, self.slices = ctx, slices
        self.B, self.C, self.HW = pr.shape
        self.groups = (1 if slices is None else len(slices) - 1) if groups is None else groups
        dev = ctx.device
        self.pred, g0 = kc.guarded(tuple(pr.shape), torch.float32, dev, src=pr.to(dev), name="pred")
        self.target, g1 = kc.guarded(tuple(tg.shape), torch.float32, dev, src=tg.to(dev), name="target")
        self.sums, g2 = kc.guarded((self.B, max(1, min(self.groups, 32)), 4), torch.float64, dev, name="sums")
        need = workspace_bytes(ctx, self.B, self.C, self.HW, slices, groups) if ws_bytes is None else ws_bytes
        self.ws_bytes = need
        self.ws, g3 = kc.guarded((max(8, need),), torch.uint8, dev, fill=0xFF, name="workspace")
        self.guards = [g0, g1, g2, g3]
        self.sums_poison = g2.poison

    def call(self):
        self.ws.fill_(0xFF)
        rc = self.ctx.lib.scot_error_sums(self.pred.data_ptr(), self.target.data_ptr(), self.B, self.C, self.HW,
                                          None if self.slices is None else int_array(self.slices), self.groups, self.sums.data_ptr(),
                                          self.ws.data_ptr(), self.ws_bytes, self.ctx.stream())
        self.ctx.sync()
        return rc

    def sums_untouched(self):
        return bool((self.sums.view(torch.int64) == self.sums_poison).all())

    def result(self):
        kc.check_all(self.guards[:3])
        # (the workspace's own bands: its body is the kernel's to write)
        kc.check_all(self.guards[3:])
        return self.sums.cpu().clone()


def check_case(ctx, B, C, HW, slices, nan_channels):
    pr, tg = make_inputs(B, C, HW, nan_channels)
    L = Launch(ctx, pr, tg, slices)
    assert L.ws_bytes > 0 and L.ws_bytes % 32 == 0
    assert L.call() == 0
    got = L.result()
    ref, ns = reference(pr, tg, slices)
    assert torch.isfinite(got).all(), got
    for g, n in enumerate(ns):
        err = np.abs(got[:, g].numpy() - ref[:, g])
        bound = 2 * (n + 2) * U64 * ref[:, g]
        print(f"\n[error_sums] B={B} C={C} HW={HW} group {g}: n={n}, worst |got-ref|/bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert (err <= bound).all(), (g, n, err, bound)
    assert L.call() == 0                                  # repeatability: the same bits from a second launch (over a poisoned workspace)
    assert torch.equal(L.result().view(torch.int64), got.view(torch.int64))
    return got


def check_chunk_constant(ctx):
    assert workspace_bytes(ctx, 1, 1, CHUNK, None) == 32 and workspace_bytes(ctx, 1, 1, CHUNK + 1, None) == 64
    assert workspace_bytes(ctx, 3, 4, CHUNK, [0, 1, 3, 4]) == 3 * (1 + 2 + 1) * 32


def check_nonfinite(ctx):
    B, C, HW, slices = 2, 4, 64, [0, 1, 3, 4]
    pr, tg = make_inputs(B, C, HW)
    base = Launch(ctx, pr, tg, slices)
    assert base.call() == 0
    s0 = base.result()
    assert torch.isfinite(s0).all()
    # +Inf in one target element: all four sums of its (sample, group)
    tg_inf = tg.clone()
    tg_inf[1, 2, 5] = float("inf")
    L = Launch(ctx, pr, tg_inf, slices)
    assert L.call() == 0
    s = L.result()
    assert (s[1, 1] == float("inf")).all(), s[1, 1]
    keep = torch.ones(B, 3, 4, dtype=torch.bool)
    keep[1, 1] = False
    assert torch.equal(s.view(torch.int64)[keep], s0.view(torch.int64)[keep])
    # NaN in one prediction element: only the two error sums of its (sample, group)
    pr_nan = pr.clone()
    pr_nan[0, 0, 3] = float("nan")
    L = Launch(ctx, pr_nan, tg, slices)
    assert L.call() == 0
    s = L.result()
    assert torch.isnan(s[0, 0, 0]) and torch.isnan(s[0, 0, 2])
    keep = torch.ones(B, 3, 4, dtype=torch.bool)
    keep[0, 0, 0] = keep[0, 0, 2] = False
    assert torch.equal(s.view(torch.int64)[keep], s0.view(torch.int64)[keep])


def check_refusals(ctx):
    B, C, HW = 2, 4, 6
    pr, tg = make_inputs(B, C, HW)
    enough = workspace_bytes(ctx, B, C, HW, [0, 1, 3, 4])
    bad = [("groups 0", list(range(34)), 0), ("groups 33", list(range(34)), 33), ("descending", [0, 3, 1, 4], None),
           ("equal", [0, 1, 1, 4], None), ("beyond C", [0, 1, 3, 5], None), ("negative", [-1, 1, 3, 4], None)]
    for label, slices, groups in bad:
        assert workspace_bytes(ctx, B, 40 if groups is not None else C, HW, slices, groups) == 0, label
        L = Launch(ctx, pr if groups is None else make_inputs(B, 40, HW)[0], tg if groups is None else make_inputs(B, 40, HW)[1], slices,
                   groups, ws_bytes=max(enough, 4096))
        assert L.call() == -1, label
        kc.check_all(L.guards)
        assert L.sums_untouched(), label
    L = Launch(ctx, pr, tg, [0, 1, 3, 4], ws_bytes=enough - 1)      # one byte short
    assert L.call() == -1
    kc.check_all(L.guards)
    assert L.sums_untouched()
    L = Launch(ctx, pr, tg, [0, 1, 3, 4], ws_bytes=enough)
    assert L.call() == 0 and not L.sums_untouched()


def pins_operands():
    """the operands tests/test_harness_cpu.py pins the metrics with: closed-form tensors, one sample with an all-zero target"""
    from poseidon_amd.synth import closed_form_tensor
    pr = np.asarray(closed_form_tensor("metrics:pred", (6, 4, 16, 16), 1.0), dtype=np.float32)
    tg = np.asarray(closed_form_tensor("metrics:target", (6, 4, 16, 16), 1.0), dtype=np.float32)
    tg[3] = 0.0
    return pr, tg


def close(a, b, tol=2e-6):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) <= tol * np.maximum(np.abs(b), 1e-30)))


def check_pins(sums_of):
    """sums_of(pred, target, slices or None) -> [6, G, 4]: the `*_from_sums` helpers on those sums reproduce tests/golden/metrics_pins.json,
    values of the real reference's metrics module, within the tolerance tests/test_harness_cpu.py uses (2e-6 relative; 1e-5 for std)"""
    import json
    import os
    from scOT import metrics as M
    pins = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_pins.json")))
    pr, tg = pins_operands()
    one = sums_of(pr, tg, None)
    assert tuple(one.shape) == (6, 1, 4) and one.dtype in (torch.float64, np.float64)
    assert float(one[3, 0, 1]) == 0.0 and float(one[3, 0, 3]) == 0.0       # the zero-target sample: the 1e-10 guard is exercised
    for p in (1, 2):
        assert close(M.lp_error_from_sums(one, p)[:, 0], pins[f"lp_error_p{p}"])
        rel = M.relative_lp_error_from_sums(one, p)[:, 0]
        assert close(rel, pins[f"relative_lp_error_p{p}"])
        assert close(M.relative_lp_error_from_sums(one, p, return_percent=False)[:, 0], pins[f"relative_lp_error_p{p}_nopercent"])
        rel = torch.as_tensor(rel).double().cpu()
        assert close(rel.mean(), pins[f"mean_relative_p{p}"]) and close(float(np.median(rel.numpy())), pins[f"median_relative_p{p}"])
    grouped = sums_of(pr, tg, PINS_SLICES)
    out = M.group_metrics_from_sums(grouped, ["rho", "uv", "p"])
    for i, n in enumerate(["rho", "uv", "p"]):
        g = pins[f"group{i}"]
        assert close(out[n + "/median_relative_l1_error"], g["median_rel"]) and close(out[n + "/mean_relative_l1_error"], g["mean_rel"])
        assert close(out[n + "/std_relative_l1_error"], g["std_rel"], 1e-5) and close(out[n + "/max_relative_l1_error"], g["max_rel"])
        assert close(out[n + "/median_l1_error"], g["median_abs"]) and close(out[n + "/std_l1_error"], g["std_abs"], 1e-5)
    assert close(out["mean_relative_l1_error"], np.mean([pins[f"group{i}"]["mean_rel"] for i in range(3)]))
    assert close(out["mean_over_median_l1_error"], np.mean([pins[f"group{i}"]["median_abs"] for i in range(3)]))
    # the same keys, the same numbers as the torch-op path on the same operands
    want = M.channel_group_metrics(torch.from_numpy(pr), torch.from_numpy(tg), PINS_SLICES, ["rho", "uv", "p"])
    assert set(out) == set(want) and all(close(out[k], want[k]) for k in want)
    single = M.group_metrics_from_sums(one, full_data=True)
    want1 = M.channel_group_metrics(pr, tg, [0, 4], full_data=True)
    assert set(single) == set(want1) and all(close(single[k], want1[k]) for k in want1)
    return one
