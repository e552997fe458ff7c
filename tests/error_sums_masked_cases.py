"""What the two scot_error_sums_masked test modules share (tests/test_error_sums_masked_emu_cpu.py on the CPU emulation,
tests/test_error_sums_masked_gpu.py on the MI355X): the shapes, the masks, the guarded launch and the checks.  A plain module on top of
tests/error_sums_cases.py; the callers pass its `Ctx`.

ORACLE.  The defining property of the masked kernel is an identity, not a tolerance: its sums are BIT FOR BIT what scot_error_sums returns
for the prediction `torch.where(mask, target, pred)`, and with overwrite = 1 it leaves exactly that tensor in `pred` (compared as int32).
So every check launches the unmasked kernel on the where-tensor and compares bits.  The fp64 bound of error_sums_cases.reference
(2·(n+2)·2⁻⁵³·ref per entry, derived there) is asserted on the where-tensor as well.

Operands, `sums`, the mask and the workspace are views inside the guard bands of tests/kernel_checks.py.  The mask's bands hold 0xA5, a
non-zero byte: a mask byte read outside the mask counts as "masked" and changes the sums."""
import numpy as np
import torch

import error_sums_cases as E
import kernel_checks as kc

# the shapes where the kernel can go wrong (error_sums_cases.CASES by name; the last one on the GPU only)
SHAPES = ("one_element", "short_odd_scalar", "vector_length_unaligned_start", "aligned_vector_pins_shape", "chunk_minus_1", "chunk",
          "chunk_plus_1", "two_chunks_plus_5", "preset_plane_128x128")
CASES = [c for c in E.CASES if c[0] in SHAPES]
assert len(CASES) == len(SHAPES)
# (label, element mask?, byte offset of the mask's base address)
MASKS = (("channel_none", False, 0), ("channel_all", False, 0), ("channel_per_sample", False, 0), ("element_30", True, 0),
         ("element_30_off1", True, 1), ("element_30_off3", True, 3))


def make_mask(label, B, C, HW):
    """bool [B, C] or [B, C, HW]"""
    if label == "channel_none":
        return torch.zeros(B, C, dtype=torch.bool)
    if label == "channel_all":
        return torch.ones(B, C, dtype=torch.bool)
    if label == "channel_per_sample":      # a different pattern per sample; at least one plane masked where there is more than one
        m = torch.tensor([[(b + 2 * c) % 3 == 0 for c in range(C)] for b in range(B)])
        if B * C > 1 and not m.any():
            m[-1, -1] = True
        return m
    g = torch.Generator().manual_seed(4242 + 31 * B + 7 * C + HW)
    return torch.rand(B, C, HW, generator=g) < 0.3


def where(mask, tg, pr):
    return torch.where(mask if mask.dim() == 3 else mask[:, :, None], tg, pr)


class MaskedLaunch(E.Launch):
    """E.Launch plus the mask as guarded bytes, its base address `offset` bytes off the 256-byte boundary"""

    def __init__(self, ctx, pr, tg, slices, mask, offset=0, **kw):
        super().__init__(ctx, pr, tg, slices, **kw)
        self.mask_full = int(mask is not None and mask.dim() == 3)
        self.mask_ptr = None
        if mask is not None:
            n = mask.numel()
            body, g = kc.guarded((n + offset,), torch.uint8, ctx.device, name="mask")      # (the first `offset` bytes keep the poison)
            # any non-zero byte means masked: use several
            body[offset:] = mask.reshape(-1).to(torch.uint8).to(ctx.device) * (1 + (torch.arange(n, device=ctx.device) % 200).to(torch.uint8))
            self.mask_body, self.mask_ptr = body, body.data_ptr() + offset
            assert self.mask_ptr % 4 == offset % 4
            self.guards.append(g)
        self.pred_before = self.pred.clone()

    def call_masked(self, overwrite):
        self.ws.fill_(0xFF)
        rc = self.ctx.lib.scot_error_sums_masked(self.pred.data_ptr(), self.target.data_ptr(), self.mask_ptr, self.mask_full, int(overwrite),
                                                 self.B, self.C, self.HW, None if self.slices is None else E.int_array(self.slices),
                                                 self.groups, self.sums.data_ptr(), self.ws.data_ptr(), self.ws_bytes, self.ctx.stream())
        self.ctx.sync()
        return rc

    def result(self):
        kc.check_all(self.guards)
        return self.sums.cpu().clone()

    def pred_bits(self):
        return self.pred.cpu().view(torch.int32)


def bits(x):
    return x.view(torch.int64)


def unmasked_sums(ctx, pr, tg, slices):
    L = E.Launch(ctx, pr, tg, slices)
    assert L.call() == 0
    return L.result()


def check_shape(ctx, B, C, HW, slices):
    """every mask of MASKS on one shape: the sums and the overwritten prediction against the where-tensor, bit for bit"""
    pr, tg = E.make_inputs(B, C, HW)
    plain = unmasked_sums(ctx, pr, tg, slices)
    null = MaskedLaunch(ctx, pr, tg, slices, None)
    assert null.call_masked(1) == 0                        # mask = NULL: scot_error_sums' bits, pred untouched (whatever `overwrite` says)
    assert torch.equal(bits(null.result()), bits(plain)) and torch.equal(null.pred_bits(), pr.view(torch.int32))
    ref_cache = {}
    for label, full, offset in MASKS:
        mask = make_mask(label, B, C, HW)
        key = label.split("_off")[0]
        if key not in ref_cache:
            w = where(mask, tg, pr)
            want = unmasked_sums(ctx, w, tg, slices)
            ref, ns = E.reference(w, tg, slices)           # the derived fp64 bound still holds on the where-tensor
            for g, n in enumerate(ns):
                assert (np.abs(want[:, g].numpy() - ref[:, g]) <= 2 * (n + 2) * E.U64 * ref[:, g]).all(), (label, g)
            ref_cache[key] = (w, want)
        w, want = ref_cache[key]
        for overwrite in (0, 1):
            L = MaskedLaunch(ctx, pr, tg, slices, mask, offset)
            assert L.call_masked(overwrite) == 0, (label, overwrite)
            got = L.result()
            assert torch.equal(bits(got), bits(want)), (label, overwrite, got, want)
            after = w if overwrite else pr
            assert torch.equal(L.pred_bits(), after.view(torch.int32)), (label, overwrite)
            assert L.call_masked(overwrite) == 0           # a second launch over a re-poisoned workspace: the same bits
            assert torch.equal(bits(L.result()), bits(want)) and torch.equal(L.pred_bits(), after.view(torch.int32)), (label, overwrite)


def check_operand_alignment(ctx):
    """pred 4 bytes off the 16-byte boundary with an aligned target, and the other way round, with run lengths that are multiples of 4:
    the masked kernel has to pick its load path from the pointers it really reads (the scalar one here), as scot_error_sums does — the
    sums and the overwritten prediction are the aligned launch's, bit for bit"""
    B, C, HW, slices = 2, 4, 256, E.PINS_SLICES
    pr, tg = E.make_inputs(B, C, HW)
    n = B * C * HW
    for label in ("channel_per_sample", "element_30"):
        mask = make_mask(label, B, C, HW)
        w = where(mask, tg, pr)
        want = unmasked_sums(ctx, w, tg, slices)
        for shifted in ("pred", "target"):
            for overwrite in (0, 1):
                L = MaskedLaunch(ctx, pr, tg, slices, mask)
                flat, g = kc.guarded((n + 1,), torch.float32, ctx.device, name=shifted + " (shifted)")
                flat[1:] = (pr if shifted == "pred" else tg).reshape(-1).to(ctx.device)
                setattr(L, shifted, flat[1:].view(B, C, HW))
                L.guards.append(g)
                assert L.pred.data_ptr() % 16 == (4 if shifted == "pred" else 0) and L.target.data_ptr() % 16 == (4 if shifted == "target" else 0)
                assert L.call_masked(overwrite) == 0
                assert torch.equal(bits(L.result()), bits(want)), (label, shifted, overwrite)
                assert torch.equal(L.pred_bits(), (w if overwrite else pr).view(torch.int32)), (label, shifted, overwrite)
                assert int(flat[:1].view(torch.int32)) == 0x7FDEAD01      # (the float in front of the shifted operand keeps the poison)


def check_nonfinite(ctx):
    B, C, HW, slices = 2, 4, 64, [0, 1, 3, 4]
    pr, tg = E.make_inputs(B, C, HW)
    for full in (False, True):
        mask = torch.zeros((B, C, HW) if full else (B, C), dtype=torch.bool)
        if full:
            mask[1, 2, 5] = mask[0, 0, 3] = mask[0, 3, 7] = True
        else:
            mask[1, 2] = mask[0, 0] = True
        clean = MaskedLaunch(ctx, pr, tg, slices, mask)
        assert clean.call_masked(0) == 0
        s0 = clean.result()
        assert torch.isfinite(s0).all()
        # NaN (and Inf) in pred at masked positions reach no sum: every sum finite and equal to the clean run's
        pr_bad = pr.clone()
        pr_bad[1, 2, 5], pr_bad[0, 0, 3] = float("nan"), float("inf")
        for overwrite in (0, 1):
            L = MaskedLaunch(ctx, pr_bad, tg, slices, mask)
            assert L.call_masked(overwrite) == 0
            s = L.result()
            assert torch.isfinite(s).all() and torch.equal(bits(s), bits(s0)), (full, overwrite, s)
            after = where(mask, tg, pr_bad) if overwrite else pr_bad
            assert torch.equal(L.pred_bits(), after.view(torch.int32))
        # +Inf in target at a masked position: d = Inf - Inf = NaN, as in the overwritten tensor: that (sample, group)'s N sums Inf, its
        # S sums NaN; all others unchanged
        tg_inf = tg.clone()
        tg_inf[1, 2, 5] = float("inf")
        want = unmasked_sums(ctx, where(mask, tg_inf, pr), tg_inf, slices)
        L = MaskedLaunch(ctx, pr, tg_inf, slices, mask)
        assert L.call_masked(0) == 0
        s = L.result()
        assert torch.isnan(s[1, 1, 0]) and torch.isnan(s[1, 1, 2]) and s[1, 1, 1] == float("inf") and s[1, 1, 3] == float("inf"), s[1, 1]
        keep = torch.ones(B, 3, 4, dtype=torch.bool)
        keep[1, 1] = False
        assert torch.equal(bits(s)[keep], bits(s0)[keep]) and torch.equal(bits(s)[keep], bits(want)[keep])
        assert torch.equal(torch.isnan(s), torch.isnan(want)) and torch.equal(s[1, 1, 1::2], want[1, 1, 1::2])


def check_refusals(ctx):
    """overwrite = 1 with groups that do not tile [0, C): -1, nothing launched, sums and pred untouched; overwrite = 0 takes them"""
    B, C, HW, slices = 2, 5, 64, [1, 3]
    pr, tg = E.make_inputs(B, C, HW)
    for full in (False, True):
        mask = torch.ones((B, C, HW) if full else (B, C), dtype=torch.bool)
        L = MaskedLaunch(ctx, pr, tg, slices, mask)
        assert L.call_masked(1) == -1
        kc.check_all(L.guards)
        assert L.sums_untouched() and torch.equal(L.pred_bits(), pr.view(torch.int32))
        assert bool((L.ws == 0xFF).all())
        assert L.call_masked(0) == 0
        assert torch.equal(bits(L.result()), bits(unmasked_sums(ctx, where(mask, tg, pr), tg, slices)))
        assert torch.equal(L.pred_bits(), pr.view(torch.int32))
    # the refusals of scot_error_sums hold with a mask too
    mask = torch.ones(B, C, dtype=torch.bool)
    for bad in ([0, 3, 1, 5], [0, 1, 1, 5], [0, 1, 3, 6]):
        L = MaskedLaunch(ctx, pr, tg, bad, mask, ws_bytes=4096)
        assert L.call_masked(1) == -1 and L.sums_untouched() and torch.equal(L.pred_bits(), pr.view(torch.int32))
    L = MaskedLaunch(ctx, pr, tg, [0, 2, 5], mask, ws_bytes=E.workspace_bytes(ctx, B, C, HW, [0, 2, 5]) - 1)
    assert L.call_masked(1) == -1 and L.sums_untouched()
