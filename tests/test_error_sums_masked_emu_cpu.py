"""scot_error_sums_masked (csrc/error_sums.hip) on the CPU emulation: the kernel source itself runs, one fiber per work-item, inside
guard bands; the shapes, the masks and the bit-for-bit oracle (scot_error_sums on the where-tensor) are tests/error_sums_masked_cases.py's,
shared with the GPU module."""
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
import error_sums_cases as E  # noqa: E402
import error_sums_masked_cases as MC  # noqa: E402
from poseidon_amd import lib as scotlib, ops, plan as plan_mod  # noqa: E402

NEW = {"scot_error_sums_masked", "scot_plan_evaluate_masked", "scot_plan_loss_masked", "scot_plan_train_step_masked"}


@pytest.fixture(scope="module")
def ctx():
    import emu_session
    return E.Ctx(plan_mod.bind(emu_session.load_emu()), torch.device("cpu"))


@pytest.mark.parametrize("case", [c for c in MC.CASES if not c[6]], ids=lambda c: c[0])
def test_sums_and_overwrite_equal_the_where_tensor_bit_for_bit(ctx, case):
    _, B, C, HW, slices, _, _ = case
    MC.check_shape(ctx, B, C, HW, slices)


def test_operands_off_the_16_byte_boundary_take_the_scalar_path(ctx):
    MC.check_operand_alignment(ctx)


def test_nonfinite_values_under_the_mask(ctx):
    MC.check_nonfinite(ctx)


def test_refusals_leave_sums_and_pred_untouched(ctx):
    MC.check_refusals(ctx)


def test_metrics_error_sums_with_a_pixel_mask(ctx, monkeypatch):
    """scOT.metrics.error_sums(..., pixel_mask=): the CPU path is error_sums of the where-tensor; the ops wrapper (what GPU tensors
    take) launches the masked kernel with overwrite = 0 and gives the unmasked kernel's bits on the where-tensor"""
    import emu_session
    from scOT import metrics as M
    B, C, HW, slices = 3, 4, 100, [0, 1, 3, 4]
    pr, tg = E.make_inputs(B, C, HW)
    pr4, tg4 = pr.view(B, C, 10, 10), tg.view(B, C, 10, 10)
    chan = MC.make_mask("channel_per_sample", B, C, HW)
    elem = MC.make_mask("element_30", B, C, HW).view(B, C, 10, 10)
    one = elem[:, :1]
    for mask, full in ((chan, chan[:, :, None, None].expand(B, C, 10, 10)), (elem, elem), (one, one.expand(B, C, 10, 10)),
                       (chan.to(torch.uint8), chan[:, :, None, None].expand(B, C, 10, 10))):
        w = torch.where(full, tg4, pr4)
        assert torch.equal(M.error_sums(pr4, tg4, slices, pixel_mask=mask), M.error_sums(w, tg4, slices))
        assert torch.equal(M.error_sums(pr4.numpy(), tg4.numpy(), None, pixel_mask=mask.numpy()), M.error_sums(w, tg4))
    with pytest.raises(ValueError, match="pixel_mask"):
        M.error_sums(pr4, tg4, slices, pixel_mask=torch.ones(B, 10, 10, dtype=torch.bool))
    emu_session.patch_ops(monkeypatch, ctx.lib)
    for mask in (chan, elem.reshape(B, C, HW)):
        out = torch.full((B, 3, 4), float("nan"), dtype=torch.float64)
        before = pr.clone()
        ops.error_sums(pr, tg, slices, out, mask.to(torch.uint8).contiguous(), mask.dim() == 3)
        want = torch.empty_like(out)
        ops.error_sums(MC.where(mask, tg, pr).contiguous(), tg, slices, want)
        assert torch.equal(out.view(torch.int64), want.view(torch.int64)) and torch.equal(pr, before)


def test_header_and_prototypes_declare_the_new_calls(ctx):
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "scot_plan.h")).read()
    declared = set(re.findall(r"\b(scot_[a-z0-9_]+)\s*\(", header))
    assert declared == set(scotlib.PLAN_PROTOTYPES) and NEW <= declared
    assert not NEW & set(scotlib.PROTOTYPES) and scotlib.ABI_VERSION == 8 and ctx.lib.scot_abi_version() == 8      # the ABI number stands
    kernel_header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scot_hip.h")).read(), flags=re.S)
    assert "scot_error_sums_masked" not in kernel_header
    listed = set(plan_mod.runtime_entry_points(ctx.lib)) | set(plan_mod.runtime_entry_points(ctx.lib, adjoint=True)) | \
        set(plan_mod.runtime_entry_points(ctx.lib, training=True))
    assert not NEW & listed                                # no recorded call list can name them
    assert "constant in time" in header                    # the one documented difference from the reference's rollout


def test_gfx950_builds_export_the_new_calls():
    for kind in ("bf16", "f16"):
        lib = scotlib.load(kind=kind)
        for name in NEW:
            assert getattr(lib, name).argtypes == scotlib.PLAN_PROTOTYPES[name]
        assert lib.scot_error_sums_masked(None, None, None, 0, 0, 1, 1, 1, None, 1, None, None, 0, None) == -1
        assert lib.scot_plan_evaluate_masked(None, None, None, None, None, 0, 1, None, 1, None, None, None) == -1
        assert lib.scot_plan_loss_masked(None, None, None, None, None, None, None, None) == -1
        assert lib.scot_plan_train_step_masked(None, None, None, None, None, None, None, None) == -1
