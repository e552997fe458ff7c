"""scot_error_sums_masked (csrc/error_sums.hip) on the MI355X, inside guard bands: the shapes, the masks and the bit-for-bit oracle
(scot_error_sums on the where-tensor) of tests/error_sums_masked_cases.py, shared with the CPU emulation module, plus the presets'
128 x 128 plane, where every chunk of a channel mask lies inside one plane."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import error_sums_cases as E  # noqa: E402
import error_sums_masked_cases as MC  # noqa: E402
from poseidon_amd import lib as scotlib  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    return E.Ctx(scotlib.load(kind="bf16"), torch.device("cuda"), lambda: torch.cuda.current_stream().cuda_stream, torch.cuda.synchronize)


@pytest.mark.parametrize("case", MC.CASES, ids=lambda c: c[0])
def test_sums_and_overwrite_equal_the_where_tensor_bit_for_bit(ctx, case):
    _, B, C, HW, slices, _, _ = case
    MC.check_shape(ctx, B, C, HW, slices)


def test_operands_off_the_16_byte_boundary_take_the_scalar_path(ctx):
    MC.check_operand_alignment(ctx)


def test_nonfinite_values_under_the_mask(ctx):
    MC.check_nonfinite(ctx)


def test_refusals_leave_sums_and_pred_untouched(ctx):
    MC.check_refusals(ctx)


def test_the_binary16_build_gives_the_same_bits(ctx):
    B, C, HW, slices = 2, 4, 256, E.PINS_SLICES
    pr, tg = E.make_inputs(B, C, HW)
    other = E.Ctx(scotlib.load(kind="f16"), ctx.device, ctx.stream, ctx.sync)
    for label in ("channel_per_sample", "element_30"):
        mask = MC.make_mask(label, B, C, HW)
        a, b = MC.MaskedLaunch(ctx, pr, tg, slices, mask), MC.MaskedLaunch(other, pr, tg, slices, mask)
        assert a.call_masked(1) == 0 and b.call_masked(1) == 0
        assert torch.equal(MC.bits(a.result()), MC.bits(b.result())) and torch.equal(a.pred_bits(), b.pred_bits())


def test_metrics_error_sums_with_a_pixel_mask_runs_the_kernel(ctx):
    """scOT.metrics.error_sums(..., pixel_mask=) on GPU tensors: the masked kernel with overwrite = 0 — error_sums of the where-tensor,
    bit for bit, and the predictions are not modified"""
    from scOT import metrics as M
    B, C, H, slices = 3, 4, 24, [0, 1, 3, 4]
    pr, tg = E.make_inputs(B, C, H * H)
    pr, tg = pr.view(B, C, H, H).to(ctx.device), tg.view(B, C, H, H).to(ctx.device)
    chan = MC.make_mask("channel_per_sample", B, C, H * H).to(ctx.device)
    elem = MC.make_mask("element_30", B, C, H * H).view(B, C, H, H).to(ctx.device)
    for mask, full in ((chan, chan[:, :, None, None].expand(B, C, H, H)), (elem, elem), (elem[:, :1], elem[:, :1].expand(B, C, H, H))):
        before = pr.clone()
        got = M.error_sums(pr, tg, slices, pixel_mask=mask)
        want = M.error_sums(torch.where(full, tg, pr), tg, slices)
        assert got.is_cuda and torch.equal(got.view(torch.int64), want.view(torch.int64)) and torch.equal(pr, before)
