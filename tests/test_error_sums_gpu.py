"""scot_error_sums (csrc/error_sums.hip) on the MI355X, inside NaN guard bands: the case list, the fp64 reference and the derived bound of
tests/error_sums_cases.py (shared with the CPU emulation module), plus the presets' 128 x 128 plane."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import error_sums_cases as E  # noqa: E402
from poseidon_amd import lib as scotlib  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    return E.Ctx(scotlib.load(kind="bf16"), torch.device("cuda"), lambda: torch.cuda.current_stream().cuda_stream, torch.cuda.synchronize)


def test_chunk_constant(ctx):
    E.check_chunk_constant(ctx)


@pytest.mark.parametrize("case", E.CASES, ids=lambda c: c[0])
def test_case_within_the_fp64_bound(ctx, case):
    _, B, C, HW, slices, nan_channels, _ = case
    E.check_case(ctx, B, C, HW, slices, nan_channels)


def test_both_builds_and_both_load_paths_give_the_same_bits(ctx):
    """the binary16 build runs the same kernel; a lane owns the same floats whether it loads them as vectors or scalars"""
    B, C, HW = 2, 4, 256
    pr, tg = E.make_inputs(B, C, HW)
    aligned = E.Launch(ctx, pr, tg, E.PINS_SLICES)
    assert aligned.call() == 0
    want = aligned.result()
    other = E.Launch(E.Ctx(scotlib.load(kind="f16"), ctx.device, ctx.stream, ctx.sync), pr, tg, E.PINS_SLICES)
    assert other.call() == 0 and torch.equal(other.result().view(torch.int64), want.view(torch.int64))
    shifted = E.Launch(ctx, pr, tg, E.PINS_SLICES)
    flat = torch.empty(B * C * HW + 64, device=ctx.device)
    flat[1:1 + B * C * HW] = pr.reshape(-1).to(ctx.device)
    shifted.pred = flat[1:1 + B * C * HW].view(B, C, HW)      # 4 bytes off the 16-byte boundary: every run takes the scalar path
    assert shifted.pred.data_ptr() % 16 == 4 and shifted.call() == 0
    assert torch.equal(shifted.result().view(torch.int64), want.view(torch.int64))


def test_nonfinite_values_go_through(ctx):
    E.check_nonfinite(ctx)


def test_refusals_leave_sums_untouched(ctx):
    E.check_refusals(ctx)


def test_from_sums_helpers_reproduce_the_reference_pins_from_the_kernel(ctx):
    """scOT.metrics.error_sums on GPU tensors (the kernel) -> the pins of the real reference's metrics module; the result stays on the device"""
    from scOT import metrics as M

    def on_gpu(pr, tg, slices):
        out = M.error_sums(torch.from_numpy(pr).to(ctx.device), torch.from_numpy(tg).to(ctx.device), slices)
        assert out.is_cuda and out.dtype == torch.float64
        return out
    E.check_pins(on_gpu)
