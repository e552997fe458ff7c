"""scot_grad_accumulate (csrc/optim.hip) on the MI355X, inside NaN guard bands: the maps, the forms and the two-rounding expectation of
tests/grad_accumulate_cases.py (shared with the CPU emulation module), plus one 8-float group more than a full sweep of the kernel's grid."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import grad_accumulate_cases as G  # noqa: E402
from poseidon_amd import lib as scotlib  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    return G.Ctx(scotlib.load(kind="bf16"), torch.device("cuda"), lambda: torch.cuda.current_stream().cuda_stream, torch.cuda.synchronize)


@pytest.mark.parametrize("in_place", [True, False], ids=["in_place", "out_of_place"])
@pytest.mark.parametrize("map_kind", G.MAPS)
@pytest.mark.parametrize("n", G.SIZES)
def test_three_adds_are_two_roundings_each(ctx, n, map_kind, in_place):
    G.check_three_adds(ctx, n, map_kind, in_place)


@pytest.mark.parametrize("in_place", [True, False], ids=["in_place", "out_of_place"])
def test_second_trip_of_the_grid(ctx, in_place):
    """the grid-stride loop's second trip: the last group of the arena is the only one a lane reaches there"""
    n = G.full_sweep_plus_one_group(ctx)
    assert 8_000_000 < n < 9_000_000
    G.check_three_adds(ctx, n, "groups", in_place)      # the last group is a parameter
    G.check_three_adds(ctx, n, "edges", in_place)       # ... and is not: nothing may be stored there


@pytest.mark.parametrize("n", G.SIZES)
def test_copy_keeps_every_bit_pattern(ctx, n):
    G.check_copy_keeps_bits(ctx, n)


def test_nonfinite_values_go_through(ctx):
    G.check_nonfinite(ctx)


def test_refusals_leave_dst_untouched(ctx):
    G.check_refusals(ctx)


def test_both_builds_give_the_same_bits(ctx):
    n = 8 * 257
    other = G.Ctx(scotlib.load(kind="f16"), ctx.device, ctx.stream, ctx.sync)
    G.check_three_adds(other, n, "edges", True)
    G.check_copy_keeps_bits(other, n)
