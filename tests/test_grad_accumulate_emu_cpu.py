"""scot_grad_accumulate (csrc/optim.hip) on the CPU emulation: the kernel source itself runs inside NaN guard bands; the maps, the forms and
the two-rounding expectation are tests/grad_accumulate_cases.py's (shared with the GPU module)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
import grad_accumulate_cases as G  # noqa: E402
from poseidon_amd import ops, plan as plan_mod  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    import emu_session
    return G.Ctx(plan_mod.bind(emu_session.load_emu()), torch.device("cpu"))


@pytest.mark.parametrize("in_place", [True, False], ids=["in_place", "out_of_place"])
@pytest.mark.parametrize("map_kind", G.MAPS)
@pytest.mark.parametrize("n", G.SIZES)
def test_three_adds_are_two_roundings_each(ctx, n, map_kind, in_place):
    G.check_three_adds(ctx, n, map_kind, in_place)


@pytest.mark.parametrize("n", G.SIZES)
def test_copy_keeps_every_bit_pattern(ctx, n):
    G.check_copy_keeps_bits(ctx, n)


def test_nonfinite_values_go_through(ctx):
    G.check_nonfinite(ctx)


def test_refusals_leave_dst_untouched(ctx):
    G.check_refusals(ctx)


def test_ops_wrapper(ctx, monkeypatch):
    import emu_session
    emu_session.patch_ops(monkeypatch, ctx.lib)
    n = 8 * 257
    m = G.make_map(n, "edges")
    on = (m != 255).repeat_interleave(8)
    g0, g1 = G.make_grads(n, 2)
    dst = torch.full((n,), 7.0)
    ops.grad_accumulate(dst, None, g0, m, G.WEIGHT)
    ops.grad_accumulate(dst, dst, g1, m, G.WEIGHT)
    assert torch.equal(dst[on], (g0 * G.WEIGHT + g1 * G.WEIGHT)[on]) and bool((dst[~on] == 7.0).all())
    with pytest.raises(Exception, match="scot_grad_accumulate"):
        ops.grad_accumulate(g0, None, g0, m, G.WEIGHT)
