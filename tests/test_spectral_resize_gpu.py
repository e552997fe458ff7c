"""scot_spectral_resize (csrc/spectral_resize.hip) on the MI355X, inside NaN guard bands: the case lists, the fp64 reference and the
derived bound of tests/spectral_resize_cases.py (shared with the CPU emulation module), plus the presets' 256 <-> 128 planes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import spectral_resize_cases as R  # noqa: E402
from poseidon_amd import lib as scotlib, plan as plan_mod  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    return R.Ctx(plan_mod.bind(scotlib.load(kind="bf16")), scotlib.load(kind="f16"), torch.device("cuda"),
                 lambda: torch.cuda.current_stream().cuda_stream, torch.cuda.synchronize)


@pytest.mark.parametrize("nimg", [1, 3])
@pytest.mark.parametrize("s,t", R.K1_SHAPES)
def test_k1_random_operands_within_the_fp64_bound(ctx, s, t, nimg):
    R.check_bound(ctx, nimg, s, t)


def test_k1_the_padded_contraction_supplies_zeros_at_s_33_to_63(ctx):
    R.check_bound(ctx, 2, 40, 35)


@pytest.mark.parametrize("s,t", R.K2_SHAPES)
def test_k2_real_operators_against_the_fft_reference(ctx, s, t):
    R.check_real_operators(s, t, ctx.device)


def test_k3_bits_repeat_and_do_not_depend_on_the_batch_or_the_build(ctx):
    R.check_bits(ctx)
    R.check_bits(ctx, s=16, t=32)
    R.check_bits(ctx, s=17, t=33)


def test_k4_nonfinite_values_stay_in_their_plane(ctx):
    R.check_nonfinite(ctx)
    R.check_nonfinite(ctx, s=17, t=18)


def test_k5_refusals_leave_y_untouched(ctx):
    R.check_refusals(ctx)


@pytest.mark.parametrize("s,t", R.K6_SHAPES)
def test_k6_preset_planes_within_the_fp64_bound(ctx, s, t):
    R.check_bound(ctx, 8, s, t)


def test_k6_the_largest_size_needs_more_than_64_kb_of_lds(ctx):
    """s = 512: 129 KB of dynamic LDS, the one size class behind the function attribute; one plane, ragged t"""
    R.check_bound(ctx, 1, 512, 40)


def test_k7_header_and_prototypes_declare_the_call(ctx):
    R.check_declared(ctx.lib)
    listed = set(plan_mod.runtime_entry_points(ctx.lib)) & set(plan_mod.runtime_entry_points(ctx.lib, adjoint=True))
    assert "scot_spectral_resize" in listed
