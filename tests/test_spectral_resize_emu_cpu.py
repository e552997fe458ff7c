"""scot_spectral_resize (csrc/spectral_resize.hip) on the CPU emulation: the kernel source itself runs, one fiber per work-item, inside
NaN guard bands; the case lists, the fp64 reference and the derived bound are tests/spectral_resize_cases.py's (shared with the GPU
module)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
import spectral_resize_cases as R  # noqa: E402
from poseidon_amd import lib as scotlib, plan as plan_mod  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    import emu_session
    return R.Ctx(plan_mod.bind(emu_session.load_emu()), emu_session.load_emu("f16"), torch.device("cpu"))


@pytest.mark.parametrize("nimg", [1, 3])
@pytest.mark.parametrize("s,t", R.K1_SHAPES)
def test_k1_random_operands_within_the_fp64_bound(ctx, s, t, nimg):
    R.check_bound(ctx, nimg, s, t)


def test_k1_the_padded_contraction_supplies_zeros_at_s_33_to_63(ctx):
    """s = 40: the contraction runs to 64 and the second row tile is ragged, with t = 35 over three column tiles"""
    R.check_bound(ctx, 2, 40, 35)


@pytest.mark.parametrize("s,t", R.K2_SHAPES)
def test_k2_real_operators_against_the_fft_reference(ctx, monkeypatch, s, t):
    import emu_session
    import scOT.model as M
    emu_session.patch_ops(monkeypatch, ctx.lib)
    monkeypatch.setattr(M, "_require_hip", lambda t: None)
    R.check_real_operators(s, t, ctx.device)


def test_k3_bits_repeat_and_do_not_depend_on_the_batch_or_the_build(ctx):
    R.check_bits(ctx)
    R.check_bits(ctx, s=16, t=32)      # the vector path of the operator loads (s % 4 == 0 also at s = 20; here whole tiles)
    R.check_bits(ctx, s=17, t=33)      # the scalar path


def test_k4_nonfinite_values_stay_in_their_plane(ctx):
    R.check_nonfinite(ctx)
    R.check_nonfinite(ctx, s=17, t=18)


def test_k5_refusals_leave_y_untouched(ctx):
    R.check_refusals(ctx)


def test_k7_header_and_prototypes_declare_the_call(ctx):
    R.check_declared(ctx.lib)
    for lib in (ctx.lib, ctx.lib_f16):
        listed = set(plan_mod.runtime_entry_points(lib)) & set(plan_mod.runtime_entry_points(lib, adjoint=True))
        assert "scot_spectral_resize" in listed and "scot_spectral_apply" not in listed


def test_k7_gfx950_builds_export_the_call():
    for kind in ("bf16", "f16"):
        lib = scotlib.load(kind=kind)
        assert lib.scot_spectral_resize.argtypes == scotlib.PROTOTYPES["scot_spectral_resize"]
        assert lib.scot_plan_describe_resize.argtypes == scotlib.PLAN_PROTOTYPES["scot_plan_describe_resize"]
        assert lib.scot_abi_version() == 8
        assert lib.scot_spectral_resize(None, None, None, None, 1, 1, 1, None) == -1      # (refused before anything touches a device)
        assert lib.scot_plan_describe_resize(None, None) == -1
