"""Exported plans at a foreign resolution (`export_plan(..., resize=True)`) on the CPU emulation: the exporter, the plan runtime and
scot_spectral_resize of libscot_emu.so against the Python model with `fused_resize = True`, bit for bit; the cases are
tests/plan_resize_cases.py's (shared with the GPU module)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import plan_resize_cases as PR  # noqa: E402
from plan_support import check_images_stand_alone, emulated, synth_model  # noqa: E402
from poseidon_amd.config import ScOTConfig  # noqa: E402


@pytest.fixture()
def env(monkeypatch):
    import emu_session
    lib = emulated(monkeypatch)

    def build(name):
        kw, compute, _ = PR.MODELS[name]
        return synth_model(ScOTConfig(**kw), compute)
    return PR.Env(torch.device("cpu"), build, lib, lambda model: emu_session.fused_adamw(model, lr=1e-3))


@pytest.mark.parametrize("r", [16, 48, 20])
def test_d1_run_is_the_fused_model_bit_for_bit(env, r):
    PR.check_run(env, r)


def test_d2_rollout_evaluate_and_masked_evaluate_at_r_24(env):
    PR.check_rollout_and_evaluate(env)


def test_d3_vjp_and_rollout_vjp_are_autograd_through_the_fused_model(env):
    PR.check_adjoint(env)


def test_d3_forward_with_grad_returns_the_input_resolution(env):
    """ScOT.forward under autograd, a resized input, no labels and no mask: the prediction goes back to the input's size (reference
    model.py:1416-1420), with either resize path"""
    for fused in (False, True):
        model = env.model("small", frozen=True)
        model.fused_resize = fused
        pv, t, _ = env.inputs("small", 48)
        out = model(pv.clone().requires_grad_(True), time=t).output
        assert tuple(out.shape) == (2, 4, 48, 48) and out.requires_grad
        with torch.no_grad():
            assert torch.equal(out.detach(), model(pv, time=t).output)


def test_d4_two_stream_plan_gives_the_one_stream_bits(env):
    PR.check_two_streams(env)


def test_d5_refusals_and_the_stand_alone_validator(env, tmp_path):
    image = PR.check_refusals(env)
    check_images_stand_alone(tmp_path, {"good": (image, 0), **PR.corrupt_images(image)})
