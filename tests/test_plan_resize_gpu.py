"""Exported plans at a foreign resolution (`export_plan(..., resize=True)`) on the MI355X: the cases of tests/plan_resize_cases.py (shared
with the CPU emulation module) against the Python model with `fused_resize = True`, bit for bit, plus the 96-wide fp16 model at 96 x 96
and the reference's own resize fixtures through the one-launch kernel."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import plan_resize_cases as PR  # noqa: E402
from conftest import load_fixture  # noqa: E402
from poseidon_amd import lib as scotlib  # noqa: E402
from poseidon_amd.config import ScOTConfig  # noqa: E402
from poseidon_amd.geometry import param_shapes  # noqa: E402
from poseidon_amd.plan import Plan  # noqa: E402
from poseidon_amd.synth import synth_state_dict  # noqa: E402
from scOT.model import ScOT  # noqa: E402
from test_model_gpu import DEV, build, inputs, rel_l2  # noqa: E402


def build_model(name):
    kw, compute, _ = PR.MODELS[name]
    cfg = ScOTConfig(**kw)
    model = ScOT(cfg, compute=compute, engine_options={"fused_min_rows": 0} if name == "c96" else None)
    model.load_state_dict(synth_state_dict(param_shapes(cfg), "trained"))
    return model.to(DEV).eval()


@pytest.fixture()
def env():
    from poseidon_amd.optim import FusedAdamW
    return PR.Env(torch.device(DEV), build_model, scotlib.load(kind="bf16"), lambda model: FusedAdamW(model, lr=1e-3),
                  lambda: torch.cuda.current_stream().cuda_stream, torch.cuda.synchronize)


@pytest.mark.parametrize("r", [16, 48, 20])
def test_d1_run_is_the_fused_model_bit_for_bit(env, r):
    PR.check_run(env, r)


def test_d2_rollout_evaluate_and_masked_evaluate_at_r_24(env):
    PR.check_rollout_and_evaluate(env)


def test_d3_vjp_and_rollout_vjp_are_autograd_through_the_fused_model(env):
    PR.check_adjoint(env)


def test_d4_two_stream_plan_gives_the_one_stream_bits(env):
    PR.check_two_streams(env)


def test_d5_refusals(env):
    PR.check_refusals(env)


def test_d6_the_96_wide_fp16_model_at_96(env):
    """WIDE (fp16, image 64, batch 1: fused layer tails, 16 x 16 windows, trunk products in the bfloat16 build) fed 96 x 96"""
    model = env.model("c96")
    pv, t, _ = env.inputs("c96", 96)
    plan = Plan.load(model.export_plan(pv, time=t, resize=True))
    assert plan.describe_resize() == (1, 64, 96, 2) and plan.describe()["operand_format"] == 1
    pv2, t2 = env.other(pv, t)
    for a, b in ((pv, t), (pv2, t2)):
        plan.poison(0xFF)
        got, want = plan.run(a, b), PR.own(model, a, b)
        assert tuple(got.shape) == (1, 4, 96, 96) and torch.isfinite(got).all() and torch.equal(got, want)
    plan.free()


@pytest.mark.parametrize("size", [64, 16])
def test_d6_reference_fixtures_through_the_fused_resize(size):
    """the reference's own outputs for a 32 x 32 model fed 64 x 64 and 16 x 16 (tests/golden), within the bounds of the two-launch path's
    test (tests/test_model_gpu.py::test_spectral_resize_path)"""
    f, meta = load_fixture(f"tiny_resize{size}")
    cfg, model = build(meta, "fp32")
    model.fused_resize = True
    with torch.no_grad():
        out = model(**inputs(cfg, meta))
    e_out, e_loss = rel_l2(out.output.cpu().numpy(), f["output"]), abs(float(out.loss) - float(f["loss"])) / abs(float(f["loss"]))
    print(f"\n[fused resize {size} -> 32] output rel-L2 {e_out:.2e}, loss rel {e_loss:.2e}")
    assert e_out < 2e-5
    assert e_loss < 5e-5
