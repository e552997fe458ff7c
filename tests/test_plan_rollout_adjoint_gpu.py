"""The adjoint of an exported model's rollout on the MI355X: scot_plan_rollout_vjp (csrc/plan.hip, include/scot_plan.h) — from Python
through ctypes here, and from a plain C program (examples/plan_rollout_adjoint_host.c) run as a child process.

The reference is the Python engine, never the plan (tests/plan_rollout_reference.py): R1, the explicit chain of single-step
`torch.autograd.grad` calls summed in the contract's order, bit for bit; R2, `torch.autograd.grad` through
`harness.rollout(..., output_all_steps=True, detach=False)`, bit for bit on the first Cout channels and within the association bound
of an n-term fp32 sum on the pass-through channels and on d_time.

The caller's six buffers (pixel_values, time, predictions, d_predictions, d_pixel_values, d_time) lie in NaN guard bands
(tests/kernel_checks.py), and the plan's scratch is filled with NaN bytes before each call."""
import os
import subprocess

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_checks as kc  # noqa: E402
import plan_rollout_reference as ref_mod  # noqa: E402
from conftest import ROOT  # noqa: E402
from poseidon_amd import build as scot_build, lib as scot_lib  # noqa: E402
from poseidon_amd.config import ScOTConfig  # noqa: E402
from poseidon_amd.geometry import param_shapes  # noqa: E402
from poseidon_amd.plan import Plan  # noqa: E402
from poseidon_amd.synth import synth_inputs, synth_state_dict  # noqa: E402
from scOT.model import ScOT  # noqa: E402
from test_model_gpu import DEV, _preset_model  # noqa: E402

BOTH = ("pixel_values", "time")
SMALL = dict(image_size=32, patch_size=4, num_channels=4, num_out_channels=4, embed_dim=16, depths=[2, 2], num_heads=[1, 2],
             skip_connections=[1, 0], window_size=4, mlp_ratio=4.0, p=1, channel_slice_list_normalized_loss=[0, 1, 3, 4],
             drop_path_rate=0.0, use_conditioning=True)
RESID = dict(SMALL, num_channels=5, num_out_channels=3, channel_slice_list_normalized_loss=[0, 1, 3], learn_residual=True)
STEPS = {"small": 3, "resid": 3, "T": 2}
_cache = {}


def exported(name, tmp_path_factory):
    """one adjoint export and one pair of references per configuration for the whole module"""
    if name not in _cache:
        if name == "T":      # Poseidon-T, fp16, batch 2, the fused layer tails switched on
            _, _, model = _preset_model("T", 128, 4, "fp16", engine_options={"fused_min_rows": 0})
            pv, t, _ = synth_inputs(2, 4, 4, 128, "smooth")
        else:
            cfg = ScOTConfig(**(SMALL if name == "small" else RESID))
            model = ScOT(cfg, compute="fp32")
            model.load_state_dict(synth_state_dict(param_shapes(cfg), "trained"))
            model = model.to(DEV)
            pv, t, _ = synth_inputs(2, cfg.num_channels, cfg.num_out_channels, 32, "smooth")
        model.eval()
        for p in model.parameters():
            p.requires_grad_(False)
        pv, t = pv.to(DEV), t.to(DEV)
        path = str(tmp_path_factory.mktemp("plan") / f"{name}_adjoint.plan")
        model.export_plan(pv, time=t, path=path, adjoint=BOTH)
        steps, cout = STEPS[name], model.config.num_out_channels
        shape = (pv.shape[0], steps, cout, *pv.shape[2:])
        g = (torch.randn(shape, generator=torch.Generator().manual_seed(11)) / (shape[0] * cout * shape[3] * shape[4])).to(DEV)
        preds, d_pv2, d_t2 = ref_mod.r2(model, pv, t, g)
        d_pv1, d_t1, terms = ref_mod.r1(model, pv, t, preds, g)
        torch.cuda.synchronize()
        _cache[name] = dict(model=model, pv=pv, t=t, path=path, g=g, preds=preds, r1=(d_pv1, d_t1), r2=(d_pv2, d_t2), terms=terms)
    return _cache[name]


@pytest.mark.parametrize("name", ["small", "resid", "T"])
def test_rollout_vjp_equals_the_python_chain(tmp_path_factory, name):
    c = exported(name, tmp_path_factory)
    model, pv, t, g, steps = c["model"], c["pv"], c["t"], c["g"], STEPS[name]
    B, cout = pv.shape[0], model.config.num_out_channels
    assert all(torch.isfinite(x).all() for x in c["r1"] + c["r2"]) and float(c["r1"][1].abs().max()) > 0.0
    if name == "T":
        assert int(model._engine.grad_overflow) == 0
    ref_mod.assert_r2_within_bound(c["r1"], c["r2"], c["terms"], cout, label=f"{name} x{steps}")
    plan = Plan.load(c["path"])
    a = plan.describe_adjoint()
    stream = torch.cuda.current_stream().cuda_stream
    shape = (steps, B, cout, *pv.shape[2:])      # the C layout
    gx, g_in = kc.guarded(tuple(pv.shape), torch.float32, DEV, src=pv, name="pixel_values")
    gt, g_t = kc.guarded((B,), torch.float32, DEV, src=t, name="time")
    preds, g_preds = kc.guarded(shape, torch.float32, DEV, name="predictions")
    gg, g_cot = kc.guarded(shape, torch.float32, DEV, src=g.transpose(0, 1), name="d_predictions")
    d_pv, g_dpv = kc.guarded(tuple(pv.shape), torch.float32, DEV, name="d_pixel_values")
    d_t, g_dt = kc.guarded((B,), torch.float32, DEV, name="d_time")
    plan.poison(0xFF)
    plan.rollout(gx.data_ptr(), gt.data_ptr(), steps, out=preds.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert torch.equal(preds.transpose(0, 1), c["preds"])
    kept = preds.clone()
    plan.poison(0xFF)
    plan.rollout_vjp(gx.data_ptr(), gt.data_ptr(), preds.data_ptr(), gg.data_ptr(), out=(d_pv, d_t), steps=steps, stream=stream)
    torch.cuda.synchronize()
    assert torch.equal(d_pv, c["r1"][0])
    assert torch.equal(d_t, c["r1"][1])
    kc.check_all([g_in, g_t, g_preds, g_cot, g_dpv, g_dt])
    assert torch.equal(gx, pv) and torch.equal(gt, t) and torch.equal(gg, g.transpose(0, 1)) and torch.equal(preds, kept)
    assert plan.grad_status() == (0, a["grad_scale_exponent"])
    # it leaves the plan un-armed
    assert plan._lib.scot_plan_vjp(plan._h, gg.data_ptr(), None, None, 0.0, stream) == -1
    if name == "small":
        # buffers that are not 16-byte aligned take the carry's scalar form: the same bits, and nothing outside the extents
        n_pv, n_g = pv.numel(), g.numel()
        off_g, g_og = kc.guarded((n_g + 1,), torch.float32, DEV, band=4096, name="d_predictions + 4 bytes")
        off_d, g_od = kc.guarded((n_pv + 1,), torch.float32, DEV, band=4096, name="d_pixel_values + 4 bytes")
        off_g[1:].copy_(gg.reshape(-1))
        first_g, first_d = off_g[:1].clone(), off_d[:1].clone()
        plan.poison(0xFF)
        plan.rollout_vjp(gx.data_ptr(), gt.data_ptr(), preds.data_ptr(), off_g.data_ptr() + 4, out=(off_d.data_ptr() + 4, d_t.data_ptr()),
                         steps=steps, stream=stream)
        torch.cuda.synchronize()
        assert torch.equal(off_d[1:].view_as(pv), c["r1"][0]) and torch.equal(d_t, c["r1"][1])
        assert torch.equal(off_g[:1].view(torch.int32), first_g.view(torch.int32)) and torch.equal(off_d[:1].view(torch.int32), first_d.view(torch.int32))
        kc.check_all([g_og, g_od, g_dt])
        # the tensor form ([B, steps, Cout, H, W], as Plan.rollout returns it), and the holder of the runtime's own
        got = plan.rollout_vjp(pv, t, c["preds"], g)
        only_t = torch.empty_like(t)
        plan.rollout_vjp(pv, t, c["preds"], g, out=(None, only_t))
        torch.cuda.synchronize()
        assert torch.equal(got[0], c["r1"][0]) and torch.equal(got[1], c["r1"][1]) and torch.equal(only_t, c["r1"][1])
    plan.free()


def test_rollout_adjoint_runs_without_python(tmp_path_factory, tmp_path):
    """examples/plan_rollout_adjoint_host.c, built with hipcc, run once as a fresh child process on the exported Poseidon-T adjoint plan
    and raw inputs: its three output files equal Python's bytes."""
    c = exported("T", tmp_path_factory)
    exe = str(tmp_path / "plan_rollout_adjoint_host")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(scot_build.HIPCC)))
    cc = subprocess.run([scot_build.HIPCC, "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                         os.path.join(ROOT, "examples", "plan_rollout_adjoint_host.c"), "-o", exe, "-ldl"], capture_output=True, text=True,
                        timeout=120)
    assert cc.returncode == 0, cc.stderr[-3000:]
    files = {k: tmp_path / f"{k}.bin" for k in ("input", "cotangents", "predictions", "d_pixel_values", "d_time")}
    files["input"].write_bytes(c["pv"].cpu().numpy().tobytes() + c["t"].cpu().numpy().tobytes())
    files["cotangents"].write_bytes(c["g"].transpose(0, 1).contiguous().cpu().numpy().tobytes())
    torch.cuda.synchronize()
    run = subprocess.run(["timeout", "-k", "10", "60", exe, scot_lib.LIB_PATHS["f16"], c["path"], str(STEPS["T"])] + [str(files[k]) for k in files],
                         capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-1000:], run.stderr[-3000:])
    assert "grad_status: 0 non-finite values counted" in run.stdout and "recorded calls" in run.stdout
    want = (c["preds"].transpose(0, 1).contiguous(), c["r1"][0], c["r1"][1])
    for k, r in zip(("predictions", "d_pixel_values", "d_time"), want):
        assert files[k].read_bytes() == r.cpu().numpy().tobytes(), k
