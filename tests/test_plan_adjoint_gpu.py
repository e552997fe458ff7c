"""Adjoint plans on the MI355X: `ScOT.export_plan(..., adjoint=("pixel_values", "time"))` records the differentiable forward and the
frozen-model backward; the plan runtime (csrc/plan.hip, include/scot_plan.h) replays them — from Python through ctypes here, and from
a plain C program (examples/plan_adjoint_host.c) run as a child process.  The reference is the Python engine through the public API
(every parameter frozen, `model.eval()`, `torch.autograd.grad(out.output, (pixel_values, time), grad_outputs=g)`); every comparison
is bit for bit.

The caller's five buffers (pixel_values, time, prediction, cotangent, the two gradients) lie in NaN guard bands (tests/kernel_checks.py):
the runtime's copies must stay inside the extents the plan describes."""
import os
import subprocess

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_checks as kc  # noqa: E402
from conftest import ROOT  # noqa: E402
from poseidon_amd import build as scot_build, lib as scot_lib  # noqa: E402
from poseidon_amd.config import ScOTConfig  # noqa: E402
from poseidon_amd.geometry import param_shapes  # noqa: E402
from poseidon_amd.plan import Plan  # noqa: E402
from poseidon_amd.synth import synth_inputs, synth_state_dict  # noqa: E402
from scOT.model import ScOT  # noqa: E402
from test_model_gpu import DEV, _preset_model  # noqa: E402

BOTH = ("pixel_values", "time")
_cache = {}


def exported(name, tmp_path_factory):
    """one adjoint export per configuration for the whole module -> (model, pixel_values, time, path)"""
    if name not in _cache:
        if name == "small":      # the small fp32 model of tests/test_plan_gpu.py
            cfg = ScOTConfig(image_size=32, patch_size=4, num_channels=4, num_out_channels=4, embed_dim=16, depths=[2, 2], num_heads=[1, 2],
                             skip_connections=[1, 0], window_size=4, mlp_ratio=4.0, p=1, channel_slice_list_normalized_loss=[0, 1, 3, 4],
                             drop_path_rate=0.0, use_conditioning=True)
            model = ScOT(cfg, compute="fp32")
            model.load_state_dict(synth_state_dict(param_shapes(cfg), "trained"))
            model = model.to(DEV)
            pv, t, _ = synth_inputs(2, 4, 4, 32, "smooth")
        else:                    # Poseidon-T, fp16, batch 2, the fused layer tails switched on: the configuration tests/test_plan_gpu.py exports
            _, _, model = _preset_model("T", 128, 4, "fp16", engine_options={"fused_min_rows": 0})
            pv, t, _ = synth_inputs(2, 4, 4, 128, "smooth")
        model.eval()
        for p in model.parameters():
            p.requires_grad_(False)
        pv, t = pv.to(DEV), t.to(DEV)
        path = str(tmp_path_factory.mktemp("plan") / f"{name}_adjoint.plan")
        model.export_plan(pv, time=t, path=path, adjoint=BOTH)
        _cache[name] = (model, pv, t, path)
    return _cache[name]


def cotangent(pred_shape, seed):
    n = 1
    for s in pred_shape:
        n *= s
    return (torch.randn(pred_shape, generator=torch.Generator().manual_seed(seed)) / n).to(DEV)


def python_side(model, pv, t, g):
    a, b = pv.clone().requires_grad_(True), t.clone().requires_grad_(True)
    out = model(pixel_values=a, time=b).output
    d_pv, d_t = torch.autograd.grad(out, (a, b), grad_outputs=g)
    return out.detach().clone(), d_pv.clone(), d_t.clone()


@pytest.mark.parametrize("name", ["small", "T"])
def test_adjoint_round_trip_is_bit_identical(tmp_path_factory, name):
    model, pv, t, path = exported(name, tmp_path_factory)
    B, Cout = pv.shape[0], model.config.num_out_channels
    plan = Plan.load(path)
    d, a = plan.describe(), plan.describe_adjoint()
    print(f"\n[{name}] device_bytes {d['device_bytes']} kept_bytes {a['kept_bytes']} calls {d['calls']} + {a['backward_calls']}")
    assert d["format"] == 2 and a["has_adjoint"] == a["d_pixel_values"] == a["d_time"] == 1 and a["backward_calls"] > 20
    S = model._engine.grad_scale_value()
    assert 2.0 ** a["grad_scale_exponent"] == S and (S > 1.0) == (name == "T")
    pv2, t2 = pv.flip(0).flip(3) * 0.5 + 0.05, t * 0.37 + 0.05
    shape = (B, Cout, *pv.shape[2:])
    g1, g2 = cotangent(shape, 3), cotangent(shape, 4)
    ref1, ref2 = python_side(model, pv, t, g1), python_side(model, pv2, t2, g2)
    assert all(torch.isfinite(r).all() for r in ref1 + ref2) and not torch.equal(ref1[1], ref2[1]) and float(ref1[2].abs().max()) > 0.0
    if name == "T":
        assert int(model._engine.grad_overflow) == 0
    for x, tt, g, ref in ((pv, t, g1, ref1), (pv2, t2, g2, ref2), (pv, t, g1, ref1)):
        plan.poison(0xFF)
        gx, g_in = kc.guarded(tuple(x.shape), torch.float32, DEV, src=x, name="pixel_values")
        gt, g_t = kc.guarded((B,), torch.float32, DEV, src=tt, name="time")
        out, g_out = kc.guarded(shape, torch.float32, DEV, name="prediction")
        gg, g_cot = kc.guarded(shape, torch.float32, DEV, src=g, name="d_prediction")
        d_pv, g_dpv = kc.guarded(tuple(x.shape), torch.float32, DEV, name="d_pixel_values")
        d_t, g_dt = kc.guarded((B,), torch.float32, DEV, name="d_time")
        plan.run(gx, gt, out=out)
        plan.vjp(gg, grad_scale=S if name == "T" else 0, out=(d_pv, d_t))
        torch.cuda.synchronize()
        assert torch.equal(out, ref[0])
        assert torch.equal(d_pv, ref[1])
        assert torch.equal(d_t, ref[2])
        kc.check_all([g_in, g_t, g_out, g_cot, g_dpv, g_dt])
        assert torch.equal(gx, x) and torch.equal(gt, tt) and torch.equal(gg, g)
    assert plan.grad_status() == (0, a["grad_scale_exponent"])
    # one vjp per run; a format-1 call sequence still works on the same plan (run alone)
    assert plan._lib.scot_plan_vjp(plan._h, g1.data_ptr(), None, None, 0.0, torch.cuda.current_stream().cuda_stream) == -1
    assert torch.equal(plan.run(pv, t), ref1[0])
    plan.free()


def test_adjoint_plan_runs_without_python(tmp_path_factory, tmp_path):
    """examples/plan_adjoint_host.c, built with hipcc, run once as a fresh child process on the exported Poseidon-T adjoint plan and raw
    inputs: its three output files equal Python's bytes."""
    model, pv, t, path = exported("T", tmp_path_factory)
    exe = str(tmp_path / "plan_adjoint_host")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(scot_build.HIPCC)))
    cc = subprocess.run([scot_build.HIPCC, "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                         os.path.join(ROOT, "examples", "plan_adjoint_host.c"), "-o", exe, "-ldl"], capture_output=True, text=True, timeout=120)
    assert cc.returncode == 0, cc.stderr[-3000:]
    g = cotangent((pv.shape[0], model.config.num_out_channels, *pv.shape[2:]), 5)
    files = {k: tmp_path / f"{k}.bin" for k in ("input", "cotangent", "prediction", "d_pixel_values", "d_time")}
    files["input"].write_bytes(pv.cpu().numpy().tobytes() + t.cpu().numpy().tobytes())
    files["cotangent"].write_bytes(g.cpu().numpy().tobytes())
    ref = python_side(model, pv, t, g)
    torch.cuda.synchronize()
    run = subprocess.run(["timeout", "-k", "10", "60", exe, scot_lib.LIB_PATHS["f16"], path] + [str(files[k]) for k in files],
                         capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-1000:], run.stderr[-3000:])
    assert "grad_status: 0 non-finite values counted" in run.stdout and "recorded calls" in run.stdout
    for k, r in zip(("prediction", "d_pixel_values", "d_time"), ref):
        assert files[k].read_bytes() == r.cpu().numpy().tobytes(), k
