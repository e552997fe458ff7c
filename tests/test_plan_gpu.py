"""Exported inference plans on the MI355X: `ScOT.export_plan` records the inference forward, the plan runtime of the library
(csrc/plan.hip, include/scot_plan.h) owns the memory and replays it — from Python through ctypes here, and from a plain C program
(examples/plan_host.c) run as a child process.  Everything is compared bit for bit with `model(...)`.

The caller's buffers (pixel_values, time, prediction) lie in NaN guard bands (tests/kernel_checks.py): the runtime's copies must stay
inside the extents the plan describes."""
import ctypes
import os
import subprocess

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_checks as kc  # noqa: E402
from conftest import ROOT  # noqa: E402
from poseidon_amd import build as scot_build, harness, lib as scot_lib, plan as plan_mod  # noqa: E402
from poseidon_amd.config import ScOTConfig  # noqa: E402
from poseidon_amd.geometry import param_shapes  # noqa: E402
from poseidon_amd.plan import Plan, PlanExportError  # noqa: E402
from poseidon_amd.synth import synth_inputs, synth_state_dict  # noqa: E402
from scOT.model import ScOT  # noqa: E402
from test_model_gpu import DEV, _preset_model  # noqa: E402

_cache = {}


def exported(name, tmp_path_factory):
    """one export per configuration for the whole module -> (model, pixel_values, time, path)"""
    if name not in _cache:
        if name == "small":      # the small fp32 model of tests/test_tape_schedule_gpu.py
            cfg = ScOTConfig(image_size=32, patch_size=4, num_channels=4, num_out_channels=4, embed_dim=16, depths=[2, 2], num_heads=[1, 2],
                             skip_connections=[1, 0], window_size=4, mlp_ratio=4.0, p=1, channel_slice_list_normalized_loss=[0, 1, 3, 4],
                             drop_path_rate=0.0, use_conditioning=True)
            model = ScOT(cfg, compute="fp32")
            model.load_state_dict(synth_state_dict(param_shapes(cfg), "trained"))
            model = model.to(DEV)
            pv, t, _ = synth_inputs(2, 4, 4, 32, "smooth")
        elif name == "roll":      # more input than output channels
            cfg = ScOTConfig(image_size=32, patch_size=4, num_channels=5, num_out_channels=3, embed_dim=16, depths=[2, 2], num_heads=[1, 2],
                             skip_connections=[1, 0], window_size=4, mlp_ratio=4.0, p=1, channel_slice_list_normalized_loss=[0, 1, 3],
                             drop_path_rate=0.0, use_conditioning=True)
            model = ScOT(cfg, compute="fp32")
            model.load_state_dict(synth_state_dict(param_shapes(cfg), "trained"))
            model = model.to(DEV)
            pv, t, _ = synth_inputs(2, 5, 3, 32, "smooth")
        else:                     # Poseidon-T, fp16, the fused layer tails switched on as tests/test_tape_schedule_gpu.py does
            _, _, model = _preset_model("T", 128, 4, "fp16", engine_options={"fused_min_rows": 0})
            pv, t, _ = synth_inputs(2, 4, 4, 128, "smooth")
        model.eval()
        pv, t = pv.to(DEV), t.to(DEV)
        path = str(tmp_path_factory.mktemp("plan") / f"{name}.plan")
        model.export_plan(pv, time=t, path=path)
        _cache[name] = (model, pv, t, path)
    return _cache[name]


def own(model, pv, t):
    with torch.no_grad():
        return model(pixel_values=pv, time=t).output.clone()


@pytest.mark.parametrize("name", ["small", "T"])
def test_plan_round_trip_is_bit_identical(tmp_path_factory, name):
    model, pv, t, path = exported(name, tmp_path_factory)
    B, Cout = pv.shape[0], model.config.num_out_channels
    plan = Plan.load(path)
    d = plan.describe()
    assert d["operand_format"] == (1 if name == "T" else 0) and d["has_time"] == 1 and d["calls"] > 20
    pv2, t2 = pv.flip(0).flip(3) * 0.5 + 0.05, t * 0.37 + 0.05
    ref1, ref2 = own(model, pv, t), own(model, pv2, t2)
    assert torch.isfinite(ref1).all() and torch.isfinite(ref2).all() and not torch.equal(ref1, ref2)
    plan.poison(0xFF)
    for x, tt, ref in ((pv, t, ref1), (pv2, t2, ref2), (pv, t, ref1)):
        gx, g_in = kc.guarded(tuple(x.shape), torch.float32, DEV, src=x, name="pixel_values")
        gt, g_t = kc.guarded((B,), torch.float32, DEV, src=tt, name="time")
        out, g_out = kc.guarded((B, Cout, *x.shape[2:]), torch.float32, DEV, name="prediction")
        plan.run(gx, gt, out=out)
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
        kc.check_all([g_in, g_t, g_out])
        assert torch.equal(gx, x) and torch.equal(gt, tt)
    plan.free()


def test_pixel_mask_is_not_an_inference_input():
    """A per-pixel pixel_mask overwrites the prediction with LABEL values (reference model.py:1411-1484): without labels the model's
    own forward refuses it, and a plan takes no labels — so the export refuses it by name and a plan never has a mask input."""
    cfg = ScOTConfig(image_size=32, patch_size=4, num_channels=4, num_out_channels=4, embed_dim=16, depths=[2, 2], num_heads=[1, 2],
                     skip_connections=[1, 0], window_size=4, mlp_ratio=4.0, p=1, channel_slice_list_normalized_loss=[0, 1, 3, 4],
                     drop_path_rate=0.0, use_conditioning=True)
    model = ScOT(cfg, compute="fp32").to(DEV).eval()
    pv, t, _ = synth_inputs(2, 4, 4, 32, "smooth")
    mask = torch.zeros(2, 4, 32, 32, dtype=torch.bool, device=DEV)
    mask[:, :, 8:16, 8:16] = True
    with torch.no_grad(), pytest.raises(ValueError, match="pixel_mask needs labels"):
        model(pixel_values=pv.to(DEV), time=t.to(DEV), pixel_mask=mask)
    with pytest.raises(PlanExportError, match="pixel_mask"):
        model.export_plan(pv.to(DEV), time=t.to(DEV), pixel_mask=mask)


def test_plan_runs_without_python(tmp_path_factory, tmp_path):
    """examples/plan_host.c, built with hipcc, run as a fresh child process on the exported Poseidon-T plan and raw inputs: its output
    file equals the Python prediction byte for byte."""
    model, pv, t, path = exported("T", tmp_path_factory)
    exe = str(tmp_path / "plan_host")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(scot_build.HIPCC)))
    cc = subprocess.run([scot_build.HIPCC, "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                         os.path.join(ROOT, "examples", "plan_host.c"), "-o", exe, "-ldl"], capture_output=True, text=True, timeout=120)
    assert cc.returncode == 0, cc.stderr[-3000:]
    raw_in, raw_out = tmp_path / "input.bin", tmp_path / "prediction.bin"
    raw_in.write_bytes(pv.cpu().numpy().tobytes() + t.cpu().numpy().tobytes())
    ref = own(model, pv, t)
    torch.cuda.synchronize()
    run = subprocess.run(["timeout", "-k", "10", "60", exe, scot_lib.LIB_PATHS["f16"], path, str(raw_in), str(raw_out)],
                         capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-1000:], run.stderr[-3000:])
    assert "recorded calls" in run.stdout
    assert raw_out.read_bytes() == ref.cpu().numpy().tobytes()


def test_plan_rollout_matches_harness(tmp_path_factory):
    model, pv, t, path = exported("roll", tmp_path_factory)
    with torch.no_grad():
        ref = harness.rollout(model, dict(pixel_values=pv, time=t), ar_steps=3, output_all_steps=True).output
    plan = Plan.load(path)
    plan.poison(0xFF)
    gx, g_in = kc.guarded(tuple(pv.shape), torch.float32, DEV, src=pv, name="pixel_values")
    out, g_out = kc.guarded((3, 2, 3, 32, 32), torch.float32, DEV, name="predictions")
    got = plan.rollout(gx, t, 3, out=out)
    torch.cuda.synchronize()
    print("steps equal:", [bool(torch.equal(got[:, k], ref[:, k])) for k in range(3)])
    assert got.shape == ref.shape == (2, 3, 3, 32, 32) and torch.equal(got, ref)
    kc.check_all([g_in, g_out])
    assert torch.equal(gx, pv)      # the caller's input is not the buffer the predictions are fed back into
    plan.free()


def test_binary16_plan_is_refused_by_the_bfloat16_build(tmp_path_factory):
    model, pv, t, path = exported("T", tmp_path_factory)
    image = open(path, "rb").read()
    assert Plan.header(image)[plan_mod.H_OPERAND] == 1
    bf16 = plan_mod.bind(scot_lib.load(kind="bf16"))
    handle = ctypes.c_void_p()
    assert plan_mod.load_raw(bf16, image, handle, torch.cuda.current_stream().cuda_stream) == -3 and not handle.value
    assert bf16.scot_plan_run(handle, pv.data_ptr(), t.data_ptr(), None, pv.data_ptr(), None) == -1
