"""scot_plan_evaluate on the MI355X: a forward or a whole rollout of an exported plan that leaves only error sums behind — through ctypes
here, and from a plain C program (examples/plan_eval_host.c) run as a child process.  The caller's buffers lie in NaN guard bands, the
plan's scratch is poisoned before every call, and every comparison with scot_plan_rollout / scot_plan_run / the stand-alone
scot_error_sums is bit for bit (tests/plan_eval_cases.py, shared with the CPU emulation module)."""
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import error_sums_cases as E  # noqa: E402
import plan_eval_cases as PE  # noqa: E402
from conftest import ROOT  # noqa: E402
from plan_support import BOTH, CFG_ROLL, SMALL, WIDE  # noqa: E402
from poseidon_amd import build as scot_build, lib as scot_lib  # noqa: E402
from poseidon_amd.config import ScOTConfig  # noqa: E402
from poseidon_amd.geometry import param_shapes  # noqa: E402
from poseidon_amd.plan import Plan  # noqa: E402
from poseidon_amd.synth import synth_inputs, synth_state_dict  # noqa: E402
from scOT.model import ScOT  # noqa: E402
from test_model_gpu import DEV  # noqa: E402

MODELS = {"roll": (CFG_ROLL, "fp32", 2), "small": (SMALL, "fp32", 2), "wide": (WIDE, "fp16", 1)}
_cache = {}


def build_model(name, train=False):
    kw, compute, _ = MODELS[name]
    cfg = ScOTConfig(**kw)
    model = ScOT(cfg, compute=compute, engine_options={"fused_min_rows": 0} if name == "wide" else None)
    model.load_state_dict(synth_state_dict(param_shapes(cfg), "trained"))
    model = model.to(DEV)
    model.train(train)
    return model


def inputs(name):
    kw, _, B = MODELS[name]
    return tuple(x.to(DEV).contiguous() for x in synth_inputs(B, kw["num_channels"], kw["num_out_channels"], kw["image_size"], "smooth"))


def exported(name, **kw):
    key = (name, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _cache:
        model = build_model(name)
        if "adjoint" in kw:
            for p in model.parameters():
                p.requires_grad_(False)
        pv, t, _ = inputs(name)
        _cache[key] = model.export_plan(pv, time=t, **kw)
        del model
    return _cache[key]


def context(plan):
    return E.Ctx(plan._lib, torch.device(DEV), lambda: torch.cuda.current_stream().cuda_stream, torch.cuda.synchronize)


@pytest.mark.parametrize("name,steps,slices", [("roll", 3, [0, 1, 3]), ("roll", 3, None), ("small", 1, [0, 1, 3, 4]), ("wide", 3, [0, 1, 3, 4]),
                                               ("wide", 1, None)])
def test_evaluate_is_rollout_plus_the_kernel(name, steps, slices):
    pv, t, _ = inputs(name)
    plan = Plan.load(exported(name))
    before = plan.describe()["device_bytes"]
    sums, targets = PE.check_evaluate(plan, context(plan), pv, t, steps, slices)
    assert plan.describe()["device_bytes"] > before
    tg = targets.to(DEV).transpose(0, 1).contiguous()
    got, preds = plan.evaluate(pv, t, tg, steps=steps, channel_slice_list=slices, predictions=True)
    torch.cuda.synchronize()
    assert got.is_cuda and PE.same_bits(got.cpu(), sums)
    ref = plan.rollout(pv, t, steps) if steps > 1 else plan.run(pv, t)[:, None]
    assert PE.same_bits(preds.cpu(), ref.cpu())
    plan.free()


def test_two_stream_plan_gives_the_one_stream_sums():
    pv, t, _ = inputs("roll")
    one, two = Plan.load(exported("roll")), Plan.load(exported("roll", streams=2))
    assert two.describe()["format"] == 5
    a, _ = PE.check_evaluate(one, context(one), pv, t, 3, [0, 1, 3])
    b, _ = PE.check_evaluate(two, context(two), pv, t, 3, [0, 1, 3])
    assert PE.same_bits(a, b)
    one.free()
    two.free()


def test_adjoint_plan_has_nothing_to_differentiate_after_an_evaluate():
    pv, t, _ = inputs("roll")
    plan = Plan.load(exported("roll", adjoint=BOTH))
    ctx = context(plan)
    g = torch.ones(2, 3, 16, 16, device=DEV)
    d_pv, d_t = torch.zeros_like(pv), torch.zeros_like(t)

    def vjp():
        rc = plan._lib.scot_plan_vjp(plan._h, g.data_ptr(), d_pv.data_ptr(), d_t.data_ptr(), 0.0, ctx.stream())
        torch.cuda.synchronize()
        return rc
    plan.run(pv, t)
    for steps in (1, 3):
        rc, sums, _ = PE.evaluate(plan, ctx, pv, t, torch.zeros(steps, 2, 3, 16, 16), steps, None, False)
        assert rc == 0 and torch.isfinite(sums).all()
        assert vjp() == -1
        plan.run(pv, t)
        assert vjp() == 0 and torch.isfinite(d_pv).all() and float(d_pv.abs().max()) > 0
        plan.run(pv, t)
    plan.free()


def test_training_plan_validates_at_the_current_weights():
    """the step forward's prediction is deterministic on the GPU (tests/test_plan_train_gpu.py compares it bit for bit): evaluate gives
    the error sums of exactly that prediction, before and after a step, and changes no state"""
    from scOT.trainer import FusedAdamW
    model = build_model("small", train=True)
    opt = FusedAdamW(model, lr=5e-5, weight_decay=0.01, max_grad_norm=5.0)
    pv, t, y = inputs("small")
    image = model.export_plan(pv, time=t, labels=y, train=opt)
    plan = Plan.load(image)
    ctx = context(plan)
    slices, seen = [0, 1, 3, 4], []
    for step in range(2):
        snap = plan.snapshot(image)
        _, pred = plan.loss(pv, t, y)
        torch.cuda.synchronize()
        rc, sums, got = PE.evaluate(plan, ctx, pv, t, y[None].contiguous(), 1, slices, True)
        assert rc == 0 and PE.same_bits(got[0], pred.cpu())
        alone = E.Launch(ctx, pred.reshape(2, 4, -1).cpu(), y.reshape(2, 4, -1).cpu(), slices)
        assert alone.call() == 0 and PE.same_bits(sums[0], alone.result())
        assert plan.snapshot(image) == snap
        seen.append(sums)
        if step == 0:
            plan.train_step(pv, t, y, 5e-5)
    assert not PE.same_bits(seen[0], seen[1])
    plan.free()


def test_refusals():
    """the refusals a plan with a time input and Cout <= Cin can show.  Cout > Cin with steps > 1 (-1) and a rollout on a plan without a
    time input (-3) are checked on the CPU emulation only (tests/test_plan_eval_emu_cpu.py): the refusals are host code that comes before
    the first copy and is the same in both builds"""
    pv, t, _ = inputs("roll")
    plan = Plan.load(exported("roll"))
    L, h, s = plan._lib, plan._h, torch.cuda.current_stream().cuda_stream
    targets = torch.zeros(3, 2, 3, 16, 16, device=DEV)
    sums = torch.full((3, 2, 2, 4), 7.0, dtype=torch.float64, device=DEV)

    def call(pixel_values=pv, time=t, tg=targets, steps=3, slices=(0, 1, 3), groups=2, out=sums):
        rc = L.scot_plan_evaluate(h, PE.addr(pixel_values), PE.addr(time), PE.addr(tg), steps, None if slices is None else E.int_array(list(slices)),
                                  groups, PE.addr(out), None, s)
        torch.cuda.synchronize()
        return rc
    for kw in (dict(pixel_values=None), dict(tg=None), dict(out=None), dict(steps=0), dict(groups=0), dict(groups=33, slices=range(34)),
               dict(slices=(0, 2, 1)), dict(slices=(0, 1, 1)), dict(slices=(0, 1, 4)), dict(time=None), dict(slices=None)):
        assert call(**kw) == -1, kw
        assert bool((sums == 7.0).all()), kw
    assert call() == 0 and torch.isfinite(sums).all() and not bool((sums == 7.0).any())
    plan.free()


def test_evaluation_runs_without_python(tmp_path):
    """examples/plan_eval_host.c, built with hipcc, run as a fresh child process on the fp16 C = 96 plan: it prints the numbers Python
    derives from Plan.evaluate's sums"""
    from scOT import metrics as M
    image = exported("wide")
    pv, t, _ = inputs("wide")
    plan = Plan.load(image)
    steps, slices = 3, [0, 1, 3, 4]
    targets = PE.targets_for(plan.rollout(pv, t, steps).transpose(0, 1).contiguous().cpu())      # C layout
    sums = plan.evaluate(pv, t, targets.to(DEV).transpose(0, 1).contiguous(), steps=steps, channel_slice_list=slices)
    rel = M.relative_lp_error_from_sums(sums, 1).cpu().numpy()                                    # [steps, B, G]
    plan.free()
    torch.cuda.synchronize()
    exe, path = str(tmp_path / "plan_eval_host"), str(tmp_path / "wide.plan")
    open(path, "wb").write(image)
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(scot_build.HIPCC)))
    cc = subprocess.run([scot_build.HIPCC, "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                         os.path.join(ROOT, "examples", "plan_eval_host.c"), "-o", exe, "-ldl"], capture_output=True, text=True, timeout=120)
    assert cc.returncode == 0, cc.stderr[-3000:]
    raw_in, raw_tg = tmp_path / "input.bin", tmp_path / "targets.bin"
    raw_in.write_bytes(pv.cpu().numpy().tobytes() + t.cpu().numpy().tobytes())
    raw_tg.write_bytes(targets.numpy().tobytes())
    run = subprocess.run(["timeout", "-k", "10", "60", exe, scot_lib.LIB_PATHS["f16"], path, str(raw_in), str(raw_tg), str(steps), "0,1,3,4"],
                         capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-1000:], run.stderr[-3000:])
    rows = [ln.split() for ln in run.stdout.splitlines() if ln.startswith("step ")]
    assert len(rows) == steps * 3
    for r in rows:
        k, g, mean, median = int(r[1]), int(r[3]), float(r[5]), float(r[7])
        assert abs(mean - rel[k, :, g].mean()) <= 1e-12 * abs(mean) and abs(median - np.median(rel[k, :, g])) <= 1e-12 * abs(median), r
