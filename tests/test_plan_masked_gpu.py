"""Pixel masks in plans on the MI355X: masked training plans (scot_plan_loss_masked, scot_plan_train_step_masked), masked evaluation
(scot_plan_evaluate_masked) and the C example (examples/plan_masked_host.c) run as a child process.

What is deterministic on the GPU is compared bit for bit: the step forward's prediction under the mask, the evaluated rollout against a
hand-driven chain of scot_plan_run calls, each step's sums against the stand-alone masked kernel.  Parameter gradients are not
bit-reproducible there (fp32 atomics commit in any order), so trained weights are held to the rule of tests/test_plan_train_gpu.py: with
`floor` the rel-L2 distance of two Python runs' final parameters, the plan's must lie within 4 * floor + 2e-5 of a Python run, and that
bound must itself be below 1e-4, or the comparison shows nothing.  The caller's buffers lie in guard bands (tests/kernel_checks.py)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import error_sums_cases as E  # noqa: E402
import kernel_checks as kc  # noqa: E402
import plan_eval_cases as PE  # noqa: E402
import plan_masked_cases as PM  # noqa: E402
from conftest import ROOT  # noqa: E402
from poseidon_amd import build as scot_build, lib as scot_lib, plan as plan_mod  # noqa: E402
from poseidon_amd.plan import Plan  # noqa: E402
from test_model_gpu import DEV  # noqa: E402
from test_plan_train_gpu import LR, build_model, guarded_batch  # noqa: E402

H = plan_mod
STEPS = 3
_cache = {}


def mask_for(name, kind, batch, k=0):
    B, C, S = batch[2].shape[0], batch[2].shape[1], batch[2].shape[2]
    if name == "T":      # the last output channel of every sample: the constant pressure plane of the reference's incompressible sets
        m = torch.zeros(B, C, dtype=torch.bool)
        m[:, -1] = True
        return m.to(DEV)
    return PM.batch_mask(kind, B, C, S, S, k).to(DEV)


def exported(name, kind, streams=1):
    key = (name, kind, streams)
    if key not in _cache:
        model, opt, batch = build_model(name)
        image = model.export_plan(batch[0], time=batch[1], labels=batch[2], pixel_mask=mask_for(name, kind, batch), train=opt, streams=streams)
        _cache[key] = (image, batch)
        del model, opt
    return _cache[key]


def context(plan):
    return E.Ctx(plan._lib, torch.device(DEV), lambda: torch.cuda.current_stream().cuda_stream, torch.cuda.synchronize)


@pytest.mark.parametrize("kind,streams", [("channel", 1), ("element", 1), ("channel", 2)])
def test_masked_loss_step_and_snapshot(kind, streams):
    image, batch = exported("small", kind, streams)
    model, opt, _ = build_model("small")
    plan = Plan.load(image)
    d, tr = plan.describe(), plan.describe_training()
    assert d["format"] == (4 if streams == 1 else 6) and d["has_pixel_mask"] == 1 and tr["mask"] == (1 if kind == "channel" else 2)
    mask = mask_for("small", kind, batch, 1)      # (another mask than the export's)
    out = model(batch[0], time=batch[1], labels=batch[2], pixel_mask=mask)
    (pv, t, y), guards = guarded_batch(batch)
    m8, g_mask = kc.guarded(tuple(mask.shape), torch.uint8, DEV, src=mask.to(torch.uint8), name="pixel_mask")
    loss, g_loss = kc.guarded((1,), torch.float32, DEV, name="loss")
    pred, g_pred = kc.guarded(tuple(y.shape), torch.float32, DEV, name="prediction")
    plan.poison(0xFF)
    plan.loss(pv, t, y, out=(loss, pred), pixel_mask=m8.data_ptr())      # (the guarded bytes themselves)
    torch.cuda.synchronize()
    assert torch.equal(pred, out.output.detach())                         # the model's own bits, the labels at the masked positions
    full = PM.expanded(mask, y.shape)
    assert bool(full.any()) and torch.equal(pred[full], y[full])
    ref = float(out.loss.detach())
    assert abs(float(loss) - ref) <= 1e-5 * abs(ref)                      # (the loss sums commit in any order)
    assert plan.snapshot(image) == image
    # one masked step: finite, applied, the caller's buffers and their bands as they were
    plan.poison(0xFF)
    plan.train_step(pv, t, y, LR, out=loss, pixel_mask=m8.data_ptr())
    st = plan.train_status()
    assert (st["applied"], st["skipped"], st["nonfinite"]) == (1, 0, 0) and np.isfinite(st["grad_norm"]) and 0.0 < st["clip_coef"] <= 1.0
    assert abs(float(loss) - ref) <= 1e-5 * abs(ref)
    kc.check_all(guards + [g_mask, g_loss, g_pred])
    assert all(torch.equal(a, b) for a, b in zip((pv, t, y), batch)) and torch.equal(m8, mask.to(torch.uint8))
    # the unmasked calls on a masked plan: the mask is missing
    s = torch.cuda.current_stream().cuda_stream
    assert plan._lib.scot_plan_loss(plan._h, pv.data_ptr(), t.data_ptr(), y.data_ptr(), loss.data_ptr(), None, s) == -1
    # snapshot -> reload -> run equals the original plan's run, without a mask
    snap = plan.snapshot(image)
    after = plan_mod.training_state(snap)
    assert torch.isfinite(after["arena"]).all() and not torch.equal(after["arena"], plan_mod.training_state(image)["arena"])
    again = Plan.load(snap)
    a, b = plan.run(batch[0], batch[1]), again.run(batch[0], batch[1])
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b)
    plan.free(), again.free()


def python_run(batch, mask):
    model, opt, _ = build_model("T")
    losses = []
    for _ in range(STEPS):
        opt.zero_grad(overlap=True)
        out = model(batch[0], time=batch[1], labels=batch[2], pixel_mask=mask)
        out.loss.backward()
        opt.step()
        losses.append(float(out.loss.detach()))
    torch.cuda.synchronize()
    assert int(model._engine.grad_overflow) == 0 and opt.skipped_steps() == 0
    return np.array(losses), model.flat_parameters().detach().cpu().clone()


def test_three_masked_steps_track_the_python_loop():
    """Poseidon-T 128 x 128 fp16, batch 4, a channel mask on the last output channel: three steps of the Python loop (twice: its own
    run-to-run floor) and of the plan; floor, bound and distance are printed before anything is asserted."""
    image, batch = exported("T", "channel")
    mask = mask_for("T", "channel", batch)
    (la, pa), (lb, pb) = python_run(batch, mask), python_run(batch, mask)
    floor = float((pa - pb).norm() / pa.norm())
    bound = 4.0 * floor + 2e-5
    plan = Plan.load(image)
    assert plan.describe_training()["mask"] == 1 and plan.describe()["pixel_mask_bytes"] == 16
    losses = torch.empty(STEPS, device=DEV)
    for k in range(STEPS):
        plan.train_step(*batch, LR, out=losses[k:k + 1], pixel_mask=mask)
    st = plan.train_status()
    lp = losses.cpu().numpy().astype(np.float64)
    pp = plan_mod.training_state(plan.snapshot(image))["arena"]
    plan.free()
    dist = float((pp - pa).norm() / pa.norm())
    gap = float(np.max(np.abs(lp - la) / la))
    print(f"\n[masked training plan, Poseidon-T fp16, {STEPS} steps] floor {floor:.2e}, bound {bound:.2e}, plan vs Python {dist:.2e}; "
          f"loss {la[0]:.4f} -> {la[-1]:.4f} / {lp[-1]:.4f}, max rel gap {gap:.2e}")
    assert bound < 1e-4, f"inconclusive: the Python loop's own run-to-run distance {floor:.2e} gives a bound of {bound:.2e}"
    assert dist <= bound
    assert (st["applied"], st["skipped"], st["nonfinite"]) == (STEPS, 0, 0)


# ------------------------------------------------------------------------------------------------------- evaluation
def small_inference():
    if "inference" not in _cache:
        model, _, batch = build_model("small")
        model.eval()
        _cache["inference"] = (model, model.export_plan(batch[0], time=batch[1]), batch)
    return _cache["inference"]


@pytest.mark.parametrize("kind", ["channel", "element"])
def test_evaluate_masked_is_the_hand_driven_chain(kind):
    _, image, batch = small_inference()
    plan = Plan.load(image)
    mask = PM.batch_mask(kind, 2, 4, 32, 32)
    PM.check_evaluate_masked(plan, context(plan), batch[0], batch[1], 3, [0, 1, 3, 4], mask)
    plan.free()


def test_evaluate_masked_follows_the_reference_trainers_chain_and_refuses_untiled_groups():
    model, image, batch = small_inference()
    plan = Plan.load(image)
    mask = PM.batch_mask("channel", 2, 4, 32, 32)
    PM.check_python_chain(plan, model, batch[0], batch[1], 3, mask, [0, 1, 3, 4])
    tg = torch.zeros(3, 2, 4, 32, 32)
    rc, s, _ = PM.evaluate_masked(plan, context(plan), batch[0], batch[1], tg, mask, 3, [1, 3], False)
    assert rc == -1 and bool((s.view(torch.int64) == 0x7FF8DEADBEEF0001).all())
    plan.free()
    masked = Plan.load(exported("small", "channel")[0])      # a masked training plan is not refused for having a mask input
    PM.check_evaluate_masked(masked, context(masked), batch[0], batch[1], 3, None, mask)
    masked.free()


def test_masked_training_and_evaluation_run_without_python(tmp_path):
    """examples/plan_masked_host.c, built with hipcc, run as a fresh child process on the small masked plan: two masked steps, then a
    masked rollout — the losses within the GPU's 1e-5 and the relative L1 errors the Python wrapper derives from the same calls"""
    from scOT import metrics as M
    image, batch = exported("small", "channel")
    rollout, steps = 3, 2
    masks = [mask_for("small", "channel", batch, k) for k in range(steps)]
    plan = Plan.load(image)
    losses = [float(plan.train_step(*batch, LR, pixel_mask=m)) for m in masks]
    targets = PE.targets_for(plan.rollout(batch[0], batch[1], rollout).transpose(0, 1).contiguous().cpu())      # C layout
    sums = plan.evaluate(batch[0], batch[1], targets.to(DEV).transpose(0, 1).contiguous(), steps=rollout, pixel_mask=masks[0])
    rel = M.relative_lp_error_from_sums(sums, 1).cpu().numpy()[:, :, 0]      # [rollout, B]
    plan.free()
    torch.cuda.synchronize()
    exe, path = str(tmp_path / "plan_masked_host"), str(tmp_path / "masked.plan")
    open(path, "wb").write(image)
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(scot_build.HIPCC)))
    cc = subprocess.run([scot_build.HIPCC, "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                         os.path.join(ROOT, "examples", "plan_masked_host.c"), "-o", exe, "-ldl"], capture_output=True, text=True, timeout=120)
    assert cc.returncode == 0, cc.stderr[-3000:]
    one = b"".join(x.cpu().numpy().tobytes() for x in batch)
    (tmp_path / "batches.bin").write_bytes(b"".join(one + m.to(torch.uint8).cpu().numpy().tobytes() for m in masks))      # (8 mask bytes: no padding)
    groups = plan_mod.training_words(image)[H.TR_GROUPS]
    (tmp_path / "lr.bin").write_bytes(np.full(steps * groups, LR, dtype=np.float32).tobytes())
    (tmp_path / "targets.bin").write_bytes(targets.numpy().tobytes())
    run = subprocess.run(["timeout", "-k", "10", "60", exe, scot_lib.LIB_PATHS["bf16"], path, str(tmp_path / "batches.bin"),
                          str(tmp_path / "lr.bin"), str(tmp_path / "targets.bin"), str(rollout)], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-1000:], run.stderr[-3000:])
    got = [float(x) for x in re.findall(r"step \d+ loss (\S+)", run.stdout)]
    assert len(got) == steps and all(abs(a - b) <= 1e-5 * abs(b) for a, b in zip(got, losses)), (got, losses)
    rows = re.findall(r"rollout (\d+) sample (\d+) relative_l1 (\S+)", run.stdout)
    assert len(rows) == rollout * 2
    for k, b, v in rows:
        # (the two fine-tunes differ by the order their gradient atomics committed in: the weights agree to ~1e-6, not bit for bit)
        assert abs(float(v) - rel[int(k), int(b)]) <= 1e-3 * abs(rel[int(k), int(b)]), (k, b, v, rel)
