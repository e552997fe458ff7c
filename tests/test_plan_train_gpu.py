"""Training plans on the MI355X: `ScOT.export_plan(..., labels=..., train=optimizer)` records one optimizer step, the plan runtime of
the library (csrc/plan.hip) owns the training state and replays the step — from Python through ctypes here, and from a plain C program
(examples/plan_train_host.c) run as a child process.

What is deterministic on the GPU is compared bit for bit: the step forward's prediction, a skipped step, a snapshot that is loaded
again.  Parameter gradients are not bit-reproducible there (fp32 atomics commit in any order: tests/test_model_gpu.py), so the
trained weights are held to the run-to-run distance of the Python loop itself: with `floor` the rel-L2 distance of two Python runs'
final parameters, the plan's must lie within 4 * floor + 2e-5 of a Python run (the rule of test_lazy_zero_grad_equals_the_eager_fill),
and that bound must itself be below the six-step test's own 1e-4, or the comparison shows nothing.

The caller's buffers lie in NaN guard bands (tests/kernel_checks.py)."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_checks as kc  # noqa: E402
from conftest import ROOT  # noqa: E402
from poseidon_amd import build as scot_build, lib as scot_lib, plan as plan_mod  # noqa: E402
from poseidon_amd.config import ScOTConfig  # noqa: E402
from poseidon_amd.geometry import param_shapes  # noqa: E402
from poseidon_amd.plan import Plan  # noqa: E402
from poseidon_amd.synth import synth_inputs, synth_state_dict  # noqa: E402
from scOT.model import ScOT  # noqa: E402
from test_model_gpu import DEV, _preset_model  # noqa: E402

H = plan_mod
STEPS, LR = 6, 5e-5
OPT = dict(lr=LR, weight_decay=0.01, max_grad_norm=5.0)


def build_model(name):
    """-> (model in training mode, its FusedAdamW, (pixel_values, time, labels) on the device)"""
    from scOT.trainer import FusedAdamW
    if name == "small":      # the small fp32 model of tests/test_plan_gpu.py, batch 2
        cfg = ScOTConfig(image_size=32, patch_size=4, num_channels=4, num_out_channels=4, embed_dim=16, depths=[2, 2], num_heads=[1, 2],
                         skip_connections=[1, 0], window_size=4, mlp_ratio=4.0, p=1, channel_slice_list_normalized_loss=[0, 1, 3, 4],
                         drop_path_rate=0.0, use_conditioning=True)
        model = ScOT(cfg, compute="fp32")
        model.load_state_dict(synth_state_dict(param_shapes(cfg), "trained"))
        model = model.to(DEV)
        batch = synth_inputs(2, 4, 4, 32, "smooth")
    else:                    # Poseidon-T 128 x 128 fp16, batch 4: the configuration of test_training_with_lazy_zero_grad_tracks_the_eager_fill
        _, _, model = _preset_model("T", 128, 4, "fp16", engine_options={"fused_min_rows": 0})
        batch = synth_inputs(4, 4, 4, 128, "smooth")
    model.train()
    return model, FusedAdamW(model, **OPT), tuple(x.to(DEV) for x in batch)


_cache = {}


def exported(name):
    """one export per configuration for the whole module -> (image, batch)"""
    if name not in _cache:
        model, opt, batch = build_model(name)
        image = model.export_plan(batch[0], time=batch[1], labels=batch[2], train=opt)
        _cache[name] = (image, batch)
        del model, opt
    return _cache[name]


def guarded_batch(batch):
    views, guards = [], []
    for x, what in zip(batch, ("pixel_values", "time", "labels")):
        v, g = kc.guarded(tuple(x.shape), torch.float32, DEV, src=x, name=what)
        views.append(v)
        guards.append(g)
    return views, guards


def with_scale(image, exponent):
    """the image with the gradient scale in its stored state set to 2^exponent"""
    h, tr = Plan.header(image), plan_mod.training_words(image)
    buf, off, n = tr[H.TR_SCALE_STATE:H.TR_SCALE_STATE + 3]
    assert n == 16
    data_off = struct.unpack_from("<Q", image, h[H.H_BUFFERS_OFF] + 32 * buf + 16)[0]
    b = bytearray(image)
    struct.pack_into("<4f", b, h[H.H_DATA_OFF] + data_off + off, 2.0 ** exponent, 2.0 ** -exponent, 0.0, 0.0)
    return bytes(b)


@pytest.mark.parametrize("name", ["small", "T"])
def test_loss_step_and_snapshot(name):
    image, batch = exported(name)
    model, opt, _ = build_model(name)
    plan = Plan.load(image)
    d, tr = plan.describe(), plan.describe_training()
    assert d["format"] == 4 and tr["has_training"] == 1 and tr["dynamic_scale"] == (name == "T") and tr["arena_floats"] == model._arena.size
    # the step forward alone: the model's own prediction bits, no state written, nothing outside the caller's extents
    out = model(batch[0], time=batch[1], labels=batch[2])
    (pv, t, y), guards = guarded_batch(batch)
    loss, g_loss = kc.guarded((1,), torch.float32, DEV, name="loss")
    pred, g_pred = kc.guarded(tuple(y.shape), torch.float32, DEV, name="prediction")
    plan.poison(0xFF)
    plan.loss(pv, t, y, out=(loss, pred))
    torch.cuda.synchronize()
    assert torch.equal(pred, out.output.detach())
    ref = float(out.loss.detach())
    assert abs(float(loss) - ref) <= 1e-5 * abs(ref)      # (the loss sums commit in any order)
    assert plan.snapshot(image) == image
    # one step: finite, applied, the caller's buffers as they were
    plan.poison(0xFF)
    plan.train_step(pv, t, y, LR, out=loss)
    st = plan.train_status()
    assert (st["applied"], st["skipped"], st["nonfinite"]) == (1, 0, 0) and np.isfinite(st["grad_norm"]) and 0.0 < st["clip_coef"] <= 1.0
    assert abs(float(loss) - ref) <= 1e-5 * abs(ref)
    kc.check_all(guards + [g_loss, g_pred])
    assert all(torch.equal(a, b) for a, b in zip((pv, t, y), batch))
    # snapshot -> reload -> run equals the original plan's run (both see the stepped weights through their 16-bit copies)
    snap = plan.snapshot(image)
    after = plan_mod.training_state(snap)
    assert torch.isfinite(after["arena"]).all() and not torch.equal(after["arena"], plan_mod.training_state(image)["arena"])
    again = Plan.load(snap)
    a, b = plan.run(batch[0], batch[1]), again.run(batch[0], batch[1])
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert not torch.equal(a, out.output.detach())
    plan.free(), again.free()


def test_skipped_step_changes_nothing():
    """gradient scale 2^30 in the image's stored state: the backward overflows binary16, the step is skipped on the device, and the
    snapshot's parameters, moments and 16-bit copies equal the previous snapshot's; the scale is halved"""
    image, batch = exported("T")
    hot = with_scale(image, 30)
    plan = Plan.load(hot)
    plan.train_step(*batch, LR)
    st = plan.train_status()
    assert (st["applied"], st["skipped"]) == (0, 1) and st["nonfinite"] > 0 and st["grad_scale"] == 2.0 ** 29
    a, b = plan_mod.training_state(hot), plan_mod.training_state(plan.snapshot(hot))
    for k in ("arena", "exp_avg", "exp_avg_sq", "shadow", "shadow_t"):
        assert torch.equal(a[k], b[k]), k
    assert b["step_state"].tolist() == [0, 1]
    plan.free()


def python_run(name, batch):
    model, opt, _ = build_model(name)
    losses = []
    for _ in range(STEPS):
        opt.zero_grad(overlap=True)
        out = model(batch[0], time=batch[1], labels=batch[2])
        out.loss.backward()
        opt.step()
        losses.append(float(out.loss.detach()))
    torch.cuda.synchronize()
    assert int(model._engine.grad_overflow) == 0 and opt.skipped_steps() == 0
    return np.array(losses), model.flat_parameters().detach().cpu().clone()


def test_six_steps_track_the_python_loop(tmp_path):
    """Six steps of the Python loop (twice: its own run-to-run floor), of the plan through the wrapper, and of the C example as a
    child process; the figures are printed before anything is asserted (recorded in profiles/plan_train/README.md)."""
    image, batch = exported("T")
    (la, pa), (lb, pb) = python_run("T", batch), python_run("T", batch)
    floor = float((pa - pb).norm() / pa.norm())
    bound = 4.0 * floor + 2e-5
    # the plan through the Python wrapper
    plan = Plan.load(image)
    losses = torch.empty(STEPS, device=DEV)
    for k in range(STEPS):
        plan.train_step(*batch, LR, out=losses[k:k + 1])
    st = plan.train_status()
    lp = losses.cpu().numpy().astype(np.float64)
    pp = plan_mod.training_state(plan.snapshot(image))["arena"]
    plan.free()
    dist = float((pp - pa).norm() / pa.norm())
    gap = float(np.max(np.abs(lp - la) / la))
    print(f"\n[training plan, Poseidon-T fp16, {STEPS} steps] floor {floor:.2e}, bound {bound:.2e}, plan vs Python {dist:.2e}; "
          f"loss {la[0]:.4f} -> {la[-1]:.4f} / {lp[-1]:.4f}, max rel gap {gap:.2e}")
    # ... and from C: a fresh child process, no Python
    exe, path, snap_path = str(tmp_path / "plan_train_host"), str(tmp_path / "train.plan"), str(tmp_path / "snapshot.plan")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(scot_build.HIPCC)))
    cc = subprocess.run([scot_build.HIPCC, "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                         os.path.join(ROOT, "examples", "plan_train_host.c"), "-o", exe, "-ldl"], capture_output=True, text=True, timeout=120)
    assert cc.returncode == 0, cc.stderr[-3000:]
    with open(path, "wb") as f:
        f.write(image)
    one = b"".join(x.cpu().numpy().tobytes() for x in batch)
    (tmp_path / "batches.bin").write_bytes(one * STEPS)
    groups = plan_mod.training_words(image)[H.TR_GROUPS]
    (tmp_path / "lr.bin").write_bytes(np.full(STEPS * groups, LR, dtype=np.float32).tobytes())
    run = subprocess.run(["timeout", "-k", "10", "120", exe, scot_lib.LIB_PATHS["f16"], path, str(tmp_path / "batches.bin"),
                          str(tmp_path / "lr.bin"), snap_path], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-1000:], run.stderr[-3000:])
    rows = re.findall(r"step (\d+) loss (\S+) applied (\d+) skipped (\d+)", run.stdout)
    assert [int(r[0]) for r in rows] == list(range(STEPS)), run.stdout[-2000:]
    lc = np.array([float(r[1]) for r in rows])
    pc = plan_mod.training_state(open(snap_path, "rb").read())["arena"]
    dist_c = float((pc - pa).norm() / pa.norm())
    gap_c = float(np.max(np.abs(lc - la) / la))
    print(f"[examples/plan_train_host.c] C vs Python {dist_c:.2e}, max rel loss gap {gap_c:.2e}, last row: {run.stdout.strip().splitlines()[-1]}")
    assert bound < 1e-4, f"inconclusive: the Python loop's own run-to-run distance {floor:.2e} gives a bound of {bound:.2e}"
    assert dist <= bound and dist_c <= bound
    assert gap < 1e-3 and gap_c < 1e-3 and float(np.max(np.abs(lb - la) / la)) < 1e-3
    assert (st["applied"], st["skipped"], st["nonfinite"]) == (STEPS, 0, 0) and (int(rows[-1][2]), int(rows[-1][3])) == (STEPS, 0)
    assert lp[-1] < lp[0] and lc[-1] < lc[0]
