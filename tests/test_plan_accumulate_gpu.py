"""Gradient accumulation in training plans on the MI355X: scot_plan_accumulate / scot_plan_apply through the Python wrapper, and from a
plain C program (examples/plan_accumulate_host.c) run as a child process.

The backward's gradients are not bit-reproducible on the GPU (fp32 atomics commit in any order), everything after them is: the
accumulator is checked bit for bit against the micro-batch gradients the plan itself produced (A_k == A_{k-1} + g_k * w as two eager
torch operations), and the update against the fused optimizer stepping on that very accumulator.  Trained weights are held to the
run-to-run distance of the Python accumulation loop itself, by the rule of test_plan_train_gpu.test_six_steps_track_the_python_loop:
with `floor` the rel-L2 distance of two Python runs' final parameters, the plan's must lie within 4 * floor + 2e-5 of a Python run,
and that bound must itself be below 1e-4, or the comparison shows nothing.

The caller's buffers lie in NaN guard bands (tests/kernel_checks.py)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_checks as kc  # noqa: E402
from conftest import ROOT  # noqa: E402
from poseidon_amd import build as scot_build, lib as scot_lib, plan as plan_mod  # noqa: E402
from poseidon_amd.plan import Plan  # noqa: E402
from test_model_gpu import DEV  # noqa: E402
from test_plan_train_gpu import LR, build_model, exported, guarded_batch, with_scale  # noqa: E402

H = plan_mod
THIRD = float(torch.tensor(1.0 / 3.0, dtype=torch.float32))      # the fp32 weight the C call receives, exactly


def micro_batch(batch, k):
    """micro-batch k of an update: the export's samples in another order (rolled along the batch dimension).  The samples are
    independent, so every micro-batch stays inside the binary16 range the export's gradient scale was picked for: the synthetic
    Poseidon-T weights overflow it on other inputs (the same batch rolled along x: 5 non-finite counts from a fresh
    plan's first forward and backward), which is the skipped-update test's subject, not these tests'."""
    return tuple(x.roll(k, 0).contiguous() for x in batch) if k else batch


def arena_distance(a, b):
    return float((a - b).norm() / b.norm())


# ------------------------------------------------------------------------------------------------------- composition, bit for bit
@pytest.mark.parametrize("name", ["small", "T"])
def test_accumulator_and_update_compose_bit_for_bit(name):
    image, batch = exported(name)
    model, opt, _ = build_model(name)
    on = (opt._map != 255).repeat_interleave(8)
    plan = Plan.load(image)
    loss, g_loss = kc.guarded((1,), torch.float32, DEV, name="loss")
    A = None
    plan.poison(0xFF)
    for k in range(3):
        (pv, t, y), guards = guarded_batch(micro_batch(batch, k))
        plan.accumulate(pv, t, y, THIRD, k == 0, out=loss)
        torch.cuda.synchronize()
        g, mine = plan.gradients(0).clone(), plan.gradients(1).clone()
        want = g * THIRD if k == 0 else A + g * THIRD
        bad = int((~torch.isfinite(g[on])).sum())
        assert bool(torch.isfinite(loss).all()) and bad == 0 and float(g[on].abs().max()) > 0.0, (k, bad, plan.train_status())
        assert torch.equal(mine[on], want[on]) and float(mine[~on].abs().max()) == 0.0, k
        kc.check_all(guards + [g_loss])
        assert all(torch.equal(a, b) for a, b in zip((pv, t, y), micro_batch(batch, k)))
        A = mine
    assert plan.accumulation_status() == dict(micro_batches=3, bytes=4 * A.numel())
    plan.apply(LR)
    snap = plan_mod.training_state(plan.snapshot(image))
    st = plan.train_status()
    plan.free()
    # the fused optimizer on that very accumulator, from the image's state: optim.hip has no atomics and a fixed grid
    plan_mod.load_training_state(image, model, opt)
    out = model(batch[0], time=batch[1], labels=batch[2])      # (the engine's 16-bit copies of the loaded weights; no state changes)
    del out
    model._arena.grad.copy_(A)
    for grp in opt.param_groups:
        grp["lr"] = LR
    opt.step()
    torch.cuda.synchronize()
    assert (st["applied"], st["skipped"], st["nonfinite"]) == (1, 0, 0)
    assert torch.equal(snap["arena"], model._arena.data.cpu()) and not torch.equal(snap["arena"], plan_mod.training_state(image)["arena"])
    assert torch.equal(snap["exp_avg"], opt.exp_avg.cpu()) and torch.equal(snap["exp_avg_sq"], opt.exp_avg_sq.cpu())
    assert torch.equal(snap["step_state"], opt._step_state.cpu())
    assert st["grad_norm"] == float(opt.last_grad_norm) and st["clip_coef"] == float(opt._clip[0])
    if "shadow" in snap:
        mine16 = model._engine.shadow.view(torch.int16).reshape(-1).cpu()
        assert torch.equal(snap["shadow"][on.cpu()], mine16[on.cpu()])


# ------------------------------------------------------------------------------------------------------- a skipped update
def test_an_overflowed_accumulation_is_one_skipped_step():
    """gradient scale 2^30 in the image's stored state: both micro-batches overflow binary16, the ONE update is skipped on the device"""
    image, batch = exported("T")
    hot = with_scale(image, 30)
    plan = Plan.load(hot)
    counted = []
    for k in range(2):
        plan.accumulate(*micro_batch(batch, k), 0.5, k == 0)
        st = plan.train_status()
        counted.append(st["nonfinite"])
        assert (st["applied"], st["skipped"], st["grad_scale"]) == (0, 0, 2.0 ** 30)      # nothing moves during an accumulation
    assert 0 < counted[0] < counted[1]
    plan.apply(LR)
    st = plan.train_status()
    assert (st["applied"], st["skipped"], st["nonfinite"], st["grad_scale"]) == (0, 1, counted[1], 2.0 ** 29)
    a, b = plan_mod.training_state(hot), plan_mod.training_state(plan.snapshot(hot))
    for k in ("arena", "exp_avg", "exp_avg_sq", "shadow", "shadow_t"):
        assert torch.equal(a[k], b[k]), k
    assert b["step_state"].tolist() == [0, 1]
    plan.free()


# ------------------------------------------------------------------------------------------------------- against the Python loop
UPDATES, MICRO = 3, 2


def python_run(batch):
    """UPDATES updates of MICRO micro-batches through the engine's accumulating backward -> (mean loss per update, final parameters)"""
    model, opt, _ = build_model("T")
    w, losses = 1.0 / MICRO, []
    for _ in range(UPDATES):
        opt.zero_grad()
        mean = 0.0
        for k in range(MICRO):
            b = micro_batch(batch, k)
            out = model(b[0], time=b[1], labels=b[2])
            (out.loss * w).backward()
            mean += float(out.loss.detach()) * w
        opt.step()
        losses.append(mean)
    torch.cuda.synchronize()
    assert int(model._engine.grad_overflow) == 0 and opt.skipped_steps() == 0
    return np.array(losses), model.flat_parameters().detach().cpu().clone()


def plan_run(image, batch, updates):
    plan = Plan.load(image)
    losses = torch.empty(updates, MICRO, device=DEV)
    for u in range(updates):
        for k in range(MICRO):
            plan.accumulate(*micro_batch(batch, k), 1.0 / MICRO, k == 0, out=losses[u, k:k + 1])
        plan.apply(LR)
    st = plan.train_status()
    arena = plan_mod.training_state(plan.snapshot(image))["arena"]
    plan.free()
    return losses.mean(1).cpu().numpy().astype(np.float64), arena, st


def test_three_updates_track_the_python_accumulation_loop(tmp_path):
    """Poseidon-T fp16, three updates of two micro-batches, w = 0.5: the Python loop (twice: its own run-to-run floor), the plan through
    the wrapper, (first = 1, weight = 1) + apply against train_step, and the C example as a child process.  The figures are printed
    before anything is asserted (recorded in profiles/plan_accumulate/README.md)."""
    image, batch = exported("T")
    (la, pa), (lb, pb) = python_run(batch), python_run(batch)
    floor = arena_distance(pb, pa)
    bound = 4.0 * floor + 2e-5
    lp, pp, st = plan_run(image, batch, UPDATES)
    dist = arena_distance(pp, pa)
    gap = float(np.max(np.abs(lp - la) / la))
    print(f"\n[accumulating plan, Poseidon-T fp16, {UPDATES} updates x {MICRO} micro-batches] floor {floor:.2e}, bound {bound:.2e}, "
          f"plan vs Python {dist:.2e}; loss {la[0]:.4f} -> {la[-1]:.4f} / {lp[-1]:.4f}, max rel gap {gap:.2e}")
    # one micro-batch of weight 1 + apply against train_step, three steps each
    whole, cut = Plan.load(image), Plan.load(image)
    for _ in range(3):
        whole.train_step(*batch, LR)
        cut.accumulate(*batch, 1.0, True)
        cut.apply(LR)
    pw, pc1 = (plan_mod.training_state(p.snapshot(image))["arena"] for p in (whole, cut))
    same = whole.train_status()["applied"] == cut.train_status()["applied"] == 3
    whole.free(), cut.free()
    dist_cut = arena_distance(pc1, pw)
    print(f"[accumulate(first=1, weight=1) + apply vs train_step, 3 steps] {dist_cut:.2e}")
    # ... and from C: a fresh child process, no Python; two updates against the wrapper's two
    exe, path, snap_path = str(tmp_path / "plan_accumulate_host"), str(tmp_path / "train.plan"), str(tmp_path / "snapshot.plan")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(scot_build.HIPCC)))
    cc = subprocess.run([scot_build.HIPCC, "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                         os.path.join(ROOT, "examples", "plan_accumulate_host.c"), "-o", exe, "-ldl"], capture_output=True, text=True, timeout=120)
    assert cc.returncode == 0, cc.stderr[-3000:]
    with open(path, "wb") as f:
        f.write(image)
    one = b"".join(b"".join(x.cpu().numpy().tobytes() for x in micro_batch(batch, k)) for k in range(MICRO))
    (tmp_path / "batches.bin").write_bytes(one * 2)
    groups = plan_mod.training_words(image)[H.TR_GROUPS]
    (tmp_path / "lr.bin").write_bytes(np.full(2 * groups, LR, dtype=np.float32).tobytes())
    run = subprocess.run(["timeout", "-k", "10", "120", exe, scot_lib.LIB_PATHS["f16"], path, str(tmp_path / "batches.bin"),
                          str(tmp_path / "lr.bin"), snap_path, str(MICRO)], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-1000:], run.stderr[-3000:])
    rows = re.findall(r"update (\d+) loss (\S+) applied (\d+) skipped (\d+)", run.stdout)
    assert [int(r[0]) for r in rows] == [0, 1], run.stdout[-2000:]
    lp2, pp2, _ = plan_run(image, batch, 2)
    pc = plan_mod.training_state(open(snap_path, "rb").read())["arena"]
    dist_c = arena_distance(pc, pp2)
    gap_c = float(np.max(np.abs(np.array([float(r[1]) for r in rows]) - lp2) / lp2))
    print(f"[examples/plan_accumulate_host.c] C vs the wrapper {dist_c:.2e}, max rel loss gap {gap_c:.2e}, last row: {run.stdout.strip().splitlines()[-1]}")
    assert bound < 1e-4, f"inconclusive: the Python loop's own run-to-run distance {floor:.2e} gives a bound of {bound:.2e}"
    assert dist <= bound and dist_cut <= bound and dist_c <= bound
    assert gap < 1e-3 and gap_c < 1e-3 and float(np.max(np.abs(lb - la) / la)) < 1e-3
    assert (st["applied"], st["skipped"], st["nonfinite"]) == (UPDATES, 0, 0) and same and (int(rows[-1][2]), int(rows[-1][3])) == (2, 0)
    assert lp[-1] < lp[0]
