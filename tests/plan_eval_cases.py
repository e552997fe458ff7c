"""What the two scot_plan_evaluate test modules share (tests/test_plan_eval_emu_cpu.py, tests/test_plan_eval_gpu.py): the call on guarded
buffers of the caller's, and the bitwise checks against scot_plan_rollout / scot_plan_run and the stand-alone scot_error_sums."""
import numpy as np
import torch

import error_sums_cases as E
import kernel_checks as kc


def addr(x):
    return None if x is None else x.data_ptr()


def targets_for(preds, seed=3):
    """targets [steps, B, Cout, H, W] near the predictions (C layout), one channel of one sample exactly zero"""
    g = torch.Generator().manual_seed(seed)
    tg = preds.cpu() * 0.9 + 0.05 * torch.randn(preds.shape, generator=g)
    tg[:, 0, 0] = 0.0
    return tg.contiguous()


def reference_predictions(plan, ctx, pv, t, steps):
    """what scot_plan_rollout (steps == 1: scot_plan_run) writes, in the C layout [steps, B, Cout, H, W], on the CPU"""
    d = plan.info
    out = torch.full((steps, d["batch"], d["out_channels"], d["height"], d["width"]), float("nan"), device=ctx.device)
    plan.poison(0xFF)
    if steps == 1:
        assert plan._lib.scot_plan_run(plan._h, addr(pv), addr(t), None, addr(out), ctx.stream()) == 0
    else:
        assert plan._lib.scot_plan_rollout(plan._h, addr(pv), addr(t), None, addr(out), steps, ctx.stream()) == 0
    ctx.sync()
    return out.cpu()


def evaluate(plan, ctx, pv, t, targets, steps, slices, with_predictions):
    """scot_plan_evaluate with every buffer of the caller's inside NaN bands, the plan's scratch poisoned first
    -> (status, sums [steps, B, G, 4] on the CPU, predictions [steps, B, Cout, H, W] on the CPU or None)"""
    dev = ctx.device
    groups = 1 if slices is None else len(slices) - 1
    gx, g0 = kc.guarded(tuple(pv.shape), torch.float32, dev, src=pv.to(dev), name="pixel_values")
    gt, g1 = (None, None) if t is None else kc.guarded(tuple(t.shape), torch.float32, dev, src=t.to(dev), name="time")
    gy, g2 = kc.guarded(tuple(targets.shape), torch.float32, dev, src=targets.to(dev), name="targets")
    gs, g3 = kc.guarded((steps, pv.shape[0], groups, 4), torch.float64, dev, name="sums")
    gp, g4 = kc.guarded(tuple(targets.shape), torch.float32, dev, name="predictions") if with_predictions else (None, None)
    plan.poison(0xFF)
    rc = plan._lib.scot_plan_evaluate(plan._h, addr(gx), addr(gt), addr(gy), steps, None if slices is None else E.int_array(slices), groups,
                                      addr(gs), addr(gp), ctx.stream())
    ctx.sync()
    kc.check_all([g for g in (g0, g1, g2, g3, g4) if g is not None])
    assert torch.equal(gx.cpu(), pv.cpu()) and torch.equal(gy.cpu(), targets.cpu())
    return rc, gs.cpu().clone(), None if gp is None else gp.cpu().clone()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64 if a.dtype == torch.float64 else torch.int32),
                                              b.contiguous().view(torch.int64 if b.dtype == torch.float64 else torch.int32))


def check_evaluate(plan, ctx, pv, t, steps, slices):
    """the bitwise checks of one (plan, inputs, steps, slices) -> (sums, targets)"""
    ref = reference_predictions(plan, ctx, pv, t, steps)
    assert torch.isfinite(ref).all()
    targets = targets_for(ref)
    rc, sums, preds = evaluate(plan, ctx, pv, t, targets, steps, slices, True)
    assert rc == 0 and same_bits(preds, ref), "predictions differ from scot_plan_rollout's / scot_plan_run's"
    assert torch.isfinite(sums).all()
    B, C = ref.shape[1], ref.shape[2]
    for k in range(steps):
        p, y = ref[k].reshape(B, C, -1), targets[k].reshape(B, C, -1)
        alone = E.Launch(ctx, p, y, slices)
        assert alone.call() == 0
        assert same_bits(sums[k], alone.result()), f"step {k}: not the stand-alone kernel's sums of that prediction"
        want, ns = E.reference(p, y, slices)
        for g, n in enumerate(ns):
            err = np.abs(sums[k, :, g].numpy() - want[:, g])
            assert (err <= 2 * (n + 2) * E.U64 * want[:, g]).all(), (k, g, err)
    rc, lean, none = evaluate(plan, ctx, pv, t, targets, steps, slices, False)
    assert rc == 0 and none is None and same_bits(lean, sums), "predictions == NULL changes the sums"
    # a run after an evaluate gives what it gave before
    out = torch.full(tuple(ref.shape[1:]), float("nan"), device=ctx.device)
    t1 = t
    if steps > 1:      # (the first forward of the rollout ran at time / steps: compare with a run at the undivided time of its own)
        first = reference_predictions(plan, ctx, pv, t, 1)[0]
    else:
        first = ref[0]
    assert plan._lib.scot_plan_run(plan._h, addr(pv), addr(t1), None, addr(out), ctx.stream()) == 0
    ctx.sync()
    assert same_bits(out.cpu(), first)
    return sums, targets
