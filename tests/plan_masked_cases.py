"""What the pixel-mask plan tests share (tests/test_plan_masked_emu_cpu.py on the CPU emulation, tests/test_plan_masked_gpu.py on the
MI355X): the masks of a batch, scot_plan_evaluate_masked on guarded buffers, and its bitwise checks against a hand-driven chain of
scot_plan_run calls and the stand-alone scot_error_sums_masked.  A plain module; the callers pass error_sums_cases.Ctx."""
import torch

import error_sums_cases as E
import error_sums_masked_cases as MC
import kernel_checks as kc
import plan_eval_cases as PE


def batch_mask(kind, B, Cout, H, W, k=0):
    """the pixel_mask of batch k: "channel" -> bool [B, Cout], a different pattern per sample and per k, the last channel of sample 0
    always masked; "element" -> bool [B, Cout, H, W], about 30 % set; "shared" -> bool [B, 1, H, W] (one mask for all channels)"""
    if kind == "channel":
        m = torch.tensor([[(b + c + k) % 3 == 0 for c in range(Cout)] for b in range(B)])
        m[0, Cout - 1] = True
        return m
    g = torch.Generator().manual_seed(900 + k)
    return torch.rand(B, Cout if kind == "element" else 1, H, W, generator=g) < 0.3


def expanded(mask, shape):
    """a mask of any accepted form -> bool of the prediction's shape"""
    return (mask[:, :, None, None] if mask.dim() == 2 else mask).expand(shape)


def evaluate_masked(plan, ctx, pv, t, targets, mask, steps, slices, with_predictions):
    """scot_plan_evaluate_masked with every buffer of the caller's inside guard bands, the plan's scratch poisoned first.  mask: bool
    [B, Cout] or [B, Cout, H, W], or None.  -> (status, sums [steps, B, G, 4], predictions [steps, B, Cout, H, W] or None) on the CPU"""
    dev = ctx.device
    groups = 1 if slices is None else len(slices) - 1
    gx, g0 = kc.guarded(tuple(pv.shape), torch.float32, dev, src=pv.to(dev), name="pixel_values")
    gt, g1 = kc.guarded(tuple(t.shape), torch.float32, dev, src=t.to(dev), name="time")
    gy, g2 = kc.guarded(tuple(targets.shape), torch.float32, dev, src=targets.to(dev), name="targets")
    gs, g3 = kc.guarded((steps, pv.shape[0], groups, 4), torch.float64, dev, name="sums")
    gp, g4 = kc.guarded(tuple(targets.shape), torch.float32, dev, name="predictions") if with_predictions else (None, None)
    gm, g5 = (None, None) if mask is None else kc.guarded(tuple(mask.shape), torch.uint8, dev, src=mask.to(torch.uint8).to(dev), name="mask")
    plan.poison(0xFF)
    rc = plan._lib.scot_plan_evaluate_masked(plan._h, PE.addr(gx), PE.addr(gt), PE.addr(gy), PE.addr(gm), int(mask is not None and mask.dim() == 4),
                                             steps, None if slices is None else E.int_array(slices), groups, PE.addr(gs), PE.addr(gp),
                                             ctx.stream())
    ctx.sync()
    kc.check_all([g for g in (g0, g1, g2, g3, g4, g5) if g is not None])
    assert torch.equal(gx.cpu(), pv.cpu()) and torch.equal(gy.cpu(), targets.cpu())
    return rc, gs.cpu().clone(), None if gp is None else gp.cpu().clone()


def hand_chain(plan, ctx, pv, t, targets, mask, steps):
    """the chain the call is defined as: scot_plan_run at time / steps (torch's own rounding on ctx.device, which the rollout follows),
    where(mask, targets[k], prediction), copy back over the first Cout input channels, repeat
    -> (raw predictions, overwritten predictions), each [steps, B, Cout, H, W] on the CPU"""
    dev = ctx.device
    x, t_step = pv.to(dev).clone(), (t.to(dev) / steps).contiguous()
    cout = targets.shape[2]
    raw, over = [], []
    for k in range(steps):
        out = torch.full(tuple(targets.shape[1:]), float("nan"), device=dev)
        plan.poison(0xFF)
        assert plan._lib.scot_plan_run(plan._h, x.data_ptr(), t_step.data_ptr(), None, out.data_ptr(), ctx.stream()) == 0
        ctx.sync()
        raw.append(out.cpu().clone())
        out = torch.where(expanded(mask, out.shape).to(dev), targets[k].to(dev), out)
        over.append(out.cpu().clone())
        x[:, :cout] = out
    return torch.stack(raw), torch.stack(over)


def check_evaluate_masked(plan, ctx, pv, t, steps, slices, mask):
    """the bitwise checks of scot_plan_evaluate_masked on one (plan, inputs, mask) -> (sums, targets, overwritten predictions)"""
    plain = PE.reference_predictions(plan, ctx, pv, t, steps)
    targets = PE.targets_for(plain)
    raw, over = hand_chain(plan, ctx, pv, t, targets, mask, steps)
    assert torch.isfinite(over).all() and not PE.same_bits(over[-1], plain[-1])      # (the mask changes the rollout)
    rc, sums, preds = evaluate_masked(plan, ctx, pv, t, targets, mask, steps, slices, True)
    assert rc == 0 and PE.same_bits(preds, over), "predictions differ from the hand-driven chain's"
    B, C = raw.shape[1], raw.shape[2]
    for k in range(steps):      # step k's sums: the stand-alone masked kernel on that step's prediction
        alone = MC.MaskedLaunch(ctx, raw[k].reshape(B, C, -1), targets[k].reshape(B, C, -1), slices,
                                mask.reshape(B, C, -1) if mask.dim() == 4 else mask)
        assert alone.call_masked(0) == 0
        assert PE.same_bits(sums[k], alone.result()), f"step {k}: not the stand-alone masked kernel's sums of that prediction"
    rc, lean, none = evaluate_masked(plan, ctx, pv, t, targets, mask, steps, slices, False)
    assert rc == 0 and none is None and PE.same_bits(lean, sums), "predictions == NULL changes the sums"
    # a NULL mask is scot_plan_evaluate, bit for bit
    rc, s_null, p_null = evaluate_masked(plan, ctx, pv, t, targets, None, steps, slices, True)
    rc2, s_plain, p_plain = PE.evaluate(plan, ctx, pv, t, targets, steps, slices, True)
    assert rc == 0 and rc2 == 0 and PE.same_bits(s_null, s_plain) and PE.same_bits(p_null, p_plain) and PE.same_bits(p_null, plain)
    return sums, targets, over


def check_python_chain(plan, model, pv, t, steps, mask, slices):
    """For masked channels whose target is constant in time, Plan.evaluate(..., pixel_mask=)'s last prediction equals the chain the
    reference's trainer runs: model(x, time=t / steps, labels=FINAL labels, pixel_mask=mask), its output fed back.  mask: bool [B, Cout]."""
    from scOT import metrics as M
    dev = pv.device
    with torch.no_grad():
        base = plan.rollout(pv, t, steps)                                   # [B, steps, Cout, H, W]
        targets = (base * 0.9 + 0.01).contiguous()
        final = targets[:, -1].contiguous()
        m5 = mask.to(dev)[:, None, :, None, None].expand(targets.shape)
        targets = torch.where(m5, final[:, None].expand(targets.shape), targets).contiguous()      # constant in time under the mask
        sums, preds = plan.evaluate(pv, t, targets, steps=steps, channel_slice_list=slices, predictions=True, pixel_mask=mask)
        x, t_step, cout = pv.clone(), t / steps, final.shape[1]
        for _ in range(steps):
            out = model(x, time=t_step, labels=final, pixel_mask=mask.to(dev)).output
            x = torch.cat([out, x[:, cout:]], 1).contiguous()
    assert PE.same_bits(preds[:, -1].cpu(), out.cpu()), "the last prediction differs from the reference trainer's chain"
    want = M.error_sums(preds[:, -1], final, slices)      # (the overwritten prediction: the mask has nothing left to change)
    assert torch.allclose(sums[-1].cpu(), want.cpu(), rtol=1e-12, atol=0.0)
    assert PE.same_bits(M.error_sums(preds[:, -1], final, slices, pixel_mask=mask).cpu(), want.cpu())
    # the uint8 form and the plain call
    again = plan.evaluate(pv, t, targets, steps=steps, channel_slice_list=slices, pixel_mask=mask.to(torch.uint8))
    assert PE.same_bits(again.cpu(), sums.cpu())
    assert not PE.same_bits(plan.evaluate(pv, t, targets, steps=steps, channel_slice_list=slices).cpu(), sums.cpu())
