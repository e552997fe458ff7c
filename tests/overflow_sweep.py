"""fp16 gradient overflow is always SEEN, never clipped: the sweep shared by tests/test_model_gpu.py (MI355X) and
tests/test_model_emu_cpu.py (the same kernels compiled for the host).

The default compute mode runs its backward under a power-of-two gradient scale S that lives on the device; FusedAdamW doubles it after
N clean steps and halves it after a step whose gradient norm is not finite, so in a long run S climbs until something overflows.
Training is correct only if an Inf produced in ANY 16-bit gradient tensor of the backward reaches the fp32 gradient arena as Inf / NaN:
then scot_clip_coef sets clip[2] and the step is skipped.  A kernel that clamps instead (a saturating convert, a max / med3 that drops
a NaN, a "safe" epilogue) lets steps with clipped gradients through.  Hence, at EVERY scale, a step is either flagged or right.

`sweep` runs one model over S = 2^k and asks the real decision path (FusedAdamW.step: scot_grad_sqnorm, scot_clip_coef, scot_adamw_step,
scot_optim_finish) at each k:
  flagged      -> parameters, both moments and the 16-bit weight copy are bit-identical to before, skipped_steps() grew by one, the
                  scale was halved, and (where the un-scale pass visits the whole arena) engine.grad_overflow grew
  not flagged  -> every parameter gradient is finite and e(S), the global relative L2 error against the fp32-mode gradients, is at most
                  1.25 e(S_auto): the backward is linear in the upstream gradient and a power of two is exact apart from underflow,
                  so above S_auto the error can only fall (0.25: the run-to-run summation order of the atomics)
  monotone     -> once a scale is flagged every larger one is; the sweep holds both kinds; its top (2^40) is flagged — a backward that
                  clamps everything cannot pass
and finally repeats S_auto: what a flagged step left in the arena, the scratch copies and the tape must not reach the next step."""
import numpy as np
import torch

TOP = 40
# e(S_auto) per model: the bound the project already asserts for that model's fp16 gradients where there is one (tiny_trained: 5e-2,
# test_engine_reduced_precision_modes), otherwise twice the value measured on the MI355X (see the tests' docstrings)
RATIO = 1.25


def fp32_arena_grads(model32, kw):
    model32.zero_grad()
    model32(**kw).loss.backward()
    return model32.flat_grads().detach().to("cpu", torch.float64).clone()


def param_mask(opt):
    """True for arena floats that belong to a parameter (the optimizer's own map: 255 = alignment padding / the key-bias slot)"""
    return (opt._map != 255).repeat_interleave(8).cpu()


def set_scale(eng, k):
    eng.scale_state.copy_(torch.tensor([2.0 ** k, 2.0 ** -k, 0.0, 0.0]))


def rel_err(g, g32, mask):
    g, r = g.detach().to("cpu", torch.float64)[mask], g32[mask]
    return float((g - r).norm() / r.norm())


def decide(model, opt):
    """One FusedAdamW.step() on the gradients in the arena -> clip[2]; a flagged step must have changed nothing but the counters and
    the scale."""
    eng = model._engine
    before = [t.clone() for t in (model.flat_parameters(), opt.exp_avg, opt.exp_avg_sq, eng.shadow)]
    clock, S = (opt.applied_steps(), opt.skipped_steps()), eng.grad_scale_value()
    opt.step()
    flagged = int(opt._clip[2]) == 1
    if flagged:
        after = (model.flat_parameters(), opt.exp_avg, opt.exp_avg_sq, eng.shadow)
        for name, a, b in zip(("p", "exp_avg", "exp_avg_sq", "16-bit shadow"), before, after):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"a flagged step changed {name}"
        assert (opt.applied_steps(), opt.skipped_steps()) == (clock[0], clock[1] + 1)
        assert eng.grad_scale_value() == S / 2
    else:
        assert (opt.applied_steps(), opt.skipped_steps()) == (clock[0] + 1, clock[1])
    return flagged


def sweep(model, kw, g32, e_auto_bound, ks=None, lazy=False, tape=False, tag="", opt=None):
    """-> dict(k_auto, first_flagged, e_auto, e={k: e(2^k)}).  `model` is an fp16-mode ScOT; `ks` defaults to log2(S_auto) .. 40;
    `opt` a FusedAdamW with lr = 0 (built here unless given)."""
    if opt is None:
        from scOT.trainer import FusedAdamW
        opt = FusedAdamW(model, lr=0.0)
    eng = model._engine
    assert eng.scale_grads and eng.shadow is not None
    eng.tape_mode = tape
    mask = param_mask(opt)
    model.zero_grad()
    model(**kw).loss.backward()                          # the first training forward chooses S_auto (and is the tape's direct step)
    k_auto = int(np.log2(eng.grad_scale_value()))
    assert 2.0 ** k_auto == eng.grad_scale_value() and int(eng.grad_overflow) == 0
    ks = list(range(k_auto, TOP + 1)) if ks is None else list(ks)
    assert ks[0] == k_auto and ks[-1] == TOP and ks == sorted(ks)
    flags, errs = {}, {}
    for k in ks + [k_auto]:
        model.zero_grad(lazy=lazy)
        assert eng.lazy_grads == lazy
        out = model(**kw)
        set_scale(eng, k)
        ov0 = int(eng.grad_overflow)
        out.loss.backward()
        assert not eng.lazy_grads
        counted = int(eng.grad_overflow) - ov0
        g = model.flat_grads().detach().clone()
        flagged = decide(model, opt)
        again = k in flags                               # the closing repeat of S_auto
        print(f"[overflow sweep {tag}] S = 2^{k}: {'flagged' if flagged else 'applied'}, grad_overflow +{counted}, "
              f"non-finite {int((~torch.isfinite(g.cpu()[mask])).sum())} of {int(mask.sum())}"
              + ("" if flagged else f", e(S) {rel_err(g, g32, mask):.3e}"))
        if flagged:
            if not lazy:
                assert counted > 0, f"S = 2^{k}: the optimizer saw an overflow the engine's counter missed"
        else:
            assert bool(torch.isfinite(g.cpu()[mask]).all()), f"S = 2^{k}: not flagged, yet non-finite parameter gradients"
            e = rel_err(g, g32, mask)
            if k == k_auto:
                assert e <= e_auto_bound, f"e(S_auto) = {e:.3e} (bound {e_auto_bound:.1e})" + (" after a flagged step" if again else "")
            else:
                assert e <= RATIO * errs[k_auto], f"S = 2^{k}: e(S) = {e:.3e} > {RATIO} x e(S_auto) = {errs[k_auto]:.3e}"
            if not again:
                errs[k] = e
        if again:
            assert not flagged, "S_auto is flagged after the sweep: a flagged step left something behind"
        else:
            flags[k] = flagged
    seq = [flags[k] for k in ks]
    assert seq == sorted(seq), f"not monotone: {flags}"                      # once flagged, always flagged
    assert not seq[0] and seq[-1], f"not bracketed / the top of the sweep is not flagged: {flags}"
    first = next(k for k in ks if flags[k])
    print(f"[overflow sweep {tag}] S_auto 2^{k_auto}, first flagged 2^{first}, e(S_auto) {errs[k_auto]:.3e}")
    return dict(k_auto=k_auto, first_flagged=first, e_auto=errs[k_auto], e=errs)


def input_grad_sweep(model, make_kw, ref, e_auto_bounds, ks=None, tag=""):
    """Frozen model, gradients with respect to pixel_values and time: at every scale each of d_pv, d_t is either non-finite with
    grad_overflow > 0 or within the rule above against the fp32-mode input gradients `ref` = (d_pv, d_t)."""
    eng = None
    flags, errs = {}, {}
    kw = make_kw()
    model(**kw).loss.backward()
    eng = model._engine
    k_auto = int(np.log2(eng.grad_scale_value()))
    ks = list(range(k_auto, TOP + 1)) if ks is None else list(ks)
    assert ks[0] == k_auto and ks[-1] == TOP
    for k in ks:
        kw = make_kw()
        out = model(**kw)
        set_scale(eng, k)
        ov0 = int(eng.grad_overflow)
        out.loss.backward()
        counted = int(eng.grad_overflow) - ov0
        got = (kw["pixel_values"].grad, kw["time"].grad)
        fin = [bool(torch.isfinite(g).all()) for g in got]
        flags[k] = not all(fin)
        msg = f"[input-gradient sweep {tag}] S = 2^{k}: grad_overflow +{counted}"
        for i, name in enumerate(("d_pv", "d_t")):
            if not fin[i]:
                msg += f", {name} non-finite"
                assert counted > 0, f"S = 2^{k}: {name} is not finite and grad_overflow did not move"
                continue
            e = float((got[i].detach().cpu().double() - ref[i]).norm() / ref[i].norm())
            msg += f", {name} e(S) {e:.3e}"
            if k == k_auto:
                errs[name] = e
                assert e <= e_auto_bounds[i], (name, e)
            else:
                assert e <= RATIO * errs[name], f"S = 2^{k}: {name} e(S) = {e:.3e} > {RATIO} x e(S_auto) = {errs[name]:.3e}"
        print(msg)
        assert all(p.grad is None for p in model.parameters())
    seq = [flags[k] for k in ks]
    assert seq == sorted(seq) and not seq[0] and seq[-1], flags
    first = next(k for k in ks if flags[k])
    print(f"[input-gradient sweep {tag}] S_auto 2^{k_auto}, first non-finite 2^{first}, e(S_auto) {errs}")
    return dict(k_auto=k_auto, first_flagged=first, e_auto=errs)


def recovery(model, kw, g32, opt, e_auto_bound, start=30):
    """Recovery through REAL overflow: the scale starts at 2^30 (GradScaler's ceiling), every backward overflows until the optimizer has
    halved it far enough, then steps are applied; with growth_interval = 2 the scale doubles after two of them, overflows again and is
    halved again.  Runs until three steps have been applied.  No flagged step is ever applied, a skipped one changes nothing, and a
    checkpoint taken in the middle of the skips restores the clock and the scale."""
    import copy
    eng = model._engine
    assert opt.growth_interval == 2 and eng.scale_grads
    mask = param_mask(opt)
    model.zero_grad()
    model(**kw).loss.backward()                          # S_auto, for the error rule of the sweep
    k_auto = int(np.log2(eng.grad_scale_value()))
    e_auto = rel_err(model.flat_grads(), g32, mask)
    assert e_auto <= e_auto_bound and int(eng.grad_overflow) == 0
    set_scale(eng, start)
    history, ckpt = [], None
    while opt.applied_steps() < 3:
        assert len(history) < 2 * start, history         # (never: at S = 1 at the latest nothing overflows)
        S = eng.grad_scale_value()
        opt.zero_grad()
        model(**kw).loss.backward()
        g = model.flat_grads().detach().clone()
        clean = bool(torch.isfinite(g.cpu()[mask]).all())
        before = [t.clone() for t in (model.flat_parameters(), opt.exp_avg, opt.exp_avg_sq, eng.shadow)]
        clock = (opt.applied_steps(), opt.skipped_steps())
        opt.step()
        flagged = int(opt._clip[2]) == 1
        history.append((int(np.log2(S)), flagged))
        assert flagged != clean, f"S = {S}: flagged {flagged}, gradients finite {clean}"     # no flagged step applied, no clean one skipped
        if flagged:
            for name, a, b in zip(("p", "exp_avg", "exp_avg_sq", "16-bit shadow"), before, (model.flat_parameters(), opt.exp_avg, opt.exp_avg_sq, eng.shadow)):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"a skipped step changed {name}"
            assert (opt.applied_steps(), opt.skipped_steps()) == (clock[0], clock[1] + 1)      # Adam's clock does not move
            assert eng.grad_scale_value() == S / 2                                              # halved exactly once per skip
            if opt.skipped_steps() == 3 and ckpt is None:
                ckpt = copy.deepcopy(opt.state_dict())
        else:
            assert (opt.applied_steps(), opt.skipped_steps()) == (clock[0] + 1, clock[1])
            assert not torch.equal(before[0], model.flat_parameters())
            if clock[0] == 0:       # the first applied step: same weights as g32's, so the sweep's rule holds for its gradients
                e = rel_err(g, g32, mask)
                assert np.log2(S) > k_auto and e <= RATIO * e_auto, f"first applied step at S = {S}: e(S) = {e:.3e}, e(S_auto) = {e_auto:.3e}"
    flags = [f for _, f in history]
    first = flags.index(False)
    print(f"[recovery] (log2 S, flagged): {history}")
    assert first >= 3 and all(flags[:first]) and [k for k, _ in history[:first + 1]] == list(range(start, start - first - 1, -1))
    assert True in flags[first:], "the scale never grew back into an overflow"                 # ... and was halved again:
    again = first + flags[first:].index(True)
    assert history[again][0] == history[first][0] + 1 and history[again + 1] == (history[first][0], False)
    assert (opt.applied_steps(), opt.skipped_steps()) == (3, first + flags[first:].count(True)) and opt.step_count == len(history)
    opt.load_state_dict(ckpt)                            # the checkpoint from the middle of the skips
    assert (opt.applied_steps(), opt.skipped_steps(), opt.step_count) == (0, 3, 3) and eng.grad_scale_value() == 2.0 ** (start - 3)
    assert float(opt.exp_avg.abs().max()) == 0.0 and float(opt.exp_avg_sq.abs().max()) == 0.0
    return history
