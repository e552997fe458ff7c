"""Gradients with respect to `pixel_values` and `time` on the MI355X, through the public API only: ScOT.forward and loss.backward().
References: the real reference's autograd (tests/golden/make_input_grads_fixture.py).

Bounds: fp32 rel-L2 2e-4 (three times the reference's own fp32 noise, see tests/test_input_grads_emu_cpu.py); Poseidon-T in the
default fp16 mode: d_pixel_values 4e-3 (the project's global bound for fp16 gradients), d_time 8e-2 (its bound for a single small,
cancelling gradient tensor: `tol_each` of tests/test_model_gpu.py).

Measured on the MI355X (Poseidon-T, batch 2, fp16, fused tails): see the docstring of test_poseidon_T_fp16_input_gradients."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import load_fixture, rel_l2  # noqa: E402
from test_model_gpu import DEV, build, grads_report, inputs  # noqa: E402

TOL32 = 2e-4
# Two runs of the same step on the GPU.  The loss's group sums and the norms' column sums are accumulated with atomics whose order varies
# from run to run, so fp32 results agree to a few units of fp32 rounding (the step-tape test of tests/test_model_gpu.py allows 2e-5 for
# the same reason).  In fp16 a last-bit difference of the loss normaliser flips roundings of the 16-bit gradient operands, each by up to
# 2^-11 relative: two runs are two rounding realisations of one fp16 computation, for which the project's bound is 1e-2 (the bound between
# two forms of a layer tail, tests/test_model_emu_cpu.py).  The CPU emulation, where nothing varies, asserts bit equality instead.
SAME_STEP = {"fp32": 1e-5, "fp16": 1e-2}


def leaf_inputs(cfg, meta):
    kw = inputs(cfg, meta)
    kw["pixel_values"] = kw["pixel_values"].clone().requires_grad_(True)
    if "time" in kw:
        kw["time"] = kw["time"].clone().requires_grad_(True)
    return kw


@pytest.mark.parametrize("name", ["tiny_trained", "tiny_odd", "tiny_shift3", "tiny_learnres_mask", "tiny_nocond_p2"])
def test_tiny_fixtures_fp32(name):
    f, meta = load_fixture("igrad_" + name)
    fp, _ = load_fixture(name)
    cfg, model = build(meta, "fp32")
    kw = leaf_inputs(cfg, meta)
    out = model(**kw)
    out.loss.backward()
    torch.cuda.synchronize()
    e_pv = rel_l2(kw["pixel_values"].grad.cpu().numpy(), f["grad:pixel_values"])
    e_t = rel_l2(kw["time"].grad.cpu().numpy(), f["grad:time"]) if cfg.use_conditioning else 0.0
    print(f"\n[{name} fp32] d_pixel_values {e_pv:.2e} d_time {e_t:.2e}")
    assert abs(float(out.loss) - float(f["loss"])) < 2e-5 * abs(float(f["loss"]))
    assert e_pv < TOL32 and e_t < TOL32
    grads_report(model, fp, tol_each=1e-3, tol_global=1e-4)


def test_poseidon_T_fp16_input_gradients():
    """Poseidon-T, batch 2, default fp16 mode on the fused layer tails (fused_min_rows=0: the kernels the timed batches run).
    Measured on the MI355X (two runs): d_pixel_values 2.64e-3 / 2.66e-3 (bound 4e-3), d_time 6.4e-4 / 7.6e-4 (bound 8e-2; d_time itself is
    -1.87 / -1.17 per sample), grad_overflow 0; stage 0 (C = 48) runs layer by layer in the backward, the C = 96 / 192 stages on the lean tails."""
    f, meta = load_fixture("igrad_poseidonT_trained")
    cfg, model = build(meta, "fp16")
    assert model.engine_options == {"fused_min_rows": 0}
    kw = leaf_inputs(cfg, meta)
    out = model(**kw)
    out.loss.backward()
    torch.cuda.synchronize()
    eng = model._engine
    forms = {plan.bwd for plan in eng._plans.values()}
    e_pv = rel_l2(kw["pixel_values"].grad.cpu().numpy(), f["grad:pixel_values"])
    e_t = rel_l2(kw["time"].grad.cpu().numpy(), f["grad:time"])
    print(f"\n[Poseidon-T fp16] d_pixel_values {e_pv:.3e} d_time {e_t:.3e} d_time {kw['time'].grad.tolist()} (reference {f['grad:time'].tolist()}) "
          f"loss {float(out.loss):.6f} (reference {float(f['loss']):.6f}) overflow {int(eng.grad_overflow)} tail forms {sorted(forms)}")
    assert "tail" in {plan.fwd for plan in eng._plans.values()}
    assert e_pv <= 4e-3
    assert e_t <= 8e-2
    assert int(eng.grad_overflow) == 0


def test_frozen_model():
    f, meta = load_fixture("igrad_tiny_trained")
    for compute in ("fp32", "fp16"):
        cfg, model = build(meta, compute)
        kw = leaf_inputs(cfg, meta)
        model(**kw).loss.backward()
        for p in model.parameters():
            p.requires_grad_(False)
        kw2 = leaf_inputs(cfg, meta)
        out = model(**kw2)
        assert out.loss.grad_fn is not None
        out.loss.backward()
        torch.cuda.synchronize()
        # the same data chain: bit for bit on the CPU emulation (tests/test_input_grads_emu_cpu.py); two runs on the GPU: SAME_STEP
        assert rel_l2(kw2["pixel_values"].grad.cpu().numpy(), kw["pixel_values"].grad.cpu().numpy()) < SAME_STEP[compute]
        assert rel_l2(kw2["time"].grad.cpu().numpy(), kw["time"].grad.cpu().numpy()) < SAME_STEP[compute]
        assert all(p.grad is None for p in model.parameters())
        if compute == "fp16":
            assert int(model._engine.grad_overflow) == 0
        # un-frozen again: a training step starts from a cleared arena
        for p in model.parameters():
            p.requires_grad_(True)
        _, fresh = build(meta, compute)
        for m in (model, fresh):
            m(**inputs(cfg, meta)).loss.backward()
        torch.cuda.synchronize()
        assert rel_l2(model._arena.grad.cpu().numpy(), fresh._arena.grad.cpu().numpy()) < SAME_STEP[compute]


def test_scalar_time_is_broadcast():
    f, meta = load_fixture("igrad_tiny_trained")
    cfg, model = build(meta, "fp32")
    kw = inputs(cfg, meta)
    B = kw["pixel_values"].shape[0]
    ts = torch.tensor(0.3, device=DEV, requires_grad=True)
    model(**dict(kw, time=ts)).loss.backward()
    tb = torch.full((B,), 0.3, device=DEV, requires_grad=True)
    model(**dict(kw, time=tb)).loss.backward()
    torch.cuda.synchronize()
    assert ts.grad.shape == () and kw["pixel_values"].grad is None
    assert abs(float(ts.grad) - float(tb.grad.sum())) <= SAME_STEP["fp32"] * float(tb.grad.abs().sum())


def test_resize_path():
    """a 64x64 input to the 32x32 model: the spectral resize in front of the engine is differentiable torch code around native kernels"""
    f, meta = load_fixture("igrad_tiny_resize64")
    cfg, model = build(meta, "fp32")
    kw = leaf_inputs(cfg, meta)
    assert kw["pixel_values"].shape[-1] == 64 and cfg.image_size == 32
    out = model(**kw)
    out.loss.backward()
    torch.cuda.synchronize()
    e_pv = rel_l2(kw["pixel_values"].grad.cpu().numpy(), f["grad:pixel_values"])
    e_t = rel_l2(kw["time"].grad.cpu().numpy(), f["grad:time"])
    print(f"\n[resize 64 -> 32] d_pixel_values {e_pv:.2e} d_time {e_t:.2e}")
    assert abs(float(out.loss) - float(f["loss"])) < 2e-5 * abs(float(f["loss"]))
    assert e_pv < TOL32 and e_t < TOL32


@pytest.mark.parametrize("compute", ["fp32", "fp16"])
def test_taped_steps(compute):
    """three consecutive training steps with fresh inputs under the default step tape (direct, recorded, replayed) against a model that
    never tapes; gradients handed out earlier are not overwritten by a later replay"""
    f, meta = load_fixture("igrad_tiny_trained")
    cfg, taped = build(meta, compute)
    _, plain = build(meta, compute)
    base = inputs(cfg, meta)
    kept = []
    for step in range(4):
        res = []
        for m in (taped, plain):
            if m._engine is not None:
                m._engine.tape_mode = m is taped
            kw = {k: (v * (1.0 + 0.25 * step) + 0.01 * step).detach().requires_grad_(k != "labels") for k, v in base.items()}
            m.zero_grad()
            m(**kw).loss.backward()
            res.append((kw["pixel_values"].grad, kw["time"].grad))
        torch.cuda.synchronize()
        if step == 0:
            continue          # (engines exist from here on)
        e = rel_l2(res[0][0].cpu().numpy(), res[1][0].cpu().numpy()), rel_l2(res[0][1].cpu().numpy(), res[1][1].cpu().numpy())
        print(f"[taped vs untaped, {compute}] step {step}: d_pixel_values {e[0]:.2e} d_time {e[1]:.2e}")
        assert e[0] < SAME_STEP[compute] and e[1] < SAME_STEP[compute], step
        kept.append((res[0][0], res[0][1], res[0][0].clone(), res[0][1].clone()))
    ent = [e for e in taped._engine._taped.values() if e["state"] == "ready"]
    assert len(ent) == 1 and "igrads" in ent[0]
    for a, b, a0, b0 in kept:
        assert torch.equal(a, a0) and torch.equal(b, b0)
    assert not torch.equal(kept[-1][0], kept[-2][0])


def test_refusals():
    f, meta = load_fixture("igrad_tiny_trained")
    cfg, model = build(meta, "fp32")
    kw = inputs(cfg, meta)
    with pytest.raises(NotImplementedError):
        model(**dict(kw, labels=kw["labels"].clone().requires_grad_(True)))
    a = kw["pixel_values"].clone().requires_grad_(True)
    (g,) = torch.autograd.grad(model(**dict(kw, pixel_values=a)).loss, a, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    torch.cuda.synchronize()
