"""The adjoint of an exported model's rollout on the CPU emulation: scot_plan_rollout_vjp (csrc/plan.hip, include/scot_plan.h) through
`Plan.rollout_vjp`, against libscot_emu.so in plain host memory.

The reference is the Python engine, never the plan (tests/plan_rollout_reference.py): R1, the explicit chain of single-step
`torch.autograd.grad` calls summed in the contract's order, bit for bit; R2, `torch.autograd.grad` through
`harness.rollout(..., output_all_steps=True, detach=False)`, bit for bit on the first Cout channels and within the association bound
of an n-term fp32 sum on the pass-through channels and on d_time.  The cotangents have the magnitude of a mean loss's gradient.

"Launches nothing" is read from the emulated runtime's launch log, `scot_plan_emu_issued()` (emulated build only)."""
import ctypes
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import plan_rollout_reference as ref_mod  # noqa: E402
from plan_support import BOTH, ROOT, SMALL, emu, frozen_exports, issued, other_inputs  # noqa: E402,F401
from plan_support import frozen_model as build_model  # noqa: E402
from poseidon_amd import lib as scotlib, plan as plan_mod  # noqa: E402
from poseidon_amd.config import ScOTConfig  # noqa: E402
from poseidon_amd.geometry import param_shapes  # noqa: E402
from poseidon_amd.plan import Plan  # noqa: E402
from poseidon_amd.synth import synth_state_dict  # noqa: E402

NAME = "scot_plan_rollout_vjp"
CASES = [("small", 1), ("small", 3), ("resid", 3), ("c96", 2)]
exported = frozen_exports()


def cotangents(model, pv, steps, seed):
    """[B, steps, Cout, H, W], O(1 / elements of one prediction)"""
    shape = (pv.shape[0], steps, model.config.num_out_channels, pv.shape[2], pv.shape[3])
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) / (shape[0] * shape[2] * shape[3] * shape[4])


_refs = {}


def references(name, steps, tmp_path_factory):
    """R1 and R2 of the case's inputs, computed once -> dict(preds, g, r1, r2, terms)"""
    key = (name, steps)
    if key not in _refs:
        model, pv, t, _ = exported(name, tmp_path_factory)
        g = cotangents(model, pv, steps, 11)
        preds, d_pv2, d_t2 = ref_mod.r2(model, pv, t, g)
        d_pv1, d_t1, terms = ref_mod.r1(model, pv, t, preds, g)
        _refs[key] = dict(preds=preds, g=g, r1=(d_pv1, d_t1), r2=(d_pv2, d_t2), terms=terms)
    return _refs[key]


def c_layout(x):
    return x.transpose(0, 1).contiguous()


def raw(plan, pv, t, preds, g, steps, d_pv, d_t, scale=0.0):
    """the C call on C-layout tensors (None -> NULL)"""
    p = lambda x: None if x is None else x.data_ptr()      # noqa: E731
    return plan._lib.scot_plan_rollout_vjp(plan._h, p(pv), p(t), p(preds), p(g), int(steps), p(d_pv), p(d_t), float(scale), None)


# ------------------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("name,steps", CASES)
def test_rollout_vjp_equals_the_python_chain(emu, tmp_path_factory, name, steps):
    """R1 bit for bit, R2 within the association bound; scratch poisoned with NaN bytes first; the plan's rollout gives the step inputs"""
    model, pv, t, path = exported(name, tmp_path_factory)
    cout = model.config.num_out_channels
    r = references(name, steps, tmp_path_factory)
    assert all(torch.isfinite(x).all() for x in r["r1"] + r["r2"]) and float(r["r1"][1].abs().max()) > 0.0
    ref_mod.assert_r2_within_bound(r["r1"], r["r2"], r["terms"], cout, label=f"{name} x{steps}")
    plan = Plan.load(path)
    plan.poison(0xFF)
    preds = plan.rollout(pv, t, steps)
    assert torch.equal(preds, r["preds"])
    plan.poison(0xFF)
    before = issued(plan)
    d_pv, d_t = plan.rollout_vjp(pv, t, preds, r["g"])
    assert issued(plan) > before
    assert torch.equal(d_pv, r["r1"][0])
    assert torch.equal(d_t, r["r1"][1])
    assert plan.grad_status() == (0, plan.describe_adjoint()["grad_scale_exponent"])
    if name == "c96":
        assert int(model._engine.grad_overflow) == 0
    if name == "c96":      # (a second emulated sweep of the wide model would only cost time)
        plan.free()
        return
    # raw addresses take the C layout, and need `out` and `steps`
    d_pv2, d_t2 = torch.full_like(d_pv, 7.0), torch.full_like(d_t, 7.0)
    with pytest.raises(ValueError, match="out"):
        plan.rollout_vjp(pv.data_ptr(), t.data_ptr(), preds.data_ptr(), r["g"].data_ptr())
    cp, cg = c_layout(preds), c_layout(r["g"])
    plan.rollout_vjp(pv.data_ptr(), t.data_ptr(), cp.data_ptr(), cg.data_ptr(), out=(d_pv2, d_t2), steps=steps)
    assert torch.equal(d_pv2, d_pv) and torch.equal(d_t2, d_t)
    plan.free()


def test_one_step_equals_run_and_vjp(emu, tmp_path_factory):
    model, pv, t, path = exported("small", tmp_path_factory)
    g = cotangents(model, pv, 1, 5)
    plan = Plan.load(path)
    plan.poison(0xFF)
    pred = plan.run(pv, t)
    want = plan.vjp(g[:, 0].contiguous())
    plan.poison(0xFF)
    got = plan.rollout_vjp(pv, t, pred.unsqueeze(1), g)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # ... and leaves the plan un-armed: it needs no run before it and keeps none for a vjp after it
    before = issued(plan)
    assert plan._lib.scot_plan_vjp(plan._h, g.data_ptr(), got[0].data_ptr(), got[1].data_ptr(), 0.0, None) == -1 and issued(plan) == before
    plan.run(pv, t)
    plan.rollout_vjp(pv, t, pred.unsqueeze(1), g)
    assert plan._lib.scot_plan_vjp(plan._h, g.data_ptr(), got[0].data_ptr(), got[1].data_ptr(), 0.0, None) == -1
    plan.free()


def test_no_state_leaks_between_calls(emu, tmp_path_factory):
    """first inputs, other inputs with another cotangent, the first again: the third result is the first"""
    model, pv, t, path = exported("resid", tmp_path_factory)
    r = references("resid", 3, tmp_path_factory)
    pv2, t2 = other_inputs(pv, t)
    g2 = cotangents(model, pv, 3, 12)
    plan = Plan.load(path)
    first = plan.rollout_vjp(pv, t, r["preds"], r["g"])
    preds2 = plan.rollout(pv2, t2, 3)
    second = plan.rollout_vjp(pv2, t2, preds2, g2)
    d_pv2, d_t2, _ = ref_mod.r1(model, pv2, t2, preds2, g2)
    assert torch.equal(second[0], d_pv2) and torch.equal(second[1], d_t2) and not torch.equal(second[0], first[0])
    again = plan.rollout_vjp(pv, t, r["preds"], r["g"])
    assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    assert torch.equal(first[0], r["r1"][0]) and torch.equal(first[1], r["r1"][1])
    plan.free()


def test_only_step_0_observed_is_the_single_step_vjp(emu, tmp_path_factory):
    """a cotangent that is zero on every step but the first: steps 2 and 1 hand zeros on, and what is left is the vjp of step 0 at
    time / steps"""
    model, pv, t, path = exported("resid", tmp_path_factory)
    r = references("resid", 3, tmp_path_factory)
    g = torch.zeros_like(r["g"])
    g[:, 0] = r["g"][:, 0]
    plan = Plan.load(path)
    d_pv, d_t = plan.rollout_vjp(pv, t, r["preds"], g)
    t_step = t / 3
    plan.run(pv, t_step)
    want = plan.vjp(g[:, 0].contiguous())
    assert torch.equal(d_pv, want[0]) and torch.equal(d_t, want[1] / 3) and float(d_pv.abs().max()) > 0.0
    plan.free()


def test_runtime_owned_holder(emu, tmp_path_factory):
    """d_pixel_values = NULL: the carry lives in a buffer of the runtime's, allocated at the first such call and described from then on"""
    model, pv, t, path = exported("resid", tmp_path_factory)
    r = references("resid", 3, tmp_path_factory)
    plan = Plan.load(path)
    held = plan.describe()["device_bytes"]
    d_t = torch.full_like(t, 7.0)
    plan.poison(0xFF)
    plan.rollout_vjp(pv, t, r["preds"], r["g"], out=(None, d_t))
    assert torch.equal(d_t, r["r1"][1])
    assert plan.describe()["device_bytes"] == held + pv.numel() * 4
    plan.rollout_vjp(pv, t, r["preds"], r["g"], out=(None, d_t))
    assert plan.describe()["device_bytes"] == held + pv.numel() * 4 and torch.equal(d_t, r["r1"][1])
    # d_time = NULL
    d_pv = torch.full_like(pv, 7.0)
    plan.rollout_vjp(pv, t, r["preds"], r["g"], out=(d_pv, None))
    assert torch.equal(d_pv, r["r1"][0])
    plan.free()


# ------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(emu, tmp_path_factory):
    model, pv, t, path = exported("small", tmp_path_factory)
    r = references("small", 3, tmp_path_factory)
    preds, g = c_layout(r["preds"]), c_layout(r["g"])
    d_pv, d_t = torch.full_like(pv, 7.0), torch.full_like(t, 7.0)

    def refused(plan, status, args=None, steps=3, out=(d_pv, d_t), scale=0.0):
        args = (pv, t, preds, g) if args is None else args
        before, armed = issued(plan), plan.describe()["device_bytes"]
        assert raw(plan, *args, steps, *out, scale) == status
        assert issued(plan) == before and plan.describe()["device_bytes"] == armed      # nothing launched, nothing allocated
        assert float(d_pv.min()) == 7.0 and float(d_t.min()) == 7.0                     # ... and nothing written
    plan = Plan.load(path)
    refused(plan, -1, steps=0)
    refused(plan, -1, steps=-2)
    for hole in range(4):      # a NULL required pointer
        refused(plan, -1, args=tuple(None if i == hole else x for i, x in enumerate((pv, t, preds, g))))
    for scale in (3.0, -2.0, float("nan"), float("inf"), 2.0, 0.5):      # the rules of scot_plan_vjp: this backward runs unscaled
        refused(plan, -1, scale=scale)
    # a refusal leaves the state as it was: a run stays armed for its vjp
    pred = plan.run(pv, t)
    refused(plan, -1, steps=0)
    want = ref_mod.r1(model, pv, t, pred.unsqueeze(1), r["g"][:, :1])
    got = plan.vjp(r["g"][:, 0].contiguous())
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert raw(plan, pv, t, preds, g, 3, d_pv, d_t, 1.0) == 0 and torch.equal(d_pv, r["r1"][0]) and torch.equal(d_t, r["r1"][1])
    plan.free()
    d_pv.fill_(7.0), d_t.fill_(7.0)
    # a format-1 plan has no adjoint
    plan = Plan.load(model.export_plan(pv, time=t))
    refused(plan, -3)
    plan.free()
    # exported without the pixel_values adjoint: no carry, so one step at most and no d_pixel_values
    _, _, _, path_t = exported("small", tmp_path_factory, ("time",))
    plan = Plan.load(path_t)
    refused(plan, -1, out=(None, d_t))                 # steps > 1
    refused(plan, -1, steps=1)                         # d_pixel_values
    assert raw(plan, pv, t, preds, g, 1, None, d_t) == 0
    plan.run(pv, t)
    assert torch.equal(d_t, plan.vjp(r["g"][:, 0].contiguous())[1])
    plan.free()
    d_t.fill_(7.0)
    # exported without the time adjoint
    _, _, _, path_pv = exported("small", tmp_path_factory, ("pixel_values",))
    plan = Plan.load(path_pv)
    refused(plan, -1)                                  # d_time
    assert raw(plan, pv, t, preds, g, 3, d_pv, None) == 0 and torch.equal(d_pv, r["r1"][0])
    plan.free()
    d_pv.fill_(7.0)
    # Cout > Cin
    from scOT.model import ScOT
    cfg = ScOTConfig(**dict(SMALL, num_channels=3, channel_slice_list_normalized_loss=[0, 1, 3, 4]))
    grow = ScOT(cfg, compute="fp32")
    grow.load_state_dict(synth_state_dict(param_shapes(cfg), "trained"))
    grow.eval()
    for p in grow.parameters():
        p.requires_grad_(False)
    grow._ensure_arena(torch.device("cpu"))
    pv3 = pv[:, :3].contiguous()
    plan = Plan.load(grow.export_plan(pv3, time=t, adjoint=BOTH))
    refused(plan, -1, args=(pv3, t, preds, g), steps=1, out=(None, d_t))
    plan.free()
    # no time input
    nocond = ScOT(ScOTConfig(**dict(SMALL, use_conditioning=False)), compute="fp32").eval()
    for p in nocond.parameters():
        p.requires_grad_(False)
    nocond._ensure_arena(torch.device("cpu"))
    plan = Plan.load(nocond.export_plan(pv, adjoint=("pixel_values",)))
    refused(plan, -3, out=(d_pv, None))
    plan.free()


def test_fp16_grad_scale_argument(emu, tmp_path_factory):
    model, pv, t, path = exported("c96", tmp_path_factory)
    r = references("c96", 2, tmp_path_factory)
    preds, g = c_layout(r["preds"]), c_layout(r["g"])
    d_pv, d_t = torch.empty_like(pv), torch.empty_like(t)
    plan = Plan.load(path)
    for scale in (3.0, -16384.0, 16384.0 * 1.5, 2.0 ** 121):
        before = issued(plan)
        assert raw(plan, pv, t, preds, g, 2, d_pv, d_t, scale) == -1 and issued(plan) == before
    plan.free()


# ------------------------------------------------------------------------------------------------------- overflow is seen
def test_overflow_is_seen_never_clipped(emu, tmp_path_factory):
    """The scale is picked on the Python path alone: doubled from the automatic value until R1 holds a non-finite value.  At that scale
    the plan's gradients have R1's finite / non-finite mask (and its bits where finite) and its counter grows; the same call at the
    automatic scale afterwards is the clean result."""
    model, pv, t, path = exported("c96", tmp_path_factory)
    r = references("c96", 2, tmp_path_factory)
    g = r["g"] * 512.0      # (still clean at the automatic scale — asserted — and a few doublings from binary16's range)
    auto = model._engine.grad_scale_value()
    clean = ref_mod.r1(model, pv, t, r["preds"], g)
    assert torch.isfinite(clean[0]).all() and torch.isfinite(clean[1]).all() and int(model._engine.grad_overflow) == 0
    k, hot, bad = int(auto).bit_length() - 1, None, None
    assert 2.0 ** k == auto
    while k < 60:
        k += 1
        hot, _, _ = build_model("c96", engine_options={"grad_scale": 2 ** k})
        bad = ref_mod.r1(hot, pv, t, r["preds"], g)
        assert hot._engine.grad_scale_value() == 2.0 ** k
        if not (torch.isfinite(bad[0]).all() and torch.isfinite(bad[1]).all()):
            break
    else:
        pytest.fail("mis-chosen case: R1 is still finite at a gradient scale of 2**60")
    grew = int(hot._engine.grad_overflow)
    print(f"\nautomatic scale 2**{int(auto).bit_length() - 1}, overflow at 2**{k}: engine.grad_overflow grew by {grew}")
    assert grew > 0
    plan = Plan.load(path)
    plan.poison(0xFF)
    d_pv, d_t = plan.rollout_vjp(pv, t, r["preds"], g, grad_scale=2.0 ** k)
    for got, want in ((d_pv, bad[0]), (d_t, bad[1])):
        fin = torch.isfinite(want)
        assert torch.equal(torch.isfinite(got), fin) and torch.equal(got[fin], want[fin])
    counted, exponent = plan.grad_status()
    print(f"the plan's un-scale passes counted {counted}")
    assert counted > 0 and exponent == k
    d_pv, d_t = plan.rollout_vjp(pv, t, r["preds"], g)
    assert torch.equal(d_pv, clean[0]) and torch.equal(d_t, clean[1])
    assert plan.grad_status() == (counted, int(auto).bit_length() - 1)
    plan.free()


# ------------------------------------------------------------------------------------------------------- header, table, builds
def test_header_prototypes_and_builds(emu):
    import emu_session
    header = open(os.path.join(ROOT, "include", "scot_plan.h")).read()
    declared = set(re.findall(r"\b(scot_[a-z0-9_]+)\s*\(", header))
    assert NAME in declared and declared == set(scotlib.PLAN_PROTOTYPES)
    assert "`steps` forwards + `steps` backwards" in header      # the stated cost
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert scotlib.PLAN_PROTOTYPES[NAME] == [P, P, P, P, P, I, P, P, F, P]
    for kind in ("bf16", "f16"):
        lib = plan_mod.bind(emu_session.load_emu(kind))
        assert getattr(lib, NAME).argtypes == scotlib.PLAN_PROTOTYPES[NAME]
        assert lib.scot_abi_version() == scotlib.ABI_VERSION == 8
        assert lib.scot_plan_rollout_vjp(None, None, None, None, None, 1, None, None, 0.0, None) == -1
        # the carry kernels are internal: neither list names anything new
        listed = plan_mod.runtime_entry_points(lib) + plan_mod.runtime_entry_points(lib, adjoint=True)
        assert set(listed) <= set(scotlib.PROTOTYPES)


def test_gfx950_builds_export_the_call():
    for kind in ("bf16", "f16"):
        lib = scotlib.load(kind=kind)
        assert getattr(lib, NAME).argtypes == scotlib.PLAN_PROTOTYPES[NAME]
        assert lib.scot_abi_version() == 8
        assert lib.scot_plan_rollout_vjp(None, None, None, None, None, 1, None, None, 0.0, None) == -1


def test_harness_rollout_detach_flag(emu, tmp_path_factory):
    """the default is the reference's (detached: no graph), detach=False carries the graph of every step, and the values are the same"""
    from poseidon_amd import harness
    model, pv, t = build_model("resid")
    a, b = pv.clone().requires_grad_(True), t.clone().requires_grad_(True)
    kept = harness.rollout(model, dict(pixel_values=a, time=b), ar_steps=2, output_all_steps=True).output
    assert not kept.requires_grad
    out = harness.rollout(model, dict(pixel_values=a, time=b), ar_steps=2, output_all_steps=True, detach=False).output
    assert out.requires_grad and torch.equal(out.detach(), kept)
    last = harness.rollout(model, dict(pixel_values=a, time=b), ar_steps=2, detach=False).output
    assert last.requires_grad and torch.equal(last.detach(), kept[:, 1])
    with pytest.raises(ValueError, match="detach"):
        harness.rollout(model, dict(pixel_values=a, time=b), ar_steps=[1, 2], detach=False)
