"""Adjoint plans on the CPU emulation: `ScOT.export_plan(..., adjoint=...)` records the differentiable forward and the frozen-model
backward against libscot_emu.so, the plan runtime of the same library (csrc/plan.hip) replays both lists in plain host memory.

The reference of every comparison is the Python engine through the public API — every parameter frozen, `model.eval()`,
`torch.autograd.grad(out.output, (pixel_values, time), grad_outputs=g)` — and every comparison is bit for bit.  The cotangents have the
magnitude of a mean loss's gradient (O(1 / number of output elements)): what the fp16 gradient scale is chosen for.

"Launches nothing" is read from the emulated runtime's launch log: `scot_plan_emu_issued()` counts every copy, fill and replayed call
the plan runtime has issued (emulated build only; not part of the C ABI)."""
import ctypes
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from plan_support import BOTH, ROOT, SMALL, check_images_stand_alone, emu, frozen_exports, issued, names_of, other_inputs  # noqa: E402,F401
from plan_support import frozen_model as build_model, patched, relocation_beyond_its_buffer, renamed, truncations, word  # noqa: E402
from poseidon_amd import engine as engine_mod, lib as scotlib, plan as plan_mod  # noqa: E402
from poseidon_amd.config import ScOTConfig  # noqa: E402
from poseidon_amd.plan import Plan, PlanExportError  # noqa: E402

NEVER_LISTED = ("scot_wgrad_group", "scot_wgrad_mlp", "scot_colsum", "scot_conv5_wgrad", "scot_dwconv7_wgrad", "scot_adamw_step")
exported = frozen_exports()


def cotangent(model, pv, seed):
    shape = (pv.shape[0], model.config.num_out_channels, pv.shape[2], pv.shape[3])
    n = shape[0] * shape[1] * shape[2] * shape[3]
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) / n


def python_side(model, pv, t, g, wrt=BOTH):
    """-> (prediction, d_pixel_values or None, d_time or None) of the Python engine through ScOT.forward and torch.autograd"""
    a = pv.clone().requires_grad_("pixel_values" in wrt)
    b = t.clone().requires_grad_("time" in wrt)
    out = model(pixel_values=a, time=b).output
    grads = list(torch.autograd.grad(out, [x for x in (a, b) if x.requires_grad], grad_outputs=g))
    return (out.detach().clone(), grads.pop(0) if a.requires_grad else None, grads.pop(0) if b.requires_grad else None)


def raw_vjp(plan, g, d_pv, d_t, scale=0.0):
    return plan._lib.scot_plan_vjp(plan._h, g.data_ptr(), None if d_pv is None else d_pv.data_ptr(), None if d_t is None else d_t.data_ptr(),
                                   float(scale), None)


# ------------------------------------------------------------------------------------------------------- round trip
@pytest.mark.parametrize("name", ["small", "resid", "c96"])
def test_adjoint_round_trip_is_bit_identical(emu, tmp_path_factory, name):
    """prediction and both gradients equal Python's bits for the export inputs, for second inputs with a second cotangent, and for the
    first inputs again; scratch poisoned with NaN bytes before each triple; fp16 at the engine's own gradient scale"""
    model, pv, t, path = exported(name, tmp_path_factory)
    image = open(path, "rb").read()
    assert Plan.header(image)[plan_mod.H_FORMAT] == plan_mod.FORMAT_ADJOINT == 2
    plan = Plan.load(path)
    d, a = plan.describe(), plan.describe_adjoint()
    assert d["format"] == 2 and a["has_adjoint"] == a["d_pixel_values"] == a["d_time"] == 1
    assert a["backward_calls"] > 20 and 0 < a["kept_bytes"] < d["device_bytes"]
    S = model._engine.grad_scale_value()
    assert (S > 1.0) == (name == "c96") and 2.0 ** a["grad_scale_exponent"] == S
    pv2, t2 = other_inputs(pv, t)
    g1, g2 = cotangent(model, pv, 3), cotangent(model, pv, 4)
    refs = [python_side(model, x, tt, g) for x, tt, g in ((pv, t, g1), (pv2, t2, g2))]
    assert all(torch.isfinite(r).all() for ref in refs for r in ref)
    assert not torch.equal(refs[0][1], refs[1][1]) and float(refs[0][2].abs().max()) > 0.0
    for (x, tt, g), ref in zip(((pv, t, g1), (pv2, t2, g2), (pv, t, g1)), (refs[0], refs[1], refs[0])):
        plan.poison(0xFF)
        pred = plan.run(x, tt)
        d_pv, d_t = plan.vjp(g, grad_scale=S if name == "c96" else 0)
        assert torch.equal(pred, ref[0])
        assert torch.equal(d_pv, ref[1])
        assert torch.equal(d_t, ref[2])
    status = plan.grad_status()
    assert status == (0, a["grad_scale_exponent"])
    if name == "c96":
        assert int(model._engine.grad_overflow) == 0
        assert "scot_block_tail_bwd" in names_of(image, "backward")
    plan.free()


# ------------------------------------------------------------------------------------------------------- requests
def test_requests(emu, tmp_path_factory):
    model, pv, t, path_pv = exported("small", tmp_path_factory, ("pixel_values",))
    g = cotangent(model, pv, 3)
    # pixel_values only: no time-gradient call in the image, a d_time request is refused
    image = open(path_pv, "rb").read()
    assert "scot_cln_dtime" not in names_of(image, "backward") + names_of(image, "forward")
    plan = Plan.load(path_pv)
    assert plan.describe_adjoint()["d_pixel_values"] == 1 and plan.describe_adjoint()["d_time"] == 0
    plan.run(pv, t)
    before = issued(plan)
    d_pv, d_t = torch.empty_like(pv), torch.empty_like(t)
    assert raw_vjp(plan, g, d_pv, d_t) == -1 and issued(plan) == before
    got = plan.vjp(g)      # (the refusal did not use the run up)
    ref = python_side(model, pv, t, g, wrt=("pixel_values",))
    assert got[1] is None and torch.equal(got[0], ref[1])
    plan.free()
    # time only
    _, _, _, path_t = exported("small", tmp_path_factory, ("time",))
    assert "scot_cln_dtime" in names_of(open(path_t, "rb").read(), "backward")
    plan = Plan.load(path_t)
    plan.poison(0xFF)
    pred = plan.run(pv, t)
    got = plan.vjp(g)
    ref = python_side(model, pv, t, g, wrt=("time",))
    assert got[0] is None and torch.equal(got[1], ref[2]) and torch.equal(pred, ref[0])
    plan.run(pv, t)
    assert raw_vjp(plan, g, d_pv, None) == -1
    plan.free()
    # the default export is the inference image: format 1, no word of the adjoint format set, and the same bytes with adjoint=()
    default, explicit = model.export_plan(pv, time=t), model.export_plan(pv, time=t, adjoint=())
    assert default == explicit
    h = Plan.header(default)
    assert h[plan_mod.H_FORMAT] == plan_mod.FORMAT == 1 and not any(h[plan_mod.H_NBACKWARD:])
    plan = Plan.load(default)
    assert plan.describe()["format"] == 1 and set(plan.describe_adjoint().values()) == {0}
    assert "scot_cln_bwd" not in names_of(default, "forward")
    plan.free()
    # refusals of the exporter
    from scOT.model import ScOT
    with pytest.raises(PlanExportError, match="adjoint"):
        model.export_plan(pv, time=t, adjoint=("labels",))
    nocond = ScOT(ScOTConfig(**dict(SMALL, use_conditioning=False)), compute="fp32").eval()
    nocond._ensure_arena(torch.device("cpu"))
    with pytest.raises(PlanExportError, match="use_conditioning"):
        nocond.export_plan(pv, adjoint=("time",))


def test_backward_host_side_step_is_named(emu, monkeypatch):
    """a Python step left in the recorded backward aborts the export by name, as one in the forward does"""
    model, pv, t = build_model("small")

    def host_side_step():
        pass
    orig_mark = engine_mod.ScOTEngine.mark

    def mark(self, label):
        if label == "bwd embed":
            self.tdo(host_side_step)
        return orig_mark(self, label)
    monkeypatch.setattr(engine_mod.ScOTEngine, "mark", mark)
    with pytest.raises(PlanExportError, match="backward holds a host-side Python step.*host_side_step"):
        model.export_plan(pv, time=t, adjoint=BOTH)


# ------------------------------------------------------------------------------------------------------- state machine
def test_vjp_state_machine(emu, tmp_path_factory):
    model, pv, t, path = exported("small", tmp_path_factory)
    g = cotangent(model, pv, 3)
    ref = python_side(model, pv, t, g)
    plan = Plan.load(path)
    d_pv, d_t = torch.full_like(pv, 7.0), torch.full_like(t, 7.0)

    def refused(status=-1, scale=0.0):
        before = issued(plan)
        assert raw_vjp(plan, g, d_pv, d_t, scale) == status
        assert issued(plan) == before                                   # nothing was launched
        assert float(d_pv.min()) == 7.0 and float(d_t.min()) == 7.0      # ... and nothing written
    refused()                       # before any run
    plan.run(pv, t)
    before = issued(plan)
    assert raw_vjp(plan, g, d_pv, d_t) == 0 and issued(plan) > before
    assert torch.equal(d_pv, ref[1]) and torch.equal(d_t, ref[2])
    d_pv.fill_(7.0), d_t.fill_(7.0)
    refused()                       # a second vjp
    out = torch.empty(3, *ref[0].shape)
    plan.rollout(pv, t, 3, out=out)
    refused()                       # after a rollout
    plan.run(pv, t)
    plan.poison(0xFF)
    refused()                       # after a poison
    # the gradient scale: a power of two, and 0 or 1 on a plan whose backward runs unscaled
    plan.run(pv, t)
    for scale in (3.0, -2.0, float("nan"), float("inf"), 2.0, 0.5):
        refused(scale=scale)
    assert raw_vjp(plan, g, d_pv, d_t, 1.0) == 0      # (the refusals did not use the run up)
    assert torch.equal(d_pv, ref[1]) and torch.equal(d_t, ref[2])
    assert plan.grad_status() == (0, 0)
    plan.free()
    # a format-1 plan has no adjoint
    plan = Plan.load(model.export_plan(pv, time=t))
    plan.run(pv, t)
    before = issued(plan)
    assert raw_vjp(plan, g, d_pv, d_t) == -3 and issued(plan) == before
    plan.free()


def test_fp16_grad_scale_argument(emu, tmp_path_factory):
    model, pv, t, path = exported("c96", tmp_path_factory)
    g = cotangent(model, pv, 3)
    plan = Plan.load(path)
    plan.run(pv, t)
    d_pv, d_t = torch.empty_like(pv), torch.empty_like(t)
    for scale in (3.0, -16384.0, 16384.0 * 1.5):
        before = issued(plan)
        assert raw_vjp(plan, g, d_pv, d_t, scale) == -1 and issued(plan) == before
    assert raw_vjp(plan, g, d_pv, d_t, 4096.0) == 0 and plan.grad_status() == (0, 12)
    plan.free()


# ------------------------------------------------------------------------------------------------------- refusals at load
def corrupt_images(image):
    """{label: (bytes, expected status)}: the corrupt variants of a good format-2 image"""
    h = Plan.header(image)
    H = plan_mod
    out = truncations(image, (h[H.H_NAMES_OFF], h[H.H_BUFFERS_OFF], h[H.H_ENTRIES_OFF], h[H.H_ARRAYS_OFF], h[H.H_IO_OFF], h[H.H_BACKWARD_OFF],
                              h[H.H_BACKWARD_OFF] + 8 * h[H.H_BACKWARD_WORDS] - 8, h[H.H_ADJ_OFF], h[H.H_ADJ_OFF] + 8 * H.ADJ_WORDS - 8,
                              h[H.H_DATA_OFF]))
    out["backward relocation beyond its buffer"] = (relocation_beyond_its_buffer(image, "backward"), -1)
    w = h[H.H_BACKWARD_OFF]
    out["backward entry renamed to a weight-gradient kernel"] = (renamed(image, word(image, w), "scot_wgrad_group"), -3)
    out["forward entry renamed to a backward-only name"] = (renamed(image, word(image, h[H.H_ENTRIES_OFF]), "scot_cln_bwd"), -3)
    out["backward n_int = 49"] = (patched(image, w + 16, 49), -1)
    out["backward section past the end"] = (patched(image, 8 * H.H_BACKWARD_WORDS, 1 << 31), -1)
    out["gradient in an input buffer"] = (patched(image, h[H.H_ADJ_OFF] + 8 * H.ADJ_DPV, word(image, h[H.H_ADJ_OFF] + 8 * H.ADJ_COT)), -1)
    out["format 3"] = (patched(image, 8 * H.H_FORMAT, 3), -3)
    return out


def test_load_refusals(emu, tmp_path_factory):
    model, pv, t, path = exported("small", tmp_path_factory)
    image = open(path, "rb").read()
    assert "scot_cln_bwd" not in plan_mod.runtime_entry_points(emu) and "scot_cln_bwd" in plan_mod.runtime_entry_points(emu, adjoint=True)
    lib = plan_mod.bind(emu)
    handle = ctypes.c_void_p()
    assert plan_mod.load_raw(lib, image, handle) == 0 and handle.value
    assert lib.scot_plan_free(handle) == 0
    g, out = cotangent(model, pv, 3), torch.empty_like(pv)
    for label, (bad, status) in corrupt_images(image).items():
        handle = ctypes.c_void_p(0xdead)
        assert plan_mod.load_raw(lib, bad, handle) == status, label
        assert not handle.value, label
        assert lib.scot_plan_vjp(handle, g.data_ptr(), out.data_ptr(), None, 0.0, None) == -1, label
        assert lib.scot_plan_describe_adjoint(handle, (ctypes.c_longlong * 8)()) == -1


def test_stand_alone_image_check_under_sanitizers(emu, tmp_path_factory, tmp_path):
    """tools/plan_image_check.cc: the validator alone, built with the address and undefined-behaviour sanitizers, over a good format-2
    image, a good format-1 image and the corrupt variants — a child process on the CPU, nothing preloaded."""
    model, pv, t, path = exported("small", tmp_path_factory)
    image = open(path, "rb").read()
    check_images_stand_alone(tmp_path, {"good": (image, 0), "good format 1": (model.export_plan(pv, time=t), 0), **corrupt_images(image)})


# ------------------------------------------------------------------------------------------------------- overflow is seen
def test_overflow_is_seen_never_clipped(emu, tmp_path_factory):
    """The scale is picked on the Python path alone: doubled from the automatic value until Python's input gradient holds a non-finite
    value.  At that scale the plan's gradients have Python's finite / non-finite mask and Python's bits where finite, its counter grows
    by what engine.grad_overflow grew, and a run + vjp at the automatic scale afterwards is the clean result again."""
    model, pv, t, path = exported("c96", tmp_path_factory)
    g = cotangent(model, pv, 3) * 512.0      # (still clean at the automatic scale — asserted — and a few doublings from binary16's range)
    auto = model._engine.grad_scale_value()
    clean = python_side(model, pv, t, g)
    assert all(torch.isfinite(x).all() for x in clean) and int(model._engine.grad_overflow) == 0
    k, hot, bad = int(auto).bit_length() - 1, None, None
    assert 2.0 ** k == auto
    while k < 60:
        k += 1
        hot, _, _ = build_model("c96", engine_options={"grad_scale": 2 ** k})
        bad = python_side(hot, pv, t, g)
        assert hot._engine.grad_scale_value() == 2.0 ** k
        if not (torch.isfinite(bad[1]).all() and torch.isfinite(bad[2]).all()):
            break
    else:
        pytest.fail("mis-chosen case: Python's input gradients are still finite at a gradient scale of 2**60")
    grew = int(hot._engine.grad_overflow)
    print(f"\nautomatic scale 2**{int(auto).bit_length() - 1}, overflow at 2**{k}: engine.grad_overflow grew by {grew}")
    assert grew > 0
    plan = Plan.load(path)
    plan.poison(0xFF)
    plan.run(pv, t)
    d_pv, d_t = plan.vjp(g, grad_scale=2.0 ** k)
    for got, ref in ((d_pv, bad[1]), (d_t, bad[2])):
        fin = torch.isfinite(ref)
        assert torch.equal(torch.isfinite(got), fin) and torch.equal(got[fin], ref[fin])
    assert plan.grad_status() == (grew, k)
    plan.run(pv, t)
    d_pv, d_t = plan.vjp(g, grad_scale=auto)
    assert torch.equal(d_pv, clean[1]) and torch.equal(d_t, clean[2])
    assert plan.grad_status() == (grew, int(auto).bit_length() - 1)
    plan.free()


# ------------------------------------------------------------------------------------------------------- header, table, lists
def test_header_prototypes_and_lists(emu):
    import emu_session
    header = open(os.path.join(ROOT, "include", "scot_plan.h")).read()
    declared = set(re.findall(r"\b(scot_[a-z0-9_]+)\s*\(", header))
    new = {"scot_plan_describe_adjoint", "scot_plan_vjp", "scot_plan_grad_status", "scot_plan_adjoint_entry_point"}
    assert declared == set(scotlib.PLAN_PROTOTYPES) and new <= declared
    assert scotlib.PLAN_PROTOTYPES["scot_plan_vjp"][4] is ctypes.c_float
    for kind in ("bf16", "f16"):
        lib = plan_mod.bind(emu_session.load_emu(kind))
        for name in new:
            assert getattr(lib, name) is not None
        assert lib.scot_abi_version() == scotlib.ABI_VERSION == 8
        fwd, bwd = plan_mod.runtime_entry_points(lib), plan_mod.runtime_entry_points(lib, adjoint=True)
        assert len(bwd) == len(set(bwd)) > 10 and set(bwd) <= set(scotlib.PROTOTYPES)
        assert all(scotlib.PROTOTYPES[n][-1] is ctypes.c_void_p for n in bwd)      # the stream, last
        assert not set(NEVER_LISTED) & (set(fwd) | set(bwd))
        assert {"scot_cln_dtime", "scot_cln_bwd", "scot_window_attn_bwd_rep", "scot_scale_inplace_dev"} <= set(bwd) - set(fwd)
        assert lib.scot_plan_adjoint_entry_point(-1) is None and lib.scot_plan_adjoint_entry_point(len(bwd)) is None


def test_gfx950_builds_export_the_adjoint_calls():
    for kind in ("bf16", "f16"):
        lib = scotlib.load(kind=kind)
        for name in ("scot_plan_describe_adjoint", "scot_plan_vjp", "scot_plan_grad_status", "scot_plan_adjoint_entry_point"):
            assert getattr(lib, name).argtypes == scotlib.PLAN_PROTOTYPES[name]
        assert lib.scot_abi_version() == 8
        assert lib.scot_plan_vjp(None, None, None, None, 0.0, None) == -1
        assert lib.scot_plan_adjoint_entry_point(0) == b"scot_gemm"
        assert not hasattr(lib, "scot_plan_emu_issued")
