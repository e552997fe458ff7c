"""What the two resized-plan test modules share (tests/test_plan_resize_emu_cpu.py on the CPU emulation, tests/test_plan_resize_gpu.py on
the MI355X): plans exported with `resize=True` at a resolution r other than config.image_size — one scot_spectral_resize in front of the
engine's forward and one behind it — against the Python model with `fused_resize = True`, bit for bit.  A plain module; the callers pass
an `Env`: the device, how to build a model there, and the library context of a loaded plan (error_sums_cases.Ctx)."""
import ctypes

import pytest
import torch

import error_sums_cases as E
import plan_eval_cases as PE
import plan_masked_cases as PM
import plan_rollout_reference as RR
from plan_support import CFG_ROLL, SMALL, WIDE, entry_records, names_of, patched, relocation_beyond_its_buffer, renamed, truncations, word
from poseidon_amd import harness, plan as plan_mod
from poseidon_amd.plan import Plan, PlanExportError
from poseidon_amd.synth import synth_inputs

MODELS = {"small": (SMALL, "fp32", 2), "roll": (CFG_ROLL, "fp32", 2), "c96": (WIDE, "fp16", 1)}
RESIZE = "scot_spectral_resize"


class Env:
    """device: where the tensors live; build(name) -> a ScOT of MODELS[name] there, synthetic trained weights, eval mode; lib: the
    bfloat16 build of the library (the fp32 models' own); stream / sync: the stream handle and the wait; optimizer(model) -> a
    FusedAdamW over it"""

    def __init__(self, device, build, lib, optimizer, stream=lambda: None, sync=lambda: None):
        self.device, self.build, self.lib, self.optimizer, self.stream, self.sync = device, build, lib, optimizer, stream, sync

    def ctx(self, plan):
        return E.Ctx(plan._lib, self.device, self.stream, self.sync)

    def model(self, name, frozen=False):
        model = self.build(name)
        model.fused_resize = True
        for p in model.parameters() if frozen else ():
            p.requires_grad_(False)
        return model

    def inputs(self, name, r):
        kw, _, B = MODELS[name]
        return tuple(x.to(self.device).contiguous() for x in synth_inputs(B, kw["num_channels"], kw["num_out_channels"], r, "smooth"))

    def other(self, pv, t):
        g = torch.Generator().manual_seed(7)
        return (pv.flip(0).flip(3) * 0.5 + 0.1 * torch.randn(pv.shape, generator=g).to(pv.device)).contiguous(), (t * 0.37 + 0.05)


def own(model, pv, t):
    with torch.no_grad():
        return model(pv, time=t).output


def check_run(env, r):
    """D1"""
    model = env.model("small")
    pv, t, _ = env.inputs("small", r)
    image = model.export_plan(pv, time=t, resize=True)
    assert Plan.header(image)[plan_mod.H_FORMAT] == 1
    names = names_of(image, "forward")
    assert names[0] == RESIZE and names[-1] == RESIZE and names.count(RESIZE) == 2
    plan = Plan.load(image)
    d = plan.describe()
    assert (d["batch"], d["channels"], d["height"], d["width"], d["out_channels"]) == (2, 4, r, r, 4)
    assert d["pixel_values_bytes"] == 2 * 4 * r * r * 4 and plan.describe_resize() == (1, 32, r, 2)
    pv2, t2 = env.other(pv, t)
    for a, b in ((pv, t), (pv2, t2), (pv, t)):
        plan.poison(0xFF)
        got, want = plan.run(a, b), own(model, a, b)
        assert tuple(got.shape) == (2, 4, r, r) and torch.isfinite(got).all() and torch.equal(got, want)
    assert not torch.equal(own(model, pv, t), own(model, pv2, t2))
    plan.free()
    return image


def check_rollout_and_evaluate(env, r=24):
    """D2"""
    model = env.model("roll")
    pv, t, _ = env.inputs("roll", r)
    plan = Plan.load(model.export_plan(pv, time=t, resize=True))
    assert plan.describe_resize() == (1, 16, r, 2)
    plan.poison(0xFF)
    got = plan.rollout(pv, t, 3)
    with torch.no_grad():
        want = harness.rollout(model, dict(pixel_values=pv, time=t), ar_steps=3, output_all_steps=True).output
    assert tuple(got.shape) == (2, 3, 3, r, r) and torch.equal(got, want)
    ctx = env.ctx(plan)
    PE.check_evaluate(plan, ctx, pv, t, 3, [0, 1, 3])
    PM.check_evaluate_masked(plan, ctx, pv, t, 3, [0, 1, 3], PM.batch_mask("element", 2, 3, r, r))
    plan.free()


def check_adjoint(env, r=48):
    """D3"""
    model = env.model("small", frozen=True)
    pv, t, _ = env.inputs("small", r)
    image = model.export_plan(pv, time=t, resize=True, adjoint=("pixel_values", "time"))
    assert Plan.header(image)[plan_mod.H_FORMAT] == 2
    back = names_of(image, "backward")
    assert back[0] == RESIZE and back[-1] == RESIZE and back.count(RESIZE) == 2
    plan = Plan.load(image)
    assert plan.describe_resize() == (1, 32, r, 4)
    a, b = pv.clone().requires_grad_(True), t.clone().requires_grad_(True)
    out = model(a, time=b).output
    assert out.shape[-1] == r and out.shape[-2] == r      # (the prediction comes back at the input's resolution under autograd too)
    gen = torch.Generator().manual_seed(5)
    g = (torch.randn(out.shape, generator=gen) / out.numel()).to(env.device)
    want = torch.autograd.grad(out, (a, b), g)
    plan.poison(0xFF)
    assert torch.equal(plan.run(pv, t), out.detach())
    got = plan.vjp(g)
    for name, x, y in zip(("d_pixel_values", "d_time"), got, want):
        assert torch.isfinite(x).all() and float(x.abs().max()) > 0 and torch.equal(x, y), name
    assert tuple(got[0].shape) == tuple(pv.shape)
    # the rollout's adjoint: the chain of single-step gradients, each through both resamplings
    steps = 2
    preds = plan.rollout(pv, t, steps)
    d_preds = (torch.randn(preds.shape, generator=gen) / preds[:, 0].numel()).to(env.device)
    d_pv, d_t, _ = RR.r1(model, pv, t, preds, d_preds)
    plan.poison(0xFF)
    got = plan.rollout_vjp(pv, t, preds, d_preds)
    assert torch.equal(got[0], d_pv) and torch.equal(got[1], d_t)
    plan.free()


def check_two_streams(env, r=16):
    """D4"""
    model = env.model("small")
    pv, t, _ = env.inputs("small", r)
    one, two = model.export_plan(pv, time=t, resize=True), model.export_plan(pv, time=t, resize=True, streams=2)
    assert Plan.header(two)[plan_mod.H_FORMAT] == 5
    handle = ctypes.c_void_p()
    lib = plan_mod.bind(env.lib)
    assert plan_mod.load_raw(lib, two, handle) == 0 and handle.value and lib.scot_plan_free(handle) == 0      # validates and loads
    every = names_of(two, "forward")
    assert plan_mod.RECORD in every and plan_mod.WAIT in every
    # in front of the first fork and behind the last join (the engine's forward joins its side stream itself), both on stream 0
    assert every[0] == RESIZE and every[-1] == RESIZE and every.count(RESIZE) == 2
    for i, (off, _, ni) in enumerate(entry_records(two, "forward")):
        if every[i] == RESIZE:
            assert [word(two, off + 32 + 16 * k + 8) for k in range(ni) if word(two, off + 32 + 16 * k) & 0xFF == plan_mod.ARG_STREAM] == [0]
    p1, p2 = Plan.load(one), Plan.load(two)
    assert p2.describe_streams()["streams"] == 2 and p2.describe_resize() == (1, 32, r, 2)
    pv2, t2 = env.other(pv, t)
    for a, b in ((pv, t), (pv2, t2)):
        p1.poison(0xFF)
        p2.poison(0xFF)
        assert torch.equal(p1.run(a, b), p2.run(a, b))
    p1.free()
    p2.free()


def corrupt_images(image):
    """{label: (bytes, expected status)}: the corrupt variants of a good resized image"""
    H = plan_mod
    h = Plan.header(image)
    out = truncations(image, (h[H.H_NAMES_OFF], h[H.H_BUFFERS_OFF], h[H.H_ENTRIES_OFF], h[H.H_ARRAYS_OFF], h[H.H_IO_OFF], h[H.H_DATA_OFF]))
    out["relocation beyond its buffer"] = (relocation_beyond_its_buffer(image, "forward"), -1)      # (of the first resize entry)
    out["resize entry renamed to an unlisted name"] = (renamed(image, 0, "scot_spectral_apply"), -3)
    out["n_int = 49"] = (patched(image, h[H.H_ENTRIES_OFF] + 16, 49), -1)
    out["wrong ABI"] = (patched(image, 8 * H.H_ABI, h[H.H_ABI] + 1), -3)
    return out


def check_refusals(env):
    """D5 -> a good resized image"""
    model = env.model("small")
    pv, t, lab = env.inputs("small", 16)
    with pytest.raises(PlanExportError, match="config.image_size"):
        model.export_plan(pv, time=t)
    with pytest.raises(PlanExportError, match="config.image_size"):
        model.export_plan(pv, time=t, resize=False)
    with pytest.raises(PlanExportError, match="image_size"):
        model.export_plan(pv, time=t, labels=lab, train=env.optimizer(model), resize=True)
    with pytest.raises(PlanExportError, match="square"):
        model.export_plan(pv[:, :, :, :12].contiguous(), time=t, resize=True)
    native = env.inputs("small", 32)
    assert model.export_plan(native[0], time=native[1], resize=True) == model.export_plan(native[0], time=native[1])
    image = model.export_plan(pv, time=t, resize=True)
    assert names_of(image, "forward")[0] == RESIZE      # (name 0 of the image's table: what corrupt_images renames)
    lib = plan_mod.bind(env.lib)
    for label, (bad, status) in corrupt_images(image).items():
        handle = ctypes.c_void_p(0xdead)
        assert plan_mod.load_raw(lib, bad, handle) == status, label
        assert not handle.value, label
    plan = Plan.load(image)
    with pytest.raises(ValueError):
        plan.run(native[0], native[1])      # the plan takes tensors at r
    plan.free()
    plain = Plan.load(model.export_plan(native[0], time=native[1]))
    assert plain.describe_resize() == (0, 32, 32, 0)
    plain.free()
    return image
