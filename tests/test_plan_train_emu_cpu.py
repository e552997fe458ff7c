"""Training plans on the CPU emulation: `ScOT.export_plan(..., labels=..., train=optimizer)` records one optimizer step against
libscot_emu.so, and the plan runtime of the same library (csrc/plan.hip) replays it in plain host memory.

The reference of every comparison is the Python loop in the same process,

    opt.zero_grad(overlap=True); out = model(pv_k, time=t_k, labels=y_k); out.loss.backward(); <set the groups' lr>; opt.step()

On the emulator the same calls run in the same order, so every comparison is bit for bit.  Each step has its own batch and its own
learning rate per group: a stale input copy or an unpatched lr shows.  "Launches nothing" is read from `scot_plan_emu_issued()`."""
import ctypes
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from plan_support import ROOT, SMALL, WIDE, check_images_stand_alone, emu, frozen_model, issued, names_of, patched  # noqa: E402,F401
from plan_support import relocation_beyond_its_buffer, renamed, synth_model, word  # noqa: E402
from poseidon_amd import lib as scotlib, plan as plan_mod  # noqa: E402
from poseidon_amd.config import ScOTConfig  # noqa: E402
from poseidon_amd.plan import Plan, PlanExportError  # noqa: E402
from poseidon_amd.synth import synth_inputs  # noqa: E402

H = plan_mod
MODELS = {"small": (SMALL, "fp32", 2), "c96": (WIDE, "fp16", 1), "small16": (SMALL, "fp16", 2)}
OPTIMIZER_ONLY = ("scot_wgrad_group", "scot_wgrad_mlp", "scot_adamw_step", "scot_optim_finish")
NEW_CALLS = {"scot_plan_describe_training", "scot_plan_loss", "scot_plan_train_step", "scot_plan_train_status", "scot_plan_snapshot",
             "scot_plan_training_entry_point"}
STATE = ("arena", "exp_avg", "exp_avg_sq", "step_state", "scale_state")


def build_model(name, **opt_kw):
    """-> (model in training mode with every parameter trainable, its FusedAdamW)"""
    import emu_session
    kw, compute, _ = MODELS[name]
    model = synth_model(ScOTConfig(**kw), compute, train=True)
    opt = emu_session.fused_adamw(model, **dict(dict(lr=1e-3, weight_decay=0.01, max_grad_norm=5.0), **opt_kw))
    return model, opt


def batch(name, k):
    """batch k: (pixel_values, time, labels), all different from batch 0"""
    kw, _, B = MODELS[name]
    pv, t, y = synth_inputs(B, kw["num_channels"], kw["num_out_channels"], kw["image_size"], "smooth")
    if k:
        g = torch.Generator().manual_seed(100 + k)
        pv = pv.roll(k, 3) * (1.0 - 0.1 * k) + 0.05 * torch.randn(pv.shape, generator=g)
        y = y.roll(k, 2) + 0.05 * torch.randn(y.shape, generator=g)
        t = t * (1.0 - 0.2 * k) + 0.03 * k
    return pv.contiguous(), t.contiguous(), y.contiguous()


def rates(opt, k):
    return [1e-3 * (1.0 + 0.5 * k) / (1.0 + g) for g in range(len(opt.param_groups))]


def python_step(model, opt, b, lr):
    opt.zero_grad(overlap=True)
    out = model(b[0], time=b[1], labels=b[2])
    out.loss.backward()
    for g, r in zip(opt.param_groups, lr):
        g["lr"] = r
    opt.step()
    return out.loss.detach().reshape(1).clone()


def python_state(model, opt):
    eng = model._engine
    st = dict(arena=model._arena.data, exp_avg=opt.exp_avg, exp_avg_sq=opt.exp_avg_sq, step_state=opt._step_state)
    if eng.scale_state is not None:
        st["scale_state"] = eng.scale_state
    return st


def assert_state_equal(image, model, opt, label=""):
    got, ref = plan_mod.training_state(image), python_state(model, opt)
    for k in STATE:
        assert (k in got) == (k in ref), (label, k)
        if k in ref:
            assert torch.equal(got[k], ref[k]), (label, k)


_cache = {}


def exported(name):
    """one export per configuration for the whole module -> (image, arena and moments as they were when it was made)"""
    if name not in _cache:
        model, opt = build_model(name)
        pv, t, y = batch(name, 0)
        before = [x.clone() for x in (model._arena.data, opt.exp_avg, opt._step_state)]
        image = model.export_plan(pv, time=t, labels=y, train=opt)
        # the export's recording run IS a step on the model's tensors: it must leave the model and the optimizer as they were
        assert all(torch.equal(a, b) for a, b in zip(before, (model._arena.data, opt.exp_avg, opt._step_state))) and opt.step_count == 0
        assert float(model._arena.grad.abs().max()) == 0.0
        _cache[name] = image
    return _cache[name]


# ------------------------------------------------------------------------------------------------------- steps
@pytest.mark.parametrize("name,steps", [("small", 4), ("c96", 2)])
def test_steps_are_bit_identical(emu, name, steps):
    image = exported(name)
    h = Plan.header(image)
    assert h[H.H_FORMAT] == plan_mod.FORMAT_TRAINING == 4 and not any(h[H.H_NBACKWARD:H.H_TRAIN_OFF]) and h[H.H_TRAIN_OFF]
    model, opt = build_model(name)
    plan = Plan.load(image)
    d, tr = plan.describe(), plan.describe_training()
    assert d["format"] == 4 and tr["has_training"] == 1 and tr["groups"] == len(opt.param_groups) and tr["arena_floats"] == model._arena.size
    assert tr["dynamic_scale"] == (name == "c96") and tr["step_calls"] > d["calls"] and 0 < tr["kept_bytes"] < d["device_bytes"]
    assert set(plan.describe_adjoint().values()) == {0}
    # the loss alone: Python's bits, and no state buffer written
    b = batch(name, 1)
    plan.poison(0xFF)
    loss, pred = plan.loss(*b)
    out = model(b[0], time=b[1], labels=b[2])
    assert torch.equal(loss, out.loss.detach().reshape(1)) and torch.equal(pred, out.output.detach())
    assert plan.snapshot(image) == image
    del out
    if name == "c96":
        assert "scot_block_tail_bwd" in names_of(image, 1) and "scot_wgrad_mlp" in names_of(image, 1)
    for k in range(steps):
        b, lr = batch(name, k), rates(opt, k)
        plan.poison(0xFF)
        ref = python_step(model, opt, b, lr)
        got = plan.train_step(*b, lr)
        assert torch.isfinite(ref).all() and torch.equal(got, ref), k
        assert_state_equal(plan.snapshot(image), model, opt, f"step {k}")
    st = plan.train_status()
    assert (st["applied"], st["skipped"], st["nonfinite"]) == (steps, 0, 0)
    assert st["grad_norm"] == float(opt.last_grad_norm) and st["clip_coef"] == float(opt._clip[0])
    assert st["grad_scale"] == model._engine.grad_scale_value()
    # the plan's inference forward sees the trained weights: the 16-bit copies are current
    model.eval()
    b = batch(name, 1)
    with torch.no_grad():
        ref = model(b[0], time=b[1]).output
    assert torch.equal(plan.run(b[0], b[1]), ref)
    plan.free()


def test_skipped_steps_follow_python(emu):
    """gradient scale 2^30 before the export: every backward overflows until the optimizer has halved the scale far enough"""
    import overflow_sweep as osw
    name = "small16"
    model, opt = build_model(name)
    b0 = batch(name, 0)
    model(b0[0], time=b0[1], labels=b0[2]).loss.backward()      # (the first training forward picks the automatic scale)
    opt.zero_grad()
    osw.set_scale(model._engine, 30)
    image = model.export_plan(*b0[:1], time=b0[1], labels=b0[2], train=opt)
    assert float(plan_mod.training_state(image)["scale_state"][0]) == 2.0 ** 30
    plan = Plan.load(image)
    history, prev = [], image
    while opt.applied_steps() < 2:
        k = len(history)
        assert k < 40, history
        b, lr = batch(name, k % 4), rates(opt, k % 4)
        ref = python_step(model, opt, b, lr)
        got = plan.train_step(*b, lr)
        snap = plan.snapshot(image)
        assert torch.equal(got, ref)
        assert_state_equal(snap, model, opt, f"step {k}")
        skipped = int(opt._clip[2]) == 1
        if skipped:      # parameters, moments and 16-bit copies untouched; the scale halved
            a, c = plan_mod.training_state(prev), plan_mod.training_state(snap)
            assert all(torch.equal(a[x], c[x]) for x in ("arena", "exp_avg", "exp_avg_sq", "shadow"))
            assert float(c["scale_state"][0]) == 0.5 * float(a["scale_state"][0])
        history.append(skipped)
        prev = snap
    st = plan.train_status()
    assert st["skipped"] == opt.skipped_steps() == sum(history) >= 1 and st["applied"] == 2
    assert st["nonfinite"] == int(model._engine.grad_overflow) > 0
    # the fp16 state back in Python: scale, non-finite counter, clock and moments, and the next step is the plan's
    model2, opt2 = build_model(name)
    plan_mod.load_training_state(prev, model2, opt2)
    assert torch.equal(model2._engine.scale_state, model._engine.scale_state)
    assert int(model2._engine.grad_overflow) == int(model._engine.grad_overflow)
    assert (opt2.applied_steps(), opt2.skipped_steps()) == (opt.applied_steps(), opt.skipped_steps())
    b, lr = batch(name, 1), rates(opt, 1)
    assert torch.equal(python_step(model2, opt2, b, lr), plan.train_step(*b, lr))
    assert_state_equal(plan.snapshot(image), model2, opt2, "continued in Python")
    plan.free()
    # an image of another compute mode is refused, whichever way round
    fp32_model, _ = build_model("small")
    with pytest.raises(ValueError, match="compute mode"):
        plan_mod.load_training_state(prev, fp32_model)
    with pytest.raises(ValueError, match="compute mode"):
        plan_mod.load_training_state(exported("small"), model2)


def test_export_keeps_accumulated_gradients(emu):
    """the recording run is a real step on the model's tensors: gradients the caller has accumulated come back too"""
    name = "small"
    model, opt = build_model(name)
    b = batch(name, 1)
    model(b[0], time=b[1], labels=b[2]).loss.backward()
    grads = model._arena.grad.clone()
    assert float(grads.abs().max()) > 0.0
    flags = (model._engine.grads_are_zero, model._engine.lazy_grads)
    model.export_plan(b[0], time=b[1], labels=b[2], train=opt)
    assert torch.equal(model._arena.grad, grads) and (model._engine.grads_are_zero, model._engine.lazy_grads) == flags


def test_resume_from_a_snapshot(emu):
    name = "small"
    image = exported(name)
    model, opt = build_model(name)
    whole, first = Plan.load(image), Plan.load(image)
    for k in range(4):
        b, lr = batch(name, k), rates(opt, k)
        python_step(model, opt, b, lr)
        whole.train_step(*b, lr)
        if k < 2:
            first.train_step(*b, lr)
    snap = first.snapshot(image)
    first.free()
    assert len(snap) == len(image) and snap != image
    # 2 steps, snapshot, a new plan from the snapshot, 2 more steps
    resumed = Plan.load(snap)
    assert resumed.train_status()["applied"] == 2
    # ... and the same snapshot back in Python: a fresh model and optimizer continue there
    model2, opt2 = build_model(name)
    plan_mod.load_training_state(snap, model2, opt2)
    assert opt2.step_count == 2
    for k in (2, 3):
        b, lr = batch(name, k), rates(opt, k)
        resumed.train_step(*b, lr)
        python_step(model2, opt2, b, lr)
    end = resumed.snapshot(snap)
    assert_state_equal(end, model, opt, "resumed plan")
    assert_state_equal(whole.snapshot(image), model, opt, "uninterrupted plan")
    for k, v in python_state(model2, opt2).items():
        assert torch.equal(v, python_state(model, opt)[k]), k
    # a model of another configuration is refused
    other, _ = build_model("c96")
    with pytest.raises(ValueError, match="arena"):
        plan_mod.load_training_state(end, other)
    whole.free(), resumed.free()


# ------------------------------------------------------------------------------------------------------- refusals
def test_runtime_refusals_launch_nothing(emu):
    name = "small"
    image = exported(name)
    pv, t, y = batch(name, 0)
    plan = Plan.load(image)
    L, hnd = plan._lib, plan._h
    loss, lr = torch.full((1,), 7.0), (ctypes.c_float * 8)(*([1e-3] * 8))
    lrp = ctypes.cast(lr, ctypes.c_void_p)
    target = (ctypes.c_uint64 * (len(image) // 8))()
    ctypes.memmove(target, image, len(image))

    def refused(status, call):
        before = issued(plan)
        assert call() == status
        assert issued(plan) == before and float(loss) == 7.0
    P = lambda x: None if x is None else x.data_ptr()      # noqa: E731
    for a, b, c, r in ((None, t, y, lrp), (pv, None, y, lrp), (pv, t, None, lrp), (pv, t, y, None)):
        refused(-1, lambda: L.scot_plan_train_step(hnd, P(a), P(b), P(c), r, P(loss), None))
    for a, b, c, o in ((None, t, y, loss), (pv, None, y, loss), (pv, t, None, loss), (pv, t, y, None)):
        refused(-1, lambda: L.scot_plan_loss(hnd, P(a), P(b), P(c), P(o), None, None))
    # a snapshot target that is not this plan's image: another size, another header, another buffer table, another training section
    h, tr_off = Plan.header(image), Plan.header(image)[H.H_TRAIN_OFF]
    refused(-1, lambda: L.scot_plan_snapshot(hnd, None, len(image), None))
    refused(-1, lambda: L.scot_plan_snapshot(hnd, target, len(image) - 8, None))
    for off in (8 * H.H_NENTRIES, h[H.H_BUFFERS_OFF] + 8, tr_off + 8 * H.TR_LR_ARG):
        word = off // 8
        target[word] += 1
        refused(-1, lambda: L.scot_plan_snapshot(hnd, target, len(image), None))
        target[word] -= 1
    assert L.scot_plan_snapshot(hnd, target, len(image), None) == 0 and bytes(target) == image
    # the adjoint calls on a training plan
    g = torch.zeros_like(y)
    refused(-3, lambda: L.scot_plan_vjp(hnd, g.data_ptr(), pv.data_ptr(), None, 0.0, None))
    refused(-3, lambda: L.scot_plan_rollout_vjp(hnd, pv.data_ptr(), t.data_ptr(), g.data_ptr(), g.data_ptr(), 1, pv.data_ptr(), None, 0.0, None))
    plan.free()
    # the training calls on a format-1 and on a format-2 plan
    model, fpv, ft = frozen_model("small")
    for kw in ({}, {"adjoint": ("pixel_values",)}):
        plan = Plan.load(model.export_plan(fpv, time=ft, **kw))
        assert set(plan.describe_training().values()) == {0}
        hnd = plan._h
        refused(-3, lambda: L.scot_plan_train_step(hnd, pv.data_ptr(), t.data_ptr(), y.data_ptr(), lrp, loss.data_ptr(), None))
        refused(-3, lambda: L.scot_plan_loss(hnd, pv.data_ptr(), t.data_ptr(), y.data_ptr(), loss.data_ptr(), None, None))
        refused(-3, lambda: L.scot_plan_snapshot(hnd, target, len(image), None))
        refused(-3, lambda: L.scot_plan_train_status(hnd, (ctypes.c_double * 6)(), None))
        plan.free()


def test_export_refusals_record_nothing(emu, monkeypatch):
    import emu_session
    from scOT.model import ScOT
    name = "small"
    model, opt = build_model(name)
    pv, t, y = batch(name, 0)
    recorded = []
    monkeypatch.setattr(plan_mod, "_record_training", lambda *a, **k: recorded.append(a))
    monkeypatch.setattr(plan_mod, "_record", lambda *a, **k: recorded.append(a))

    def refused(match, m=model, **kw):
        with pytest.raises(PlanExportError, match=match):
            m.export_plan(**dict(dict(pixel_values=pv, time=t, labels=y, train=opt), **kw))
        assert not recorded
    refused("labels", train=None)                                   # today's refusal and message
    refused("train= without labels", labels=None)
    refused("pixel_mask", pixel_mask=torch.ones(pv.shape[0], 32, 32, dtype=torch.bool))
    refused("adjoint= together with train=", adjoint=("pixel_values",))
    refused("FusedAdamW", train=torch.optim.AdamW(model.parameters(), lr=1e-3))
    other, other_opt = build_model(name)
    refused("this very model", train=other_opt)
    refused("image_size", pixel_values=torch.zeros(pv.shape[0], pv.shape[1], 16, 16), labels=torch.zeros(pv.shape[0], 4, 16, 16))
    refused("labels have shape", labels=y[:, :2].contiguous())
    # stochastic depth
    cfg = ScOTConfig(**dict(SMALL, drop_path_rate=0.1))
    dp = ScOT(cfg, compute="fp32").train()
    dp._ensure_arena(torch.device("cpu"))
    refused("drop_path_rate", m=dp, train=emu_session.fused_adamw(dp, lr=1e-3))
    # a frozen parameter
    p = next(other.parameters())
    p.requires_grad_(False)
    refused("requires_grad=False", m=other, train=other_opt)
    p.requires_grad_(True)
    # a data-parallel reducer (the engine's range hook, or the model's gradient-ready hook)
    other._engine.on_grads_final = lambda prefix: None
    refused("data-parallel", m=other, train=other_opt)
    other._engine.on_grads_final = None
    other.register_grad_ready_hook(lambda m: None)
    refused("data-parallel", m=other, train=other_opt)


# ------------------------------------------------------------------------------------------------------- refusals at load
def corrupt_images(image):
    """{label: (bytes, expected status)}: the corrupt variants of a good format-4 image"""
    h, tr = Plan.header(image), plan_mod.training_words(image)
    out = {}

    def buffer_word(buf, w):
        return word(image, h[H.H_BUFFERS_OFF] + 32 * buf + 8 * w)
    for s, what in enumerate(("step forward", "step backward", "update")):      # first relocation of the list's first entry
        out[f"{what}: relocation beyond its buffer"] = (relocation_beyond_its_buffer(image, s), -1)
    upd = tr[H.TR_UPD + 1]
    out["update entry renamed to a name outside the training list"] = (renamed(image, word(image, upd), "scot_dp_pack"), -3)
    out["inference entry renamed to scot_adamw_step"] = (renamed(image, word(image, h[H.H_ENTRIES_OFF]), "scot_adamw_step"), -3)
    t_off = h[H.H_TRAIN_OFF]
    assert tr[H.TR_LR_ENTRY] != 0
    out["lr patch point on another entry"] = (patched(image, t_off + 8 * H.TR_LR_ENTRY, 0), -1)
    out["lr patch point past the update"] = (patched(image, t_off + 8 * H.TR_LR_ENTRY, tr[H.TR_UPD]), -1)
    out["lr patch point on another argument"] = (patched(image, t_off + 8 * H.TR_LR_ARG, 0), -1)
    wd_arg = tr[H.TR_LR_ARG] + 1      # (the weight-decay array: same kind, same length, not a patch point)
    out["lr patch point on the weight-decay array"] = (patched(image, t_off + 8 * H.TR_LR_ARG, wd_arg), -1)
    out["two state spans over the same bytes"] = (patched(image, t_off + 8 * H.TR_EXP_AVG_SQ, tr[H.TR_EXP_AVG]), -1)
    out["lr patch point with the wrong length"] = (patched(image, t_off + 8 * H.TR_GROUPS, tr[H.TR_GROUPS] + 1), -1)
    constant = next(i for i in range(h[H.H_NBUFFERS]) if buffer_word(i, 0) == H.CONSTANT and buffer_word(i, 1) >= 8)
    out["state span inside a constant"] = (patched(patched(image, t_off + 8 * (H.TR_STEP_STATE + 1), 0), t_off + 8 * H.TR_STEP_STATE, constant), -1)
    out["labels in an output buffer"] = (patched(image, t_off + 8 * H.TR_LABELS, tr[H.TR_PRED]), -1)
    out["state buffer not stored"] = (patched(image, h[H.H_BUFFERS_OFF] + 32 * tr[H.TR_ARENA] + 24, 0), -1)
    out["state content past the data section"] = (patched(image, h[H.H_BUFFERS_OFF] + 32 * tr[H.TR_ARENA] + 16, h[H.H_DATA_BYTES]), -1)
    out["training section past the end"] = (patched(image, 8 * H.H_TRAIN_OFF, len(image) - 8 * (H.TRAIN_WORDS - 1)), -1)
    out["update list past the end"] = (patched(image, t_off + 8 * (H.TR_UPD + 2), 1 << 31), -1)
    out["truncated"] = (image[:t_off + 8], -1)
    out["format 3"] = (patched(image, 8 * H.H_FORMAT, 3), -3)
    out["relabelled format 1"] = (patched(image, 8 * H.H_FORMAT, 1), -3)      # (its name table holds names no inference image may hold)
    return out


def test_load_refusals(emu):
    image = exported("small")
    lib = plan_mod.bind(emu)
    handle = ctypes.c_void_p()
    assert plan_mod.load_raw(lib, image, handle) == 0 and handle.value
    assert lib.scot_plan_free(handle) == 0
    for label, (bad, status) in corrupt_images(image).items():
        handle = ctypes.c_void_p(0xdead)
        assert plan_mod.load_raw(lib, bad, handle) == status, label
        assert not handle.value, label
        assert lib.scot_plan_describe_training(handle, (ctypes.c_longlong * 8)()) == -1


def test_stand_alone_image_check_under_sanitizers(emu, tmp_path):
    """tools/plan_image_check.cc: the validator alone, built with the address and undefined-behaviour sanitizers, over a good format-4
    image and the corrupt variants — a child process on the CPU, nothing preloaded."""
    image = exported("small")
    check_images_stand_alone(tmp_path, {"good": (image, 0), **corrupt_images(image)})


# ------------------------------------------------------------------------------------------------------- header, table, lists
def test_header_prototypes_and_lists(emu):
    import emu_session
    header = open(os.path.join(ROOT, "include", "scot_plan.h")).read()
    declared = set(re.findall(r"\b(scot_[a-z0-9_]+)\s*\(", header))
    assert declared == set(scotlib.PLAN_PROTOTYPES) and NEW_CALLS <= declared
    for kind in ("bf16", "f16"):
        lib = plan_mod.bind(emu_session.load_emu(kind))
        assert lib.scot_abi_version() == scotlib.ABI_VERSION == 8
        fwd, bwd = plan_mod.runtime_entry_points(lib), plan_mod.runtime_entry_points(lib, adjoint=True)
        trn = plan_mod.runtime_entry_points(lib, training=True)
        assert not set(OPTIMIZER_ONLY) & (set(fwd) | set(bwd)) and set(OPTIMIZER_ONLY) <= set(trn)
        assert set(fwd) <= set(trn) and len(trn) == len(set(trn)) and set(trn) <= set(scotlib.PROTOTYPES)
        assert all(scotlib.PROTOTYPES[n][-1] is ctypes.c_void_p for n in trn)      # the stream, last
        assert lib.scot_plan_training_entry_point(-1) is None and lib.scot_plan_training_entry_point(len(trn)) is None
    image = exported("small")
    assert not set(OPTIMIZER_ONLY) & set(names_of(image, "forward"))
    assert names_of(image, 2)[-1] in ("scot_optim_finish", "scot_transpose_cast") and "scot_adamw_step" in names_of(image, 2)
    assert names_of(image, 1)[0] in ("scot_memset_async", "scot_segments_scale")      # the gradient fill comes first


def test_gfx950_builds_export_the_training_calls():
    for kind in ("bf16", "f16"):
        lib = scotlib.load(kind=kind)
        for name in NEW_CALLS:
            assert getattr(lib, name).argtypes == scotlib.PLAN_PROTOTYPES[name]
        assert lib.scot_abi_version() == 8
        assert lib.scot_plan_train_step(None, None, None, None, None, None, None) == -1
        assert lib.scot_plan_training_entry_point(0) == b"scot_gemm"
