"""Gradient accumulation in training plans on the CPU emulation: scot_plan_accumulate runs a micro-batch into the plan's fp32 accumulator,
scot_plan_apply runs the recorded update from it (csrc/plan.hip, csrc/optim.hip: scot_grad_accumulate).

The reference of every comparison is the Python loop in the same process, per micro-batch

    opt.zero_grad(); model(pv_k, time=t_k, labels=y_k).loss.backward(); g = arena.grad.clone(); A = g * w   (later: A = A + g * w)

and per update: A written into arena.grad, the groups' lr set, opt.step().  On the emulator the same calls run in the same order, so every
comparison is bit for bit.  "Launches nothing" is read from `scot_plan_emu_issued()`."""
import ctypes
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from plan_support import ROOT, emu, frozen_model, issued  # noqa: E402,F401
from poseidon_amd import lib as scotlib, plan as plan_mod  # noqa: E402
from poseidon_amd.plan import Plan  # noqa: E402
from test_plan_masked_emu_cpu import exported as exported_masked, mask_of  # noqa: E402
from test_plan_train_emu_cpu import assert_state_equal, batch, build_model, exported, python_state, rates  # noqa: E402,F401

NEW_CALLS = {"scot_grad_accumulate", "scot_grad_accumulate_blocks", "scot_plan_accumulate", "scot_plan_apply", "scot_plan_gradients",
             "scot_plan_accumulation_status"}
THIRD = float(torch.tensor(1.0 / 3.0, dtype=torch.float32))      # the fp32 weight the C call receives, exactly


def parameter_positions(opt):
    return (opt._map != 255).repeat_interleave(8)


def python_micro_batch(model, opt, b, mask=None):
    """-> (loss [1], this micro-batch's own gradient arena)"""
    opt.zero_grad()
    out = model(b[0], time=b[1], labels=b[2], **({} if mask is None else {"pixel_mask": mask}))
    out.loss.backward()
    return out.loss.detach().reshape(1).clone(), model._arena.grad.clone()


def python_apply(model, opt, A, lr):
    model._arena.grad.copy_(A)
    for g, r in zip(opt.param_groups, lr):
        g["lr"] = r
    opt.step()


def accumulate_both(plan, model, opt, batches, w, masks=None):
    """the micro-batches through the plan and through Python, compared after each -> Python's accumulator"""
    on, A = parameter_positions(opt), None
    for k, b in enumerate(batches):
        m = None if masks is None else masks[k]
        ref, g = python_micro_batch(model, opt, b, m)
        A = g * w if k == 0 else A + g * w
        got = plan.accumulate(*b, w, k == 0, pixel_mask=m)
        assert torch.equal(got, ref), k
        mine = plan.gradients(1)
        assert mine.shape == A.shape and torch.equal(mine[on], A[on]) and float(mine[~on].abs().max()) == 0.0, k
        assert plan.accumulation_status() == dict(micro_batches=k + 1, bytes=4 * A.numel())
    return A


def updates_follow_python(name, image, updates=2, micro=3, masks=None):
    model, opt = build_model(name)
    plan = Plan.load(image)
    for u in range(updates):
        ks = [u * micro + k for k in range(micro)]
        plan.poison(0xFF)
        A = accumulate_both(plan, model, opt, [batch(name, k) for k in ks], THIRD, None if masks is None else [masks(k) for k in ks])
        lr = rates(opt, u)
        python_apply(model, opt, A, lr)
        plan.apply(lr)
        assert plan.accumulation_status()["micro_batches"] == 0
        assert_state_equal(plan.snapshot(image), model, opt, f"update {u}")
    st = plan.train_status()
    assert (st["applied"], st["skipped"], st["nonfinite"]) == (updates, 0, 0)
    assert st["grad_norm"] == float(opt.last_grad_norm) and st["clip_coef"] == float(opt._clip[0])
    assert st["grad_scale"] == model._engine.grad_scale_value()
    plan.free()


# ------------------------------------------------------------------------------------------------------- cases 1, 3, 4
@pytest.mark.parametrize("name", ["small", "c96"])
def test_updates_of_three_micro_batches_are_bit_identical(emu, name):
    updates_follow_python(name, exported(name))


def test_two_stream_plan_gives_the_same_bits(emu):
    name = "small"
    model, opt = build_model(name)
    pv, t, y = batch(name, 0)
    image = model.export_plan(pv, time=t, labels=y, train=opt, streams=2)
    assert Plan.header(image)[plan_mod.H_FORMAT] == plan_mod.FORMAT_TRAINING_STREAMS
    updates_follow_python(name, image)


def test_masked_plan_follows_the_masked_loop(emu):
    name, kind = "small", "element"
    image = exported_masked(name, kind)
    updates_follow_python(name, image, updates=1, masks=lambda k: mask_of(name, kind, k))
    # the mask exactly where the plan is a masked one: -1 and nothing issued
    b = batch(name, 0)
    for img, mask in ((image, None), (exported(name), mask_of(name, kind, 0))):
        plan = Plan.load(img)
        before = issued(plan)
        with pytest.raises(scotlib.ScotLibraryError, match="bad shape"):
            plan.accumulate(*b, 1.0, True, pixel_mask=mask)
        assert issued(plan) == before and plan.accumulation_status() == dict(micro_batches=0, bytes=0)
        plan.free()


# ------------------------------------------------------------------------------------------------------- case 2
@pytest.mark.parametrize("name", ["small", "c96"])
def test_one_micro_batch_of_weight_one_is_train_step(emu, name):
    image = exported(name)
    whole, cut = Plan.load(image), Plan.load(image)
    _, opt = build_model(name)
    for k in range(2):
        b, lr = batch(name, k), rates(opt, k)
        a = whole.train_step(*b, lr)
        c = cut.accumulate(*b, 1.0, True)
        cut.apply(lr)
        assert torch.equal(a, c) and whole.snapshot(image) == cut.snapshot(image), k
        assert whole.train_status() == cut.train_status()
    whole.free(), cut.free()


# ------------------------------------------------------------------------------------------------------- case 5
def test_an_overflowed_accumulation_is_one_skipped_step(emu):
    """gradient scale 2^30 before the export: both micro-batches overflow, the update is skipped ONCE"""
    import overflow_sweep as osw
    name = "small16"
    model, opt = build_model(name)
    b0 = batch(name, 0)
    model(b0[0], time=b0[1], labels=b0[2]).loss.backward()      # (the first training forward picks the automatic scale)
    opt.zero_grad()
    osw.set_scale(model._engine, 30)
    image = model.export_plan(*b0[:1], time=b0[1], labels=b0[2], train=opt)
    before = plan_mod.training_state(image)
    assert float(before["scale_state"][0]) == 2.0 ** 30
    plan = Plan.load(image)
    counted = []
    on = parameter_positions(opt)
    for k in range(2):
        b = batch(name, k)
        ref, g = python_micro_batch(model, opt, b)
        A = g * 0.5 if k == 0 else A + g * 0.5
        assert torch.equal(plan.accumulate(*b, 0.5, k == 0), ref)
        counted.append(int(model._engine.grad_overflow))
        assert not bool(torch.isfinite(plan.gradients(1)[on]).all())
        assert float(plan_mod.training_state(plan.snapshot(image))["scale_state"][0]) == 2.0 ** 30      # the scale does not move meanwhile
    assert 0 < counted[0] < counted[1]
    lr = rates(opt, 0)
    python_apply(model, opt, A, lr)
    plan.apply(lr)
    snap = plan.snapshot(image)
    assert_state_equal(snap, model, opt, "skipped update")
    after = plan_mod.training_state(snap)
    assert all(torch.equal(before[x], after[x]) for x in ("arena", "exp_avg", "exp_avg_sq", "shadow"))
    assert float(after["scale_state"][0]) == 2.0 ** 29
    st = plan.train_status()
    assert (st["applied"], st["skipped"], st["nonfinite"]) == (0, 1, counted[1]) and opt.skipped_steps() == 1
    plan.free()


# ------------------------------------------------------------------------------------------------------- case 6
def test_the_host_may_rewrite_the_accumulator_before_apply(emu):
    """where a data-parallel host all-reduces: here it halves the accumulator in place"""
    name = "small"
    image = exported(name)
    model, opt = build_model(name)
    plan = Plan.load(image)
    A = accumulate_both(plan, model, opt, [batch(name, k) for k in range(2)], 0.5)
    view = plan.gradients(1)
    assert view.data_ptr() == plan.gradients(1).data_ptr()      # a view of the plan's own buffer, not a copy
    view.mul_(0.5)
    lr = rates(opt, 1)
    python_apply(model, opt, A * 0.5, lr)
    plan.apply(lr)
    assert_state_equal(plan.snapshot(image), model, opt, "halved accumulator")
    assert torch.equal(plan.gradients(0)[parameter_positions(opt)], (A * 0.5)[parameter_positions(opt)])      # what the update read
    plan.free()


# ------------------------------------------------------------------------------------------------------- case 7
def test_refusals_and_interactions(emu):
    name = "small"
    image = exported(name)
    pv, t, y = batch(name, 0)
    plan = Plan.load(image)
    L, hnd = plan._lib, plan._h
    floats = plan.describe_training()["arena_floats"]
    loss, lr = torch.full((1,), 7.0), (ctypes.c_float * 8)(*([1e-3] * 8))
    lrp = ctypes.cast(lr, ctypes.c_void_p)
    ptr, n = ctypes.c_void_p(), ctypes.c_size_t()
    status = (ctypes.c_longlong * 2)(5, 5)

    def refused(code, call):
        before = issued(plan)
        assert call() == code
        assert issued(plan) == before and float(loss) == 7.0

    def accumulate(first, w=1.0, p=pv, lab=y, h=None):
        return L.scot_plan_accumulate(h or hnd, p.data_ptr() if p is not None else None, t.data_ptr(), lab.data_ptr() if lab is not None else None,
                                      None, w, first, loss.data_ptr(), None)
    # nothing open yet
    refused(-1, lambda: accumulate(0))
    refused(-1, lambda: L.scot_plan_apply(hnd, lrp, None))
    refused(-1, lambda: L.scot_plan_gradients(hnd, 1, ctypes.byref(ptr), ctypes.byref(n)))
    refused(-1, lambda: L.scot_plan_gradients(hnd, 2, ctypes.byref(ptr), ctypes.byref(n)))
    refused(-1, lambda: accumulate(1, p=None))
    refused(-1, lambda: accumulate(1, lab=None))
    refused(-1, lambda: accumulate(1, w=float("inf")))
    assert L.scot_plan_accumulation_status(hnd, status) == 0 and list(status) == [0, 0]
    assert L.scot_plan_gradients(hnd, 0, ctypes.byref(ptr), ctypes.byref(n)) == 0 and ptr.value and n.value == floats
    # the accumulator is allocated at the first accumulate, counted once
    before_bytes = plan.describe()["device_bytes"]
    start = plan.snapshot(image)
    loss.fill_(7.0)
    plan.accumulate(pv, t, y, 0.5, True)
    assert plan.describe()["device_bytes"] == before_bytes + 4 * floats
    plan.accumulate(pv, t, y, 0.5, False)
    assert plan.describe()["device_bytes"] == before_bytes + 4 * floats and plan.accumulation_status() == dict(micro_batches=2, bytes=4 * floats)
    # while it is open: a step is refused; apply without rates is refused; validation is allowed and writes neither A nor a state buffer
    refused(-1, lambda: L.scot_plan_train_step(hnd, pv.data_ptr(), t.data_ptr(), y.data_ptr(), lrp, loss.data_ptr(), None))
    refused(-1, lambda: L.scot_plan_apply(hnd, None, None))
    A = plan.gradients(1).clone()
    plan.run(pv, t)
    plan.loss(pv, t, y)
    plan.evaluate(pv, t, y)
    assert torch.equal(plan.gradients(1).view(torch.int32), A.view(torch.int32))
    assert plan.snapshot(image) == start and plan.accumulation_status()["micro_batches"] == 2
    # poison fills A and discards the accumulation
    plan.poison(0xFF)
    assert bool(torch.isnan(plan.gradients(1)).all()) and plan.accumulation_status() == dict(micro_batches=0, bytes=4 * floats)
    refused(-1, lambda: accumulate(0))
    refused(-1, lambda: L.scot_plan_apply(hnd, lrp, None))
    assert accumulate(1) == 0 and float(loss) != 7.0      # ... and a first micro-batch opens the next one, the rest of A zero again
    assert bool(torch.isfinite(plan.gradients(1)).all())
    loss.fill_(7.0)
    plan.free()
    # the training calls of this section on a format-1 plan
    model, fpv, ft = frozen_model("small")
    frozen = Plan.load(model.export_plan(fpv, time=ft))
    fh = frozen._h
    refused(-3, lambda: accumulate(1, h=fh))
    refused(-3, lambda: L.scot_plan_apply(fh, lrp, None))
    refused(-3, lambda: L.scot_plan_gradients(fh, 0, ctypes.byref(ptr), ctypes.byref(n)))
    assert L.scot_plan_accumulation_status(fh, status) == -3
    frozen.free()


# ------------------------------------------------------------------------------------------------------- case 8
def test_header_prototypes_and_symbols(emu):
    import emu_session
    header = open(os.path.join(ROOT, "include", "scot_plan.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_CALLS:
        m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m, name
        params = [p.strip() for p in m.group(2).split(",")]

        def ctype(p):
            if "*" in p or "scot_plan_t" in p or "scot_stream_t" in p:
                return ctypes.c_void_p
            return {"size_t": ctypes.c_size_t, "float": ctypes.c_float, "int": ctypes.c_int}[p.split()[0]]
        assert [ctype(p) for p in params] == scotlib.PLAN_PROTOTYPES[name], name
    assert not NEW_CALLS & set(scotlib.PROTOTYPES)
    kernel_header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scot_hip.h")).read(), flags=re.S)
    assert not any(name in kernel_header for name in NEW_CALLS)
    for kind in ("bf16", "f16"):
        lib = plan_mod.bind(emu_session.load_emu(kind))
        assert lib.scot_abi_version() == scotlib.ABI_VERSION == 8
        listed = set(plan_mod.runtime_entry_points(lib)) | set(plan_mod.runtime_entry_points(lib, training=True))
        assert not NEW_CALLS & listed                      # no recorded call list can name them
    for text in ("covered: stochastic depth", "never been run on more than one GPU", "two roundings"):
        assert text in header


def test_gfx950_builds_export_the_accumulation_calls():
    for kind in ("bf16", "f16"):
        lib = scotlib.load(kind=kind)
        for name in NEW_CALLS:
            assert getattr(lib, name).argtypes == scotlib.PLAN_PROTOTYPES[name]
        assert lib.scot_abi_version() == 8
        assert lib.scot_plan_accumulate(None, None, None, None, None, 1.0, 1, None, None) == -1
        assert lib.scot_plan_apply(None, None, None) == -1
        assert lib.scot_plan_gradients(None, 0, None, None) == -1
        assert lib.scot_plan_accumulation_status(None, None) == -1
        assert lib.scot_grad_accumulate(None, None, None, None, 8, 1.0, None) == -1
        assert lib.scot_grad_accumulate_blocks(8) == 1
