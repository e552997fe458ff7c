"""Pixel masks in plans on the CPU emulation: masked training plans (`export_plan(..., pixel_mask=M, train=opt)`,
scot_plan_loss_masked, scot_plan_train_step_masked) and masked evaluation (scot_plan_evaluate_masked), replayed by the plan runtime of
libscot_emu.so in plain host memory.

The reference of every training comparison is the Python loop in the same process with the same mask passed to `model(...)`; on the
emulator the same calls run in the same order, so every comparison is bit for bit.  Each step has its own batch, its own mask and its
own learning rates: a stale mask copy shows."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import error_sums_cases as E  # noqa: E402
import plan_eval_cases as PE  # noqa: E402
import plan_masked_cases as PM  # noqa: E402
from plan_support import check_images_stand_alone, emu, frozen_model, issued, names_of, patched  # noqa: E402,F401
from poseidon_amd import plan as plan_mod  # noqa: E402
from poseidon_amd.plan import Plan, PlanExportError  # noqa: E402
from test_plan_train_emu_cpu import MODELS, assert_state_equal, batch, build_model, exported as exported_unmasked, rates  # noqa: E402

H = plan_mod
_cache = {}


def mask_of(name, kind, k):
    kw, _, B = MODELS[name]
    return PM.batch_mask(kind, B, kw["num_out_channels"], kw["image_size"], kw["image_size"], k)


def exported(name, kind, streams=1):
    """one masked export per (model, mask kind, streams) for the whole module"""
    key = (name, kind, streams)
    if key not in _cache:
        model, opt = build_model(name)
        pv, t, y = batch(name, 0)
        before = [x.clone() for x in (model._arena.data, opt.exp_avg, opt._step_state)]
        _cache[key] = model.export_plan(pv, time=t, labels=y, pixel_mask=mask_of(name, kind, 0), train=opt, streams=streams)
        assert all(torch.equal(a, b) for a, b in zip(before, (model._arena.data, opt.exp_avg, opt._step_state))) and opt.step_count == 0
    return _cache[key]


def python_step(model, opt, b, mask, lr):
    opt.zero_grad(overlap=True)
    out = model(b[0], time=b[1], labels=b[2], pixel_mask=mask)
    out.loss.backward()
    for g, r in zip(opt.param_groups, lr):
        g["lr"] = r
    opt.step()
    return out.loss.detach().reshape(1).clone()


# ------------------------------------------------------------------------------------------------------- training
@pytest.mark.parametrize("name,kind,streams", [("small", "channel", 1), ("small", "element", 1), ("small", "shared", 1), ("c96", "channel", 1),
                                               ("c96", "element", 1), ("small", "channel", 2)])
def test_masked_steps_are_bit_identical(emu, name, kind, streams):
    image = exported(name, kind, streams)
    kw, _, B = MODELS[name]
    n = B * kw["num_out_channels"] * (1 if kind == "channel" else kw["image_size"] ** 2)
    h, tr = Plan.header(image), plan_mod.training_words(image)
    assert h[H.H_FORMAT] == (4 if streams == 1 else 6)                      # the header still says format 4 / 6
    assert tr[H.TR_FLAGS] & 6 == (2 if kind == "channel" else 6)
    plan = Plan.load(image)
    d = plan.describe()
    assert d["has_pixel_mask"] == 1 and d["pixel_mask_bytes"] == n and plan.describe_training()["mask"] == (1 if kind == "channel" else 2)
    for lst in (0, 1):      # the recorded loss names the mask; the list is C-ABI calls only (the exporter refuses anything else)
        assert ("scot_head_finalize", "scot_loss_bwd")[lst] in names_of(image, lst)
    model, opt = build_model(name)
    # the loss alone: Python's bits with the same mask, the labels at the masked positions, and no state buffer written
    b, m = batch(name, 1), mask_of(name, kind, 1)
    plan.poison(0xFF)
    loss, pred = plan.loss(*b, pixel_mask=m)
    out = model(b[0], time=b[1], labels=b[2], pixel_mask=m)
    assert torch.equal(loss, out.loss.detach().reshape(1)) and torch.equal(pred, out.output.detach())
    full = PM.expanded(m, pred.shape)
    assert bool(full.any()) and torch.equal(pred[full], b[2][full])
    assert plan.snapshot(image) == image
    del out
    for k in range(3):      # a different batch, mask and lr per step
        b, m, lr = batch(name, k), mask_of(name, kind, k), rates(opt, k)
        plan.poison(0xFF)
        ref = python_step(model, opt, b, m, lr)
        given = m
        if k == 1:      # the uint8 form of the plan's own mask shape
            given = (m if kind == "channel" else PM.expanded(m, b[2].shape)).to(torch.uint8)
        got = plan.train_step(*b, lr, pixel_mask=given)
        assert torch.isfinite(ref).all() and torch.equal(got, ref), k
        assert_state_equal(plan.snapshot(image), model, opt, f"step {k}")
    st = plan.train_status()
    assert (st["applied"], st["skipped"], st["nonfinite"]) == (3, 0, 0)
    # scot_plan_run at the current weights, without a mask; a snapshot resumes
    model.eval()
    with torch.no_grad():
        ref = model(b[0], time=b[1]).output
    assert torch.equal(plan.run(b[0], b[1]), ref)
    again = Plan.load(plan.snapshot(image))
    assert again.train_status()["applied"] == 3 and torch.equal(again.run(b[0], b[1]), ref)
    plan.free(), again.free()


@pytest.mark.parametrize("kind", ["channel", "element"])
def test_an_all_false_mask_gives_the_unmasked_plans_bits(emu, kind):
    name = "small"
    masked, plain = Plan.load(exported(name, kind)), Plan.load(exported_unmasked(name))
    _, opt = build_model(name)
    for k in range(3):
        b, lr = batch(name, k), rates(opt, k)
        none = torch.zeros_like(mask_of(name, kind, k))
        la, pa = masked.loss(*b, pixel_mask=none)
        lb, pb = plain.loss(*b)
        assert torch.equal(la, lb) and torch.equal(pa, pb)
        assert torch.equal(masked.train_step(*b, lr, pixel_mask=none), plain.train_step(*b, lr))
        a, c = plan_mod.training_state(masked.snapshot(exported(name, kind))), plan_mod.training_state(plain.snapshot(exported_unmasked(name)))
        assert a.keys() == c.keys() and all(torch.equal(a[x], c[x]) for x in a), k
    masked.free(), plain.free()


def test_an_unmasked_export_is_what_it_was(emu):
    """An unmasked export writes no mask word: FLAGS <= 1, no mask input, kind 0.  (Byte-identity with the exporter before the masks was
    compared once on fresh exports of this model from both trees: the images were equal byte for byte.)"""
    image = exported_unmasked("small")
    tr, io = plan_mod.training_words(image), Plan.header(image)[H.H_IO_OFF]
    assert tr[H.TR_FLAGS] <= 1
    assert int.from_bytes(image[io + 8 * H.IO_HAS_MASK:][:8], "little") == 0
    plan = Plan.load(image)
    assert plan.describe()["has_pixel_mask"] == 0 and plan.describe_training()["mask"] == 0
    plan.free()


def test_runtime_refusals_launch_nothing(emu):
    name = "small"
    pv, t, y = batch(name, 0)
    loss, lr = torch.full((1,), 7.0), (ctypes.c_float * 8)(*([1e-3] * 8))
    lrp = ctypes.cast(lr, ctypes.c_void_p)
    chan, elem = mask_of(name, "channel", 0).to(torch.uint8), mask_of(name, "element", 0).to(torch.uint8)
    P = lambda x: None if x is None else x.data_ptr()      # noqa: E731

    def refused(plan, status, call):
        before = issued(plan)
        assert call() == status
        assert issued(plan) == before and float(loss) == 7.0
    masked, plain = Plan.load(exported(name, "channel")), Plan.load(exported_unmasked(name))
    L, hm, hp = masked._lib, masked._h, plain._h
    # a masked plan: the unmasked calls (the mask is missing) and a NULL mask
    refused(masked, -1, lambda: L.scot_plan_loss(hm, P(pv), P(t), P(y), P(loss), None, None))
    refused(masked, -1, lambda: L.scot_plan_train_step(hm, P(pv), P(t), P(y), lrp, P(loss), None))
    refused(masked, -1, lambda: L.scot_plan_loss_masked(hm, P(pv), P(t), P(y), None, P(loss), None, None))
    refused(masked, -1, lambda: L.scot_plan_train_step_masked(hm, P(pv), P(t), P(y), None, lrp, P(loss), None))
    for a, b, c in ((None, t, y), (pv, None, y), (pv, t, None)):
        refused(masked, -1, lambda: L.scot_plan_train_step_masked(hm, P(a), P(b), P(c), P(chan), lrp, P(loss), None))
    with pytest.raises(ValueError, match="channel"):
        masked.loss(pv, t, y, pixel_mask=elem)
    # an unmasked training plan: a mask is refused, a NULL mask is the unmasked call
    refused(plain, -1, lambda: L.scot_plan_loss_masked(hp, P(pv), P(t), P(y), P(chan), P(loss), None, None))
    refused(plain, -1, lambda: L.scot_plan_train_step_masked(hp, P(pv), P(t), P(y), P(chan), lrp, P(loss), None))
    a, b = torch.empty(1), torch.empty(1)
    assert L.scot_plan_loss_masked(hp, P(pv), P(t), P(y), None, P(a), None, None) == 0
    assert L.scot_plan_loss(hp, P(pv), P(t), P(y), P(b), None, None) == 0 and torch.equal(a, b)
    masked.free(), plain.free()
    # format 1, 2 and 5 plans
    model, fpv, ft = frozen_model("small")
    for kw in ({}, {"adjoint": ("pixel_values",)}, {"streams": 2}):
        plan = Plan.load(model.export_plan(fpv, time=ft, **kw))
        hnd = plan._h
        refused(plan, -3, lambda: L.scot_plan_loss_masked(hnd, P(pv), P(t), P(y), P(chan), P(loss), None, None))
        refused(plan, -3, lambda: L.scot_plan_train_step_masked(hnd, P(pv), P(t), P(y), P(chan), lrp, P(loss), None))
        plan.free()


def test_export_takes_the_three_forms_and_refuses_the_rest(emu, monkeypatch):
    """the three accepted forms are recorded — with the mask as the plan's input bytes —, every other shape or dtype is refused with
    nothing recorded, and a mask without train= is refused as before"""
    name = "small"
    model, opt = build_model(name)
    pv, t, y = batch(name, 0)
    recorded = []
    real = plan_mod._record_training

    def recording(*a, **k):
        out = real(*a, **k)
        recorded.append(out[-1]["mask"])
        return out
    monkeypatch.setattr(plan_mod, "_record_training", recording)
    for kind, shape in (("channel", (2, 4)), ("element", (2, 4, 32, 32)), ("shared", (2, 4, 32, 32))):
        m = mask_of(name, kind, 0)
        image = model.export_plan(pv, time=t, labels=y, pixel_mask=m, train=opt)
        got = recorded.pop()
        assert not recorded and got.dtype == torch.uint8 and tuple(got.shape) == shape and torch.equal(got != 0, PM.expanded(m, shape) if len(shape) == 4 else m)
        assert Plan.load(image).describe()["pixel_mask_bytes"] == got.numel()
    monkeypatch.setattr(plan_mod, "_record_training", lambda *a, **k: recorded.append(a))
    monkeypatch.setattr(plan_mod, "_record", lambda *a, **k: recorded.append(a))
    B, C, S = pv.shape[0], 4, 32
    for bad in (torch.ones(B, S, S, dtype=torch.bool), torch.ones(B, C + 1, dtype=torch.bool), torch.ones(B, 2, S, S, dtype=torch.bool),
                torch.ones(B, C, dtype=torch.float32), torch.ones(C, dtype=torch.bool), torch.ones(B, C, S, S, 1, dtype=torch.bool)):
        with pytest.raises(PlanExportError, match="pixel_mask"):
            model.export_plan(pv, time=t, labels=y, pixel_mask=bad, train=opt)
        assert not recorded
    with pytest.raises(PlanExportError, match="pixel_mask overwrites the prediction"):      # without train=: as before
        model.export_plan(pv, time=t, pixel_mask=torch.ones(B, C, dtype=torch.bool))
    assert not recorded


def corrupt_images(image):
    """{label: (bytes, -1)}: a masked training image whose mask words disagree"""
    h, tr = Plan.header(image), plan_mod.training_words(image)
    io, t_off = h[H.H_IO_OFF], h[H.H_TRAIN_OFF]
    n = int.from_bytes(image[io + 8 * (H.IO_MASK_BUF + 2):][:8], "little")
    return {"flag without a mask input": (patched(image, io + 8 * H.IO_HAS_MASK, 0), -1),
            "mask input without the flag": (patched(image, t_off + 8 * H.TR_FLAGS, tr[H.TR_FLAGS] & 1), -1),
            "element flag without the mask flag": (patched(patched(image, t_off + 8 * H.TR_FLAGS, (tr[H.TR_FLAGS] & 1) | 4), io + 8 * H.IO_HAS_MASK, 0), -1),
            "the other kind's bytes": (patched(image, t_off + 8 * H.TR_FLAGS, tr[H.TR_FLAGS] ^ 4), -1),
            "one mask byte short": (patched(image, io + 8 * (H.IO_MASK_BUF + 2), n - 1), -1),
            "one mask byte long": (patched(image, io + 8 * (H.IO_MASK_BUF + 2), n + 1), -1),
            "an unknown flag": (patched(image, t_off + 8 * H.TR_FLAGS, tr[H.TR_FLAGS] | 8), -1),
            "the mask in an output buffer": (patched(image, io + 8 * H.IO_MASK_BUF, tr[H.TR_PRED]), -1)}


def test_load_refusals_and_the_stand_alone_check(emu, tmp_path):
    """the validator on the good and the corrupt masked images: through the runtime's load, and alone under the host sanitizers
    (tools/plan_image_check.cc — a child process on the CPU, nothing preloaded)"""
    lib = plan_mod.bind(emu)
    cases = {}
    for kind in ("channel", "element"):
        image = exported("small", kind)
        cases[f"good {kind}"] = (image, 0)
        cases.update({f"{kind}: {k}": v for k, v in corrupt_images(image).items()})
    cases["good two-stream"] = (exported("small", "channel", 2), 0)
    for label, (data, status) in cases.items():
        handle = ctypes.c_void_p(0xdead)
        assert plan_mod.load_raw(lib, data, handle) == status, label
        assert bool(handle.value) == (status == 0), label
        if status == 0:
            assert lib.scot_plan_free(handle) == 0
    check_images_stand_alone(tmp_path, cases)


# ------------------------------------------------------------------------------------------------------- evaluation
def context(plan):
    return E.Ctx(plan._lib, torch.device("cpu"))


@pytest.mark.parametrize("kind", ["channel", "element"])
def test_evaluate_masked_is_the_hand_driven_chain(emu, kind):
    model, pv, t = frozen_model("small")
    plan = Plan.load(model.export_plan(pv, time=t))
    mask = PM.batch_mask(kind, 2, 4, 32, 32)
    PM.check_evaluate_masked(plan, context(plan), pv, t, 3, [0, 1, 3, 4], mask)
    PM.check_evaluate_masked(plan, context(plan), pv, t, 1, None, mask)
    plan.free()


def test_evaluate_masked_follows_the_reference_trainers_chain(emu):
    model, pv, t = frozen_model("small")
    plan = Plan.load(model.export_plan(pv, time=t))
    PM.check_python_chain(plan, model, pv, t, 3, PM.batch_mask("channel", 2, 4, 32, 32), [0, 1, 3, 4])
    plan.free()


def test_evaluate_masked_refusals_and_a_masked_training_plan(emu):
    name = "small"
    pv, t, y = batch(name, 0)
    plan = Plan.load(exported(name, "channel"))      # a masked TRAINING plan is not refused for having a mask input
    ctx = context(plan)
    mask = mask_of(name, "channel", 0)
    sums, _, _ = PM.check_evaluate_masked(plan, ctx, pv, t, 3, [0, 1, 3, 4], mask)
    assert torch.isfinite(sums).all()
    tg, m8 = torch.zeros(3, *y.shape), mask.to(torch.uint8)
    out = torch.full((3, 2, 2, 4), 7.0, dtype=torch.float64)
    L, h = plan._lib, plan._h

    def call(slices, mask_ptr, pixel_values=pv, targets=tg, sums=out, steps=3):
        """-> (status, copies, fills and calls the runtime issued for it)"""
        before = issued(plan)
        rc = L.scot_plan_evaluate_masked(h, PE.addr(pixel_values), t.data_ptr(), PE.addr(targets), mask_ptr, 0, steps, E.int_array(slices),
                                         len(slices) - 1, PE.addr(sums), None, None)
        return rc, issued(plan) - before
    for slices in ([1, 3], [0, 3], [1, 4]):      # groups that do not tile [0, Cout) under a mask: -1, before anything is copied or launched
        assert call(slices, m8.data_ptr()) == (-1, 0) and bool((out == 7.0).all()), slices
    for kw in (dict(pixel_values=None), dict(targets=None), dict(sums=None), dict(steps=0)):      # scot_plan_evaluate's refusals hold
        assert call([0, 4], m8.data_ptr(), **kw) == (-1, 0) and bool((out == 7.0).all()), kw
    assert call([0, 3, 1], m8.data_ptr()) == (-1, 0) and call([0, 5], m8.data_ptr()) == (-1, 0) and bool((out == 7.0).all())
    rc, n = call([1, 3], None)                   # without a mask those groups are accepted, as before
    assert rc == 0 and n > 0 and torch.isfinite(out).all()
    plan.free()
