"""Two-stream plans on the CPU emulation: `export_plan(..., streams=2)` records the engine's own two-stream program over stand-in
handles and writes an image of format 5 (inference) or 6 (training); the plan runtime of the emulated library replays it.

The emulation runs every entry to completion where it is issued, so what the streams and events mean here is the ORDER the image
admits: `image_entries` turns a list of an image into `tape_schedule.Entry` objects, `tape_schedule` derives legal orders from the
image's own stream indices and event edges, `scot_plan_issue_order` issues them, and every legal order has to give the bits of the
recorded order — which are the one-stream plan's and the model's own.  Taking an event edge out of the constraint set has to show."""
import ctypes
import os
import struct
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tape_schedule as ts  # noqa: E402
from plan_support import CFG96, SMALL, call_list, check_images_stand_alone, emu, entry_records, issued, names_of, other_inputs  # noqa: E402,F401
from plan_support import patched, renamed, synth_model, word  # noqa: E402
from poseidon_amd import plan as plan_mod  # noqa: E402
from poseidon_amd.config import ScOTConfig  # noqa: E402
from poseidon_amd.plan import Plan, PlanExportError  # noqa: E402
from poseidon_amd.synth import synth_inputs  # noqa: E402

H = plan_mod
MODELS = {"small": (SMALL, "fp32", 2), "c96": (CFG96, "fp16", 1)}
LISTS = {"forward": 0, 0: 2, 1: 3, 2: 4}      # plan_support's name of a call list -> SCOT_PLAN_CALLS_*
STATE = ("arena", "exp_avg", "exp_avg_sq", "step_state", "scale_state")
SEEDS = (11, 12, 13, 14)
# entry points that write parameter gradients and nothing else
WEIGHT_GRADIENTS = ("scot_wgrad_group", "scot_wgrad_mlp", "scot_conv5_wgrad", "scot_dwconv7_wgrad", "scot_nchw_channel_sum",
                    "scot_partial_colsum_batch")


# ------------------------------------------------------------------------------------------------------- models and exports
def inputs(name, k=0):
    kw, _, B = MODELS[name]
    pv, t, y = synth_inputs(B, kw["num_channels"], kw["num_out_channels"], kw["image_size"], "smooth")
    if k:
        g = torch.Generator().manual_seed(100 + k)
        pv = pv.roll(k, 3) * (1.0 - 0.1 * k) + 0.05 * torch.randn(pv.shape, generator=g)
        y = y.roll(k, 2) + 0.05 * torch.randn(y.shape, generator=g)
        t = t * (1.0 - 0.2 * k) + 0.03 * k
    return pv.contiguous(), t.contiguous(), y.contiguous()


def build_model(name, train=False):
    """-> (model, its FusedAdamW or None)"""
    import emu_session
    kw, compute, _ = MODELS[name]
    model = synth_model(ScOTConfig(**kw), compute, train=train)
    opt = emu_session.fused_adamw(model, lr=1e-3, weight_decay=0.01, max_grad_norm=5.0) if train else None
    return model, opt


_cache = {}


def exported(name, train=False, streams=2):
    """one export per (model, kind, streams) for the whole module"""
    key = (name, train, streams)
    if key not in _cache:
        model, opt = build_model(name, train)
        pv, t, y = inputs(name)
        kw = dict(labels=y, train=opt) if train else {}
        _cache[key] = model.export_plan(pv, time=t, streams=streams, **kw) if streams != "default" else model.export_plan(pv, time=t, **kw)
    return _cache[key]


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
    st = dict(arena=model._arena.data, exp_avg=opt.exp_avg, exp_avg_sq=opt.exp_avg_sq, step_state=opt._step_state)
    if model._engine.scale_state is not None:
        st["scale_state"] = model._engine.scale_state
    return st


# ------------------------------------------------------------------------------------------------------- an image's lists as tapes
def image_records(image, which):
    """one call list of an image -> [(byte offset, name, [(tag, value)])]"""
    h = Plan.header(image)
    names = [image[h[H.H_NAMES_OFF] + i * H.NAME_BYTES:][:H.NAME_BYTES].split(b"\0")[0].decode() for i in range(h[H.H_NNAMES])]
    out = []
    for off, name, ni in entry_records(image, which):
        pairs = struct.unpack_from(f"<{2 * ni}Q", image, off + 32)
        out.append((off, names[name], [(pairs[2 * k] & 0xFF, pairs[2 * k + 1]) for k in range(ni)]))
    return out


def image_entries(image, which):
    """one call list of an image -> tape_schedule entries: the stream is the STREAM pair's index, the event the EVENT pair's"""
    out = []
    for i, (_, name, pairs) in enumerate(image_records(image, which)):
        streams = [v for tag, v in pairs if tag == H.ARG_STREAM]
        events = [v for tag, v in pairs if tag == H.ARG_EVENT]
        assert len(streams) == 1, (which, i, name)      # every listed entry point takes exactly one stream
        if name == H.RECORD:
            assert [tag for tag, _ in pairs] == [H.ARG_EVENT, H.ARG_STREAM]
            out.append(ts.Entry(i, ts.RECORD, streams[0], events[0]))
        elif name == H.WAIT:
            assert [tag for tag, _ in pairs] == [H.ARG_STREAM, H.ARG_EVENT]
            out.append(ts.Entry(i, ts.WAIT, streams[0], events[0]))
        else:
            assert not events, (which, i, name)
            out.append(ts.Entry(i, ts.LAUNCH, streams[0], None))
    return out


def closed(entries):
    """the closed-list rule, from the entries alone: a wait pairs with an earlier record; stream 1 starts behind a record of stream 0 and
    its last entry is a record that stream 0 waits for afterwards"""
    side = [e for e in entries if e.stream == 1]
    recs = {}
    for e in entries:
        if e.kind == ts.RECORD:
            recs[e.event] = e
        elif e.kind == ts.WAIT and e.event not in recs:
            return False
    if not side:
        return True
    first, last = side[0], side[-1]
    by_event = {}
    for e in entries:
        if e.kind == ts.RECORD:
            by_event.setdefault(e.event, []).append(e)
    forked = first.kind == ts.WAIT and any(r.stream == 0 and r.index < first.index for r in by_event.get(first.event, []))
    joined = last.kind == ts.RECORD and any(e.kind == ts.WAIT and e.stream == 0 and e.event == last.event and e.index > last.index for e in entries)
    return forked and joined


def orders(entries):
    yield "late", ts.late(entries, 1)
    yield "early", ts.early(entries, 1)
    for seed in SEEDS:
        yield f"random {seed}", ts.random(entries, seed)


# ------------------------------------------------------------------------------------------------------- the images
def test_default_exports_are_unchanged(emu):
    """without streams= (and with streams=1) the exporter writes what it wrote: formats 1 and 4, byte for byte"""
    for train in (False, True):
        a, b = exported("small", train, "default"), exported("small", train, 1)
        assert a == b and Plan.header(a)[H.H_FORMAT] == (4 if train else 1) and Plan.header(a)[H.H_STREAMS_OFF] == 0
        assert H.RECORD not in names_of(a, "forward")


@pytest.mark.parametrize("name", ["small", "c96"])
def test_streamed_images(emu, name):
    for train, fmt, lists in ((False, 5, ("forward",)), (True, 6, ("forward", 0, 1, 2))):
        image = exported(name, train)
        h = Plan.header(image)
        assert h[H.H_FORMAT] == fmt and h[H.H_STREAMS_OFF]
        n_streams, n_events = struct.unpack_from("<2Q", image, h[H.H_STREAMS_OFF])
        assert n_streams == 2 and n_events >= 1
        plan = Plan.load(image)      # (the validator has passed every list)
        assert plan.describe()["format"] == fmt
        assert plan.describe_streams() == dict(streams=2, events=n_events, overlaps=0, host_stream=0)
        plan.free()
        seen = set()
        for which in lists:
            entries = image_entries(image, which)
            assert closed(entries), which
            assert all(e.stream in (0, 1) and (e.event is None or e.event < n_events) for e in entries)
            st = ts.structure(entries, main=0)
            assert not st["unpaired_waits"] and not st["opaque"] and all(st["joined"].values())
            seen |= {e.event for e in entries if e.event is not None}
        assert seen == set(range(n_events))
        fwd = image_entries(image, "forward")
        assert {e.stream for e in fwd if e.kind == ts.LAUNCH} == {0, 1} and any(e.kind == ts.RECORD for e in fwd)
        if train:      # the weight gradients run on the side stream
            bwd = image_records(image, 1)
            wg = [(name_, [v for tag, v in pairs if tag == H.ARG_STREAM]) for _, name_, pairs in bwd if name_ in WEIGHT_GRADIENTS]
            assert len({n for n, _ in wg}) >= 3 and all(s == [1] for _, s in wg), wg
            if name == "c96":
                assert {"scot_wgrad_group", "scot_wgrad_mlp"} <= {n for n, _ in wg}
    if name == "c96":
        assert "scot_block_tail_fwd" in names_of(exported(name), "forward") and "scot_dwconv7" in names_of(exported(name), "forward")


# ------------------------------------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("name", ["small", "c96"])
def test_prediction_is_the_one_stream_plans_and_the_models(emu, name):
    model, _ = build_model(name)
    two, one = Plan.load(exported(name)), Plan.load(exported(name, streams=1))
    for k in (1, 0):
        pv, t, _ = inputs(name, k)
        with torch.no_grad():
            ref = model(pv, time=t).output
        two.poison(0xFF)
        got = two.run(pv, t)
        assert torch.equal(got, ref) and torch.equal(got, one.run(pv, t))
    two.free()
    one.free()


def test_training_steps_are_the_python_loops(emu):
    name = "small"
    image = exported(name, train=True)
    model, opt = build_model(name, train=True)
    plan = Plan.load(image)
    assert plan.describe_training()["has_training"] == 1
    for k in range(3):
        b, lr = inputs(name, k), rates(opt, k)
        plan.poison(0xFF)
        ref = python_step(model, opt, b, lr)
        got = plan.train_step(*b, lr)
        assert torch.isfinite(ref).all() and torch.equal(got, ref), k
        state, want = plan_mod.training_state(plan.snapshot(image)), python_state(model, opt)
        for key in STATE:
            assert (key in state) == (key in want) and (key not in want or torch.equal(state[key], want[key])), (k, key)
    st = plan.train_status()
    assert (st["applied"], st["skipped"]) == (3, 0) and st["grad_scale"] == model._engine.grad_scale_value()
    plan.free()


# ------------------------------------------------------------------------------------------------------- legal orders
@pytest.mark.parametrize("name", ["small", "c96"])
def test_every_legal_order_of_the_forward_gives_the_same_bits(emu, name):
    image = exported(name)
    entries = image_entries(image, "forward")
    plan = Plan.load(image)
    pv, t, _ = inputs(name)
    canonical = plan.run(pv, t).clone()
    moved = 0
    for label, order in orders(entries):
        ts.check(order, entries)
        moved += order != ts.canonical(entries)
        plan.issue_order(LISTS["forward"], None)
        plan.run(*other_inputs(pv, t))
        plan.issue_order(LISTS["forward"], order)
        assert torch.equal(plan.run(pv, t), canonical), label
    assert moved >= 4
    plan.issue_order(LISTS["forward"], None)
    assert torch.equal(plan.run(pv, t), canonical)
    plan.free()


def test_every_legal_order_of_a_training_step_gives_the_same_bits(emu):
    name = "small"
    image = exported(name, train=True)
    tapes = {which: image_entries(image, which) for which in (0, 1, 2)}
    model, opt = build_model(name, train=True)
    b, other, lr = inputs(name, 0), inputs(name, 2), rates(opt, 1)
    plan = Plan.load(image)
    plan.train_step(*other, lr)
    ref_loss = plan.train_step(*b, lr).clone()
    ref = plan_mod.training_state(plan.snapshot(image))
    plan.free()
    generated = {which: dict(orders(tapes[which])) for which in tapes}
    # (the engine issues a side-stream task the moment it forks it, so `early` can be the recorded order itself; `late` never is)
    assert generated[1]["late"] != ts.canonical(tapes[1]) and sum(o != ts.canonical(tapes[1]) for o in generated[1].values()) >= 4
    for label in generated[1]:
        plan = Plan.load(image)
        plan.train_step(*other, lr)
        for which in tapes:
            ts.check(generated[which][label], tapes[which])
            plan.issue_order(LISTS[which], generated[which][label])
        loss = plan.train_step(*b, lr)
        got = plan_mod.training_state(plan.snapshot(image))
        assert torch.equal(loss, ref_loss) and all(torch.equal(got[k], ref[k]) for k in ref), label
        plan.free()


def test_a_missing_edge_is_seen(emu):
    """CPU only: an order that is legal once one event edge is taken out of the constraint set reads stale (in-bounds) memory of the
    emulated slab — the join of the skip blocks: the decoder reads the skip before the side stream has written it; their fork: the
    side stream reads the encoder stage's output before the main stream has written it"""
    name = "c96"
    image = exported(name)
    entries = image_entries(image, "forward")
    by = {e.index: e for e in entries}
    pairs, _ = ts._pairs(entries)
    joins = [w for r, w in pairs if by[r].stream == 1 and by[w].stream == 0]
    forks = [w for r, w in pairs if by[r].stream == 0 and by[w].stream == 1]
    assert len(joins) >= 2 and len(forks) >= 2
    plan = Plan.load(image)
    pv, t, _ = inputs(name)
    canonical = plan.run(pv, t).clone()
    for what, wait in (("join", joins[-1]), ("fork", forks[-1])):
        reduced = ts.without(entries, wait)
        changed = []
        for label, order in orders(reduced):
            order = list(order) + [wait]      # (the wait itself does nothing on the emulation: issued last)
            with pytest.raises(ts.ScheduleError):
                ts.check(order, entries)
            plan.issue_order(LISTS["forward"], None)
            plan.run(*other_inputs(pv, t))
            plan.issue_order(LISTS["forward"], order)
            got = plan.run(pv, t)
            changed.append(not torch.equal(got, canonical))
            if changed[-1]:      # (one order that shows it is what is asked for)
                break
        assert any(changed), what
    plan.free()


# ------------------------------------------------------------------------------------------------------- refusals
def test_refusals_issue_nothing(emu):
    model, _ = build_model("small")
    pv, t, _ = inputs("small")
    one, two = Plan.load(exported("small", streams=1)), Plan.load(exported("small"))
    before = issued(one)
    with pytest.raises(PlanExportError, match="adjoint.*streams=2"):
        model.export_plan(pv, time=t, adjoint=("pixel_values",), streams=2)
    with pytest.raises(PlanExportError, match="streams=3"):
        model.export_plan(pv, time=t, streams=3)
    assert one._lib.scot_plan_set_side_stream(one._h, ctypes.c_void_p(8)) == -3
    assert one.describe_streams() == dict(streams=1, events=0, overlaps=0, host_stream=0)
    n = two.describe()["calls"]
    order = (ctypes.c_int * n)(*([0, 0] + list(range(2, n))))
    assert two._lib.scot_plan_issue_order(two._h, 0, ctypes.cast(order, ctypes.c_void_p), n) == -1
    assert two._lib.scot_plan_issue_order(two._h, 0, ctypes.cast(order, ctypes.c_void_p), n - 1) == -1
    assert two._lib.scot_plan_issue_order(two._h, 5, ctypes.cast(order, ctypes.c_void_p), n) == -1
    assert issued(one) == before
    # a side stream of the host's: taken between the load and the first run, refused afterwards
    assert two._lib.scot_plan_set_side_stream(two._h, ctypes.c_void_p(16)) == 0 and two.describe_streams()["host_stream"] == 1
    ref = one.run(pv, t)
    assert torch.equal(two.run(pv, t), ref)
    assert two._lib.scot_plan_set_side_stream(two._h, ctypes.c_void_p(24)) == -1
    one.free()
    two.free()


# ------------------------------------------------------------------------------------------------------- corrupt images
def pair_at(image, which, want_name, want_tag, nth=0):
    """byte offset of the `nth` argument pair with tag `want_tag` among the entries called `want_name` (None: any) of a list"""
    for off, name, pairs in image_records(image, which):
        if want_name is None or name == want_name:
            for k, (tag, _) in enumerate(pairs):
                if tag == want_tag:
                    if nth == 0:
                        return off + 32 + 16 * k
                    nth -= 1
    raise AssertionError((which, want_name, want_tag))


def without_entry(image, which, index):
    """the image with entry `index` of a call list cut out: the list's later entries move up, its count and words shrink"""
    recs = image_records(image, which)
    n, start = call_list(image, which)
    end = recs[-1][0] + 8 * (4 + 2 * len(recs[-1][2]) + word(image, recs[-1][0] + 24))
    off = recs[index][0]
    size = (recs[index + 1][0] if index + 1 < len(recs) else end) - off
    b = bytearray(image)
    b[off:end] = image[off + size:end] + bytes(size)
    assert which == "forward"
    b[8 * H.H_NENTRIES:8 * H.H_NENTRIES + 8] = struct.pack("<Q", n - 1)
    b[8 * H.H_ENTRIES_WORDS:8 * H.H_ENTRIES_WORDS + 8] = struct.pack("<Q", Plan.header(image)[H.H_ENTRIES_WORDS] - size // 8)
    return bytes(b)


def swapped(image, which, index):
    """the image with entries `index` and `index + 1` of a call list (of one size) exchanged"""
    recs = image_records(image, which)
    a, c = recs[index][0], recs[index + 1][0]
    size = c - a
    b = bytearray(image)
    b[a:a + size], b[c:c + size] = image[c:c + size], image[a:a + size]
    return bytes(b)


def corrupt_images():
    inf, tr, plain, plain_tr = exported("small"), exported("small", True), exported("small", streams=1), exported("small", True, 1)
    h = Plan.header(inf)
    n_events = word(inf, h[H.H_STREAMS_OFF] + 8)
    fwd = image_entries(inf, "forward")
    by = {e.index: e for e in fwd}
    pairs, _ = ts._pairs(fwd)
    fork = next((r, w) for r, w in pairs if w == r + 1 and by[r].stream == 0 and by[w].stream == 1)      # record, then its wait
    closing = [w for r, w in pairs if by[r].stream == 1 and by[w].stream == 0][-1]
    inference_only = max(e.event for e in fwd if e.event is not None)      # an event of the inference forward of the training image
    assert all(e.event != inference_only for e in image_entries(tr, 0) if e.kind == ts.RECORD)
    names = [plain[Plan.header(plain)[H.H_NAMES_OFF] + i * H.NAME_BYTES:][:H.NAME_BYTES].split(b"\0")[0].decode()
             for i in range(Plan.header(plain)[H.H_NNAMES])]
    return {
        "accepted: format 5": (inf, 0),
        "accepted: format 6": (tr, 0),
        "stream index 2": (patched(inf, pair_at(inf, "forward", "scot_gemm", H.ARG_STREAM) + 8, 2), -1),
        "event index = the event count": (patched(inf, pair_at(inf, "forward", H.RECORD, H.ARG_EVENT) + 8, n_events), -1),
        "a wait in front of its record": (swapped(inf, "forward", fork[0]), -1),
        "a wait whose record is in another list": (patched(tr, pair_at(tr, 0, H.WAIT, H.ARG_EVENT) + 8, inference_only), -1),
        "the closing join removed": (without_entry(inf, "forward", closing), -1),
        "an EVENT pair on scot_gemm": (patched(patched(inf, pair_at(inf, "forward", "scot_gemm", H.ARG_INT), H.ARG_EVENT),
                                               pair_at(inf, "forward", "scot_gemm", H.ARG_INT) + 8, 0), -1),
        "a record entry in a format-1 image": (renamed(plain, names.index("scot_add"), H.RECORD), -3),
        "stream value 1 in a format-4 image": (patched(plain_tr, pair_at(plain_tr, 1, None, H.ARG_STREAM) + 8, 1), -1),
        "stream value 1 in a format-1 image": (patched(plain, pair_at(plain, "forward", None, H.ARG_STREAM) + 8, 1), -1),
        "a truncated streams section": (patched(inf, 8 * H.H_STREAMS_OFF, len(inf) - 8), -1),
        "three streams": (patched(inf, h[H.H_STREAMS_OFF], 3), -1),
    }


def test_corrupt_images_are_refused_before_anything_is_issued(emu, tmp_path):
    cases = corrupt_images()
    probe = Plan.load(exported("small", streams=1))
    before = issued(probe)
    for label, (data, status) in cases.items():
        if status == 0:
            continue
        handle = ctypes.c_void_p()
        assert plan_mod.load_raw(emu, data, handle) == status and not handle.value, label
    assert issued(probe) == before
    probe.free()
    check_images_stand_alone(tmp_path, cases)
