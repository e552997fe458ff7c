"""The recorded forward and backward replayed in every kind of legal stream order (tests/tape_schedule.py) on the MI355X.

The engine orders its two HIP streams with ~130 event edges per step and reuses buffers by address.  On the GPU a missing edge is a
race that usually goes the right way: side-stream work is issued right behind its fork and the main chain is long.  Here the tape's
entries are issued from Python in a chosen legal order with a device synchronisation at every stream switch, so the GPU executes
exactly that order: side-stream work as late as its join allows (`late`: a buffer reused on the main stream while a queued weight
gradient still reads it), as early as its fork allows (`early`: a consumer whose wait is missing runs ahead of its producer), and
seeded random interleavings.  Every order must give the result of the tape's own order.

Protocol per configuration: the engine is brought to a `ready` tape by ordinary steps; a run copies inputs into the recorded input
buffers, clears the gradient arena the way the recorded backward variant expects, issues the forward order then the backward order and
clones loss, prediction, gradient arena (and input gradients).  Every compared run on inputs B follows a canonical run on inputs A, so
every recorded buffer holds the OTHER inputs' values: a consumer that runs ahead of its producer reads wrong data, not merely old data.
Bound: the project's own (test_lazy_zero_grad_equals_the_eager_fill): 4 x floor + 2e-5, floor = what canonical runs differ by
(float atomics commit in any order; the largest of several repeats, see canonical_floor), measured here and never on the schedule under test.

What a pass means: the event edges of the recorded forward and backward order every producer before its consumers and every reader
before the overwrite, at entry-point granularity.  Not covered: hazards between the launches inside one C call, the unrecorded first
steps, the optimizer and the overlapped gradient fill outside the tapes, data-parallel callbacks.  Measured values:
profiles/tape_schedules/README.md."""
import time as _time

import pytest
import torch

pytestmark = pytest.mark.gpu

import tape_schedule as ts  # noqa: E402
from poseidon_amd import lib as scot_lib  # noqa: E402
from poseidon_amd import ops  # noqa: E402
from poseidon_amd.config import ScOTConfig  # noqa: E402
from poseidon_amd.geometry import param_shapes  # noqa: E402
from poseidon_amd.synth import synth_inputs, synth_state_dict  # noqa: E402
from scOT.model import ScOT  # noqa: E402
from test_input_grads_gpu import SAME_STEP  # noqa: E402
from test_model_gpu import DEV, _preset_model  # noqa: E402

SEEDS = range(8)
# upstream gradients of the two input sets.  (Not above 1: Poseidon-T's fp16 backward runs under the gradient scale 2^17, and with twice the
# upstream gradient on the B inputs a query gradient of stage 0 leaves binary16's range — through the public API just the same; the
# dynamic scale's business, not this test's.)
DLOSS_A, DLOSS_B = 1.0, 0.5
# host callables a recorded backward may hold, all at its head: the wait for an overlapped gradient fill, the fp16 pre-scale of gradients
# already in the arena, and the fp16 multiply of the caller's dloss by the gradient scale (a torch call: the lambda of _backward_chain)
HEAD_OPAQUE = {"fill_done", "prescale", "<lambda>"}


def replay_in_order(cmds, order, entries=None):
    """Issue the tape's entries from Python in `order` (checked against the constraints first): torch.cuda.synchronize() whenever the
    stream of the next entry differs from the previous one's, after every opaque entry, and at the end; a non-zero status raises.
    Stream handles, scratch addresses and events stay as recorded.  `entries`: the parsed tape when an entry was taken out of it."""
    if entries is None:
        entries = ts.parse(cmds, scot_lib.PROTOTYPES)
    return ts.issue(cmds, order, entries, sync=torch.cuda.synchronize)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


class RecordedStep:
    """one model brought to a `ready` step tape, and runs of that tape in chosen orders"""

    def __init__(self, model, kw, lazy=False, input_grads=False):
        self.model, self.lazy, self.input_grads = model, lazy, input_grads
        self.A = {k: v.detach().clone() for k, v in kw.items()}
        self.B = {k: (v * 1.25 + 0.01) for k, v in self.A.items()}
        for step in range(3):          # direct, recording, replayed — as test_step_tape_replay_matches_direct_launches
            self._ordinary_step(False, step)
        if lazy:                       # the second recorded backward: first writers store
            for step in range(2):
                self._ordinary_step(True, step)
        torch.cuda.synchronize()
        self.eng, self.arena = model._engine, model._arena
        ents = [e for e in self.eng._taped.values() if e.get("state") == "ready"]
        assert len(ents) == 1
        self.ent = ents[0]
        assert self.eng.use_side and self.eng.side is not None
        self.main, self.side = torch.cuda.current_stream().cuda_stream, self.eng.side.cuda_stream
        assert self.main != self.side
        self.fwd = self.ent["fwd"]
        self.bwd = {v: rec for v, (rec, _) in self.ent["bwd"].items()}
        assert set(self.bwd) == ({False, True} if lazy else {False})
        self.efwd = ts.parse(self.fwd, scot_lib.PROTOTYPES)
        self.ebwd = {v: ts.parse(rec, scot_lib.PROTOTYPES) for v, rec in self.bwd.items()}
        if lazy:
            self.small = torch.zeros(self.arena.size, dtype=torch.bool, device=DEV)
            for o, n in self.eng._small_chunks[0].tolist():
                self.small[o:o + n] = True

    def _ordinary_step(self, lazy, step):
        kw = {k: (v * (1.0 + 0.25 * step) + 0.01 * step) for k, v in self.A.items()}
        if self.input_grads:
            kw = {k: v.requires_grad_(k != "labels") for k, v in kw.items()}
        self.model.zero_grad(overlap=True) if lazy else self.model.zero_grad()
        out = self.model(**kw)
        (out.loss / (1.0 + step)).backward()          # a different upstream gradient every step

    def run(self, inputs, dloss, variant, fwd_order, bwd_order, bwd_entries=None):
        ent, eng = self.ent, self.eng
        for dst, src in zip(ent["in"], (inputs["pixel_values"], inputs.get("time"), inputs["labels"], None)):
            if dst is not None:
                dst.copy_(src)
        if variant:                    # ScOT.zero_grad(overlap=True): only the accumulated part is filled; whatever the rest holds must be stored over
            self.arena.grad[~self.small] = float("nan")
            self.arena.grad[self.small] = 3.0
            self.model.zero_grad(overlap=True)
        else:
            self.arena.grad.fill_(7.0)
            self.model.zero_grad()
        torch.cuda.synchronize()
        prev = ops.use(eng.lib_kind)
        try:
            n = replay_in_order(self.fwd, fwd_order, self.efwd)
            ent["dloss"].fill_(dloss)
            n += replay_in_order(self.bwd[variant], bwd_order, self.ebwd[variant] if bwd_entries is None else bwd_entries)
        finally:
            ops.use(prev)
            eng.grads_are_zero = eng.lazy_grads = False
        torch.cuda.synchronize()
        res = dict(loss=ent["out"][0].clone(), pred=ent["out"][1].clone(), grad=self.arena.grad.clone(), syncs=n)
        if self.input_grads:
            res["d_pixel_values"], res["d_time"] = (t.clone() for t in ent["igrads"][variant])
        return res

    def canonical(self, variant):
        return ts.canonical(self.efwd), ts.canonical(self.ebwd[variant])

    def distance(self, got, ref):
        keys = ["grad", "loss", "pred"] + (["d_pixel_values", "d_time"] if self.input_grads else [])
        for k in keys:
            assert bool(torch.isfinite(got[k]).all()), f"{k} is not finite"
        return {k: rel(got[k], ref[k]) for k in keys}

    def worst_tensors(self, got, ref, top=5):
        d, r = (got["grad"] - ref["grad"]).double().cpu(), float(ref["grad"].double().norm())
        per = []
        for name in self.arena.shapes:
            g = self.arena.gview(name)                               # (the name's place in the gradient arena)
            o = (g.data_ptr() - self.arena.grad.data_ptr()) // 4
            per.append((float(d[o:o + g.numel()].norm()) / r, name))
        return [(f"{v:.2e}", n) for v, n in sorted(per, reverse=True)[:top]]


def describe(cmds, indices):
    return [(j, ts.entry_name(cmds[j][0])) for j in indices]


def check_structure(tag, cmds, entries, main, side, backward):
    """structural facts of one tape, and what keeps the schedules from passing without checking anything -> (summary, late order)"""
    s = ts.structure(entries, main)
    assert set(s["per_stream"]) <= {main, side}, s["per_stream"]
    assert not s["unpaired_waits"], describe(cmds, s["unpaired_waits"])            # every wait has its record in the same tape
    if s["rerecorded"]:       # (the engine takes a fresh event per edge; if it ever reuses one, the waits of the first record must stay ahead of the second)
        assert any(why == "re-record" for _, _, why in ts.constraints(entries))
        print(f"[{tag}] {len(s['rerecorded'])} event(s) recorded more than once: re-record constraints in force")
    assert all(s["joined"].values()), s["joined"]                                  # the tape ends joined
    assert not ts.shared_workspaces(ts.workspace_ranges(cmds, entries))            # no scratch range handed to both streams
    names = [ts.entry_name(cmds[j][0]) for j in s["opaque"]]
    if backward:
        first_launch = next(e.index for e in entries if e.kind == ts.LAUNCH and ts.entry_name(cmds[e.index][0]) == "scot_loss_bwd")
        assert set(names) <= HEAD_OPAQUE and "fill_done" in names and all(j < first_launch for j in s["opaque"]), list(zip(s["opaque"], names))
        assert s["per_stream"].get(side, {}).get(ts.LAUNCH, 0) >= 1
    else:
        assert not names, list(zip(s["opaque"], names))      # drop_path_rate 0, no pixel mask: nothing of the forward is a host step
    lt = ts.late(entries, side)
    over = ts.overtaken(lt, entries, main, side)
    regions = ts.fork_regions(entries, main, side)
    for r in regions:
        assert r["join"] is not None
        if r["passable"]:       # the join is not the very next main-stream launch: `late` must carry side-stream work past main-stream work
            assert any(over[x] > 0 for x in r["launches"]), (tag, describe(cmds, r["launches"][:4]), r["fork"], r["join"])
    moved = sum(1 for x in over.values() if x > 0)
    per = s["per_stream"]
    summary = dict(main=per.get(main), side=per.get(side), event_edges=s["event_edges"], opaque=list(zip(s["opaque"], names)),
                   regions=len(regions), passable_regions=sum(1 for r in regions if r["passable"]), side_launches=len(over), moved=moved)
    print(f"[{tag}] main {per.get(main)} side {per.get(side)} event edges {s['event_edges']} opaque {summary['opaque']} "
          f"fork regions {len(regions)} ({summary['passable_regions']} with main-stream launches to pass); "
          f"late(side) moves {moved}/{len(over)} side launches past main-stream launches")
    return summary


FLOOR_RUNS = 6


def canonical_floor(step, variant, ref):
    """What canonical(A)-then-canonical(B) replays differ from `ref` by, per compared quantity: the largest of FLOOR_RUNS repeats.
    One repeat is not a floor.  Measured on the MI355X (Poseidon-T fp16, 10 repeats each of the serialised canonical order, the engine's
    own unsynchronised replay and late(side)): a run lands on one of a few discrete results — float atomics on the chain commit in one of
    a few orders and the 16-bit roundings downstream follow — so its distance from `ref` is either 1.4e-4 .. 2.0e-4 or, when it lands on
    `ref`'s own result (2 to 3 runs in 10, in all three kinds of run alike), 2e-8.  A floor taken from one such repeat put the bound
    at 2.0e-5 under schedules that sat at 1.8e-4 like every other run."""
    canon = step.canonical(variant)
    worst = None
    for _ in range(FLOOR_RUNS):
        step.run(step.A, DLOSS_A, variant, *canon)
        d = step.distance(step.run(step.B, DLOSS_B, variant, *canon), ref)
        worst = d if worst is None else {k: max(worst[k], d[k]) for k in d}
    return worst


def run_schedules(tag, step, variant):
    t0 = _time.time()
    A, B = step.A, step.B
    canon = step.canonical(variant)
    sf = check_structure(f"{tag} forward", step.fwd, step.efwd, step.main, step.side, backward=False)
    sb = check_structure(f"{tag} backward", step.bwd[variant], step.ebwd[variant], step.main, step.side, backward=True)
    step.run(A, DLOSS_A, variant, *canon)
    ref = step.run(B, DLOSS_B, variant, *canon)
    floors = canonical_floor(step, variant, ref)
    floor = floors["grad"]
    bound = 4.0 * floor + 2e-5
    # Loss and prediction are held to the arena's bound.  The input gradients are not: d_time is one float per sample at the end of the whole
    # 16-bit chain, so its distance between two runs is a ratio of a few rounding realisations, not an average over millions of elements —
    # four times ONE measured floor is exceeded by chance.  They are held to the project's bound for the input gradients of two runs of one
    # fp16 step (SAME_STEP of tests/test_input_grads_gpu.py: 1e-2; fp32: 1e-5); a misordered run computes them from the other inputs, O(1).
    bounds = {k: (SAME_STEP[step.model.compute] if k in ("d_pixel_values", "d_time") else bound) for k in floors}
    ef, eb = step.efwd, step.ebwd[variant]
    schedules = [("late(side)", ts.late(ef, step.side), ts.late(eb, step.side)), ("early(side)", ts.early(ef, step.side), ts.early(eb, step.side))]
    schedules += [(f"random({seed})", ts.random(ef, seed), ts.random(eb, 1000 + seed)) for seed in SEEDS]
    worst = {k: (0.0, "") for k in floors}
    failures = []
    for name, of, ob in schedules:
        step.run(A, DLOSS_A, variant, *canon)
        got = step.run(B, DLOSS_B, variant, of, ob)
        d = step.distance(got, ref)
        for k, v in d.items():
            if v > worst[k][0]:
                worst[k] = (v, name)
            if not v < bounds[k]:
                failures.append((name, k, f"{v:.3e} against {bounds[k]:.3e}", step.worst_tensors(got, ref), "forward moved furthest:",
                                 describe(step.fwd, [j for j, _ in ts.displaced(of, ef)]), "backward moved furthest:",
                                 describe(step.bwd[variant], [j for j, _ in ts.displaced(ob, eb)])))
    secs = _time.time() - t0
    print(f"[{tag}] floor {floor:.2e} bound {bound:.2e}; worst of {len(schedules)} schedules {worst['grad'][0]:.2e} ({worst['grad'][1]}); {secs:.1f} s")
    for k in floors:
        if k != "grad":
            print(f"[{tag}]   {k}: floor {floors[k]:.2e} bound {bounds[k]:.2e} worst {worst[k][0]:.2e} ({worst[k][1]})")
    assert bound < 2e-2, (floor, bound)
    assert not failures, failures
    return sf, sb


def small_fp32_model():
    """the conditioned 32x32, embed 16, depths [2, 2] model of test_overlapped_gradient_fill_is_ordered_before_the_backward, batch 2"""
    cfg = ScOTConfig(image_size=32, patch_size=4, num_channels=4, num_out_channels=4, embed_dim=16, depths=[2, 2], num_heads=[1, 2],
                     skip_connections=[1, 0], window_size=4, mlp_ratio=4.0, p=1, channel_slice_list_normalized_loss=[0, 1, 3, 4],
                     drop_path_rate=0.0, use_conditioning=True)
    model = ScOT(cfg, compute="fp32")
    model.load_state_dict(synth_state_dict(param_shapes(cfg), "trained"))
    pv, t, lab = synth_inputs(2, 4, 4, 32, "smooth")
    return model.to(DEV), dict(pixel_values=pv.to(DEV), time=t.to(DEV), labels=lab.to(DEV))


def poseidon_t():
    """Poseidon-T fp16 at 128x128, 4 channels, batch 2, on the fused layer tails the timed batches run"""
    _, _, model = _preset_model("T", 128, 4, "fp16", engine_options={"fused_min_rows": 0})
    pv, t, lab = synth_inputs(2, 4, 4, 128, "smooth")
    return model, dict(pixel_values=pv.to(DEV), time=t.to(DEV), labels=lab.to(DEV))


def on_stream(cmds, entries, name):
    return {e.stream for e in entries if e.kind == ts.LAUNCH and ts.entry_name(cmds[e.index][0]) == name}


def test_small_fp32_model_in_every_schedule():
    model, kw = small_fp32_model()
    step = RecordedStep(model, kw)
    run_schedules("small fp32", step, False)


@pytest.fixture(scope="module")
def poseidon_t_step():
    model, kw = poseidon_t()
    return RecordedStep(model, kw, lazy=True)


@pytest.mark.parametrize("variant", [False, True], ids=["eager_fill", "first_writers_store"])
def test_poseidon_t_fp16_in_every_schedule(poseidon_t_step, variant):
    step = poseidon_t_step
    cmds, entries = step.bwd[variant], step.ebwd[variant]
    # the lean-tail path of the timed batches: fused backward tail on the chain, its weight gradients and the norms' partial sums beside it
    assert on_stream(cmds, entries, "scot_block_tail_bwd") == {step.main}
    assert on_stream(cmds, entries, "scot_wgrad_mlp") == {step.side}
    assert on_stream(cmds, entries, "scot_partial_colsum_batch") == {step.side}
    run_schedules(f"Poseidon-T fp16 {'store' if variant else 'eager'}", step, variant)
    assert int(step.eng.grad_overflow) == 0


def test_poseidon_t_fp16_with_input_gradients_in_every_schedule():
    model, kw = poseidon_t()
    step = RecordedStep(model, kw, input_grads=True)
    cmds, entries = step.bwd[False], step.ebwd[False]
    assert on_stream(cmds, entries, "scot_cln_dtime") == {step.main, step.side}      # the two rows of the time accumulator, one per stream
    run_schedules("Poseidon-T fp16 input gradients", step, False)
    assert int(step.eng.grad_overflow) == 0


LAYOUT_ARG, ACCUMULATE_ARG = 0, 24      # scot_gemm: `layout` is its first argument, `accumulate` its 25th (include/scot_hip.h)


def is_weight_gradient_gemm(cmd):
    fn, args = cmd
    name = ts.entry_name(fn)
    return name == "scot_wgrad_group" or (name == "scot_gemm" and args[LAYOUT_ARG] == ops.TN and args[ACCUMULATE_ARG] == 1)


def test_a_removed_wait_is_detected_on_the_real_tape():
    """The method finds a missing edge on the engine's own tape: without the side stream's wait in front of the first weight-gradient
    GEMMs of the backward, `early(side)` runs them ahead of the main-stream kernels that produce their operands — on the previous
    step's activations — and the gradient arena leaves the bound.  The dependants of the removed edge are weight-gradient GEMMs only:
    they read activations and write the gradient arena (no index table, no pointer array), so the reordered run touches allocated
    memory only.  Run once."""
    model, kw = small_fp32_model()
    step = RecordedStep(model, kw)
    cmds, entries = step.bwd[False], step.ebwd[False]
    groups, cur = [], None
    for e in entries:                  # the side stream's launches, grouped by the wait that orders them behind the main chain
        if e.stream != step.side:
            continue
        if e.kind == ts.WAIT:
            cur = (e.index, [])
            groups.append(cur)
        elif e.kind == ts.LAUNCH and cur is not None:
            cur[1].append(e.index)
    pick = next(((w, ls) for w, ls in groups if ls and all(is_weight_gradient_gemm(cmds[j]) for j in ls)), None)
    assert pick is not None, [(w, describe(cmds, ls)) for w, ls in groups[:6]]
    wait, launches = pick
    first = next(j for _, ls in groups for j in ls if is_weight_gradient_gemm(cmds[j]))
    print(f"\n[removed wait] entry {wait} orders {describe(cmds, launches)}; the tape's first weight-gradient GEMM is entry {first}")
    canon = step.canonical(False)
    step.run(step.A, DLOSS_A, False, *canon)
    ref = step.run(step.B, DLOSS_B, False, *canon)
    floor = canonical_floor(step, False, ref)["grad"]
    bound = 4.0 * floor + 2e-5
    cut = ts.without(entries, wait)
    order = ts.early(cut, step.side)
    pos = {j: p for p, j in enumerate(order)}
    rec = next(a for a, b, why in ts.constraints(entries) if b == wait and why == "event")
    assert pos[launches[0]] < pos[rec]          # the GEMMs now run ahead of the point they were forked from
    step.run(step.A, DLOSS_A, False, *canon)
    got = step.run(step.B, DLOSS_B, False, canon[0], order, bwd_entries=cut)
    d = step.distance(got, ref)["grad"]
    print(f"[removed wait] floor {floor:.2e} bound {bound:.2e}; early(side) without the wait: {d:.2e}; tensors {step.worst_tensors(got, ref, 3)}")
    assert bound < 2e-2
    assert d > bound, (d, bound)
    # ... and the intact tape in the same order kind stays inside it (the same run as in test_small_fp32_model_in_every_schedule)
    step.run(step.A, DLOSS_A, False, *canon)
    ok = step.distance(step.run(step.B, DLOSS_B, False, canon[0], ts.early(entries, step.side)), ref)["grad"]
    assert ok < bound, (ok, bound)
