"""tests/tape_schedule.py without a GPU: the linearisations against a brute-force enumeration of every legal order of small synthetic
tapes, and the whole method end to end on the emulated library — a hand-built two-stream tape gives bit-identical results in every
legal order, and with either of its two waits taken out one of the generated orders changes the result (a consumer ahead of its
producer; a reader behind the overwrite)."""
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
import tape_schedule as ts  # noqa: E402
from poseidon_amd import lib as scot_lib  # noqa: E402
from poseidon_amd import ops  # noqa: E402

PROTO = scot_lib.PROTOTYPES


# ------------------------------------------------------------------------------------------ synthetic tapes
def _c(name):
    def fn(*args):
        return 0
    fn.__name__ = name
    return fn


def tape(*items):
    """("L", stream) launch | ("R", event, stream) | ("W", stream, event) | ("O",) host callable | ("C",) C entry without a stream"""
    cmds = []
    for it in items:
        if it[0] == "L":
            cmds.append((_c("scot_memset_async"), (None, 0, 0, it[1] or None)))
        elif it[0] == "R":
            cmds.append((_c("scot_event_record"), (it[1], it[2] or None)))
        elif it[0] == "W":
            cmds.append((_c("scot_stream_wait_event"), (it[1] or None, it[2])))
        elif it[0] == "O":
            cmds.append((lambda: None, None))
        else:
            cmds.append((_c("scot_set_use_tr"), (1,)))
    return cmds


TAPES = {
    # fork, two launches beside one, join
    "fork_join": tape(("L", 0), ("R", 11, 0), ("W", 1, 11), ("L", 1), ("L", 1), ("R", 12, 1), ("L", 0), ("W", 0, 12), ("L", 0)),
    # one event recorded twice on the same stream: the first wait must stay in front of the second record
    "rerecorded": tape(("R", 11, 0), ("W", 1, 11), ("L", 1), ("L", 0), ("R", 11, 0), ("W", 1, 11), ("L", 1), ("L", 0)),
    # a wait whose record is not in the tape (and a later record of that event, which it must not see)
    "lone_wait": tape(("L", 0), ("W", 1, 19), ("L", 1), ("L", 0), ("R", 19, 0), ("L", 0), ("L", 1)),
    # a host callable and a stream-less C entry in the middle
    "barriers": tape(("L", 0), ("R", 11, 0), ("W", 1, 11), ("L", 1), ("O",), ("L", 1), ("L", 0), ("C",), ("L", 1)),
    # the side stream never used
    "empty_side": tape(("L", 0), ("R", 11, 0), ("L", 0), ("O",), ("L", 0)),
    # three streams: two forked from one record, one joined
    "three": tape(("L", 0), ("R", 11, 0), ("W", 1, 11), ("W", 2, 11), ("L", 1), ("L", 2), ("R", 12, 2), ("W", 0, 12), ("L", 0)),
}
# one event recorded on two streams: the record-order constraint is a restriction here (see the module text of tape_schedule)
CROSS = tape(("R", 11, 0), ("W", 2, 11), ("R", 11, 1), ("W", 2, 11), ("L", 2), ("L", 0), ("L", 1))


def brute_force(entries):
    """Every order that (i) keeps each stream's entries in order, (ii) keeps every opaque entry between what preceded and what followed
    it, and (iii) lets every wait see the record it sees in tape order — decided by simulating the order, not from constraints()."""
    by = {e.index: e for e in entries}
    idx = [e.index for e in entries]

    def seen(order):
        last, out = {}, {}
        for j in order:
            e = by[j]
            if e.kind == ts.RECORD:
                last[e.event] = j
            elif e.kind == ts.WAIT:
                out[j] = last.get(e.event)
        return out
    want = seen(idx)
    legal = []

    def rec(done, order):
        if len(order) == len(idx):
            if seen(order) == want:
                legal.append(tuple(order))
            return
        for j in idx:
            if j in done:
                continue
            e = by[j]
            earlier = [k for k in idx if k < j and k not in done]
            if e.kind == ts.OPAQUE:
                ok = not earlier
            else:
                ok = not any(by[k].kind == ts.OPAQUE or by[k].stream == e.stream for k in earlier)
            if ok:
                rec(done | {j}, order + [j])
    rec(frozenset(), [])
    return legal


def topological_orders(entries):
    """every order that respects ts.constraints(entries)"""
    idx = [e.index for e in entries]
    pred = {j: set() for j in idx}
    for a, b, _ in ts.constraints(entries):
        pred[b].add(a)
    out = []

    def rec(done, order):
        if len(order) == len(idx):
            out.append(tuple(order))
            return
        for j in idx:
            if j not in done and pred[j] <= done:
                rec(done | {j}, order + [j])
    rec(frozenset(), [])
    return out


def _others_before(order, entries, stream):
    by = {e.index: e for e in entries}
    out, front = {}, set()
    for j in order:
        if by[j].stream == stream and by[j].kind != ts.OPAQUE:
            out[j] = set(front)
        else:
            front.add(j)
    return out


@pytest.mark.parametrize("name", sorted(TAPES))
def test_generated_orders_against_every_legal_order(name):
    cmds = TAPES[name]
    assert len(cmds) <= 9
    entries = ts.parse(cmds, PROTO)
    legal = brute_force(entries)
    assert tuple(ts.canonical(entries)) in legal
    assert set(topological_orders(entries)) == set(legal)          # constraints() describes exactly the legal orders
    rng = __import__("random").Random(0)
    idx = [e.index for e in entries]
    for _ in range(300):                                            # ... and check() decides by them
        p = idx[:]
        rng.shuffle(p)
        if tuple(p) in legal:
            ts.check(p, entries)
        else:
            with pytest.raises(ts.ScheduleError):
                ts.check(p, entries)
    streams = sorted({e.stream for e in entries if e.kind != ts.OPAQUE} | {1})
    made = {("canonical",): ts.canonical(entries)}
    for s in streams:
        made[("late", s)], made[("early", s)] = ts.late(entries, s), ts.early(entries, s)
    for seed in range(24):
        made[("random", seed)] = ts.random(entries, seed)
    for key, order in made.items():
        assert tuple(order) in legal, key
        ts.check(order, entries)
    if len(legal) > 3:
        assert len({tuple(made[("random", s)]) for s in range(24)}) > 1, "the random orders never leave one order"
    assert ts.random(entries, 5) == ts.random(entries, 5)
    for s in streams:
        lt, el = _others_before(made[("late", s)], entries, s), _others_before(made[("early", s)], entries, s)
        for p in legal:
            here = _others_before(p, entries, s)
            for j in here:
                # late: nothing of another stream can be issued in front of j that `late` does not already put there
                assert here[j] <= lt[j], (name, s, j, p)
                # early: j has only what it depends on in front of it
                assert el[j] <= here[j], (name, s, j, p)
    if name == "empty_side":
        assert ts.late(entries, 1) == ts.early(entries, 1) == ts.canonical(entries)


def test_one_event_recorded_on_two_streams_is_restricted_not_widened():
    entries = ts.parse(CROSS, PROTO)
    legal = set(brute_force(entries))
    passing = set(topological_orders(entries))
    assert passing and passing <= legal
    assert ts.structure(entries)["rerecorded"] == [11]
    for order in (ts.late(entries, 1), ts.early(entries, 1), ts.late(entries, 2), ts.early(entries, 0), ts.random(entries, 3)):
        assert tuple(order) in legal


def test_check_rejects_illegal_orders():
    entries = ts.parse(TAPES["fork_join"], PROTO)
    ts.check(list(range(9)), entries)
    with pytest.raises(ts.ScheduleError, match="event"):
        ts.check([0, 2, 1, 3, 4, 5, 6, 7, 8], entries)          # the side stream's wait ahead of its record
    with pytest.raises(ts.ScheduleError, match="event"):
        ts.check([0, 1, 2, 3, 4, 6, 7, 5, 8], entries)          # the join ahead of the side stream's record
    with pytest.raises(ts.ScheduleError, match="stream"):
        ts.check([0, 1, 2, 4, 3, 5, 6, 7, 8], entries)          # two launches of one stream swapped
    with pytest.raises(ts.ScheduleError, match="permutation"):
        ts.check([0, 1, 2, 3, 4, 5, 6, 7, 7], entries)
    with pytest.raises(ts.ScheduleError, match="permutation"):
        ts.check([0, 1, 2, 3, 4, 5, 6, 7], entries)
    bar = ts.parse(TAPES["barriers"], PROTO)
    with pytest.raises(ts.ScheduleError, match="barrier"):
        ts.check([0, 1, 2, 3, 5, 4, 6, 7, 8], bar)
    re_ = ts.parse(TAPES["rerecorded"], PROTO)
    with pytest.raises(ts.ScheduleError, match="re-record"):
        ts.check([0, 3, 4, 1, 2, 5, 6, 7], re_)                 # the first wait would now see the second record


def test_parse_structure_regions_and_issue():
    cmds = TAPES["fork_join"]
    entries = ts.parse(cmds, PROTO)
    assert [e.kind for e in entries] == ["launch", "record", "wait", "launch", "launch", "record", "launch", "wait", "launch"]
    assert [e.stream for e in entries] == [0, 0, 1, 1, 1, 1, 0, 0, 0] and entries[2].event == 11 and entries[5].event == 12
    s = ts.structure(entries)
    assert s["main"] == 0 and s["event_edges"] == 2 and not s["rerecorded"] and not s["unpaired_waits"] and not s["opaque"]
    assert s["per_stream"] == {0: {"launch": 3, "record": 1, "wait": 1}, 1: {"launch": 2, "record": 1, "wait": 1}}
    assert s["joined"] == {1: True}
    (reg,) = ts.fork_regions(entries, 0, 1)
    assert reg == dict(launches=[3, 4], fork=1, join=7, passable=[6])
    lt = ts.late(entries, 1)
    assert lt == [0, 1, 6, 2, 3, 4, 5, 7, 8]
    assert ts.overtaken(lt, entries, 0, 1) == {3: 1, 4: 1} and ts.overtaken(ts.canonical(entries), entries, 0, 1) == {3: 0, 4: 0}
    assert ts.displaced(lt, entries, top=1) == [(6, 4)]
    # not joined: the side stream's last launch has no record behind it that the main stream waits for
    open_ = ts.parse(tape(("L", 0), ("R", 11, 0), ("W", 1, 11), ("L", 1), ("R", 12, 1), ("W", 0, 12), ("L", 1)), PROTO)
    assert ts.structure(open_)["joined"] == {1: False}
    lone = ts.structure(ts.parse(TAPES["lone_wait"], PROTO))
    assert lone["unpaired_waits"] == [1] and lone["event_edges"] == 0
    bar = ts.structure(ts.parse(TAPES["barriers"], PROTO))
    assert bar["opaque"] == [4, 7]
    assert ts.structure(ts.parse(TAPES["rerecorded"], PROTO))["rerecorded"] == [11]
    # issue(): a synchronisation at every stream switch, around every opaque entry, and at the end
    seen = []
    logged = [((lambda j=j: seen.append(j) or 0) if a is None else (lambda *x, j=j: seen.append(j) or 0), a) for j, (f, a) in enumerate(cmds)]
    n = ts.issue(logged, lt, entries, sync=lambda: seen.append("sync"))
    assert seen == [0, 1, 6, "sync", 2, 3, 4, 5, "sync", 7, 8, "sync"] and n == 3
    cmds_b = TAPES["barriers"]
    seen.clear()
    logged = [((lambda j=j: seen.append(j) or 0) if a is None else (lambda *x, j=j: seen.append(j) or 0), a) for j, (f, a) in enumerate(cmds_b)]
    ts.issue(logged, range(9), ts.parse(cmds_b, PROTO), sync=lambda: seen.append("sync"))
    assert seen == [0, 1, "sync", 2, 3, "sync", 4, "sync", 5, "sync", 6, "sync", 7, "sync", 8, "sync"]
    bad = [(f, a) for f, a in cmds]
    bad[4] = (lambda *a: -4, cmds[4][1])
    with pytest.raises(RuntimeError, match="entry 4"):
        ts.issue(bad, range(9), entries)
    with pytest.raises(ts.ScheduleError):
        ts.issue(cmds, [0, 2, 1, 3, 4, 5, 6, 7, 8], entries)
    with pytest.raises(ts.ScheduleError, match="not an entry point"):
        ts.parse([(_c("scot_no_such_entry"), (1,))], PROTO)
    with pytest.raises(ts.ScheduleError, match="arguments"):
        ts.parse([(_c("scot_event_record"), (1,))], PROTO)


# ------------------------------------------------------------------------------------------ the C ABI's own declarations
def _declarations():
    text = open(os.path.join(os.path.dirname(HERE), "include", "scot_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = {}
    for m in re.finditer(r"\b(scot_\w+)\s*\(([^();{}]*)\)\s*;", text):
        params = [p.strip() for p in m.group(2).split(",")] if m.group(2).strip() not in ("", "void") else []
        out[m.group(1)] = params
    return out


def test_stream_and_workspace_positions_match_the_header():
    decl = _declarations()
    assert set(PROTO) <= set(decl), sorted(set(PROTO) - set(decl))
    for name, proto in PROTO.items():
        params = decl[name]
        assert len(params) == len(proto), name
        has_stream = bool(params) and re.search(r"\b(scot_stream_t|hipStream_t)\s+\w+$", params[-1]) is not None
        if name == "scot_stream_wait_event":
            assert re.search(r"\b(scot_stream_t|hipStream_t)\s+\w+$", params[0]) and not has_stream
            continue
        assert has_stream == (name not in ts.NO_STREAM), name
        assert not any(re.search(r"\b(scot_stream_t|hipStream_t)\b", p) for p in params[:-1]), name       # one stream per entry point, last
    assert ts.NO_STREAM <= set(PROTO)
    for name, (p, n) in ts.WORKSPACE_ARGS.items():
        assert re.search(r"\bvoid\s*\*\s*workspace$", decl[name][p]) and re.search(r"\bsize_t\s+ws_bytes$", decl[name][n]), name
    # ... and these are all the launches that take caller-owned scratch by (pointer, bytes) beside the norm backward, whose partial matrix
    # is a fresh tensor of the step (engine.norm_bwd), never a pooled one
    assert {k for k, v in decl.items() if k in PROTO and k not in ts.NO_STREAM and any(re.search(r"\bws_bytes$", p) for p in v)} == \
        set(ts.WORKSPACE_ARGS) | {"scot_cln_bwd"}


# ------------------------------------------------------------------------------------------ end to end on the emulated library
@pytest.fixture()
def emu(monkeypatch):
    import emu_session
    lib = emu_session.load_emu()
    emu_session.patch_ops(monkeypatch, lib)
    return lib


M, N, K = 64, 24, 40
E1, E2 = 101, 102


def _rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


class _HandTape:
    """main: Y = X W^T; record e1 | side: wait e1; dW += Y^T X; record e2 | main: V = X2 W^T (independent of the side stream: what the
    weight gradient runs beside, so that the tape has more than one legal order); wait e2; Y = X2 W^T (the pooled-buffer pattern: the
    rows are reused by address); Z = X dW^T (reads dW)."""

    def __init__(self, monkeypatch, shared_scratch=False):
        self.X, self.X2, self.W = _rnd(M, K, seed=1), _rnd(M, K, seed=2), _rnd(N, K, seed=3) * K ** -0.5
        self.Y, self.dW, self.Z, self.V = torch.empty(M, N), torch.empty(N, K), torch.empty(M, N), torch.empty(M, N)
        cur = [0]
        scratch = [torch.empty(1 << 20, dtype=torch.uint8) for _ in range(2)]
        monkeypatch.setattr(ops, "stream", lambda: cur[0] or None)
        monkeypatch.setattr(ops, "workspace", lambda need=0: scratch[0 if shared_scratch else ops._slot])
        self.cmds = []
        prev = ops.set_recorder(self.cmds)
        try:
            ops.linear_fwd(ops.F32, self.X, self.W, self.Y)
            ops.event_record(E1, None)
            ops.stream_wait_event(1, E1)
            cur[0], slot = 1, ops.set_workspace_slot(1)
            ops.linear_wgrad(ops.F32, self.Y, self.X, self.dW)
            cur[0] = 0
            ops.set_workspace_slot(slot)
            ops.event_record(E2, 1)
            ops.linear_fwd(ops.F32, self.X2, self.W, self.V)
            ops.stream_wait_event(None, E2)
            ops.linear_fwd(ops.F32, self.X2, self.W, self.Y)
            ops.linear_fwd(ops.F32, self.X, self.dW, self.Z)
        finally:
            ops.set_recorder(prev)
        self.entries = ts.parse(self.cmds, PROTO)

    def run(self, order, entries=None):
        # what an earlier step left behind: other activations in the reused rows, nothing in the outputs
        self.Y.copy_(_rnd(M, N, seed=9))
        self.dW.fill_(0.5)
        self.Z.fill_(float("nan"))
        self.V.fill_(float("nan"))
        ts.issue(self.cmds, order, self.entries if entries is None else entries)
        return self.dW.clone(), self.Y.clone(), self.Z.clone(), self.V.clone()


def test_hand_built_tape_on_the_emulated_library(emu, monkeypatch):
    t = _HandTape(monkeypatch)
    e = t.entries
    assert [x.kind for x in e] == ["launch", "record", "wait", "launch", "record", "launch", "wait", "launch", "launch"]
    assert [x.stream for x in e] == [0, 0, 1, 1, 1, 0, 0, 0, 0]
    s = ts.structure(e)
    assert s["event_edges"] == 2 and s["joined"] == {1: True} and not s["unpaired_waits"] and not s["rerecorded"] and not s["opaque"]
    assert not ts.shared_workspaces(ts.workspace_ranges(t.cmds, e))
    ref = t.run(ts.canonical(e))
    Y0 = t.X.double() @ t.W.double().t()
    assert float((ref[0].double() - (0.5 + Y0.t() @ t.X.double())).norm()) < 1e-4 * float((Y0.t() @ t.X.double()).norm())
    assert float((ref[1].double() - t.X2.double() @ t.W.double().t()).norm()) < 1e-5 * float(ref[1].norm())
    orders = [ts.late(e, 1), ts.early(e, 1), ts.late(e, 0), ts.early(e, 0)] + [ts.random(e, seed) for seed in range(8)]
    legal = brute_force(e)
    assert len(legal) > 1 and {tuple(o) for o in orders} <= set(legal)
    for order in legal:                       # the emulation is serial and deterministic: every legal order, bit for bit
        got = t.run(order)
        assert all(torch.equal(a, b) for a, b in zip(got, ref)), order

    def differs(got):
        return float((got[0] - ref[0]).norm()) > 0.1 * float(ref[0].norm())
    # without wait(side, e1): `early(side)` runs the weight gradient on rows the first product has not written yet
    fork = next(x.index for x in e if x.kind == ts.WAIT and x.stream == 1)
    cut = ts.without(e, fork)
    assert ts.early(cut, 1).index(3) < ts.early(cut, 1).index(0)
    assert differs(t.run(ts.early(cut, 1), cut))
    assert not differs(t.run(ts.canonical(cut), cut))            # ... which the tape's own order never shows
    # without wait(main, e2): `late(side)` runs it on the rows the second product has overwritten
    join = next(x.index for x in e if x.kind == ts.WAIT and x.stream == 0)
    cut = ts.without(e, join)
    assert ts.late(cut, 1).index(3) > ts.late(cut, 1).index(7)
    got = t.run(ts.late(cut, 1), cut)
    assert differs(got) and bool(torch.isfinite(got[0]).all())
    assert not differs(t.run(ts.canonical(cut), cut))
    # (with the edges in place neither order can do either)
    assert ts.early(e, 1).index(3) > ts.early(e, 1).index(0) and ts.late(e, 1).index(3) < ts.late(e, 1).index(7) and ts.late(e, 1).index(3) > ts.late(e, 1).index(5)


def test_scratch_shared_between_streams_is_reported(emu, monkeypatch):
    t = _HandTape(monkeypatch, shared_scratch=True)
    bad = ts.shared_workspaces(ts.workspace_ranges(t.cmds, t.entries))
    assert bad and {bad[0][0], bad[0][2]} == {0, 1}
    a, b = {0: {(4096, 1024)}, 1: {(5120, 64)}}, {0: {(4096, 1024)}, 1: {(5119, 64)}}
    assert not ts.shared_workspaces(a) and ts.shared_workspaces(b) == [(0, (4096, 1024), 1, (5119, 64))]
