"""Legal stream orders of a recorded step tape (test helper: pure Python, nothing of torch.cuda is touched at import).

A recorded forward or backward (`ScOTEngine._taped[...]["fwd"]`, `["bwd"][variant][0]`) is a list of `(fn, args)` C-ABI calls and
`(callable, None)` host steps.  On the GPU the event records and stream waits between the two HIP streams are ordinary entries with
explicit handles, and every launch names its stream as its last argument, so the tape contains its own happens-before relation:

  * the entries of one stream keep their order (a HIP stream is in-order);
  * a wait goes behind the record it pairs with — the latest record of that event before it in tape order — and in front of the next
    record of the same event (issued later it would pair with that one instead); the records of one event keep their order (implied by
    stream order when they sit on one stream, which is all the engine does; with records on several streams it is an extra restriction
    that keeps every wait paired with the record it was written for);
  * an opaque entry — a host callable, or a C entry without a stream parameter — is a full barrier.

Any permutation that respects these is a legal execution: issued with a device synchronisation at every stream switch, the GPU executes
exactly that permutation.  If the event edges are complete every legal order computes the same thing; if one is missing, some legal
order runs a consumer before its producer or a reader behind the overwrite.  `late` / `early` / `random` are the orders that look for it.
"""
from __future__ import annotations

import ctypes
import heapq
import random as _random
from typing import Callable, Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

LAUNCH, RECORD, WAIT, OPAQUE = "launch", "record", "wait", "opaque"

# C entries whose last parameter is NOT a stream although it may be a pointer (queries, configuration, the communicator, the replayer
# itself); tests/test_tape_schedule_cpu.py holds this list against include/scot_hip.h
NO_STREAM = frozenset({
    "scot_abi_version", "scot_operand_format", "scot_set_use_tr", "scot_get_use_tr", "scot_gemm_route", "scot_wgrad_group_route",
    "scot_block_tail_route", "scot_route_table", "scot_gemm_workspace_bytes", "scot_gemm_wide_config", "scot_gemm_splitk_config",
    "scot_wgrad_group_workspace_bytes", "scot_block_tail_workgroups", "scot_wgrad_mlp_workspace_bytes", "scot_cln_bwd_workspace_bytes",
    "scot_cln_dtime_workspace_bytes", "scot_tape_replay", "scot_dp_unique_id", "scot_dp_init", "scot_dp_world", "scot_dp_rank",
    "scot_dp_finalize", "scot_optim_blocks"})

# (pointer, bytes) positions of the scratch a launch is handed (include/scot_hip.h): split-K partial tiles / partial sums, reused by address
WORKSPACE_ARGS = {"scot_gemm": (26, 27), "scot_wgrad_group": (9, 10), "scot_wgrad_mlp": (12, 13), "scot_cln_dtime": (13, 14)}


class Entry(NamedTuple):
    index: int                  # position in the recorded list
    kind: str                   # LAUNCH | RECORD | WAIT | OPAQUE
    stream: Optional[int]       # handle (0 = the default stream); None for an opaque entry
    event: Optional[int]        # handle, for RECORD / WAIT


class ScheduleError(AssertionError):
    pass


def entry_name(fn) -> str:
    """a C entry point's symbol; for a host callable the innermost function it wraps (engine.tdo_dynamic wraps its argument)"""
    name = getattr(fn, "__name__", None)
    if name and name.startswith("scot_"):
        return name
    for cell in getattr(fn, "__closure__", None) or ():
        try:
            inner = cell.cell_contents
        except ValueError:
            continue
        if callable(inner) and getattr(inner, "__name__", None) and name == "run":
            return entry_name(inner)
    return name or repr(fn)


def _handle(v) -> int:
    if v is None:
        return 0
    if isinstance(v, ctypes.c_void_p):
        return v.value or 0
    return int(v)


def parse(cmds: Sequence[tuple], prototypes: Dict[str, list]) -> List[Entry]:
    """recorded list -> entries; the stream comes from where the prototype puts it: last argument of a launch and of scot_event_record,
    first argument of scot_stream_wait_event"""
    out = []
    for i, (fn, args) in enumerate(cmds):
        if args is None:
            out.append(Entry(i, OPAQUE, None, None))
            continue
        name = getattr(fn, "__name__", None)
        if name not in prototypes:
            raise ScheduleError(f"tape entry {i}: {name!r} is not an entry point of the C ABI")
        proto = prototypes[name]
        if len(args) != len(proto):
            raise ScheduleError(f"tape entry {i}: {name} recorded with {len(args)} arguments, its prototype has {len(proto)}")
        if name == "scot_stream_wait_event":
            out.append(Entry(i, WAIT, _handle(args[0]), _handle(args[1])))
        elif name == "scot_event_record":
            out.append(Entry(i, RECORD, _handle(args[-1]), _handle(args[0])))
        elif name in NO_STREAM or not proto or proto[-1] is not ctypes.c_void_p:
            out.append(Entry(i, OPAQUE, None, None))
        else:
            out.append(Entry(i, LAUNCH, _handle(args[-1]), None))
    return out


def constraints(entries: Sequence[Entry]) -> List[Tuple[int, int, str]]:
    """(before, after, why) over tape indices; see the module text"""
    edges = []
    last_on: Dict[int, int] = {}
    last_rec: Dict[int, int] = {}
    waits_since: Dict[int, List[int]] = {}
    barrier, seg = None, []
    for e in entries:
        if e.kind == OPAQUE:
            edges += [(j, e.index, "barrier") for j in seg]
            if barrier is not None and not seg:
                edges.append((barrier, e.index, "barrier"))
            barrier, seg = e.index, []
            continue
        if barrier is not None:
            edges.append((barrier, e.index, "barrier"))
        seg.append(e.index)
        if e.stream in last_on:
            edges.append((last_on[e.stream], e.index, "stream"))
        last_on[e.stream] = e.index
        if e.kind == WAIT:
            if e.event in last_rec:
                edges.append((last_rec[e.event], e.index, "event"))
            waits_since.setdefault(e.event, []).append(e.index)
        elif e.kind == RECORD:
            edges += [(w, e.index, "re-record") for w in waits_since.pop(e.event, [])]
            if e.event in last_rec:
                edges.append((last_rec[e.event], e.index, "record order"))
            last_rec[e.event] = e.index
    return edges


def check(order: Sequence[int], entries: Sequence[Entry]) -> None:
    """raise unless `order` is a permutation of the entries' indices that respects every constraint"""
    idx = [e.index for e in entries]
    if len(order) != len(idx) or sorted(order) != sorted(idx):
        raise ScheduleError("not a permutation of the tape's entries")
    pos = {j: p for p, j in enumerate(order)}
    for a, b, why in constraints(entries):
        if pos[a] > pos[b]:
            raise ScheduleError(f"entry {b} issued before entry {a} ({why})")


# ------------------------------------------------------------------------------------------ linearisations
def canonical(entries: Sequence[Entry]) -> List[int]:
    return [e.index for e in entries]


def _graph(entries, reverse=False):
    succ = {e.index: [] for e in entries}
    npred = {e.index: 0 for e in entries}
    for a, b, _ in constraints(entries):
        if reverse:
            a, b = b, a
        succ[a].append(b)
        npred[b] += 1
    return succ, npred


def _hold_back(entries: Sequence[Entry], stream: int, reverse: bool) -> List[int]:
    """topological order that issues an entry of `stream` only when nothing else is ready (ties: tape order); on the reversed graph when
    `reverse`.  `stream`'s entries are a chain, so when one is issued every entry still waiting descends from it: no legal order has
    more of the others in front of it."""
    succ, npred = _graph(entries, reverse)
    mine = {e.index for e in entries if e.stream == stream and e.kind != OPAQUE}
    sign = -1 if reverse else 1
    heaps = ([], [])          # others, mine
    for j, n in npred.items():
        if n == 0:
            heapq.heappush(heaps[j in mine], sign * j)
    out = []
    while heaps[0] or heaps[1]:
        j = sign * heapq.heappop(heaps[0] if heaps[0] else heaps[1])
        out.append(j)
        for k in succ[j]:
            npred[k] -= 1
            if npred[k] == 0:
                heapq.heappush(heaps[k in mine], sign * k)
    if len(out) != len(npred):
        raise ScheduleError("the tape's constraints are cyclic")
    return out


def late(entries: Sequence[Entry], stream: int) -> List[int]:
    """every entry of `stream` at the last legal moment: immediately before the first entry that depends on it, or the next barrier"""
    return _hold_back(entries, stream, False)


def early(entries: Sequence[Entry], stream: int) -> List[int]:
    """the mirror of `late`: every entry of `stream` as soon as what it depends on has been issued, everything else delayed as far as legal"""
    return _hold_back(entries, stream, True)[::-1]


def random(entries: Sequence[Entry], seed: int, bursts: Sequence[int] = (1, 1, 2, 3, 5, 8, 16, 48)) -> List[int]:
    """at each step one of the streams whose next entry is ready, for a burst of random length (seeded)"""
    rng = _random.Random(seed)
    succ, npred = _graph(entries)
    lanes: Dict[object, List[int]] = {}
    for e in entries:
        lanes.setdefault("opaque" if e.kind == OPAQUE else e.stream, []).append(e.index)
    keys = sorted(lanes, key=str)
    head = {k: 0 for k in keys}
    out = []
    while len(out) < len(npred):
        ready = [k for k in keys if head[k] < len(lanes[k]) and npred[lanes[k][head[k]]] == 0]
        if not ready:
            raise ScheduleError("the tape's constraints are cyclic")
        k = rng.choice(ready)
        for _ in range(rng.choice(bursts)):
            if head[k] == len(lanes[k]) or npred[lanes[k][head[k]]]:
                break
            j = lanes[k][head[k]]
            head[k] += 1
            out.append(j)
            for s in succ[j]:
                npred[s] -= 1
    return out


# ------------------------------------------------------------------------------------------ facts about a tape
def main_stream(entries: Sequence[Entry]) -> Optional[int]:
    """the stream the step is issued on: its first entry's (the engine forks from and joins into the stream that is current)"""
    return next((e.stream for e in entries if e.kind != OPAQUE), None)


def _pairs(entries):
    """[(record index, wait index)] of the event edges, and the waits that pair with no record of this tape"""
    last_rec, pairs, lone = {}, [], []
    for e in entries:
        if e.kind == RECORD:
            last_rec[e.event] = e.index
        elif e.kind == WAIT:
            if e.event in last_rec:
                pairs.append((last_rec[e.event], e.index))
            else:
                lone.append(e.index)
    return pairs, lone


def structure(entries: Sequence[Entry], main: Optional[int] = None) -> dict:
    main = main_stream(entries) if main is None else main
    by = {e.index: e for e in entries}
    per: Dict[int, Dict[str, int]] = {}
    nrec: Dict[int, int] = {}
    for e in entries:
        if e.kind != OPAQUE:
            per.setdefault(e.stream, {LAUNCH: 0, RECORD: 0, WAIT: 0})[e.kind] += 1
        if e.kind == RECORD:
            nrec[e.event] = nrec.get(e.event, 0) + 1
    pairs, lone = _pairs(entries)
    joined = {}
    for s in per:
        if s == main:
            continue
        launches = [e.index for e in entries if e.stream == s and e.kind == LAUNCH]
        joined[s] = not launches or any(by[r].stream == s and r > launches[-1] and by[w].stream == main for r, w in pairs)
    return dict(main=main, per_stream=per, event_edges=len(pairs), rerecorded=sorted(ev for ev, n in nrec.items() if n > 1),
                unpaired_waits=lone, opaque=[e.index for e in entries if e.kind == OPAQUE], joined=joined)


def workspace_ranges(cmds: Sequence[tuple], entries: Sequence[Entry]) -> Dict[int, set]:
    """per stream the (pointer, bytes) scratch ranges its launches were handed (WORKSPACE_ARGS)"""
    out: Dict[int, set] = {}
    for e in entries:
        if e.kind != LAUNCH:
            continue
        fn, args = cmds[e.index]
        at = WORKSPACE_ARGS.get(getattr(fn, "__name__", None))
        if at is None:
            continue
        p, n = _handle(args[at[0]]), int(args[at[1]] or 0)
        if p and n:
            out.setdefault(e.stream, set()).add((p, n))
    return out


def shared_workspaces(ranges: Dict[int, set]) -> list:
    """[(stream a, range, stream b, range)] of scratch ranges of different streams that overlap"""
    bad = []
    streams = sorted(ranges)
    for i, a in enumerate(streams):
        for b in streams[i + 1:]:
            bad += [(a, ra, b, rb) for ra in sorted(ranges[a]) for rb in sorted(ranges[b]) if ra[0] < rb[0] + rb[1] and rb[0] < ra[0] + ra[1]]
    return bad


def fork_regions(entries: Sequence[Entry], main: int, side: int) -> List[dict]:
    """`side`'s launches grouped by the join that hands them back: a record on `side` that `main` waits for.  Per region: its launches,
    the main-stream record its first wait pairs with (`fork`), the main-stream wait that joins it (`join`, None when nothing does) and
    `passable`, the main-stream launches between the two — what the region's launches may run beside."""
    by = {e.index: e for e in entries}
    pairs, _ = _pairs(entries)
    fork_of = {w: r for r, w in pairs if by[w].stream == side and by[r].stream == main}
    joins = {}
    for r, w in pairs:
        if by[r].stream == side and by[w].stream == main:
            joins[r] = min(w, joins.get(r, w))
    regions, cur = [], dict(launches=[], fork=None, join=None)
    for e in entries:
        if e.stream != side or e.kind == OPAQUE:
            continue
        if e.kind == WAIT and cur["fork"] is None and not cur["launches"]:
            cur["fork"] = fork_of.get(e.index)
        elif e.kind == LAUNCH:
            cur["launches"].append(e.index)
        elif e.kind == RECORD and e.index in joins:
            cur["join"] = joins[e.index]
            regions.append(cur)
            cur = dict(launches=[], fork=None, join=None)
    if cur["launches"]:
        regions.append(cur)
    mains = [e.index for e in entries if e.stream == main and e.kind == LAUNCH]
    for r in regions:
        lo = r["fork"] if r["fork"] is not None else -1
        hi = r["join"] if r["join"] is not None else float("inf")
        r["passable"] = [m for m in mains if lo < m < hi]
    return [r for r in regions if r["launches"]]


def overtaken(order: Sequence[int], entries: Sequence[Entry], main: int, side: int) -> Dict[int, int]:
    """side launch -> number of main-stream launches that sit behind it in the tape but are issued in front of it in `order`"""
    pos = {j: p for p, j in enumerate(order)}
    mains = sorted(e.index for e in entries if e.stream == main and e.kind == LAUNCH)
    main_pos = sorted(pos[m] for m in mains)
    import bisect
    out = {}
    for e in entries:
        if e.stream == side and e.kind == LAUNCH:
            # main-stream launches keep their own order, so those issued before e are a prefix of `mains`
            out[e.index] = max(0, bisect.bisect_left(main_pos, pos[e.index]) - bisect.bisect_left(mains, e.index))
    return out


def displaced(order: Sequence[int], entries: Sequence[Entry], top: int = 6) -> List[Tuple[int, int]]:
    """[(tape index, positions moved)] of the entries `order` moved furthest from their place in the tape"""
    rank = {e.index: p for p, e in enumerate(entries)}
    d = sorted(((abs(p - rank[j]), j) for p, j in enumerate(order)), reverse=True)
    return [(j, n) for n, j in d[:top] if n]


def without(entries: Sequence[Entry], index: int) -> List[Entry]:
    """the tape with one entry taken out (a replay of an order of the result does not issue it)"""
    assert any(e.index == index for e in entries)
    return [e for e in entries if e.index != index]


def issue(cmds: Sequence[tuple], order: Iterable[int], entries: Sequence[Entry], sync: Callable[[], None] = lambda: None) -> int:
    """Issue the entries in `order` (checked first).  `sync` is called whenever the stream of the next entry differs from the previous
    one's, after every opaque entry, and at the end; a non-zero status raises.  Returns the number of sync calls."""
    order = list(order)
    check(order, entries)
    by = {e.index: e for e in entries}
    prev, nsync = None, 0
    for j in order:
        e = by[j]
        fn, args = cmds[j]
        if prev is not None and e.stream != prev:      # (an opaque entry has no stream: it differs from any)
            sync()
            nsync += 1
        if args is None:
            fn()
        else:
            rc = fn(*args)
            if rc:
                raise RuntimeError(f"step tape entry {j}: {entry_name(fn)} returned {rc}")
        if e.kind == OPAQUE:
            sync()
            nsync += 1
            prev = None
        else:
            prev = e.stream
    sync()
    return nsync + 1
