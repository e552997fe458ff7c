"""Exported inference plans: a trained model that runs from the C ABI alone (include/scot_plan.h, csrc/plan.hip).

`export_plan` makes one dedicated recording of the engine's inference forward for exactly the given input shapes — on one stream, the
weight-gradient stream switched off, so the list is linear and needs no events — and turns it into a relocatable image
(csrc/plan_image.h): every argument of every recorded call is classified from its `argtypes`; a device address becomes (buffer index,
byte offset), where the buffers are what the allocation funnels (`engine.new` / `engine.pool`, `ops.workspace`, the engine's own list
of constants, the input copies) registered WHILE the forward was recorded; the stream becomes a placeholder.  Constants are stored by
value.  Before the file is written the image is loaded through the runtime in this process, its scratch filled with NaN bytes, and run
on the export inputs: the prediction has to be finite and bit-identical to the model's own.

`export_plan(..., adjoint=("pixel_values", "time"))` records two lists instead — the forward a differentiable call runs and the frozen-model
backward from a cotangent of the prediction — and writes a format-2 image whose second entries section `scot_plan_vjp` replays; the
self-check then also requires the engine's own bits for both input gradients.  The same image differentiates a whole rollout:
`Plan.rollout_vjp` (scot_plan_rollout_vjp) recomputes every step from the rollout's predictions, from the last to the first.

`export_plan(..., labels=y, train=optimizer)` (a `FusedAdamW` over this model) writes a TRAINING image, format 4: beside the inference
forward it holds one optimizer step as three lists — the forward through the loss, the backward with the weight gradients (behind the
zero fill of the accumulated gradients, before the un-scale passes), and what `FusedAdamW.step` issues — and, by value, everything a
step changes: the fp32 parameters, both 16-bit copies, both moments, the step counters, the clip floats, the gradient scale.
`Plan.train_step` runs one step from C (scot_plan_train_step), `Plan.snapshot` reads the state back into the image, and
`load_training_state` brings such an image's state back into a `ScOT` and its optimizer.

`export_plan(..., streams=2)` (inference and training plans) records the engine's own TWO-stream program instead — the weight-gradient
stream left on, on the CPU emulation with stand-in handles — and writes a format-5 / format-6 image: stream arguments become stream
indices (0 the caller's, 1 the plan's side stream), the engine's fork and join edges stay in the lists as `scot_event_record` /
`scot_stream_wait_event` entries over event indices, and every list is closed (the exporter appends the join where the engine leaves
the side stream unjoined).  The runtime gives such a plan a side stream and its events; every call works on it unchanged.

`Plan` is the ctypes wrapper of the runtime, for the tests and for a Python process that wants inference without torch (it imports
torch only if the caller hands it tensors).
"""
from __future__ import annotations

import contextlib
import ctypes
import struct
import sys

from . import lib as _lib

MAGIC = 0x4e414c50544f4353
FORMAT = 1
FORMAT_ADJOINT = 2      # + a backward entries section and the adjoint words (csrc/plan_image.h)
FORMAT_TRAINING = 4     # + the training words, which name three step lists and the state spans (3 is unassigned)
FORMAT_STREAMS = 5      # format 1 + the streams section: lists on two streams with event entries
FORMAT_TRAINING_STREAMS = 6      # format 4 + the streams section
STREAMED = {FORMAT: FORMAT_STREAMS, FORMAT_TRAINING: FORMAT_TRAINING_STREAMS}      # one-stream format -> its two-stream form
HEADER_WORDS, NAME_BYTES, IO_WORDS, ADJ_WORDS, TRAIN_WORDS, STREAMS_WORDS = 32, 48, 24, 24, 64, 2
CONSTANT, INPUT, OUTPUT, SCRATCH, STATE = range(5)
ARG_INT, ARG_NULL, ARG_PTR, ARG_STREAM, ARG_ARRAY, ARG_EVENT = range(6)
MAX_EVENTS = 4096
RECORD, WAIT = "scot_event_record", "scot_stream_wait_event"      # (EVENT, STREAM) and (STREAM, EVENT): SCOT_PLAN_SYNC_ENTRY_POINTS
COMPUTE_CODE = {"fp32": 0, "fp16": 1, "bf16": 2, "bf16x3": 3}
MAX_INT, MAX_FLT = 48, 8
(H_MAGIC, H_FORMAT, H_ABI, H_OPERAND, H_COMPUTE, H_BYTES, H_NNAMES, H_NAMES_OFF, H_NBUFFERS, H_BUFFERS_OFF, H_NENTRIES, H_ENTRIES_OFF,
 H_ENTRIES_WORDS, H_NARRAYS, H_ARRAYS_OFF, H_ARRAYS_WORDS, H_IO_OFF, H_DATA_OFF, H_DATA_BYTES, H_NBACKWARD, H_BACKWARD_OFF,
 H_BACKWARD_WORDS, H_ADJ_OFF, H_TRAIN_OFF, H_STREAMS_OFF) = range(25)


def _slots(*words):
    """the first word of each slot, given every slot's length in order — as the C enums of csrc/plan_image.h compute them
    (1: a plain word; 3: a list (count, offset, words) or a span (buffer, offset, bytes))"""
    return [sum(words[:i]) for i in range(len(words))]


ADJ_FLAGS, ADJ_COT, ADJ_DPV, ADJ_DTIME, ADJ_STATE, ADJ_COUNTER, ADJ_SCALE_EXP, ADJ_KEPT_BYTES = _slots(1, 3, 3, 3, 3, 3, 1, 1)
(TR_FLAGS, TR_GROUPS, TR_ARENA_FLOATS, TR_FWD, TR_BWD, TR_UPD, TR_LR_ENTRY, TR_LR_ARG, TR_KEPT_BYTES, TR_LABELS, TR_LOSS, TR_PRED, TR_ARENA,
 TR_EXP_AVG, TR_EXP_AVG_SQ, TR_SHADOW, TR_SHADOW_T, TR_STEP_STATE, TR_CLIP, TR_SCALE_STATE, TR_COUNTER) = _slots(1, 1, 1, 3, 3, 3, 1, 1, 1, *[3] * 12)
assert ADJ_KEPT_BYTES < ADJ_WORDS and TR_COUNTER + 3 <= TRAIN_WORDS
# the runtime's three tables of entry points: which call enumerates each, and the X-macro of csrc/plan_image.h behind it
ENTRY_POINT_TABLES = {"forward": ("scot_plan_entry_point", "SCOT_PLAN_ENTRY_POINTS"),
                      "adjoint": ("scot_plan_adjoint_entry_point", "SCOT_PLAN_ADJOINT_ENTRY_POINTS"),
                      "training": ("scot_plan_training_entry_point", "SCOT_PLAN_TRAINING_ENTRY_POINTS")}
DESCRIBE_STREAMS = ("streams", "events", "overlaps", "host_stream")
DESCRIBE_TRAINING = ("has_training", "groups", "arena_floats", "step_calls", "labels_bytes", "kept_bytes", "dynamic_scale", "mask")
TR_FLAG_DYNAMIC, TR_FLAG_MASK, TR_FLAG_MASK_FULL = 1, 2, 4      # SCOT_PLAN_TR_FLAGS: bit 1 = the batch has a mask, bit 2 = an element mask
(IO_HAS_MASK, IO_MASK_BUF) = (11, 12)      # SCOT_PLAN_IO_HAS_MASK, then (buffer, offset, bytes)
TRAIN_STATUS = ("applied", "skipped", "grad_scale", "grad_norm", "clip_coef", "nonfinite")
# host arrays of floats among the recorded arguments: {entry point: {argument index: index of the argument that holds the count}}
HOST_FLOAT_ARRAYS = {"scot_adamw_step": {6: 8, 7: 8}}
LR_ARGUMENT = ("scot_adamw_step", 6)
DESCRIBE_ADJOINT = ("has_adjoint", "d_pixel_values", "d_time", "backward_calls", "kept_bytes", "grad_scale_exponent")
DESCRIBE = ("batch", "channels", "height", "width", "out_channels", "has_time", "time_bytes", "has_pixel_mask", "pixel_mask_bytes",
            "operand_format", "compute", "device_bytes", "calls", "pixel_values_bytes", "prediction_bytes", "format")


class PlanExportError(RuntimeError):
    pass


def bind(lib):
    """type the plan calls of a loaded build of the library (idempotent)"""
    for name, argtypes in _lib.PLAN_PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = _lib.restype(name)
    return lib


def runtime_entry_points(lib, adjoint=False, training=False):
    """the entry points the runtime of this build lists: what a plan's forward (adjoint: its backward; training: the three step lists
    of a training plan) may call"""
    bind(lib)
    table = next(name for name, asked in (("training", training), ("adjoint", adjoint), ("forward", True)) if asked)
    query = getattr(lib, ENTRY_POINT_TABLES[table][0])
    out, i = [], 0
    while True:
        n = query(i)
        if n is None:
            return out
        out.append(n.decode())
        i += 1


# ----------------------------------------------------------------------------------------------------------------- export
class _Registry:
    """The allocations an export's recording touches, registered where they are made."""

    def __init__(self):
        self.bufs = {}      # address -> dict(addr, bytes, kind, name, tensor)
        self.streams = None      # a two-stream recording: {stream handle: index} — the current stream 0, the engine's side stream 1
        self.mask_u8 = None      # a masked training recording: the mask INPUT, which the engine uses as its byte mask as it stands

    def add(self, t, kind, name, stored=False):
        """stored: a STATE buffer the image holds by value (a training plan's; otherwise the runtime zeroes it at load)"""
        n = t.numel() * t.element_size()
        if n == 0:
            return
        if not t.is_contiguous():
            raise PlanExportError(f"export_plan: buffer {name} is not contiguous")
        a = t.data_ptr()
        cur = self.bufs.get(a)
        if cur is None or cur["bytes"] < n:
            self.bufs[a] = dict(addr=a, bytes=n, kind=kind if cur is None else min(kind, cur["kind"]), name=name, tensor=t,
                                stored=bool(stored or (cur is not None and cur["stored"])))

    def scratch(self, t):
        self.add(t, SCRATCH, "scratch")

    def freeze(self):
        self.order = sorted(self.bufs.values(), key=lambda b: b["addr"])
        self.starts = [b["addr"] for b in self.order]
        for a, b in zip(self.order, self.order[1:]):
            if a["addr"] + a["bytes"] > b["addr"]:
                raise PlanExportError(f"export_plan: registered buffers {a['name']} and {b['name']} overlap")

    def resolve(self, addr):
        import bisect
        i = bisect.bisect_right(self.starts, addr) - 1
        if i >= 0 and addr < self.order[i]["addr"] + self.order[i]["bytes"]:
            return self.order[i], addr - self.order[i]["addr"]
        return None, 0


def _address(fn):
    return ctypes.cast(fn, ctypes.c_void_p).value


def _check_request(model, pixel_values, time, pixel_mask, labels, train=None, resize=False):
    from . import ops
    cfg = model.config
    if labels is not None and train is None:
        raise PlanExportError("export_plan: labels are not part of a plan (it covers the inference forward: no loss)")
    if pixel_mask is not None and train is None:
        raise PlanExportError("export_plan: pixel_mask overwrites the prediction with label values (reference model.py:1411-1484) and a "
                              "plan takes no labels: apply the mask to the plan's prediction in the host program")
    if pixel_values is None or pixel_values.dim() != 4:
        raise PlanExportError("export_plan: pixel_values [B, C, H, W] is required")
    try:
        ops.ptr(pixel_values)
    except _lib.ScotLibraryError as e:
        raise PlanExportError("export_plan: a CPU model cannot be exported — the forward that is recorded runs on the GPU "
                              f"(move the model and the example inputs there first): {e}") from None
    if pixel_values.shape[2] != cfg.image_size or pixel_values.shape[3] != cfg.image_size:
        if not resize:
            raise PlanExportError(f"export_plan: input size {tuple(pixel_values.shape[2:])} differs from config.image_size = {cfg.image_size}; the "
                                  "spectral resize lives outside the engine and a plan covers the engine forward only (pass resize=True "
                                  "for a plan that resamples a square input to config.image_size and the prediction back)")
        if pixel_values.shape[2] != pixel_values.shape[3]:
            raise PlanExportError(f"export_plan: resize=True with a non-square input {tuple(pixel_values.shape[2:])}: the spectral resize "
                                  "assumes square images (as the reference does)")
        if pixel_values.shape[2] > 512 or cfg.image_size > 512:
            raise PlanExportError("export_plan: resize=True covers sizes up to 512 (scot_spectral_resize)")
        if train is not None:
            raise PlanExportError(f"export_plan: resize=True together with train=: a training plan runs at image_size = {cfg.image_size} "
                                  "only (the loss at another resolution is not a kernel yet)")
    if pixel_values.shape[1] != cfg.num_channels:
        raise PlanExportError(f"export_plan: pixel_values has {pixel_values.shape[1]} channels, the model takes {cfg.num_channels}")
    if train is not None and float(getattr(cfg, "drop_path_rate", 0.0) or 0.0) > 0.0:
        raise PlanExportError("export_plan: a training plan cannot hold stochastic depth (drop_path_rate > 0): the training-mode masks "
                              "are host draws")
    if model.training and float(getattr(cfg, "drop_path_rate", 0.0) or 0.0) > 0.0:
        raise PlanExportError("export_plan: the model is in training mode with stochastic depth (drop_path_rate > 0): its forward draws "
                              "random masks on the host; call model.eval() first")
    if cfg.use_conditioning and time is None:
        raise PlanExportError("export_plan: time is required when use_conditioning=True")
    if pixel_mask is not None:
        _mask_bytes(pixel_mask, pixel_values.shape[0], cfg.num_out_channels, pixel_values.shape[2], pixel_values.shape[3],
                    PlanExportError, "export_plan: ")


def _mask_bytes(m, B, Cout, H, W, error=ValueError, prefix=""):
    """the reference's pixel_mask in one of the forms a masked training plan takes -> (uint8 tensor: the plan's mask input, whether it
    is an element mask).  bool (or uint8) [B, Cout]: a channel mask, B * Cout bytes; [B, Cout, H, W]: an element mask; [B, 1, H, W]:
    expanded over the channels into an element mask.  Anything else: `error`, naming pixel_mask."""
    import torch
    ok = hasattr(m, "dim") and m.dtype in (torch.bool, torch.uint8)
    shape = tuple(m.shape) if hasattr(m, "shape") else None
    if ok and shape == (B, Cout):
        return (m != 0).to(torch.uint8).contiguous(), False
    if ok and shape in ((B, Cout, H, W), (B, 1, H, W)):
        return (m != 0).to(torch.uint8).expand(B, Cout, H, W).contiguous(), True
    raise error(f"{prefix}pixel_mask is {'a ' + str(m.dtype) + ' tensor of shape ' + str(shape) if shape is not None else repr(type(m))}: a "
                f"training plan takes a bool mask of shape {(B, Cout)} (whole planes), {(B, Cout, H, W)} or {(B, 1, H, W)} (elements)")


def _check_adjoint(model, adjoint):
    adjoint = tuple(sorted(set(adjoint or ())))
    if not set(adjoint) <= {"pixel_values", "time"}:
        raise PlanExportError(f"export_plan: adjoint names unknown input(s) {sorted(set(adjoint) - {'pixel_values', 'time'})}; a plan "
                              "differentiates with respect to pixel_values and time")
    if "time" in adjoint and not model.config.use_conditioning:
        raise PlanExportError("export_plan: adjoint=('time',) needs use_conditioning=True: this model's prediction does not depend on time")
    return adjoint


def _check_training(model, pixel_values, labels, train, adjoint):
    """the refusals of a training export that need more than the request's shapes; nothing has been recorded yet"""
    from .optim import FusedAdamW
    if adjoint:
        raise PlanExportError("export_plan: adjoint= together with train=: a training plan differentiates with respect to the "
                              "parameters; export the input adjoint as an image of its own")
    if labels is None:
        raise PlanExportError("export_plan: train= without labels: a training plan records the loss, so it needs example labels "
                              "[B, num_out_channels, H, W]")
    if not isinstance(train, FusedAdamW) or train.model is not model:
        raise PlanExportError("export_plan: train= takes the optimizer whose step is recorded: a poseidon_amd.optim.FusedAdamW built "
                              "over this very model")
    frozen = [n for n, p in model.named_parameters() if not p.requires_grad]
    if frozen:
        raise PlanExportError(f"export_plan: {len(frozen)} parameter(s) have requires_grad=False ({frozen[0]}, ...): a partially frozen "
                              "model cannot be exported for training (the recorded backward is all-or-nothing)")
    eng = model._engine
    if eng.on_grads_final is not None or model._grad_hooks:
        raise PlanExportError("export_plan: a data-parallel reducer is attached to this model: a training plan is one device's step "
                              "(detach the reducer first)")
    want = (pixel_values.shape[0], model.config.num_out_channels, pixel_values.shape[2], pixel_values.shape[3])
    if tuple(labels.shape) != want:
        raise PlanExportError(f"export_plan: labels have shape {tuple(labels.shape)}, the model's output has {want}")


def _kind(const):
    return STATE if const in ("state", "stored") else (CONSTANT if const else SCRATCH)


def _register(reg, buffers, only_new=False):
    for name, ten, const in buffers:
        if not (only_new and ten.data_ptr() in reg.bufs):
            if const == "stored":
                reg.add(ten, STATE, name, stored=True)
            else:
                reg.add(ten, _kind(const), name)


_ENGINE_SWITCHES = ("use_side", "stage_timing", "stochastic", "collect_attn")
_ENGINE_SAVED = _ENGINE_SWITCHES + ("last_hidden", "last_hidden_aliased", "_rec", "_rec_keep", "_fwd_flags")


@contextlib.contextmanager
def _recording(eng, reg, side_rows, refresh, extra_saved=(), snapshot=None, streams=1):
    """What every export's recording run needs around it -> (recorded calls, kept tensors), both filled by the body: the engine's build
    of the library in use, the 16-bit weight copies current (`refresh`: the transposed ones too; never part of a recording), the
    engine's switches off, `ops.workspace` registering itself, the registry and the recorder installed — and all of it put back
    afterwards.  snapshot() is called once the copies are current and returns what to call right after the recorder has been taken out.
    streams=2: the weight-gradient stream stays ON (and the one-stream stand-in for its rows off): the recording is the engine's own
    two-stream program, and reg.streams classifies its stream handles afterwards.  An engine on the CPU emulation records it over
    stand-in handles (engine._cur_stream)."""
    from . import ops
    inner_workspace = ops.workspace

    def workspace(need=0):      # the split-K scratch of the wrappers is an allocation funnel too
        w = inner_workspace(need)
        reg.add(w, SCRATCH, "workspace")
        return w
    saved = {k: getattr(eng, k) for k in _ENGINE_SAVED + tuple(extra_saved) + (("side", "_standin") if streams == 2 else ())}
    rec, keep = [], []
    prev_lib = ops.use(eng.lib_kind)
    try:
        eng.refresh_weight_copies(refresh)
        put_back = snapshot() if snapshot is not None else None
        ops.workspace = workspace
        for k in _ENGINE_SWITCHES:
            setattr(eng, k, False)
        eng._export, eng._rec, eng._rec_keep = reg, rec, keep
        eng._export_side_rows = side_rows and streams != 2
        if streams == 2:
            from .engine import _StandIn
            eng.use_side = True
            if eng.device.type != "cuda":
                eng.side, eng._standin = None, dict(cur=_StandIn(ops.stream()), events=0)
            main = _handle(ops.stream())
        prev_rec = ops.set_recorder(rec)
        try:
            yield rec, keep
        finally:
            ops.set_recorder(prev_rec)
            if streams == 2:
                reg.streams = {main: 0}
                if eng.side is not None:
                    reg.streams.setdefault(_handle(eng.side.cuda_stream), 1)
            if put_back is not None:
                put_back()
    finally:
        ops.workspace = inner_workspace
        eng._export = None
        for k, v in saved.items():
            setattr(eng, k, v)
        ops.use(prev_lib)


def _handle(v):
    """a stream or event handle among recorded arguments -> int (0: the default stream)"""
    if v is None:
        return 0
    return (v.value or 0) if isinstance(v, ctypes.c_void_p) else int(v)


def _input_copies(reg, pv, t):
    pv_in = pv.clone()
    t_in = None if t is None else t.clone()
    reg.add(pv_in, INPUT, "pixel_values")
    if t_in is not None:
        reg.add(t_in, INPUT, "time")
    return pv_in, t_in


class _Resize:
    """The two resamplings around the engine of a plan at a foreign resolution r (export_plan(..., resize=True)), each ONE
    scot_spectral_resize call through `ops` — so a recording sees it: `into` r -> image_size in front of the forward, `back` image_size
    -> r behind it, and their adjoints (the same call with the transposed operators) around the backward.  What ScOT.forward runs with
    `fused_resize = True`, call for call."""

    def __init__(self, model, r, device):
        from scOT.model import _resize_mats
        self.r, self.S = int(r), int(model.config.image_size)
        self.m_in, self.m_out = _resize_mats(self.r, self.S, device), _resize_mats(self.S, self.r, device)

    def constants(self, adjoint):
        """[(name, operator matrix)] a plan's lists name"""
        keys = ("pr", "pi") + (("prT", "piT") if adjoint else ())
        return [(f"resize_{side}_{k}", m[k]) for side, m in (("in", self.m_in), ("out", self.m_out)) for k in keys]

    @staticmethod
    def _apply(x, pr, pi, s, t, out=None):
        import torch
        from . import ops
        if out is None:
            out = torch.empty(*x.shape[:-2], t, t, dtype=torch.float32, device=x.device)
        ops.spectral_resize(x, pr, pi, out, x.numel() // (s * s), s, t)
        return out

    def into(self, x, out=None):
        return self._apply(x, self.m_in["pr"], self.m_in["pi"], self.r, self.S, out)

    def back(self, y, out=None):
        return self._apply(y, self.m_out["pr"], self.m_out["pi"], self.S, self.r, out)

    def back_adjoint(self, g, out=None):      # a cotangent at r -> at image_size
        return self._apply(g, self.m_out["prT"], self.m_out["piT"], self.r, self.S, out)

    def into_adjoint(self, g, out=None):      # d_pixel_values at image_size -> at r
        return self._apply(g, self.m_in["prT"], self.m_in["piT"], self.S, self.r, out)


def _record(model, pv, t, adjoint=(), streams=1, rs=None):
    """-> (registry, recorded calls, kept tensors, prediction tensor, input copies, adjoint record or None): ONE dedicated, linear
    recording of engine._forward — with `adjoint`, of the forward a differentiable call runs (train=True without stochastic depth,
    these input gradients, no parameter gradient) followed by engine._backward from a cotangent of the prediction alone; the adjoint
    record holds where the second list starts and the cotangent / gradient tensors.
    rs (a _Resize; pv is at its r): the forward list is resize, engine forward, resize; the backward list resize adjoint, engine
    backward, resize adjoint.  The resampled tensors are scratch of the plan, the operator matrices constants."""
    import torch
    eng = model._engine
    reg = _Registry()
    _register(reg, eng.plan_buffers(adjoint=bool(adjoint)))
    pv_in, t_in = _input_copies(reg, pv, t)
    B, S, dev = pv.shape[0], model.config.image_size, pv.device
    Cin, Cout = pv.shape[1], model.config.num_out_channels

    def room(name, *shape):
        x = torch.empty(*shape, dtype=torch.float32, device=dev)
        reg.add(x, SCRATCH, name)
        return x
    if rs is not None:
        for name, m in rs.constants(bool(adjoint)):
            reg.add(m, CONSTANT, name)
        pv_s, pred_r = room("resized input", B, Cin, S, S), room("resized prediction", B, Cout, rs.r, rs.r)
    adj = None
    if adjoint:
        cot = torch.zeros(B, Cout, pv.shape[2], pv.shape[3], dtype=torch.float32, device=dev)
        reg.add(cot, INPUT, "d_prediction")
    with _recording(eng, reg, bool(eng.use_side and not eng.stage_timing), bool(adjoint), streams=streams) as (rec, keep):
        x = pv_in if rs is None else rs.into(pv_in, pv_s)
        if adjoint:      # forced for the export, whatever the caller's tensors require
            eng._fwd_flags = (adjoint, False)
            _, pred, tape = eng._forward(x, t_in, None, None, True)
            if rs is not None:
                pred = rs.back(pred, pred_r)
            n_fwd = len(rec)
            cot.copy_(pred / float(pred.numel()))      # (a value for the recording run; a vjp copies the caller's in)
            counted = None if eng.grad_overflow is None else eng.grad_overflow.clone()
            d_pv, d_t = eng._backward(tape, None, cot if rs is None else rs.back_adjoint(cot, room("resized cotangent", B, Cout, S, S)))
            if rs is not None and d_pv is not None:
                d_pv = rs.into_adjoint(d_pv, room("resized d_pixel_values", B, Cin, rs.r, rs.r))
            if counted is not None:      # (the recording run is not a step of the model's: its un-scale passes do not count)
                eng.grad_overflow.copy_(counted)
            keep.append(tape)
            adj = dict(n_fwd=n_fwd, cot=cot, d_pv=d_pv, d_t=d_t)
        else:
            _, pred, _ = eng._forward(x, t_in, None, None, False)
            if rs is not None:
                pred = rs.back(pred, pred_r)
    _register(reg, eng.plan_buffers(adjoint=bool(adjoint)), only_new=True)      # (tables the forward created on first use)
    return reg, rec, keep, pred, pv_in, t_in, adj


def _training_state(model, opt):
    """every tensor a training step changes, in a fixed order"""
    eng = model._engine
    ts = [eng.arena.data, opt.exp_avg, opt.exp_avg_sq, opt._step_state, opt._clip]
    ts += [x for x in (eng.shadow, eng.shadow_t, eng.scale_state, eng.grad_overflow) if x is not None]
    ts += [ls["scratch"] for _, ls in sorted(eng._ls.items())]
    return ts


def _record_training(model, opt, pv, t, labels, streams=1, mask=None):
    """-> (registry, recorded calls, kept tensors, inference prediction, input copies, training record): ONE linear recording of four
    lists on one stream — the inference forward; the step's forward through the loss; the fill of the accumulated gradients, the
    backward from d loss = 1 with the store-form weight gradients and the un-scale passes; what FusedAdamW.step issues.  The recording
    run IS a step on the model's own tensors, so everything it changes is saved before and put back afterwards.
    streams=2: the engine's two-stream step; the fill is the side stream's first task of the step backward, and the main stream waits for
    it before the backward's first entry.
    mask (uint8 [B, Cout] or [B, Cout, H, W]): the step is recorded with a pixel_mask.  The engine's own byte mask is a fresh tensor it
    fills with a torch copy — no C-ABI call —, so the export hands it the plan's mask INPUT to use as that tensor (engine._forward): the
    recorded scot_head_finalize / scot_loss_bwd name the input buffer, and the runtime copies the caller's bytes there."""
    import torch
    from . import ops
    eng = model._engine
    reg = _Registry()
    _register(reg, eng.plan_buffers(train=opt))
    pv_in, t_in = _input_copies(reg, pv, t)
    lab_in = labels.clone()
    reg.add(lab_in, INPUT, "labels")
    mask_in = None
    if mask is not None:
        mask_in = reg.mask_u8 = mask.clone()
        reg.add(mask_in, INPUT, "pixel_mask")
    one = None
    if not eng.scale_grads:      # d loss = 1 as a constant of the image (under a gradient scale the backward copies S from the state)
        one = torch.ones(1, dtype=torch.float32, device=pv.device)
        reg.add(one, CONSTANT, "one")
    state = _training_state(model, opt)

    def snapshot():      # (both 16-bit copies are current by now: the image stores them by value)
        before, step_count = [x.clone() for x in state], opt.step_count
        grads_before = (eng.arena.grad.clone(), eng.grads_are_zero, eng.lazy_grads)      # (what the caller has accumulated so far)

        def put_back():
            with torch.no_grad():
                for x, b in zip(state, before):
                    x.copy_(b)
                eng.arena.grad.copy_(grads_before[0])
            opt.step_count = step_count
            eng.grads_are_zero, eng.lazy_grads = grads_before[1], grads_before[2]
            model.mark_weights_dirty()
            if eng.shadow is not None:      # (put back with the master weights: current again)
                eng._shadow_v = eng._shadow_t_v = model._weights_version()
        return put_back
    with _recording(eng, reg, False, True, extra_saved=("grad_fill_event",), snapshot=snapshot, streams=streams) as (rec, keep):
        eng.grad_fill_event = None
        eng._fwd_flags = ((), True)
        _, pred, _ = eng._forward(pv_in, t_in, None, None, False)
        n_inf = len(rec)
        loss, pred_step, tape = eng._forward(pv_in, t_in, lab_in, mask_in, True)
        n_fwd = len(rec)
        _register(reg, eng.plan_buffers(train=opt), only_new=True)
        lazy = eng._small_chunks is not None      # ScOT.zero_grad(overlap=True): only what is accumulated into is filled

        def fill():
            if lazy:
                eng.fill_small_grads()
            else:
                ops.memset_async(eng.arena.grad, 0)
        _, filled = eng.fork_task(fill) if streams == 2 else (fill(), None)
        eng.wait_task(filled)      # (both streams write gradients: the fill is in front of the first writer on either)
        eng.grads_are_zero, eng.lazy_grads = True, lazy
        eng._backward(tape, one, None)
        eng.grads_are_zero = eng.lazy_grads = False
        n_bwd = len(rec)
        opt.step()
        keep.append(tape)
    _register(reg, eng.plan_buffers(train=opt), only_new=True)      # (tables the step created on first use)
    tr = dict(n_inf=n_inf, n_fwd=n_fwd, n_bwd=n_bwd, labels=lab_in, loss=loss, pred=pred_step, opt=opt, mask=mask_in)
    return reg, rec, keep, pred, pv_in, t_in, tr


def _libraries(eng):
    """(the engine's build of the library, the bfloat16 build if that is another one)"""
    from . import ops
    prev = ops.use(eng.lib_kind)
    try:
        own = ops._raw()
        ops.use("bf16")
        peer = ops._raw() if eng.lib_kind != "bf16" else None
    finally:
        ops.use(prev)
    return own, peer


def _bytes_of(t):
    return t.detach().reshape(-1).cpu().contiguous().view(__import__("torch").uint8).numpy().tobytes()


class _CallList:
    """one recorded call list on its way into an image: `what` it is (in messages, and its section's name in the layout), the table of
    entry points it is held to, where it ends in the recording; then its encoded entries and the buffers its arguments touch"""

    def __init__(self, what, table, end, own):
        self.what, self.table, self.end = what, table, end
        self.macro = ENTRY_POINT_TABLES[table][1]
        self.listed = set(runtime_entry_points(own, **({} if table == "forward" else {table: True})))
        self.entries, self.touched = [], set()

    def words(self):
        ws = []
        for name, which, ints, flts in self.entries:
            ws += [name, which, len(ints), len(flts)]
            for tag, val in ints:
                ws += [tag, val]
            ws += flts
        return ws


class _Relocator:
    """device addresses -> (buffer index, byte offset) over the frozen registry; `used` numbers the buffers in the order of first use"""

    def __init__(self, reg):
        self.reg, self.used, self._index = reg, [], {}

    def index(self, b):
        i = self._index.get(b["addr"])
        if i is None:
            i = self._index[b["addr"]] = len(self.used)
            self.used.append(b)
        return i

    def pair(self, value, what, touched):
        """a device address among a call's arguments -> argument pair"""
        if not value:
            return (ARG_NULL, 0)
        b, off = self.reg.resolve(value)
        if b is None:
            raise PlanExportError(f"export_plan: {what} is a device address (0x{value:x}) inside no buffer the export registered")
        touched.add(b["addr"])
        return (ARG_PTR | (self.index(b) << 8), off)

    def span(self, t, what, kind):
        """a tensor the runtime itself addresses -> [buffer index, byte offset, bytes]; its buffer becomes one of `kind`"""
        n = t.numel() * t.element_size()
        b, off = self.reg.resolve(t.data_ptr())
        if b is None or off + n > b["bytes"]:
            raise PlanExportError(f"export_plan: {what} lies in no registered buffer")
        b["kind"] = kind
        return [self.index(b), off, n]

    def kept_bytes(self, first, second):
        """what `first` leaves for `second`: the scratch both lists name (saved activations; the split-K workspace aside)"""
        both = first.touched & second.touched
        return sum(b["bytes"] for b in self.used if b["addr"] in both and b["kind"] == SCRATCH and b["name"] != "workspace")


def _float_bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def _sync_pairs(name, args, streams, events):
    """the argument pairs of a recorded scot_event_record (EVENT, STREAM) / scot_stream_wait_event (STREAM, EVENT); events get their
    indices in order of first appearance"""
    ev, st = (args[0], args[1]) if name == RECORD else (args[1], args[0])
    if _handle(st) not in streams:
        raise PlanExportError(f"export_plan: {name} names stream 0x{_handle(st):x}, which is neither the current stream nor the engine's "
                              "side stream: a plan has two streams")
    pair = {"e": (ARG_EVENT, events.setdefault(_handle(ev), len(events))), "s": (ARG_STREAM, streams[_handle(st)])}
    return [pair["e"], pair["s"]] if name == RECORD else [pair["s"], pair["e"]]


def _side_open(entries, names):
    """the closed-list rule of csrc/plan_image.h over encoded entries -> whether the list leaves stream 1 unjoined (the first two
    rules — a wait pairs with an earlier record of the list, stream 1 starts behind a record of stream 0 — raise)"""
    recorded, side, join_event = {}, 0, None
    for name, _, ints, _ in entries:
        on = max([v for tag, v in ints if tag == ARG_STREAM], default=0)
        ev = next((v for tag, v in ints if tag == ARG_EVENT), None)
        kind = names[name] if names[name] in (RECORD, WAIT) else None
        if kind == WAIT and ev not in recorded:
            raise PlanExportError("export_plan: a recorded stream wait pairs with no earlier event record of its own list")
        if on:
            if not side and not (kind == WAIT and recorded[ev] == 0):
                raise PlanExportError("export_plan: the side stream's first entry of a list is not ordered behind the main stream")
            side, join_event = 1, (ev if kind == RECORD else None)
        elif kind == WAIT and ev == join_event and recorded[ev] == 1:
            side = 2
        if kind == RECORD:
            recorded[ev] = on
    return side == 1


def _encode_calls(rec, lists, loc, own, peer, host_floats, streams=None):
    """(a) the recorded calls -> the entries of the list each falls into.  -> (names, host arrays, lr patch point or None: (entry,
    argument, groups) of the scot_adamw_step call, number of events).  host_floats: classify HOST_FLOAT_ARRAYS (a training recording).
    streams ({handle: index}, a two-stream recording): stream arguments become their index, the record / wait entries stay in the
    lists over event indices, and a list the engine leaves with the side stream unjoined gets the join appended"""
    names, name_index, arrays, lr_point, events = [], {}, [], None, {}

    def name_of(name):
        if name not in name_index:
            name_index[name] = len(names)
            names.append(name)
        return name_index[name]
    for pos, (fn, args) in enumerate(rec):
        lst = next(x for x in lists if pos < x.end)
        if args is None:
            label = getattr(fn, "__qualname__", None) or getattr(fn, "__name__", None) or repr(fn)
            raise PlanExportError(f"export_plan: the recorded {lst.what} holds a host-side Python step ({label}); a plan is C-ABI calls only")
        name = fn.__name__
        if streams is not None and name in (RECORD, WAIT):
            lst.entries.append((name_of(name), 0, _sync_pairs(name, args, streams, events), []))
            continue
        if name not in lst.listed:
            raise PlanExportError(f"export_plan: the {lst.what} calls {name}, which the plan runtime of this library does not list "
                                  f"(csrc/plan_image.h, {lst.macro})")
        addr = _address(fn)
        if addr == _address(getattr(own, name)):
            which = 0
        elif peer is not None and addr == _address(getattr(peer, name)):
            which = 1
        else:
            raise PlanExportError(f"export_plan: {name} was recorded from a library that is neither the engine's build nor the bfloat16 build")
        argtypes = fn.argtypes
        if len(args) != len(argtypes):
            raise PlanExportError(f"export_plan: {name} was recorded with {len(args)} arguments, its prototype has {len(argtypes)}")
        ints, flts = [], []
        last = len(args) - 1
        for k, (a, ty) in enumerate(zip(args, argtypes)):
            what = f"argument {k} of {name}"
            if ty is ctypes.c_float:
                flts.append(_float_bits(a))
            elif host_floats and k in HOST_FLOAT_ARRAYS.get(name, ()):      # a host array of floats, passed by address
                count = int(args[HOST_FLOAT_ARRAYS[name][k]])
                values = (ctypes.c_float * count).from_address(a.value if isinstance(a, ctypes.c_void_p) else int(a))
                if (name, k) == LR_ARGUMENT:
                    if lr_point is not None:
                        raise PlanExportError(f"export_plan: the update calls {name} more than once")
                    lr_point = (len(lst.entries), len(ints), count)
                ints.append((ARG_ARRAY, len(arrays)))
                arrays.append((2, [(ARG_INT, _float_bits(x)) for x in values]))
            elif ty is ctypes.c_void_p and k == last:
                if streams is not None and _handle(a) not in streams:
                    raise PlanExportError(f"export_plan: {name} was issued on stream 0x{_handle(a):x}, which is neither the current "
                                          "stream nor the engine's side stream: a plan has two streams")
                # one stream per entry point, last: the caller's at run time (a two-stream plan: 1 = its side stream)
                ints.append((ARG_STREAM, 0 if streams is None else streams[_handle(a)]))
            elif isinstance(a, ctypes.Array):
                elem = a._type_
                if elem is ctypes.c_int:
                    items = [(ARG_INT, int(x) & 0xFFFFFFFFFFFFFFFF) for x in a]
                    kind = 0
                elif elem is ctypes.c_void_p:
                    items = [loc.pair(x or 0, f"element {j} of {what}", lst.touched) for j, x in enumerate(a)]
                    kind = 1
                else:
                    raise PlanExportError(f"export_plan: {what} is a host array of {elem!r}")
                ints.append((ARG_ARRAY, len(arrays)))
                arrays.append((kind, items))
            elif ty is ctypes.c_void_p:
                v = a.value if isinstance(a, ctypes.c_void_p) else a
                ints.append(loc.pair(int(v or 0), what, lst.touched))
            elif a is None:
                ints.append((ARG_INT, 0))
            elif isinstance(a, int):
                ints.append((ARG_INT, a & 0xFFFFFFFFFFFFFFFF))
            else:
                raise PlanExportError(f"export_plan: {what} = {a!r} has no place in a plan image")
        if len(ints) > MAX_INT or len(flts) > MAX_FLT:
            raise PlanExportError(f"export_plan: {name} does not fit the replay's calling convention")
        lst.entries.append((name_of(name), which, ints, flts))
    for lst in lists if streams is not None else ():
        if _side_open(lst.entries, names):      # the engine joins its side stream where the NEXT list needs it: a list is closed
            ev = len(events)
            events[("join", lst.what)] = ev
            lst.entries.append((name_of(RECORD), 0, [(ARG_EVENT, ev), (ARG_STREAM, 1)], []))
            lst.entries.append((name_of(WAIT), 0, [(ARG_STREAM, 0), (ARG_EVENT, ev)], []))
    if len(events) > MAX_EVENTS:
        raise PlanExportError(f"export_plan: the recording holds {len(events)} events, an image at most {MAX_EVENTS}")
    return names, arrays, lr_point, len(events)


def _adjoint_words(eng, loc, adj, forward, backward):
    """(b) the adjoint words of a format-2 image"""
    w = [0] * ADJ_WORDS
    w[ADJ_COT:ADJ_COT + 3] = loc.span(adj["cot"], "the cotangent copy", INPUT)
    if adj["d_pv"] is not None:
        w[ADJ_FLAGS] |= 1
        w[ADJ_DPV:ADJ_DPV + 3] = loc.span(adj["d_pv"], "d_pixel_values", OUTPUT)
    if adj["d_t"] is not None:
        w[ADJ_FLAGS] |= 2
        w[ADJ_DTIME:ADJ_DTIME + 3] = loc.span(adj["d_t"], "d_time", OUTPUT)
    if eng.scale_grads:
        import math
        w[ADJ_STATE:ADJ_STATE + 3] = loc.span(eng.scale_state, "the gradient-scale state", STATE)
        w[ADJ_COUNTER:ADJ_COUNTER + 3] = loc.span(eng.grad_overflow, "the non-finite counter", STATE)
        S = eng.grad_scale_value()
        m, e = math.frexp(S)
        if m != 0.5:
            raise PlanExportError(f"export_plan: the engine's gradient scale {S} is not a power of two")
        w[ADJ_SCALE_EXP] = (e - 1) & 0xFFFFFFFFFFFFFFFF
    w[ADJ_KEPT_BYTES] = loc.kept_bytes(forward, backward)      # what a run leaves for the vjp (the prediction aside)
    return w


def _training_words(eng, loc, train, names, lr_point, step_forward, step_backward, update):
    """(b) the training words of a format-4 image, but for the three lists' places in the file (the layout's)"""
    opt = train["opt"]
    if lr_point is None or names[update.entries[lr_point[0]][0]] != LR_ARGUMENT[0]:
        raise PlanExportError("export_plan: the recorded update holds no scot_adamw_step call")
    w = [0] * TRAIN_WORDS
    for slot, t, what, kind in ((TR_LABELS, train["labels"], "the labels' copy", INPUT), (TR_LOSS, train["loss"], "the loss", OUTPUT),
                                (TR_PRED, train["pred"], "the step forward's prediction", OUTPUT),
                                (TR_ARENA, eng.arena.data, "the parameter arena", STATE), (TR_EXP_AVG, opt.exp_avg, "exp_avg", STATE),
                                (TR_EXP_AVG_SQ, opt.exp_avg_sq, "exp_avg_sq", STATE), (TR_SHADOW, eng.shadow, "the 16-bit copy", STATE),
                                (TR_SHADOW_T, eng.shadow_t, "the transposed 16-bit copy", STATE),
                                (TR_STEP_STATE, opt._step_state, "step_state", STATE), (TR_CLIP, opt._clip, "the clip floats", STATE),
                                (TR_SCALE_STATE, eng.scale_state, "the gradient-scale state", STATE),
                                (TR_COUNTER, eng.grad_overflow, "the non-finite counter", STATE)):
        if t is not None:
            w[slot:slot + 3] = loc.span(t, what, kind)
    w[TR_FLAGS] = TR_FLAG_DYNAMIC if eng.scale_grads else 0
    if train.get("mask") is not None:
        w[TR_FLAGS] |= TR_FLAG_MASK | (TR_FLAG_MASK_FULL if train["mask"].dim() == 4 else 0)
    w[TR_GROUPS], w[TR_ARENA_FLOATS] = lr_point[2], eng.arena.size
    w[TR_LR_ENTRY], w[TR_LR_ARG] = lr_point[0], lr_point[1]
    w[TR_KEPT_BYTES] = loc.kept_bytes(step_forward, step_backward)
    if len(opt.param_groups) != lr_point[2]:
        raise PlanExportError("export_plan: the recorded update has another number of parameter groups than the optimizer")
    return w


def _layout(sections):
    """(c) {section name: bytes} in file order -> ({section name: offset in the file}, offset of the data section): every section on an
    8-byte boundary behind the header, the data on a 64-byte boundary behind the last one"""
    offs, cur = {}, HEADER_WORDS * 8
    for name, sct in sections.items():
        offs[name] = cur
        cur += len(sct) + (-len(sct) % 8)
    return offs, cur + (-cur % 64)


def build_image(model, reg, rec, pred, pv_in, t_in, own, peer, adj=None, train=None, streams=1):
    """recorded calls + registered buffers -> the bytes of a plan image (adj: the adjoint record of _record -> a format-2 image; train:
    the training record of _record_training -> a format-4 image)"""
    eng = model._engine
    reg.freeze()
    loc = _Relocator(reg)
    if train is not None:
        ends = zip(("step forward", "step backward", "update"), (train["n_fwd"], train["n_bwd"], len(rec)))
        lists = [_CallList("forward", "forward", train["n_inf"], own)] + [_CallList(what, "training", end, own) for what, end in ends]
    elif adj is not None:
        lists = [_CallList("forward", "forward", adj["n_fwd"], own), _CallList("backward", "adjoint", len(rec), own)]
    else:
        lists = [_CallList("forward", "forward", len(rec), own)]
    forward, others = lists[0], lists[1:]
    names, arrays, lr_point, n_events = _encode_calls(rec, lists, loc, own, peer, host_floats=train is not None,
                                                      streams=reg.streams if streams == 2 else None)

    io = [0] * IO_WORDS
    io[0:5] = [*pv_in.shape, pred.shape[1]]      # B, Cin, H, W, Cout
    io[5:7] = loc.span(pv_in, "the input copy", INPUT)[:2]
    if t_in is not None:
        io[7] = 1
        io[8:11] = loc.span(t_in, "the time copy", INPUT)
    if train is not None and train.get("mask") is not None:
        io[IO_HAS_MASK] = 1
        io[IO_MASK_BUF:IO_MASK_BUF + 3] = loc.span(train["mask"], "the mask copy", INPUT)
    io[15:17] = loc.span(pred, "the prediction", OUTPUT)[:2]
    adj_words = _adjoint_words(eng, loc, adj, forward, *others) if adj is not None else None
    tr_words = _training_words(eng, loc, train, names, lr_point, *others) if train is not None else None

    def words(ws):
        return struct.pack(f"<{len(ws)}Q", *ws)
    data, buf_words = bytearray(), []
    for b in loc.used:
        off = 0
        stored = b["kind"] == STATE and b["stored"] and train is not None
        if b["kind"] == CONSTANT or stored:
            data.extend(b"\0" * (-len(data) % 64))
            off = len(data)
            raw = _bytes_of(b["tensor"])
            assert len(raw) == b["bytes"]
            data.extend(raw)
        buf_words += [b["kind"], b["bytes"], off, 1 if stored else 0]
    data.extend(b"\0" * (-len(data) % 8))
    arr_words = []
    for kind, items in arrays:
        arr_words += [kind, len(items)]
        for tag, val in items:
            arr_words += [tag, val]
    # the sections in file order; a list's section has the list's name
    sections = {"names": b"".join(n.encode().ljust(NAME_BYTES, b"\0") for n in names), "buffers": words(buf_words),
                "forward": words(forward.words()), "arrays": words(arr_words), "io": words(io)}
    sections.update((x.what, words(x.words())) for x in others)
    if adj is not None:
        sections["adjoint"] = words(adj_words)
    if train is not None:
        sections["training"] = bytes(TRAIN_WORDS * 8)      # (names the step lists' offsets: filled in once they are known)
    if streams == 2:
        sections["streams"] = words([2, n_events])
    offs, data_off = _layout(sections)

    def named(x):      # how a header or the training words name a list: (count, offset, words)
        return [len(x.entries), offs[x.what], len(sections[x.what]) // 8]
    h = [0] * HEADER_WORDS
    h[H_MAGIC], h[H_FORMAT], h[H_ABI], h[H_OPERAND] = MAGIC, FORMAT, own.scot_abi_version(), own.scot_operand_format()
    h[H_COMPUTE], h[H_BYTES] = COMPUTE_CODE[model.compute], data_off + len(data)
    h[H_NNAMES], h[H_NAMES_OFF] = len(names), offs["names"]
    h[H_NBUFFERS], h[H_BUFFERS_OFF] = len(loc.used), offs["buffers"]
    h[H_NENTRIES:H_NENTRIES + 3] = named(forward)
    h[H_NARRAYS], h[H_ARRAYS_OFF], h[H_ARRAYS_WORDS] = len(arrays), offs["arrays"], len(arr_words)
    h[H_IO_OFF], h[H_DATA_OFF], h[H_DATA_BYTES] = offs["io"], data_off, len(data)
    if adj is not None:
        (backward,) = others
        h[H_FORMAT], h[H_ADJ_OFF] = FORMAT_ADJOINT, offs["adjoint"]
        h[H_NBACKWARD:H_NBACKWARD + 3] = named(backward)
    if train is not None:
        h[H_FORMAT], h[H_TRAIN_OFF] = FORMAT_TRAINING, offs["training"]
        for slot, x in zip((TR_FWD, TR_BWD, TR_UPD), others):
            tr_words[slot:slot + 3] = named(x)
        sections["training"] = words(tr_words)
    if streams == 2:
        h[H_FORMAT], h[H_STREAMS_OFF] = STREAMED[h[H_FORMAT]], offs["streams"]
    out = bytearray(words(h))
    for name, sct in sections.items():
        assert len(out) == offs[name]
        out.extend(sct)
        out.extend(b"\0" * (-len(sct) % 8))
    out.extend(b"\0" * (data_off - len(out)))
    out.extend(data)
    assert len(out) == h[H_BYTES]
    return bytes(out)


def export_plan(model, pixel_values, time=None, pixel_mask=None, path=None, labels=None, *, adjoint=(), train=None, streams=1, resize=False):
    """Record `model`'s inference forward for exactly these input shapes and write it as a plan image to `path` (None: only return it).
    Returns the image's bytes.  The weights are a snapshot; see the module docstring and DESIGN.md §3 for what a plan does not cover.
    adjoint: () or some of ("pixel_values", "time") — the image (format 2) then also holds the frozen-model backward from a cotangent of
    the prediction to these inputs' gradients (scot_plan_vjp), and its forward is the one a differentiable call runs.
    train: a FusedAdamW over this model, with labels — the image (format 4) then also holds one optimizer step and the training state by
    value (scot_plan_train_step, scot_plan_snapshot); the model and the optimizer are left as they were.
    pixel_mask (with train= only): bool [B, Cout] (a channel mask), [B, Cout, H, W] or [B, 1, H, W] (an element mask) — the step is
    recorded with the reference's mask (`prediction[pixel_mask] = labels[pixel_mask]` before the loss), the image has the mask as one
    more input, and every batch brings its own (scot_plan_loss_masked, scot_plan_train_step_masked).
    streams: 1, or 2 — the image (format 5, with train= format 6) then holds the engine's two-stream program, and the runtime runs the
    bias tables, the skip blocks and the weight gradients on a side stream of its own beside the main chain.  Not with adjoint=.
    resize: True — square inputs of a size r other than config.image_size are accepted (inference, adjoint and two-stream plans, not
    train=): the forward list becomes one scot_spectral_resize from the input [B, Cin, r, r] to image_size, the engine's forward, and
    one scot_spectral_resize of its prediction to [B, Cout, r, r]; an adjoint plan's backward list gets the two adjoints around the
    engine's backward.  The plan then takes and returns tensors at r, bit-identical to the model with `fused_resize = True`.  At
    r == image_size the image is the one resize=False gives."""
    import torch
    if streams not in (1, 2):
        raise PlanExportError(f"export_plan: streams={streams!r}: a plan runs on 1 stream or on 2 (the caller's and one side stream)")
    if streams == 2 and adjoint:
        raise PlanExportError("export_plan: adjoint= together with streams=2: an adjoint plan runs on one stream (the frozen backward has "
                              "no weight-gradient stream to put beside the main chain)")
    _check_request(model, pixel_values, time, pixel_mask, labels, train, resize)
    dev = pixel_values.device
    if train is not None:
        model._ensure_arena(dev)
        _check_training(model, pixel_values, labels, train, adjoint)
    adjoint = _check_adjoint(model, adjoint)
    model._ensure_arena(dev)
    pv = pixel_values.detach().to(torch.float32).contiguous()
    t = None
    if model.config.use_conditioning:      # as ScOT.forward prepares it
        t = torch.as_tensor(time, device=dev).detach().reshape(-1).to(torch.float32).contiguous()
        if t.numel() == 1 and pv.shape[0] > 1:
            t = t.expand(pv.shape[0]).contiguous()
        if t.numel() != pv.shape[0]:
            raise PlanExportError(f"export_plan: time has {t.numel()} values for a batch of {pv.shape[0]}")
    own, peer = _libraries(model._engine)
    bind(own)
    with torch.no_grad():
        if train is not None:
            mask = None
            if pixel_mask is not None:
                mask = _mask_bytes(pixel_mask, pv.shape[0], model.config.num_out_channels, pv.shape[2], pv.shape[3])[0].to(dev)
            image = _export_training(model, train, pv, t, labels.detach().to(device=dev, dtype=torch.float32).contiguous(), own, peer, streams,
                                     mask)
        else:
            image = _export_frozen(model, pv, t, adjoint, own, peer, streams, resize)
    if path is not None:
        with open(path, "wb") as f:
            f.write(image)
    return image


@contextlib.contextmanager
def _self_check(image, own, peer):
    """the image that was built, loaded through the runtime with its scratch poisoned: a constant the export missed fails here, not at a
    user's site"""
    plan = Plan.load(image, lib=own, peer=peer)
    try:
        plan.poison(0xFF)
        yield plan
    finally:
        plan.free()


def _export_frozen(model, pv, t, adjoint, own, peer, streams=1, resize=False):
    """record, build, and check through the runtime: the model's own prediction bits and, with `adjoint`, the engine's own gradients.
    resize (pv at another size than config.image_size): the reference is resize(engine(resize(pv))) on the one-launch kernel, and for
    the gradients its adjoints around the engine's backward — what ScOT.forward computes with `fused_resize = True`."""
    import torch
    eng, dev = model._engine, pv.device
    ref_g = None
    rs = _Resize(model, pv.shape[2], dev) if resize and pv.shape[2] != model.config.image_size else None
    x = pv if rs is None else rs.into(pv)      # what the engine sees
    if adjoint:      # the engine's own bits of the differentiable call: its prediction, and a vjp
        _, ref, tape = eng.forward(x, t, None, None, train=True, stochastic=False, input_grads=adjoint, param_grads=False)
        ref = ref.clone() if rs is None else rs.back(ref)
        # (the cotangent of the self-check: the prediction brought to at most 1 / its element count — the magnitude a mean loss
        # hands back and the fp16 gradient scale is chosen for)
        cot = ref / (float(ref.numel()) * max(1.0, float(ref.abs().max())))
        counted = 0 if eng.grad_overflow is None else int(eng.grad_overflow)
        ref_g = eng.backward(tape, None, cot.clone() if rs is None else rs.back_adjoint(cot))
        if rs is not None and ref_g[0] is not None:
            ref_g = (rs.into_adjoint(ref_g[0]), ref_g[1])
        counted = 0 if eng.grad_overflow is None else int(eng.grad_overflow) - counted
        del tape
        for p in model._params:      # (as after any frozen backward: by-products of the fused tails may sit in the gradient arena)
            p.grad = None
    else:
        _, ref, _ = eng.forward(x, t, None, None, train=False, stochastic=False)      # the model's own prediction
        if rs is not None:
            ref = rs.back(ref)
    reg, rec, keep, pred, pv_in, t_in, adj = _record(model, pv, t, adjoint, streams, rs)
    image = build_image(model, reg, rec, pred, pv_in, t_in, own, peer, adj, streams=streams)
    with _self_check(image, own, peer) as plan:
        got = plan.run(pv, t)
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        if not bool(torch.isfinite(got).all()):
            raise PlanExportError("export_plan: the plan's prediction is not finite with poisoned scratch: the recorded forward reads "
                                  "a buffer the image does not initialise")
        if not torch.equal(got, ref):
            raise PlanExportError("export_plan: the plan's prediction differs from the model's own "
                                  f"(max |difference| {float((got - ref).abs().max()):.3e})")
        if adjoint:
            got_g = plan.vjp(cot.clone())
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            for name, a, b in zip(("d_pixel_values", "d_time"), got_g, ref_g):
                # the engine's own bits; where its fp16 backward overflowed, the same elements are non-finite (never clipped)
                same = (a is None) == (b is None)
                if same and a is not None:
                    fin = torch.isfinite(b)
                    same = torch.equal(torch.isfinite(a), fin) and torch.equal(a[fin], b[fin])
                if not same:
                    raise PlanExportError(f"export_plan: the plan's {name} differs from the engine's own for the export inputs")
            if plan.grad_status()[0] != counted:
                raise PlanExportError(f"export_plan: the plan's un-scale passes counted {plan.grad_status()[0]} non-finite values, the "
                                      f"engine's {counted}")
    del keep
    return image


def _export_training(model, opt, pv, t, lab, own, peer, streams=1, mask=None):
    """record, build, and check through the runtime: scratch poisoned, one scot_plan_loss and one scot_plan_train_step on the export
    inputs — the engine's own prediction bits, a finite loss, finite parameters.  The image that is returned holds the pre-step state."""
    import torch
    eng = model._engine
    # the engine's own prediction (under a mask: with the labels at the masked positions)
    _, ref, tape = eng.forward(pv, t, lab, None if mask is None else mask != 0, train=True, stochastic=False, param_grads=True)
    ref = ref.clone()
    del tape
    reg, rec, keep, pred, pv_in, t_in, tr = _record_training(model, opt, pv, t, lab, streams, mask)
    image = build_image(model, reg, rec, pred, pv_in, t_in, own, peer, train=tr, streams=streams)
    del keep
    with _self_check(image, own, peer) as plan:
        loss, got = plan.loss(pv, t, lab, pixel_mask=mask)
        if not torch.equal(got, ref):
            raise PlanExportError("export_plan: the training plan's prediction differs from the engine's own "
                                  f"(max |difference| {float((got - ref).abs().max()):.3e})")
        if not bool(torch.isfinite(loss).all()):
            raise PlanExportError("export_plan: the training plan's loss is not finite with poisoned scratch")
        plan.poison(0xFF)
        loss = plan.train_step(pv, t, lab, [float(g["lr"]) for g in opt.param_groups], pixel_mask=mask)
        if not bool(torch.isfinite(loss).all()):
            raise PlanExportError("export_plan: the loss of the training plan's step is not finite with poisoned scratch")
        after = training_state(plan.snapshot(image))
        if not bool(torch.isfinite(after["arena"]).all()):
            raise PlanExportError("export_plan: the parameters are not finite after one step of the training plan with poisoned scratch: "
                                  "the recorded step reads a buffer the image does not initialise")
    plan = Plan.load(image, lib=own, peer=peer)      # (the image as it will be written: the state before any step)
    plan.free()
    return image


_STATE_SPANS = (("arena", TR_ARENA, "float32"), ("exp_avg", TR_EXP_AVG, "float32"), ("exp_avg_sq", TR_EXP_AVG_SQ, "float32"),
                ("shadow", TR_SHADOW, "int16"), ("shadow_t", TR_SHADOW_T, "int16"), ("step_state", TR_STEP_STATE, "int32"),
                ("clip", TR_CLIP, "float32"), ("scale_state", TR_SCALE_STATE, "float32"), ("nonfinite", TR_COUNTER, "int32"))


def training_words(image):
    """the training words of a format-4 image (a tuple of TRAIN_WORDS ints)"""
    h = Plan.header(image)
    if h[H_FORMAT] not in (FORMAT_TRAINING, FORMAT_TRAINING_STREAMS):
        raise _lib.ScotLibraryError(f"not a training image: format {h[H_FORMAT]}")
    return struct.unpack_from(f"<{TRAIN_WORDS}Q", image, h[H_TRAIN_OFF])


def training_state(image):
    """{name: tensor} of the state a training image holds by value (copies; the 16-bit copies as raw int16): arena, exp_avg, exp_avg_sq,
    shadow, shadow_t, step_state, clip, scale_state, nonfinite — absent ones left out"""
    import torch
    h, tr = Plan.header(image), training_words(image)
    out = {}
    for name, slot, dtype in _STATE_SPANS:
        buf, off, n = tr[slot:slot + 3]
        if n:
            _, _, data_off, _ = struct.unpack_from("<4Q", image, h[H_BUFFERS_OFF] + 32 * buf)
            start = h[H_DATA_OFF] + data_off + off
            out[name] = torch.frombuffer(bytearray(image[start:start + n]), dtype=getattr(torch, dtype)).clone()
    return out


def load_training_state(image, model, optimizer=None):
    """Copy a training image's parameters into `model` (a ScOT of the same configuration: the arena layout is the configuration's, so
    no name table is needed) and, with `optimizer` (its FusedAdamW), the moments, the step counters and the gradient scale: a fine-tune
    done from C comes back as a normal checkpoint.  image: bytes or a path."""
    import torch
    image = image if isinstance(image, (bytes, bytearray)) else open(image, "rb").read()
    st = training_state(image)
    p0 = next(model.parameters())
    model._ensure_arena(p0.device)
    eng, arena = model._engine, model._arena
    if st["arena"].numel() != arena.size:
        raise ValueError(f"load_training_state: the image's parameter arena holds {st['arena'].numel()} floats, this model's {arena.size}: "
                         "another configuration")
    compute = {v: k for k, v in COMPUTE_CODE.items()}.get(Plan.header(image)[H_COMPUTE])
    if compute != model.compute:
        raise ValueError(f"load_training_state: the image was exported in compute mode {compute}, this model computes in {model.compute}: "
                         "the gradient scale and the 16-bit copies belong to the mode")
    if bool(training_words(image)[TR_FLAGS] & 1) != (eng.scale_state is not None):
        raise ValueError("load_training_state: the image and this model disagree about a dynamic gradient scale (engine option grad_scale)")
    with torch.no_grad():
        arena.data.copy_(st["arena"])
        model.mark_weights_dirty()
        if eng.scale_state is not None and "scale_state" in st:
            eng.scale_state.copy_(st["scale_state"])
            eng.grad_overflow.copy_(st["nonfinite"])
            eng._scale_ready = True
        if optimizer is not None:
            if optimizer.model is not model:
                raise ValueError("load_training_state: the optimizer belongs to another model")
            optimizer.exp_avg.copy_(st["exp_avg"])
            optimizer.exp_avg_sq.copy_(st["exp_avg_sq"])
            optimizer._step_state.copy_(st["step_state"])
            optimizer._clip.copy_(st["clip"])
            optimizer.step_count = int(st["step_state"].sum())
    return model


# ----------------------------------------------------------------------------------------------------------------- runtime wrapper
def _load_library(kind):
    """the build of the library for operand format `kind`: through the package's loader when torch is already in the process (its HIP
    runtime has to be the one the library binds to), straight from the file otherwise"""
    if "torch" in sys.modules:
        from . import ops
        prev = ops.use(kind)
        try:
            return ops._raw()
        finally:
            ops.use(prev)
    import os
    path = os.environ.get("SCOT_LIB_" + kind.upper()) or _lib.LIB_PATHS[kind]
    if not os.path.exists(path):
        raise _lib.ScotLibraryError(f"{path} not found: build it with `python -m poseidon_amd.build`")
    return ctypes.CDLL(path)


def _is_tensor(x):
    return hasattr(x, "data_ptr")


def _addr(x, what):
    if x is None or isinstance(x, int):
        return x
    if not _is_tensor(x):
        raise TypeError(f"{what}: a tensor or a raw device address")
    import torch
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise TypeError(f"{what}: contiguous float32")
    return x.data_ptr()


class Plan:
    """A loaded plan.  `run` / `rollout` / `evaluate` / `vjp` / `rollout_vjp` / `loss` / `train_step` / `accumulate` take torch tensors (and return them) or raw
    device addresses (then `out` is required)."""

    def __init__(self, lib, handle):
        self._lib, self._h = lib, handle
        self.info = self.describe()

    @staticmethod
    def header(image):
        if len(image) < HEADER_WORDS * 8:
            raise _lib.ScotLibraryError("not a plan image: shorter than its header")
        h = struct.unpack(f"<{HEADER_WORDS}Q", image[:HEADER_WORDS * 8])
        if h[H_MAGIC] != MAGIC:
            raise _lib.ScotLibraryError("not a plan image: wrong magic")
        return h

    @classmethod
    def load(cls, source, lib=None, peer=None, stream=None, side_stream=None):
        """source: a path or the image's bytes.  lib: the build to load into (default: the one the image's operand format names).
        side_stream: a raw stream handle of the caller's for a two-stream plan, instead of the one the load picks."""
        image = source if isinstance(source, (bytes, bytearray)) else open(source, "rb").read()
        if lib is None:
            kind = {0: "bf16", 1: "f16"}.get(cls.header(image)[H_OPERAND])
            if kind is None:
                raise _lib.ScotLibraryError("plan image: unknown operand format")
            lib = _load_library(kind)
            if kind != "bf16" and peer is None and "torch" in sys.modules:
                peer = _load_library("bf16")
        bind(lib)
        if peer is not None:
            _lib.check(lib.scot_plan_peer_library(str(peer._name).encode()), "scot_plan_peer_library")
        handle = ctypes.c_void_p()
        rc = load_raw(lib, image, handle, stream)
        if rc != 0:
            raise _lib.ScotLibraryError(f"scot_plan_load refused the image: status {rc} ({_lib._ERR.get(rc, rc)})")
        plan = cls(lib, handle)
        if side_stream is not None:
            plan._call("scot_plan_set_side_stream", side_stream)
        return plan

    def describe_streams(self):
        """-> {streams, events, overlaps: the side stream was measured to run beside the load's stream, host_stream: it is the caller's}"""
        out = (ctypes.c_longlong * 4)()
        self._call("scot_plan_describe_streams", out)
        return dict(zip(DESCRIBE_STREAMS, [int(x) for x in out]))

    def issue_order(self, which, order):
        """test aid (scot_plan_issue_order): later calls issue call list `which` (0 forward, 2 / 3 / 4 the step lists) entry by entry in
        `order`, both streams synchronised at every stream switch; None restores the normal replay.  Legality is the caller's."""
        if order is None:
            return self._call("scot_plan_issue_order", int(which), None, 0)
        arr = (ctypes.c_int * max(1, len(order)))(*[int(x) for x in order])
        self._call("scot_plan_issue_order", int(which), ctypes.cast(arr, ctypes.c_void_p), len(order))

    def _call(self, name, *args):
        """the runtime's `name`(this plan, ...), its status checked"""
        _lib.check(getattr(self._lib, name)(self._h, *args), name)

    def describe(self):
        out = (ctypes.c_longlong * 16)()
        self._call("scot_plan_describe", out)
        return dict(zip(DESCRIBE, [int(x) for x in out]))

    def describe_resize(self):
        """-> (resized 0 / 1, the size the model runs at, the size of the host's tensors, scot_spectral_resize entries in all lists)"""
        out = (ctypes.c_longlong * 4)()
        self._call("scot_plan_describe_resize", out)
        return tuple(int(x) for x in out)

    def poison(self, byte=0xFF, stream=None):
        self._call("scot_plan_poison", int(byte), self._stream(stream, None))

    @staticmethod
    def _stream(stream, like):
        if stream is not None:
            return stream
        if like is not None and _is_tensor(like) and like.is_cuda:
            import torch
            return torch.cuda.current_stream(like.device).cuda_stream
        if "torch" in sys.modules:
            import torch
            if torch.cuda.is_available() and torch.cuda.is_initialized():
                return torch.cuda.current_stream().cuda_stream
        return None

    def _shape(self, channels="channels"):
        d = self.info
        return (d["batch"], d[channels], d["height"], d["width"])

    def _require(self, x, what, channels="channels"):
        """x is a tensor of this plan's shape"""
        if not _is_tensor(x) or tuple(x.shape) != self._shape(channels):
            raise ValueError(f"this plan takes {what} of shape {self._shape(channels)}")

    def _time(self, time, counted=True):
        """a time tensor as the runtime reads it: flat, float32, contiguous (counted: one value per sample)"""
        if time is None or not _is_tensor(time):
            return time
        import torch
        time = time.reshape(-1).to(torch.float32).contiguous()
        if counted and time.numel() != self.info["batch"]:
            raise ValueError("time: one value per sample")
        return time

    def _empty(self, like, channels="out_channels", steps=()):
        import torch
        return torch.empty(*steps, *self._shape(channels), dtype=torch.float32, device=like.device)

    def _gradient_pair(self, like):
        """buffers for (d_pixel_values, d_time): None for a gradient the plan was not exported with"""
        import torch
        a = self.describe_adjoint()
        return (self._empty(like, "channels") if a["d_pixel_values"] else None,
                torch.empty(self.info["batch"], dtype=torch.float32, device=like.device) if a["d_time"] else None)

    def run(self, pixel_values, time=None, pixel_mask=None, out=None, stream=None):
        if _is_tensor(pixel_values):
            self._require(pixel_values, "pixel_values")
            time = self._time(time)
            if out is None:
                out = self._empty(pixel_values)
        elif out is None:
            raise ValueError("raw addresses need `out`")
        self._call("scot_plan_run", _addr(pixel_values, "pixel_values"), _addr(time, "time"), _addr(pixel_mask, "pixel_mask"), _addr(out, "out"),
                   self._stream(stream, pixel_values))
        return out

    def rollout(self, pixel_values, time, steps, pixel_mask=None, out=None, stream=None):
        """-> [B, steps, Cout, H, W] for tensors (what harness.rollout(..., output_all_steps=True).output is); with raw addresses `out`
        receives the C layout [steps][B, Cout, H, W]."""
        tensors = _is_tensor(pixel_values)
        if tensors:
            time = self._time(time, counted=False)
            if out is None:
                out = self._empty(pixel_values, steps=(int(steps),))
        elif out is None:
            raise ValueError("raw addresses need `out`")
        self._call("scot_plan_rollout", _addr(pixel_values, "pixel_values"), _addr(time, "time"), _addr(pixel_mask, "pixel_mask"), _addr(out, "out"),
                   int(steps), self._stream(stream, pixel_values))
        return out.transpose(0, 1).contiguous() if tensors and _is_tensor(out) else out

    def evaluate(self, pixel_values, time, targets, steps=1, channel_slice_list=None, predictions=False, stream=None, pixel_mask=None,
                 mask_full=None):
        """-> error sums, float64 [steps, B, G, 4]: per step, sample and channel group `[channel_slice_list[g], channel_slice_list[g+1])`
        of the Cout output channels (None: one group) the sums Σ|p−t|, Σ|t|, Σ(p−t)², Σt² of the prediction against `targets`
        (scot_plan_evaluate; scOT.metrics' `*_from_sums` turn them into the reference's metrics).  steps == 1: one forward, as `run`,
        targets [B, Cout, H, W]; steps > 1: the chain of `rollout`, targets [B, steps, Cout, H, W] as `rollout` returns predictions.
        predictions=True: -> (sums, predictions [B, steps, Cout, H, W]); otherwise no prediction leaves the plan.
        With raw addresses `targets` is in the C layout [steps][B, Cout, H, W] and `predictions` is None or the address of a buffer in
        that layout; the sums still come back as a tensor (on the GPU where there is one).
        pixel_mask (scot_plan_evaluate_masked): bool or uint8 [B, Cout] (whole planes) or [B, Cout, H, W] / [B, 1, H, W] (elements), the
        same for every step — or a raw address with mask_full=.  After every forward the targets of that step are stored over the
        masked positions of the prediction, as the reference's `prediction[pixel_mask] = labels[pixel_mask]` does: the sums, the next
        step's input and the returned predictions carry them.  The channel slices have to tile all Cout channels then."""
        import torch
        steps = int(steps)
        if steps < 1:
            raise ValueError("steps >= 1")
        groups = 1 if channel_slice_list is None else len(channel_slice_list) - 1
        slices = None if channel_slice_list is None else ctypes.cast((ctypes.c_int * (groups + 1))(*[int(c) for c in channel_slice_list]),
                                                                     ctypes.c_void_p)
        tensors = _is_tensor(pixel_values)
        if tensors:
            self._require(pixel_values, "pixel_values")
            b, c, h, w = self._shape("out_channels")
            want = (b, c, h, w) if steps == 1 and _is_tensor(targets) and targets.dim() == 4 else (b, steps, c, h, w)
            if not _is_tensor(targets) or tuple(targets.shape) != want:
                raise ValueError(f"this plan's evaluation over {steps} step(s) takes targets of shape {want}")
            device = pixel_values.device
            targets = targets.to(device=device, dtype=torch.float32)
            targets = (targets if targets.dim() == 4 else targets.transpose(0, 1)).contiguous()
            time = self._time(time, counted=steps == 1)
            if _is_tensor(time):
                time = time.to(device)
            # (the converted copies are temporaries of torch's CURRENT stream: held until the next call, so that a call on an explicit
            # `stream=` never reads memory the allocator has handed on)
            self._held = (targets, time)
            out = self._empty(pixel_values, steps=(steps,)) if predictions else None
        else:
            if isinstance(predictions, bool) and predictions:
                raise ValueError("raw addresses need `predictions` to be an address (or None)")
            device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
            out = predictions or None
        sums = torch.empty(steps, self.info["batch"], groups, 4, dtype=torch.float64, device=device)
        if pixel_mask is not None:
            mask, full = self._mask(pixel_mask, pixel_values if tensors else None, mask_full)
            self._call("scot_plan_evaluate_masked", _addr(pixel_values, "pixel_values"), _addr(time, "time"), _addr(targets, "targets"), mask,
                       int(full), steps, slices, groups, sums.data_ptr(), _addr(out, "predictions"), self._stream(stream, pixel_values))
        else:
            self._call("scot_plan_evaluate", _addr(pixel_values, "pixel_values"), _addr(time, "time"), _addr(targets, "targets"), steps, slices,
                       groups, sums.data_ptr(), _addr(out, "predictions"), self._stream(stream, pixel_values))
        if out is None:
            return sums
        return sums, (out.transpose(0, 1).contiguous() if tensors and _is_tensor(out) else out)

    def describe_adjoint(self):
        out = (ctypes.c_longlong * 8)()
        self._call("scot_plan_describe_adjoint", out)
        return dict(zip(DESCRIBE_ADJOINT, [int(x) for x in out]))

    def vjp(self, d_prediction, grad_scale=0, out=None, stream=None):
        """-> (d_pixel_values, d_time) = J^T d_prediction at the inputs of the last `run` (None for a gradient the plan was not exported
        with).  out: (buffer or None, buffer or None) to receive them; required with raw addresses.  grad_scale: scot_plan.h."""
        if _is_tensor(d_prediction):
            self._require(d_prediction, "a cotangent", "out_channels")
            if out is None:
                out = self._gradient_pair(d_prediction)
        elif out is None:
            raise ValueError("raw addresses need `out`")
        self._call("scot_plan_vjp", _addr(d_prediction, "d_prediction"), _addr(out[0], "d_pixel_values"), _addr(out[1], "d_time"), float(grad_scale),
                   self._stream(stream, d_prediction))
        return out

    def rollout_vjp(self, pixel_values, time, predictions, d_predictions, grad_scale=0, out=None, stream=None, steps=None):
        """-> (d_pixel_values, d_time): the gradient of sum_k <d_predictions[:, k], predictions[:, k]> through the rollout with no detach
        between the steps (scot_plan_rollout_vjp: recomputes every step, `steps` forwards + `steps` backwards).  Tensors come in the
        layout `rollout` returns, [B, steps, Cout, H, W], `predictions` being what `rollout(pixel_values, time, steps)` gave.  None for
        a gradient the plan was not exported with.  out: (buffer or None, buffer or None) to receive them.  With raw addresses
        `predictions` / `d_predictions` are in the C layout [steps][B, Cout, H, W], and `out` and `steps=` are required."""
        if _is_tensor(pixel_values):
            import torch
            if not (_is_tensor(predictions) and _is_tensor(d_predictions)) or predictions.dim() != 5 or predictions.shape != d_predictions.shape:
                raise ValueError("predictions and d_predictions: tensors of one shape [B, steps, Cout, H, W]")
            if tuple(predictions.shape[:1] + predictions.shape[2:]) != self._shape("out_channels"):
                b, c, h, w = self._shape("out_channels")
                raise ValueError(f"this plan's rollout is of shape {(b, 'steps', c, h, w)}")
            if steps is not None and int(steps) != predictions.shape[1]:
                raise ValueError(f"steps={steps}, predictions hold {predictions.shape[1]} steps")
            steps = predictions.shape[1]
            predictions = predictions.to(torch.float32).transpose(0, 1).contiguous()
            d_predictions = d_predictions.to(torch.float32).transpose(0, 1).contiguous()
            time = self._time(time, counted=False)
            if out is None:
                out = self._gradient_pair(pixel_values)
        elif out is None or steps is None:
            raise ValueError("raw addresses need `out` and `steps`")
        self._call("scot_plan_rollout_vjp", _addr(pixel_values, "pixel_values"), _addr(time, "time"), _addr(predictions, "predictions"),
                   _addr(d_predictions, "d_predictions"), int(steps), _addr(out[0], "d_pixel_values"), _addr(out[1], "d_time"), float(grad_scale),
                   self._stream(stream, pixel_values))
        return out

    def grad_status(self, stream=None):
        """-> (non-finite values the un-scale passes have counted since load, the last vjp's scale as a power-of-two exponent)"""
        out = (ctypes.c_longlong * 2)()
        self._call("scot_plan_grad_status", out, self._stream(stream, None))
        return int(out[0]), int(out[1])

    def describe_training(self):
        out = (ctypes.c_longlong * 8)()
        self._call("scot_plan_describe_training", out)
        return dict(zip(DESCRIBE_TRAINING, [int(x) for x in out]))

    def _mask(self, pixel_mask, like=None, full=None):
        """a pixel_mask as the runtime reads it -> (address or None, whether it is an element mask): a bool / uint8 tensor [B, Cout]
        (whole planes) or [B, Cout, H, W] / [B, 1, H, W] (elements) becomes contiguous bytes on `like`'s device, held until the next
        call; a raw address passes through with `full`"""
        if pixel_mask is None or isinstance(pixel_mask, int):
            return pixel_mask, bool(full)
        if not _is_tensor(pixel_mask):
            raise TypeError("pixel_mask: a tensor or a raw device address")
        m, full = _mask_bytes(pixel_mask, *self._shape("out_channels"))
        if like is not None and _is_tensor(like):
            m = m.to(like.device)
        self._held_mask = m
        return m.data_ptr(), full

    def _batch(self, pixel_values, time, labels, pixel_mask=None):
        if _is_tensor(pixel_values):
            self._require(pixel_values, "pixel_values")
            self._require(labels, "labels", "out_channels")
            time = self._time(time)
        mask, full = self._mask(pixel_mask, pixel_values)
        if mask is not None and _is_tensor(pixel_mask) and self.describe_training()["mask"] not in (0, 2 if full else 1):
            raise ValueError(f"this plan was exported with {'a channel' if full else 'an element'} mask")
        return _addr(pixel_values, "pixel_values"), _addr(time, "time"), _addr(labels, "labels"), mask

    def loss(self, pixel_values, time, labels, out=None, stream=None, pixel_mask=None):
        """-> (loss [1], prediction) of the step's forward at the current weights (scot_plan_loss); changes no state.  out: (loss buffer,
        prediction buffer or None), required with raw addresses.  pixel_mask: the batch's mask on a masked plan (scot_plan_loss_masked;
        bool or uint8 [B, Cout] / [B, Cout, H, W] / [B, 1, H, W], or the address of the plan's mask bytes): the prediction then holds the
        labels at the masked positions."""
        pv, t, lab, mask = self._batch(pixel_values, time, labels, pixel_mask)
        if out is None:
            if not _is_tensor(pixel_values):
                raise ValueError("raw addresses need `out`")
            import torch
            out = (torch.empty(1, dtype=torch.float32, device=pixel_values.device), self._empty(pixel_values))
        if pixel_mask is None:
            self._call("scot_plan_loss", pv, t, lab, _addr(out[0], "loss"), _addr(out[1], "prediction"), self._stream(stream, pixel_values))
        else:
            self._call("scot_plan_loss_masked", pv, t, lab, mask, _addr(out[0], "loss"), _addr(out[1], "prediction"),
                       self._stream(stream, pixel_values))
        return out

    def train_step(self, pixel_values, time, labels, lr, out=None, stream=None, pixel_mask=None):
        """one optimizer step on the batch (scot_plan_train_step) -> the loss before the update ([1], on the device).  lr: one float
        per parameter group, in the export's group order (a single float: the same for all).  out: a loss buffer of the caller's.
        pixel_mask: the batch's mask on a masked plan, as for `loss` (scot_plan_train_step_masked)."""
        rates = self._rates(lr)
        pv, t, lab, mask = self._batch(pixel_values, time, labels, pixel_mask)
        if out is None and _is_tensor(pixel_values):
            import torch
            out = torch.empty(1, dtype=torch.float32, device=pixel_values.device)
        if pixel_mask is None:
            self._call("scot_plan_train_step", pv, t, lab, ctypes.cast(rates, ctypes.c_void_p), _addr(out, "loss"),
                       self._stream(stream, pixel_values))
        else:
            self._call("scot_plan_train_step_masked", pv, t, lab, mask, ctypes.cast(rates, ctypes.c_void_p), _addr(out, "loss"),
                       self._stream(stream, pixel_values))
        return out

    def _rates(self, lr):
        """lr -> the host array a step or an apply reads: one float per parameter group (a single float: the same for all)"""
        groups = self.describe_training()["groups"]
        lr = [float(lr)] * groups if isinstance(lr, (int, float)) else [float(x) for x in lr]
        if len(lr) != groups:
            raise ValueError(f"this plan has {groups} parameter groups, lr has {len(lr)} values")
        return (ctypes.c_float * max(1, groups))(*lr)

    def accumulate(self, pixel_values, time, labels, weight, first, out=None, stream=None, pixel_mask=None):
        """one micro-batch into the plan's gradient accumulator (scot_plan_accumulate): forward and backward as `train_step` runs them,
        then A = weight * g (first) or A += weight * g; no state changes -> the micro-batch's own unweighted loss ([1], on the device).
        `apply` ends the accumulation with the update.  out: a loss buffer of the caller's.  pixel_mask: as for `train_step`."""
        pv, t, lab, mask = self._batch(pixel_values, time, labels, pixel_mask)
        if out is None and _is_tensor(pixel_values):
            import torch
            out = torch.empty(1, dtype=torch.float32, device=pixel_values.device)
        self._call("scot_plan_accumulate", pv, t, lab, mask, float(weight), int(bool(first)), _addr(out, "loss"),
                   self._stream(stream, pixel_values))
        return out

    def apply(self, lr, stream=None):
        """the optimizer update from the accumulated gradient (scot_plan_apply); lr as for `train_step`.  Clipping, the skip of a
        non-finite norm, the counters and the fp16 scale are the device's decisions on the accumulated gradient (`train_status`)."""
        rates = self._rates(lr)
        self._call("scot_plan_apply", ctypes.cast(rates, ctypes.c_void_p), self._stream(stream, None))

    def gradients(self, which):
        """-> a float32 [arena_floats] VIEW (no copy) of the plan's own memory: which = 0 the gradient arena the update reads, 1 the
        accumulator (scot_plan_gradients).  Valid until the plan is freed; read and write it in the plan's stream order — an
        all-reduce of the accumulator goes between the last `accumulate` and `apply`.  On the GPU a CUDA tensor on the current device,
        on the CPU emulation a tensor over the host buffer."""
        import torch
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._call("scot_plan_gradients", int(which), ctypes.byref(p), ctypes.byref(n))
        if hasattr(self._lib, "scot_plan_emu_issued"):      # the emulation: the buffer is host memory
            return torch.frombuffer((ctypes.c_float * n.value).from_address(p.value), dtype=torch.float32)

        class _Device:      # (the owner torch keeps alive with the view is this object, not the plan)
            __cuda_array_interface__ = {"shape": (n.value,), "typestr": "<f4", "data": (p.value, False), "version": 2, "strides": None}
        return torch.as_tensor(_Device(), device="cuda")

    def accumulation_status(self):
        """-> {micro_batches: in the open accumulation (0: none is open), bytes: of the accumulator (0 before the first accumulate)}"""
        out = (ctypes.c_longlong * 2)()
        self._call("scot_plan_accumulation_status", out)
        return {"micro_batches": int(out[0]), "bytes": int(out[1])}

    def train_status(self, stream=None):
        """-> {applied, skipped, grad_scale, grad_norm, clip_coef, nonfinite} (scot_plan_train_status: waits for the stream)"""
        out = (ctypes.c_double * 6)()
        self._call("scot_plan_train_status", out, self._stream(stream, None))
        vals = [float(x) for x in out]
        return dict(zip(TRAIN_STATUS, [int(vals[0]), int(vals[1]), vals[2], vals[3], vals[4], int(vals[5])]))

    def snapshot(self, image, stream=None):
        """-> the bytes of `image` (THE image this plan was loaded from) with every state buffer's current value written back
        (scot_plan_snapshot): a valid training image that resumes exactly"""
        buf, n = _aligned_copy(image)
        self._call("scot_plan_snapshot", ctypes.cast(buf, ctypes.c_void_p), n, self._stream(stream, None))
        return bytes(memoryview(buf).cast("B")[:n])      # (not ctypes.string_at: its size is a C int, an image can pass 2 GiB)

    def free(self):
        if self._h is not None and self._h.value:
            self._lib.scot_plan_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _aligned_copy(image):
    """-> (a copy of the image's bytes in 8-byte aligned memory, their number)"""
    n = len(image)
    buf = (ctypes.c_uint64 * ((n + 7) // 8 or 1))()
    ctypes.memmove(buf, bytes(image), n)
    return buf, n


def load_raw(lib, image, handle, stream=None):
    """scot_plan_load on `image` (bytes) -> status; `handle` (c_void_p) receives the plan.  The image is copied to 8-byte aligned memory."""
    bind(lib)
    buf, n = _aligned_copy(image)
    return lib.scot_plan_load(ctypes.cast(buf, ctypes.c_void_p), n, ctypes.byref(handle), stream)
