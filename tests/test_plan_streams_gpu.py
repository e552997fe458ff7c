"""Two-stream plans on the MI355X: `export_plan(..., streams=2)` writes the engine's own two-stream program (image formats 5 and 6),
the plan runtime gives it a side stream and events and replays it — through ctypes here, and from examples/plan_train_host.c, unchanged,
as a child process.

Inference is compared bit for bit with `model(...)` and with the one-stream plan, in the recorded order and in legal orders derived
from the image's own event edges (tests/tape_schedule.py; `scot_plan_issue_order` issues them with both streams synchronised at every
stream switch).  Training follows the rule of tests/test_plan_train_gpu.py: parameter gradients are not bit-reproducible on the GPU, so
the trained weights are held to 4 * floor + 2e-5 of a Python run, `floor` being the distance of two Python runs, and that bound must
itself be below 1e-4.  The caller's buffers lie in NaN guard bands (tests/kernel_checks.py)."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_checks as kc  # noqa: E402
import tape_schedule as ts  # noqa: E402
from conftest import ROOT  # noqa: E402
from poseidon_amd import build as scot_build, lib as scot_lib, plan as plan_mod  # noqa: E402
from poseidon_amd.config import ScOTConfig  # noqa: E402
from poseidon_amd.geometry import param_shapes  # noqa: E402
from poseidon_amd.plan import Plan  # noqa: E402
from poseidon_amd.synth import synth_inputs, synth_state_dict  # noqa: E402
from scOT.model import ScOT  # noqa: E402
from test_model_gpu import DEV, _preset_model  # noqa: E402

H = plan_mod
STEPS, LR = 6, 5e-5
OPT = dict(lr=LR, weight_decay=0.01, max_grad_norm=5.0)
SMALL = dict(image_size=32, patch_size=4, num_channels=4, num_out_channels=4, embed_dim=16, depths=[2, 2], num_heads=[1, 2],
             skip_connections=[1, 0], window_size=4, mlp_ratio=4.0, p=1, channel_slice_list_normalized_loss=[0, 1, 3, 4],
             drop_path_rate=0.0, use_conditioning=True)
# 96 channels wide, 64 x 64: the fused layer tails and a skip with a ConvNeXt block
CFG96 = dict(image_size=64, patch_size=4, num_channels=4, num_out_channels=4, embed_dim=96, depths=[2, 1], num_heads=[3, 6],
             skip_connections=[1, 0], window_size=16, mlp_ratio=4.0, qkv_bias=True, drop_path_rate=0.0, hidden_act="gelu", p=1,
             channel_slice_list_normalized_loss=[0, 1, 3, 4], residual_model="convnext", use_conditioning=True, learn_residual=False)
INFERENCE = {"small": (SMALL, "fp32", 2, None), "c96": (CFG96, "fp16", 1, {"fused_min_rows": 0})}
LISTS = {"forward": 0, 0: 2, 1: 3, 2: 4}      # a call list -> SCOT_PLAN_CALLS_*


# ------------------------------------------------------------------------------------------------------- an image's lists as tapes
def image_entries(image, which):
    """one call list of an image ("forward", or step list 0 / 1 / 2) -> tape_schedule entries over stream and event INDICES"""
    h = Plan.header(image)
    names = [image[h[H.H_NAMES_OFF] + i * H.NAME_BYTES:][:H.NAME_BYTES].split(b"\0")[0].decode() for i in range(h[H.H_NNAMES])]
    n, off = (h[H.H_NENTRIES], h[H.H_ENTRIES_OFF]) if which == "forward" else plan_mod.training_words(image)[H.TR_FWD + 3 * which:][:2]
    out = []
    for i in range(n):
        name, _, ni, nf = struct.unpack_from("<4Q", image, off)
        pairs = struct.unpack_from(f"<{2 * ni}Q", image, off + 32)
        stream = [pairs[2 * k + 1] for k in range(ni) if pairs[2 * k] & 0xFF == H.ARG_STREAM]
        event = [pairs[2 * k + 1] for k in range(ni) if pairs[2 * k] & 0xFF == H.ARG_EVENT]
        assert len(stream) == 1
        kind = {H.RECORD: ts.RECORD, H.WAIT: ts.WAIT}.get(names[name], ts.LAUNCH)
        out.append(ts.Entry(i, kind, stream[0], event[0] if event else None))
        off += 8 * (4 + 2 * ni + nf)
    return out


def orders(entries, seeds=(21, 22, 23)):
    yield "late", ts.late(entries, 1)
    yield "early", ts.early(entries, 1)
    for seed in seeds:
        yield f"random {seed}", ts.random(entries, seed)


def install(plan, image, which, order):
    if order is not None:
        ts.check(order, image_entries(image, which))
    plan.issue_order(LISTS[which], order)


# ------------------------------------------------------------------------------------------------------- inference
_inference = {}


def inference_export(name):
    """one model and its two exports for the whole module -> (model, pixel_values, time, two-stream image, one-stream image)"""
    if name not in _inference:
        kw, compute, batch, options = INFERENCE[name]
        cfg = ScOTConfig(**kw)
        model = ScOT(cfg, compute=compute, engine_options=options)
        model.load_state_dict(synth_state_dict(param_shapes(cfg), "trained"))
        model = model.to(DEV).eval()
        pv, t, _ = synth_inputs(batch, cfg.num_channels, cfg.num_out_channels, cfg.image_size, "smooth")
        pv, t = pv.to(DEV), t.to(DEV)
        _inference[name] = (model, pv, t, model.export_plan(pv, time=t, streams=2), model.export_plan(pv, time=t))
    return _inference[name]


def own(model, pv, t):
    with torch.no_grad():
        return model(pixel_values=pv, time=t).output.clone()


@pytest.mark.parametrize("name", ["small", "c96"])
def test_inference_is_bit_identical_in_every_legal_order(name):
    model, pv, t, image, plain = inference_export(name)
    assert Plan.header(image)[H.H_FORMAT] == 5 and Plan.header(plain)[H.H_FORMAT] == 1
    entries = image_entries(image, "forward")
    assert {e.stream for e in entries if e.kind == ts.LAUNCH} == {0, 1}
    if name == "c96":
        names = {image[Plan.header(image)[H.H_NAMES_OFF] + i * H.NAME_BYTES:][:H.NAME_BYTES].split(b"\0")[0] for i in range(Plan.header(image)[H.H_NNAMES])}
        assert b"scot_block_tail_fwd" in names
    plan, one = Plan.load(image), Plan.load(plain)
    d = plan.describe_streams()
    assert d["streams"] == 2 and d["events"] >= 1 and d["overlaps"] in (0, 1) and d["host_stream"] == 0
    assert one.describe_streams() == dict(streams=1, events=0, overlaps=0, host_stream=0)
    B, Cout = pv.shape[0], model.config.num_out_channels
    pv2, t2 = pv.flip(0).flip(3) * 0.5 + 0.05, t * 0.37 + 0.05
    ref, ref2 = own(model, pv, t), own(model, pv2, t2)
    assert torch.isfinite(ref).all() and not torch.equal(ref, ref2)
    assert torch.equal(one.run(pv, t), ref)

    def guarded_run(x, tt, want, label):
        gx, g_in = kc.guarded(tuple(x.shape), torch.float32, DEV, src=x, name="pixel_values")
        gt, g_t = kc.guarded((B,), torch.float32, DEV, src=tt, name="time")
        out, g_out = kc.guarded((B, Cout, *x.shape[2:]), torch.float32, DEV, name="prediction")
        plan.run(gx, gt, out=out)
        torch.cuda.synchronize()
        assert torch.equal(out, want), label
        kc.check_all([g_in, g_t, g_out])
        assert torch.equal(gx, x) and torch.equal(gt, tt)
    guarded_run(pv, t, ref, "as recorded")
    plan.poison(0xFF)
    guarded_run(pv2, t2, ref2, "poisoned")
    plan.poison(0xFF)
    guarded_run(pv, t, ref, "poisoned")
    for label, order in orders(entries):
        install(plan, image, "forward", None)
        plan.run(pv2, t2)      # (each compared run follows a run on other inputs)
        install(plan, image, "forward", order)
        guarded_run(pv, t, ref, label)
    install(plan, image, "forward", None)
    # three steps of the rollout
    a, b = plan.rollout(pv, t, 3), one.rollout(pv, t, 3)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b)
    plan.free(), one.free()


# ------------------------------------------------------------------------------------------------------- training
def build_model():
    """Poseidon-T 128 x 128 fp16, batch 4 (tests/test_plan_train_gpu.py) -> (model in training mode, its FusedAdamW, batch)"""
    from scOT.trainer import FusedAdamW
    _, _, model = _preset_model("T", 128, 4, "fp16", engine_options={"fused_min_rows": 0})
    batch = synth_inputs(4, 4, 4, 128, "smooth")
    model.train()
    return model, FusedAdamW(model, **OPT), tuple(x.to(DEV) for x in batch)


_training = {}


def training_export():
    if not _training:
        model, opt, batch = build_model()
        _training["image"] = (model.export_plan(batch[0], time=batch[1], labels=batch[2], train=opt, streams=2), batch)
    return _training["image"]


def with_scale(image, exponent):
    """the image with the gradient scale in its stored state set to 2^exponent"""
    h, tr = Plan.header(image), plan_mod.training_words(image)
    buf, off, n = tr[H.TR_SCALE_STATE:H.TR_SCALE_STATE + 3]
    assert n == 16
    data_off = struct.unpack_from("<Q", image, h[H.H_BUFFERS_OFF] + 32 * buf + 16)[0]
    b = bytearray(image)
    struct.pack_into("<4f", b, h[H.H_DATA_OFF] + data_off + off, 2.0 ** exponent, 2.0 ** -exponent, 0.0, 0.0)
    return bytes(b)


def test_loss_skipped_step_and_snapshot():
    image, batch = training_export()
    assert Plan.header(image)[H.H_FORMAT] == 6
    bwd = image_entries(image, 1)
    assert {e.stream for e in bwd if e.kind == ts.LAUNCH} == {0, 1}
    model, opt, _ = build_model()
    plan = Plan.load(image)
    assert plan.describe()["format"] == 6 and plan.describe_training()["has_training"] == 1 and plan.describe_streams()["streams"] == 2
    out = model(batch[0], time=batch[1], labels=batch[2])
    views, guards = [], []
    for x, what in zip(batch, ("pixel_values", "time", "labels")):
        v, g = kc.guarded(tuple(x.shape), torch.float32, DEV, src=x, name=what)
        views.append(v)
        guards.append(g)
    loss, g_loss = kc.guarded((1,), torch.float32, DEV, name="loss")
    pred, g_pred = kc.guarded(tuple(batch[2].shape), torch.float32, DEV, name="prediction")
    plan.poison(0xFF)
    plan.loss(*views, out=(loss, pred))
    torch.cuda.synchronize()
    assert torch.equal(pred, out.output.detach())
    ref = float(out.loss.detach())
    assert abs(float(loss) - ref) <= 1e-5 * abs(ref)      # (the loss sums commit in any order)
    assert plan.snapshot(image) == image
    plan.poison(0xFF)
    plan.train_step(*views, LR, out=loss)
    st = plan.train_status()
    assert (st["applied"], st["skipped"], st["nonfinite"]) == (1, 0, 0) and np.isfinite(st["grad_norm"]) and 0.0 < st["clip_coef"] <= 1.0
    kc.check_all(guards + [g_loss, g_pred])
    assert all(torch.equal(a, b) for a, b in zip(views, batch))
    # snapshot -> load -> run equals the original plan's run
    snap = plan.snapshot(image)
    after = plan_mod.training_state(snap)
    assert torch.isfinite(after["arena"]).all() and not torch.equal(after["arena"], plan_mod.training_state(image)["arena"])
    again = Plan.load(snap)
    a, b = plan.run(batch[0], batch[1]), again.run(batch[0], batch[1])
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b) and not torch.equal(a, out.output.detach())
    plan.free(), again.free()
    # a skipped step: gradient scale 2^30 in the stored state, the backward overflows binary16, nothing but the scale changes
    hot = with_scale(image, 30)
    plan = Plan.load(hot)
    plan.train_step(*batch, LR)
    st = plan.train_status()
    assert (st["applied"], st["skipped"]) == (0, 1) and st["nonfinite"] > 0 and st["grad_scale"] == 2.0 ** 29
    a, b = plan_mod.training_state(hot), plan_mod.training_state(plan.snapshot(hot))
    for k in ("arena", "exp_avg", "exp_avg_sq", "shadow", "shadow_t"):
        assert torch.equal(a[k], b[k]), k
    assert b["step_state"].tolist() == [0, 1]
    plan.free()


def python_run(batch):
    model, opt, _ = build_model()
    losses = []
    for _ in range(STEPS):
        opt.zero_grad(overlap=True)
        out = model(batch[0], time=batch[1], labels=batch[2])
        out.loss.backward()
        opt.step()
        losses.append(float(out.loss.detach()))
    torch.cuda.synchronize()
    assert int(model._engine.grad_overflow) == 0 and opt.skipped_steps() == 0
    return np.array(losses), model.flat_parameters().detach().cpu().clone()


def plan_run(image, batch, ordered=()):
    """six steps of the plan -> (losses, final parameters, status); ordered: {step: label of the order its three lists are issued in}"""
    plan = Plan.load(image)
    generated = {which: dict(orders(image_entries(image, which), seeds=())) for which in (0, 1, 2)} if ordered else {}
    losses = torch.empty(STEPS, device=DEV)
    for k in range(STEPS):
        for which in (0, 1, 2) if ordered else ():
            install(plan, image, which, generated[which][ordered[k]] if k in ordered else None)
        plan.train_step(*batch, LR, out=losses[k:k + 1])
    st = plan.train_status()
    arena = plan_mod.training_state(plan.snapshot(image))["arena"]
    plan.free()
    return losses.cpu().numpy().astype(np.float64), arena, st


def test_six_steps_track_the_python_loop(tmp_path):
    """Six steps of the Python loop (twice: its run-to-run floor), of the two-stream plan as recorded, of the plan with one step issued in
    `late` and one in `early` order, and of examples/plan_train_host.c, unchanged, on the format-6 image; figures before assertions."""
    image, batch = training_export()
    (la, pa), (lb, pb) = python_run(batch), python_run(batch)
    floor = float((pa - pb).norm() / pa.norm())
    bound = 4.0 * floor + 2e-5
    results = {"as recorded": plan_run(image, batch), "late / early": plan_run(image, batch, {1: "late", 3: "early"})}
    figures = {}
    for label, (lp, pp, st) in results.items():
        figures[label] = (float((pp - pa).norm() / pa.norm()), float(np.max(np.abs(lp - la) / la)))
        print(f"\n[two-stream training plan, Poseidon-T fp16, {STEPS} steps, {label}] floor {floor:.2e}, bound {bound:.2e}, plan vs Python "
              f"{figures[label][0]:.2e}; loss {la[0]:.4f} -> {la[-1]:.4f} / {lp[-1]:.4f}, max rel gap {figures[label][1]:.2e}")
    # from C: a fresh child process under its own time limit, the host program as it is
    exe, path, snap_path = str(tmp_path / "plan_train_host"), str(tmp_path / "train.plan"), str(tmp_path / "snapshot.plan")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(scot_build.HIPCC)))
    cc = subprocess.run([scot_build.HIPCC, "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                         os.path.join(ROOT, "examples", "plan_train_host.c"), "-o", exe, "-ldl"], capture_output=True, text=True, timeout=120)
    assert cc.returncode == 0, cc.stderr[-3000:]
    with open(path, "wb") as f:
        f.write(image)
    (tmp_path / "batches.bin").write_bytes(b"".join(x.cpu().numpy().tobytes() for x in batch) * STEPS)
    groups = plan_mod.training_words(image)[H.TR_GROUPS]
    (tmp_path / "lr.bin").write_bytes(np.full(STEPS * groups, LR, dtype=np.float32).tobytes())
    run = subprocess.run(["timeout", "-k", "10", "120", exe, scot_lib.LIB_PATHS["f16"], path, str(tmp_path / "batches.bin"),
                          str(tmp_path / "lr.bin"), snap_path], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-1000:], run.stderr[-3000:])
    rows = re.findall(r"step (\d+) loss (\S+) applied (\d+) skipped (\d+)", run.stdout)
    assert [int(r[0]) for r in rows] == list(range(STEPS)), run.stdout[-2000:]
    lc = np.array([float(r[1]) for r in rows])
    pc = plan_mod.training_state(open(snap_path, "rb").read())["arena"]
    dist_c, gap_c = float((pc - pa).norm() / pa.norm()), float(np.max(np.abs(lc - la) / la))
    print(f"[examples/plan_train_host.c on the format-6 image] C vs Python {dist_c:.2e}, max rel loss gap {gap_c:.2e}")
    assert bound < 1e-4, f"inconclusive: the Python loop's own run-to-run distance {floor:.2e} gives a bound of {bound:.2e}"
    for label, (dist, gap) in figures.items():
        assert dist <= bound and gap <= 1e-3, label
        st = results[label][2]
        assert (st["applied"], st["skipped"], st["nonfinite"]) == (STEPS, 0, 0), label
    assert dist_c <= bound and gap_c <= 1e-3 and float(np.max(np.abs(lb - la) / la)) <= 1e-3
    assert (int(rows[-1][2]), int(rows[-1][3])) == (STEPS, 0)


# ------------------------------------------------------------------------------------------------------- the stream probe
def test_stream_probe_agrees_with_the_plan():
    """scot_stream_overlaps answers 0 for a stream against itself and 0 or 1 for a pair; for the pair a plan was given, its answer is what
    the plan describes.  Whether two streams overlap is the machine's business: no time is asserted."""
    _, _, _, image, _ = inference_export("small")
    lib = Plan.load(image)
    cur = torch.cuda.current_stream().cuda_stream
    side = torch.cuda.Stream()
    flag = ctypes.c_int(-1)
    assert lib._lib.scot_stream_overlaps(side.cuda_stream, side.cuda_stream, ctypes.byref(flag)) == 0 and flag.value == 0
    lib.free()
    plan = Plan.load(image, side_stream=side.cuda_stream)
    d = plan.describe_streams()
    assert d["streams"] == 2 and d["host_stream"] == 1 and d["overlaps"] in (0, 1)
    flag = ctypes.c_int(-1)
    assert plan._lib.scot_stream_overlaps(cur, side.cuda_stream, ctypes.byref(flag)) == 0 and flag.value in (0, 1)
    print(f"\n[scot_stream_overlaps] the current stream and a fresh torch stream: {flag.value}; the plan describes {d['overlaps']}")
    assert flag.value == d["overlaps"]
    model, pv, t, _, _ = inference_export("small")
    assert torch.equal(plan.run(pv, t), own(model, pv, t))      # (the host's stream is the one that is used)
    torch.cuda.synchronize()
    plan.free()
