"""scot_plan_evaluate on the CPU emulation: a forward or a whole rollout of an exported plan that leaves only error sums behind
(csrc/plan.hip, csrc/error_sums.hip), on every image format, with the caller's buffers in NaN guard bands and the plan's scratch
poisoned; `Plan.evaluate`; `Trainer.evaluate_on_device`.  Every comparison with scot_plan_rollout / scot_plan_run / the stand-alone
kernel is bit for bit; "issues nothing" is read from `scot_plan_emu_issued()`."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import error_sums_cases as E  # noqa: E402
import plan_eval_cases as PE  # noqa: E402
from plan_support import BOTH, CFG_ROLL, ROOT, SMALL, emu, issued, synth_model  # noqa: E402,F401
from poseidon_amd import plan as plan_mod  # noqa: E402
from poseidon_amd.config import ScOTConfig  # noqa: E402
from poseidon_amd.plan import Plan  # noqa: E402
from poseidon_amd.synth import synth_inputs  # noqa: E402

_cache = {}


def inputs(kw, batch=2):
    pv, t, y = synth_inputs(batch, kw["num_channels"], kw["num_out_channels"], kw["image_size"], "smooth")
    return pv.contiguous(), t.contiguous(), y.contiguous()


def exported(name, **kw):
    """one export per (configuration, request) for the whole module -> the image's bytes"""
    key = (name, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _cache:
        cfg = dict(roll=CFG_ROLL, small=SMALL, untimed=dict(SMALL, use_conditioning=False),
                   widening=dict(SMALL, num_channels=3, num_out_channels=4))[name]
        model = synth_model(ScOTConfig(**cfg), "fp32")
        for p in model.parameters():
            p.requires_grad_(False)
        pv, t, _ = inputs(cfg)
        _cache[key] = model.export_plan(pv, time=t if cfg["use_conditioning"] else None, **kw)
    return _cache[key]


def context(emu):
    return E.Ctx(plan_mod.bind(emu), torch.device("cpu"))


@pytest.mark.parametrize("slices", [[0, 1, 3], None], ids=["slices_0_1_3", "one_group"])
def test_rollout_leaves_only_sums(emu, slices):
    """CFG_ROLL (5 -> 3 channels, 16 x 16, batch 2, fp32), 3 steps"""
    ctx = context(emu)
    pv, t, _ = inputs(CFG_ROLL)
    plan = Plan.load(exported("roll"))
    before = plan.describe()["device_bytes"]
    sums, targets = PE.check_evaluate(plan, ctx, pv, t, 3, slices)
    assert plan.describe()["device_bytes"] > before          # the kernel's workspace, held from the first evaluate call on
    held = plan.describe()["device_bytes"]
    # the Python surface: tensors in rollout's layout
    got = plan.evaluate(pv, t, targets.transpose(0, 1), steps=3, channel_slice_list=slices)
    assert got.dtype == torch.float64 and PE.same_bits(got, sums)
    got, preds = plan.evaluate(pv, t, targets.transpose(0, 1), steps=3, channel_slice_list=slices, predictions=True)
    assert PE.same_bits(got, sums) and PE.same_bits(preds, plan.rollout(pv, t, 3)) and preds.shape == (2, 3, 3, 16, 16)
    raw = plan.evaluate(pv.data_ptr(), t.data_ptr(), targets.data_ptr(), steps=3, channel_slice_list=slices)
    assert PE.same_bits(raw, sums) and plan.describe()["device_bytes"] == held
    with pytest.raises(ValueError):
        plan.evaluate(pv, t, targets, steps=3)               # the C layout is not the tensor layout
    plan.free()


def test_single_step_is_the_forward_of_run(emu):
    """SMALL (4 -> 4 channels, 32 x 32), steps == 1, with and without a time input"""
    ctx = context(emu)
    pv, t, _ = inputs(SMALL)
    plan = Plan.load(exported("small"))
    sums, targets = PE.check_evaluate(plan, ctx, pv, t, 1, [0, 1, 3, 4])
    got = plan.evaluate(pv, t, targets[0], channel_slice_list=[0, 1, 3, 4])
    assert got.shape == (1, 2, 3, 4) and PE.same_bits(got, sums)
    plan.free()
    plan = Plan.load(exported("untimed"))
    assert plan.info["has_time"] == 0
    PE.check_evaluate(plan, ctx, pv, None, 1, None)
    plan.free()


def test_two_stream_plan_gives_the_one_stream_sums(emu):
    ctx = context(emu)
    pv, t, _ = inputs(CFG_ROLL)
    one, two = Plan.load(exported("roll")), Plan.load(exported("roll", streams=2))
    assert two.describe()["format"] == 5 and two.describe_streams()["streams"] == 2
    a, targets = PE.check_evaluate(one, ctx, pv, t, 3, [0, 1, 3])
    b, _ = PE.check_evaluate(two, ctx, pv, t, 3, [0, 1, 3])
    assert PE.same_bits(a, b)
    one.free()
    two.free()


def test_adjoint_plan_has_nothing_to_differentiate_after_an_evaluate(emu):
    ctx = context(emu)
    pv, t, _ = inputs(CFG_ROLL)
    plan = Plan.load(exported("roll", adjoint=BOTH))
    assert plan.describe()["format"] == 2
    g = torch.ones(2, 3, 16, 16)
    d_pv, d_t = torch.zeros_like(pv), torch.zeros_like(t)

    def vjp():
        return plan._lib.scot_plan_vjp(plan._h, g.data_ptr(), d_pv.data_ptr(), d_t.data_ptr(), 0.0, None)
    plan.run(pv, t)
    for steps in (1, 3):
        targets = torch.zeros(steps, 2, 3, 16, 16)
        rc, sums, _ = PE.evaluate(plan, ctx, pv, t, targets, steps, None, False)
        assert rc == 0 and torch.isfinite(sums).all()
        before = issued(plan)
        assert vjp() == -1 and issued(plan) == before
        plan.run(pv, t)
        assert vjp() == 0 and torch.isfinite(d_pv).all() and float(d_pv.abs().max()) > 0
        plan.run(pv, t)
    plan.free()


def test_training_plan_validates_at_the_current_weights(emu):
    """evaluate before and after one scot_plan_train_step: the error sums of scot_plan_loss's prediction at those weights, and no state
    change (snapshots taken before and after an evaluate are equal)"""
    import emu_session
    ctx = context(emu)
    model = synth_model(ScOTConfig(**SMALL), "fp32", train=True)
    opt = emu_session.fused_adamw(model, lr=1e-3, weight_decay=0.01, max_grad_norm=5.0)
    pv, t, y = inputs(SMALL)
    image = model.export_plan(pv, time=t, labels=y, train=opt)
    plan = Plan.load(image)
    assert plan.describe()["format"] == 4
    slices = [0, 1, 3, 4]
    seen = []
    for step in range(2):
        snap = plan.snapshot(image)
        _, pred = plan.loss(pv, t, y)
        rc, sums, got = PE.evaluate(plan, ctx, pv, t, y[None].contiguous(), 1, slices, True)
        assert rc == 0 and PE.same_bits(got[0], pred)
        alone = E.Launch(ctx, pred.reshape(2, 4, -1), y.reshape(2, 4, -1), slices)
        assert alone.call() == 0 and PE.same_bits(sums[0], alone.result())
        assert plan.snapshot(image) == snap
        seen.append(sums)
        if step == 0:
            plan.train_step(pv, t, y, 1e-3)
    assert not PE.same_bits(seen[0], seen[1])
    plan.free()


def test_refusals_issue_nothing(emu):
    ctx = context(emu)
    pv, t, _ = inputs(CFG_ROLL)
    plan = Plan.load(exported("roll"))
    L, h = plan._lib, plan._h
    targets = torch.zeros(3, 2, 3, 16, 16)
    sums = torch.full((3, 2, 2, 4), 7.0, dtype=torch.float64)
    ok = [0, 1, 3]

    def refused(status, pixel_values=pv, time=t, tg=targets, steps=3, slices=ok, groups=None, out=sums, handle=h):
        before = issued(plan)
        groups = (1 if slices is None else len(slices) - 1) if groups is None else groups
        rc = L.scot_plan_evaluate(handle, PE.addr(pixel_values), PE.addr(time), PE.addr(tg), steps, None if slices is None else E.int_array(slices),
                                  groups, PE.addr(out), None, None)
        assert rc == status and issued(plan) == before and bool((sums == 7.0).all()), (rc, status)
    refused(-1, pixel_values=None)
    refused(-1, tg=None)
    refused(-1, out=None)
    refused(-1, steps=0)
    refused(-1, steps=-2)
    refused(-1, slices=list(range(34)), groups=0)
    refused(-1, slices=list(range(34)), groups=33)
    refused(-1, slices=None, groups=2)
    refused(-1, slices=[0, 2, 1])
    refused(-1, slices=[0, 1, 1])
    refused(-1, slices=[0, 1, 4])          # beyond Cout = 3 (Cin is 5)
    refused(-1, time=None)                 # the plan takes a time
    refused(-1, time=None, steps=1)
    assert L.scot_plan_evaluate(h, pv.data_ptr(), t.data_ptr(), targets.data_ptr(), 3, E.int_array(ok), 2, sums.data_ptr(), None, None) == 0
    assert not bool((sums == 7.0).any())
    sums.fill_(7.0)
    plan.free()
    # a plan without a time input: one forward works (test_single_step...), a rollout is -3; a time given to it is -1
    spv, st, _ = inputs(SMALL)
    untimed = Plan.load(exported("untimed"))
    tg4 = torch.zeros(3, 2, 4, 32, 32)
    big = torch.full((3, 2, 1, 4), 7.0, dtype=torch.float64)
    for steps, time, status in ((3, None, -3), (3, st, -3), (1, st, -1)):
        before = issued(untimed)
        rc = L.scot_plan_evaluate(untimed._h, spv.data_ptr(), PE.addr(time), tg4.data_ptr(), steps, None, 1, big.data_ptr(), None, None)
        assert rc == status and issued(untimed) == before and bool((big == 7.0).all()), (steps, rc)
    untimed.free()
    # more output than input channels: one forward works, a rollout is -1
    wide = Plan.load(exported("widening"))
    wpv, wt, _ = inputs(dict(SMALL, num_channels=3, num_out_channels=4))
    before = issued(wide)
    assert L.scot_plan_evaluate(wide._h, wpv.data_ptr(), wt.data_ptr(), tg4.data_ptr(), 3, None, 1, big.data_ptr(), None, None) == -1
    assert issued(wide) == before and bool((big == 7.0).all())
    assert L.scot_plan_evaluate(wide._h, wpv.data_ptr(), wt.data_ptr(), tg4.data_ptr(), 1, None, 1, big.data_ptr(), None, None) == 0
    assert issued(wide) > before and torch.isfinite(big[0]).all() and bool((big[1:] == 7.0).all())
    wide.free()
    assert L.scot_plan_evaluate(None, pv.data_ptr(), t.data_ptr(), targets.data_ptr(), 3, None, 1, sums.data_ptr(), None, None) == -1


def test_example_compiles_with_the_system_c_compiler(tmp_path):
    """examples/plan_eval_host.c is plain C against the header and the HIP runtime's C API (it runs in tests/test_plan_eval_gpu.py: the
    emulated library has no HIP runtime for it to allocate from)"""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        import build_emu
        cc = build_emu.CLANG
    from poseidon_amd import build as scot_build
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(scot_build.HIPCC)))
    run = subprocess.run([cc, "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I",
                          os.path.join(rocm, "include"), "-c", os.path.join(ROOT, "examples", "plan_eval_host.c"), "-o", str(tmp_path / "plan_eval_host.o")],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-3000:]


# ------------------------------------------------------------------------------------------------------- Trainer.evaluate_on_device
class Samples(torch.utils.data.Dataset):
    """the tiny synthetic data set of tests/test_trainer_emu_cpu.py, with the reference's channel description"""
    channel_slice_list = [0, 1, 3, 4]
    printable_channel_description = ["rho", "uv", "p"]

    def __init__(self, n, cfg, seed):
        g = torch.Generator().manual_seed(seed)
        R = cfg.image_size
        self.x = torch.randn(n, cfg.num_channels, R, R, generator=g)
        self.y = 0.5 * self.x[:, :cfg.num_out_channels] + 0.1 * torch.randn(n, cfg.num_out_channels, R, R, generator=g)
        self.t = torch.rand(n, generator=g)
        self.mask = torch.zeros(cfg.num_out_channels, dtype=torch.bool)

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        return {"pixel_values": self.x[i], "labels": self.y[i], "time": float(self.t[i]), "pixel_mask": self.mask}


@pytest.mark.parametrize("ar_steps", [None, 2])
def test_trainer_evaluates_on_the_device(emu, tmp_path, ar_steps):
    from conftest import load_fixture
    from poseidon_amd.geometry import param_shapes
    from poseidon_amd.synth import synth_state_dict
    from scOT.metrics import channel_group_metrics
    from scOT.model import ScOT
    from scOT.trainer import Trainer, TrainingArguments
    f, meta = load_fixture("tiny_trained")
    cfg = ScOTConfig(**meta["cfg"])
    assert cfg.num_out_channels == 4
    model = ScOT(cfg, compute="fp32")
    model.load_state_dict(synth_state_dict(param_shapes(cfg), meta["regime"]))
    evals = Samples(3, cfg, 1)
    fired = []

    class Spy:
        def on_evaluate(self, args, state, control, metrics=None, **kw):
            fired.append(metrics)
    args = TrainingArguments(output_dir=str(tmp_path), per_device_train_batch_size=2, per_device_eval_batch_size=2, num_train_epochs=1)
    tr = Trainer(model=model, args=args, train_dataset=evals, eval_dataset=evals)
    tr.add_callback(Spy())
    if ar_steps:
        tr.set_ar_steps(ar_steps)
    out = tr.predict(evals, metric_key_prefix="eval")
    want = channel_group_metrics(out.predictions, out.label_ids, evals.channel_slice_list, evals.printable_channel_description)
    got = tr.evaluate_on_device()
    assert set(got) == {"eval_loss"} | {"eval_" + k for k in want}
    assert got["eval_loss"] == out.metrics["eval_loss"]
    for k, v in want.items():
        assert E.close(got["eval_" + k], v), (k, got["eval_" + k], v)
    assert fired == [got] and tr.state["log_history"][-1] == dict(got, step=tr.state["global_step"])
    # without a channel description: one group, the single-group keys
    plain = Samples(3, cfg, 1)
    plain.channel_slice_list = plain.printable_channel_description = None
    one = tr.evaluate_on_device(plain, metric_key_prefix="test")
    # (against the torch-op path on fp64 copies: its fp32 sums are 1e-7 off per sample, which the std of three samples magnifies)
    want1 = channel_group_metrics(out.predictions.astype(np.float64), out.label_ids.astype(np.float64), [0, 4])
    assert set(one) == {"test_loss"} | {"test_" + k for k in want1}
    for k, v in want1.items():
        assert E.close(one["test_" + k], v), (k, one["test_" + k], v)
