"""Exported inference plans on the CPU emulation: `ScOT.export_plan` (poseidon_amd/plan.py) records the engine's inference forward
against libscot_emu.so, the plan runtime of the same library (csrc/plan.hip) loads the image into plain host memory and replays it.
Bit-identity with the engine's own forward, the refusals of the exporter and of the loader, and the header / prototype table."""
import ctypes
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from conftest import load_fixture  # noqa: E402
from plan_support import CFG96, CFG_ROLL, ROOT, check_images_stand_alone, emulated, other_inputs, patched, relocation_beyond_its_buffer  # noqa: E402
from plan_support import renamed, synth_model as build_model, truncations  # noqa: E402
from poseidon_amd import engine as engine_mod, harness, lib as scotlib, plan as plan_mod  # noqa: E402
from poseidon_amd.config import ScOTConfig  # noqa: E402
from poseidon_amd.plan import Plan, PlanExportError  # noqa: E402
from poseidon_amd.synth import synth_inputs  # noqa: E402
from scOT.model import ScOT  # noqa: E402


@pytest.fixture()
def emu(monkeypatch):
    return emulated(monkeypatch, hip_guard=True)      # (ScOT.forward keeps refusing CPU tensors here)


def own_forward(model, pv, t):
    with torch.no_grad():
        return model._engine.forward(pv, t, None, None, train=False, stochastic=False)[1].clone()


_cache = {}


def exported(name, tmp_path_factory):
    """one export per configuration for the whole module: (model, inputs, path of the plan file)"""
    if name not in _cache:
        if name == "tiny_odd":
            meta = load_fixture("tiny_odd")[1]
            cfg, compute = ScOTConfig(**meta["cfg"]), "fp32"
            pv, t, _ = synth_inputs(meta["batch"], cfg.num_channels, cfg.num_out_channels, meta.get("size", cfg.image_size), meta["kind"])
        elif name == "c96":
            cfg, compute = ScOTConfig(**CFG96), "fp16"
            pv, t, _ = synth_inputs(1, 4, 4, 64, "smooth")
        else:
            cfg, compute = ScOTConfig(**CFG_ROLL), "fp32"
            pv, t, _ = synth_inputs(2, 5, 3, 16, "smooth")
        model = build_model(cfg, compute)
        path = str(tmp_path_factory.mktemp("plan") / f"{name}.plan")
        model.export_plan(pv, time=t, path=path)
        _cache[name] = (model, pv, t, path)
    return _cache[name]


@pytest.mark.parametrize("name", ["tiny_odd", "c96"])
def test_plan_round_trip_is_bit_identical(emu, tmp_path_factory, name):
    """The ragged tiny model in fp32 (padding, conditioned norms) and the 96-wide 16x16-window model in fp16 (fused layer tails, bias
    tables, trunk products in the bfloat16 build): export, load, run on the export inputs and on other inputs, scratch poisoned with
    NaN bytes first; a run after other inputs still gives the first answer, so nothing is carried between runs."""
    model, pv, t, path = exported(name, tmp_path_factory)
    assert os.path.getsize(path) > model._arena.data.numel() * 4
    plan = Plan.load(path)
    d = plan.describe()
    assert (d["batch"], d["channels"], d["height"], d["width"], d["out_channels"]) == (*pv.shape, model.config.num_out_channels)
    assert d["has_time"] == 1 and d["time_bytes"] == 4 * pv.shape[0] and d["has_pixel_mask"] == 0
    assert d["operand_format"] == (1 if name == "c96" else 0) and d["compute"] == plan_mod.COMPUTE_CODE[model.compute]
    assert d["device_bytes"] > 0 and d["calls"] > 10
    plan.poison(0xFF)
    pv2, t2 = other_inputs(pv, t)
    ref1, ref2 = own_forward(model, pv, t), own_forward(model, pv2, t2)
    assert torch.isfinite(ref1).all() and not torch.equal(ref1, ref2)
    got1 = plan.run(pv, t)
    assert torch.equal(got1, ref1)
    got2 = plan.run(pv2, t2)
    assert torch.equal(got2, ref2)
    assert torch.equal(plan.run(pv, t), ref1)
    if name == "tiny_odd":      # raw addresses instead of tensors
        out = torch.full_like(ref1, float("nan"))
        plan.run(pv2.data_ptr(), t2.data_ptr(), out=out.data_ptr())
        assert torch.equal(out, ref2)
    plan.free()


def test_plan_is_linear_and_relocated(emu, tmp_path_factory):
    """the image names entry points the runtime lists, holds no event entry, and no argument but the tagged ones"""
    model, pv, t, path = exported("c96", tmp_path_factory)
    image = open(path, "rb").read()
    h = Plan.header(image)
    names = [image[h[plan_mod.H_NAMES_OFF] + i * plan_mod.NAME_BYTES:][:plan_mod.NAME_BYTES].split(b"\0")[0].decode()
             for i in range(h[plan_mod.H_NNAMES])]
    assert set(names) <= set(plan_mod.runtime_entry_points(emu)) and "scot_block_tail_fwd" in names
    assert not {"scot_event_record", "scot_stream_wait_event"} & set(names)
    assert h[plan_mod.H_ABI] == scotlib.ABI_VERSION == 8 and h[plan_mod.H_OPERAND] == 1 and h[plan_mod.H_BYTES] == len(image)


def test_plan_rollout_matches_harness(emu, tmp_path_factory, monkeypatch):
    """num_channels > num_out_channels: 3 steps equal harness.rollout(..., ar_steps=3, output_all_steps=True) bit for bit"""
    model, pv, t, path = exported("roll", tmp_path_factory)

    def call(pixel_values=None, time=None, **kw):      # (ScOT.forward refuses CPU tensors: the engine below that guard, as model(...) calls it)
        from scOT.model import ScOTOutput
        tt = torch.as_tensor(time).reshape(-1).to(torch.float32).contiguous()
        return ScOTOutput(loss=None, output=own_forward(model, pixel_values.contiguous(), tt))
    monkeypatch.setattr(ScOT, "forward", lambda self, **kw: call(**kw))
    ref = harness.rollout(model, dict(pixel_values=pv, time=t), ar_steps=3, output_all_steps=True).output
    assert ref.shape == (2, 3, 3, 16, 16)
    plan = Plan.load(path)
    plan.poison(0xFF)
    got = plan.rollout(pv, t, 3)
    assert torch.equal(got, ref)
    assert not torch.equal(got[:, 0], got[:, 1])
    assert plan._lib.scot_plan_rollout(plan._h, pv.data_ptr(), t.data_ptr(), None, got.data_ptr(), 0, None) == -1
    plan.free()


# ------------------------------------------------------------------------------------------------------- refusals at export
def test_export_refusals(emu, monkeypatch, tmp_path):
    cfg = ScOTConfig(**CFG_ROLL)
    model = build_model(cfg, "fp32")
    pv, t, lab = synth_inputs(2, 5, 3, 16, "smooth")
    with pytest.raises(PlanExportError, match="labels"):
        model.export_plan(pv, time=t, labels=lab)
    with pytest.raises(PlanExportError, match="pixel_mask"):
        model.export_plan(pv, time=t, pixel_mask=torch.zeros(2, 3, dtype=torch.bool))
    with pytest.raises(PlanExportError, match="config.image_size"):
        model.export_plan(synth_inputs(2, 5, 3, 32, "smooth")[0], time=t)
    # stochastic depth in training mode
    m2 = build_model(ScOTConfig(**dict(CFG_ROLL, drop_path_rate=0.1)), "fp32")
    m2.train()
    with pytest.raises(PlanExportError, match="stochastic depth"):
        m2.export_plan(pv, time=t)
    # a host-side Python step left in the recording is named
    def host_side_step():
        pass
    orig_mark = engine_mod.ScOTEngine.mark

    def mark(self, label):
        if label == "fwd head":
            self.tdo(host_side_step)
        return orig_mark(self, label)
    monkeypatch.setattr(engine_mod.ScOTEngine, "mark", mark)
    with pytest.raises(PlanExportError, match="host_side_step"):
        model.export_plan(pv, time=t)
    monkeypatch.setattr(engine_mod.ScOTEngine, "mark", orig_mark)
    # an entry point the runtime does not list
    listed = plan_mod.runtime_entry_points
    monkeypatch.setattr(plan_mod, "runtime_entry_points", lambda lib: [n for n in listed(lib) if n != "scot_conv5"])
    with pytest.raises(PlanExportError, match="scot_conv5"):
        model.export_plan(pv, time=t)
    monkeypatch.setattr(plan_mod, "runtime_entry_points", listed)
    # a device address no funnel registered: the entry point and the argument index are named
    orig_add = plan_mod._Registry.add

    def add(self, ten, kind, name):
        if name != "cpb_coords":
            orig_add(self, ten, kind, name)
    monkeypatch.setattr(plan_mod._Registry, "add", add)
    with pytest.raises(PlanExportError, match=r"argument 4 of scot_cpb_fwd_batched"):
        model.export_plan(pv, time=t)
    monkeypatch.setattr(plan_mod._Registry, "add", orig_add)
    # nothing was written by a refused export, and a good one still works afterwards
    path = tmp_path / "ok.plan"
    model.export_plan(pv, time=t, path=str(path))
    assert path.exists()


def test_export_refuses_a_cpu_model():
    """without the emulation's patches a CPU tensor has no device address: refused before anything is recorded"""
    model = ScOT(ScOTConfig(**CFG_ROLL), compute="fp32")
    pv, t, _ = synth_inputs(2, 5, 3, 16, "smooth")
    with pytest.raises(PlanExportError, match="CPU model"):
        model.export_plan(pv, time=t)


# ------------------------------------------------------------------------------------------------------- refusals at load
def corrupt_images(image):
    """{label: (bytes, expected status)}: the corrupt variants of a good image"""
    h = Plan.header(image)
    H = plan_mod
    out = truncations(image, (h[H.H_NAMES_OFF], h[H.H_BUFFERS_OFF], h[H.H_ENTRIES_OFF], h[H.H_ARRAYS_OFF], h[H.H_IO_OFF], h[H.H_DATA_OFF]))
    out["relocation beyond its buffer"] = (relocation_beyond_its_buffer(image, "forward"), -1)
    out["unknown entry point"] = (renamed(image, 0, "scot_adamw_step"), -3)
    out["n_int = 49"] = (patched(image, h[H.H_ENTRIES_OFF] + 16, 49), -1)
    out["wrong ABI"] = (patched(image, 8 * H.H_ABI, h[H.H_ABI] + 1), -3)
    out["other operand format"] = (patched(image, 8 * H.H_OPERAND, 1 - h[H.H_OPERAND]), -3)
    return out


def test_load_refusals(emu, tmp_path_factory):
    """each corrupt image gets a negative status and no plan; a run on the null handle is rejected"""
    import emu_session
    model, pv, t, path = exported("roll", tmp_path_factory)
    image = open(path, "rb").read()
    lib = plan_mod.bind(emu)
    handle = ctypes.c_void_p()
    assert plan_mod.load_raw(lib, image, handle) == 0 and handle.value
    assert lib.scot_plan_free(handle) == 0
    out = torch.empty(2, 3, 16, 16)
    for label, (bad, status) in corrupt_images(image).items():
        handle = ctypes.c_void_p(0xdead)
        assert plan_mod.load_raw(lib, bad, handle) == status, label
        assert not handle.value, label
        assert lib.scot_plan_run(handle, pv.data_ptr(), t.data_ptr(), None, out.data_ptr(), None) < 0, label
        assert lib.scot_plan_describe(handle, (ctypes.c_longlong * 16)()) < 0
    # the image of one operand format into the other build (both real builds, nothing patched)
    other = plan_mod.bind(emu_session.load_emu("f16"))
    handle = ctypes.c_void_p()
    assert plan_mod.load_raw(other, image, handle) == -3 and not handle.value
    with pytest.raises(scotlib.ScotLibraryError, match="refused"):
        Plan.load(image, lib=other)
    # wrong inputs for a good plan
    plan = Plan.load(image)
    assert lib.scot_plan_run(plan._h, pv.data_ptr(), None, None, out.data_ptr(), None) == -1       # time is an input of this plan
    assert lib.scot_plan_run(plan._h, None, t.data_ptr(), None, out.data_ptr(), None) == -1
    with pytest.raises(ValueError):
        plan.run(pv[:1], t[:1])
    plan.free()


# ------------------------------------------------------------------------------------------------------- header, table, checker
def test_plan_header_and_prototype_table(emu):
    """scot_plan.h and lib.PLAN_PROTOTYPES hold the same names, each exported by both builds (emulated here; the gfx950 builds are
    checked where the library is loaded: lib.load binds the plan table too); the kernel header does not know them."""
    import emu_session
    header = open(os.path.join(ROOT, "include", "scot_plan.h")).read()
    declared = set(re.findall(r"\b(scot_[a-z0-9_]+)\s*\(", header))
    assert declared == set(scotlib.PLAN_PROTOTYPES)
    assert {"scot_plan_load", "scot_plan_describe", "scot_plan_run", "scot_plan_rollout", "scot_plan_free"} <= declared
    for kind in ("bf16", "f16"):
        lib = emu_session.load_emu(kind)
        for name in declared:
            assert getattr(lib, name) is not None
    assert not set(scotlib.PLAN_PROTOTYPES) & set(scotlib.PROTOTYPES)
    assert "scot_plan_" not in re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scot_hip.h")).read(), flags=re.S)
    listed = plan_mod.runtime_entry_points(emu)
    assert set(listed) <= set(scotlib.PROTOTYPES) and len(listed) == len(set(listed))
    assert all(scotlib.PROTOTYPES[n][-1] is ctypes.c_void_p for n in listed)      # the stream, last


def test_gfx950_builds_export_the_plan_calls():
    for kind in ("bf16", "f16"):
        lib = scotlib.load(kind=kind)
        for name in scotlib.PLAN_PROTOTYPES:
            assert getattr(lib, name).argtypes == scotlib.PLAN_PROTOTYPES[name]
        assert lib.scot_abi_version() == 8
        assert lib.scot_plan_run(None, None, None, None, None, None) == -1 and lib.scot_plan_free(None) == 0


def test_stand_alone_image_check_under_sanitizers(emu, tmp_path_factory, tmp_path):
    """tools/plan_image_check.cc: csrc/plan_image.h's validator alone, built with the address and undefined-behaviour sanitizers, over a
    good image and the corrupt variants — a child process on the CPU."""
    model, pv, t, path = exported("roll", tmp_path_factory)
    image = open(path, "rb").read()
    check_images_stand_alone(tmp_path, {"good": (image, 0), **corrupt_images(image)})
