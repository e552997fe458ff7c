"""What the plan tests on the CPU emulation share (tests/test_plan*_emu_cpu.py): the emulated session, the model configurations and
builders, the walker over an image's call lists, the common corrupt images, and the stand-alone validator under the host sanitizers.
A plain module: fixtures are imported by name into the modules that use them."""
import ctypes
import os
import struct
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
from conftest import ROOT  # noqa: E402
from poseidon_amd import engine as engine_mod, lib as scotlib, plan as plan_mod  # noqa: E402
from poseidon_amd.config import ScOTConfig  # noqa: E402
from poseidon_amd.geometry import param_shapes  # noqa: E402
from poseidon_amd.plan import Plan  # noqa: E402
from poseidon_amd.synth import synth_inputs, synth_state_dict  # noqa: E402

H = plan_mod
BOTH = ("pixel_values", "time")
SMALL = dict(image_size=32, patch_size=4, num_channels=4, num_out_channels=4, embed_dim=16, depths=[2, 2], num_heads=[1, 2],
             skip_connections=[1, 0], window_size=4, mlp_ratio=4.0, p=1, channel_slice_list_normalized_loss=[0, 1, 3, 4],
             drop_path_rate=0.0, use_conditioning=True)
RESID = dict(SMALL, num_channels=5, num_out_channels=3, channel_slice_list_normalized_loss=[0, 1, 3], learn_residual=True)
WIDE = dict(image_size=64, patch_size=4, num_channels=4, num_out_channels=4, embed_dim=96, depths=[1, 1], num_heads=[3, 6],
            skip_connections=[1, 0], window_size=16, mlp_ratio=4.0, qkv_bias=True, drop_path_rate=0.0, hidden_act="gelu", p=1,
            channel_slice_list_normalized_loss=[0, 1, 3, 4], residual_model="convnext", use_conditioning=True, learn_residual=False)
CFG96 = dict(WIDE, depths=[2, 1])
# more input than output channels: the rollout passes the extra channels through
CFG_ROLL = dict(image_size=16, patch_size=4, num_channels=5, num_out_channels=3, embed_dim=16, depths=[1, 1], num_heads=[1, 2],
                skip_connections=[1, 0], window_size=4, mlp_ratio=2.0, qkv_bias=True, drop_path_rate=0.0, p=1,
                channel_slice_list_normalized_loss=[0, 1, 3], use_conditioning=True)
# the frozen models of the adjoint tests: (configuration, compute mode, batch)
FROZEN_MODELS = {"small": (SMALL, "fp32", 2), "resid": (RESID, "fp32", 2), "c96": (WIDE, "fp16", 1)}


# ------------------------------------------------------------------------------------------------------- session and models
def emulated(monkeypatch, hip_guard=False):
    """the emulated library behind `poseidon_amd.ops` for one test, one stream, the tiny models on the fused layer tails.
    hip_guard: ScOT.forward keeps refusing CPU tensors (otherwise `model(...)` runs on the emulation too)"""
    import emu_session
    lib = emu_session.load_emu()
    emu_session.patch_ops(monkeypatch, lib)
    monkeypatch.setenv("SCOT_SIDE_STREAM", "0")
    monkeypatch.setenv("SCOT_TAPE", "0")
    monkeypatch.setitem(engine_mod.ENGINE_OPTIONS, "fused_min_rows", 0)
    if not hip_guard:
        import scOT.model as M
        monkeypatch.setattr(M, "_require_hip", lambda t: None)
    return lib


@pytest.fixture()
def emu(monkeypatch):
    return emulated(monkeypatch)


def synth_model(cfg, compute, engine_options=None, train=False):
    """a ScOT with the synthetic trained weights, in eval (train: training) mode, its arena built on the CPU"""
    from scOT.model import ScOT
    model = ScOT(cfg, compute=compute, engine_options=engine_options)
    model.load_state_dict(synth_state_dict(param_shapes(cfg), "trained"))
    model.train(train)
    model._ensure_arena(torch.device("cpu"))
    return model


def frozen_model(name, engine_options=None):
    """-> (one of FROZEN_MODELS with every parameter frozen, pixel_values, time)"""
    kw, compute, batch = FROZEN_MODELS[name]
    cfg = ScOTConfig(**kw)
    model = synth_model(cfg, compute, engine_options)
    for p in model.parameters():
        p.requires_grad_(False)
    pv, t, _ = synth_inputs(batch, cfg.num_channels, cfg.num_out_channels, cfg.image_size, "smooth")
    return model, pv, t


def frozen_exports():
    """-> exported(name, tmp_path_factory, adjoint=BOTH) -> (model, pixel_values, time, path): one export per (configuration, request)
    for the whole of the calling module"""
    cache = {}

    def exported(name, tmp_path_factory, adjoint=BOTH):
        key = (name, adjoint)
        if key not in cache:
            model, pv, t = frozen_model(name)
            path = str(tmp_path_factory.mktemp("plan") / f"{name}_{len(adjoint)}.plan")
            model.export_plan(pv, time=t, path=path, adjoint=adjoint)
            cache[key] = (model, pv, t, path)
        return cache[key]
    return exported


def other_inputs(pv, t):
    g = torch.Generator().manual_seed(7)
    return pv.flip(0).flip(3) * 0.5 + 0.1 * torch.randn(pv.shape, generator=g), (t * 0.37 + 0.05)


def issued(plan):
    """the emulated runtime's launch log: every copy, fill and replayed call the plan runtime has issued"""
    fn = plan._lib.scot_plan_emu_issued
    fn.restype, fn.argtypes = ctypes.c_longlong, []
    return int(fn())


# ------------------------------------------------------------------------------------------------------- images
def word(image, off):
    return struct.unpack_from("<Q", image, off)[0]


def call_list(image, which):
    """(records, byte offset) of one call list of an image: "forward", "backward" (format 2) or step list 0 / 1 / 2 (format 4)"""
    h = Plan.header(image)
    if which == "forward":
        return h[H.H_NENTRIES], h[H.H_ENTRIES_OFF]
    if which == "backward":
        return h[H.H_NBACKWARD], h[H.H_BACKWARD_OFF]
    return plan_mod.training_words(image)[H.TR_FWD + 3 * which: H.TR_FWD + 3 * which + 2]


def entry_records(image, which):
    """the entry records of one call list -> (byte offset, name index, n_int) of each"""
    n, off = call_list(image, which)
    for _ in range(n):
        name, _, ni, nf = struct.unpack_from("<4Q", image, off)
        yield off, name, ni
        off += 8 * (4 + 2 * ni + nf)


def names_of(image, which):
    """entry-point names of the calls in one call list of an image"""
    h = Plan.header(image)
    names = [image[h[H.H_NAMES_OFF] + i * H.NAME_BYTES:][:H.NAME_BYTES].split(b"\0")[0].decode() for i in range(h[H.H_NNAMES])]
    return [names[name] for _, name, _ in entry_records(image, which)]


def patched(image, off, value):
    b = bytearray(image)
    b[off:off + 8] = struct.pack("<Q", value)
    return bytes(b)


def renamed(image, index, name):
    """the image with entry `index` of its name table replaced"""
    b = bytearray(image)
    o = Plan.header(image)[H.H_NAMES_OFF] + index * H.NAME_BYTES
    b[o:o + H.NAME_BYTES] = name.encode().ljust(H.NAME_BYTES, b"\0")
    return bytes(b)


def truncations(image, cuts):
    """{label: (bytes, -1)} of the image cut at each of `cuts`, at its last word, inside and before its header"""
    return {f"truncated at {c}": (image[:c], -1) for c in sorted({*cuts, H.HEADER_WORDS * 8, len(image) - 8, 8, 0})}


def relocation_beyond_its_buffer(image, which):
    """the image with the first relocation of the first entry of a call list moved to offset = its buffer's size"""
    h = Plan.header(image)
    off, _, ni = next(entry_records(image, which))
    for k in range(ni):
        tag = word(image, off + 32 + 16 * k)
        if tag & 0xFF == H.ARG_PTR:
            return patched(image, off + 32 + 16 * k + 8, word(image, h[H.H_BUFFERS_OFF] + 32 * (tag >> 8) + 8))
    raise AssertionError(f"the first entry of list {which!r} holds no relocation")


def check_images_stand_alone(tmp_path, cases):
    """tools/plan_image_check.cc — the validator alone, built with the address and undefined-behaviour sanitizers — over
    {label: (image bytes, expected status)}: a child process on the CPU, nothing preloaded"""
    import build_emu
    exe = str(tmp_path / "plan_image_check")
    cc = subprocess.run([build_emu.CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-I", os.path.join(ROOT, "poseidon_amd", "csrc"), os.path.join(ROOT, "tools", "plan_image_check.cc"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    args = [exe, str(scotlib.ABI_VERSION), "0"]
    for i, (label, (data, status)) in enumerate(cases.items()):
        p = tmp_path / f"case{i}.plan"
        p.write_bytes(data)
        args += [str(p), str(status)]
    run = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert f"{len(cases)} images checked" in run.stdout
