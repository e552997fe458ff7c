"""scot_error_sums (csrc/error_sums.hip) on the CPU emulation: the kernel source itself runs, one fiber per work-item, inside NaN guard
bands; the case list, the fp64 reference and the derived bound are tests/error_sums_cases.py's (shared with the GPU module)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
import error_sums_cases as E  # noqa: E402
from poseidon_amd import lib as scotlib, ops, plan as plan_mod  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    import emu_session
    return E.Ctx(plan_mod.bind(emu_session.load_emu()), torch.device("cpu"))


def test_chunk_constant(ctx):
    E.check_chunk_constant(ctx)


@pytest.mark.parametrize("case", [c for c in E.CASES if not c[6]], ids=lambda c: c[0])
def test_case_within_the_fp64_bound(ctx, case):
    _, B, C, HW, slices, nan_channels, _ = case
    E.check_case(ctx, B, C, HW, slices, nan_channels)


def test_vector_and_scalar_loads_give_the_same_bits(ctx):
    """a lane owns the same floats on both paths: the sums do not depend on the operands' alignment"""
    B, C, HW = 2, 4, 256
    pr, tg = E.make_inputs(B, C, HW)
    aligned = E.Launch(ctx, pr, tg, E.PINS_SLICES)
    assert aligned.call() == 0
    want = aligned.result()
    shifted = E.Launch(ctx, pr, tg, E.PINS_SLICES)
    flat = torch.empty(B * C * HW + 1)
    flat[1:] = pr.reshape(-1)
    shifted.pred = flat[1:].view(B, C, HW)           # 4 bytes off the 16-byte boundary: every run takes the scalar path
    assert shifted.pred.data_ptr() % 16 == 4 and shifted.call() == 0
    assert torch.equal(shifted.result().view(torch.int64), want.view(torch.int64))


def test_nonfinite_values_go_through(ctx):
    E.check_nonfinite(ctx)


def test_refusals_leave_sums_untouched(ctx):
    E.check_refusals(ctx)


def test_from_sums_helpers_reproduce_the_reference_pins():
    """the CPU path of scOT.metrics.error_sums (plain fp64) -> the pins of the real reference's metrics module"""
    from scOT import metrics as M
    for wrap in (lambda x: x, torch.from_numpy):
        one = E.check_pins(lambda pr, tg, sl: M.error_sums(wrap(pr), wrap(tg), sl))
    assert isinstance(M.lp_error_from_sums(one.numpy()), np.ndarray) and isinstance(M.lp_error_from_sums(one), torch.Tensor)
    with pytest.raises(ValueError):
        M.error_sums(np.zeros((2, 4, 3)), np.zeros((2, 4, 3)), [0, 3, 1])
    with pytest.raises(ValueError):
        M.lp_error_from_sums(one, p=3)


def test_pins_through_the_emulated_kernel_and_ops_wrapper(ctx, monkeypatch):
    """the same pins from the kernel's sums, launched through poseidon_amd.ops.error_sums (what scOT.metrics.error_sums calls for GPU
    tensors), and those sums against the plain fp64 path within the bound"""
    import emu_session
    from scOT import metrics as M
    emu_session.patch_ops(monkeypatch, ctx.lib)

    def through_ops(pr, tg, slices):
        p, t = torch.from_numpy(pr).contiguous(), torch.from_numpy(tg).contiguous()
        out = torch.full((p.shape[0], 1 if slices is None else len(slices) - 1, 4), float("nan"), dtype=torch.float64)
        ops.error_sums(p, t, slices, out)
        ref = M.error_sums(p, t, slices)
        n = p[0].numel() if slices is None else None
        assert torch.isfinite(out).all() and ((out - ref).abs() <= 2 * (p[0].numel() + 2) * E.U64 * ref).all(), n
        return out
    E.check_pins(through_ops)
    with pytest.raises(ValueError):
        ops.error_sums(torch.zeros(2, 4, 3), torch.zeros(2, 4, 3), [0, 5], torch.zeros(2, 1, 4, dtype=torch.float64))


def test_header_and_prototypes_declare_the_new_calls(ctx):
    import re
    from conftest import ROOT
    new = {"scot_error_sums_workspace_bytes", "scot_error_sums", "scot_plan_evaluate"}
    header = open(os.path.join(ROOT, "include", "scot_plan.h")).read()
    declared = set(re.findall(r"\b(scot_[a-z0-9_]+)\s*\(", header))
    assert declared == set(scotlib.PLAN_PROTOTYPES) and new <= declared
    assert not new & set(scotlib.PROTOTYPES) and scotlib.ABI_VERSION == 8 and ctx.lib.scot_abi_version() == 8
    kernel_header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scot_hip.h")).read(), flags=re.S)
    assert "scot_error_sums" not in kernel_header
    listed = set(plan_mod.runtime_entry_points(ctx.lib)) | set(plan_mod.runtime_entry_points(ctx.lib, adjoint=True)) | \
        set(plan_mod.runtime_entry_points(ctx.lib, training=True))
    assert not new & listed                                # no recorded call list can name them
    for text in ("lp_error", "1e-10", "median"):           # how a host turns sums into the reference's numbers
        assert text in header


def test_gfx950_builds_export_the_new_calls():
    for kind in ("bf16", "f16"):
        lib = scotlib.load(kind=kind)
        for name in ("scot_error_sums_workspace_bytes", "scot_error_sums", "scot_plan_evaluate"):
            assert getattr(lib, name).argtypes == scotlib.PLAN_PROTOTYPES[name]
        assert lib.scot_abi_version() == 8
        assert lib.scot_error_sums_workspace_bytes(1, 1, E.CHUNK + 1, None, 1) == 64
        assert lib.scot_error_sums(None, None, 1, 1, 1, None, 1, None, None, 0, None) == -1
        assert lib.scot_plan_evaluate(None, None, None, None, 1, None, 1, None, None, None) == -1
