"""Self-tests of tests/kernel_checks.py: every fault class the guard bands and the per-element bound are meant to catch, on plain CPU
tensors (no kernel involved).  The last group evaluates the suite's OLD metric — one global relative L2 norm — beside the new one on the
same faulty results and shows it staying under the old tolerance: the evidence that the gap is real."""
import pytest
import torch

import kernel_checks as kc
import test_kernels_gpu as G

DTYPES = [torch.float32, torch.float16, torch.bfloat16, torch.uint8, torch.int32, torch.int64]


# ------------------------------------------------------------------------------------------------------------------ guard bands
@pytest.mark.parametrize("dtype", DTYPES)
def test_untouched_guard_passes(dtype):
    v, g = kc.guarded((5, 7), dtype, "cpu", ld=12)
    assert v.data_ptr() % 256 == 0 and tuple(v.shape) == (5, 7) and tuple(v.stride()) == (12, 1)
    v.fill_(3)                                             # the whole body may be written
    g.check()
    assert g.problems() is None
    v2, g2 = kc.guarded((2, 3, 8), torch.float32, "cpu")   # dense: a contiguous view
    assert v2.is_contiguous() and v2.data_ptr() % 256 == 0 and bool(torch.isnan(v2).all())
    v2.zero_()
    g2.check()


def test_default_band_holds_a_stray_tile_row():
    _, g = kc.guarded((3, 100), torch.float32, "cpu", ld=104)
    off = g.members[0][0]
    assert off >= 128 * 104 and g.flat.numel() - (off + 2 * 104 + 100) >= 128 * 104
    _, g = kc.guarded((3, 8), torch.float32, "cpu")
    assert g.members[0][0] >= 4096


def test_src_and_fill_bodies():
    src = torch.arange(12.0).view(3, 4)
    v, g = kc.guarded((3, 4), torch.float32, "cpu", src=src, ld=9)
    assert torch.equal(v, src)
    v, g = kc.guarded((3, 4), torch.bfloat16, "cpu", fill=0.0)
    assert bool((v == 0).all())
    g.check()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8])
def test_store_just_before_the_view(dtype):
    v, g = kc.guarded((4, 8), dtype, "cpu", fill=0)
    g.flat[g.members[0][0] - 1] = 1
    with pytest.raises(AssertionError, match=r"front band at offset -1 .*row -1, column 7"):
        g.check()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.int32])
def test_store_just_after_the_view(dtype):
    v, g = kc.guarded((4, 8), dtype, "cpu", fill=0)
    g.flat[g.members[0][0] + 32] = 1
    with pytest.raises(AssertionError, match=r"back band at offset \+32 .*row 4, column 0"):
        g.check()


def test_store_after_a_strided_view_is_not_taken_for_a_gap():
    v, g = kc.guarded((4, 8), torch.float32, "cpu", fill=0, ld=10)
    g.flat[g.members[0][0] + 3 * 10 + 8] = 0.0           # the element right behind the last row
    with pytest.raises(AssertionError, match=r"back band at offset \+38"):
        g.check()


def test_store_in_a_row_gap():
    v, g = kc.guarded((4, 8), torch.float32, "cpu", fill=0, ld=12)
    base = g.members[0][0]
    g.flat[base + 2 * 12 + 9] = 5.0                        # row 2, one past the row's end + 1
    g.flat[base + 1 * 12 + 8] = 5.0
    msg = g.problems()
    assert "2 element(s)" in msg and "first in the row gap at offset +20 from the view (row 1, column 8" in msg
    assert "last in the row gap at offset +33 (row 2, column 9)" in msg
    with pytest.raises(AssertionError):
        g.check()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_nan_overwritten_by_another_nan(dtype):
    """NaN != NaN and NaN "==" nothing: the compare goes through the integer view of the same bytes."""
    v, g = kc.guarded((4, 8), dtype, "cpu", fill=0)
    assert bool(torch.isnan(g.flat[:16]).all())
    g.flat[5] = float("nan")                               # the default quiet NaN: another bit pattern than the poison
    assert bool(torch.isnan(g.flat[5]))
    with pytest.raises(AssertionError, match="front band"):
        g.check()


def test_group_padding_is_a_band():
    shapes = [(3, 10), (5, 20), (7,)]
    views, g = kc.guarded_group(shapes, torch.float32, "cpu", fills=[0.0, None, 1.0])
    assert [tuple(v.shape) for v in views] == shapes and all(v.data_ptr() % 256 == 0 for v in views)
    assert (views[1].data_ptr() - views[0].data_ptr()) // 4 == 64 and (views[2].data_ptr() - views[1].data_ptr()) // 4 == 128
    assert bool(torch.isnan(views[1]).all())
    for v in views:
        v.fill_(2.0)
    g.check()
    g.flat[g.members[0][0] + 30] = 0.0                     # first float behind member 0 (30 floats used of 64)
    with pytest.raises(AssertionError, match=r"padding behind member 0 at offset \+30"):
        g.check()
    with pytest.raises(AssertionError):
        kc.check_all([g])


def test_worst_rows_names_the_row():
    ref = torch.randn(50, 16, dtype=torch.float64)
    got = ref.clone()
    got[17] *= 1.5
    got[3, 2] += 0.01
    e, idx = kc.worst_rows(got, ref, k=3)
    assert idx[:2] == [17, 3] and abs(float(e[17]) - 0.5) < 1e-12
    assert "17 (tile row 1)" in kc.describe_worst(got, ref, tile=16)
    got[40, 0] = float("nan")
    assert kc.worst_rows(got, ref)[1][0] == 40


def test_row_model_excess():
    g = torch.Generator().manual_seed(0)
    exact = torch.randn(64, 32, generator=g, dtype=torch.float64)
    model = exact.to(torch.bfloat16).double()
    assert kc.row_model_excess(model, exact, model, 1.0)[0] <= 1.0
    got = model.clone()
    got[9] = exact[9] + 5 * (model[9] - exact[9])
    worst, row = kc.row_model_excess(got, exact, model, 2.0)
    assert row == 9 and worst > 1.0
    z = exact.clone()
    z[5] = 0
    with pytest.raises(AssertionError, match="nearly"):
        kc.row_model_excess(z, z, z, 2.0)


# ------------------------------------------------------------------------------------------------------- the per-element bound
SHAPES = sorted({(M, N, K) for M, N, K in G.GEMM_SHAPES + [c[:3] for c in G.WIDE_CASES] if M * N * K <= 1.3e9})      # bounded for the CPU
OLD_TOL = {torch.float16: 1.2e-3, torch.bfloat16: 6e-3}      # test_gemm_wide_tiles' tol16, the tightest 16-bit tolerance of the suite


def _product(M, N, K, dt, drop=None):
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).to(dt)
    B = (torch.randn(N, K, generator=g) * K ** -0.5).to(dt)
    Af = A.float()
    if drop is not None:
        r0, k0 = drop
        Af = Af.clone()
        Af[r0:r0 + 16, k0:k0 + 32] = 0
    got = (Af @ B.float().t()).to(dt)                      # fp32 accumulation, one rounding: what a correct kernel computes
    return got, A.double() @ B.double().t(), A.double().abs() @ B.double().abs().t()


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_excess_accepts_fp32_then_round(M, N, K, dt):
    got, ref, ab = _product(M, N, K, dt)
    worst, idx = kc.gemm_excess(got, ref, ab, K, kc.UNIT[dt])
    print(f"gemm_excess {M}x{N}x{K} {dt}: {worst:.3f} at {idx}")
    assert worst <= 1.0
    assert kc.gemm_excess(got.float(), ref, ab, K, kc.UNIT[dt], u_add=2.0 ** -23)[0] <= worst


FAULT_SHAPE = (1024, 768, 768)


@pytest.fixture(scope="module", params=[torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def clean(request):
    dt = request.param
    M, N, K = FAULT_SHAPE
    got, ref, ab = _product(M, N, K, dt)
    assert kc.gemm_excess(got, ref, ab, K, kc.UNIT[dt])[0] <= 1.0 and G.rel(got, ref) < OLD_TOL[dt]
    return dt, got, ref, ab


def test_fault_one_element_by_twice_its_bound(clean):
    dt, got, ref, ab = clean
    K, u = FAULT_SHAPE[2], kc.UNIT[dt]
    bad = got.double()
    i, j = 700, 13
    b = u * abs(float(ref[i, j])) + K * 2.0 ** -24 * (1 + u) * float(ab[i, j])
    bad[i, j] += 2 * b * (1.0 if bad[i, j] >= ref[i, j] else -1.0)
    worst, idx = kc.gemm_excess(bad, ref, ab, K, u)
    assert worst > 1.0 and idx == (i, j)
    assert G.rel(bad, ref) < OLD_TOL[dt]                   # the old assertion passes


def test_fault_dropped_k_slice(clean):
    dt, got, ref, ab = clean
    M, N, K = FAULT_SHAPE
    bad, _, _ = _product(M, N, K, dt, drop=(1008, 736))    # the last 16 rows lose the last 32-deep K slice
    worst, idx = kc.gemm_excess(bad, ref, ab, K, kc.UNIT[dt])
    frac = kc.excess_fraction(bad, ref, ab, K, kc.UNIT[dt])
    print(f"dropped K slice {dt}: excess {worst:.1f}, flagged {float(frac[1008:].min()):.0%}..{float(frac[1008:].max()):.0%} of each row; "
          f"old metric {G.rel(bad, ref):.2e}")
    assert worst > 1.0 and idx[0] >= 1008
    assert float(frac[1008:].min()) > 0.5 and float(frac[:1008].max()) == 0.0
    assert kc.worst_rows(bad, ref, k=16)[1][0] >= 1008


def test_fault_row_scaled(clean):
    dt, got, ref, ab = clean
    K = FAULT_SHAPE[2]
    bad = got.clone()
    bad[333] = (got[333].float() * 1.03).to(dt)
    worst, idx = kc.gemm_excess(bad, ref, ab, K, kc.UNIT[dt])
    frac = kc.excess_fraction(bad, ref, ab, K, kc.UNIT[dt])
    old = G.rel(bad, ref)
    print(f"row x 1.03 {dt}: excess {worst:.1f}, flagged {float(frac[333]):.0%} of the row; old metric {old:.2e} (tolerance {OLD_TOL[dt]:.1e})")
    assert worst > 1.0 and idx[0] == 333 and float(frac[333]) > 0.5
    assert kc.worst_rows(bad, ref)[1][0] == 333
    assert old < OLD_TOL[dt]                               # the old assertion passes


def test_fault_row_replaced_by_its_neighbour(clean):
    dt, got, ref, ab = clean
    bad = got.clone()
    bad[512] = got[511]
    worst, idx = kc.gemm_excess(bad, ref, ab, FAULT_SHAPE[2], kc.UNIT[dt])
    assert worst > 1.0 and idx[0] == 512 and kc.worst_rows(bad, ref)[1][0] == 512


def test_gemm_excess_counts_non_finite_as_infinite(clean):
    dt, got, ref, ab = clean
    bad = got.clone()
    bad[5, 5] = float("nan")
    worst, idx = kc.gemm_excess(bad, ref, ab, FAULT_SHAPE[2], kc.UNIT[dt])
    assert worst == float("inf") and idx == (5, 5)


def test_gemm_excess_absolute_term():
    """abs_extra widens the bound by an absolute amount (an operand's known deviation, an approximation's absolute error) and by nothing else"""
    ref = torch.tensor([[0.0, 1.0], [-2.0, 1e-9]], dtype=torch.float64)
    zero = torch.zeros_like(ref)
    got = ref + torch.tensor([[1e-7, 0.0], [0.0, -1e-7]], dtype=torch.float64)
    assert kc.gemm_excess(got, ref, zero, 0, kc.U32)[0] > 1.0
    worst, idx = kc.gemm_excess(got, ref, zero, 0, kc.U32, abs_extra=torch.full_like(ref, 2e-7))
    assert worst <= 0.51 and idx in ((0, 0), (1, 1))
    assert kc.gemm_excess(got, ref, zero, 0, kc.U32, abs_extra=torch.full_like(ref, 0.5e-7))[0] > 1.0
