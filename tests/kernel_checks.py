"""What the kernel parity tests look with, beside the global relative L2 norm `rel()`:

  guarded()      an operand or result as a view inside one larger allocation whose bands (in front, behind, between the rows of a strided
                 view, between the members of a group) hold NaN of ONE fixed bit pattern.  A kernel that stores outside the extent it was
                 given changes a band (Guard.check() names the place); a kernel that loads outside it and lets the value reach an MFMA or a
                 sum turns its own result into NaN (0 * NaN = NaN), which the finite check and the bit-equality with the unguarded launch see.
  gemm_excess()  per-ELEMENT error of a product against the componentwise bound of an fp32-accumulated inner product: no stored tolerance.
  worst_rows()   per-row relative errors, printed by every failing assertion so that a failure names a row or a tile, not a norm.
  row_model_excess()  per-row comparison against a rounding model where no rigorous bound is practical (attention, conditional layer norm).

Plain module, device-agnostic: every function takes `device=`; callers pass `test_kernels_gpu.DEV` read at call time, so the CPU emulation's
patch of that name reaches them.  Nothing here provokes a fault: a stray access of up to a whole 128-row tile stays inside one torch
allocation."""
import torch

ALIGN_BYTES = 256          # poseidon_amd/arena.py aligns every parameter / gradient to 256 bytes; satisfies the 16 / 32-byte rules of scot_hip.h
ARENA_ALIGN_FLOATS = 64    # the same in fp32 elements: the spacing of neighbours in the flat arenas
MIN_BAND = 4096            # elements
TILE_ROWS = 128            # the widest kernel's tile (csrc/gemm_wide.hip, csrc/wgrad_wide.hip): one stray tile row must land inside a band

U32, U16F, U16B = 2.0 ** -24, 2.0 ** -11, 2.0 ** -8      # unit roundoff of fp32 / binary16 / bfloat16 (round to nearest)
UNIT = {torch.float32: U32, torch.float16: U16F, torch.bfloat16: U16B}
# half the spacing of the format's subnormals: the absolute rounding error of a result below the smallest normal number
SUBNORMAL_HALF_ULP = {U32: 2.0 ** -150, U16F: 2.0 ** -25, U16B: 2.0 ** -134}

# (integer view dtype, poison).  Floating formats: a quiet NaN with a payload no arithmetic produces (hardware NaNs are 0x7FC00000 / 0xFFC00000
# and their 16-bit kin), so "a NaN was stored over the band" is visible too.  Integer / byte tensors: a fixed non-zero pattern.
_POISON = {
    torch.float32: (torch.int32, 0x7FDEAD01),
    torch.float16: (torch.int16, 0x7E5A),
    torch.bfloat16: (torch.int16, 0x7FD5),
    torch.float64: (torch.int64, 0x7FF8DEADBEEF0001),
    torch.uint8: (torch.uint8, 0xA5),
    torch.int8: (torch.int8, 0x5A),
    torch.int16: (torch.int16, 0x5A5A),
    torch.int32: (torch.int32, 0x5A5A5A5A),
    torch.int64: (torch.int64, 0x5A5A5A5A5A5A5A5A),
}


def _geometry(shape, ld):
    shape = tuple(int(s) for s in shape)
    if not shape or any(s <= 0 for s in shape):
        raise ValueError(f"guarded(): bad shape {shape}")
    width = shape[-1]
    rows = 1
    for s in shape[:-1]:
        rows *= s
    ld = width if ld is None else int(ld)
    if ld < width:
        raise ValueError(f"guarded(): ld {ld} < row width {width}")
    strides, acc = [1], ld
    for s in reversed(shape[1:-1]):
        strides.append(acc)
        acc *= s
    if len(shape) > 1:
        strides.append(acc)
    strides = tuple(reversed(strides)) if len(shape) > 1 else (1,)
    return shape, rows, width, ld, strides


class Guard:
    """The poisoned surroundings of one or more views of one flat allocation."""

    def __init__(self, flat, name):
        self.flat = flat
        self.name = name
        self.idt, self.poison = _POISON[flat.dtype]
        self.ints = flat.view(self.idt)
        self.ints.fill_(self.poison)
        self.mask = torch.ones(flat.numel(), dtype=torch.bool, device=flat.device)     # True = guard element
        self.members = []        # (offset, rows, width, ld) of every view, in allocation order

    def _place(self, off, shape, rows, width, ld, strides):
        view = self.flat.as_strided(shape, strides, off) if ld != width else self.flat[off:off + rows * width].view(shape)
        self.mask.as_strided((rows, width), (ld, 1), off).fill_(False)
        self.members.append((off, rows, width, ld))
        return view

    def _where(self, i):
        """Name flat index i: which member it lies nearest to, which band, and the offset relative to that member's first element."""
        k = 0
        for j, (off, rows, width, ld) in enumerate(self.members):
            if i >= off:
                k = j
        off, rows, width, ld = self.members[k]
        end = off + (rows - 1) * ld + width
        relo = i - off
        if relo < 0:
            band = "front band"
        elif i >= end:
            band = "back band" if k == len(self.members) - 1 else f"padding behind member {k}"
        else:
            band = "row gap"
        tag = f" of member {k}" if len(self.members) > 1 and "member" not in band else ""
        return band + tag, relo, (relo // ld, relo % ld)

    def touched(self):
        """Flat indices of guard elements whose bits changed (int64 tensor on the CPU, ascending)."""
        bad = (self.ints != self.poison) & self.mask
        return bad.nonzero().flatten().cpu()

    def problems(self):
        idx = self.touched()
        if idx.numel() == 0:
            return None
        first, last = int(idx[0]), int(idx[-1])
        b0, r0, rc0 = self._where(first)
        b1, r1, rc1 = self._where(last)
        bits0 = int(self.ints[first])
        return (f"guard '{self.name}': {idx.numel()} element(s) outside the view were written; first in the {b0} at offset {r0:+d} from the view "
                f"(row {rc0[0]}, column {rc0[1]}; bits {bits0 & ((1 << 8 * self.flat.element_size()) - 1):#x}), last in the {b1} at offset {r1:+d} "
                f"(row {rc1[0]}, column {rc1[1]})")

    def check(self):
        """Bands, gaps and padding bit for bit (through the integer view: NaN != NaN)."""
        msg = self.problems()
        assert msg is None, msg


def _band(band, ld):
    return max(MIN_BAND, TILE_ROWS * ld) if band is None else int(band)


def _fill_body(view, src, fill):
    if src is not None:
        if tuple(src.shape) != tuple(view.shape):
            raise ValueError(f"guarded(): src shape {tuple(src.shape)} != {tuple(view.shape)}")
        view.copy_(src)
    elif fill is not None:
        view.fill_(fill)
    # else: the body keeps the poison (a result that the op stores; an accumulating op passes src= or fill=)


def guarded(shape, dtype, device, *, src=None, fill=None, ld=None, band=None, name="tensor"):
    """(view, guard): a view of `shape` (row width = last dimension, row stride `ld`, rows contiguous otherwise) that starts 256-byte
    aligned inside one flat allocation, with a band of `band` elements (default max(4096, 128 rows x ld)) in front and behind and, for
    ld > width, the ld - width elements behind every row poisoned as well.  Body: a copy of `src`, else `fill`, else poison (NaN)."""
    shape, rows, width, ld, strides = _geometry(shape, ld)
    band = _band(band, ld)
    es = torch.empty((), dtype=dtype).element_size()
    slack = ALIGN_BYTES // es
    span = (rows - 1) * ld + width
    flat = torch.empty(band + slack + span + band, dtype=dtype, device=device)
    g = Guard(flat, name)
    off = band + ((-(flat.data_ptr() + band * es)) % ALIGN_BYTES) // es
    view = g._place(off, shape, rows, width, ld, strides)
    assert view.data_ptr() % ALIGN_BYTES == 0
    _fill_body(view, src, fill)
    return view, g


def guarded_group(shapes, dtype, device, *, srcs=None, fills=None, align=ARENA_ALIGN_FLOATS, band=None, name="group"):
    """([views], guard): dense tensors back to back in ONE flat allocation the way poseidon_amd/arena.py lays parameters and gradients out:
    every member starts at the next multiple of `align` elements (256 bytes for fp32), the padding between neighbours is poisoned and
    checked like a band."""
    geo = [_geometry(s, None) for s in shapes]
    band = _band(band, max(g[2] for g in geo))
    es = torch.empty((), dtype=dtype).element_size()
    slack = ALIGN_BYTES // es
    offs, cur = [], 0
    for _, rows, width, _, _ in geo:
        offs.append(cur)
        cur += (rows * width + align - 1) // align * align
    flat = torch.empty(band + slack + cur + band, dtype=dtype, device=device)
    g = Guard(flat, name)
    base = band + ((-(flat.data_ptr() + band * es)) % ALIGN_BYTES) // es
    views = []
    for i, ((shape, rows, width, ld, strides), o) in enumerate(zip(geo, offs)):
        v = g._place(base + o, shape, rows, width, ld, strides)
        _fill_body(v, None if srcs is None else srcs[i], None if fills is None else fills[i])
        views.append(v)
    return views, g


def check_all(guards):
    msgs = [m for m in (g.problems() for g in guards) if m is not None]
    assert not msgs, "\n".join(msgs)


# ------------------------------------------------------------------------------------------------------------- per-element bound
def gemm_excess(got, ref64, absAB64, K, u_out, extra=0.0, u_add=U32, abs_extra=None):
    """(max over elements of |got - ref| / bound, index of that element) with

        bound = (u_out + extra) |ref|  +  K u_add (1 + u_out) (|A| |B|)  +  half a subnormal spacing of the output format

    i.e. ONE rounding of the result to the output format (u_out = 2^-24 / 2^-11 / 2^-8 for fp32 / binary16 / bfloat16) on top of the
    textbook componentwise bound of a K-term inner product accumulated in fp32 in ANY order (Higham, Accuracy and Stability of Numerical
    Algorithms, §3.1: |fl(x.y) - x.y| <= gamma_K |x|.|y|, gamma_K ~ K u).  `ref64` and `absAB64` = |A| |B| are fp64 on the operands as the
    MFMA sees them (after rounding to the operand format, after GELU-on-load).  `extra` is what an epilogue adds in fp32 before the single
    rounding, stated and derived at every call site.  The last term only matters for binary16 results below 2^-14, whose rounding error
    is absolute (2^-25), not relative.  A correct kernel cannot exceed 1; no measured number enters.

    Two assumptions.  u_out assumes a round-to-nearest-even conversion, which is what csrc/common.h states for its converters
    (v_cvt_pk_*): a store path that truncates fails this check, and should.  u_add = 2^-24 is the per-add roundoff of the fp32 MFMA (a
    k-ordered fmaf chain); the 16-bit MFMAs sum 32 products internally in an undocumented order and rounding, so their call sites pass
    u_add = 2^-23 (any faithfully rounding adder is within one ulp) — that loosens the K term only.

    abs_extra (optional, fp64 tensor like ref64) is an ABSOLUTE term added to the bound, for what is not relative to the result: an operand
    that reaches the MFMA with a known deviation from the reference operand (E |B|: the hi + lo split, a 16-bit re-rounding of a recomputed
    operand), the absolute error of the library's erf approximation in a GELU epilogue.  Derived at the call site like `extra`.

    A non-finite element of `got` (where the reference is finite) counts as an infinite excess."""
    got64 = got.double()
    bound = (u_out + extra) * ref64.abs() + K * u_add * (1.0 + u_out) * absAB64 + SUBNORMAL_HALF_ULP.get(u_out, 0.0)
    if abs_extra is not None:
        bound = bound + (1.0 + u_out) * abs_extra
    diff = (got64 - ref64).abs()
    ratio = diff / bound
    ratio = torch.where(diff == 0, torch.zeros_like(ratio), ratio)
    ratio = torch.where(torch.isfinite(got64), ratio, torch.full_like(ratio, float("inf")))
    flat = int(ratio.argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape)) if ratio.dim() else ()
    return float(ratio.reshape(-1)[flat]), idx


def excess_fraction(got, ref64, absAB64, K, u_out, extra=0.0, u_add=U32):
    """[rows] fraction of every row's elements above the bound of gemm_excess (reports: how much of a row / tile is wrong)."""
    bound = (u_out + extra) * ref64.abs() + K * u_add * (1.0 + u_out) * absAB64 + SUBNORMAL_HALF_ULP.get(u_out, 0.0)
    over = ~((got.double() - ref64).abs() <= bound)
    return over.reshape(-1, over.shape[-1]).double().mean(-1)


def row_errors(got, ref64):
    """[rows] relative L2 error of every row (rows = all dimensions but the last); a zero reference row divides by 1e-300."""
    d = (got.double() - ref64).reshape(-1, ref64.shape[-1])
    return d.norm(dim=-1) / ref64.reshape(-1, ref64.shape[-1]).norm(dim=-1).clamp_min(1e-300)


def worst_rows(got, ref64, k=5):
    """(per-row relative L2 errors, indices of the worst k rows, worst first)."""
    e = row_errors(got, ref64)
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
    k = min(k, e.numel())
    return e, [int(i) for i in torch.topk(e, k).indices]


def describe_worst(got, ref64, k=5, tile=None):
    e, idx = worst_rows(got, ref64, k)
    t = (lambda r: f" (tile row {r // tile})") if tile else (lambda r: "")
    return "worst rows: " + ", ".join(f"{r}{t(r)}: {float(e[r]):.2e}" for r in idx) + f"; median row {float(e.median()):.2e}"


def row_model_excess(got, exact64, model64, margin):
    """Per-row check where no rigorous bound is practical.  `model64` is the fp64 restatement with a rounding hook at the points the kernel
    documents; e_model[row] is its relative error against the exact fp64 result, e_kernel[row] the kernel's.  Returns
    (max over rows of e_kernel / (margin * max(e_model[row], median(e_model))), row).  NO row is left out: callers assert that no reference
    row norm is below 1e-6 of the median row norm (asserted here too), so the relative comparison is meaningful for every row."""
    n = exact64.shape[-1]
    rn = exact64.reshape(-1, n).norm(dim=-1)
    assert float(rn.min()) >= 1e-6 * float(rn.median()), "a reference row is (nearly) zero: compare it absolutely against the median row's bound"
    e_model = row_errors(model64, exact64)
    e_kernel = row_errors(got, exact64)
    e_kernel = torch.where(torch.isfinite(e_kernel), e_kernel, torch.full_like(e_kernel, float("inf")))
    allowed = margin * torch.maximum(e_model, e_model.median())
    ratio = e_kernel / allowed.clamp_min(1e-300)
    r = int(ratio.argmax())
    return float(ratio[r]), r
