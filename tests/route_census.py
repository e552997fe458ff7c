"""Which kernel routes the engine's calls take — counted on the CPU, without running a kernel.

`scot_gemm`, `scot_wgrad_group` and the fused layer tails pick their kernel from shapes, dtypes, epilogue operands, pointer alignment and
policy thresholds.  The planners are pure and the library answers `scot_*_route` for any call (include/scot_hip.h), so the engine's host
program can be run against a proxy of the emulated library that launches NOTHING:

  * an entry point that launches is logged as (name, arguments) and answered with the status its planner gives (0, or the decline the
    real call would return, so that the engine's fall-backs run as they do on the GPU);
  * size, workspace, route and configuration queries go to the emulated library itself.

`census(config)` runs one training forward + backward of the engine that way and returns the calls; `key_of(lib, name, args)` turns one
call into its ROUTE KEY:

  (entry point, the route ints that name code, the epilogue class)

  scot_gemm         ("scot_gemm", layout, compute, family, row | variant, commit, split, zl, wide epilogue class,
                     a_dt, b_dt, c_dt, bias, colscale, aux: 0 | 1 gelu'(aux) | 2 aux as is, aux_dt, resid, res_dt, accumulate,
                     C2: 0 | 1 | 2 (C2 == C), colsum_out, a_gelu, b_gelu)
  scot_wgrad_group  ("scot_wgrad_group", status, kernel, variant, split, zl)
  fused tails       (entry point, status, C, HC, TT, qkv, pro, recomp)

Grid sizes and the values of M, N, K are not part of a key.  tests/test_kernel_routes_gpu.py holds one guarded case per key and the
closure test that every census key has one.

Dry-run buffers are torch.empty and mostly untouched: what the engine itself writes on the host (index tables, the parameter and gradient
arenas, fills of small tensors) is all that becomes resident.  Every configuration of CONFIGS fits: the peak resident size of the largest,
Poseidon-L at 128 x 128 and batch 128 in fp16, is 8.4 GB (10.8 GB where the other configurations ran in the same process before it; its
fp32 parameter and gradient arenas and their 16-bit copies; Poseidon-B at batch 64: 2.4 GB), and the nine configurations together take about 45 s — so no call had to be added by hand.  `python tests/route_census.py`
prints calls, keys, seconds and peak resident size per configuration, and every key with one engine call that has it.

No host read of the engine depends on a buffer the dry run leaves undefined (what it reads back — the gradient-scale state — it has
initialised on the host itself), so the proxy fills nothing.  tests/test_kernel_routes_gpu.py pins that on the GPU: a recorded real step of
Poseidon-T has exactly the key set of the dry run."""
import ctypes
import os
import sys
from collections import OrderedDict

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE, os.path.join(HERE, "hipemu")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from poseidon_amd import lib as scot_lib, ops  # noqa: E402

# (tag, image size, channels, batch, compute, input_grads): the five batch sizes bench.py times (tests/test_model_gpu.py TIMED) in fp16;
# Poseidon-B at batch 8 in the other three modes (the fp32 and bf16x3 tile rows, the generic kernel's engine forms); input gradients once
CONFIGS = [("B", 128, 4, 64, "fp16", ()), ("T", 128, 4, 32, "fp16", ()), ("B", 256, 4, 32, "fp16", ()), ("L", 128, 5, 128, "fp16", ()),
           ("L", 128, 5, 16, "fp16", ()), ("B", 128, 4, 8, "bf16", ()), ("B", 128, 4, 8, "fp32", ()), ("B", 128, 4, 8, "bf16x3", ()),
           ("T", 128, 4, 32, "fp16", ("pixel_values", "time"))]
CENSUS_NOTES = {}      # config -> (calls, peak resident MB), filled by census()

# entry points that launch nothing: forwarded to the emulated library
QUERIES = {n for n in scot_lib.PROTOTYPES if n.endswith(("_workspace_bytes", "_route", "_route_table", "_config"))} | {
    "scot_abi_version", "scot_operand_format", "scot_selftest_tr", "scot_set_use_tr", "scot_get_use_tr", "scot_block_tail_workgroups",
    "scot_optim_blocks", "scot_dp_world", "scot_dp_rank"}
ROUTED = ("scot_gemm", "scot_wgrad_group", "scot_mlp_block_fwd", "scot_mlp_block_bwd", "scot_proj_cln_fwd", "scot_proj_cln_bwd",
          "scot_block_tail_fwd", "scot_block_tail_bwd")


def _p(a):
    """a ctypes pointer argument as an integer (None / 0 = absent)"""
    if a is None:
        return 0
    if isinstance(a, ctypes.c_void_p):
        return a.value or 0
    return int(a)


def _tail_query(name, args):
    """(family, C, M, rows_per_sample, hid, qkv, pro, recomp) of a fused-tail launch, from its positional arguments (include/scot_hip.h)"""
    if name == "scot_mlp_block_fwd":          # ..., M, rows_per_sample, C, hid, eps, stream
        M, rps, C, hid = args[-6:-2]
        return ops.TAIL_MLP_FWD, C, M, rps, hid, 0, 0, 0
    if name == "scot_mlp_block_bwd":          # ..., M, rows_per_sample, C, hid, stream
        M, rps, C, hid = args[-5:-1]
        return ops.TAIL_MLP_BWD, C, M, rps, hid, 0, 0, 0
    if name == "scot_proj_cln_fwd":           # ..., M, rows_per_sample, C, eps, stream
        M, rps, C = args[-5:-2]
        return ops.TAIL_PROJ_FWD, C, M, rps, -1, 0, 0, 0
    if name == "scot_proj_cln_bwd":           # ..., M, rows_per_sample, C, stream
        M, rps, C = args[-4:-1]
        return ops.TAIL_PROJ_BWD, C, M, rps, -1, 0, 0, 0
    if name == "scot_block_tail_fwd":         # 33 pointers (the last: qkv), z_dt, time, M, rows_per_sample, C, hid, eps, stream
        M, rps, C, hid = args[-6:-2]
        return ops.TAIL_FWD, C, M, rps, hid, int(_p(args[32]) != 0), 0, 0
    if name == "scot_block_tail_bwd":         # g, g_out, 15 MLP pointers (dact: the 7th), 13 projection pointers, dqkv, Wqkv, ..., M, rps, C, hid, stream
        M, rps, C, hid = args[-5:-1]
        return ops.TAIL_BWD, C, M, rps, hid, 0, int(_p(args[30]) != 0), int(_p(args[8]) == 0)
    raise KeyError(name)


def route_of(lib, name, args):
    """the library's route answer (list of ints) for one logged launch; `args` as the launch received them (the stream last)"""
    route = (ctypes.c_int * scot_lib.ROUTE_INTS)()
    if name == "scot_gemm":
        rc = lib.scot_gemm_route(*args[:-1], route)
    elif name == "scot_wgrad_group":
        rc = lib.scot_wgrad_group_route(*args[:-1], route)
    else:
        rc = lib.scot_block_tail_route(*_tail_query(name, args), route)
    assert rc == 0, (name, rc)
    return list(route)


def status_of(name, route):
    """what the launch itself would answer from its plan: route[0] is the status except for scot_gemm, where it is the family (>= 0)"""
    return min(route[0], 0) if name == "scot_gemm" else route[0]


def key_of(lib, name, args):
    """the route key of one launch (module docstring)"""
    r = route_of(lib, name, args)
    if name == "scot_gemm":
        (layout, compute, M, N, K, A, a_dt, lda, a_gelu, B, b_dt, ldb, b_gelu, C, c_dt, ldc, bias, colscale, aux, aux_dt, ldaux, resid,
         res_dt, ldres, accumulate, colsum_out, ws, ws_bytes, aux_mul, C2) = args[:30]
        aux_on, res_on = _p(aux) != 0, _p(resid) != 0
        return ("scot_gemm", layout, compute, r[0], r[1], r[6], int(r[5] > 1), r[8], r[7],
                a_dt, b_dt, c_dt, int(_p(bias) != 0), int(_p(colscale) != 0), (2 if aux_mul else 1) if aux_on else 0, aux_dt if aux_on else 0,
                int(res_on), res_dt if res_on else 0, int(bool(accumulate)), 0 if not _p(C2) else (2 if _p(C2) == _p(C) else 1),
                int(_p(colsum_out) != 0), int(bool(a_gelu)), int(bool(b_gelu)))
    if name == "scot_wgrad_group":
        return ("scot_wgrad_group", r[0], r[1], r[2], int(r[3] > 1), r[4])
    return (name, r[0], r[1], r[2], r[3], r[5], r[6], r[7])


GEMM_KEY_FIELDS = ("layout", "compute", "family", "row", "commit", "split", "zl", "wide_epi", "a_dt", "b_dt", "c_dt", "bias", "colscale", "aux",
                   "aux_dt", "resid", "res_dt", "accumulate", "C2", "colsum_out", "a_gelu", "b_gelu")
FAMILY = {0: "panel", 1: "wide", 2: "fast", 3: "generic"}
FAST_ROWS = ("T_64x64", "T_64x64_GLDS", "T_64x64_BK32", "T_64x64_DEEP", "T_64x96", "T_96x96", "T_F32_64x64", "T_X3_64x64", "T_X3_64x96", "T_X3_96x96")
GROUP_KERNELS = ("GROUP_64x64", "GROUP_64x64_KG2", "GROUP_96x96", "GROUP_WIDE")


def describe_key(key):
    """a key in words, for failure messages"""
    if key[0] == "scot_gemm":
        d = dict(zip(GEMM_KEY_FIELDS, key[1:]))
        fam = FAMILY.get(d["family"], f"status {d['family']}")
        row = FAST_ROWS[d["row"]] if d["family"] == 2 else d["row"]
        flags = [f for f in ("bias", "colscale", "resid", "accumulate", "colsum_out", "a_gelu", "b_gelu") if d[f]]
        flags += [("aux(gelu')", "aux_mul")[d["aux"] - 1] + f":{d['aux_dt']}"] if d["aux"] else []
        flags += [("C2", "C2==C")[d["C2"] - 1]] if d["C2"] else []
        return (f"scot_gemm {('NT', 'NN', 'TN')[d['layout']]} compute {d['compute']} -> {fam} {row} commit {d['commit']} split {d['split']} zl {d['zl']} "
                f"epi {d['wide_epi']}; A/B/C dt {d['a_dt']}/{d['b_dt']}/{d['c_dt']} res_dt {d['res_dt']}; " + (" + ".join(flags) or "plain"))
    if key[0] == "scot_wgrad_group":
        return f"scot_wgrad_group status {key[1]} {GROUP_KERNELS[key[2]] if key[1] == 0 else '-'} variant {key[3]} split {key[4]} zl {key[5]}"
    return f"{key[0]} status {key[1]} C {key[2]} HC {key[3]} TT {key[4]} qkv {key[5]} pro {key[6]} recomp {key[7]}"


def describe_call(name, args, where):
    """one engine call in words: where the engine issued it, its shape and flags"""
    if name == "scot_gemm":
        return f"{where}: M {args[2]} N {args[3]} K {args[4]} lda {args[7]} ldb {args[11]} ldc {args[15]}"
    if name == "scot_wgrad_group":
        n = args[1]
        return f"{where}: K {args[2]} " + ", ".join(f"{args[7][i]}x{args[8][i]}" for i in range(n))
    q = _tail_query(name, args)
    return f"{where}: C {q[1]} M {q[2]} rows_per_sample {q[3]} hid {q[4]}"


def _where():
    """the engine function (and layer prefix, where one is in scope) that issued the launch being logged"""
    f = sys._getframe(2)
    while f is not None and not f.f_code.co_filename.endswith("engine.py"):
        f = f.f_back
    if f is None:
        return "?"
    out = f"{f.f_code.co_name}:{f.f_lineno}"
    g = f
    while g is not None and g.f_code.co_filename.endswith("engine.py"):
        for v in ("blk", "rec", "prefix"):
            o = g.f_locals.get(v)
            o = getattr(o, "blk", o)
            name = o if isinstance(o, str) else getattr(o, "prefix", None)
            if isinstance(name, str):
                return f"{name} {out}"
        g = g.f_back
    return out


class DryLibrary:
    """The proxy: logs launches, answers them from their plan, forwards queries."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name in QUERIES:
            return fn
        lib, log = self._lib, self._log

        def call(*args):
            rc = status_of(name, route_of(lib, name, args)) if name in ROUTED else 0
            if rc != -3:      # (as ops._Recording: a decline launches nothing, the caller falls back)
                log.append((name, args, _where()))
            return rc
        return call


def install(monkeypatch, log, load=None):
    """point poseidon_amd.ops at the proxy for one test, the way emu_session.patch_ops installs the emulated library: CPU tensors go down
    the same wrappers.  load(kind) -> the library that answers the queries: the emulated build (default), or on a GPU machine the real one
    (poseidon_amd.lib.load) — nothing is launched either way."""
    if load is None:
        import emu_session
        load = emu_session.load_emu
    ws = torch.empty(1 << 30, dtype=torch.uint8)      # never touched
    monkeypatch.setattr(ops, "L", lambda: DryLibrary(load(ops._active), log))
    monkeypatch.setattr(ops, "ptr", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(ops, "stream", lambda: None)
    monkeypatch.setattr(ops, "workspace", lambda need=0: ws)
    monkeypatch.setenv("SCOT_SIDE_STREAM", "0")      # HIP streams / events do not exist here: one in-order "stream"
    monkeypatch.setenv("SCOT_TAPE", "0")


def census(monkeypatch, tag, size, channels, batch, compute, input_grads=(), load=None):
    """-> [(name, args, where)] of one training forward + backward of a preset, nothing launched"""
    import resource
    from poseidon_amd.config import preset
    from scOT.model import ScOT
    log = []
    install(monkeypatch, log, load)
    cfg = preset(tag, image_size=size, num_channels=channels, num_out_channels=channels,
                 channel_slice_list_normalized_loss=[0, 1, channels - 1, channels])
    model = ScOT(cfg, compute=compute)
    model._ensure_arena(torch.device("cpu"))
    pv = torch.empty(batch, channels, size, size)
    t = torch.empty(batch) if cfg.use_conditioning else None
    loss, pred, tape = model._engine.forward(pv, t, torch.empty_like(pv), None, train=True, input_grads=input_grads)
    model._prepare_grads()
    model._engine.backward(tape, torch.ones(1), None)
    CENSUS_NOTES[(tag, size, channels, batch, compute, tuple(input_grads))] = (len(log), resource.getrusage(resource.RUSAGE_SELF).ru_maxrss // 1024)
    return log


def keys_of(log, lib=None):
    """{key: first (name, args, where) that has it} over the routed launches of a log, in call order"""
    if lib is None:
        import emu_session
        lib = emu_session.load_emu()
    out = OrderedDict()
    for name, args, where in log:
        if name in ROUTED:      # (the two builds of the library plan alike: the operand format is no input of any planner)
            out.setdefault(key_of(lib, name, args), (name, args, where))
    return out


if __name__ == "__main__":      # the census as a report: calls, keys and peak resident size per configuration
    import time
    import pytest
    total = OrderedDict()
    for cfg_ in CONFIGS:
        t0 = time.time()
        with pytest.MonkeyPatch.context() as mp:
            ks = keys_of(census(mp, *cfg_))
        new = [k for k in ks if k not in total]
        for k in new:
            total[k] = (cfg_, ks[k])
        n, rss = CENSUS_NOTES[cfg_[:5] + (tuple(cfg_[5]),)]
        print(f"{cfg_}: {n} launches, {len(ks)} keys ({len(new)} new), peak RSS {rss} MB, {time.time() - t0:.1f} s")
    for k, (cfg_, (name, args, where)) in total.items():
        print(describe_key(k), "|", cfg_[:5], describe_call(name, args, where))
    by = OrderedDict()
    for k in total:
        by[k[0]] = by.get(k[0], 0) + 1
    print(dict(by), "total", len(total))
