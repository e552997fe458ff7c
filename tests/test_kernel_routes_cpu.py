"""The kernel routes on the CPU (tests/route_census.py, tests/test_kernel_routes_gpu.py): no GPU, nothing launched except on the emulated
kernels.

  closure      every route key of the engine's calls, over all census configurations, has a case in ROUTE_CASES: a policy change that moves
               a preset's call onto a route without a guarded case fails here, naming the key and one engine call that has it;
  drift        every case takes the route it declares on the emulated library (the planners are the GPU library's own sources);
  dead rows    every row of gemm_fast's tile table x layout, every 128 x 128 variant, every grouped weight-gradient kernel and every
               (row, family) of the fused tails' table is the route of at least one case — also those only the C ABI reaches;
  emulation    the cases small enough run their guarded body on the emulated kernels."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
import route_census as RC  # noqa: E402
import test_kernel_routes_gpu as R  # noqa: E402
from poseidon_amd import ops  # noqa: E402


@pytest.fixture()
def emu_bodies(monkeypatch):
    """the guarded bodies on CPU tensors and the emulated library (as tests/test_kernels_emu_cpu.py runs them)"""
    import emu_session
    import test_kernels_gpu as G
    lib = emu_session.load_emu()
    emu_session.patch_ops(monkeypatch, lib)
    monkeypatch.setattr(G, "DEV", "cpu")
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    return lib


_census = {}


def census_keys():
    """{key: (configuration, one engine call that has it)} over RC.CONFIGS, computed once per session"""
    if not _census:
        import gc
        for cfg in RC.CONFIGS:
            with pytest.MonkeyPatch.context() as mp:
                keys = RC.keys_of(RC.census(mp, *cfg))
            for k, call in keys.items():
                _census.setdefault(k, (cfg, call))
            gc.collect()
    return _census


def test_every_census_key_has_a_route_case():
    have = {k for c in R.ROUTE_CASES for k in c.keys}
    census = census_keys()
    by_entry = {}
    for k in census:
        by_entry[k[0]] = by_entry.get(k[0], 0) + 1
    print(f"census: {len(census)} keys {by_entry}; cases: {len(R.ROUTE_CASES)} with {len(have)} keys; peak resident MB per configuration: "
          f"{ {c[:5]: v[1] for c, v in RC.CENSUS_NOTES.items()} }")
    missing = [k for k in census if k not in have]
    assert not missing, f"{len(missing)} route key(s) of the engine's calls have no guarded case in ROUTE_CASES:\n" + "\n".join(
        f"  {RC.describe_key(k)}\n      e.g. {census[k][0][:5]} {RC.describe_call(*census[k][1])}\n      key = {k}" for k in missing)


def test_the_census_sees_every_configuration_family():
    """the census itself is alive: every configuration issues routed calls, the 16-bit ones reach all four entry-point kinds"""
    census = census_keys()
    assert {k[0] for k in census} == {"scot_gemm", "scot_wgrad_group", "scot_block_tail_fwd", "scot_block_tail_bwd"}
    assert all(n > 500 for n, _ in RC.CENSUS_NOTES.values()), RC.CENSUS_NOTES


@pytest.mark.parametrize("case", R.ROUTE_CASES, ids=R.CASE_IDS)
def test_case_takes_its_declared_route(emu_bodies, case):
    if case.body == "gemm":
        R.run_case(case, dry=True)      # the body's own assertion on its guarded arguments, strided and dense; nothing is launched
    else:
        took = R.shape_keys(case, emu_bodies)
        assert took == set(case.keys), "declared " + "; ".join(RC.describe_key(k) for k in case.keys) + "\ntakes " + "; ".join(RC.describe_key(k) for k in took)


def table_rows():
    """every (kind, ...) a route can name, from the library's own tables"""
    rows = []
    for i, r in enumerate(ops.route_table(0)):
        rows += [("fast", i, l) for l in range(3) if r[4] >> l & 1]
    rows += [("wide", v) for v in range(len(ops.route_table(2)))]
    rows += [("group", g) for g in range(len(ops.route_table(3)))]
    entry = {ops.TAIL_MLP_FWD: "scot_mlp_block_fwd", ops.TAIL_MLP_BWD: "scot_mlp_block_bwd", ops.TAIL_PROJ_FWD: "scot_proj_cln_fwd",
             ops.TAIL_PROJ_BWD: "scot_proj_cln_bwd", ops.TAIL_FWD: "scot_block_tail_fwd", ops.TAIL_BWD: "scot_block_tail_bwd"}
    for r in ops.route_table(1):
        rows += [(entry[f], r[1], r[2], r[3]) for f in range(6) if r[4] >> f & 1]
    return rows


def covered_rows():
    out = set()
    for c in R.ROUTE_CASES:
        for k in c.keys:
            if k[0] == "scot_gemm" and k[3] == ops.ROUTE_FAST:
                out.add(("fast", k[4], k[1]))
            elif k[0] == "scot_gemm" and k[3] == ops.ROUTE_WIDE:
                out.add(("wide", k[4]))
            elif k[0] == "scot_wgrad_group":
                out.add(("group", k[2]))
            elif k[0] != "scot_gemm":
                out.add((k[0], k[2], k[3], k[4]))
    return out


def test_no_table_row_is_without_a_case(emu_bodies):
    rows = table_rows()
    assert len(rows) > 40 and ("fast", R.T_64x64_GLDS, ops.NT) in rows and ("scot_block_tail_bwd", 48, 192, 1) in rows
    dead = [r for r in rows if r not in covered_rows()]
    unknown = [r for r in dead if r not in R.UNREACHABLE_ROWS]
    assert not unknown, f"table rows that no case in ROUTE_CASES takes: {unknown}"
    stale = [r for r in R.UNREACHABLE_ROWS if r not in dead]
    assert not stale, f"listed as unreachable but covered, or no longer in the table: {stale}"


@pytest.mark.parametrize("row", sorted(R.UNREACHABLE_ROWS), ids=lambda r: "-".join(str(x) for x in r))
def test_unreachable_row(emu_bodies, row, request):
    request.applymarker(pytest.mark.xfail(reason=R.UNREACHABLE_ROWS[row], strict=True))
    assert row in covered_rows()


EMU_CASES = [(c, i) for c, i in zip(R.ROUTE_CASES, R.CASE_IDS) if c.emu]


@pytest.mark.parametrize("case", [c for c, _ in EMU_CASES], ids=[i for _, i in EMU_CASES])
def test_route_case_on_the_emulated_kernels(emu_bodies, case):
    R.run_case(case)
