"""CPU execution of HIP kernel SOURCES through tests/hipemu (a host stand-in for hip_runtime.h: the work-items of a block as fibers,
wave64 cross-lane operations by rendezvous — see tests/hipemu/hip/hip_runtime.h).  Covers the fused block kernels of
poseidon_amd/csrc/mlp_fused.hip, (GPU parity: tests/test_kernels_gpu.py): index algebra, LDS aliasing and
barrier placement are checked here against double-precision loops.  No GPU, no libscot_hip.so: the kernel file is compiled
as plain C++ by the ROCm clang."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = os.environ.get("HIPEMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no host clang with __bf16 vector support")
    exe = str(tmp_path_factory.mktemp("hipemu") / "emu_fused")
    cmd = [CLANG, "-std=c++20", "-O2", "-pthread", "-I", os.path.join(HERE, "hipemu"), os.path.join(HERE, "hipemu", "emu_fused.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


# the in-process emulation tests (test_kernels_emu_cpu.py) run the default configuration (64 rows per workgroup, 64 hidden units per
# LDS chunk); the variants selected by environment variables that the library reads once per process are covered here
CASES = [  # case, C, B, L, cond, train, use_tr, SCOT_MLP_TT (16-row tiles per wave)
    ("mlp_fwd", 96, 1, 128, 1, 1, 1, 2), ("mlp_fwd", 96, 1, 100, 0, 1, 1, 1), ("mlp_bwd", 96, 1, 128, 1, 1, 1, 2),
    ("mlp_bwd", 96, 1, 64, 0, 1, 0, 1), ("proj_fwd", 96, 1, 128, 0, 0, 1, 2), ("proj_bwd", 96, 1, 128, 1, 1, 1, 2),
    ("proj_bwd", 96, 1, 192, 1, 1, 1, 3),    # a value other than 1 / 2 counts as unset: every 64-row tile of the 192 rows is processed
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_fused_block_kernels_on_cpu(emu, case):
    *args, tt = case
    env = dict(os.environ, SCOT_MLP_TT=str(tt))
    r = subprocess.run([emu, *[str(a) for a in args]], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout + r.stderr[-2000:]
