"""ms per call of `scot_plan_evaluate_masked` (a channel mask and an element mask) against `scot_plan_evaluate` — Poseidon-B, fp16,
128 x 128, batch 64, one step and eight.  `predictions == NULL` throughout: nothing but the sums leaves the plan.

usage: python tools/bench_plan_eval_masked.py [--batch 64] [--steps 1,8] [--plain-only] [--root CHECKOUT] [--repeat N]
  --plain-only  only `scot_plan_evaluate` (what a checkout without the masked call can run)
  --root        import the package from another checkout (the parent commit, built there) to time ITS evaluate in the same visit
  --repeat      time every case N times, the cases alternating: the values become lists
Prints one JSON line per step count.  Numbers: profiles/plan_eval/README.md."""
import argparse
import ctypes
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--steps", default="1,8")
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--repeat", type=int, default=2)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402
from poseidon_amd.config import preset  # noqa: E402
from poseidon_amd.plan import Plan  # noqa: E402
from scOT.model import ScOT  # noqa: E402

SLICES = [0, 1, 3, 4]


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.calls * 1e3


cfg = preset("B", image_size=128, num_channels=4, num_out_channels=4, channel_slice_list_normalized_loss=SLICES)
torch.manual_seed(1234)
model = ScOT(cfg, compute="fp16").to("cuda").eval()
B = args.batch
pv, t = torch.randn(B, 4, 128, 128, device="cuda"), torch.rand(B, device="cuda")
with torch.no_grad():
    plan = Plan.load(model.export_plan(pv, time=t))
lib, h, stream = plan._lib, plan._h, torch.cuda.current_stream().cuda_stream
arr = ctypes.cast((ctypes.c_int * 4)(*SLICES), ctypes.c_void_p)
# the reference's incompressible sets: the last output channel (the constant pressure plane) of every sample; and 30 % of the elements
channel = torch.zeros(B, 4, dtype=torch.uint8, device="cuda")
channel[:, 3] = 1
element = (torch.rand(B, 4, 128, 128, device="cuda") < 0.3).to(torch.uint8)
for K in [int(k) for k in args.steps.split(",")]:
    targets = torch.randn(K, B, 4, 128, 128, device="cuda")
    sums = torch.empty(K, B, 3, 4, dtype=torch.float64, device="cuda")

    def plain():
        rc = lib.scot_plan_evaluate(h, pv.data_ptr(), t.data_ptr(), targets.data_ptr(), K, arr, 3, sums.data_ptr(), None, stream)
        assert rc == 0, rc

    def masked(mask, full):
        rc = lib.scot_plan_evaluate_masked(h, pv.data_ptr(), t.data_ptr(), targets.data_ptr(), mask.data_ptr(), full, K, arr, 3, sums.data_ptr(),
                                           None, stream)
        assert rc == 0, rc
    cases = {"evaluate": plain}
    if not args.plain_only:
        cases["evaluate_masked_channel"] = lambda: masked(channel, 0)
        cases["evaluate_masked_element"] = lambda: masked(element, 1)
    times = {key: [] for key in cases}
    for _ in range(max(1, args.repeat)):
        for key, fn in cases.items():
            times[key].append(round(timed(fn), 3))
    res = dict(model="Poseidon-B", compute="fp16", batch=B, steps=K, calls=args.calls, warmup=args.warmup, root=os.path.abspath(args.root))
    res.update({f"{key}_ms": v for key, v in times.items()})
    if not args.plain_only:
        base = min(times["evaluate"])
        for key in ("evaluate_masked_channel", "evaluate_masked_element"):
            res[f"{key}_minus_evaluate_us_per_step"] = [round((v - base) / K * 1e3, 1) for v in times[key]]
        res["nonfinite_sums"] = int((~torch.isfinite(sums)).sum())
    res["GPU_MAX_HW_QUEUES"] = os.environ.get("GPU_MAX_HW_QUEUES")
    print(json.dumps(res), flush=True)
plan.free()
