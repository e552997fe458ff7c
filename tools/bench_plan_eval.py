"""ms per call of an exported plan's evaluation (`scot_plan_evaluate`: a rollout that leaves only error sums behind) against the rollout
alone (`scot_plan_rollout`) and against the torch-op path that existed before (the rollout followed by `scOT.metrics.channel_group_metrics`
on the device, once per step), and the `scot_error_sums` kernel alone — Poseidon-B, fp16, 128 x 128, batch 64 and batch 1, 8 steps.

usage: python tools/bench_plan_eval.py [--batches 64,1] [--steps 8] [--rollout-only | --kernel-only] [--root CHECKOUT] [--repeat N]
                                       [--kernel-launches 200]
  --rollout-only  only `scot_plan_rollout` (what a checkout without the evaluation call can run)
  --kernel-only   only the `scot_error_sums` kernel alone
  --root          import the package from another checkout (the parent commit, built there) to time ITS rollout in the same visit
  --repeat        time every case N times, the cases alternating: the values become lists
Prints one JSON line per batch size and one for the kernel.  Numbers: profiles/plan_eval/README.md."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="64,1")
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--rollout-only", action="store_true")
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--repeat", type=int, default=2)
ap.add_argument("--kernel-launches", type=int, default=200)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402
from poseidon_amd.config import preset  # noqa: E402
from poseidon_amd.plan import Plan  # noqa: E402
from scOT.model import ScOT  # noqa: E402

SLICES = [0, 1, 3, 4]
HBM_COPY_TBPS = 6.29      # the measured copy rate the kernel's floor is quoted against


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
model = None if args.kernel_only else ScOT(cfg, compute="fp16").to("cuda").eval()
K = args.steps
for B in ([] if args.kernel_only else [int(b) for b in args.batches.split(",")]):
    pv, t = torch.randn(B, 4, 128, 128, device="cuda"), torch.rand(B, device="cuda")
    res = dict(model="Poseidon-B", compute="fp16", batch=B, steps=K, calls=args.calls, warmup=args.warmup, root=os.path.abspath(args.root))
    with torch.no_grad():
        plan = Plan.load(model.export_plan(pv, time=t))
        stream = torch.cuda.current_stream().cuda_stream
        out = torch.empty(K, B, 4, 128, 128, device="cuda")            # the C layout: no transpose in the timed region
        targets = torch.randn(K, B, 4, 128, 128, device="cuda")
        cases = {"rollout": lambda: plan.rollout(pv.data_ptr(), t.data_ptr(), K, out=out.data_ptr(), stream=stream)}
        if not args.rollout_only:
            from scOT import metrics as M
            lib, h = plan._lib, plan._h
            import ctypes
            arr = ctypes.cast((ctypes.c_int * 4)(*SLICES), ctypes.c_void_p)
            sums = torch.empty(K, B, 3, 4, dtype=torch.float64, device="cuda")

            def evaluate(predictions):
                rc = lib.scot_plan_evaluate(h, pv.data_ptr(), t.data_ptr(), targets.data_ptr(), K, arr, 3, sums.data_ptr(), predictions, stream)
                assert rc == 0, rc

            def torch_metrics():
                plan.rollout(pv.data_ptr(), t.data_ptr(), K, out=out.data_ptr(), stream=stream)
                return [M.channel_group_metrics(out[k], targets[k], SLICES) for k in range(K)]

            def evaluate_and_statistics():
                evaluate(None)
                return [M.group_metrics_from_sums(sums[k]) for k in range(K)]
            cases["evaluate_with_predictions"] = lambda: evaluate(out.data_ptr())
            cases["evaluate"] = lambda: evaluate(None)
            cases["rollout_then_torch_metrics"] = torch_metrics
            cases["evaluate_then_statistics"] = evaluate_and_statistics
        times = {key: [] for key in cases}
        for _ in range(max(1, args.repeat)):
            for key, fn in cases.items():
                times[key].append(round(timed(fn), 3))
        res.update({f"{key}_ms": v for key, v in times.items()})
        if not args.rollout_only:
            base = min(times["rollout"])
            res["evaluate_minus_rollout_us_per_step"] = [round((v - base) / K * 1e3, 1) for v in times["evaluate"]]
            res["evaluate_with_predictions_minus_rollout_us_per_step"] = [round((v - base) / K * 1e3, 1) for v in times["evaluate_with_predictions"]]
            # the two paths agree: the same keys, the same numbers (the torch path sums in fp32)
            import math
            worst = (0.0, None, None, None)
            for k, (a, b) in enumerate(zip(torch_metrics(), evaluate_and_statistics())):
                assert set(a) == set(b)
                for key in a:
                    both_nan = math.isnan(a[key]) and math.isnan(b[key])
                    gap = 0.0 if both_nan or a[key] == b[key] else abs(a[key] - b[key]) / max(abs(a[key]), 1e-300)
                    if not gap <= worst[0]:
                        worst = (gap, f"step {k} {key}", a[key], b[key])
            res["paths_worst_relative_gap"] = worst
            res["nonfinite_predictions"] = int((~torch.isfinite(out)).sum())
        res["device_MB"] = round(plan.describe()["device_bytes"] / 1e6, 1)
        res["GPU_MAX_HW_QUEUES"] = os.environ.get("GPU_MAX_HW_QUEUES")
        plan.free()
    print(json.dumps(res), flush=True)

if not args.rollout_only:
    # the kernel alone at [64, 4, 128 * 128]: device-event time over back-to-back launches (two launches per call: chunks, then the ordered finish)
    from poseidon_amd import ops
    B, C, HW = 64, 4, 128 * 128
    # ten operand pairs in rotation, 335 MB: more than the 256 MB last-level cache holds, so every launch reads HBM ("cold"); and one pair
    # over and over, 33.5 MB, which that cache can serve ("warm")
    pairs = [(torch.randn(B, C, HW, device="cuda"), torch.randn(B, C, HW, device="cuda")) for _ in range(10)]
    sums = torch.empty(B, 3, 4, dtype=torch.float64, device="cuda")
    # (the launches are queued behind three large matrix products, so that the events bracket kernels the device already holds, not the
    # pace at which Python issues them; both events lie BETWEEN launches of the kernel itself, 50 launches behind the products: an event
    # recorded straight behind another kind of work was seen to take that work's start for its time)
    blocker = torch.randn(8192, 8192, device="cuda")
    runs = {"cold": [], "warm": []}
    for _ in range(max(1, args.repeat)):
        for mode in runs:
            use = pairs if mode == "cold" else pairs[:1]
            for i in range(20):
                ops.error_sums(*use[i % len(use)], SLICES, sums)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            for _ in range(3):
                blocker @ blocker
            for i in range(50):
                ops.error_sums(*use[i % len(use)], SLICES, sums)
            e0.record()
            for i in range(args.kernel_launches):
                ops.error_sums(*use[i % len(use)], SLICES, sums)
            e1.record()
            torch.cuda.synchronize()
            runs[mode].append(round(e0.elapsed_time(e1) / args.kernel_launches * 1e3, 2))
    read_bytes = 2 * B * C * HW * 4
    floor_us = read_bytes / (HBM_COPY_TBPS * 1e12) * 1e6
    print(json.dumps(dict(kernel="scot_error_sums", shape=[B, C, HW], slices=SLICES, launches=args.kernel_launches, us_per_call_cold=runs["cold"],
                          us_per_call_warm=runs["warm"], read_MB=round(read_bytes / 1e6, 1), hbm_floor_us=round(floor_us, 2),
                          share_of_hbm_bound_cold=[round(floor_us / r, 3) for r in runs["cold"]])), flush=True)
