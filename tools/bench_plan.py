"""ms per `scot_plan_run` (an exported plan, one stream, no Python between launches) against ms per `model(...)` (the engine's taped
inference forward: two streams, replayed from C behind a Python call) — Poseidon-B, fp16, batch 64 and batch 1, 20 timed calls after 5
warm-up calls.

usage: python tools/bench_plan.py [--batches 64,1] [--taped-only] [--root CHECKOUT] [--streams 1,2] [--repeat N]
  --taped-only   only the taped forward (what a checkout without the plan runtime can run)
  --streams      the plans to time: 1 = the one-stream plan (the default), 2 = the two-stream plan (`export_plan(..., streams=2)`: `plan2_ms`,
                 with the `describe_streams` overlap flag of its side stream); "1,2" times both in one process
  --repeat       time every case N times, the cases alternating (taped, plan, plan2, taped, ...): the values become lists
  --root         import the package from another checkout (the parent commit, built there) to time ITS taped forward in the same visit
Prints one JSON line per batch size.  Numbers: profiles/plan/README.md."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="64,1")
ap.add_argument("--taped-only", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--streams", default="1")
ap.add_argument("--repeat", type=int, default=1)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402
from poseidon_amd.config import preset  # noqa: E402
from scOT.model import ScOT  # noqa: E402


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.calls * 1e3


cfg = preset("B", image_size=128, num_channels=4, num_out_channels=4, channel_slice_list_normalized_loss=[0, 1, 3, 4])
torch.manual_seed(1234)
model = ScOT(cfg, compute="fp16").to("cuda").eval()
for B in [int(b) for b in args.batches.split(",")]:
    pv, t = torch.randn(B, 4, 128, 128, device="cuda"), torch.rand(B, device="cuda")
    res = dict(model="Poseidon-B", compute="fp16", batch=B, calls=args.calls, warmup=args.warmup, root=os.path.abspath(args.root))
    with torch.no_grad():
        plans = {}
        if not args.taped_only:
            from poseidon_amd.plan import Plan
            for n in [int(x) for x in args.streams.split(",")]:
                key = "plan" if n == 1 else f"plan{n}"
                t0 = time.perf_counter()
                image = model.export_plan(pv, time=t, **({} if n == 1 else dict(streams=n)))
                res[f"{key}_export_s"] = round(time.perf_counter() - t0, 2)
                res[f"{key}_image_MB"] = round(len(image) / 1e6, 1)
                plans[key] = Plan.load(image)
                del image
                if n > 1:
                    res[f"{key}_streams"] = plans[key].describe_streams()
        out = torch.empty(B, 4, 128, 128, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        cases = {"taped": lambda: model(pixel_values=pv, time=t)}
        cases.update({key: (lambda plan=plan: plan.run(pv, t, out=out, stream=stream)) for key, plan in plans.items()})
        times = {key: [] for key in cases}
        for _ in range(max(1, args.repeat)):
            for key, fn in cases.items():
                times[key].append(round(timed(fn), 3))
        res.update({f"{key}_ms": v[0] if args.repeat <= 1 else v for key, v in times.items()})
        ref = model(pixel_values=pv, time=t).output
        for key, plan in plans.items():
            plan.run(pv, t, out=out, stream=stream)
            res.update({f"{key}_device_MB": round(plan.info["device_bytes"] / 1e6, 1), f"{key}_calls_per_run": plan.info["calls"],
                        f"{key}_identical": bool(torch.equal(out, ref))})
            plan.free()
        res["GPU_MAX_HW_QUEUES"] = os.environ.get("GPU_MAX_HW_QUEUES")
    model._engine.reset_tapes()
    print(json.dumps(res), flush=True)
