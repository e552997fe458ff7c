"""ms per `scot_plan_run` (an exported plan, one stream, no Python between launches) against ms per `model(...)` (the engine's taped
inference forward: two streams, replayed from C behind a Python call) — Poseidon-B, fp16, batch 64 and batch 1, 20 timed calls after 5
warm-up calls.

usage: python tools/bench_plan.py [--batches 64,1] [--taped-only] [--root CHECKOUT]
  --taped-only   only the taped forward (what a checkout without the plan runtime can run)
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
        res["taped_ms"] = round(timed(lambda: model(pixel_values=pv, time=t)), 3)
        if not args.taped_only:
            from poseidon_amd.plan import Plan
            t0 = time.perf_counter()
            image = model.export_plan(pv, time=t)
            res["export_s"] = round(time.perf_counter() - t0, 2)
            res["image_MB"] = round(len(image) / 1e6, 1)
            plan = Plan.load(image)
            del image
            out = torch.empty(B, 4, 128, 128, device="cuda")
            stream = torch.cuda.current_stream().cuda_stream
            res["plan_ms"] = round(timed(lambda: plan.run(pv, t, out=out, stream=stream)), 3)
            res["plan_device_MB"] = round(plan.info["device_bytes"] / 1e6, 1)
            res["calls_per_run"] = plan.info["calls"]
            res["identical"] = bool(torch.equal(out, model(pixel_values=pv, time=t).output))
            plan.free()
    model._engine.reset_tapes()
    print(json.dumps(res), flush=True)
