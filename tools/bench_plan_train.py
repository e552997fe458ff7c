"""ms per `scot_plan_train_step` (an exported training plan: one stream, the weight gradients in line, no Python between launches)
against ms per step of the Python loop — `opt.zero_grad(overlap=True)`, the taped step (two streams: the weight gradients hidden on the
second), `opt.step()` — Poseidon-B, fp16, batch 64 and batch 1, 20 timed steps after 5 warm-up steps.

usage: python tools/bench_plan_train.py [--batches 64,1] [--python-only] [--root CHECKOUT] [--streams 1,2] [--repeat N]
  --python-only  only the Python loop (what a checkout without training plans can run)
  --streams      the plans to time: 1 = the one-stream plan (the default), 2 = the two-stream plan (`export_plan(..., streams=2)`: `plan2_ms`,
                 with the `describe_streams` overlap flag of its side stream); "1,2" times both in one process
  --repeat       time every case N times, the cases alternating (python, plan, plan2, python, ...): the values become lists
  --root         import the package from another checkout (the parent commit, built there) to time ITS Python loop in the same process environment
Prints one JSON line per batch size.  Numbers: profiles/plan_train/README.md."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="64,1")
ap.add_argument("--python-only", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--streams", default="1")
ap.add_argument("--repeat", type=int, default=1)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402
from poseidon_amd.config import preset  # noqa: E402
from poseidon_amd.optim import FusedAdamW  # noqa: E402
from scOT.model import ScOT  # noqa: E402


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.steps * 1e3


cfg = preset("B", image_size=128, num_channels=4, num_out_channels=4, channel_slice_list_normalized_loss=[0, 1, 3, 4])
for B in [int(b) for b in args.batches.split(",")]:
    torch.manual_seed(1234)
    model = ScOT(cfg, compute="fp16").to("cuda").train()
    opt = FusedAdamW(model, lr=5e-5, weight_decay=0.01, max_grad_norm=5.0)
    pv, t, y = torch.randn(B, 4, 128, 128, device="cuda"), torch.rand(B, device="cuda"), torch.randn(B, 4, 128, 128, device="cuda")
    res = dict(model="Poseidon-B", compute="fp16", batch=B, steps=args.steps, warmup=args.warmup, root=os.path.abspath(args.root),
               parameter_MB=round(model._arena.size * 4 / 1e6, 1))
    plans = {}
    if not args.python_only:      # (exported first: the image holds the weights the Python loop starts from, too)
        from poseidon_amd.plan import Plan
        for n in [int(x) for x in args.streams.split(",")]:
            key = "plan" if n == 1 else f"plan{n}"
            t0 = time.perf_counter()
            image = model.export_plan(pv, time=t, labels=y, train=opt, **({} if n == 1 else dict(streams=n)))
            res[f"{key}_export_s"] = round(time.perf_counter() - t0, 2)
            res[f"{key}_image_MB"] = round(len(image) / 1e6, 1)
            print(json.dumps(dict(batch=B, streams=n, exported_MB=res[f"{key}_image_MB"], export_s=res[f"{key}_export_s"])), file=sys.stderr, flush=True)
            plans[key] = Plan.load(image)
            del image
            if n > 1:
                res[f"{key}_streams"] = plans[key].describe_streams()

    def python_step():
        opt.zero_grad(overlap=True)
        model(pixel_values=pv, time=t, labels=y).loss.backward()
        opt.step()
    loss = torch.empty(1, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    cases = {"python": python_step}
    cases.update({key: (lambda plan=plan: plan.train_step(pv, t, y, 5e-5, out=loss, stream=stream)) for key, plan in plans.items()})
    times = {key: [] for key in cases}
    for _ in range(max(1, args.repeat)):
        for key, fn in cases.items():
            times[key].append(round(timed(fn), 3))
    res.update({f"{key}_ms": v[0] if args.repeat <= 1 else v for key, v in times.items()})
    res["python_skipped"] = opt.skipped_steps()
    for key, plan in plans.items():
        st, tr = plan.train_status(), plan.describe_training()
        res.update({f"{key}_device_MB": round(plan.info["device_bytes"] / 1e6, 1), f"{key}_calls_per_step": tr["step_calls"],
                    f"{key}_kept_MB": round(tr["kept_bytes"] / 1e6, 1), f"{key}_applied": st["applied"], f"{key}_skipped": st["skipped"]})
        plan.free()
    res["GPU_MAX_HW_QUEUES"] = os.environ.get("GPU_MAX_HW_QUEUES")
    model._engine.reset_tapes()
    del model, opt, plans, cases
    torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
