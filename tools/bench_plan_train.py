"""ms per `scot_plan_train_step` (an exported training plan: one stream, the weight gradients in line, no Python between launches)
against ms per step of the Python loop — `opt.zero_grad(overlap=True)`, the taped step (two streams: the weight gradients hidden on the
second), `opt.step()` — Poseidon-B, fp16, batch 64 and batch 1, 20 timed steps after 5 warm-up steps.

usage: python tools/bench_plan_train.py [--batches 64,1] [--python-only] [--root CHECKOUT]
  --python-only  only the Python loop (what a checkout without training plans can run)
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
    plan = None
    if not args.python_only:      # (exported first: the image holds the weights the Python loop starts from, too)
        from poseidon_amd.plan import Plan
        t0 = time.perf_counter()
        image = model.export_plan(pv, time=t, labels=y, train=opt)
        res["export_s"] = round(time.perf_counter() - t0, 2)
        res["image_MB"] = round(len(image) / 1e6, 1)
        print(json.dumps(dict(batch=B, exported_MB=res["image_MB"], export_s=res["export_s"])), file=sys.stderr, flush=True)
        plan = Plan.load(image)
        del image

    def python_step():
        opt.zero_grad(overlap=True)
        model(pixel_values=pv, time=t, labels=y).loss.backward()
        opt.step()
    res["python_ms"] = round(timed(python_step), 3)
    res["python_skipped"] = opt.skipped_steps()
    if plan is not None:
        loss = torch.empty(1, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        res["plan_ms"] = round(timed(lambda: plan.train_step(pv, t, y, 5e-5, out=loss, stream=stream)), 3)
        st, tr = plan.train_status(), plan.describe_training()
        res.update(plan_device_MB=round(plan.info["device_bytes"] / 1e6, 1), calls_per_step=tr["step_calls"], kept_MB=round(tr["kept_bytes"] / 1e6, 1),
                   plan_applied=st["applied"], plan_skipped=st["skipped"], plan_loss=round(float(loss), 4))
        plan.free()
    model._engine.reset_tapes()
    del model, opt, plan
    torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
