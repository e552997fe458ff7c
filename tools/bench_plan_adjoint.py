"""ms per (forward + vjp) of the frozen surrogate — Poseidon-B, fp16, batch 64 and batch 1, 20 timed calls after 5 warm-up calls:
the Python frozen step (`model(...)` with inputs that require a gradient, every parameter frozen, then `torch.autograd.grad` from a
cotangent of the prediction: two streams; a call without labels is issued through the op wrappers, the step tape records labelled
steps only) against `scot_plan_run` + `scot_plan_vjp` of an adjoint
plan (one stream, no Python between launches).

usage: python tools/bench_plan_adjoint.py [--batches 64,1] [--python-only] [--root CHECKOUT] [--repeat N] [--rollout-steps N]
  --python-only  only the Python frozen step (what a checkout without adjoint plans can run)
  --root         import the package from another checkout (the parent commit, built there) to time ITS frozen step in the same visit
  --repeat       time the Python step N times (the spread of repeated runs is what two trees are compared against)
  --rollout-steps N  also time the adjoint of an N-step rollout of the same plan in the same process (`Plan.rollout_vjp`: N recomputed
                 forwards + N backwards, the forward rollout that produced the predictions not included), next to N x plan_ms
Prints one JSON line per batch size.  Numbers: profiles/plan_adjoint/README.md."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="64,1")
ap.add_argument("--python-only", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeat", type=int, default=1)
ap.add_argument("--rollout-steps", type=int, default=0)
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
for p in model.parameters():
    p.requires_grad_(False)
for B in [int(b) for b in args.batches.split(",")]:
    pv, t = torch.randn(B, 4, 128, 128, device="cuda"), torch.rand(B, device="cuda")
    g = torch.randn(B, 4, 128, 128, device="cuda") / (B * 4 * 128 * 128)
    a, b = pv.clone().requires_grad_(True), t.clone().requires_grad_(True)
    res = dict(model="Poseidon-B", compute="fp16", batch=B, calls=args.calls, warmup=args.warmup, root=os.path.abspath(args.root))

    def python_step():
        out = model(pixel_values=a, time=b).output
        return torch.autograd.grad(out, (a, b), grad_outputs=g)
    res["python_ms"] = [round(timed(python_step), 3) for _ in range(args.repeat)]
    if not args.python_only:
        from poseidon_amd.plan import Plan
        ref = python_step()
        t0 = time.perf_counter()
        image = model.export_plan(pv, time=t, adjoint=("pixel_values", "time"))
        res["export_s"] = round(time.perf_counter() - t0, 2)
        res["image_MB"] = round(len(image) / 1e6, 1)
        plan = Plan.load(image)
        del image
        out = torch.empty(B, 4, 128, 128, device="cuda")
        grads = (torch.empty_like(pv), torch.empty_like(t))
        stream = torch.cuda.current_stream().cuda_stream
        S = model._engine.grad_scale_value()

        def plan_step():
            plan.run(pv, t, out=out, stream=stream)
            plan.vjp(g, grad_scale=S, out=grads, stream=stream)
        res["plan_ms"] = round(timed(plan_step), 3)
        info = plan.describe_adjoint()
        res["plan_device_MB"] = round(plan.info["device_bytes"] / 1e6, 1)
        res["plan_kept_MB"] = round(info["kept_bytes"] / 1e6, 1)
        res["calls_per_run"], res["calls_per_vjp"] = plan.info["calls"], info["backward_calls"]
        res["identical"] = bool(torch.equal(grads[0], ref[0]) and torch.equal(grads[1], ref[1]))
        if args.rollout_steps > 0:
            N = args.rollout_steps
            preds = torch.empty(N, B, 4, 128, 128, device="cuda")      # the C layout, as scot_plan_rollout writes it
            plan.rollout(pv.data_ptr(), t.data_ptr(), N, out=preds.data_ptr(), stream=stream)
            gs = (torch.randn(N, B, 4, 128, 128, device="cuda") / (B * 4 * 128 * 128)).contiguous()

            def rollout_vjp():
                plan.rollout_vjp(pv.data_ptr(), t.data_ptr(), preds.data_ptr(), gs.data_ptr(), grad_scale=S, out=grads, steps=N, stream=stream)
            res["rollout_steps"] = N
            res["rollout_vjp_ms"] = round(timed(rollout_vjp), 3)
            res["steps_x_plan_ms"] = round(N * res["plan_ms"], 3)
            res["rollout_vjp_over_steps_x_plan"] = round(res["rollout_vjp_ms"] / res["steps_x_plan_ms"], 4)
            res["rollout_finite"] = bool(torch.isfinite(grads[0]).all() and torch.isfinite(grads[1]).all())
        res["nonfinite_counted"] = plan.grad_status()[0]
        plan.free()
    model._engine.reset_tapes()
    print(json.dumps(res), flush=True)
