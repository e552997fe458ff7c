"""Gradient accumulation in training plans, measured with device events — Poseidon-B, fp16, 128 x 128.

  kernel   scot_grad_accumulate alone over Poseidon-B's parameter arena with the optimizer's own group map, its three forms:
           first (dst = w g: 8 bytes per float), add (dst = acc + w g in place: 12), copy (dst = 1 g: 8) — us per launch, TB/s and the
           share of the 6.29 TB/s a float4 copy reaches on this chip.
  plan     one effective batch of `--micro` recorded batches at batch `--batch`: `--micro` x scot_plan_train_step against `--micro` x
           scot_plan_accumulate + scot_plan_apply, on a one-stream and a two-stream plan — ms per effective batch.
  against  `plan` in child processes that alternate between this checkout and `--against CHECKOUT` (the parent commit, built there;
           it times train_step alone): the parent's own run-to-run spread and both differences come out of one visit.

usage: python tools/bench_plan_accumulate.py kernel | plan [--steps-only] | against --against CHECKOUT [--rounds 2]
       [--batch 64] [--micro 4] [--streams 1,2] [--repeat 7] [--warmup 2] [--root CHECKOUT]
Every figure is the median of `--repeat` (>= 5) timed repeats after `--warmup` untimed ones, with the spread (max - min) beside it.
Prints JSON lines.  Numbers: profiles/plan_accumulate/README.md."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["kernel", "plan", "against"])
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--micro", type=int, default=4)
ap.add_argument("--streams", default="1,2")
ap.add_argument("--repeat", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--root", default=HERE)
ap.add_argument("--steps-only", action="store_true")
ap.add_argument("--against")
ap.add_argument("--rounds", type=int, default=2)
args = ap.parse_args()
args.repeat = max(5, args.repeat)
ROOF_TBS = 6.29      # float4 copy, measured on the MI355X


def summary(values):
    return dict(median=round(statistics.median(values), 4), spread=round(max(values) - min(values), 4), n=len(values))


if args.mode == "against":
    # children alternate: parent, this checkout, parent, ... — each exports its own plans and prints one JSON line per stream count
    if not args.against:
        ap.error("against: --against CHECKOUT")
    rows = {}
    for r in range(args.rounds):
        for who, root in (("parent", os.path.abspath(args.against)), ("this", HERE)):
            cmd = [sys.executable, os.path.abspath(__file__), "plan", "--root", root, "--batch", str(args.batch), "--micro", str(args.micro),
                   "--streams", args.streams, "--repeat", str(args.repeat), "--warmup", str(args.warmup)] + (["--steps-only"] if who == "parent" else [])
            out = subprocess.run(["timeout", "-k", "10", "420"] + cmd, capture_output=True, text=True)
            if out.returncode != 0:
                sys.exit(f"{who} (round {r}) ended with status {out.returncode}:\n{out.stderr[-3000:]}")      # nothing more runs after a failure
            for line in out.stdout.splitlines():
                if line.startswith("{"):
                    d = json.loads(line)
                    for key in ("steps_ms", "accumulate_apply_ms"):
                        if key in d:
                            rows.setdefault((d["streams"], who, key), []).extend(d[key])
    for s in sorted({k[0] for k in rows}):
        parent, steps, accum = (rows[(s, who, key)] for who, key in (("parent", "steps_ms"), ("this", "steps_ms"), ("this", "accumulate_apply_ms")))
        res = dict(streams=s, batch=args.batch, micro=args.micro, rounds=args.rounds, parent_steps_ms=summary(parent), steps_ms=summary(steps),
                   accumulate_apply_ms=summary(accum))
        res["steps_minus_parent_ms"] = round(res["steps_ms"]["median"] - res["parent_steps_ms"]["median"], 4)
        res["accumulate_apply_minus_parent_ms"] = round(res["accumulate_apply_ms"]["median"] - res["parent_steps_ms"]["median"], 4)
        print(json.dumps(res), flush=True)
    sys.exit(0)

sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
from poseidon_amd.config import preset  # noqa: E402
from poseidon_amd.plan import Plan  # noqa: E402
from scOT.model import ScOT  # noqa: E402
from scOT.trainer import FusedAdamW  # noqa: E402


def timed(fn):
    """ms of fn() between two device events: args.repeat values after args.warmup untimed calls"""
    for _ in range(args.warmup):
        fn()
    out = []
    for _ in range(args.repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


cfg = preset("B", image_size=128, num_channels=4, num_out_channels=4, channel_slice_list_normalized_loss=[0, 1, 3, 4])
torch.manual_seed(1234)
model = ScOT(cfg, compute="fp16").to("cuda").train()
opt = FusedAdamW(model, lr=5e-5, weight_decay=0.01, max_grad_norm=5.0)

if args.mode == "kernel":
    from poseidon_amd import ops
    n = model._arena.size
    params = int((opt._map != 255).sum()) * 8
    grad, acc = torch.randn(n, device="cuda"), torch.randn(n, device="cuda")
    forms = {"first": (lambda: ops.grad_accumulate(acc, None, grad, opt._map, 0.25), 8), "add": (lambda: ops.grad_accumulate(acc, acc, grad, opt._map, 0.25), 12),
             "copy": (lambda: ops.grad_accumulate(acc, None, grad, opt._map, 1.0), 8)}
    times = {key: timed(fn) for key, (fn, _) in forms.items()}
    res = dict(kernel="scot_grad_accumulate", arena_floats=n, parameter_floats=params, roof_tbs=ROOF_TBS)
    for key, (_, bytes_per_float) in forms.items():
        ms = summary(times[key])
        tbs = bytes_per_float * params / (ms["median"] * 1e-3) / 1e12
        res[key] = dict(us=round(ms["median"] * 1e3, 1), spread_us=round(ms["spread"] * 1e3, 1), n=ms["n"], bytes=bytes_per_float * params,
                        tbs=round(tbs, 3), share_of_roof=round(tbs / ROOF_TBS, 3))
    print(json.dumps(res), flush=True)
    sys.exit(0)

B, M = args.batch, args.micro
pv, t, y = torch.randn(B, 4, 128, 128, device="cuda"), torch.rand(B, device="cuda"), torch.randn(B, 4, 128, 128, device="cuda")
for streams in [int(s) for s in args.streams.split(",")]:
    plan = Plan.load(model.export_plan(pv, time=t, labels=y, train=opt, streams=streams))

    def steps():
        for _ in range(M):
            plan.train_step(pv, t, y, 5e-5)

    def accumulate_apply():
        for k in range(M):
            plan.accumulate(pv, t, y, 1.0 / M, k == 0)
        plan.apply(5e-5)
    res = dict(model="Poseidon-B", compute="fp16", batch=B, micro=M, streams=streams, root=os.path.abspath(args.root),
               overlaps=plan.describe_streams()["overlaps"], steps_ms=[round(v, 4) for v in timed(steps)])
    if not args.steps_only:
        res["accumulate_apply_ms"] = [round(v, 4) for v in timed(accumulate_apply)]
    st = plan.train_status()
    res.update(applied=st["applied"], skipped=st["skipped"], GPU_MAX_HW_QUEUES=os.environ.get("GPU_MAX_HW_QUEUES"))
    for key in ("steps_ms", "accumulate_apply_ms"):
        if key in res:
            res[key + "_summary"] = summary(res[key])
    print(json.dumps(res), flush=True)
    plan.free()
