#!/usr/bin/env python
"""bench.py — PDE-grid samples/s (forward + backward, loss included, optimizer excluded) of the scOT hot path.

  python bench.py --gpus N --steps K --warmup W [--full]          (N>1: launched by torch.distributed.run, one rank per GPU)

Workload (BASELINE.json metric / configs[2]): Poseidon-B, per-GPU batch 64, 128x128x4 synthetic CE-RP-shaped grids
(N(0,1) channels, all active, groups [0,1,3,4]), 16-bit MFMA compute with fp32 accumulation, weak scaling (per-device batch
fixed, as reference train.py:281).  Default --compute fp16: the fastest mode whose ScOT.forward output stays within the north
star's 1e-3 rel-L2 of the real reference on trained-like parameters — with --full, checked IN THIS PROCESS against the committed golden
fixture before anything is timed (config.parity); bf16 operands (--compute bf16) do not meet it (6e-3).  A "step" = zero the gradient arena + ScOT.forward (incl. grouped relative-L1 loss) + backward into the
arena (+ mean all-reduce of the arena for N>1).  Inputs are resident in HBM before the timed region.
A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line.  --full adds everything else: the parity and
batch-consistency checks, the per-launch table behind `roofline`'s kernel families, the forward / backward split, the weight-refresh
time, the exposed and GPU time of the gradient exchange (N>1), BASELINE.json's other configurations and the CPU baseline.
Prints ONE JSON line (rank 0).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# forward GFLOP/sample F (excl. CPB) and batch-independent CPB GFLOP/step P; fwd+bwd = 3(B·F + P)
FLOPS = {"T": (2.784, 0.139), "B": (18.286, 0.277), "L": (67.948, 0.277)}
FLOPS_AT = {("B", 256): (74.502, 0.521)}      # Poseidon-B at 256 x 256 (not 4x the 128 x 128 figure: windows / shifts differ)
# BASELINE.json configs 2, 5, 4 (config 3 is the headline; config 1 is the CPU plumbing case inside cpu_baseline): (model, per-GPU batch, size, channels)
OTHER_CONFIGS = [("T", 32, 128, 4), ("B", 32, 256, 4), ("L", 128, 128, 5)]
PEAK_TFLOPS = {"fp16": 2500.0, "bf16": 2500.0, "fp32": 157.3, "bf16x3": 2500.0 / 3}   # bf16x3 = three bf16 MFMAs per product  # dense MFMA peaks, /opt/skills/guides/MI355X_MICROARCH.md


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", default="B", choices=["T", "B", "L"])
    ap.add_argument("--batch", type=int, default=64, help="per-GPU batch")
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--channels", type=int, default=4)
    ap.add_argument("--compute", default="fp16", choices=["fp16", "bf16", "fp32", "bf16x3"])
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: the parity and consistency checks, the per-launch table and "
                         "per-kernel roofline, the phase split, the weight-refresh and gradient-exchange timings, the other configurations "
                         "and the CPU baseline (the --no-* switches below leave parts of it out)")
    ap.add_argument("--no-parity", action="store_true", help="--full: skip the in-process parity check against the golden fixture")
    ap.add_argument("--no-graph", action="store_true", help="eager launches of the recorded step (the default; overrides --graph)")
    ap.add_argument("--graph", action="store_true",
                    help="time hipGraph replay of the step instead of eager launches (slower on MI355X: 32.9 vs 18.3 ms for the default "
                         "workload: the two-stream fork / join is serialised; a process capturing the two-stream step under a 2-hardware-queue "
                         "runtime has died with no error)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline (`cpu_baseline`)")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="--full: skip the short runs of BASELINE.json's configs 2, 4 and 5 that it appends to the single-GPU headline run (`other_configs`)")
    ap.add_argument("--rccl-channels", type=int, default=0,
                    help="N>1: cap RCCL at this many channels (NCCL_MAX_NCHANNELS, set before the process group exists): every channel is a "
                         "workgroup the collectives take from a backward that is throughput-bound on both of its streams; 0 = RCCL's choice")
    ap.add_argument("--cpu-seconds", type=float, default=20.0)
    ap.add_argument("--wire", default="fp32", choices=["bf16", "fp32"], help="gradient all-reduce wire format (N>1)")
    ap.add_argument("--dp-collective", default="allreduce", choices=["allreduce", "rs_ag"],
                    help="N>1: one all-reduce per gradient chunk, or reduce-scatter + all-gather (poseidon_amd/dp.py)")
    ap.add_argument("--dp-backend", default="torch", choices=["torch", "native"],
                    help="N>1: the collectives of the torch process group (default), or the C ABI's own RCCL communicator "
                         "(scot_dp_init / scot_dp_allreduce_bucket, include/scot_hip.h; all-reduce only)")
    ap.add_argument("--dp", default="auto", choices=["auto", "overlap", "after", "none"],
                    help="N>1: all-reduce each gradient range from inside the backward as soon as it is final (RCCL on a side "
                         "stream, eager launches), or one chunked all-reduce after the step (works with hipGraph replay); "
                         "auto: time both in the warm-up, keep the faster; none: no exchange (diagnostic: what the process group costs)")
    ap.add_argument("--launch-dump", default=None, help="--full: write every launch of the per-launch-timed steps (entry point, integer "
                                                        "arguments, stream, start/end in ms since the step's first launch) to this JSON file")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step computed (rank 0) to DIR/<name>.npy: the prediction, the "
                         "loss, per-parameter gradient norms and a fixed, seeded sample of the gradients (float32 / float64, <= 64 MB in all)")
    ap.add_argument("--_cpu-worker", dest="cpu_worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--_emu", dest="emu", action="store_true", help=argparse.SUPPRESS)      # tests/test_bench_flow_cpu.py (see _enter_emulation)
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if a.launch_dump and not a.full:
        ap.error("--launch-dump needs --full (the per-launch table is one of its runs)")
    return a


def usable_cores(cap=32):
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:  # cgroup v2 CPU quota
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(int(q) / int(per))))
    except Exception:
        pass
    return max(1, min(n, cap))


def cpu_baseline(model_tag, size, channels, budget_s):
    """Runs `_cpu_baseline_worker` in a child process with a hard wall-clock limit (a thread-oversubscribed host must
    not be able to stall the GPU measurement)."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--_cpu-worker", "--model", model_tag, "--size", str(size),
           "--channels", str(channels), "--cpu-seconds", str(budget_s)]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=budget_s * 4 + 60)
        for line in reversed(out.stdout.strip().splitlines()):
            if line.startswith("{"):
                return json.loads(line)
        return {"error": "no result", "stderr": out.stderr[-300:]}
    except subprocess.TimeoutExpired:
        return {"error": f"cpu baseline exceeded {budget_s * 4 + 60:.0f}s"}


def _cpu_baseline_worker(model_tag, size, channels, budget_s):
    """Oracle (CPU restatement, torch CPU ops, fp32) timed on this host's cores: fwd+bwd, small batch, bounded time."""
    from oracle import scot_cpu
    from poseidon_amd.config import preset
    from poseidon_amd.geometry import param_shapes
    cores = usable_cores()
    torch.set_num_threads(cores)
    groups = [0, 1, channels - 1, channels]
    cfg = preset(model_tag, image_size=size, num_channels=channels, num_out_channels=channels,
                 channel_slice_list_normalized_loss=groups)
    g = torch.Generator().manual_seed(0)
    sd = {}
    for k, shp in param_shapes(cfg).items():
        t = torch.randn(*shp, generator=g) * 0.02
        if k.endswith("logit_scale"):
            t = torch.full(shp, 2.3026)
        sd[k] = t.requires_grad_(True)
    bs = 2
    pv, lab, tt = torch.randn(bs, channels, size, size, generator=g), torch.randn(bs, channels, size, size, generator=g), torch.rand(bs, generator=g)

    def step():
        for v in sd.values():
            v.grad = None
        loss, _ = scot_cpu.scot_forward(sd, cfg, pv, tt, lab)
        loss.backward()
    step()  # warm-up
    times, t_start = [], time.time()
    while len(times) < 2 or (time.time() - t_start < budget_s and len(times) < 10):
        t0 = time.time()
        step()
        times.append(time.time() - t0)
    times.sort()
    med = times[len(times) // 2]
    # ... and on ONE core: the same step on one sample, one torch thread, best of two
    one = None
    if cores > 1:
        torch.set_num_threads(1)
        pv, lab, tt = pv[:1], lab[:1], tt[:1]
        t1 = []
        for _ in range(2):
            t0 = time.time()
            step()
            t1.append(time.time() - t0)
        one = 1.0 / min(t1)
    # the same model at batch 8 (one step, when the budget allows) and BASELINE config 1 (Poseidon-T, batch 2, forward only)
    torch.set_num_threads(cores)
    b8 = None
    if med * 4 < max(budget_s, 20.0):
        pv, lab, tt = torch.randn(8, channels, size, size, generator=g), torch.randn(8, channels, size, size, generator=g), torch.rand(8, generator=g)
        t0 = time.time()
        step()
        b8 = 8 / (time.time() - t0)
    cfg1 = preset("T", image_size=128, num_channels=4, num_out_channels=4, channel_slice_list_normalized_loss=[0, 1, 3, 4])
    sd1 = {}
    for k, shp in param_shapes(cfg1).items():
        sd1[k] = torch.full(shp, 2.3026) if k.endswith("logit_scale") else torch.randn(*shp, generator=g) * 0.02
    pv1, tt1 = torch.randn(2, 4, 128, 128, generator=g), torch.rand(2, generator=g)
    t1 = []
    with torch.no_grad():
        for _ in range(3):
            t0 = time.time()
            scot_cpu.scot_forward(sd1, cfg1, pv1, tt1, None)
            t1.append(time.time() - t0)
    cfg1_fwd = 2 / min(t1[1:])
    return {"value": bs / med, "unit": "samples/s", "cores": cores, "kind": "port",
            "pinned_by": "tests/test_oracle_golden.py (oracle/scot_cpu.py against tests/golden/*.npz: outputs, losses and gradients produced by "
                         "importing the real reference, tests/golden/make_*.py)",
            "batch8_value": b8, "batch8_sample": f"one fwd+bwd step of the same model at batch 8, {cores} torch threads",
            "config1_forward_only_value": cfg1_fwd,
            "config1_sample": f"BASELINE config 1: Poseidon-T, batch 2, 128x128x4, fp32 forward only, best of 2, {cores} torch threads",
            "sample": f"oracle/scot_cpu.py fp32 fwd+bwd, Poseidon-{model_tag} batch {bs} {size}x{size}x{channels}, "
                      f"median of {len(times)} steps, {cores} torch threads",
            "one_core_value": one, "one_core_sample": "the same step on batch 1 with one torch thread, best of 2"}


def parity_check(model_tag, compute, size, channels):
    """Output of the mode about to be timed against the golden vector of the REAL reference (tests/golden/poseidon<X>_trained.npz:
    produced by tests/golden/make_fixtures.py importing /root/reference; trained-like parameter statistics, the hard regime for
    16-bit operands) — same closed-form parameters and inputs, forward + loss on this GPU.  Fixtures are data; nothing under
    oracle/ is touched."""
    import numpy as np
    from poseidon_amd.config import ScOTConfig
    from poseidon_amd.geometry import param_shapes
    from poseidon_amd.synth import synth_inputs, synth_state_dict
    from scOT.model import ScOT
    name = f"poseidon{model_tag}{size if size != 128 else ''}_trained"      # (poseidonB256_trained: BASELINE config 5)
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    if not os.path.exists(path):
        return {"fixture": None, "note": f"no golden fixture for Poseidon-{model_tag}"}
    f = np.load(path)
    meta = json.loads(bytes(f["__meta__"]).decode())
    cfg = ScOTConfig(**meta["cfg"])
    if cfg.image_size != size:
        return {"fixture": None, "note": f"golden fixture is at {cfg.image_size}x{cfg.image_size}"}
    with torch.device("cuda"):
        # the fixture is a batch of 1-2: `fused_min_rows=0` makes it run the kernels the TIMED batch selects (the fused layer tails, which the
        # engine's policy leaves to batches of >= 4096 token rows), so that what is checked against the reference is what is timed
        model = ScOT(cfg, compute=compute, engine_options={"fused_min_rows": 0})
    model.load_state_dict(synth_state_dict(param_shapes(cfg), meta["regime"]))
    pv, t, lab = synth_inputs(meta["batch"], cfg.num_channels, cfg.num_out_channels, cfg.image_size, meta["kind"])
    with torch.no_grad():
        out = model(pixel_values=pv.cuda(), time=t.cuda(), labels=lab.cuda())
    ref = f["output"].astype(np.float64)
    got = out.output.double().cpu().numpy()
    rel = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    lrel = abs(float(out.loss) - float(f["loss"])) / abs(float(f["loss"]))
    del model
    torch.cuda.empty_cache()
    return {"fixture": f"tests/golden/{name}.npz (outputs of the real reference on {'trained-like (closed-form, poseidon_amd/synth.py)' if meta['regime'] == 'trained' else meta['regime']} parameters, batch {meta['batch']})",
            "output_rel_l2": rel, "loss_rel": lrel, "bound": 1e-5 if compute == "fp32" else 1e-3, "meets_bound": rel < (1e-5 + 5e-6 if compute == "fp32" else 1e-3)}


def step_flops(model_tag, size, batch):
    """algorithmic TFLOP of one forward + backward step per GPU: 3 (B F + P), SURVEY.md 8(d)"""
    F, P = FLOPS_AT.get((model_tag, size)) or (FLOPS[model_tag][0] * (size / 128.0) ** 2, FLOPS[model_tag][1])
    return 3.0 * (batch * F + P) / 1e3


def attainable_model(cfg, batch):
    """What THIS decomposition (one launch per Linear / norm / attention core at C >= 384, one fused tail + one attention launch per direction at
    C = 96 / 192, weight gradients beside the chain) could reach if every kernel sat on its own roof: per stage the maximum of
      mfma   algorithmic FLOPs / 2.5 PF                                   (2 M 12 C^2 + 4 M Nw C per layer forward, x 3 for fwd + bwd)
      hbm    bytes the layout moves / 6.3 TB/s                            (110 C B/token/layer fused, 270 C unfused + 28 C^2 B of weights / gradients)
      floor  dependent launches x 1.5 us boundary + GEMM K loops          (64 x 64 tile, 16 KB per 64-deep K step at ~50 GB/s per CU = 0.33 us, + 3 us ramp)
    summed over the stages (+ 0.6 ms of trunk / skip / head launches that overlap nothing).  The constants are measured ones: profiles/round6/attainable.md."""
    from poseidon_amd.geometry import stage_plan
    _, enc, dec = stage_plan(cfg)
    stages, total = [], 0.0
    for st in enc + dec:
        C, M, nl = st.dim, batch * st.res[0] * st.res[1], len(st.blocks)
        ws = st.blocks[0].window_shift()[0]
        fused = C in (96, 192)
        flops = 3.0 * nl * (2.0 * M * 12 * C * C + 4.0 * M * ws * ws * C)
        mfma = flops / 2.5e15 * 1e3
        hbm = nl * ((110 if fused else 270) * C * M + 28.0 * C * C) / 6.3e12 * 1e3
        if fused:
            floor = nl * 5 * 1.5e-3
        else:       # forward 7 + backward 9 dependent launches; K steps of qkv, proj, fc1, fc2 and their data gradients (the same four contractions)
            ksteps = 2 * (C + C + C + 4 * C) / 64.0
            floor = nl * (16 * 1.5e-3 + ksteps * 0.33e-3 + 8 * 3e-3 + 2 * 5e-3 + 4 * 4e-3)     # + attention fwd / bwd (5 us each) + 4 norm launches (4 us)
        t = max(mfma, hbm, floor)
        total += t
        stages.append({"stage": st.prefix, "tokens": M, "C": C, "mfma_ms": round(mfma, 3), "hbm_ms": round(hbm, 3), "floor_ms": round(floor, 3),
                       "bound": "mfma" if t == mfma else ("hbm" if t == hbm else "launch+K-loop")})
    total += 0.6
    return {"ms_per_step": round(total, 2), "samples_per_s": round(batch / total * 1e3, 1), "stages": stages,
            "note": "ceiling of the layer-by-layer decomposition with every kernel on its own roof (profiles/round6/attainable.md); the 70 % MFMA "
                    "target needs a different decomposition (whole layers on chip: ~10x fewer bytes, ~7x fewer launches), not faster kernels"}


def trained_like_model(cfg, compute, engine_options=None):
    """random weights with "trained-like" statistics, so that every branch carries O(1) signal (random data, section 5.4 rule 25)"""
    from scOT.model import ScOT
    model = ScOT(cfg, compute=compute, engine_options=engine_options)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.endswith("weight.bias") and ("norm" in k):
                p.fill_(1.0)
            elif k.startswith("residual_blocks") and k.count(".") == 2 and k.endswith(".weight"):
                p.fill_(0.5)
            elif p.dim() >= 2 and p.shape[-1] > 2:
                fan = p[0].numel()
                p.normal_(0, 1.0 / fan ** 0.5)
    return model.to(DEV)


def other_config(model_tag, batch, size, channels, compute, steps=10, warmup=5):
    """One of BASELINE.json's non-headline configurations through the SAME step as the headline (zero-grad + forward + loss + backward on
    resident synthetic inputs, eager replay of the recorded step), `warmup` untimed + `steps` timed steps, with the parity of the mode
    against the real reference's fixture of that configuration."""
    from poseidon_amd.config import preset
    res = {"workload": f"Poseidon-{model_tag} fwd+bwd, {size}x{size}x{channels} grids, per-GPU batch {batch}", "dtype": compute}
    try:
        par = parity_check(model_tag, compute, size, channels)
        res["parity_output_rel_l2"] = par.get("output_rel_l2")
        res["parity_fixture"] = par.get("fixture") or par.get("note")
        res["parity_meets_bound"] = par.get("meets_bound")
        cfg = preset(model_tag, image_size=size, num_channels=channels, num_out_channels=channels,
                     channel_slice_list_normalized_loss=[0, 1, channels - 1, channels])
        torch.manual_seed(1234)
        model = trained_like_model(cfg, compute)
        torch.manual_seed(100)
        kw = dict(pixel_values=torch.randn(batch, channels, size, size, device="cuda"),
                  time=torch.randint(0, 8, (batch,), device="cuda").float() / 10.0,
                  labels=torch.randn(batch, channels, size, size, device="cuda"))
        loss = torch.zeros((), device="cuda")

        def one():
            model.zero_grad(overlap=True)
            out = model(**kw)
            out.loss.backward()
            loss.copy_(out.loss.detach())
        for _ in range(max(3, warmup)):      # (call 1 runs the ops, call 2 records the step, later calls replay it)
            one()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            one()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        tf = step_flops(model_tag, size, batch) / (ms / 1e3)
        ovf = model._engine.grad_overflow
        res.update({"ms_per_step": ms, "samples_per_s": batch / (ms / 1e3), "steps": steps, "warmup": max(3, warmup), "tflops": tf,
                    "frac_of_mfma_peak": tf / PEAK_TFLOPS[compute], "loss": float(loss), "grad_overflow": int(ovf) if ovf is not None else None})
        model._engine.reset_tapes()
        del model, kw
        torch.cuda.empty_cache()
    except Exception as e:  # pragma: no cover
        res["error"] = repr(e)
    return res


def launch_table(engine, run_step, nsteps=3, dump=None):
    """Per-launch GPU durations INSIDE real steps: the recorded step is replayed with a HIP-event pair around every C-ABI
    call, each pair on the stream the call launches on (main or weight-gradient side stream), so concurrency and cache state
    are the step's own.  Returns {family: {ms_per_step, launches_per_step, gflop_per_step}}, plus the worst wgrad instance."""
    engine.launch_timer = []
    for _ in range(nsteps):
        run_step()
    _sync()
    log, engine.launch_timer = engine.launch_timer, None
    fam, inst = {}, {}
    main = torch.cuda.current_stream().cuda_stream
    chain_ms = 0.0
    if dump and log:
        # tools/launch_summary.py groups these by (entry point, shape arguments, stream): the per-stage view of the chain
        rows, first = [], log[0][2]
        for name, args, e0, e1 in log:
            ints = [int(x) for x in args if isinstance(x, int) and not isinstance(x, bool) and -(1 << 31) < x < (1 << 31)]
            rows.append([name, ints, int((args[-1] or 0) == main), round(first.elapsed_time(e0), 4), round(e0.elapsed_time(e1), 4)])
        json.dump({"nsteps": nsteps, "rows": rows}, open(dump, "w"))
    for name, args, e0, e1 in log:
        ms = e0.elapsed_time(e1)
        if (args[-1] or 0) == main:
            chain_ms += ms
        fl = 0.0
        key = name.replace("scot_", "")
        if name == "scot_wgrad_group":
            key = "wgrad_group (all weight gradients of a layer, incl. grouped split-K reduce)"
            n = args[1]
            fl = sum(2.0 * args[2] * args[7][i] * args[8][i] for i in range(n))
            d = inst.setdefault((tuple(args[7][i] for i in range(n)), tuple(args[8][i] for i in range(n)), args[2]), [0.0, 0, fl])
            d[0] += ms
            d[1] += 1
        if name == "scot_wgrad_mlp":
            # fc1 / fc2 weight gradients of one layer; the kernel also recomputes u = h·W1^T and du = gelu'(u)·(dz·W2) (the same
            # FLOPs again) instead of reading them — only the two weight-gradient products count as algorithmic work
            key = "wgrad_mlp (fc1 + fc2 weight gradients, gelu(u) / du recomputed in the kernel)"
            fl = 2 * 2.0 * args[9] * args[10] * args[11]
        if name == "scot_window_attn_bwd_rep":      # the same kernels, accumulating the table / scale gradients into replicas
            name, key = "scot_window_attn_bwd", "window_attn_bwd"
        if name in ("scot_window_attn_fwd", "scot_window_attn_bwd"):
            # algorithmic work of a (window, head): 4 N^2 d forward (QK^T, PV), 10 N^2 d backward (dV, dP, dQ, dK + the recomputed S);
            # the backward kernels execute 14 N^2 d (S and dP once per half)
            o = 6 if name.endswith("fwd") else 10
            batch, Hp, Wp, C, ws = args[o], args[o + 1], args[o + 2], args[o + 3], args[o + 5]
            fl = (4.0 if name.endswith("fwd") else 10.0) * (ws * ws) ** 2 * C * batch * (Hp // ws) * (Wp // ws)
        if name == "scot_block_tail_fwd":       # projection + fc1 + fc2 (+ the next layer's qkv projection as epilogue)
            M, C, hid = args[35], args[37], args[38]
            fl = 2.0 * M * (C * C + 2 * C * hid + (3 * C * C if args[32] else 0))
        if name == "scot_block_tail_bwd":       # data gradients of fc2, fc1, projection (+ the qkv data gradient as prologue)
            M, C, hid = args[38], args[40], args[41]
            fl = 2.0 * M * (C * C + 2 * C * hid + (3 * C * C if args[30] else 0))
        if name == "scot_gemm":
            lay, M, N, K = args[0], args[2], args[3], args[4]
            key = ("gemm NT (forward Linear)", "gemm NN (dgrad)", "gemm TN (wgrad, incl. split-K reduce)")[lay]
            fl = 2.0 * M * N * K
            if lay == 2:
                d = inst.setdefault((M, N, K), [0.0, 0, fl])
                d[0] += ms
                d[1] += 1
        d = fam.setdefault(key, [0.0, 0, 0.0])
        d[0] += ms
        d[1] += 1
        d[2] += fl
    table = {k: {"ms_per_step": v[0] / nsteps, "launches_per_step": v[1] / nsteps, "gflop_per_step": v[2] / nsteps / 1e9}
             for k, v in sorted(fam.items(), key=lambda kv: -kv[1][0])}
    worst = None
    for (M, N, K), (ms, n, fl) in inst.items():
        tf = fl * n / ms / 1e9
        if n / nsteps >= 8 and (worst is None or tf < worst["tflops"]):    # a per-layer instance, not one of the few trunk GEMMs
            worst = {"shape_MNK": [M, N, K], "us_per_launch": ms / n * 1e3, "tflops": tf, "launches_per_step": n / nsteps}
    launch_table.main_stream_ms_per_step = chain_ms / nsteps
    launch_table.wgrad_instances = sorted(({"shape_MNK": [list(k[0]) if isinstance(k[0], tuple) else k[0], list(k[1]) if isinstance(k[1], tuple) else k[1], k[2]],
                                            "us_per_launch": round(ms / n * 1e3, 1), "tflops": round(fl * n / ms / 1e9, 1),
                                            "launches_per_step": n / nsteps} for k, (ms, n, fl) in inst.items()),
                                          key=lambda d: -d["us_per_launch"] * d["launches_per_step"])[:8]
    return table, worst


DUMP_BUDGET = 64 << 20      # bytes: every file --dump-outputs writes, together


def dump_outputs(out_dir, model, pred, loss):
    """--dump-outputs: what a caller of the timed step holds after its last call — the prediction, the loss and the parameter gradients —
    as .npy files, so that two builds can be compared output for output (the inputs and weights are seeded: identical with the same
    arguments).  The prediction is written whole while it fits in half of DUMP_BUDGET (`output.npy`, float32), else as a seeded sample of
    its elements (`output_sample.npy`).  The gradients, taken in named_parameters() order: one L2 norm per parameter (`grad_norms.npy`,
    float64) and their concatenation, whole while it fits in a quarter of the budget (`grads.npy`), else a seeded sample (`grads_sample.npy`).
    The sample positions depend only on the seed and the element count, so two runs of one configuration sample the same elements."""
    import numpy as np

    def fit(flat, k, seed):
        if flat.numel() <= k:
            return flat, ""
        idx = torch.randint(0, flat.numel(), (k,), generator=torch.Generator().manual_seed(seed)).sort().values
        return flat[idx.to(flat.device)], "_sample"

    grads = [p.grad.detach().float().reshape(-1) for _, p in model.named_parameters() if p.grad is not None]
    out, tag = fit(pred.detach().float().reshape(-1), DUMP_BUDGET // 2 // 4, 1)
    files = {"output" + tag: out.reshape(pred.shape) if not tag else out,
             "loss": torch.tensor([float(loss)], dtype=torch.float64),
             "grad_norms": torch.stack([g.double().norm() for g in grads])}
    gs, tag = fit(torch.cat(grads), DUMP_BUDGET // 4 // 4, 2)
    files["grads" + tag] = gs
    arrays = {k: v.cpu().numpy() for k, v in files.items()}
    assert sum(v.nbytes for v in arrays.values()) <= DUMP_BUDGET
    os.makedirs(out_dir, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), v)


DEV = "cuda"     # "cpu" only under the hidden --_emu switch: the CPU-emulated kernels of tests/hipemu over gloo, for the control-flow test


class _HostEvent:
    """stand-in for torch.cuda.Event on the emulated (CPU) run: execution is synchronous there, so host time is device time"""

    def __init__(self, enable_timing=True):
        self.t = None

    def record(self, stream=None):
        self.t = time.perf_counter()

    def elapsed_time(self, other):
        return (other.t - self.t) * 1e3


def _sync():
    if DEV == "cuda":
        torch.cuda.synchronize()


def _event():
    return torch.cuda.Event(enable_timing=True) if DEV == "cuda" else _HostEvent()


def _enter_emulation():
    """tests/test_bench_flow_cpu.py: this file's main() — launcher contract, rank-0-only sections, --dp auto probes, timing all-reduces, the
    JSON line — with world size 2 over gloo on the CPU-emulated kernels and a tiny model.  Never a measurement: the line says `emulated`."""
    global DEV
    DEV = "cpu"
    here = os.path.join(ROOT, "tests", "hipemu")
    sys.path.insert(0, here)
    import emu_session
    import scOT.model as M
    from poseidon_amd import ops
    lib = emu_session.load_emu()
    ws = torch.empty(32 << 20, dtype=torch.uint8)
    ops.L = lambda: ops._Recording(lib if ops._active == "bf16" else emu_session.load_emu(ops._active), ops._recorder) \
        if ops._recorder is not None else (lib if ops._active == "bf16" else emu_session.load_emu(ops._active))
    ops.stream, ops.workspace = (lambda: None), (lambda need=0: ws)
    ops.ptr = lambda t: None if t is None else t.data_ptr()
    M._require_hip = lambda t: None


def main():
    a = parse()
    if a.cpu_worker:
        print(json.dumps(_cpu_baseline_worker(a.model, a.size, a.channels, a.cpu_seconds)), flush=True)
        return
    if a.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` by itself: become the launcher — one rank per GPU under torch.distributed.run (RCCL over xGMI),
        # rank 0 prints the one JSON line (the reference launches its driver the same way: `accelerate launch`, README.md:50-57)
        import socket
        import subprocess
        have = torch.cuda.device_count()
        if have < a.gpus:
            raise SystemExit(f"bench.py: --gpus {a.gpus} but only {have} GPU(s) are visible")
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}: launch as `python bench.py --gpus N` (self-launching) or under "
                         "`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N`")
    if a.emu:
        _enter_emulation()
        a.no_parity = a.no_graph = a.no_cpu_baseline = a.no_other_configs = True
    else:
        torch.cuda.set_device(local)
    dist = None
    rccl_log = None
    if a.emu and (world > 1 or "RANK" in os.environ):
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
    elif world > 1 or "RANK" in os.environ:   # under torchrun the collective path is exercised even with one rank
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if a.rccl_channels > 0:
            # every RCCL channel is one workgroup of each collective kernel: a cap bounds the CUs the gradient exchange takes from a
            # backward that is throughput-bound on both of its streams (DESIGN.md section 7 has the recommended value)
            os.environ["NCCL_MAX_NCHANNELS"] = str(a.rccl_channels)
            os.environ["NCCL_MIN_NCHANNELS"] = str(min(a.rccl_channels, int(os.environ.get("NCCL_MIN_NCHANNELS", a.rccl_channels))))
        if "NCCL_DEBUG_FILE" not in os.environ:
            # RCCL's own log goes to a per-rank file in a private directory (a box-wide NCCL_DEBUG=VERSION would otherwise put its banner on
            # stdout beside the one JSON line), removed once parsed.  Every rank asks for the same INFO subsystems (init-time lines only:
            # nothing is logged per collective), rank 0's file is parsed into the line's `rccl` — what RCCL chose for the gradient exchange
            # (rings, channels, algorithm / protocol) — so that an N-GPU line can be read without re-running it
            import tempfile
            rccl_dir = tempfile.mkdtemp(prefix="scot_rccl_")
            os.environ["NCCL_DEBUG_FILE"] = os.path.join(rccl_dir, f"rank{rank}.log")
            os.environ.update(NCCL_DEBUG="INFO", NCCL_DEBUG_SUBSYS="INIT,GRAPH,TUNING,ENV")
            rccl_log = os.environ["NCCL_DEBUG_FILE"]
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        if dist.get_world_size() != a.gpus:
            raise SystemExit(f"RCCL process group has {dist.get_world_size()} ranks, --gpus {a.gpus}")

    from poseidon_amd.config import preset
    from poseidon_amd.dp import GradAllReducer, OverlappedGradAllReducer
    from scOT.model import ScOT

    ch = a.channels
    cfg = preset(a.model, image_size=a.size, num_channels=ch, num_out_channels=ch,
                 channel_slice_list_normalized_loss=[0, 1, ch - 1, ch])
    if a.emu:      # a model the emulated kernels step through in seconds (the control flow is what is under test)
        from poseidon_amd.config import ScOTConfig
        cfg = ScOTConfig(image_size=a.size, patch_size=4, num_channels=ch, num_out_channels=ch, embed_dim=16, depths=[2, 2], num_heads=[1, 2],
                         skip_connections=[1, 0], window_size=4, mlp_ratio=4.0, qkv_bias=True, drop_path_rate=0.0, p=1,
                         channel_slice_list_normalized_loss=[0, 1, ch - 1, ch], use_conditioning=True)
    parity = None
    if rank == 0 and a.full and not a.no_parity:
        parity = parity_check(a.model, a.compute, a.size, ch)
        if parity.get("fixture") and not parity["meets_bound"]:
            print(f"bench.py: --compute {a.compute} is at {parity['output_rel_l2']:.2e} from the reference fixture (bound "
                  f"{parity['bound']:.0e}): the number below is NOT a compliant measurement", file=sys.stderr)
    torch.manual_seed(1234)  # identical initial weights on every rank (no broadcast needed)
    # (fused_min_rows=0 changes no launch of the timed batch — every fused stage has >= 16384 token rows at the headline batch; it keeps the
    #  one-sample forwards of the consistency check below on the same kernel family as the batch they are compared with)
    from poseidon_amd.engine import ENGINE_OPTIONS
    from poseidon_amd.geometry import stage_plan
    fused_rows = [a.batch * st.res[0] * st.res[1] for st in stage_plan(cfg)[1] if st.dim in (96, 192)]
    same_launches = bool(fused_rows) and min(fused_rows) >= ENGINE_OPTIONS["fused_min_rows"] and not a.emu
    model = trained_like_model(cfg, a.compute, engine_options={"fused_min_rows": 0} if same_launches else None)
    torch.manual_seed(100 + rank)
    B = a.batch
    pv = torch.randn(B, ch, a.size, a.size, device=DEV)
    lab = torch.randn(B, ch, a.size, a.size, device=DEV)
    tt = torch.randint(0, 8, (B,), device=DEV).float() / 10.0
    kw = dict(pixel_values=pv, time=tt, labels=lab)

    # The launch policies of the TIMED batch against the batch-1 path (the golden fixture above is batch 1: 128-row tails, grouped weight
    # gradients, direct-to-LDS / four-register-set GEMMs and the XCD-local attention grid are only selected at the large row counts):
    # samples are independent, so prediction[i] of the batch must equal the prediction of sample i alone, up to accumulation order.
    consistency = None
    if rank == 0 and a.full and not a.no_parity:
        full = model(**kw).output.detach().clone()       # (grad mode on: the training forward, the one that is timed)
        worst = 0.0
        for i in sorted({0, B // 3, B - 1}):
            one = model(pixel_values=pv[i:i + 1].contiguous(), time=tt[i:i + 1].contiguous(), labels=lab[i:i + 1].contiguous()).output.detach()
            worst = max(worst, float((one - full[i:i + 1]).norm() / full[i:i + 1].norm()))
        model._engine.reset_tapes()
        consistency = {"samples": sorted({0, B // 3, B - 1}), "max_rel_l2_vs_batch1": worst,
                       "note": "training-mode forward of the timed batch vs the same samples one at a time (same weights, same mode)"}
        if parity is not None:
            parity["batch_consistency"] = consistency

    after = GradAllReducer(model, dist, wire=a.wire, collective=a.dp_collective, backend=a.dp_backend) if dist is not None else None
    overlapped = (OverlappedGradAllReducer(model, dist, wire=a.wire, collective=a.dp_collective, backend=a.dp_backend)
                  if (dist is not None and a.dp != "after") else None)
    exchange = [None if (dist is None or a.dp == "none") else ("after" if a.dp != "overlap" else "overlap")]   # current mode
    loss_buf = torch.zeros((), device=DEV)

    def compute_step():
        model.zero_grad(overlap=True)      # as poseidon_amd.train.Trainer does: the gradient arena's fill runs beside the forward
        out = model(**kw)
        out.loss.backward()
        loss_buf.copy_(out.loss.detach())
        return out.output.detach()

    # warm-up (eager): builds the arena, runs the device self test, fills allocator pools, records the step tape
    for i in range(4):   # (call 1 of a step signature runs the ops, call 2 records the step tape, later calls replay it)
        compute_step()
        if exchange[0] == "after":
            after.allreduce()
        if exchange[0] == "overlap" and i == 0:
            overlapped.attach()   # the engine exists now: from here on the backward launches the range all-reduces itself
    _sync()

    graph = graph_pred = None
    if a.graph and not a.no_graph and exchange[0] != "overlap":
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            graph_pred = compute_step()       # (the recorded step's prediction: every replay rewrites it)
        _sync()

    use_graph = [graph is not None]

    def step():
        if use_graph[0]:
            graph.replay()
            pred = graph_pred
        else:
            pred = compute_step()
        if exchange[0] == "after":
            after.allreduce()
        return pred

    def probe(flag, n=3):
        use_graph[0] = flag
        step()
        _sync()
        t = time.perf_counter()
        for _ in range(n):
            step()
        t_enq = time.perf_counter() - t
        _sync()
        return (time.perf_counter() - t) / n, t_enq / n

    # hipGraph replay removes the CPU launch cost but (ROCm 7.2) serialises most of the side-stream overlap; eager launches overlap the
    # weight-gradient stream with the main chain and won every measured run (rounds 3-6: 18.3-19.8 vs 32.9-34.5 ms), so they are the
    # default and the graph is timed only on request (--graph)
    mode_info = {}
    if dist is not None and a.dp == "auto" and exchange[0] is not None:
        # gradient exchange: one chunked all-reduce after the step vs range all-reduces launched from inside the backward
        ug = use_graph[0]
        t_after, _ = probe(ug)
        overlapped.attach()
        exchange[0] = "overlap"
        for _ in range(3):
            probe(False, n=1)                       # warm / record / first replay of the hooked step
        t_over, _ = probe(False)
        tt2 = torch.tensor([t_after, t_over], device=DEV, dtype=torch.float64)
        dist.all_reduce(tt2, op=dist.ReduceOp.MAX)
        t_after, t_over = float(tt2[0]), float(tt2[1])
        mode_info.update({"probe_dp_after_ms": t_after * 1e3, "probe_dp_overlap_ms": t_over * 1e3})
        if t_after <= t_over:
            overlapped.detach()
            exchange[0] = "after"
            for _ in range(3):
                probe(ug, n=1)
            use_graph[0] = ug
        else:
            use_graph[0] = False
    for _ in range(a.warmup):
        step()
    if dist:
        dist.barrier()
    _sync()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        pred = step()
    _sync()
    if dist:
        dist.barrier()
    dt = time.perf_counter() - t0
    if dist:
        tmax = torch.tensor([dt], device=DEV, dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax)
    ms = dt / a.steps * 1e3
    if a.dump_outputs and rank == 0:      # before anything below steps the model again
        dump_outputs(a.dump_outputs, model, pred, loss_buf)
    # exposed communication = timed step - the same step with the gradient exchange switched off (same process, same mode)
    exposed = None
    if a.full and dist is not None and exchange[0] is not None:
        mode = exchange[0]
        if mode == "overlap":
            overlapped.detach()
        exchange[0] = None
        for _ in range(3):
            probe(use_graph[0] if mode != "overlap" else False, n=1)
        t_bare, _ = probe(use_graph[0] if mode != "overlap" else False, n=max(3, a.steps // 2))
        tb = torch.tensor([t_bare], device=DEV, dtype=torch.float64)
        dist.all_reduce(tb, op=dist.ReduceOp.MAX)
        exposed = {"step_without_exchange_ms": float(tb) * 1e3, "exposed_ms_per_step": ms - float(tb) * 1e3}
        exchange[0] = mode
        if mode == "overlap":
            overlapped.attach()
            for _ in range(3):
                probe(False, n=1)
    comm = None
    if a.full and dist is not None and exchange[0] is not None:   # GPU time of the gradient exchange alone (pack + collective + unpack), outside the timed region
        if exchange[0] == "overlap":
            overlapped.timing = []
            for _ in range(3):
                step()
            _sync()
            comm = overlapped.comm_ms() / 3
            overlapped.timing = None
        else:
            e0, e1 = _event(), _event()
            _sync()
            e0.record()
            for _ in range(3):
                after.allreduce()
            e1.record()
            _sync()
            comm = e0.elapsed_time(e1) / 3
    # What the metric (forward + backward, no optimizer) does NOT contain: producing the 16-bit / transposed operand copies of changed
    # weights.  In training the fused optimizer emits them while it updates the master weights (scot_adamw_step + scot_transpose_cast);
    # a loop around a foreign optimizer pays this pass at the top of every forward.  Reported, not included in `value`.
    refresh_ms = None
    eng = model._engine
    if a.full and eng.shadow is not None:
        from poseidon_amd import ops as _ops
        prev = _ops.use(eng.lib_kind)
        try:
            e0, e1 = _event(), _event()
            _sync()
            e0.record()
            for _ in range(3):
                model.mark_weights_dirty()
                eng.refresh_weight_copies(True)
            e1.record()
            _sync()
            refresh_ms = e0.elapsed_time(e1) / 3
        finally:
            _ops.use(prev)
    overflow = int(model._engine.grad_overflow) if model._engine.grad_overflow is not None else None   # fp16 gradient scale
    # forward / backward split of the step on the GPU's clock: three events on the main stream around the two halves of a few extra
    # steps (the backward's last act is the main stream's wait for the weight-gradient stream, so its end covers both streams)
    phase = None
    if a.full and not use_graph[0]:
        ev = [[_event() for _ in range(3)] for _ in range(5)]
        for e in ev:
            model.zero_grad(overlap=True)
            e[0].record()
            out = model(**kw)
            e[1].record()
            out.loss.backward()
            e[2].record()
            if exchange[0] == "after":
                after.allreduce()
        _sync()
        phase = {"forward_ms": sorted(e[0].elapsed_time(e[1]) for e in ev)[2], "backward_ms": sorted(e[1].elapsed_time(e[2]) for e in ev)[2]}
    table = worst = None
    table_err = None
    if a.full:
        try:   # every rank steps (under DP a step contains collectives); rank 0 reports
            if a.emu:
                raise RuntimeError("per-launch HIP-event timing needs the GPU")
            eager = use_graph[0]
            use_graph[0] = False
            table, worst = launch_table(model._engine, step, dump=a.launch_dump if rank == 0 else None)
            use_graph[0] = eager
        except Exception as e:  # pragma: no cover
            table_err = repr(e)
    total_samples = B * world * a.steps
    value = total_samples / dt

    if rank == 0:
        step_tflop = step_flops(a.model, a.size, B)             # per GPU per step
        achieved = step_tflop / (ms / 1e3)                       # TFLOP/s per GPU
        peak = PEAK_TFLOPS[a.compute]
        step_roof = {"bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
                     "scope": "whole step, algorithmic FLOPs 3(B*F+P) per GPU (SURVEY.md 8d)"}
        roof = dict(step_roof, traffic=None)
        launches = None
        if a.full:      # the per-kernel roofline needs the per-launch table
            try:
                # the dominant kernel family of the committed rocprof summary (profiles/round2: the grouped weight-gradient GEMMs),
                # timed live inside real steps (launch_table above)
                if table is None:
                    raise RuntimeError(table_err)
                launches = {"launches_per_step": sum(v["launches_per_step"] for v in table.values()),
                            "kernel_ms_per_step": sum(v["ms_per_step"] for v in table.values()),
                            "main_stream_ms_per_step": launch_table.main_stream_ms_per_step,
                            "wgrad_instances": launch_table.wgrad_instances,
                            "top": {k: {kk: round(vv, 3) for kk, vv in v.items()} for k, v in list(table.items())[:10]}}
                # the GEMM family with the most in-step time is the one the roofline is quoted on (round 3: gemm_fast_kernel<NT>, the
                # forward Linear layers and — on the transposed weight copies — the data gradients of the deep stages)
                gemm_fams = {k: v for k, v in table.items() if v["gflop_per_step"] > 0}
                if gemm_fams:
                    name, wg = max(gemm_fams.items(), key=lambda kv: kv[1]["ms_per_step"])
                    tf = wg["gflop_per_step"] / wg["ms_per_step"]      # GFLOP / ms = TFLOP/s
                    traffic, traffic_src, tj = None, None, {}
                    for rnd in ("round6", "round5", "round4", "round3", "round2"):   # HBM bytes per launch (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes)
                        tpath = os.path.join(ROOT, "profiles", rnd, "pmc_traffic.json")
                        if os.path.exists(tpath):
                            tj = json.load(open(tpath))
                            traffic_src = f"profiles/{rnd}/pmc_traffic.json"
                            traffic = (tj.get("bytes_per_launch") or {}).get(name.split(" ")[0] + (" " + name.split(" ")[1] if name.startswith("gemm") else ""))
                            if traffic is None and name.startswith("wgrad_group"):
                                traffic = tj.get("wgrad_bytes_per_launch")
                            break
                    # every family under its two roofs: algorithmic FLOPs against the dense MFMA peak, HBM bytes (PMC passes of the newest
                    # committed profile) against the 6.3 TB/s a streaming copy reaches on this part
                    fams = {}
                    tb = (tj.get("bytes_per_launch") or {}) if traffic_src else {}
                    for k, v in table.items():
                        short = k.split(" ")[0] + (" " + k.split(" ")[1] if k.startswith("gemm") else "")
                        e = {"ms_per_step": round(v["ms_per_step"], 3), "launches_per_step": v["launches_per_step"]}
                        if v["gflop_per_step"] > 0:
                            e["tflops"] = round(v["gflop_per_step"] / v["ms_per_step"], 1)
                            e["frac_mfma"] = round(v["gflop_per_step"] / v["ms_per_step"] / peak, 4)
                        if short in tb:
                            gb = tb[short] * v["launches_per_step"] / 1e9
                            e["hbm_gb_per_step"] = round(gb, 2)
                            e["frac_hbm"] = round(gb / v["ms_per_step"] / 6.3, 4)         # GB / ms = TB/s
                        if "frac_mfma" in e or "frac_hbm" in e:
                            e["nearer_roof"] = "hbm" if e.get("frac_hbm", 0) > e.get("frac_mfma", 0) else "mfma"
                        if v["ms_per_step"] >= 0.05:
                            fams[k] = e
                    roof = {"bound": "mfma", "achieved": tf, "peak": peak, "unit": "TFLOP/s", "frac": tf / peak, "traffic": traffic,
                            "families": fams, "traffic_source": traffic_src,
                            "kernel": name + ": in-step durations (HIP events on the launching stream around every call of the replayed step)",
                            "us_per_launch": wg["ms_per_step"] / wg["launches_per_step"] * 1e3,
                            "launches_per_step": wg["launches_per_step"], "algorithmic_gflop_per_step": wg["gflop_per_step"],
                            "gemm_families": {k: {"tflops": round(v["gflop_per_step"] / v["ms_per_step"], 1), "frac": round(v["gflop_per_step"] / v["ms_per_step"] / peak, 4),
                                                  "ms_per_step": round(v["ms_per_step"], 3), "launches_per_step": v["launches_per_step"]}
                                              for k, v in gemm_fams.items()},
                            "worst_wgrad_instance": worst, "whole_step": step_roof}
            except Exception as e:  # pragma: no cover
                roof = dict(step_roof, traffic=None, error=repr(e))
        weight_refresh = None
        if a.full:
            weight_refresh = {"ms": refresh_ms, "included_in_value": False,
                              "ms_per_step_incl": (ms + refresh_ms) if refresh_ms is not None else None,
                              "note": "16-bit + transposed operand copies of the weights, needed once per optimizer step: written by "
                                      "FusedAdamW.step (outside forward + backward), or by the next forward after a foreign optimizer"}
        # whole-step HBM traffic of the newest committed PMC passes against the 8 TB/s peak and SURVEY 8(d)'s ideal fused traffic
        hbm = None
        for rnd in ("round6", "round5", "round4", "round3"):
            tpath = os.path.join(ROOT, "profiles", rnd, "pmc_traffic.json")
            if os.path.exists(tpath) and a.model == "B" and a.size == 128 and B == 64:
                ws_ = (json.load(open(tpath)).get("whole_step") or {})
                if ws_.get("hbm_gb_per_step"):
                    by = ws_["hbm_gb_per_step"] * 1e9
                    ideal = 80e6 * B
                    hbm = {"bytes_per_step": by, "source": f"profiles/{rnd}/pmc_traffic.json (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE, separate passes)",
                           "frac_of_8TBs": by / (ms * 1e-3) / 8e12, "ideal_bytes_per_step": ideal, "waste_ratio": by / ideal,
                           "note": "ideal = SURVEY 8(d)'s ~80 MB per sample of fused activation traffic"}
                break
        if isinstance(roof, dict):
            roof["hbm"] = hbm
            try:
                att = attainable_model(cfg, B)
                att["frac_of_mfma_peak"] = round(step_tflop / (att["ms_per_step"] / 1e3) / peak, 4)
                att["measured_over_attainable"] = round(ms / att["ms_per_step"], 2)
                roof["attainable"] = att
            except Exception as e:  # pragma: no cover
                roof["attainable"] = {"error": repr(e)}
        rccl = None
        if rccl_log and os.path.exists(rccl_log):
            try:
                import re as _re
                txt = open(rccl_log, errors="replace").read()
                rccl = {"max_nchannels_requested": a.rccl_channels or None,
                        "version": (_re.findall(r"(?:RCCL|NCCL) version[^\n]*", txt) or [None])[0],
                        "n_channels": (_re.findall(r"Channel \d+/(\d+)", txt) or [None])[0],
                        "graph_search": sorted(set(_re.findall(r"Pattern \d+, crossNic \d+, nChannels \d+, bw [\d./]+, type \S+", txt)))[:6],
                        "rings": [l.strip()[:160] for l in _re.findall(r"\[RINGS\][^\n]*", txt)[:2]],
                        "algo_proto": sorted(set(_re.findall(r"[Aa]lgo(?:rithm)?\s*[:=]?\s*\w+[^\n]{0,40}[Pp]roto(?:col)?\s*[:=]?\s*\w+", txt)))[:8],
                        "transports": sorted(set(_re.findall(r"via (P2P[^\s]*|SHM[^\s]*|NET[^\s]*|direct[^\s]*)", txt)))[:6]}
            except Exception as e:  # pragma: no cover
                rccl = {"error": repr(e)}
        res = {**({"emulated": "CPU emulation of the kernels over gloo (tests/test_bench_flow_cpu.py): control flow only, NOT a measurement"} if a.emu else {}),
               "metric": "PDE-grid samples/sec (fwd+bwd)", "value": value, "unit": "samples/s", "n_gpus": world, "steps": a.steps,
               "warmup": a.warmup, "ms_per_step": ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
               "dtype": a.compute, "data": "synthetic",
               "baseline_dtype": "bf16 in BASELINE.json's config text; this library's bf16 build sits at 6.2e-3 from the reference (non-compliant with "
                                 "the 1e-3 bound), its fp16 build (same width, same MFMA rate, fp32 accumulation) at 6.9e-4: fp16 is what is timed",
               "parity": parity, "phases": phase, "weight_refresh": weight_refresh, "grad_overflow": overflow,
               "grad_comm_ms_per_step": comm, "grad_exchange_exposed": exposed, "rccl": rccl,
               "config": {"workload": f"Poseidon-{a.model} fwd+bwd, {a.size}x{a.size}x{ch} grids, per-GPU batch {B}",
                          "global_batch": B * world, "parallelism": f"dp{world}", "graph": bool(use_graph[0]), "full": a.full, **mode_info,
                          "grad_wire": a.wire if dist is not None else None, "grad_exchange": exchange[0],
                          "grad_collective": a.dp_collective if dist is not None else None, "grad_backend": a.dp_backend if dist is not None else None, "grad_comm_ms_per_step": comm,
                          "loss": float(loss_buf),
                          "weight_refresh": weight_refresh, "parity": parity, "grad_overflow": overflow, "phases": phase,
                          "in_step_launches": launches},
               "roofline": roof}
        headline = (a.model, B, a.size, ch) == ("B", 64, 128, 4)
        if a.full and world == 1 and dist is None and headline and not a.no_other_configs:
            # the other BASELINE.json configurations, timed by this same process (the driver's line then referees all five)
            model._engine.reset_tapes()
            torch.cuda.empty_cache()
            res["other_configs"] = [other_config(*c, a.compute) for c in OTHER_CONFIGS]
        if a.full and world == 1 and not a.no_cpu_baseline:
            try:
                res["cpu_baseline"] = cpu_baseline(a.model, a.size, ch, a.cpu_seconds)
            except Exception as e:  # pragma: no cover
                res["cpu_baseline"] = {"error": repr(e)}
        print(json.dumps(res), flush=True)
    if dist:
        dist.destroy_process_group()
    if rccl_log:      # this rank's RCCL log and its private directory
        import shutil
        shutil.rmtree(os.path.dirname(rccl_log), ignore_errors=True)


if __name__ == "__main__":
    main()
