"""The spectral resize, measured: (a) the two-launch form — an fp32 NT GEMM that writes U = X [Pr; Pi]^T, then scot_spectral_apply —
against the one-launch scot_spectral_resize, 256 planes, device events, the two alternated in one process; (b) a Poseidon-B fp16
batch-64 plan `run` at 256 x 256 and 64 x 64 (`export_plan(..., resize=True)`) against the native 128 x 128 plan.

usage: python tools/bench_resize.py --part kernel|plan [--repeat 3] [--seconds 0.5] [--nimg 256]
  --part kernel   one JSON line per (s, t) in (256,128), (128,256), (64,128), (128,64): us per call of either form (a list: one value per
                  repeat, the forms alternating), both outputs against the fp64 reference within the bound of
                  tests/spectral_resize_cases.py, and the shape's own roof: FLOPs 4 t s (s + t) per plane over the f32-MFMA peak, bytes
                  4 (s^2 + t^2) per plane over the HBM peak, and which of the two binds
  --part plan     one JSON line: ms per `run` of the three plans (lists, alternating), and what the two resamplings add
Every timed window holds at least --seconds of device work (the launch count is calibrated first) behind a warm-up at that shape.
Numbers: profiles/plan_resize/README.md."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=("kernel", "plan"), required=True)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--seconds", type=float, default=0.5)
ap.add_argument("--nimg", type=int, default=256)
ap.add_argument("--batch", type=int, default=64)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from poseidon_amd import ops  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_resize: no GPU (a timing needs the device; nothing is measured on the CPU)")
PEAK_F32_MFMA, PEAK_HBM = 157.3e12, 8.0e12
SHAPES = [(256, 128), (128, 256), (64, 128), (128, 64)]
U32 = 2.0 ** -24


def window(fn, launches):
    """device-event milliseconds of `launches` back-to-back calls of fn"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def calibrated(fn):
    """warm-up, then the number of calls that fill --seconds"""
    for _ in range(5):
        fn()
    per_call = window(fn, 20) / 20
    return max(20, int(args.seconds * 1e3 / max(per_call, 1e-3)) + 1)


def alternate(cases):
    """{name: fn} -> {name: [per-call time of every repeat]} (in the unit of `window`), the cases alternating inside every repeat"""
    counts = {k: calibrated(fn) for k, fn in cases.items()}
    out = {k: [] for k in cases}
    for _ in range(max(1, args.repeat)):
        for k, fn in cases.items():
            out[k].append(window(fn, counts[k]) / counts[k])
    return out, counts


def kernel_part():
    from scOT.model import resize_operator
    nimg = args.nimg
    for s, t in SHAPES:
        pr64, pi64 = resize_operator(s, t)
        pr, pi = (torch.as_tensor(a, dtype=torch.float32).contiguous().cuda() for a in (pr64, pi64))
        cat = torch.cat([pr, pi], 0).contiguous()
        g = torch.Generator().manual_seed(17 * s + t)
        X = torch.randn(nimg, s, s, generator=g).cuda()
        U = torch.empty(nimg * s, 2 * t, dtype=torch.float32, device="cuda")
        Y_pair, Y_fused = torch.empty(nimg, t, t, device="cuda"), torch.empty(nimg, t, t, device="cuda")

        def pair():
            ops.linear_fwd(ops.F32, X.view(nimg * s, s), cat, U)
            ops.spectral_apply(U, pr, pi, Y_pair, nimg, s, t)

        def fused():
            ops.spectral_resize(X, pr, pi, Y_fused, nimg, s, t)
        times, counts = alternate({"pair": pair, "fused": fused})
        # both outputs against fp64 on the same fp32 operands, per element (tests/spectral_resize_cases.py: K1's bound)
        x, a, b = X.double(), pr.double(), pi.double()
        ref = a @ x @ a.T - b @ x @ b.T
        bound = (3 * s + 4) * U32 * (a.abs() @ x.abs() @ a.abs().T + b.abs() @ x.abs() @ b.abs().T)
        worst = {k: float(((y.double() - ref).abs() / bound).max()) for k, y in (("pair", Y_pair), ("fused", Y_fused))}
        flops, nbytes = 4.0 * t * s * (s + t) * nimg, 4.0 * (s * s + t * t) * nimg
        roof_flops_us, roof_bytes_us = flops / PEAK_F32_MFMA * 1e6, nbytes / PEAK_HBM * 1e6
        roof = max(roof_flops_us, roof_bytes_us)
        us = {k: [round(v * 1e3, 2) for v in vs] for k, vs in times.items()}
        print(json.dumps(dict(part="kernel", s=s, t=t, nimg=nimg, us_pair=us["pair"], us_fused=us["fused"], launches=counts,
                              speedup=[round(p / f, 3) for p, f in zip(us["pair"], us["fused"])],
                              worst_error_over_bound=worst, within_bound=all(v <= 1.0 for v in worst.values()),
                              roof_flops_us=round(roof_flops_us, 2), roof_bytes_us=round(roof_bytes_us, 2),
                              binds="flops" if roof_flops_us >= roof_bytes_us else "bytes",
                              fused_share_of_roof=[round(roof / v, 3) for v in us["fused"]],
                              fused_TFLOPs=[round(flops / (v * 1e-6) / 1e12, 1) for v in us["fused"]],
                              pair_intermediate_MB=round(U.numel() * 4 / 1e6, 1), GPU_MAX_HW_QUEUES=os.environ.get("GPU_MAX_HW_QUEUES"))), flush=True)
        assert all(v <= 1.0 for v in worst.values()), worst


def plan_part():
    from poseidon_amd.config import preset
    from poseidon_amd.plan import Plan
    from scOT.model import ScOT
    B = args.batch
    cfg = preset("B", image_size=128, num_channels=4, num_out_channels=4, channel_slice_list_normalized_loss=[0, 1, 3, 4])
    torch.manual_seed(1234)
    model = ScOT(cfg, compute="fp16").to("cuda").eval()
    model.fused_resize = True
    stream = torch.cuda.current_stream().cuda_stream
    plans, cases, keep = {}, {}, []
    with torch.no_grad():
        for r in (128, 256, 64):
            pv, t = torch.randn(B, 4, r, r, device="cuda"), torch.rand(B, device="cuda")
            plan = Plan.load(model.export_plan(pv, time=t, resize=True))
            out = torch.empty(B, 4, r, r, device="cuda")
            keep.append((pv, t, out))
            plans[r] = plan
            cases[f"r{r}"] = (lambda plan=plan, pv=pv, t=t, out=out: plan.run(pv.data_ptr(), t.data_ptr(), out=out.data_ptr(), stream=stream))
        times, counts = alternate(cases)
    ms = {k: [round(v, 3) for v in vs] for k, vs in times.items()}
    res = dict(part="plan", model="Poseidon-B", compute="fp16", batch=B, native=128, ms_per_run=ms, runs=counts,
               describe_resize={f"r{r}": plans[r].describe_resize() for r in plans},
               resize_adds_ms={k: [round(a - b, 3) for a, b in zip(ms[k], ms["r128"])] for k in ("r256", "r64")},
               resize_share_of_run={k: [round((a - b) / a, 3) for a, b in zip(ms[k], ms["r128"])] for k in ("r256", "r64")},
               nonfinite=int(sum((~torch.isfinite(o)).sum() for _, _, o in keep)), GPU_MAX_HW_QUEUES=os.environ.get("GPU_MAX_HW_QUEUES"))
    for plan in plans.values():
        plan.free()
    print(json.dumps(res), flush=True)


kernel_part() if args.part == "kernel" else plan_part()
