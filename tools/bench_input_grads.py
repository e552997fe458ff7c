"""Step time of a training step that also differentiates with respect to its inputs.

    python tools/bench_input_grads.py [--tag B] [--batch 64] [--size 128] [--compute fp16] [--steps 20] [--warmup 5]

Four cases of forward + backward through ScOT.forward / loss.backward() on the step tape (no optimizer; zero_grad(overlap=True) between
steps as the training loops do): parameter gradients only; plus d_pixel_values; plus d_pixel_values and d_time; every parameter
frozen with both input gradients (the surrogate inside an inverse problem).  Prints one line per case: the median step in ms over
`steps` steps timed with HIP events, and the number of C-ABI launches of the recorded backward.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poseidon_amd.config import preset  # noqa: E402
from poseidon_amd.geometry import param_shapes  # noqa: E402
from poseidon_amd.synth import synth_inputs, synth_state_dict  # noqa: E402
from scOT.model import ScOT  # noqa: E402


def run_case(name, cfg, sd, compute, batch, size, want_pv, want_t, frozen, steps, warmup):
    model = ScOT(cfg, compute=compute)
    model.load_state_dict(sd)
    model = model.to("cuda")
    model.train()
    if frozen:
        for p in model.parameters():
            p.requires_grad_(False)
    pv, t, lab = (x.to("cuda") for x in synth_inputs(batch, cfg.num_channels, cfg.num_out_channels, size, "smooth"))
    times = []
    for i in range(warmup + steps):
        a = pv.clone().requires_grad_(want_pv)
        b = t.clone().requires_grad_(want_t)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if not frozen:
            model.zero_grad(overlap=True)
        model(pixel_values=a, time=b, labels=lab).loss.backward()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1))
        assert (a.grad is not None) == want_pv and (b.grad is not None) == want_t
    ent = [e for e in model._engine._taped.values() if e.get("state") == "ready"]
    nb = sum(1 for _, args in next(iter(ent[0]["bwd"].values()))[0] if args is not None) if ent else -1
    ndt = sum(1 for fn, args in next(iter(ent[0]["bwd"].values()))[0] if args is not None and fn.__name__ == "scot_cln_dtime") if ent else -1
    ov = model._engine.grad_overflow
    print(f"{name:44s} {statistics.median(times):8.3f} ms/step (min {min(times):.3f}, max {max(times):.3f}; {steps} steps)   "
          f"backward launches {nb} (scot_cln_dtime {ndt})   grad_overflow {int(ov) if ov is not None else 0}", flush=True)
    del model
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="B")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--channels", type=int, default=4)
    ap.add_argument("--compute", default="fp16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    cfg = preset(a.tag, image_size=a.size, num_channels=a.channels, num_out_channels=a.channels,
                 channel_slice_list_normalized_loss=[0, 1, a.channels - 1, a.channels])
    sd = synth_state_dict(param_shapes(cfg), "trained")
    print(f"Poseidon-{a.tag} {a.size}x{a.size}x{a.channels} batch {a.batch} {a.compute}: forward + backward, step tape, no optimizer")
    for name, pvg, tg, frozen in (("parameters only", False, False, False), ("parameters + d_pixel_values", True, False, False),
                                  ("parameters + d_pixel_values + d_time", True, True, False),
                                  ("frozen: d_pixel_values + d_time", True, True, True)):
        run_case(name, cfg, sd, a.compute, a.batch, a.size, pvg, tg, frozen, a.steps, a.warmup)


if __name__ == "__main__":
    main()
