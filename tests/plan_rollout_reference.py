"""The two Python references of the rollout's adjoint (scot_plan_rollout_vjp / Plan.rollout_vjp), shared by the emulated and the GPU
tests.  Both run the Python engine through the public API with every parameter frozen and `model.eval()`; neither touches a plan.

R1  the explicit chain rule: one `torch.autograd.grad` per step, from the last step to the first, each at that step's input
    cat(predictions[k-1], pixel_values[:, Cout:]) and at time / steps, with the cotangent d_predictions[k] + g_{k+1}[:, :Cout]; the
    pass-through channels and the time gradient summed as ((x_{K-1} + x_{K-2}) + ...) + x_0, the time gradient then divided by steps.
    The plan has to give these bits.
R2  one `torch.autograd.grad` through `harness.rollout(..., output_all_steps=True, detach=False)`.  Autograd adds the same terms in an
    order of its own, so R2 equals R1 bit for bit where there is one term (the first Cout channels) and up to the association of an
    n-term fp32 sum elsewhere: two recursive sums of the same n terms each lie within (n-1) * 2^-24 * sum|term| of the exact sum, so they
    differ by at most 2 * (n-1) * 2^-24 * sum|term| (`association_bound`; the terms are R1's)."""
import torch

from poseidon_amd import harness


def forward_chain(model, pv, t, steps):
    """-> (R2's graph output [B, steps, Cout, H, W], the leaves it hangs on)"""
    a, b = pv.clone().requires_grad_(True), t.clone().requires_grad_(True)
    out = harness.rollout(model, dict(pixel_values=a, time=b), ar_steps=steps, output_all_steps=True, detach=False).output
    return out, (a, b)


def r2(model, pv, t, d_preds):
    """-> (predictions, d_pixel_values, d_time) by autograd through the attached rollout"""
    out, leaves = forward_chain(model, pv, t, d_preds.shape[1])
    d_pv, d_t = torch.autograd.grad(out, leaves, grad_outputs=d_preds)
    return out.detach().clone(), d_pv.clone(), d_t.clone()


def r1(model, pv, t, preds, d_preds):
    """-> (d_pixel_values, d_time, terms): the chain of single-step gradients at the step inputs `preds` gives, summed in the contract's
    order; terms = (the per-step terms of the pass-through channels, those of d_time), for `association_bound`"""
    steps, cout = d_preds.shape[1], model.config.num_out_channels
    t_step = t / steps
    carry, passed, tau = None, None, None
    pass_terms, tau_terms = [], []
    for k in range(steps - 1, -1, -1):
        x = pv if k == 0 else torch.cat([preds[:, k - 1], pv[:, cout:]], dim=1)
        a, b = x.clone().requires_grad_(True), t_step.clone().requires_grad_(True)
        out = model(pixel_values=a, time=b).output
        cot = d_preds[:, k] if carry is None else d_preds[:, k] + carry
        g, tk = torch.autograd.grad(out, (a, b), grad_outputs=cot.contiguous())
        carry = g[:, :cout]
        passed = g[:, cout:].clone() if passed is None else passed + g[:, cout:]
        tau = tk.clone() if tau is None else tau + tk
        pass_terms.append(g[:, cout:].clone())
        tau_terms.append(tk / steps)
    return torch.cat([carry, passed], dim=1).contiguous(), tau / steps, (pass_terms, tau_terms)


def association_bound(terms):
    """elementwise 2 * (n-1) * 2^-24 * sum_k |term_k|, in float64"""
    n = len(terms)
    return 2.0 * (n - 1) * 2.0 ** -24 * torch.stack([x.double().abs() for x in terms]).sum(0)


def assert_r2_within_bound(ref1, ref2, terms, cout, label=""):
    """R2 against R1: the first Cout channels bit for bit, the pass-through channels and d_time within the association bound"""
    d_pv1, d_t1 = ref1
    d_pv2, d_t2 = ref2
    assert torch.equal(d_pv2[:, :cout], d_pv1[:, :cout]), f"{label}: d_pixel_values[:, :Cout] of R2 differs from R1"
    for name, x1, x2, tm in (("pass-through channels", d_pv1[:, cout:], d_pv2[:, cout:], terms[0]), ("d_time", d_t1, d_t2, terms[1])):
        if x1.numel() == 0:
            continue
        err, bound = (x2.double() - x1.double()).abs(), association_bound(tm)
        print(f"[{label}] {name}: max |R2 - R1| {float(err.max()):.3e}, max bound {float(bound.max()):.3e}, "
              f"max error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), f"{label}: {name} of R2 leaves the association bound around R1"
