"""Gradients with respect to `pixel_values` and `time` — the engine and every kernel on the CPU emulation (tests/hipemu), against
the real reference's fixtures (tests/golden/make_input_grads_fixture.py) and the fp64 autograd of the oracle.

Bounds.  fp32: rel-L2 2e-4 — three times the reference's own fp32 noise (the real reference against the fp64 oracle is at most 6.7e-5
on these configurations, the fp32 oracle against the fp64 oracle at most 6.5e-5).  Reduced precision: the bounds
tests/test_model_emu_cpu.py applies to parameter gradients (bf16x3 2e-3, fp16 5e-2, bf16 0.7); between two forms of a layer tail:
the bounds those tests use between forms (fp16 1e-2, bf16 5e-2)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
from conftest import load_fixture, rel_l2  # noqa: E402
from oracle import scot_cpu  # noqa: E402
from poseidon_amd import engine as engine_mod, ops  # noqa: E402
from poseidon_amd.config import ScOTConfig  # noqa: E402
from poseidon_amd.geometry import param_shapes  # noqa: E402
from poseidon_amd.synth import synth_inputs, synth_state_dict  # noqa: E402

TOL32 = 2e-4
BOTH = ("pixel_values", "time")


@pytest.fixture()
def emu(monkeypatch):
    import emu_session
    lib = emu_session.load_emu()
    emu_session.patch_ops(monkeypatch, lib)
    monkeypatch.setenv("SCOT_SIDE_STREAM", "0")
    monkeypatch.setenv("SCOT_TAPE", "0")
    monkeypatch.setitem(engine_mod.ENGINE_OPTIONS, "fused_min_rows", 0)
    return lib


def fixture_inputs(meta, cfg):
    size = meta.get("size", cfg.image_size)
    pv, t, lab = synth_inputs(meta["batch"], cfg.num_channels, cfg.num_out_channels, size, meta["kind"])
    pm = None
    if meta.get("with_mask"):
        pm = torch.zeros(meta["batch"], cfg.num_out_channels, dtype=torch.bool)
        pm[:, -1] = True
    return pv, (t if cfg.use_conditioning else None), lab, pm


def make_model(cfg, sd, compute, options=None):
    from scOT.model import ScOT
    model = ScOT(cfg, compute=compute, engine_options=options)
    model.load_state_dict(sd)
    model._ensure_arena(torch.device("cpu"))
    return model


def step(model, pv, t, lab, pm, input_grads=BOTH, param_grads=True, **fw):
    """one forward + backward through the engine -> (loss, pred, d_pixel_values, d_time, tape)"""
    eng = model._engine
    kw = dict(input_grads=input_grads, param_grads=param_grads) if input_grads is not None else {}
    loss, pred, tape = eng.forward(pv, t, lab, pm, train=True, **kw, **fw)
    if param_grads:
        model._prepare_grads()
    res = eng.backward(tape, torch.ones(1), None)
    d_pv, d_t = res if res is not None else (None, None)
    return loss, pred, d_pv, d_t, tape


def oracle_grads(cfg, sd, pv, t, lab, pm, drop_masks=None, dtype=torch.float64):
    sd_ = {k: v.to(dtype) for k, v in sd.items()}
    pv_ = pv.to(dtype).requires_grad_(True)
    t_ = t.to(dtype).requires_grad_(True) if t is not None else None
    loss, _ = scot_cpu.scot_forward(sd_, cfg, pv_, t_, lab.to(dtype), pm, drop_masks=drop_masks)
    g = torch.autograd.grad(loss, [pv_] + ([t_] if t_ is not None else []))
    return g[0].detach(), (g[1].detach() if t_ is not None else None)


def grads_global(model, f):
    num = den = 0.0
    for k, p in model.named_parameters():
        if "grad:" + k in f.files:
            ref = f["grad:" + k].astype(np.float64)
            num += float(((p.grad.numpy().astype(np.float64) - ref) ** 2).sum())
            den += float((ref ** 2).sum())
    return (num / max(den, 1e-300)) ** 0.5


def launches(fn):
    """names (and, for scot_gemm, layouts) of the C-ABI launches fn() issues"""
    log = []
    prev = ops.set_recorder(log)
    try:
        fn()
    finally:
        ops.set_recorder(prev)
    return [(f.__name__, a[0] if f.__name__ == "scot_gemm" else None) for f, a in log if a is not None]


# ------------------------------------------------------------------------------------------------------------- fp32, the reference's fixtures
@pytest.mark.parametrize("name", ["tiny_trained", "tiny_odd", "tiny_shift3", "tiny_learnres_mask", "tiny_nocond_p2"])
def test_input_grads_fp32_vs_reference_fixture(emu, name):
    f, meta = load_fixture("igrad_" + name)
    fp, _ = load_fixture(name)                       # the parameter gradients of the same step (make_fixtures.py)
    cfg = ScOTConfig(**meta["cfg"])
    pv, t, lab, pm = fixture_inputs(meta, cfg)
    sd = synth_state_dict(param_shapes(cfg), meta["regime"])
    model = make_model(cfg, sd, "fp32")
    loss, pred, d_pv, d_t, _ = step(model, pv, t, lab, pm)
    o_pv, o_t = oracle_grads(cfg, sd, pv, t, lab, pm)
    e = dict(pv_fix=rel_l2(d_pv.numpy(), f["grad:pixel_values"]), pv_orc=rel_l2(d_pv.numpy(), o_pv.numpy()),
             orc_fix=rel_l2(o_pv.numpy(), f["grad:pixel_values"]))
    if cfg.use_conditioning:
        e.update(t_fix=rel_l2(d_t.numpy(), f["grad:time"]), t_orc=rel_l2(d_t.numpy(), o_t.numpy()), t_orc_fix=rel_l2(o_t.numpy(), f["grad:time"]))
    else:
        assert d_t is None and "grad:time" not in f.files
    print(f"\n[{name}] " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert abs(float(loss) - float(f["loss"])) < 2e-5 * abs(float(f["loss"]))
    assert all(v < TOL32 for v in e.values()), e
    assert tuple(d_pv.shape) == tuple(pv.shape)
    assert grads_global(model, fp) < 1e-4            # the parameter gradients of the same backward: their bound still holds


@pytest.mark.parametrize("compute,tol", [("bf16x3", 2e-3), ("fp16", 5e-2), ("bf16", 0.7)])
def test_input_grads_reduced_precision(emu, compute, tol):
    f, meta = load_fixture("igrad_tiny_trained")
    cfg = ScOTConfig(**meta["cfg"])
    pv, t, lab, pm = fixture_inputs(meta, cfg)
    model = make_model(cfg, synth_state_dict(param_shapes(cfg), meta["regime"]), compute)
    _, _, d_pv, d_t, _ = step(model, pv, t, lab, pm)
    e_pv, e_t = rel_l2(d_pv.numpy(), f["grad:pixel_values"]), rel_l2(d_t.numpy(), f["grad:time"])
    print(f"\n[{compute}] d_pixel_values {e_pv:.2e} d_time {e_t:.2e}")
    assert e_pv < tol and e_t < tol
    if compute == "fp16":
        assert model._engine.scale_grads and int(model._engine.grad_overflow) == 0


# ------------------------------------------------------------------------------------------------------------- every form of the layer tail
def wide_cfg(embed=96, image=64, depths=(1, 1), window=16, mlp_ratio=4.0):
    return ScOTConfig(image_size=image, patch_size=4, num_channels=4, num_out_channels=4, embed_dim=embed, depths=list(depths), num_heads=[3, 6],
                      skip_connections=[1, 0], window_size=window, mlp_ratio=mlp_ratio, qkv_bias=True, drop_path_rate=0.0, hidden_act="gelu", p=1,
                      channel_slice_list_normalized_loss=[0, 1, 3, 4], residual_model="convnext", use_conditioning=True, learn_residual=False)


def run_form(cfg, sd, pv, t, lab, compute, options):
    """-> (forms the backward took, loss, pred, d_pv, d_t); also checks that asking for input gradients leaves the forward bit-identical"""
    model = make_model(cfg, sd, compute, options)
    l0, p0, _ = model._engine.forward(pv, t, lab, None, train=True)
    l0, p0 = l0.clone(), p0.clone()
    loss, pred, d_pv, d_t, tape = step(model, pv, t, lab, None)
    assert torch.equal(loss, l0) and torch.equal(pred, p0)
    forms = {r["blk"].dim: r["plan"].bwd for st in tape["enc"] + tape["dec"] for r in st[0]}
    if compute == "fp16":
        assert int(model._engine.grad_overflow) == 0
    return forms, loss, pred, d_pv, d_t


def compare_forms(res, ref_key, tol_forms, tol_mode, oracle):
    o_pv, o_t = oracle
    for k, (_, _, _, d_pv, d_t) in res.items():
        e = (rel_l2(d_pv.numpy(), res[ref_key][3].numpy()), rel_l2(d_t.numpy(), res[ref_key][4].numpy()),
             rel_l2(d_pv.numpy(), o_pv.numpy()), rel_l2(d_t.numpy(), o_t.numpy()))
        print(f"[{k}] vs {ref_key}: d_pv {e[0]:.2e} d_time {e[1]:.2e}; vs fp64 oracle: d_pv {e[2]:.2e} d_time {e[3]:.2e}")
        assert e[0] < tol_forms and e[1] < tol_forms and e[2] < tol_mode and e[3] < tol_mode, (k, e)


def test_input_grads_every_tail_form_c96(emu):
    """C = 96 / 192 in fp16: layer by layer, the projection pair + layer-by-layer MLP (hidden width not a multiple of 128), the whole
    tail in its stored form and in its lean form (16-bit pre-norm rows; the qkv-dgrad prologue is taken out of the tail)."""
    print()
    for ratio, variants in ((4.0, dict(layers=dict(fused_mlp=False), tail=dict(lean_tail=False), lean=dict())), (3.0, dict(layers=dict(fused_mlp=False), proj=dict()))):
        cfg = wide_cfg(depths=(2, 1), mlp_ratio=ratio)
        sd = synth_state_dict(param_shapes(cfg), "trained")
        pv, t, lab = synth_inputs(1, 4, 4, 64, "smooth")
        res = {}
        for want, opt in variants.items():
            res[want] = run_form(cfg, sd, pv, t, lab, "fp16", opt)
            assert set(res[want][0].values()) == {want}, (want, res[want][0])
        compare_forms(res, "layers", 1e-2, 5e-2, oracle_grads(cfg, sd, pv, t, lab, None))


def test_input_grads_every_tail_form_bf16(emu):
    """the configuration of test_engine_fused_block_kernels (batch 2) in bf16: layer by layer against the lean tail"""
    print()
    cfg = wide_cfg(depths=(1, 1))
    sd = synth_state_dict(param_shapes(cfg), "trained")
    pv, t, lab = synth_inputs(2, 4, 4, 64, "smooth")
    res = {}
    for want, opt in dict(layers=dict(fused_mlp=False), lean=dict()).items():
        res[want] = run_form(cfg, sd, pv, t, lab, "bf16", opt)
        assert set(res[want][0].values()) == {want}
    compare_forms(res, "layers", 5e-2, 0.7, oracle_grads(cfg, sd, pv, t, lab, None))


def test_input_grads_fused_tail_c48(emu):
    """the configuration of test_engine_fused_tails_c48: the stored-gelu' tail at C = 48 (fp16)"""
    print()
    cfg = wide_cfg(embed=48, image=32, depths=(2, 1), window=4)
    sd = synth_state_dict(param_shapes(cfg), "trained")
    pv, t, lab = synth_inputs(1, 4, 4, 32, "smooth")
    res = {}
    for want, opt in dict(layers=dict(fused_fwd48=False, fused_bwd48=False), tail=dict(fused_fwd48=True, fused_bwd48=True)).items():
        res[want] = run_form(cfg, sd, pv, t, lab, "fp16", opt)
        assert res[want][0][48] == want, res[want][0]
    compare_forms(res, "layers", 1e-2, 5e-2, oracle_grads(cfg, sd, pv, t, lab, None))


# ------------------------------------------------------------------------------------------------------------- drop path
def test_input_grads_with_drop_path(emu):
    f, meta = load_fixture("tiny_droppath")
    cfg = ScOTConfig(**meta["cfg"])
    sd = synth_state_dict(param_shapes(cfg), meta["regime"])
    pv, t, lab = synth_inputs(meta["batch"], cfg.num_channels, cfg.num_out_channels, cfg.image_size, meta["kind"])
    masks = {}
    for k in f.files:
        if k.startswith("mask:"):
            _, name, which = k.split(":")
            masks[(name, int(which))] = torch.from_numpy(f[k])
    assert any(float(m.min()) == 0.0 for m in masks.values())
    model = make_model(cfg, sd, "fp32")
    model._engine.drop_path_masks = masks
    loss, _, d_pv, d_t, _ = step(model, pv, t, lab, None, stochastic=True)
    assert abs(float(loss) - float(f["loss"])) < 2e-5 * abs(float(f["loss"]))
    o_pv, o_t = oracle_grads(cfg, sd, pv, t, lab, None, drop_masks=masks)
    e = rel_l2(d_pv.numpy(), o_pv.numpy()), rel_l2(d_t.numpy(), o_t.numpy())
    print(f"\n[drop path] d_pixel_values {e[0]:.2e} d_time {e[1]:.2e}")
    assert e[0] < TOL32 and e[1] < TOL32
    assert grads_global(model, f) < 1e-4


# ------------------------------------------------------------------------------------------------------------- frozen parameters / no request
WGRAD_ONLY = ("scot_wgrad_group", "scot_wgrad_mlp", "scot_colsum", "scot_conv5_wgrad", "scot_dwconv7_wgrad")


@pytest.mark.parametrize("name,compute", [("tiny_trained", "fp32"), ("tiny_learnres_mask", "fp32")])
def test_frozen_backward_is_the_same_data_chain(emu, name, compute):
    f, meta = load_fixture("igrad_" + name)
    cfg = ScOTConfig(**meta["cfg"])
    pv, t, lab, pm = fixture_inputs(meta, cfg)
    sd = synth_state_dict(param_shapes(cfg), meta["regime"])
    ref = step(make_model(cfg, sd, compute), pv, t, lab, pm)
    model = make_model(cfg, sd, compute)
    out = {}
    names = launches(lambda: out.update(r=step(model, pv, t, lab, pm, param_grads=False)))
    loss, pred, d_pv, d_t, _ = out["r"]
    assert torch.equal(loss, ref[0]) and torch.equal(pred, ref[1])
    assert torch.equal(d_pv, ref[2]) and torch.equal(d_t, ref[3])               # bit for bit
    assert all(p.grad is None for p in model.parameters())
    assert not [n for n in names if n[0] in WGRAD_ONLY or n == ("scot_gemm", ops.TN)], sorted(set(names))
    assert ("scot_cln_dtime", None) in names
    assert not model._engine.grads_are_zero and not model._engine.lazy_grads     # the arena counts as dirty


def test_frozen_backward_fused_tails_fp16(emu):
    """the lean tails still write their norms' partial rows and the fp16 chain runs under the gradient scale: same input gradients as
    the training backward, no weight-gradient launch, and a training step afterwards starts from a cleared arena"""
    import scOT.model as M
    cfg = wide_cfg(depths=(1, 1))
    sd = synth_state_dict(param_shapes(cfg), "trained")
    pv, t, lab = synth_inputs(1, 4, 4, 64, "smooth")
    ref_model = make_model(cfg, sd, "fp16")
    ref = step(ref_model, pv, t, lab, None)
    g_ref = ref_model._arena.grad.clone()
    model = make_model(cfg, sd, "fp16")
    out = {}
    names = launches(lambda: out.update(r=step(model, pv, t, lab, None, param_grads=False)))
    assert torch.equal(out["r"][2], ref[2]) and torch.equal(out["r"][3], ref[3])
    assert not [n for n in names if n[0] in WGRAD_ONLY or n == ("scot_gemm", ops.TN)]
    assert int(model._engine.grad_overflow) == 0
    for p in model.parameters():          # what ScOT's backward does after a frozen step: nothing stays attached to the arena
        p.grad = None
    step(model, pv, t, lab, None, input_grads=())
    assert rel_l2(model._arena.grad.numpy(), g_ref.numpy()) < 1e-6


def test_no_request_issues_the_same_launches(emu):
    f, meta = load_fixture("igrad_tiny_trained")
    cfg = ScOTConfig(**meta["cfg"])
    pv, t, lab, pm = fixture_inputs(meta, cfg)
    sd = synth_state_dict(param_shapes(cfg), meta["regime"])
    for compute in ("fp32", "fp16"):
        m0, m1, m2 = (make_model(cfg, sd, compute) for _ in range(3))
        plain = launches(lambda: step(m0, pv, t, lab, pm, input_grads=None))
        explicit = launches(lambda: step(m1, pv, t, lab, pm, input_grads=()))
        asked = launches(lambda: step(m2, pv, t, lab, pm))
        assert "scot_cln_dtime" not in [n for n, _ in plain] and len(plain) == len(explicit) and plain == explicit
        assert [n for n, _ in asked].count("scot_cln_dtime") > 10 and len(asked) > len(plain)
        assert torch.equal(m0._arena.grad, m2._arena.grad)      # and the parameter gradients do not notice the request


# ------------------------------------------------------------------------------------------------------------- step tape
def test_input_grads_through_the_step_tape(emu, monkeypatch):
    f, meta = load_fixture("igrad_tiny_trained")
    cfg = ScOTConfig(**meta["cfg"])
    pv, t, lab, pm = fixture_inputs(meta, cfg)
    sd = synth_state_dict(param_shapes(cfg), meta["regime"])
    batches = [(pv * (1.0 + 0.1 * i), t + 0.05 * i, lab + 0.05 * i) for i in range(3)]
    plain = make_model(cfg, sd, "fp16")
    monkeypatch.setenv("SCOT_TAPE", "1")
    taped = make_model(cfg, sd, "fp16")
    assert taped._engine.tape_mode and not plain._engine.tape_mode
    got = []
    for i, b in enumerate(batches):
        taped.zero_grad()
        _, _, d_pv, d_t, _ = step(taped, b[0], b[1], b[2], None)
        got.append((d_pv, d_t, d_pv.clone(), d_t.clone()))
    ent = [e for e in taped._engine._taped.values() if e["state"] == "ready"]
    assert len(ent) == 1 and "igrads" in ent[0]          # step 2 recorded, step 3 replayed
    plain.zero_grad()
    _, _, r_pv, r_t, _ = step(plain, *batches[2], None)
    assert rel_l2(got[2][0].numpy(), r_pv.numpy()) < 1e-6 and rel_l2(got[2][1].numpy(), r_t.numpy()) < 1e-6
    assert rel_l2(taped._arena.grad.numpy(), plain._arena.grad.numpy()) < 1e-6
    assert torch.equal(got[1][0], got[1][2]) and torch.equal(got[1][1], got[1][3])      # step 2's tensors survived the replay
    assert not torch.equal(got[1][0], got[2][0])
    # another request is another signature: it does not replay this recording
    _, _, d_pv, d_t, _ = step(taped, *batches[2], None, input_grads=("pixel_values",))
    assert d_t is None and rel_l2(d_pv.numpy(), r_pv.numpy()) < 1e-6


# ------------------------------------------------------------------------------------------------------------- public API
def test_public_api_input_gradients(emu, monkeypatch):
    """ScOT.forward / loss.backward() on the emulation (the HIP-only guard patched out, as test_output_attentions_match_reference does):
    leaf gradients, the frozen model, a broadcast scalar time, the refusals."""
    import scOT.model as M
    monkeypatch.setattr(M, "_require_hip", lambda t: None)
    f, meta = load_fixture("igrad_tiny_trained")
    cfg = ScOTConfig(**meta["cfg"])
    pv, t, lab, pm = fixture_inputs(meta, cfg)
    sd = synth_state_dict(param_shapes(cfg), meta["regime"])
    fp, _ = load_fixture("tiny_trained")

    model = M.ScOT(cfg, compute="fp32")
    model.load_state_dict(sd)
    a, b = pv.clone().requires_grad_(True), t.clone().requires_grad_(True)
    out = model(pixel_values=a, time=b, labels=lab)
    out.loss.backward()
    assert rel_l2(a.grad.numpy(), f["grad:pixel_values"]) < TOL32 and rel_l2(b.grad.numpy(), f["grad:time"]) < TOL32
    assert grads_global(model, fp) < 1e-4
    g_train = model._arena.grad.clone()

    # frozen: the inference path would have no grad_fn; here the backward works and leaves every .grad None
    for p in model.parameters():
        p.requires_grad_(False)
    a2, b2 = pv.clone().requires_grad_(True), t.clone().requires_grad_(True)
    out = model(pixel_values=a2, time=b2, labels=lab)
    assert out.loss.grad_fn is not None
    out.loss.backward()
    assert torch.equal(a2.grad, a.grad) and torch.equal(b2.grad, b.grad)
    assert all(p.grad is None for p in model.parameters())
    with torch.no_grad():
        assert model(pixel_values=a2, time=b2, labels=lab).loss.grad_fn is None
    # ... and nothing requested at all is still the inference path
    assert model(pixel_values=pv, time=t, labels=lab).loss.grad_fn is None
    # un-frozen again: the arena the frozen backward may have written into is cleared before it is used
    for p in model.parameters():
        p.requires_grad_(True)
    model(pixel_values=pv, time=t, labels=lab).loss.backward()
    assert rel_l2(model._arena.grad.numpy(), g_train.numpy()) < 1e-6

    # a 0-dim time is broadcast over the batch: its gradient is the sum; only `time` asked for
    ts = torch.tensor(0.3, requires_grad=True)
    model(pixel_values=pv, time=ts, labels=lab).loss.backward()
    tb = torch.full((pv.shape[0],), 0.3, requires_grad=True)
    model(pixel_values=pv, time=tb, labels=lab).loss.backward()
    assert ts.grad.shape == () and abs(float(ts.grad) - float(tb.grad.sum())) <= 1e-6 * float(tb.grad.abs().sum())
    # the gradient of the prediction (no labels): a caller's own loss
    a3 = pv.clone().requires_grad_(True)
    pred = model(pixel_values=a3, time=t).output
    ((pred - lab) ** 2).mean().backward()
    o_pv, _ = oracle_grads(ScOTConfig(**dict(meta["cfg"], p=2, channel_slice_list_normalized_loss=None)), sd, pv, t, lab, None)
    assert rel_l2(a3.grad.numpy(), o_pv.numpy()) < TOL32

    # refusals
    with pytest.raises(NotImplementedError):
        model(pixel_values=pv, time=t, labels=lab.clone().requires_grad_(True))
    a4 = pv.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(model(pixel_values=a4, time=t, labels=lab).loss, a4, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


# ------------------------------------------------------------------------------------------------------------- the corners of the pixel chain
def test_mask_tokens_and_absolute_positions(emu):
    """bool_masked_pos: a masked token's embedding is the mask token, so no pixel (and no time) gradient flows through its patch;
    use_absolute_embeddings: the position table is added behind the norm and changes nothing upstream.  Against the oracle's fp64 autograd."""
    from poseidon_amd.synth import synth_token_mask
    _, meta = load_fixture("tiny_masktoken")
    cfg = ScOTConfig(**dict(meta["cfg"], use_absolute_embeddings=True))
    pv, t, lab, _ = fixture_inputs(meta, cfg)
    bmp = synth_token_mask(meta["batch"], (cfg.image_size // cfg.patch_size) ** 2)
    sd = synth_state_dict(param_shapes(cfg, use_mask_token=True), meta["regime"])
    from scOT.model import ScOT
    model = ScOT(cfg, compute="fp32", use_mask_token=True)
    model.load_state_dict(sd)
    model._ensure_arena(torch.device("cpu"))
    _, _, d_pv, d_t, _ = step(model, pv, t, lab, None, bool_masked_pos=bmp)
    sd64 = {k: v.double() for k, v in sd.items()}
    a, b = pv.double().requires_grad_(True), t.double().requires_grad_(True)
    loss, _ = scot_cpu.scot_forward(sd64, cfg, a, b, lab.double(), None, bool_masked_pos=bmp)
    o_pv, o_t = torch.autograd.grad(loss, [a, b])
    assert rel_l2(d_pv.numpy(), o_pv.numpy()) < TOL32 and rel_l2(d_t.numpy(), o_t.numpy()) < TOL32
    p = cfg.patch_size
    g = cfg.image_size // p
    patches = d_pv.view(meta["batch"], cfg.num_channels, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(meta["batch"], g * g, -1)
    m = bmp.reshape(meta["batch"], -1).bool()
    assert m.any() and float(patches[m].abs().max()) == 0.0 and float(patches[~m].abs().max()) > 0.0


def test_callers_gradient_of_the_prediction_respects_the_pixel_mask(emu, monkeypatch):
    """learn_residual + pixel_mask + a caller's own gradient of the returned prediction on top of the loss: where the mask overwrote the
    prediction with the label nothing upstream sees a gradient — neither the model nor the residual path into pixel_values."""
    import scOT.model as M
    monkeypatch.setattr(M, "_require_hip", lambda t: None)
    f, meta = load_fixture("igrad_tiny_learnres_mask")
    cfg = ScOTConfig(**meta["cfg"])
    pv, t, lab, pm = fixture_inputs(meta, cfg)
    sd = synth_state_dict(param_shapes(cfg), meta["regime"])
    w = torch.linspace(-1.0, 1.0, lab.numel()).view_as(lab)
    model = M.ScOT(cfg, compute="fp32")
    model.load_state_dict(sd)
    a, b = pv.clone().requires_grad_(True), t.clone().requires_grad_(True)
    out = model(pixel_values=a, time=b, labels=lab, pixel_mask=pm)
    (out.loss + (out.output * w).sum() * 1e-3).backward()
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    a64, b64 = pv.double().requires_grad_(True), t.double().requires_grad_(True)
    loss, pred = scot_cpu.scot_forward(sd64, cfg, a64, b64, lab.double(), pm)
    (loss + (pred * w.double()).sum() * 1e-3).backward()
    assert rel_l2(a.grad.numpy(), a64.grad.numpy()) < TOL32 and rel_l2(b.grad.numpy(), b64.grad.numpy()) < TOL32
    num = den = 0.0
    for k, p_ in model.named_parameters():
        num += float((p_.grad.double() - sd64[k].grad).norm()) ** 2
        den += float(sd64[k].grad.norm()) ** 2
    assert (num / den) ** 0.5 < 1e-4
