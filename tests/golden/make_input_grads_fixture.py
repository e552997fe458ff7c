"""Input-gradient fixtures from the REAL reference (run where the reference is installed; it does not travel):

  igrad_<name>.npz — `loss`, `grad:pixel_values` and (with conditioning) `grad:time` of
  `torch.autograd.grad(loss, [pixel_values, time])` through the reference's ScOT.forward, for the configurations of
  make_fixtures.py whose parameter gradients are pinned already: TINY, tiny_odd, tiny_shift3, tiny_learnres_mask (with its pixel
  mask), tiny_nocond_p2 (no time), the 64x64 input to the 32x32 model (spectral-resize path) and Poseidon-T at batch 2.

Parameters and inputs are closed form (poseidon_amd.synth), so only results are stored.  `build` / `synth_inputs` come from
make_fixtures.py unchanged.

usage: python tests/golden/make_input_grads_fixture.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as mf  # noqa: E402  (installs the API-drift shim and imports the reference)
from make_fixtures import MODEL_MAP, TINY, build, save, synth_inputs  # noqa: E402


def run(cfg_kw, regime, batch, kind="smooth", with_mask=False, size=None):
    cfg, model = build(cfg_kw, regime)
    size = size or cfg_kw["image_size"]
    pv, t, lab = synth_inputs(batch, cfg_kw["num_channels"], cfg_kw["num_out_channels"], size, kind)
    cond = bool(cfg_kw.get("use_conditioning", False))
    pv = pv.clone().requires_grad_(True)
    kw = dict(pixel_values=pv, labels=lab)
    if cond:
        t = t.clone().requires_grad_(True)
        kw["time"] = t
    if with_mask:
        pm = torch.zeros(batch, cfg_kw["num_out_channels"], dtype=torch.bool)
        pm[:, -1] = True
        kw["pixel_mask"] = pm
    out = model(**kw)
    grads = torch.autograd.grad(out.loss, [pv, t] if cond else [pv])
    res = {"loss": out.loss.detach().numpy(), "grad:pixel_values": grads[0].numpy()}
    if cond:
        res["grad:time"] = grads[1].numpy()
    return res


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    odd = dict(TINY, image_size=36)
    sh = dict(TINY, image_size=64, embed_dim=16, depths=[2, 2, 2], num_heads=[1, 2, 4], skip_connections=[2, 1, 0])
    nocond = dict(TINY, use_conditioning=False, channel_slice_list_normalized_loss=None, p=2)
    lr = dict(TINY, learn_residual=True, num_channels=5, channel_slice_list_normalized_loss=[0, 1, 3, 4])
    for name, kw, extra in (("tiny_trained", TINY, {}), ("tiny_odd", odd, {}), ("tiny_shift3", sh, {}),
                            ("tiny_learnres_mask", lr, dict(with_mask=True)), ("tiny_nocond_p2", nocond, {}),
                            ("tiny_resize64", TINY, dict(size=64))):
        res = run(kw, "trained", 2, **extra)
        save("igrad_" + name, res, dict(cfg=kw, regime="trained", batch=2, kind="smooth", **extra))
    kwT = dict(image_size=128, patch_size=4, num_channels=4, num_out_channels=4, num_heads=[3, 6, 12, 24],
               skip_connections=[2, 2, 2, 0], window_size=16, mlp_ratio=4.0, qkv_bias=True, drop_path_rate=0.0,
               hidden_act="gelu", p=1, channel_slice_list_normalized_loss=[0, 1, 3, 4], residual_model="convnext",
               use_conditioning=True, learn_residual=False, **MODEL_MAP["T"])
    res = run(kwT, "trained", 2)
    save("igrad_poseidonT_trained", res, dict(cfg=kwT, regime="trained", batch=2, kind="smooth"))


if __name__ == "__main__":
    main()
