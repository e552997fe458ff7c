"""scOT.metrics — evaluation metrics with the reference module's import path and function names
(reference scOT/metrics.py:4-55), plus the per-channel-group statistics the reference's inference driver derives from them
(reference scOT/inference.py:76-199, `compute_metrics`).

The reference works on numpy arrays after HF `Trainer.predict` has copied every prediction to the host.  These versions take
numpy arrays OR torch tensors; given GPU tensors (e.g. the `.output` of `scOT.trainer.rollout`) the reductions run on the
device and only the per-sample error vectors / the final statistics cross PCIe.  Semantics, including
the 1e-10 guard of an all-zero target and the percent scaling, are the reference's.

`error_sums` and the `*_from_sums` functions are the same metrics in two steps: one fused reduction of (prediction, target) to four
fp64 sums per sample and channel group — on the GPU the `scot_error_sums` kernel, which `Plan.evaluate` and
`Trainer.evaluate_on_device` also run — and the few flops per sample that turn the sums into the reference's numbers.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch


def _t(x) -> torch.Tensor:
    return x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))


def _like(res: torch.Tensor, ref_arg):
    """numpy in → numpy out (the reference's types); tensors stay tensors (and stay on their device)."""
    return res if isinstance(ref_arg, torch.Tensor) else res.cpu().numpy()


def _sums(preds, targets, p):
    pr, tg = _t(preds), _t(targets)
    n, c = pr.shape[0], pr.shape[1]
    pr, tg = pr.reshape(n, c, -1).to(torch.float64 if pr.dtype == torch.float64 else torch.float32), tg.reshape(n, c, -1)
    tg = tg.to(pr.dtype)
    err = (pr - tg).abs().pow(p).sum(-1).sum(-1)          # Σ_channels Σ_pixels |pred - target|^p   per sample
    return err, tg


def lp_error(preds, targets, p=1):
    """(Σ_{c,x} |pred - target|^p)^(1/p) per sample → [num_samples]   (reference metrics.py:4-9)."""
    err, _ = _sums(preds, targets, p)
    return _like(err.pow(1.0 / p), preds)


def relative_lp_error(preds, targets, p=1, return_percent=True):
    """lp_error / (Σ_{c,x} |target|^p)^(1/p) per sample, in percent by default; a zero denominator is replaced by 1e-10
    (reference metrics.py:12-36)."""
    err, tg = _sums(preds, targets, p)
    norm = tg.abs().pow(p).sum(-1).sum(-1)
    norm = torch.where(norm == 0, torch.full_like(norm, 1e-10), norm)
    res = (err / norm).pow(1.0 / p)
    if return_percent:
        res = res * 100
    return _like(res, preds)


def mean_relative_lp_error(preds, targets, p=1, return_percent=True):
    e = relative_lp_error(preds, targets, p, return_percent)
    return e.mean(0) if isinstance(e, torch.Tensor) else np.mean(e, axis=0)


def median_relative_lp_error(preds, targets, p=1, return_percent=True):
    e = relative_lp_error(preds, targets, p, return_percent)
    if isinstance(e, torch.Tensor):   # numpy's median averages the two middle elements of an even-sized sample
        return torch.quantile(e.to(torch.float64), 0.5, dim=0, interpolation="midpoint").to(e.dtype)
    return np.median(e, axis=0)


def _stats(e: torch.Tensor, suffix: str) -> Dict[str, float]:
    e64 = e.to(torch.float64)
    return {
        "median_" + suffix: float(torch.quantile(e64, 0.5, interpolation="midpoint")),
        "mean_" + suffix: float(e64.mean()),
        "std_" + suffix: float(e64.std(unbiased=False)),      # np.std: population standard deviation
        "min_" + suffix: float(e64.min()),
        "max_" + suffix: float(e64.max()),
    }


def channel_group_metrics(preds, targets, channel_slice_list: Sequence[int], channel_names: Optional[Sequence[str]] = None,
                          full_data: bool = False) -> Dict[str, object]:
    """The dictionary the reference's `compute_metrics` returns (inference.py:76-199): relative and absolute L1 errors per
    channel group `[channel_slice_list[i], channel_slice_list[i+1])`, their median/mean/std/min/max over samples, and — for more
    than one group — the means over groups (`mean_relative_l1_error` = mean over the groups' means, ...).  `channel_names` are the
    dataset's `printable_channel_description`."""
    pr, tg = _t(preds), _t(targets)
    groups = [(channel_slice_list[i], channel_slice_list[i + 1]) for i in range(len(channel_slice_list) - 1)]
    rel = [_t(relative_lp_error(pr[:, a:b], tg[:, a:b], p=1, return_percent=True)) for a, b in groups]
    ab = [_t(lp_error(pr[:, a:b], tg[:, a:b], p=1)) for a, b in groups]
    rel_stats = [_stats(e, "relative_l1_error") for e in rel]
    abs_stats = [_stats(e, "l1_error") for e in ab]
    if len(groups) == 1:
        out: Dict[str, object] = {**rel_stats[0], **abs_stats[0]}
        if full_data:
            out["relative_full_data"] = rel[0].tolist()
            out["full_data"] = ab[0].tolist()
        return out
    names = list(channel_names) if channel_names is not None else [f"group{i}" for i in range(len(groups))]
    out = {
        "mean_relative_l1_error": float(np.mean([s["mean_relative_l1_error"] for s in rel_stats])),
        "mean_over_median_relative_l1_error": float(np.mean([s["median_relative_l1_error"] for s in rel_stats])),
        "mean_l1_error": float(np.mean([s["mean_l1_error"] for s in abs_stats])),
        "mean_over_median_l1_error": float(np.mean([s["median_l1_error"] for s in abs_stats])),
    }
    for i, st in enumerate(rel_stats):
        for k, v in st.items():
            out[names[i] + "/" + k] = v
        if full_data:
            out[names[i] + "/relative_full_data"] = rel[i].tolist()
    for i, st in enumerate(abs_stats):
        for k, v in st.items():
            out[names[i] + "/" + k] = v
        if full_data:
            out[names[i] + "/full_data"] = ab[i].tolist()
    return out


# ---------------------------------------------------------------------------------------------------------------- from error sums
SUM_ABS_ERR, SUM_ABS, SUM_SQ_ERR, SUM_SQ = range(4)      # the last axis of error sums: S1, N1, S2, N2 (include/scot_plan.h)


def _mask_like(pixel_mask, pr):
    """the reference's pixel_mask against predictions [N, C, ...] -> (bool mask [N, C] or of pr's shape, whether it is element-wise):
    [N, C] masks whole planes; pr's own shape, or [N, 1, ...], masks elements (expanded over the channels)"""
    m = _t(pixel_mask)
    m = (m != 0) if m.dtype != torch.bool else m
    if m.dim() == 2 and tuple(m.shape) == tuple(pr.shape[:2]):
        return m, False
    if m.dim() == pr.dim() and m.shape[0] == pr.shape[0] and m.shape[1] in (1, pr.shape[1]) and m.shape[2:] == pr.shape[2:]:
        return m.expand(pr.shape), True
    raise ValueError(f"error_sums: pixel_mask of shape {tuple(m.shape)} against predictions {tuple(pr.shape)}")


def error_sums(preds, targets, channel_slice_list: Optional[Sequence[int]] = None, pixel_mask=None) -> torch.Tensor:
    """[N, G, 4] float64: per sample and channel group `[channel_slice_list[g], channel_slice_list[g+1])` (None: one group of all
    channels) the sums Σ|p−t|, Σ|t|, Σ(p−t)², Σt² over the group's channels and all pixels.  GPU tensors go through the
    `scot_error_sums` kernel (one pass over both operands, no temporaries; the result stays on the device); numpy arrays and CPU
    tensors use a plain fp64 computation.  Both convert the fp32 values to fp64 first, then subtract.
    pixel_mask (bool or uint8: [N, C] whole planes, or the predictions' shape, or [N, 1, ...] expanded over the channels): the sums of
    `where(pixel_mask, targets, preds)`, what the reference scores after `prediction[pixel_mask] = labels[pixel_mask]` — on the GPU by
    `scot_error_sums_masked` in the same pass (the predictions are not modified)."""
    pr, tg = _t(preds), _t(targets)
    if pr.shape != tg.shape or pr.dim() < 2:
        raise ValueError(f"error_sums: predictions {tuple(pr.shape)} against targets {tuple(tg.shape)}")
    n, c = pr.shape[0], pr.shape[1]
    slices = [0, c] if channel_slice_list is None else [int(s) for s in channel_slice_list]
    if len(slices) < 2 or slices[0] < 0 or slices[-1] > c or any(b <= a for a, b in zip(slices, slices[1:])):
        raise ValueError(f"error_sums: channel slices {slices} over {c} channels")
    mask, mask_full = (None, False) if pixel_mask is None else _mask_like(pixel_mask, pr)
    if pr.is_cuda:
        from poseidon_amd import ops
        pr, tg = pr.to(torch.float32).contiguous(), tg.to(device=pr.device, dtype=torch.float32).contiguous()
        out = torch.empty(n, len(slices) - 1, 4, dtype=torch.float64, device=pr.device)
        if n:
            m8 = None if mask is None else mask.to(device=pr.device, dtype=torch.uint8).contiguous()
            ops.error_sums(pr, tg, None if channel_slice_list is None else slices, out, m8, mask_full)
        return out
    if mask is not None:
        mask = mask.to(pr.device)
        pr = torch.where(mask if mask_full else mask.reshape(n, c, *([1] * (pr.dim() - 2))), tg.to(pr.dtype), pr)
    pr, tg = pr.reshape(n, c, -1).to(torch.float64), tg.reshape(n, c, -1).to(torch.float64)
    d = pr - tg
    per_channel = torch.stack([d.abs().sum(-1), tg.abs().sum(-1), (d * d).sum(-1), (tg * tg).sum(-1)], -1)      # [N, C, 4]
    return torch.stack([per_channel[:, a:b].sum(1) for a, b in zip(slices, slices[1:])], 1)


def _sum_pair(sums, p):
    if p not in (1, 2):
        raise ValueError("error sums hold the terms of p = 1 and p = 2")
    s = _t(sums).to(torch.float64)
    return (s[..., SUM_ABS_ERR], s[..., SUM_ABS]) if p == 1 else (s[..., SUM_SQ_ERR], s[..., SUM_SQ])


def lp_error_from_sums(sums, p=1):
    """`lp_error` of every (sample, group) of `error_sums`' result: S^(1/p), shape sums.shape[:-1]."""
    err, _ = _sum_pair(sums, p)
    return _like(err.pow(1.0 / p), sums)


def relative_lp_error_from_sums(sums, p=1, return_percent=True):
    """`relative_lp_error` of every (sample, group): (S / N)^(1/p), in percent by default, N == 0 replaced by 1e-10."""
    err, norm = _sum_pair(sums, p)
    norm = torch.where(norm == 0, torch.full_like(norm, 1e-10), norm)
    res = (err / norm).pow(1.0 / p)
    if return_percent:
        res = res * 100
    return _like(res, sums)


def group_metrics_from_sums(sums, channel_names: Optional[Sequence[str]] = None, full_data: bool = False) -> Dict[str, object]:
    """The dictionary `channel_group_metrics` returns, with the same keys, from the [N, G, 4] sums of the same predictions, targets
    and channel slices: only the order statistics over the N samples are left to do."""
    s = _t(sums)
    if s.dim() != 3 or s.shape[-1] != 4:
        raise ValueError(f"group_metrics_from_sums: sums of shape [N, G, 4], not {tuple(s.shape)}")
    groups = s.shape[1]
    rel_all, ab_all = _t(relative_lp_error_from_sums(s, 1, True)), _t(lp_error_from_sums(s, 1))
    rel, ab = [rel_all[:, g] for g in range(groups)], [ab_all[:, g] for g in range(groups)]
    return _group_dictionary(rel, ab, channel_names, full_data)


def _group_dictionary(rel, ab, channel_names, full_data):
    """per-group relative and absolute L1 errors (one [N] tensor per group each) -> the dictionary of `channel_group_metrics`"""
    parts = [("relative_l1_error", "relative_full_data", rel), ("l1_error", "full_data", ab)]
    stats = {suffix: [_stats(e, suffix) for e in errs] for suffix, _, errs in parts}
    if len(rel) == 1:
        out: Dict[str, object] = {**stats["relative_l1_error"][0], **stats["l1_error"][0]}
        if full_data:
            out.update({data_key: errs[0].tolist() for _, data_key, errs in parts})
        return out
    names = list(channel_names) if channel_names is not None else [f"group{i}" for i in range(len(rel))]
    out = {}
    for suffix in ("relative_l1_error", "l1_error"):
        out["mean_" + suffix] = float(np.mean([st["mean_" + suffix] for st in stats[suffix]]))
        out["mean_over_median_" + suffix] = float(np.mean([st["median_" + suffix] for st in stats[suffix]]))
    for suffix, data_key, errs in parts:
        for i, st in enumerate(stats[suffix]):
            out.update({names[i] + "/" + k: v for k, v in st.items()})
            if full_data:
                out[names[i] + "/" + data_key] = errs[i].tolist()
    return out
