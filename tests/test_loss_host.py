"""Host-side half of the contrastive loss (clip_lora_match_amd.evaluate.loss_from_lse /
batched_loss, distributed.merge_lse) against tests/golden/contrastive_loss.npz, the reference's own
compute_clip_contrastive_loss on the fixture's inputs (tests/golden/make_loss_golden.py).

The combiner is fed fp64 torch.logsumexp rows of the fp64 cosine matrix, so what is tested is its
arithmetic: fp64 at N = 257 must meet the reference's fp64 loss within 1e-9, and its fp32 loss
within the gap the fixture recorded between the two plus 1e-9.
"""
import os

import numpy as np
import pytest
import torch

import clip_lora_match_amd as clm
from clip_lora_match_amd import distributed as D
from clip_lora_match_amd import evaluate as EV

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contrastive_loss.npz"))


def _cos64(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return (a / a.norm(dim=-1, keepdim=True)) @ (b / b.norm(dim=-1, keepdim=True)).T


def test_loss_combiner_matches_reference():
    T = float(GOLD["T"])
    S = _cos64(GOLD["a"], GOLD["b"])
    out = EV.loss_from_lse(torch.logsumexp(S / T, dim=1), torch.logsumexp(S / T, dim=0), S.diagonal(), T)
    assert set(out) == {"loss", "loss_i2t", "loss_t2i", "err"} and out["err"] == 0.0
    assert abs(out["loss"] - float(GOLD["loss64"])) <= 1e-9
    assert abs(out["loss"] - float(GOLD["loss32"])) <= float(GOLD["gap"]) + 1e-9
    assert abs(out["loss"] - (out["loss_i2t"] + out["loss_t2i"]) / 2) <= 1e-15
    # the bounds' mean is reported
    e = EV.loss_from_lse(torch.zeros(4), torch.zeros(4), torch.zeros(4), T, torch.full((4,), 2e-3, dtype=torch.float64),
                         torch.zeros(4))
    assert abs(e["err"] - 1e-3) <= 1e-12
    with pytest.raises(ValueError):
        EV.loss_from_lse(torch.zeros(3), torch.zeros(4), torch.zeros(4), T)
    with pytest.raises(ValueError):
        EV.loss_from_lse(torch.zeros(4), torch.zeros(4), torch.zeros(4), 0.0)


def test_batched_loss_matches_reference():
    """train_lora.py:213-241's number at B = 32: 8 full batches and one of a single pair"""
    T, B = float(GOLD["T"]), int(GOLD["B"])
    out = EV.batched_loss(GOLD["a"], GOLD["b"], T, B, scores=_cos64)
    assert abs(out["loss"] - float(GOLD["batch64"])) <= 1e-9
    assert abs(out["loss"] - float(GOLD["batch32"])) <= float(GOLD["batch_gap"]) + 1e-9
    # one batch of everything is the whole-set loss
    whole = EV.batched_loss(GOLD["a"], GOLD["b"], T, 257, scores=_cos64)
    assert abs(whole["loss"] - float(GOLD["loss64"])) <= 1e-9
    with pytest.raises(ValueError):
        EV.batched_loss(GOLD["a"], GOLD["b"], T, 0, scores=_cos64)


def test_merge_lse_three_way_split():
    g = torch.Generator().manual_seed(0)
    x = 30.0 * torch.randn(9, 1000, generator=g, dtype=torch.float64)
    cuts = [0, 137, 610, 1000]
    parts = [torch.logsumexp(x[:, cuts[i]:cuts[i + 1]], dim=1) for i in range(3)]
    lse, err = D.merge_lse(parts)
    assert (lse - torch.logsumexp(x, dim=1)).abs().max() <= 1e-12
    assert err.shape == lse.shape and err.abs().max() <= 1e-12
    # shard bounds combine share-weighted: between the weighted mean and the maximum
    errs = [torch.full((9,), 1e-3), torch.zeros(9), torch.full((9,), 4e-3)]
    _, e = D.merge_lse(parts, errs)
    w = torch.stack([torch.exp(p - lse) for p in parts])
    mean = (w * torch.stack(errs).double()).sum(dim=0)
    assert (e >= mean - 1e-12).all() and (e <= 4e-3 + 1e-12).all()
    with pytest.raises(ValueError):
        D.merge_lse(parts, errs[:2])


def test_package_exports_contrastive_loss():
    assert clm.contrastive_loss is EV.contrastive_loss
    assert "contrastive_loss" in clm.__all__ and "contrastive_loss" in EV.__all__
