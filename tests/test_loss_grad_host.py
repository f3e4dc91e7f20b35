"""Host-side half of the streaming contrastive-loss gradient: the numpy float64 restatement
(tests/loss_grad_ref.py) against the reference's own autograd gradients
(tests/golden/contrastive_loss_grad.npz, made by make_loss_grad_golden.py), and the O(N d) pieces of
clip_lora_match_amd.evaluate (unit_gradients, normalize_backward, loss_grad_from_sums) fed that
restatement's weighted sums. No GPU: the streamed sums themselves are tests/test_gpu_loss_grad.py's.
"""
import math
import os

import numpy as np
import pytest
import torch

import clip_lora_match_amd as clm
from clip_lora_match_amd import _capi
from clip_lora_match_amd import evaluate as EV
from clip_lora_match_amd import search as S
import loss_grad_ref as R

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contrastive_loss_grad.npz"))


def _rel(x, want):
    return float(np.abs(np.asarray(x) - want).max() / np.abs(want).max())


def test_reference_restatement_matches_autograd():
    """1e-12 relative to the largest gradient entry, both sides; the reference's own fp32 run sits
    within the recorded gap of its fp64 one"""
    a, b, T = GOLD["a"], GOLD["b"], float(GOLD["T"])
    ga, gb, aq, ar = R.contrastive_grad_ref(a, b, T)
    assert _rel(ga, GOLD["grad_a64"]) <= 1e-12 and _rel(gb, GOLD["grad_b64"]) <= 1e-12
    assert np.abs(GOLD["grad_a32"] - GOLD["grad_a64"]).max() <= float(GOLD["gap"])
    # a row's weight mass: its own softmax sums to 1, the other direction's share is positive
    assert (aq > 1).all() and (ar > 1).all() and abs(aq.sum() - 2 * 257) <= 1e-9 and abs(ar.sum() - 2 * 257) <= 1e-9


@pytest.mark.parametrize("chunk", [1, 64, 100, 256])
def test_reference_is_chunk_independent(chunk):
    a, b, T = GOLD["a"], GOLD["b"], float(GOLD["T"])
    whole = R.contrastive_grad_ref(a, b, T)
    part = R.contrastive_grad_ref(a, b, T, chunk=chunk)
    for w, p in zip(whole, part):
        assert _rel(p, w) <= 1e-13


def test_evaluate_helpers_reproduce_golden():
    """the package's O(N d) tail on the restatement's unit-vector sums, on CPU tensors"""
    a, b, T = GOLD["a"], GOLD["b"], float(GOLD["T"])
    au, bu = R.unit(a), R.unit(b)
    dq, dr, _, _ = R.softmax_grad_ref(au, bu, 1.0 / T, R.lse_rows(au, bu, 1.0 / T), R.lse_rows(bu, au, 1.0 / T))
    ga, gb = EV.loss_grad_from_sums(torch.from_numpy(dq), torch.from_numpy(dr), torch.from_numpy(a),
                                    torch.from_numpy(b), T)
    assert ga.dtype == torch.float64 and ga.shape == (257, 64)
    assert _rel(ga.numpy(), GOLD["grad_a64"]) <= 1e-12 and _rel(gb.numpy(), GOLD["grad_b64"]) <= 1e-12
    # the two pieces on their own
    ua, ub = EV.unit_gradients(torch.from_numpy(dq), torch.from_numpy(dr), torch.from_numpy(au), torch.from_numpy(bu), T)
    assert _rel(ua.numpy(), dq / (2 * 257 * T) - bu / (257 * T)) <= 1e-15
    nb = EV.normalize_backward(ua, torch.from_numpy(a)).numpy()
    assert _rel(nb, R.normalize_backward_ref(ua.numpy(), a)) <= 1e-14
    # a gradient through the normalisation has no component along the row
    assert np.abs((nb * a).sum(axis=1)).max() <= 1e-15 * np.abs(a).max() * 64


def test_one_directional_sums_are_softmax_readout():
    """wq = 1 without row_lse: dq = softmax(scale * s) @ ru and the masses are 1"""
    g = np.random.default_rng(3)
    qu, ru = R.unit(g.standard_normal((5, 16))), R.unit(g.standard_normal((40, 16)))
    dq, dr, aq, ar = R.softmax_grad_ref(qu, ru, 20.0, R.lse_rows(qu, ru, 20.0), None, 1.0, 0.0, chunk=7)
    p = torch.softmax(torch.from_numpy(20.0 * qu @ ru.T), dim=1).numpy()
    assert np.abs(dq - p @ ru).max() <= 1e-14 and np.abs(dr - p.T @ qu).max() <= 1e-14
    assert np.abs(aq - 1).max() <= 1e-14 and abs(ar.sum() - 5) <= 1e-13


def test_bounds_are_what_the_design_states():
    """softmax_grad_bound: the certified rho is led by expm1(scale * E) (0.0355 at 1 / 0.07, 0.28 at
    100), the tight one is a few 2^-11; both grow with the terms summed; tau is far below them"""
    assert abs(math.expm1(S.PASS_E / 0.07) - 0.0355) <= 1e-4 and abs(math.expm1(100 * S.PASS_E) - 0.2767) <= 1e-3
    for scale in (1 / 0.07, 100.0):
        rho, tau = S.softmax_grad_bound(scale, 3000)
        lead = math.expm1(scale * S.PASS_E)
        assert lead < rho <= (1 + lead) * (1 + 5 * 2.0 ** -11) - 1
        rt, tau_t = S.softmax_grad_bound(scale, 3000, dim=512)
        assert 2 * 2.0 ** -11 < rt < 4 * 2.0 ** -11 + math.expm1(scale * (512 * 2.0 ** -24 + 1e-6) * 1.5)
        assert tau == tau_t and 0 < tau < 1e-2 * rt
        assert S.softmax_grad_bound(scale, 10 ** 7)[0] > rho


def test_python_layer_argument_errors():
    a = torch.zeros(4, 8)
    for fn in (EV.contrastive_loss_grad, EV.contrastive_loss_tensor):
        with pytest.raises(ValueError):
            fn(a, torch.zeros(5, 8))
        with pytest.raises(ValueError):
            fn(a, torch.zeros(4, 8), temperature=0.0)
        with pytest.raises(ValueError):
            fn(a, torch.zeros(4, 8), temperature=float("nan"))
        with pytest.raises(ValueError):
            fn(torch.zeros(0, 8), torch.zeros(0, 8))
    with pytest.raises(ValueError):
        EV.contrastive_loss_tensor(a.numpy(), a.numpy())
    with pytest.raises(ValueError):
        EV.contrastive_loss_tensor(a.long(), a.long())
    assert clm.contrastive_loss_grad is EV.contrastive_loss_grad and clm.contrastive_loss_tensor is EV.contrastive_loss_tensor
    assert clm.ContrastiveLoss is EV.ContrastiveLoss
    assert {"clm_index_softmax_grad", "clm_gemm_softw", "clm_transpose16"} <= set(_capi.EXPORTED)
