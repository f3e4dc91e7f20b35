"""Streaming log-sum-exp over the resident index (CosineIndex.logsumexp / softmax_topk,
clm_index_lse, include/clm.h) and the contrastive loss built on it (evaluate.contrastive_loss).

Yardstick: fp64 torch.logsumexp(scale * S), S = cosine_similarity() on the same rows -- exact_scores,
the routine both routes take their exact scores from, so the same s_j.

  exact route   |lse - yardstick| <= 1e-10 (an fp64 sum of <= 3000 terms is ~7e-13: 100x), err == 0,
                two calls bit-equal
  fast route    |lse - yardstick| <= err + 1e-10 for every query, two calls bit-equal, lse_stats()
                shows the route ran; on the peaked (even) queries at head = 64 the bound is not
                vacuous: err <= 1e-6 at scale 100, <= 1e-3 at scale 1 / 0.07

Every case runs on the default route (at these sizes: exact), the forced fast route (CLM_LSE_FAST)
and the forced exact route (CLM_LSE_EXACT). Shapes and generator: test_gpu_rank.py's.

The reference route (CosineIndex.logsumexp64, contrastive_loss(head=0)): unrounded fp64 cosines,
held against torch in fp64 on host cosines and against the reference's own fp64 loss (the golden).
"""
import os

import numpy as np
import pytest
import torch

from clip_lora_match_amd import _capi as C
from clip_lora_match_amd import evaluate as EV
from clip_lora_match_amd.distributed import merge_lse
from clip_lora_match_amd.search import CosineIndex
from clip_lora_match_amd.similarity import cosine_similarity

pytestmark = pytest.mark.gpu
SCALES = (1.0 / 0.07, 100.0)
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contrastive_loss.npz"))


def _problem(N, dim, nq, seed):
    """test_gpu_rank._problem: Gaussian rows; even queries are row[target] + 0.3 noise (peaked),
    odd ones Gaussian (flat)"""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn(N, dim, generator=g)
    tgt = torch.randint(0, N, (nq,), generator=g)
    q = torch.randn(nq, dim, generator=g)
    near = torch.arange(nq) % 2 == 0
    q[near] = rows[tgt[near]] + 0.3 * q[near]
    return rows, q


def _scores(q, rows):
    return cosine_similarity(q.float(), rows.float()).reshape(q.shape[0], rows.shape[0]).cpu().double()


def _index(rows, offset=0):
    idx = CosineIndex(rows.shape[1], capacity=max(rows.shape[0], 1))
    idx.append(rows)
    if offset:
        idx.set_offset(offset)
    return idx


def _check_exact(idx, q, want, scale, head, flag):
    before = idx.lse_stats()
    lse, err = idx.logsumexp(q, scale, head=head, band_cap=flag)
    lse2, _ = idx.logsumexp(q, scale, head=head, band_cap=flag)
    assert lse.dtype == torch.float64 and err.dtype == torch.float32
    d = (lse.cpu() - want).abs().max().item()
    print(f"exact  scale {scale:.4g} head {head}: max |lse - yardstick| {d:.3e}")
    assert d <= 1e-10
    assert (err == 0).all()
    assert torch.equal(lse, lse2)
    after = idx.lse_stats()
    assert after["exact"] - before["exact"] == 2 * q.shape[0] and after["fast"] == before["fast"]
    return lse


def _check_fast(idx, q, want, scale, head, cap=0):
    before = idx.lse_stats()
    lse, err = idx.logsumexp(q, scale, head=head, band_cap=C.CLM_LSE_FAST | cap)
    lse2, err2 = idx.logsumexp(q, scale, head=head, band_cap=C.CLM_LSE_FAST | cap)
    d = (lse.cpu() - want).abs()
    e = err.cpu().double()
    print(f"fast   scale {scale:.4g} head {head}: max |lse - yardstick| {d.max().item():.3e}, max err {e.max().item():.3e}, "
          f"max err (even queries) {e[::2].max().item():.3e}")
    assert (e >= 0).all() and (d <= e + 1e-10).all(), f"worst excess {(d - e).max().item():.3e}"
    assert torch.equal(lse, lse2) and torch.equal(err, err2)
    after = idx.lse_stats()
    assert after["fast"] - before["fast"] == 2 * q.shape[0] and after["exact"] == before["exact"]
    return lse, err


@pytest.mark.parametrize("dim", [64, 192, 512])
@pytest.mark.parametrize("N", [1, 255, 3000])
def test_lse_shapes(N, dim):
    """N = 255: the ragged (scalar) epilogue; 3000: no multiple of the 192 / 256 tiles"""
    for nq in (1, 17, 300):
        rows, q = _problem(N, dim, nq, 1000 * N + dim + nq)
        idx = _index(rows)
        S = _scores(q, rows)
        for scale in SCALES:
            want = torch.logsumexp(scale * S, dim=1)
            for head in (1, 64, N + 5):
                _check_exact(idx, q, want, scale, head, 0)                 # default: nq x N <= 2^24
                _check_exact(idx, q, want, scale, head, C.CLM_LSE_EXACT)
                # head >= N: every row is a band row; the capacity must hold them (default 2048)
                _, err = _check_fast(idx, q, want, scale, head, cap=N if head > N else 0)
                if head == 64:   # the bound on the peaked queries is not vacuous
                    assert err[::2].max().item() <= (1e-6 if scale == 100.0 else 1e-3)
            lse0, err0 = idx.logsumexp(q, scale, head=0, band_cap=C.CLM_LSE_FAST)   # no floors: exact
            assert (lse0.cpu() - want).abs().max() <= 1e-10 and (err0 == 0).all()
        idx.close()


def test_lse_two_query_blocks():
    """nq = 2600 > the 2560-query block: two balanced blocks of the fast pass"""
    rows, q = _problem(1000, 64, 2600, 7)
    idx = _index(rows)
    S = _scores(q, rows)
    for scale in SCALES:
        want = torch.logsumexp(scale * S, dim=1)
        _check_exact(idx, q, want, scale, 64, C.CLM_LSE_EXACT)
        _check_fast(idx, q, want, scale, 64)
    idx.close()


def test_lse_default_route_is_fast_on_a_large_problem():
    """nq x N > 2^24: the default route is the MFMA pass; the forced exact route bounds it"""
    rows, q = _problem(20000, 256, 900, 41)
    idx = _index(rows)
    scale = SCALES[0]
    want = torch.logsumexp(scale * _scores(q, rows), dim=1)
    lse, err = idx.logsumexp(q, scale)
    st = idx.lse_stats()
    assert st["fast"] == 900 and st["exact"] == 0 and st["overflow"] == 0, st
    ex, e0 = idx.logsumexp(q, scale, band_cap=C.CLM_LSE_EXACT)
    assert idx.lse_stats()["exact"] == 900 and (e0 == 0).all()
    assert (ex.cpu() - want).abs().max() <= 1e-10
    d = (lse - ex).abs().cpu()
    print(f"N 20000 dim 256: max |fast - exact| {d.max().item():.3e}, max err {err.max().item():.3e}, "
          f"max err (even) {err[::2].max().item():.3e}")
    assert (d <= err.cpu().double() + 1e-10).all()
    idx.close()


def test_lse_band_overflow():
    """5000 rows v + 1e-4 noise: every row is inside the margin of every floor, so each band holds
    all 5000 rows -- past the default capacity (2048) and past a capacity of 4; the exact route
    serves those queries: its bits, err = 0, and the overflow counter moves"""
    g = torch.Generator().manual_seed(5)
    v = torch.randn(64, generator=g)
    rows = v[None, :] + 1e-4 * torch.randn(5000, 64, generator=g)
    q = torch.cat([v[None, :] + 0.5 * torch.randn(12, 64, generator=g), torch.randn(12, 64, generator=g)])
    idx = _index(rows)
    scale = 100.0
    want = torch.logsumexp(scale * _scores(q, rows), dim=1)
    ex, _ = idx.logsumexp(q, scale, band_cap=C.CLM_LSE_EXACT)
    assert (ex.cpu() - want).abs().max() <= 1e-10
    a, ea = idx.logsumexp(q, scale, band_cap=C.CLM_LSE_FAST)
    st = idx.lse_stats()
    assert st["overflow"] == 24 and st["fast"] == 0 and st["exact"] == 48, st
    b, eb = idx.logsumexp(q, scale, band_cap=C.CLM_LSE_FAST | 4)
    assert idx.lse_stats()["overflow"] == 48
    assert torch.equal(a, ex) and torch.equal(b, ex) and (ea == 0).all() and (eb == 0).all()
    idx.close()


def test_lse_offset_and_fp16_only_index():
    rows, q = _problem(1500, 128, 64, 21)
    for scale in SCALES:
        idx = _index(rows, 1000)            # global ids do not enter the sum
        want = torch.logsumexp(scale * _scores(q, rows), dim=1)
        _check_exact(idx, q, want, scale, 64, 0)
        _check_fast(idx, q, want, scale, 64)
        idx.close()
        idx = _index(rows.half())           # no fp32 copy: the exact score is that of the fp16 rows
        assert C.lib().clm_index_has_f32(idx._h) == 0
        kept = idx.read()
        for qq in (q, q.half()):
            want = torch.logsumexp(scale * _scores(qq.float(), kept), dim=1)
            _check_exact(idx, qq, want, scale, 64, C.CLM_LSE_EXACT)
            _check_fast(idx, qq, want, scale, 64)
        idx.close()


def test_lse_zero_row_and_zero_query():
    rows, q = _problem(400, 64, 6, 31)
    idx = _index(rows)
    for flag in (0, C.CLM_LSE_FAST, C.CLM_LSE_EXACT):   # a zero query: every score is NaN
        lse, _ = idx.logsumexp(torch.zeros(3, 64), 100.0, band_cap=flag)
        assert torch.isnan(lse).all()
    idx.close()
    rows[123] = 0
    idx = _index(rows)
    want = torch.logsumexp(100.0 * _scores(q, rows), dim=1)
    assert torch.isnan(want).all()
    for flag in (0, C.CLM_LSE_FAST, C.CLM_LSE_EXACT):   # a zero row: the whole call goes exact
        before = idx.lse_stats()
        lse, _ = idx.logsumexp(q, 100.0, band_cap=flag)
        after = idx.lse_stats()
        assert torch.isnan(lse).all()
        assert after["exact"] - before["exact"] == 6 and after["fast"] == before["fast"]
    idx.close()


def test_lse_sharded_merge():
    """two half-indices, each with floors of its own, merged by merge_lse, against the whole"""
    rows, q = _problem(3000, 64, 40, 3)
    for scale in SCALES:
        want = torch.logsumexp(scale * _scores(q, rows), dim=1)
        a, b = _index(rows[:1257], 0), _index(rows[1257:], 1257)
        for flag in (C.CLM_LSE_FAST, C.CLM_LSE_EXACT):
            la, ea = a.logsumexp(q, scale, band_cap=flag)
            lb, eb = b.logsumexp(q, scale, band_cap=flag)
            lse, err = merge_lse([la, lb], [ea, eb])
            d = (lse - want).abs()
            print(f"merge  scale {scale:.4g} flag {flag:#x}: max |lse - yardstick| {d.max().item():.3e}, max err {err.max().item():.3e}")
            assert (d <= err + 1e-10).all()
            if flag == C.CLM_LSE_EXACT:
                assert (err == 0).all()
        a.close()
        b.close()


def test_softmax_topk():
    rows, q = _problem(300, 64, 17, 13)
    idx = _index(rows, 50)
    for scale in SCALES:
        p, i, err = idx.softmax_topk(q, 300, scale=scale)
        assert p.dtype == torch.float64 and p.shape == (17, 300) and i.dtype == torch.int64
        assert (p >= 0).all() and (p <= 1).all()
        assert ((p.sum(dim=1) - 1).abs().cpu() <= err.cpu().double() + 1e-9).all()
        s, i2 = idx.search(q, 300)
        lse, _ = idx.logsumexp(q, scale)
        assert torch.equal(i, i2) and torch.equal(p, torch.exp(scale * s.double() - lse[:, None]))
        assert (p[:, :-1] >= p[:, 1:]).all()
    p, i, _ = idx.softmax_topk(q, 310)          # slots past the index size
    assert (i[:, 300:] == -1).all() and (p[:, 300:] == 0).all() and (i[:, :300] >= 50).all()
    idx.close()


def _cos64(q, rows):
    q64, r64 = q.double(), rows.double()
    return (q64 / q64.norm(dim=1, keepdim=True)) @ (r64 / r64.norm(dim=1, keepdim=True)).T


def test_logsumexp64_reference_route():
    """CosineIndex.logsumexp64 (clm_index_lse64) against torch in fp64 on unrounded host cosines:
    |lse - logsumexp| <= 1e-10 (the exact route's bound: fp64 sums of <= 3000 terms), the pair score
    within 1e-13 of the host cosine (two fp64 dot products of <= 512 terms in different orders:
    512 * 2^-53 = 6e-14), two calls bit-equal; with an offset, on fp16-only rows, f16 queries, a
    zero row (NaN) and a target the index does not hold (NaN pair)."""
    for (N, dim, nq, seed) in ((1, 64, 1, 1), (255, 192, 17, 2), (3000, 512, 300, 3)):
        rows, q = _problem(N, dim, nq, seed)
        tgt = torch.arange(nq) % N
        S = _cos64(q, rows)
        idx = _index(rows, 1000)
        for scale in SCALES:
            lse, pair = idx.logsumexp64(q, scale, tgt + 1000)
            lse2, pair2 = idx.logsumexp64(q, scale, tgt + 1000)
            d = (lse.cpu() - torch.logsumexp(scale * S, dim=1)).abs().max().item()
            dp = (pair.cpu() - S[torch.arange(nq), tgt]).abs().max().item()
            print(f"lse64 N {N} dim {dim} nq {nq} scale {scale:.3f}: |d| {d:.3e}, pair {dp:.3e}")
            assert d <= 1e-10 and dp <= 1e-13
            assert torch.equal(lse, lse2) and torch.equal(pair, pair2)
        lse, pair = idx.logsumexp64(q, 100.0)
        assert pair is None and torch.equal(lse, lse2)
        bad = tgt + 1000
        bad[0] = 1000 + N
        assert torch.isnan(idx.logsumexp64(q, 100.0, bad)[1][0])
        with pytest.raises(ValueError):
            idx.logsumexp64(q, 100.0, tgt[:0])
        with pytest.raises(ValueError):
            idx.logsumexp64(q, 0.0)
        idx.close()
    rows, q = _problem(400, 128, 6, 4)
    idx = _index(rows.half())               # no fp32 copy: the cosines of the fp16 rows as kept
    kept = idx.read()
    for qq in (q, q.half()):
        lse, _ = idx.logsumexp64(qq, 100.0)
        assert (lse.cpu() - torch.logsumexp(100.0 * _cos64(qq.float(), kept.float()), dim=1)).abs().max() <= 1e-10
    idx.close()
    rows[123] = 0
    idx = _index(rows)
    assert torch.isnan(idx.logsumexp64(q, 100.0)[0]).all()
    idx.close()


def test_golden_loss_exact_route():
    """contrastive_loss at head = 0 against the reference's fp64 loss, 1e-9: the reference route,
    log-sum-exps and pair scores of unrounded fp64 cosines. (The exact scores of logsumexp / rank are
    rounded to fp32; a loss from them sits 3.8e-9 from this golden, the figure that rounding the
    fixture's fp64 cosine matrix to fp32 on the host reproduces -- hence the separate route.)"""
    out = EV.contrastive_loss(GOLD["a"], GOLD["b"], float(GOLD["T"]), head=0)
    d = abs(out["loss"] - float(GOLD["loss64"]))
    print(f"golden exact route: loss {out['loss']:.12f} vs {float(GOLD['loss64']):.12f}: |d| {d:.3e}")
    assert out["err"] == 0.0
    assert d <= 1e-9
    again = EV.contrastive_loss(GOLD["a"], GOLD["b"], float(GOLD["T"]), head=0)
    assert again == out
    # the exact route on the library's fp32-rounded scores: within 2^-24 / T of it (each score is off
    # by at most 2^-25, so each lse and each t / T by at most 2^-25 / T)
    ex = EV.contrastive_loss(GOLD["a"], GOLD["b"], float(GOLD["T"]), band_cap=C.CLM_LSE_EXACT)
    print(f"golden exact route, fp32-rounded scores: |d| {abs(ex['loss'] - out['loss']):.3e}")
    assert ex["err"] == 0.0 and abs(ex["loss"] - out["loss"]) <= 2.0 ** -24 / float(GOLD["T"])


def test_golden_loss_fast_route():
    out = EV.contrastive_loss(GOLD["a"], GOLD["b"], float(GOLD["T"]), band_cap=C.CLM_LSE_FAST)
    d = abs(out["loss"] - float(GOLD["loss64"]))
    print(f"golden fast route: loss {out['loss']:.12f}: |d| {d:.3e}, err {out['err']:.3e}")
    assert out["err"] > 0
    assert d <= out["err"] + 1e-9
    ex = EV.contrastive_loss(GOLD["a"], GOLD["b"], float(GOLD["T"]), band_cap=C.CLM_LSE_EXACT)
    assert abs(out["loss"] - ex["loss"]) <= out["err"] + 1e-12


def test_golden_loss_batched():
    """batch_size = 32 against the reference's per-batch mean (fp64), 1e-9, and its fp32 value
    within the recorded gap: B x B blocks of fp64 cosines on the host."""
    out = EV.contrastive_loss(GOLD["a"], GOLD["b"], float(GOLD["T"]), batch_size=int(GOLD["B"]))
    d = abs(out["loss"] - float(GOLD["batch64"]))
    print(f"golden batched: loss {out['loss']:.12f} vs {float(GOLD['batch64']):.12f}: |d| {d:.3e}")
    assert d <= 1e-9
    assert abs(out["loss"] - float(GOLD["batch32"])) <= float(GOLD["batch_gap"]) + 1e-9


def test_lse_argument_errors():
    rows, q = _problem(100, 64, 4, 1)
    idx = _index(rows)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            idx.logsumexp(q, bad)
    with pytest.raises(ValueError):
        idx.logsumexp(torch.zeros(4, 32), 100.0)
    lse, err = idx.logsumexp(torch.zeros(0, 64), 100.0)
    assert lse.numel() == 0 and err.numel() == 0
    idx.close()
    empty = CosineIndex(64)
    with pytest.raises(ValueError):
        empty.logsumexp(q, 100.0)
    empty.close()
    with pytest.raises(ValueError):
        EV.contrastive_loss(torch.zeros(3, 8), torch.zeros(4, 8))
    with pytest.raises(ValueError):
        EV.contrastive_loss(torch.ones(3, 8), torch.ones(3, 8), temperature=0.0)
