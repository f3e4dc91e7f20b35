"""Exact retrieval ranks on the resident index (CosineIndex.rank / count_above, clm_index_rank /
clm_index_count_above, include/clm.h).

Yardstick: cosine_similarity() on the same rows -- exact_scores, the routine the rank path's
re-score goes through -- so the ranks must be EQUAL, no exclusions:

    rank == 1 + ((S > t) | ((S == t) & (j < g))).sum()

Every case runs on the default route, with the MFMA band pass forced (CLM_RANK_BAND: at these
sizes the default is the exact route) and with the exact route forced (CLM_RANK_EXACT): the flag
bits of band_cap, clm.h.
"""
import numpy as np
import pytest
import torch

from clip_lora_match_amd import _capi as C
from clip_lora_match_amd.search import CosineIndex
from clip_lora_match_amd.similarity import cosine_similarity

pytestmark = pytest.mark.gpu
ROUTES = {"default": 0, "band": C.CLM_RANK_BAND, "exact": C.CLM_RANK_EXACT}


def _problem(N, dim, nq, seed):
    """Gaussian rows; half the queries are row[target] + 0.3 noise (shallow ranks), half Gaussian
    (deep ranks)"""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn(N, dim, generator=g)
    tgt = torch.randint(0, N, (nq,), generator=g)
    q = torch.randn(nq, dim, generator=g)
    near = torch.arange(nq) % 2 == 0
    q[near] = rows[tgt[near]] + 0.3 * q[near]
    return rows, q, tgt


def _yardstick(q, rows, tgt, offset=0):
    """(ranks, target scores) from the full exact score matrix; tgt: local row numbers"""
    S = cosine_similarity(q.float(), rows.float()).reshape(q.shape[0], rows.shape[0]).cpu()
    t = S[torch.arange(q.shape[0]), tgt][:, None]
    j = torch.arange(rows.shape[0])[None, :]
    ahead = (S > t) | ((S == t) & (j < tgt[:, None]))
    return 1 + ahead.sum(dim=1), t[:, 0]


def _index(rows, offset=0):
    idx = CosineIndex(rows.shape[1], capacity=max(rows.shape[0], 1))
    idx.append(rows)
    if offset:
        idx.set_offset(offset)
    return idx


def _all_routes(idx, q, tgt, want_r, want_s, cap=0):
    for name, flag in ROUTES.items():
        r, s = idx.rank(q, tgt, band_cap=flag | cap)
        assert r.dtype == torch.int64 and s.dtype == torch.float32
        assert torch.equal(r.cpu(), want_r), f"route {name}: ranks differ at {(r.cpu() != want_r).nonzero()[:5].tolist()}"
        assert torch.equal(s.cpu(), want_s), f"route {name}: target scores differ"


@pytest.mark.parametrize("dim", [64, 192, 512])
@pytest.mark.parametrize("N", [1, 255, 3000])
def test_rank_shapes(N, dim):
    """N = 255: the ragged (scalar) epilogue; 3000: no multiple of the 192 / 256 tiles. Every
    rank <= k is also the position search() returns the target at."""
    for nq in (1, 17, 300):
        rows, q, tgt = _problem(N, dim, nq, 1000 * N + dim + nq)
        idx = _index(rows)
        want_r, want_s = _yardstick(q, rows, tgt)
        _all_routes(idx, q, tgt, want_r, want_s)
        if N > 1 and nq > 1:
            assert want_r.min() <= 3 < want_r.max(), "both shallow and deep ranks occur"
        k = min(N, 1024)
        _, si = idx.search(q, k)
        si = si.cpu()
        for i in range(nq):
            if want_r[i] <= k:
                assert si[i, want_r[i] - 1] == tgt[i]
        st = idx.rank_stats()
        assert st["band"] == nq and st["exact"] == 2 * nq and st["overflow"] == 0
        idx.close()


def test_rank_two_query_blocks():
    """nq = 2600 > the 2560-query block: two balanced blocks of the band pass"""
    rows, q, tgt = _problem(1000, 64, 2600, 7)
    idx = _index(rows)
    want_r, want_s = _yardstick(q, rows, tgt)
    _all_routes(idx, q, tgt, want_r, want_s)
    idx.close()


def test_rank_exact_ties():
    """50 rows, each 3 times: the copies score identically, so the first / middle / last copy's
    ranks differ by exactly the index order"""
    g = torch.Generator().manual_seed(11)
    base = torch.randn(50, 128, generator=g)
    rows = torch.cat([base, base, base])            # copies of row r at r, 50 + r, 100 + r
    q = base + 0.2 * torch.randn(50, 128, generator=g)
    idx = _index(rows)
    ranks = {}
    for c in range(3):
        tgt = torch.arange(50) + 50 * c
        want_r, want_s = _yardstick(q, rows, tgt)
        _all_routes(idx, q, tgt, want_r, want_s)
        ranks[c] = want_r
    assert torch.equal(ranks[1], ranks[0] + 1) and torch.equal(ranks[2], ranks[0] + 2)
    idx.close()


def test_rank_band_overflow():
    """5000 rows v + 1e-4 noise: every row is inside the margin of every target, so each band
    holds all 5000 rows -- past the default capacity (2048) and past a capacity of 4; the exact
    route redoes those queries and the counts are the yardstick's either way"""
    g = torch.Generator().manual_seed(5)
    v = torch.randn(64, generator=g)
    rows = v[None, :] + 1e-4 * torch.randn(5000, 64, generator=g)
    q = torch.cat([v[None, :] + 0.5 * torch.randn(12, 64, generator=g), torch.randn(12, 64, generator=g)])
    tgt = torch.randint(0, 5000, (24,), generator=g)
    idx = _index(rows)
    want_r, want_s = _yardstick(q, rows, tgt)
    r_def, s_def = idx.rank(q, tgt, band_cap=C.CLM_RANK_BAND)
    st = idx.rank_stats()
    assert st["overflow"] == 24 and st["exact"] == 24 and st["band"] == 0, st
    r_4, s_4 = idx.rank(q, tgt, band_cap=C.CLM_RANK_BAND | 4)
    assert idx.rank_stats()["overflow"] == 48
    assert torch.equal(r_def.cpu(), want_r) and torch.equal(r_4.cpu(), want_r)
    assert torch.equal(s_def.cpu(), want_s) and torch.equal(s_4, s_def)
    idx.close()


def test_rank_sharded_ids():
    """set_offset(1000): targets and tie-breaks are global ids; count_above over two half-indices
    sums to the whole index's above"""
    g = torch.Generator().manual_seed(3)
    base = torch.randn(300, 64, generator=g)
    rows = torch.cat([base, base])[torch.randperm(600, generator=g)]   # exact ties across the halves
    q = torch.randn(40, 64, generator=g)
    tgt = torch.randint(0, 600, (40,), generator=g)
    q[::2] = rows[tgt[::2]] + 0.3 * q[::2]
    want_r, want_s = _yardstick(q, rows, tgt)
    whole = _index(rows, 1000)
    _all_routes(whole, q, tgt + 1000, want_r, want_s)
    with pytest.raises(ValueError):
        whole.rank(q[:1], torch.tensor([999]))      # a local id is not a global one
    a, b = _index(rows[:257], 1000), _index(rows[257:], 1257)
    for flag in ROUTES.values():
        above = whole.count_above(q, want_s, tgt + 1000, band_cap=flag)
        parts = a.count_above(q, want_s, tgt + 1000, band_cap=flag) + b.count_above(q, want_s, tgt + 1000, band_cap=flag)
        assert torch.equal(above.cpu(), want_r - 1) and torch.equal(parts.cpu(), want_r - 1)
    for i in (whole, a, b):
        i.close()


def test_rank_fp16_only_index():
    """rows appended as fp16, no fp32 copy kept: the exact score is that of the fp16 rows
    (index.read()); fp16 queries too"""
    rows, q, tgt = _problem(1500, 128, 64, 21)
    idx = _index(rows.half())
    assert C.lib().clm_index_has_f32(idx._h) == 0
    kept = idx.read()
    assert torch.equal(kept, rows.half().float())
    want_r, want_s = _yardstick(q, kept, tgt)
    _all_routes(idx, q, tgt, want_r, want_s)
    want_r, want_s = _yardstick(q.half().float(), kept, tgt)
    _all_routes(idx, q.half(), tgt, want_r, want_s)
    idx.close()


def test_rank_degenerate_inputs():
    rows, q, tgt = _problem(400, 64, 6, 31)
    idx = _index(rows, 50)
    # a zero query: every score is NaN, ties among NaNs break by index
    for flag in ROUTES.values():
        r, s = idx.rank(torch.zeros(6, 64), tgt + 50, band_cap=flag)
        assert torch.equal(r.cpu(), 1 + tgt) and torch.isnan(s).all()
    # a target of -1 or >= N, with and without the offset
    for bad in (-1, 49, 450, 1 << 40):
        with pytest.raises(ValueError):
            idx.rank(q[:1], torch.tensor([bad]))
    with pytest.raises(ValueError):
        idx.rank(q, tgt[:3] + 50)
    idx.close()
    # a zero row scores NaN: it counts above every finite target, on every route
    rows[123] = 0
    idx = _index(rows)
    tgt = torch.where(tgt == 123, tgt + 1, tgt)
    S = cosine_similarity(q, rows).reshape(6, 400).cpu()
    assert torch.isnan(S[:, 123]).all() and torch.isnan(S).sum() == 6
    t = S[torch.arange(6), tgt][:, None]
    j = torch.arange(400)[None, :]
    want = 1 + ((S > t) | ((S == t) & (j < tgt[:, None]))).sum(dim=1) + 1
    for flag in ROUTES.values():
        r, _ = idx.rank(q, tgt, band_cap=flag)
        assert torch.equal(r.cpu(), want)
    # ... and as the target it ranks first (NaN above every number)
    r, s = idx.rank(q, torch.full((6,), 123))
    assert torch.equal(r.cpu(), torch.ones(6, dtype=torch.int64)) and torch.isnan(s).all()
    idx.close()
    empty = CosineIndex(64)
    with pytest.raises(ValueError):
        empty.rank(q, tgt)
    with pytest.raises(ValueError):
        empty.count_above(q, torch.zeros(6), tgt)
    empty.close()


def test_rank_path_independence():
    """the same queries through the default route (here large enough for the band pass:
    nq x N > 2^24) and with the exact route forced: identical ranks and scores"""
    rows, q, tgt = _problem(20000, 256, 900, 41)
    idx = _index(rows)
    r0, s0 = idx.rank(q, tgt)
    st = idx.rank_stats()
    assert st["band"] == 900 and st["exact"] == 0, st
    r1, s1 = idx.rank(q, tgt, band_cap=C.CLM_RANK_EXACT)
    assert idx.rank_stats()["exact"] == 900
    assert torch.equal(r0, r1) and torch.equal(s0, s1)
    want_r, want_s = _yardstick(q, rows, tgt)
    assert torch.equal(r0.cpu(), want_r) and torch.equal(s0.cpu(), want_s)
    idx.close()
