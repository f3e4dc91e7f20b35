"""The multi-pass regimes of three device routines, each of which starts past a size threshold that
no other test crosses:

  topk_any (k_search.hip)        k > 8192: more than one LDS run of 8192 composites per row, merged by
                                 merge_runs_kernel in passes that alternate between two buffers;
  threshold search (k_range.hip) segments of more than two runs: several merge passes, runs without a
                                 partner, segments of different run counts in one pass loop, and the
                                 grid-stride item loops past 65535 / 16384 items;
  mask_scan (k_mask.hip)         more than 256 mask blocks (N > 2 097 152 rows): the carry between
                                 rounds of the one-workgroup scan.

Every comparison is bit-exact. The references are numpy restatements of the documented order (direct
hooks clm_topk_any / clm_mask_rows), the lexsort of the project's own cosine_similarity() -- the
routine every exact score comes from, the yardstick of tests/test_gpu_range.py -- and, for the top-k,
fp64 numpy cosines up to near-ties as well.
"""
import ctypes

import numpy as np
import pytest
import torch

import range_ref as R
from clip_lora_match_amd import _capi as C
from clip_lora_match_amd.distributed import merge_topk_gpu
from clip_lora_match_amd.search import CosineIndex
from clip_lora_match_amd.similarity import cosine_similarity
from oracle import search_ref as S
from test_gpu_range import ROUTES, _all_routes
from test_gpu_search import _agree

pytestmark = pytest.mark.gpu

SENT_S, SENT_I = -12345.5, -777


# ---- 1. clm_topk_any ------------------------------------------------------------------------------

def _float_key(v):
    """kernels.hpp float_key on the uint32 view: a set sign bit flips every bit, else the sign bit is set"""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return np.where((u >> np.uint32(31)) == 1, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _topk_any_ref(sc, ix, k, base):
    """the first k takeable entries by (float_key desc, low 32 bits of the index or column asc), then
    (-inf, -1); ids are the list's values, or base + column"""
    nq, _ = sc.shape
    out_s = np.full((nq, k), -np.inf, np.float32)
    out_i = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        cols = np.arange(sc.shape[1]) if ix is None else np.flatnonzero(ix[q] >= 0)
        ids = cols.astype(np.int64) if ix is None else ix[q, cols]
        key = _float_key(sc[q, cols]).astype(np.int64)
        order = np.lexsort((ids & 0xFFFFFFFF, -key))[:k]
        out_s[q, : order.size] = sc[q, cols[order]]
        out_i[q, : order.size] = ids[order] + (base if ix is None else 0)
    return out_s, out_i


def _run_topk_any(sc, ix, k, base):
    """one call on rows of stride C + 5 (the idx rows: C + 3) whose padding would win every order, into
    sentinel-filled outputs one row taller than nq; returns (rc, scores, ids, the spare rows untouched)"""
    nq, Cn = sc.shape
    buf = np.full((nq, Cn + 5), np.inf, np.float32)
    buf[:, :Cn] = sc
    d_s = torch.from_numpy(buf).cuda()
    d_i, p_i, ldi = None, None, 0
    if ix is not None:
        ibuf = np.full((nq, Cn + 3), 7, np.int64)
        ibuf[:, :Cn] = ix
        d_i = torch.from_numpy(ibuf).cuda()
        p_i, ldi = C.ptr(d_i), Cn + 3
    o_s = torch.full((nq + 1, k), SENT_S, dtype=torch.float32, device="cuda")
    o_i = torch.full((nq + 1, k), SENT_I, dtype=torch.int64, device="cuda")
    rc = C.lib().clm_topk_any(0, C.ptr(d_s), Cn + 5, p_i, ldi, nq, Cn, k, base, C.ptr(o_s), C.ptr(o_i),
                              C.stream_of(d_s.device))
    torch.cuda.synchronize()
    spare = bool((o_s[nq] == SENT_S).all()) and bool((o_i[nq] == SENT_I).all())
    return rc, o_s[:nq].cpu().numpy(), o_i[:nq].cpu().numpy(), spare


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def _distinct_gauss(rng, n):
    v = np.unique(rng.standard_normal(n + n // 8 + 64).astype(np.float32))
    assert v.size >= n
    return rng.permutation(v)[:n]


def _quarters(rng, n):
    """multiples of 1/4, uniform over max(1, n // 4096) values: every tie group holds ~4096 .. 8191
    entries (all n of them below 4096)"""
    g = max(1, n // 4096)
    return ((rng.integers(0, g, n) - g // 2) / 4.0).astype(np.float32)


def _sprinkled(rng, n):
    """Gaussians, a fifth of them replaced by +-inf, NaNs of both signs (two payloads each) and +-0.0"""
    v = rng.standard_normal(n).astype(np.float32)
    special = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFE, 0x00000000,
                        0x80000000], np.uint32).view(np.float32)
    pos = rng.permutation(n)[: n // 5]
    v[pos] = special[rng.integers(0, special.size, pos.size)]
    return v


def _tie_group(vals, k):
    """the number of entries equal to the min(k, n)-th largest of vals"""
    s = np.sort(vals)[::-1]
    return int((vals == s[min(k, vals.size) - 1]).sum())


def _assert_tie_group(vals, k):
    # more than 2048 (one 11-bit pass of the low-word select cannot settle it) wherever the row holds
    # that many entries at all; the shorter rows (k = 1025, C <= 1026) tie as a whole
    n = _tie_group(vals, k)
    assert n > 2048 if vals.size > 2048 else n == vals.size, (n, vals.size)


TOPK_K = [1025, 8192, 8193, 16385, 40000]   # kp = 2048 / 8192 (no merge pass) / 16384 (1) / 32768 (2) / 65536 (3)
TOPK_C = {"k-7": lambda k: k - 7, "k": lambda k: k, "k+1": lambda k: k + 1, "3k+11": lambda k: 3 * k + 11}


@pytest.mark.parametrize("cname", list(TOPK_C))
@pytest.mark.parametrize("k", TOPK_K)
def test_topk_any_direct(k, cname):
    """clm_topk_any against the numpy order, nq = 3, lds = C + 5. k = 8193 / 16385 / 40000 run one / two /
    three merge passes (the result in the second / first / second buffer). Three calls per shape: rows
    {distinct Gaussians, multiples of 1/4, all equal} by column with base 5e9, rows {specials, specials,
    multiples of 1/4} by column, and the first rows again under an index list (a permutation of values
    below 2^32 with 0 and 2^32 - 1, every 97th slot -1, the last row short of k, base ignored).
    C = k - 7 leaves every row short of k: (-inf, -1) padding."""
    Cn = TOPK_C[cname](k)
    rng = np.random.default_rng(1000 * k + Cn)
    plain = np.stack([_distinct_gauss(rng, Cn), _quarters(rng, Cn), np.full((Cn,), 0.75, np.float32)])
    special = np.stack([_sprinkled(rng, Cn), _sprinkled(rng, Cn), _quarters(rng, Cn)])
    assert np.unique(plain[0]).size == Cn
    _assert_tie_group(plain[1], k)
    _assert_tie_group(special[2], k)
    for u in (0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x00000000, 0x80000000):
        assert (special[0].view(np.uint32) == u).any()
    base = 5_000_000_000
    for sc in (plain, special):
        rc, gs, gi, spare = _run_topk_any(sc, None, k, base)
        assert rc == C.CLM_OK and spare
        ws, wi = _topk_any_ref(sc, None, k, base)
        assert np.array_equal(gi, wi)
        assert _same_bits(gs, ws)
        m = min(k, Cn)
        assert (gi[:, m:] == -1).all() and _same_bits(gs[:, m:], np.full((3, k - m), -np.inf, np.float32))
        assert (gi[:, :m] >= base).all()

    vals = np.setdiff1d(np.unique(rng.integers(0, 1 << 32, Cn + Cn // 8 + 64, dtype=np.int64)), [0, (1 << 32) - 1])
    assert vals.size >= Cn
    ix = np.stack([rng.permutation(vals)[:Cn] for _ in range(3)])
    ix[:, 1], ix[:, 2] = (1 << 32) - 1, 0           # slots that are no multiple of 97
    ix[0, 1], ix[0, 2] = 0, (1 << 32) - 1
    ix[:, ::97] = -1
    ix[2, min(k, Cn) // 2:] = -1                    # fewer valid entries than k
    ok1 = ix[1] >= 0
    _assert_tie_group(plain[1][ok1], k)
    rc, gs, gi, spare = _run_topk_any(plain, ix, k, 12345)
    assert rc == C.CLM_OK and spare
    ws, wi = _topk_any_ref(plain, ix, k, 0)
    assert np.array_equal(gi, wi)
    assert _same_bits(gs, ws)
    for q in range(3):
        m = min(k, int((ix[q] >= 0).sum()))
        assert m < k or q < 2
        assert (gi[q, m:] == -1).all() and (gi[q, :m] >= 0).all() and np.isneginf(gs[q, m:]).all()
    # the all-equal, short row comes back whole in index order: 0 leads it, 2^32 - 1 ends it
    m2 = int((ix[2] >= 0).sum())
    assert gi[2, 0] == 0 and gi[2, m2 - 1] == (1 << 32) - 1 and (np.diff(gi[2, :m2]) > 0).all()


def test_topk_any_refusals_write_nothing():
    """k < 1, nq > 65535, C > 2^32 - 1 (and a stride below C): CLM_E_ARG, the outputs keep their sentinel"""
    d_s = torch.zeros((4, 16), dtype=torch.float32, device="cuda")
    d_i = torch.zeros((4, 16), dtype=torch.int64, device="cuda")
    o_s = torch.full((4, 8), SENT_S, dtype=torch.float32, device="cuda")
    o_i = torch.full((4, 8), SENT_I, dtype=torch.int64, device="cuda")
    st = C.stream_of(d_s.device)
    L = C.lib()
    big = 1 << 32
    for lds, ldi, nq, Cn, k, with_idx in ((16, 16, 4, 16, 0, False), (16, 16, 4, 16, -3, True),
                                          (16, 16, 65536, 16, 2, False), (big, big, 1, big, 2, False),
                                          (big, big, 1, big, 2, True), (15, 16, 4, 16, 2, False),
                                          (16, 15, 4, 16, 2, True)):
        rc = L.clm_topk_any(0, C.ptr(d_s), lds, C.ptr(d_i) if with_idx else None, ldi, nq, Cn, k, 0, C.ptr(o_s),
                            C.ptr(o_i), st)
        assert rc == C.CLM_E_ARG, (lds, ldi, nq, Cn, k)
    host = torch.zeros((4, 16), dtype=torch.float32)
    assert L.clm_topk_any(0, C.ptr(host), 16, None, 0, 4, 16, 2, 0, C.ptr(o_s), C.ptr(o_i), st) == C.CLM_E_ARG
    torch.cuda.synchronize()
    assert bool((o_s == SENT_S).all()) and bool((o_i == SENT_I).all())
    # the same buffers, a shape that is taken: the sentinels go
    assert L.clm_topk_any(0, C.ptr(d_s), 16, None, 0, 4, 16, 8, 0, C.ptr(o_s), C.ptr(o_i), st) == C.CLM_OK
    torch.cuda.synchronize()
    assert o_i.cpu().tolist() == [list(range(8))] * 4 and bool((o_s == 0).all())


# ---- 2. the same regime end to end ---------------------------------------------------------------

BIG_N, BIG_DUP, BIG_NQ = 20_000, 300, 5


class _BigProblem:
    """20 000 Gaussian rows of dim 64 and the first 300 again (N = 20 300: exact ties 20 000 ids apart),
    5 queries; built once for the module, never modified"""

    def __init__(self):
        g = torch.Generator().manual_seed(41)
        base = torch.randn(BIG_N, 64, generator=g)
        self.rows = torch.cat([base, base[:BIG_DUP]], 0)
        self.q = torch.randn(BIG_NQ, 64, generator=g)
        self.exact = S.cosine_scores(self.q.numpy().astype(np.float64), self.rows.numpy().astype(np.float64))
        self.idx = CosineIndex(64, capacity=self.rows.shape[0])
        self.idx.append(self.rows)
        self.S = cosine_similarity(self.q, self.rows).reshape(BIG_NQ, -1).cpu().numpy()
        self.order = _search_order(self.S)


def _search_order(Sm):
    n = Sm.shape[1]
    return np.lexsort((np.broadcast_to(np.arange(n), Sm.shape), -Sm.astype(np.float64)), axis=-1)


@pytest.fixture(scope="module")
def big():
    p = _BigProblem()
    yield p
    p.idx.close()


def _assert_search(idx, q, k, Sm, order, offset=0):
    s, i = idx.search(q, k)
    s, i = s.cpu().numpy(), i.cpu().numpy()
    assert np.array_equal(i, order[:, :k] + offset)
    assert _same_bits(s, np.take_along_axis(Sm, order[:, :k], 1))
    return i


@pytest.mark.parametrize("k", [8193, 16385, BIG_N + BIG_DUP])
def test_search_large_k(big, k):
    """CosineIndex.search past one LDS run (one pass, two passes, and k = N with both): ids and score
    bits equal the lexsort (score desc, id asc) of cosine_similarity() on the same rows; the ids agree
    with the order of fp64 numpy cosines up to near-ties; the duplicated rows come in id order"""
    assert np.array_equal(big.S[:, :BIG_DUP], big.S[:, BIG_N:])
    i = _assert_search(big.idx, big.q, k, big.S, big.order)
    _, oi = S.topk(big.exact, k)
    _agree(i, oi, big.exact)
    for q in range(BIG_NQ):
        pos = {int(r): j for j, r in enumerate(i[q])}
        pairs = [(pos[r], pos[r + BIG_N]) for r in range(BIG_DUP) if r in pos and r + BIG_N in pos]
        assert len(pairs) >= 50 and all(b == a + 1 for a, b in pairs)


def test_search_large_k_offset_and_fp16_index(big):
    """set_offset(2^33): the ids come back shifted whole; an index appended in fp16 keeps no fp32 copy and
    ranks the fp16 rows' own exact scores"""
    big.idx.set_offset(1 << 33)
    try:
        _assert_search(big.idx, big.q, 16385, big.S, big.order, offset=1 << 33)
    finally:
        big.idx.set_offset(0)
    idx = CosineIndex(64, capacity=big.rows.shape[0])
    idx.append(big.rows.half())
    assert C.lib().clm_index_has_f32(idx._h) == 0
    kept = idx.read()
    S16 = cosine_similarity(big.q, kept).reshape(BIG_NQ, -1).cpu().numpy()
    order = _search_order(S16)
    exact16 = S.cosine_scores(big.q.numpy().astype(np.float64), kept.numpy().astype(np.float64))
    for k in (8193, BIG_N + BIG_DUP):
        i = _assert_search(idx, big.q, k, S16, order)
        _agree(i, S.topk(exact16, k)[1], exact16)
    idx.set_offset(1 << 33)
    _assert_search(idx, big.q, 16385, S16, order, offset=1 << 33)
    idx.close()


@pytest.mark.parametrize("k", [9000, 17000])
def test_merge_past_one_run(k):
    """merge_topk_gpu / clm_topk_merge with k > 8192 (kp = 16384: one merge pass, 32768: two), the tied
    scores and -1 slots of test_merge_past_one_sort: the (score desc, index asc) order of the union"""
    g = np.random.default_rng(5)
    nq, parts, k_in = 3, 4, 5000
    sc = (g.integers(0, 200, (nq, parts * k_in)) / 200.0).astype(np.float32)   # many ties
    ix = np.stack([g.permutation(10 * parts * k_in)[:parts * k_in] for _ in range(nq)]).astype(np.int64)
    ix[:, ::97] = -1
    s, i = merge_topk_gpu(torch.from_numpy(sc).cuda(), torch.from_numpy(ix).cuda(), parts, k)
    s, i = s.cpu().numpy(), i.cpu().numpy()
    for q in range(nq):
        ok = ix[q] >= 0
        assert ok.sum() >= k
        order = np.lexsort((ix[q][ok], -sc[q][ok]))[:k]
        assert np.array_equal(i[q], ix[q][ok][order]) and _same_bits(s[q], sc[q][ok][order])


# ---- 3. threshold search: long, mixed segments ---------------------------------------------------

RANGE_N = 41_000
LENS_A = [0, 1, 2, 8191, 8192, 8193, 16384, 16385, 24576, 24577, 32769, 41000]   # 3 passes: L = 8192, 16384, 32768
LENS_B = [5, 8193, 20000, 24577, 32768, 300]                                     # 2 passes: back in the first buffer


class _RangeProblem:
    def __init__(self):
        g = torch.Generator().manual_seed(77)
        self.rows = torch.randn(RANGE_N, 64, generator=g)
        self.q = torch.randn(32, 64, generator=g)
        self.S = cosine_similarity(self.q, self.rows).reshape(32, RANGE_N).cpu()
        assert not torch.isnan(self.S).any()
        self.sorted = torch.sort(self.S, dim=1, descending=True)[0]
        self.idx = CosineIndex(64, capacity=RANGE_N)
        self.idx.append(self.rows)

    def call(self, lengths, first):
        """queries from `first` on, one per target length (a query whose L-th and (L + 1)-th largest
        scores are equal is skipped): (queries, tau, the reference triple)"""
        qs, taus, nxt = [], [], first
        for L in lengths:
            while True:
                row = self.sorted[nxt]
                ok = L == 0 or L == RANGE_N or bool(row[L] < row[L - 1])
                nxt += 1
                if ok:
                    break
            qs.append(nxt - 1)
            taus.append(float("inf") if L == 0 else float(row[L - 1]))
        sel = torch.tensor(qs)
        tau = torch.tensor(taus, dtype=torch.float32)
        want = R.above_from_scores(self.S[sel], tau)
        assert (want[0][1:] - want[0][:-1]).tolist() == list(lengths)
        return self.q[sel], tau, want


@pytest.fixture(scope="module")
def ranged():
    p = _RangeProblem()
    yield p
    p.idx.close()


def test_range_mixed_long_segments(ranged):
    """One 41 000-row index, thresholds set to the L-th largest score of each query so that the segment
    lengths are exactly the targets (asserted). Call A: 1, 2, 3, 4, 5 and 6 runs, 1-element last runs,
    runs without a partner, three merge passes. Call B: two passes, the result back in the first
    buffer -- before A, and again after A with equal bits (nothing stale in the second buffer). Every
    call on the default, band and exact routes: offsets, score bits and ids equal the reference."""
    perm = torch.randperm(len(LENS_A), generator=torch.Generator().manual_seed(3)).tolist()
    lens_a = [LENS_A[j] for j in perm]
    assert lens_a != LENS_A
    qa, ta, want_a = ranged.call(lens_a, 0)
    qb, tb, want_b = ranged.call(LENS_B, 16)
    _all_routes(ranged.idx, qb, tb, want_b)
    before = [ranged.idx.search_above(qb, tb, band_cap=f) for f in ROUTES.values()]
    _all_routes(ranged.idx, qa, ta, want_a)
    for f, held in zip(ROUTES.values(), before):
        again = ranged.idx.search_above(qb, tb, band_cap=f)
        assert R.same(again, held) and R.same(again, want_b)
        assert torch.equal(again[1].view(torch.int32), held[1].view(torch.int32))
    _all_routes(ranged.idx, qa, ta, want_a)


def _all_rows_problem(nq, N, seed):
    """every query keeps all N rows: (index, queries, the reference triple)"""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn(N, 64, generator=g)
    q = torch.randn(nq, 64, generator=g)
    Sm = cosine_similarity(q, rows).reshape(nq, N).cpu().numpy()
    assert not np.isnan(Sm).any()
    order = np.argsort(-Sm.astype(np.float64), axis=1, kind="stable")     # score desc, id asc
    want = (torch.arange(nq + 1, dtype=torch.int64) * N, torch.from_numpy(np.take_along_axis(Sm, order, 1).reshape(-1)),
            torch.from_numpy(order.reshape(-1).astype(np.int64)))
    idx = CosineIndex(64, capacity=N)
    idx.append(rows)
    return idx, q, want


def test_range_item_loops_wrap():
    """70 000 queries on a 64-row index, every query returning all 64 rows: 70 000 run items and 70 000
    decode items in one launch each (the grids hold 65535, so the item loops wrap). tau = -inf on the
    band and exact routes (a non-finite tau is served by the exact route on either), and tau = -2 --
    below every cosine, finite -- on the band route, where the filter pass itself lists all 64 rows of
    every query in 28 blocks of queries (range_stats: all 70 000 served fast)."""
    nq = 70_000
    idx, q, want = _all_rows_problem(nq, 64, 9)
    _all_routes(idx, q, -float("inf"), want, routes={"band": C.CLM_RANK_BAND, "exact": C.CLM_RANK_EXACT})
    st0 = idx.range_stats()
    _all_routes(idx, q, -2.0, want, routes={"band": C.CLM_RANK_BAND})
    st1 = idx.range_stats()
    assert st1["fast"] - st0["fast"] == nq and st1["exact"] == st0["exact"] and st1["overflow"] == st0["overflow"]
    idx.close()


def test_range_plan_items_wrap():
    """keep_kernel walks the plan items of ONE block of queries (at most 2560) with 16384 waves, so its
    loop wraps only when a block's lists hold more than 16384 chunks of 64 rows: 2560 queries that each
    list all 512 rows of the index (tau = -2, capacity 512) make 8 x 2560 = 20480 items, counted and
    emitted by the band route (range_stats: all served fast, none overflowed)."""
    nq, N = 2560, 512
    idx, q, want = _all_rows_problem(nq, N, 10)
    _all_routes(idx, q, -2.0, want, routes={"band": C.CLM_RANK_BAND})
    assert idx.range_stats() == {"fast": nq, "exact": 0, "overflow": 0}
    idx.close()


# ---- 4. clm_mask_rows ------------------------------------------------------------------------------

MASK_BLOCK = 8192    # rows per mask block (256 words)
MASK_N = [1, 31, 32, 33, 8191, 8192, 8193, 2_097_152, 2_097_153, 6_299_654]


def _mask_ref(words, N):
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:N]
    rows = np.flatnonzero(bits)
    nblk = (N + MASK_BLOCK - 1) // MASK_BLOCK
    padded = np.zeros((nblk * MASK_BLOCK,), np.uint8)
    padded[:N] = bits
    bcnt = padded.reshape(nblk, MASK_BLOCK).sum(1, dtype=np.int64)
    boff = np.concatenate([[0], np.cumsum(bcnt)]).astype(np.int64)
    return rows, bcnt, boff


def _masks(N, rng):
    nw = (N + 31) // 32
    tail = np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF) if N % 32 else np.uint32(0)   # the bits at or past N
    full = np.full((nw,), 0xFFFFFFFF, np.uint32)
    full[-1] &= ~tail
    half = rng.integers(0, 1 << 32, nw, dtype=np.uint64).astype(np.uint32)
    half[-1] &= ~tail
    one = np.zeros((nw,), np.uint32)
    one[(N - 1) >> 5] = np.uint32(1) << np.uint32((N - 1) & 31)
    junk = rng.integers(0, 1 << 32, nw, dtype=np.uint64).astype(np.uint32)
    junk[-1] |= tail
    return {"empty": np.zeros((nw,), np.uint32), "full": full, "half": half, "last_bit": one, "garbage_tail": junk}


@pytest.mark.parametrize("N", MASK_N)
def test_mask_rows_direct(N):
    """clm_mask_rows (mask_prepare, mask_scan, mask_compact in clm_index_search_masked's order) against
    numpy: the list, P and every boff[b], bcnt[b]. 2 097 152 rows are 256 blocks -- one round of the scan
    exactly --, one more row starts a second round with one block, 6 299 654 rows take four rounds and
    end in a ragged word. A full round sums to 2^21; the garbage bits at or past N of the caller's last
    word are cleared in the prepared words and stay in the caller's. Every output buffer is one element
    longer than its extent, and that element keeps its sentinel."""
    rng = np.random.default_rng(N)
    nw, nblk = (N + 31) // 32, (N + MASK_BLOCK - 1) // MASK_BLOCK
    L = C.lib()
    for name, words in _masks(N, rng).items():
        rows, bcnt, boff = _mask_ref(words, N)
        P = rows.size
        if name == "full":
            assert P == N and (nblk <= 256 or boff[256] == 1 << 21)
        if name == "garbage_tail" and N % 32:
            assert int(words[-1]) >> (N % 32) == (1 << (32 - N % 32)) - 1
        d_in = torch.from_numpy(words.view(np.int32)).cuda()
        d_words = torch.full((nw + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        d_bcnt = torch.full((nblk + 1,), -3, dtype=torch.int32, device="cuda")
        d_boff = torch.full((nblk + 2,), -5, dtype=torch.int64, device="cuda")
        d_list = torch.full((P + 1,), -7, dtype=torch.int32, device="cuda")
        got_p = ctypes.c_int64(-1)
        C.check(L.clm_mask_rows(0, C.ptr(d_in), N, C.ptr(d_words), C.ptr(d_bcnt), C.ptr(d_boff), C.ptr(d_list),
                                ctypes.byref(got_p), C.stream_of(d_in.device)), "clm_mask_rows")
        torch.cuda.synchronize()
        assert got_p.value == P, name
        assert np.array_equal(d_in.cpu().numpy().view(np.uint32), words), name      # the caller's words
        clean = words.copy()
        if N % 32:
            clean[-1] &= np.uint32((1 << (N % 32)) - 1)
        w = d_words.cpu().numpy()
        assert np.array_equal(w[:nw].view(np.uint32), clean) and w[nw] == 0x5A5A5A5A, name
        b = d_bcnt.cpu().numpy()
        assert np.array_equal(b[:nblk].astype(np.int64), bcnt) and b[nblk] == -3, name
        o = d_boff.cpu().numpy()
        assert o.dtype == np.int64 and np.array_equal(o[: nblk + 1], boff) and o[nblk + 1] == -5, name
        lst = d_list.cpu().numpy()
        assert np.array_equal(lst[:P].view(np.uint32).astype(np.int64), rows) and lst[P] == -7, name


def test_mask_rows_refusals_and_no_list():
    """N < 1, N > 2^32 - 1, a host pointer: CLM_E_ARG with nothing written; a NULL list and a NULL P skip
    the list alone"""
    L = C.lib()
    d_in = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    d_words = torch.full((2,), 9, dtype=torch.int32, device="cuda")
    d_bcnt = torch.full((1,), 9, dtype=torch.int32, device="cuda")
    d_boff = torch.full((2,), 9, dtype=torch.int64, device="cuda")
    st = C.stream_of(d_in.device)
    for N in (0, -5, 1 << 32):
        assert L.clm_mask_rows(0, C.ptr(d_in), N, C.ptr(d_words), C.ptr(d_bcnt), C.ptr(d_boff), None, None, st) == C.CLM_E_ARG
    host = torch.zeros((2,), dtype=torch.int32)
    assert L.clm_mask_rows(0, C.ptr(host), 40, C.ptr(d_words), C.ptr(d_bcnt), C.ptr(d_boff), None, None, st) == C.CLM_E_ARG
    torch.cuda.synchronize()
    assert d_words.tolist() == [9, 9] and d_bcnt.tolist() == [9] and d_boff.tolist() == [9, 9]
    C.check(L.clm_mask_rows(0, C.ptr(d_in), 40, C.ptr(d_words), C.ptr(d_bcnt), C.ptr(d_boff), None, None, st))
    torch.cuda.synchronize()
    assert d_words.tolist() == [-1, 0xFF] and d_bcnt.tolist() == [40] and d_boff.tolist() == [0, 40]
