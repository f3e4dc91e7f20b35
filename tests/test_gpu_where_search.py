"""Keyed search on the GPU: CosineIndex.search_where / clm_index_search_keyed -- one inclusive value range
per query in one batched pass -- against the yardstick of the filtered search, mask_ref.masked_topk,
applied query by query with that query's mask (tests/where_ref.py). Scores come from
cosine_similarity(), the routine every exact score comes from, so the comparison is bitwise (M.same).
Every case runs on the default, the exact and the pass route; where_stats() says which route served.
"""
import ctypes

import numpy as np
import pytest
import torch

import mask_ref as M
import where_ref as R
from clip_lora_match_amd import _capi as C
from clip_lora_match_amd.search import CosineIndex, TextSearchIndex
from clip_lora_match_amd.similarity import cosine_similarity

pytestmark = pytest.mark.gpu
ROUTES = {"default": 0, "exact": C.CLM_MASK_EXACT, "pass": C.CLM_MASK_PASS}
CAND_CAP = 2048


def _problem(N, dim, nq, seed):
    """Gaussian rows; half the queries are a row + 0.3 noise (cosine ~0.96 with it), half Gaussian"""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn(N, dim, generator=g)
    tgt = torch.randint(0, N, (nq,), generator=g)
    q = torch.randn(nq, dim, generator=g)
    near = torch.arange(nq) % 2 == 0
    q[near] = rows[tgt[near]] + 0.3 * q[near]
    return rows, q


def _scores(q, rows):
    return cosine_similarity(q.float(), rows.float()).reshape(q.shape[0], rows.shape[0]).cpu()


def _index(rows, offset=0):
    idx = CosineIndex(rows.shape[1], capacity=max(rows.shape[0], 1))
    idx.append(rows)
    if offset:
        idx.set_offset(offset)
    return idx


def _delta(idx, before):
    now = idx.where_stats()
    return {k: now[k] - before[k] for k in now}


def _patterns(N, seed):
    """name -> (values [N], keep or None): all equal, key = row number, 8 random categories, random values
    under a batch-wide filter (the -1 sentinel keys)"""
    g = torch.Generator().manual_seed(seed)
    return {"equal": (torch.full((N,), 7, dtype=torch.int64), None),
            "rownum": (torch.arange(N, dtype=torch.int64), None),
            "cats": (torch.randint(0, 8, (N,), generator=g), None),
            "sentinel": (torch.randint(-20, 50, (N,), generator=g), torch.rand(N, generator=g) < 0.6)}


def _check(idx, q, k, keys, lo, hi, open_, want, keep=None, routes=ROUTES, served=None):
    """search_where on every route against the yardstick's lists `want` (of the open rows `open_`); pads
    exactly past min(k, rows in range); served: {route name: {counter: queries}}"""
    nq = q.shape[0]
    full = torch.from_numpy(np.minimum(open_.sum(1), k))
    live = torch.arange(k)[None, :] < full[:, None]
    for name, flag in routes.items():
        before = idx.where_stats()
        got = idx.search_where(q, k, keys, lo, hi, allow=keep, route=flag)
        assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and got[0].is_cuda and got[1].is_cuda
        assert got[0].shape == (nq, k) and got[1].shape == (nq, k)
        assert torch.equal(got[1].cpu(), want[1]), f"route {name}: ids differ"
        assert M.same(got, want), f"route {name}: scores differ"
        assert torch.equal(got[1].cpu() >= 0, live) and bool((got[0].cpu()[~live] == -float("inf")).all())
        d = _delta(idx, before)
        assert sum(d.values()) == nq, f"route {name}: {d}"
        if served and name in served:
            assert d == served[name], f"route {name}: {d}"


@pytest.mark.parametrize("dim", [64, 192, 512])
@pytest.mark.parametrize("N", [1, 31, 255, 3000])
def test_where_shapes(N, dim):
    """N = 255: the ragged (scalar) epilogue; 3000: no multiple of the 192 / 256 tiles. Every key pattern,
    with ranges of every kind mixed inside one batch (where_ref.ranges), every nq of {1, 17, 300} and every
    k of {1, 5, 100}, on every route. The yardstick is computed once per pattern and k for 300 queries:
    the lists of fewer queries are its first rows. A handful of queries per case are also compared, bit
    for bit, with the filtered search of that query under its own mask on the GPU."""
    rows, qall = _problem(N, dim, 300, 1000 * N + dim)
    idx = _index(rows)
    Sall = _scores(qall, rows)
    for pname, (values, keep) in _patterns(N, N + dim).items():
        plan = idx.key_plan(values, allow=keep)
        assert plan.keys.dtype == torch.int32 and plan.keys.is_cuda and plan.n == N
        for k in (1, 5, 100):
            lo, hi, kinds = R.ranges(values, keep, 300, k, N + k)
            open_ = R.open_rows(values, lo, hi, 300, keep)
            full = R.keyed_topk(Sall, open_, k)
            for nq in (1, 17, 300):
                want = (full[0][:nq].contiguous(), full[1][:nq].contiguous())
                exact = {"exact": {"pass": 0, "exact": nq}}
                _check(idx, qall[:nq], k, plan, lo[:nq], hi[:nq], open_[:nq], want, served=exact)
                if nq == 17:   # values planned on the fly, and one kind of every range against search(allow=)
                    _check(idx, qall[:nq], k, values, lo[:nq], hi[:nq], open_[:nq], want, keep=keep,
                           routes={"default": 0})
                    got = idx.search_where(qall[:nq], k, plan, lo[:nq], hi[:nq])
                    for i in range(len(R.KINDS)):
                        ms, mi = idx.search(qall[i], k, allow=torch.from_numpy(open_[i]))
                        assert torch.equal(mi[0], got[1][i]), (pname, k, kinds[i])
                        assert torch.equal(ms[0].view(torch.int32), got[0][i].view(torch.int32)), (pname, k, kinds[i])
        if N == 3000 and pname == "rownum":   # the kinds the values allow are all there
            assert set(kinds) == set(R.KINDS) and int(open_[kinds.index("k_minus_1")].sum()) == 99
            assert int(open_[kinds.index("one_row")].sum()) == 1
    idx.close()


def test_default_routing_mixed_selectivities():
    """N = 70,001 x 64, nq = 300, k = 5: above the pass route's size bound (4 x 8,192 rows). One batch mixes
    ranges holding 100 %, 60 %, 5 % and 0.1 % of the rows, 3 rows (fewer than k) and none; a batch whose
    ranges each hold at least half the rows is served by the pass route alone."""
    N, nq, k = 70001, 300, 5
    rows, q = _problem(N, 64, nq, 5)
    idx = _index(rows)
    S = _scores(q, rows)
    g = torch.Generator().manual_seed(6)
    values = torch.randperm(N, generator=g)            # a range [0, f N) holds f N rows scattered over the index
    plan = idx.key_plan(values)
    sizes = [N, int(0.6 * N), int(0.05 * N), N // 1000, 3, 0]
    hi = torch.tensor([sizes[i % 6] - 1 for i in range(nq)], dtype=torch.float64)
    lo = torch.zeros(nq, dtype=torch.float64)
    lo[5::6], hi[5::6] = 10.0, 9.0                     # the empty range: lo > hi
    open_ = R.open_rows(values, lo, hi, nq)
    assert open_.sum(1)[:6].tolist() == sizes
    want = R.keyed_topk(S, open_, k)
    _check(idx, q, k, plan, lo, hi, open_, want, served={"exact": {"pass": 0, "exact": nq}})
    # every range at least half the rows: nothing is redone
    lo2 = torch.tensor([(i % 4) * (N // 8) for i in range(nq)], dtype=torch.float64)
    hi2 = lo2 + (N // 2 + (torch.arange(nq) % 5) * 1000).double()
    open2 = R.open_rows(values, lo2, hi2, nq)
    assert int(open2.sum(1).min()) >= N // 2
    _check(idx, q, k, plan, lo2, hi2, open2, R.keyed_topk(S, open2, k), routes={"default": 0},
           served={"default": {"pass": nq, "exact": 0}})
    # k > 256 has no pass route
    _check(idx, q[:12], 300, plan, lo[:12], hi[:12], open_[:12], R.keyed_topk(S[:12], open_[:12], 300),
           served={n: {"pass": 0, "exact": 12} for n in ROUTES})
    idx.close()


def test_near_duplicates_overflow_the_candidate_list():
    """N = 40,999 x 64 with 6,000 copies of one row, the queries that row: 3,000 copies carry value 1,
    3,000 value 2, every other row 0. Query 0's range [0, 1] and query 2's [2, 2] hold 3,000 near
    duplicates each -- more than the 2,048 candidates of the pass route, redone exactly --, query 1's
    [0, 0] holds none and is not"""
    N, k = 40999, 5
    rows, _ = _problem(N, 64, 2, 31)
    g = torch.Generator().manual_seed(32)
    dup = torch.randperm(N, generator=g)[:6000]
    rows[dup] = rows[dup[0]].clone()
    values = torch.zeros(N, dtype=torch.int64)
    values[dup[:3000]] = 1
    values[dup[3000:]] = 2
    q = rows[dup[0]].clone().repeat(3, 1)
    lo, hi = torch.tensor([0, 0, 2]), torch.tensor([1, 0, 2])
    idx = _index(rows)
    S = _scores(q, rows)
    open_ = R.open_rows(values, lo, hi, 3)
    assert int(open_[0].sum()) > CAND_CAP and int(open_[2].sum()) == 3000 > CAND_CAP
    want = R.keyed_topk(S, open_, k)
    redone = {"pass": 1, "exact": 2}
    _check(idx, q, k, values, lo, hi, open_, want,
           served={"default": redone, "pass": redone, "exact": {"pass": 0, "exact": 3}})
    assert torch.equal(want[1][0], torch.sort(dup[:3000]).values[:k])
    assert torch.equal(want[1][2], torch.sort(dup[3000:]).values[:k])
    assert not set(want[1][1].tolist()) & set(dup.tolist())
    idx.close()


def test_nan_scores():
    """a zero row in the index: the exact route serves whatever is asked for, and the row leads the lists
    of the ranges that hold it; a zero query gets the filtered search's result (id order), redone exactly
    when the pass route met it"""
    N = 3000
    rows, q = _problem(N, 64, 6, 41)
    rows[1234] = 0
    q[4] = 0
    values = torch.arange(N) % 100
    lo = torch.tensor([0, 34, 35, 0, 10, 34])
    hi = torch.tensor([99, 34, 99, 33, 60, 40])
    idx = _index(rows)
    S = _scores(q, rows)
    assert torch.isnan(S[:, 1234]).all() and torch.isnan(S[4]).all() and int(values[1234]) == 34
    open_ = R.open_rows(values, lo, hi, 6)
    want = R.keyed_topk(S, open_, 5)
    _check(idx, q, 5, values, lo, hi, open_, want, served={n: {"pass": 0, "exact": 6} for n in ROUTES})
    assert want[1][[0, 1, 5], 0].tolist() == [1234] * 3 and not bool((want[1][[2, 3]] == 1234).any())
    idx.close()
    rows[1234] = 1.0                                  # finite norms: the pass route runs
    idx = _index(rows)
    S = _scores(q, rows)
    want = R.keyed_topk(S, open_, 5)
    _check(idx, q, 5, values, lo, hi, open_, want, routes={"pass": C.CLM_MASK_PASS},
           served={"pass": {"pass": 5, "exact": 1}})
    assert torch.isnan(want[0][4]).all() and torch.equal(want[1][4], torch.nonzero(torch.from_numpy(open_[4]))[:5, 0])
    ms, mi = idx.search(q[4], 5, allow=torch.from_numpy(open_[4]))
    assert torch.equal(mi[0].cpu(), want[1][4])
    idx.close()


def test_variants_offset_fp16_and_late_rows():
    N = 3000
    rows, q = _problem(N, 64, 17, 51)
    g = torch.Generator().manual_seed(52)
    values = torch.randint(0, 40, (N,), generator=g).float() * 0.5     # float values, halves
    lo, hi, _ = R.ranges(values, None, 17, 5, 53)
    open_ = R.open_rows(values, lo, hi, 17)
    idx = _index(rows, offset=1000)
    want = R.keyed_topk(_scores(q, rows), open_, 5, offset=1000)
    assert int(want[1][want[1] >= 0].min()) >= 1000
    _check(idx, q, 5, values, lo, hi, open_, want)
    qh = q.half()                                                      # fp16 queries
    _check(idx, qh, 5, values, lo, hi, open_, R.keyed_topk(_scores(qh.float(), rows), open_, 5, offset=1000))
    with pytest.raises(ValueError):                                    # one value per row
        idx.search_where(q, 5, values[:-1], lo, hi)
    with pytest.raises(ValueError):                                    # a plan holds its own filter
        idx.search_where(q, 5, idx.key_plan(values), lo, hi, allow=torch.ones(N, dtype=torch.bool))
    with pytest.raises(ValueError):                                    # k > 1024: no route serves it
        idx.search_where(q, 1025, values, lo, hi)
    idx.close()
    h = rows.half()
    idx = _index(h)                                                    # fp16 only: the fp16 rows are the caller's rows
    _check(idx, q, 5, values, lo, hi, open_, R.keyed_topk(_scores(q, h.float()), open_, 5))
    idx.close()
    idx = _index(h[:1700])                                             # rows appended after the first search
    plan = idx.key_plan(values[:1700])
    _check(idx, q, 5, plan, lo, hi, open_[:, :1700], R.keyed_topk(_scores(q, h[:1700].float()), open_[:, :1700], 5))
    idx.append(rows[1700:])
    with pytest.raises(ValueError):                                    # the plan is of 1,700 rows
        idx.search_where(q, 5, plan, lo, hi)
    mixed = torch.cat([h[:1700].float(), rows[1700:]], 0)
    _check(idx, q, 5, idx.key_plan(values), lo, hi, open_, R.keyed_topk(_scores(q, mixed), open_, 5))
    idx.close()


def test_two_query_blocks_on_the_pass_route():
    """nq = 2,600 > the 2,560-query block at N = 7,000 with CLM_MASK_PASS: two query blocks, each with its
    own slice of the ranges"""
    N, nq = 7000, 2600
    rows, q = _problem(N, 64, nq, 61)
    idx = _index(rows)
    g = torch.Generator().manual_seed(62)
    values = torch.randint(0, 1000, (N,), generator=g)
    lo = torch.randint(0, 500, (nq,), generator=g)
    hi = lo + torch.randint(300, 500, (nq,), generator=g)
    open_ = R.open_rows(values, lo, hi, nq)
    _check(idx, q, 5, values, lo, hi, open_, R.keyed_topk(_scores(q, rows), open_, 5),
           routes={"pass": C.CLM_MASK_PASS}, served={"pass": {"pass": nq, "exact": 0}})
    idx.close()


def _np(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_raw_c_abi():
    """host pointers for the keys, the bounds, n_in and the outputs, device pointers for them all, n_in =
    NULL; an n_in that is too small, CLM_MASK_GATHER, k = 0, k = 1025 and an empty index are CLM_E_ARG"""
    N, k, nq = 3000, 5, 6
    rows, q = _problem(N, 64, nq, 71)
    idx = _index(rows)
    S = _scores(q, rows)
    g = torch.Generator().manual_seed(72)
    keys = torch.randint(-1, 12, (N,), generator=g).to(torch.int32).numpy()       # raw keys, -1 among them
    lo = np.array([0, 3, 5, 7, 0, 11], np.int32)
    hi = np.array([11, 3, 9, 6, 2, 40], np.int32)                                  # query 3: lo > hi
    open_ = (keys[None, :] >= lo[:, None]) & (keys[None, :] <= hi[:, None])
    n_in = open_.sum(1).astype(np.int64)
    want = R.keyed_topk(S, open_, k)
    L = C.lib()
    qd = q.cuda().contiguous()
    st = C.stream_of(idx.device)
    dk, dlo, dhi, dn = (torch.from_numpy(a).cuda() for a in (keys, lo, hi, n_in))
    for flag in ROUTES.values():
        for counts in (n_in, None):
            hs, hi_ = np.empty((nq, k), np.float32), np.empty((nq, k), np.int64)
            C.check(L.clm_index_search_keyed(idx._h, C.ptr(qd), C.CLM_F32, nq, k, _np(keys), _np(lo), _np(hi),
                                             _np(counts) if counts is not None else None, flag, _np(hs), _np(hi_), st))
            assert M.same((torch.from_numpy(hs), torch.from_numpy(hi_)), want)
            ds = torch.empty((nq, k), dtype=torch.float32, device="cuda")
            di = torch.empty((nq, k), dtype=torch.int64, device="cuda")
            C.check(L.clm_index_search_keyed(idx._h, C.ptr(qd), C.CLM_F32, nq, k, C.ptr(dk), C.ptr(dlo), C.ptr(dhi),
                                             C.ptr(dn) if counts is not None else None, flag, C.ptr(ds), C.ptr(di), st))
            assert M.same((ds, di), want)
    ds = torch.empty((nq, 1024), dtype=torch.float32, device="cuda")    # room for the largest k below
    di = torch.empty((nq, 1024), dtype=torch.int64, device="cuda")

    def call(flag=0, kk=k, counts=None, n=nq):
        return L.clm_index_search_keyed(idx._h, C.ptr(qd), C.CLM_F32, n, kk, C.ptr(dk), C.ptr(dlo), C.ptr(dhi),
                                        None if counts is None else C.ptr(counts), flag, C.ptr(ds), C.ptr(di), st)
    small = dn.clone()
    small[0] = 2                                      # query 0 lists 5 rows of a range said to hold 2
    assert call(C.CLM_MASK_PASS, counts=small) == C.CLM_E_ARG and b"n_in" in L.clm_last_error()
    assert call(C.CLM_MASK_GATHER) == C.CLM_E_ARG
    assert call(kk=0) == C.CLM_E_ARG and call(kk=1025) == C.CLM_E_ARG
    assert call(kk=1024) == C.CLM_OK
    assert call(n=0) == C.CLM_OK and call(n=-1) == C.CLM_E_ARG
    assert L.clm_index_search_keyed(idx._h, C.ptr(qd), C.CLM_F32, nq, k, None, C.ptr(dlo), C.ptr(dhi), None, 0,
                                    C.ptr(ds), C.ptr(di), st) == C.CLM_E_ARG
    # the other searches' counters are untouched by all of this
    v = (ctypes.c_int64 * 20)()
    C.check(L.clm_index_stats2(idx._h, v, 20))
    assert list(v) == [0] * 20
    idx.reset()
    assert call() == C.CLM_E_ARG and b"empty" in L.clm_last_error()
    idx.close()


def test_layers_text_index_finder_and_plan_filter():
    N, dim = 300, 64
    rows, q = _problem(N, dim, 4, 91)
    paths = [f"img/{i}.jpg" for i in range(N)]
    texts = [("wallet" if i % 3 == 0 else "keys") + f" {i}" for i in range(N)]
    ts = TextSearchIndex(embeddings=rows, image_paths=paths, texts=texts)
    unit = rows / rows.norm(dim=-1, keepdim=True)
    S = _scores(q, unit)
    found_at = torch.tensor([1000 + 7 * (i % 40) for i in range(N)])       # a timestamp per item
    lost_at = torch.tensor([1000, 1100, 1273, 5000])                       # each seeker: found after they lost
    open_ = R.open_rows(found_at, lost_at, None, 4)
    want = R.keyed_topk(S, open_, 5)
    bs, bi = ts.search_batch(q, 5, keys=lambda i, p, t: 1000 + 7 * (int(t.split()[1]) % 40), lo=lost_at, hi=None)
    assert M.same((bs, bi), want) and bool((bi[3] == -1).all())
    # with a batch-wide filter
    wallet = torch.tensor([t.startswith("wallet") for t in texts])
    bs, bi = ts.search_batch(q, 5, allow=lambda i, p, t: t.startswith("wallet"), keys=found_at, lo=lost_at, hi=None)
    open_w = R.open_rows(found_at, lost_at, None, 4, wallet)
    assert M.same((bs, bi), R.keyed_topk(S, open_w, 5))
    # key_plan(allow=) equals search(allow= that mask AND the range), query by query
    plan = ts._gpu.key_plan(found_at, allow=wallet)
    ps, pi = ts._gpu.search_where(q, 5, plan, lost_at, None)
    for i in range(4):
        ms, mi = ts._gpu.search(q[i], 5, allow=torch.from_numpy(open_w[i]))
        assert torch.equal(mi[0], pi[i]) and torch.equal(ms[0].view(torch.int32), ps[i].view(torch.int32))
    with pytest.raises(ValueError):
        ts.search_batch(q, 5, keys=found_at, lo=0, hi=1, group_by="text")

    from clip_lora_match_amd.finder import FinderIndex
    f = FinderIndex.__new__(FinderIndex)
    f.index = ts
    res = f.search_many(q, 5, found_at, lost_at, None)
    assert len(res) == 4 and res[3] == [] and [len(r) for r in res[:3]] == [5, 5, 5]
    for i in range(3):
        assert [r.index for r in res[i]] == want[1][i].tolist()
        assert torch.tensor([r.score for r in res[i]]).view(torch.int32).tolist() == want[0][i].view(torch.int32).tolist()
        assert all(r.text == texts[r.index] and r.image_path == paths[r.index] for r in res[i])
        assert all(int(found_at[r.index]) >= int(lost_at[i]) for r in res[i])

    import socket
    import torch.distributed as dist
    from clip_lora_match_amd.distributed import ShardedIndex
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        sh = ShardedIndex(dim, N)
        sh.append_shard(unit)
        assert M.same(sh.search_where(q, 5, found_at, lost_at, None), want)
        assert M.same(sh.search_where(q, 5, found_at, lost_at, None, allow=wallet), R.keyed_topk(S, open_w, 5))
    finally:
        dist.destroy_process_group()
