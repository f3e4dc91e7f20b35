"""Grouped search on the resident index (CosineIndex.search_grouped, clm_topk_distinct, include/clm.h)
and the layers on top.

Yardstick: cosine_similarity() on the same rows -- exact_scores, the routine every exact score comes
from -- through group_ref.grouped_topk: walk the allowed rows by (NaN first, score desc, id asc), keep a
row iff its group is new, the first k kept rows, (-inf, -1, -1) past the number of distinct allowed
groups. Ids and gids must be equal, scores are compared by their bits (a NaN must be a NaN).

The hook is driven directly on hand-made lists against group_ref.distinct_lists; every end-to-end case
runs on the default routing and with every query forced through the threshold route.
"""
import numpy as np
import pytest
import torch

import group_ref as G
from clip_lora_match_amd import _capi as C
from clip_lora_match_amd.search import GROUP_ROUTE_THRESHOLD, CosineIndex, TextSearchIndex, group_row_bound
from clip_lora_match_amd.similarity import cosine_similarity

pytestmark = pytest.mark.gpu
ROUTES = {"default": 0, "threshold": GROUP_ROUTE_THRESHOLD}


# ---- 1. the hook -----------------------------------------------------------------------------------
def _call(s, i, g, offsets, ld, nq, k, spare=3):
    """clm_topk_distinct on device copies of numpy lists; outputs carry `spare` guard rows that must
    come back untouched. Returns (rc, scores, ids, gids, found) as CPU tensors."""
    ds = torch.from_numpy(np.ascontiguousarray(s, np.float32)).cuda()
    di = torch.from_numpy(np.ascontiguousarray(i, np.int64)).cuda()
    dg = torch.from_numpy(np.ascontiguousarray(g, np.int64)).cuda()
    do = None if offsets is None else torch.from_numpy(np.asarray(offsets, np.int64)).cuda()
    rows = max(nq, 0) + spare
    os_ = torch.full((rows, k if 1 <= k <= 1024 else 1), 7.5, dtype=torch.float32, device="cuda")
    oi = torch.full(os_.shape, -77, dtype=torch.int64, device="cuda")
    og = torch.full(os_.shape, -78, dtype=torch.int64, device="cuda")
    fo = torch.full((rows,), -79, dtype=torch.int32, device="cuda")
    rc = C.lib().clm_topk_distinct(0, C.ptr(ds), C.ptr(di), C.ptr(dg), C.ptr(do) if do is not None else None, ld, nq,
                                   k, C.ptr(os_), C.ptr(oi), C.ptr(og), C.ptr(fo), C.stream_of(ds.device))
    torch.cuda.synchronize()
    n = max(nq, 0) if rc == C.CLM_OK else 0       # a refused call writes nothing at all
    assert bool((os_[n:] == 7.5).all()) and bool((oi[n:] == -77).all()) and bool((og[n:] == -78).all())
    assert bool((fo[n:] == -79).all())
    n = max(nq, 0)
    return rc, os_[:n].cpu(), oi[:n].cpu(), og[:n].cpu(), fo[:n].cpu()


def _check_ragged(s, i, g, offsets, k):
    rc, gs, gi, gg, gf = _call(s, i, g, offsets, 0, len(offsets) - 1, k)
    assert rc == C.CLM_OK
    ws, wi, wg, wf = G.distinct_lists(s, i, g, offsets, k)
    assert torch.equal(gf, wf), (gf, wf)
    assert G.same((gs, gi, gg), (ws, wi, wg))
    return gs, gi, gg, gf


def _check_fixed(s, i, g, k):
    """s / i / g [nq, ld]"""
    nq, ld = s.shape
    rc, gs, gi, gg, gf = _call(s, i, g, None, ld, nq, k)
    assert rc == C.CLM_OK
    ws, wi, wg, wf = G.distinct_lists(s.reshape(-1), i.reshape(-1), g.reshape(-1), np.arange(nq + 1) * ld, k)
    assert torch.equal(gf, wf), (gf, wf)
    assert G.same((gs, gi, gg), (ws, wi, wg))


def _lists(rng, nq, ld, n_groups, gid_of=lambda x: x):
    s = -np.sort(-rng.standard_normal((nq, ld)).astype(np.float32), axis=1)
    i = np.stack([rng.permutation(ld * 4)[:ld] for _ in range(nq)]).astype(np.int64)
    g = gid_of(rng.integers(0, n_groups, (nq, ld)).astype(np.int64))
    return s, i, g


@pytest.mark.parametrize("ld", [1, 63, 64, 65, 1024, 1025])
def test_hook_lengths(ld):
    """1 / 63 / 64 / 65: one entry, a wave and its edges; 1,024 / 1,025: one full chunk and the first
    entry of a second one. Few groups (k above the distinct count), many groups, k = 1 / 5 / 1,024."""
    rng = np.random.default_rng(ld)
    for n_groups in (1, max(ld // 3, 1), 1 << 20):
        s, i, g = _lists(rng, 3, ld, n_groups)
        for k in (1, 5, 1024):
            _check_fixed(s, i, g, k)


def test_hook_ragged_mix_with_an_empty_list():
    """5,000 entries in lists of 0, 5, 1,024 (one exact chunk), 0, 2,471 and 1,500 entries"""
    rng = np.random.default_rng(1)
    off = np.cumsum([0, 0, 5, 1024, 0, 2471, 1500])
    assert off[-1] == 5000
    s = rng.standard_normal(5000).astype(np.float32)
    i = rng.permutation(20000)[:5000].astype(np.int64)
    g = rng.integers(0, 300, 5000).astype(np.int64)
    for k in (1, 7, 299, 1024):
        gs, gi, gg, gf = _check_ragged(s, i, g, off, k)
        assert gf[0] == 0 and gf[3] == 0 and bool((gi[0] == -1).all()) and bool(torch.isinf(gs[3]).all())
    # two calls, the same bits
    a = _call(s, i, g, off, 0, 6, 299)
    b = _call(s, i, g, off, 0, 6, 299)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[1:], b[1:]))


def test_hook_one_group_all_distinct_and_the_second_chunk():
    rng = np.random.default_rng(2)
    n = 3000
    s = -np.sort(-rng.standard_normal(n).astype(np.float32))
    i = rng.permutation(n).astype(np.int64)
    off = [0, n]
    # all entries in one group: one result
    gs, gi, gg, gf = _check_ragged(s, i, np.full(n, 42, np.int64), off, 5)
    assert gf.tolist() == [1] and gi[0, 0] == i[0]
    # all groups distinct: the list's head
    for k in (1, 5, 1024):
        gs, gi, gg, gf = _check_ragged(s, i, np.arange(n, dtype=np.int64) * 3, off, k)
        assert gi[0].tolist() == i[:k].tolist()
    # the wanted 4th group first appears in the second chunk (position 1,500); three groups fill the rest
    g = (np.arange(n) % 3).astype(np.int64)
    g[1500] = 9
    gs, gi, gg, gf = _check_ragged(s, i, g, off, 4)
    assert gg[0].tolist() == [0, 1, 2, 9] and gi[0, 3] == i[1500] and gf.tolist() == [4]
    # ... and in the third, with k above what the list holds
    g = (np.arange(n) % 3).astype(np.int64)
    g[2999] = 9
    gs, gi, gg, gf = _check_ragged(s, i, g, off, 6)
    assert gg[0].tolist() == [0, 1, 2, 9, -1, -1] and gf.tolist() == [4]
    # a new group at every chunk edge
    g = np.zeros(n, np.int64)
    g[[1023, 1024, 2047, 2048]] = [5, 6, 7, 8]
    gs, gi, gg, gf = _check_ragged(s, i, g, off, 5)
    assert gg[0].tolist() == [0, 5, 6, 7, 8]


def test_hook_struck_out_entries():
    """id < 0 entries in the middle are skipped wherever they stand: a group whose first entry is struck
    out is represented by its next one, a group with only such entries is absent"""
    rng = np.random.default_rng(3)
    n = 2500
    s = -np.sort(-rng.standard_normal(n).astype(np.float32))
    i = rng.permutation(n).astype(np.int64)
    g = rng.integers(0, 400, n).astype(np.int64)
    i[rng.random(n) < 0.4] = -1
    i[:3] = -1                         # the head of the list
    i[g == 7] = -1                     # a whole group
    for k in (1, 50, 1024):
        gs, gi, gg, gf = _check_ragged(s, i, g, [0, n], k)
        assert 7 not in gg[0].tolist() and bool((gi[0, : int(gf[0])] >= 0).all())
    _check_ragged(s, np.full(n, -1, np.int64), g, [0, n], 5)          # nothing to keep
    s2, i2, g2 = _lists(rng, 4, 300, 40)
    i2[:, 100:200] = -1
    _check_fixed(s2, i2, g2, 64)


def _same_slot_gids(count):
    """gids that hash to ONE slot of the kernel's 4,096-slot table (k_group.hip: the top 12 bits of gid *
    0x9E3779B97F4A7C15 mod 2^64): every one of them collides with every other"""
    cand = np.arange(1, 1 << 23, dtype=np.uint64)
    slot = (cand * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(52)
    hit = cand[slot == slot[0]]
    assert hit.size >= count
    return hit[:count].astype(np.int64)


def test_hook_gid_values():
    """gids that are multiples of 4,096 (equal low bits), gids near 2^40 with gid 0 among them, and gids
    that all fall into one slot of the table: told apart by their whole value"""
    rng = np.random.default_rng(4)
    for name, gid_of, n_groups in (("x4096", lambda x: x * 4096, 700), ("x2^32", lambda x: x << 32, 700),
                                   ("2^40", lambda x: np.where(x == 0, 0, (1 << 40) - 350 + x), 700)):
        s, i, g = _lists(rng, 2, 2100, n_groups, gid_of)
        g[:, 5] = 0                    # gid 0 among them, whatever was drawn
        assert g.min() == 0 and g.max() >= 4096 * 600
        for k in (5, 1024):
            _check_fixed(s, i, g, k)
    pool = _same_slot_gids(600)
    s, i, g = _lists(rng, 2, 2100, 600, lambda x: pool[x])
    for k in (5, 600, 1024):
        _check_fixed(s, i, g, k)


def test_hook_argument_errors():
    rng = np.random.default_rng(5)
    s, i, g = _lists(rng, 2, 10, 4)
    for nq, ld, k in ((2, 10, 0), (2, 10, 1025), (2, 10, -1), (-1, 10, 5), (2, -1, 5)):
        rc, gs, gi, gg, gf = _call(s, i, g, None, ld, nq, k, spare=4)   # the guard rows cover every output
        assert rc == C.CLM_E_ARG, (nq, ld, k)
    assert _call(s, i, g, None, 10, 0, 5)[0] == C.CLM_OK               # nq == 0: a no-op
    L = C.lib()
    ds, di, dg = (torch.from_numpy(a).cuda() for a in (s, i, g))
    os_ = torch.zeros((2, 5), dtype=torch.float32, device="cuda")
    oi = torch.zeros((2, 5), dtype=torch.int64, device="cuda")
    og = torch.zeros((2, 5), dtype=torch.int64, device="cuda")
    fo = torch.zeros((2,), dtype=torch.int32, device="cuda")
    ok = [C.ptr(ds), C.ptr(di), C.ptr(dg), None, 10, 2, 5, C.ptr(os_), C.ptr(oi), C.ptr(og), C.ptr(fo)]
    assert L.clm_topk_distinct(0, *ok, None) == C.CLM_OK
    host = torch.zeros((2, 10), dtype=torch.int64)
    for pos in (0, 1, 2, 7, 8, 9, 10):
        bad = list(ok)
        bad[pos] = None
        assert L.clm_topk_distinct(0, *bad, None) == C.CLM_E_ARG, pos      # a null pointer with nq > 0
        bad[pos] = C.ptr(host)
        assert L.clm_topk_distinct(0, *bad, None) == C.CLM_E_ARG, pos      # host memory
    bad = list(ok)
    bad[3] = C.ptr(host)                                                   # host offsets
    assert L.clm_topk_distinct(0, *bad, None) == C.CLM_E_ARG
    torch.cuda.synchronize()


# ---- 2. end to end ---------------------------------------------------------------------------------
def _problem(N, dim, nq, seed):
    """Gaussian rows; half the queries are a row + 0.3 noise, half Gaussian"""
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


def _layouts(N, seed):
    g = torch.Generator().manual_seed(seed)
    return {"own": torch.arange(N), "pairs": torch.arange(N) // 2,
            "random": torch.randint(0, max(N // 8, 1), (N,), generator=g) * 4096 + 11,
            "one": torch.full((N,), 5, dtype=torch.int64)}


def _masks(N, seed):
    g = torch.Generator().manual_seed(seed)
    first = torch.zeros(N, dtype=torch.bool)
    first[0] = True
    return {"none": None, "half": torch.rand(N, generator=g) < 0.5, "tenth": torch.rand(N, generator=g) < 0.1,
            "zeros": torch.zeros(N, dtype=torch.bool), "first": first}


def _both_routes(idx, q, k, groups, keep, want, budget=None):
    """search_grouped on both routes against `want`; returns the default route's group_stats delta"""
    nq, deltas = q.shape[0], {}
    for name, flag in ROUTES.items():
        before = idx.group_stats()
        kw = {} if budget is None else {"block_budget": budget}
        got = idx.search_grouped(q, k, groups, allow=keep, route=flag, **kw)
        assert all(t.is_cuda for t in got) and got[0].dtype == torch.float32
        assert got[1].dtype == torch.int64 and got[2].dtype == torch.int64
        assert all(t.shape == (nq, k) for t in got)
        assert torch.equal(got[1].cpu(), want[1]), f"route {name}: ids differ"
        assert torch.equal(got[2].cpu(), want[2]), f"route {name}: gids differ"
        assert G.same(got, want), f"route {name}: scores differ"
        now = idx.group_stats()
        deltas[name] = {r: now[r] - before[r] for r in now}
        assert sum(deltas[name].values()) == nq, (name, deltas[name])
    assert deltas["threshold"] == {"list": 0, "threshold": nq}
    return deltas["default"]


@pytest.mark.parametrize("dim", [64, 512])
@pytest.mark.parametrize("N", [1, 31, 255, 3000])
def test_grouped_shapes(N, dim):
    """every layout under every mask with k = 1 / 5 / 64 on both routes. The yardstick is computed once per
    (layout, mask) at k = 64: the result of a smaller k is its first columns (the rule is a prefix rule)."""
    nq = 9
    rows, q = _problem(N, dim, nq, 1000 * N + dim)
    idx = _index(rows)
    S = _scores(q, rows)
    for lname, groups in _layouts(N, N + dim).items():
        for mname, keep in _masks(N, 3 * N + dim).items():
            full = G.grouped_topk(S, groups, 64, keep)
            allowed = groups if keep is None else groups[keep]
            P, n_groups = allowed.numel(), torch.unique(allowed).numel()
            m = int(torch.bincount(allowed - allowed.min()).max()) if P else 0
            for k in (1, 5, 64):
                want = tuple(t[:, :k].contiguous() for t in full)
                assert bool((want[1][:, min(n_groups, k):] == -1).all())
                assert bool((want[1][:, : min(n_groups, k)] >= 0).all())
                d = _both_routes(idx, q, k, groups, keep, want)
                if min(group_row_bound(k, m), P) <= 1024:      # the list holds the bound, or every row
                    assert d == {"list": nq, "threshold": 0}, (lname, mname, k, d)
                if lname == "one" and N == 3000 and mname in ("none", "half") and k > 1:
                    assert d == {"list": 0, "threshold": nq}   # 1,024 rows of one group: never k groups
                if lname == "own":                              # what search() returns
                    us, ui = idx.search(q, k) if keep is None else idx.search(q, k, allow=keep)
                    got = idx.search_grouped(q, k, groups, allow=keep)
                    assert torch.equal(got[1], ui) and torch.equal(got[0].view(torch.int32), us.view(torch.int32))
                    assert torch.equal(got[2], ui)                 # gid = row = id here, -1 in the pads
    idx.close()


def test_plan_is_reusable_and_validates():
    N = 255
    rows, q = _problem(N, 64, 5, 11)
    idx = _index(rows)
    S = _scores(q, rows)
    groups = torch.arange(N) // 4
    keep = _masks(N, 12)["half"]
    plan = idx.group_plan(groups, allow=keep)
    sizes = torch.bincount(groups[keep])
    assert plan.m == int(sizes.max()) and plan.n_groups == int((sizes > 0).sum()) and plan.n_allowed == int(keep.sum())
    from clip_lora_match_amd.search import unpack_mask
    reps = unpack_mask(plan.reps, N).cpu()
    assert int(reps.sum()) == plan.n_groups and int((reps & ~keep).sum()) == 0
    assert sorted(groups[reps].tolist()) == torch.unique(groups[keep]).tolist()
    for gid in torch.unique(groups[keep]).tolist():              # the lowest allowed row of each group
        assert int(torch.nonzero(reps & (groups == gid))[0]) == int(torch.nonzero(keep & (groups == gid))[0])
    want = G.grouped_topk(S, groups, 5, keep)
    for flag in ROUTES.values():
        assert G.same(idx.search_grouped(q, 5, plan, route=flag), want)
        assert G.same(idx.search_grouped(q[0], 5, plan, route=flag), tuple(t[:1] for t in want))   # a 1-D query
    with pytest.raises(ValueError):
        idx.search_grouped(q, 5, plan, allow=keep)               # the plan holds its own filter
    for bad in (groups[:-1], groups.float(), groups - 1, groups.bool()):
        with pytest.raises(ValueError):
            idx.search_grouped(q, 5, bad)
    for k in (0, 1025):
        with pytest.raises(ValueError):
            idx.search_grouped(q, k, groups)
    assert idx.search_grouped(q, 1024, groups)[0].shape == (5, 1024)
    idx.append(rows[:1])
    with pytest.raises(ValueError):
        idx.search_grouped(q, 5, plan)                           # made for 255 rows
    idx.reset()
    with pytest.raises(ValueError):
        idx.search_grouped(q, 5, torch.zeros(0, dtype=torch.int64))   # an empty index, as search refuses it
    idx.close()


def test_offset_ties_and_nan():
    """set_offset (ids past 2^33); duplicated rows in different groups and in one group, to pin the tie
    order (the lower id first, and as its group's representative); a zero row, whose score is NaN for
    every query and leads every walk -- with k = 1 the threshold route's theta is that NaN"""
    N, dim, off = 255, 64, (1 << 33) + 5
    rows, q = _problem(N, dim, 8, 21)
    rows[200] = rows[10]
    rows[77] = rows[10]
    rows[150] = rows[40]
    rows[41] = rows[40]
    q[0] = rows[10]
    q[1] = rows[40]
    groups = torch.arange(N) // 2          # 10 / 77 / 200 in three groups; 40 and 41 in one, 150 in another
    idx = _index(rows, off)
    S = _scores(q, rows)
    for keep in (None, _masks(N, 22)["half"] | (torch.arange(N) == 77) | (torch.arange(N) == 200)):
        for k in (1, 3, 20):
            want = G.grouped_topk(S, groups, k, keep, offset=off)
            _both_routes(idx, q, k, groups, keep, want)
    want = G.grouped_topk(S, groups, 3, None, offset=off)
    assert want[1][0].tolist() == [off + 10, off + 77, off + 200] and want[1][1].tolist()[:2] == [off + 40, off + 150]
    idx.close()
    rows[3] = 0.0
    rows[90] = 0.0
    idx = _index(rows)
    S = _scores(q, rows)
    assert bool(torch.isnan(S[:, 3]).all()) and bool(torch.isnan(S[:, 90]).all())
    for groups in (torch.arange(N) // 2, torch.arange(N) % 87):   # rows 3 and 90 share group 3 in the second
        for k in (1, 2, 5):
            want = G.grouped_topk(S, groups, k)
            assert want[1][:, 0].tolist() == [3] * 8
            _both_routes(idx, q, k, groups, None, want)
    idx.close()


@pytest.mark.parametrize("dim", [64, 512])
def test_giant_group_reaches_the_threshold_route(dim):
    """N = 3,000: rows [0, 1,500) = base + 0.05 noise in ONE group, the rest Gaussian rows each a group of
    its own, rows and groups shuffled by one permutation; even queries = base + 0.05 noise, odd queries
    Gaussian; generator seed 7, k = 5. The first 1,024 rows of every even query lie in the giant group, so
    the list route finds one group and leaves them to the threshold route; every odd query finds its 5
    groups in its list (both checked on the yardstick's scores below, then asserted of group_stats).
    Repeated with a block budget of 4,000 entries: two lists of about 1,500 per block, four blocks."""
    N, nq, k = 3000, 16, 5
    g = torch.Generator().manual_seed(7)
    base = torch.randn(dim, generator=g)
    rows = torch.randn(N, dim, generator=g)
    rows[:1500] = base + 0.05 * rows[:1500]
    groups = torch.arange(N) + 10
    groups[:1500] = 3
    perm = torch.randperm(N, generator=g)
    rows, groups = rows[perm].contiguous(), groups[perm].contiguous()
    q = torch.randn(nq, dim, generator=g)
    q[0::2] = base + 0.05 * q[0::2]
    S = _scores(q, rows)
    head = torch.argsort(S, dim=1, descending=True, stable=True)[:, :1024]     # no NaN, ties keep the lower id
    distinct = torch.tensor([torch.unique(groups[head[j]]).numel() for j in range(nq)])
    assert distinct[0::2].tolist() == [1] * (nq // 2) and bool((distinct[1::2] >= k).all()), distinct
    idx = _index(rows)
    want = G.grouped_topk(S, groups, k)
    assert _both_routes(idx, q, k, groups, None, want) == {"list": nq // 2, "threshold": nq // 2}
    lens = idx.count_above(q[0::2], idx.search(q[0::2], k, allow=idx.group_plan(groups).reps)[0][:, k - 1],
                           torch.full((nq // 2,), 2 ** 63 - 1, dtype=torch.int64))
    assert bool((lens >= 1500).all()) and bool((lens < 2000).all())            # so 4,000 holds exactly two
    assert _both_routes(idx, q, k, groups, None, want, budget=4000) == {"list": nq // 2, "threshold": nq // 2}
    assert _both_routes(idx, q, k, groups, None, want, budget=1) == {"list": nq // 2, "threshold": nq // 2}
    keep = _masks(N, 8)["half"]
    _both_routes(idx, q, k, groups, keep, G.grouped_topk(S, groups, k, keep), budget=4000)
    # the threshold route replaced the held threshold-search result; a copy taken before stays whole
    held = idx.search_above(q[:2], 0.5)
    copy = tuple(t.clone() for t in held)
    idx.search_grouped(q, k, groups, route=GROUP_ROUTE_THRESHOLD)
    assert all(torch.equal(a, b) for a, b in zip(held, copy))
    idx.close()


# ---- 3. the layers above ---------------------------------------------------------------------------
def test_text_index_and_finder_group_by():
    N, dim = 300, 64
    rows, q = _problem(N, dim, 3, 31)
    paths = [f"img/{i // 3}.jpg" for i in range(N)]                       # three rows per item
    texts = [("wallet" if i % 2 == 0 else "keys") + f" {i % 7}" for i in range(N)]
    ts = TextSearchIndex(embeddings=rows, image_paths=paths, texts=texts)
    unit = rows / rows.norm(dim=-1, keepdim=True)
    S = _scores(q, unit)
    by_path = torch.arange(N) // 3
    by_text = torch.tensor([sorted(set(texts), key=texts.index).index(t) for t in texts])
    keep = torch.tensor([t.startswith("wallet") for t in texts])

    def wallet(i, p, t):
        return t.startswith("wallet")

    cases = (("image_path", by_path), (lambda i, p, t: t, by_text), ((torch.arange(N) % 50).tolist(), torch.arange(N) % 50))
    for group_by, gids in cases:
        for allow, mask in ((None, None), (wallet, keep), (keep, keep)):
            want = G.grouped_topk(S, gids, 6, mask)
            got = ts.search_batch(q, 6, allow=allow, group_by=group_by)
            assert len(got) == 3 and G.same(got, want)
            res = ts.search_with_embedding(q[0], top_k=6, allow=allow, group_by=group_by)
            assert [r.index for r in res] == want[1][0].tolist()
            assert len({int(gids[r.index]) for r in res}) == len(res)      # one result per group
            assert all(r.image_path == paths[r.index] and r.text == texts[r.index] for r in res)
            assert torch.tensor([r.score for r in res]).view(torch.int32).tolist() == \
                want[0][0].view(torch.int32).tolist()
    # fewer groups than top_k: the pads are dropped
    res = ts.search_with_embedding(q[0], top_k=10, group_by=lambda i, p, t: t[:3])
    assert len(res) == 2 and {r.text[:3] for r in res} == {"wal", "key"}
    res = ts.search_with_embedding(q[0], top_k=10, group_by="text", allow=wallet)
    assert len(res) == len({t for t in texts if t.startswith("wallet")})
    # a reusable plan; today's calls untouched
    plan = ts._gpu.group_plan(by_path)
    assert G.same(ts.search_batch(q, 6, group_by=plan), G.grouped_topk(S, by_path, 6))
    assert len(ts.search_batch(q, 6)) == 2 and len(ts.search_with_embedding(q[0], top_k=5)) == 5

    from clip_lora_match_amd.finder import FinderIndex
    f = FinderIndex.__new__(FinderIndex)
    f.index = ts
    want = G.grouped_topk(S[:1], by_path, 5, keep)
    res = f.search(q[0], top_k=5, where=wallet, group_by="image_path")
    assert [r.index for r in res] == want[1][0].tolist() and len({r.image_path for r in res}) == 5
    want = G.grouped_topk(S[:1], by_path, 5)
    assert [r.index for r in f.search(q[0], top_k=5, group_by="image_path")] == want[1][0].tolist()
    assert [r.index for r in f.search(q[0], top_k=3)] == [r.index for r in ts.search_with_embedding(q[0], top_k=3)]


@pytest.mark.parametrize("parts", [2, 3])
def test_merge_grouped_gpu_equals_the_cpu_merge(parts):
    """shard lists as ShardedIndex.search_grouped gathers them: each part the k best groups of its row
    slice (groups span the slices, ties across them, an empty part), merged on the GPU and on the CPU --
    and both equal to the whole index's answer"""
    from clip_lora_match_amd.distributed import merge_grouped_gpu, shard_range
    N, dim, nq = 400, 64, 7
    rows, q = _problem(N, dim, nq, 41)
    rows[N - 1] = rows[0]
    q[0] = rows[0]
    S = _scores(q, rows)
    gen = torch.Generator().manual_seed(42)
    groups = torch.randint(0, 60, (N,), generator=gen) * 4096
    for k in (1, 5, 40, 100):
        ls = []
        for r in range(parts):
            a, b = shard_range(N, r, parts)
            ls.append(G.grouped_topk(S[:, a:b], groups[a:b], k, offset=a))
        ls.append(G.grouped_topk(S[:, :1], groups[:1], k, allow=torch.zeros(1, dtype=torch.bool)))   # an empty part
        s_all, i_all, g_all = (torch.cat([p[j] for p in ls], 1) for j in range(3))
        want = G.merge_grouped(s_all, i_all, g_all, parts + 1, k)
        assert G.same(want, G.grouped_topk(S, groups, k))
        got = merge_grouped_gpu(s_all.cuda(), i_all.cuda(), g_all.cuda(), parts + 1, k)
        assert all(t.is_cuda for t in got) and G.same(got, want), k


def test_sharded_index_world_one():
    """ShardedIndex.search_grouped at world size 1 (the collective plumbing at world 2 runs on CPU
    stand-ins in tests/test_group_host.py; the merge it would call is tested above)"""
    import socket

    import torch.distributed as dist
    from clip_lora_match_amd.distributed import ShardedIndex
    N, dim = 300, 64
    rows, q = _problem(N, dim, 4, 51)
    groups = torch.arange(N) // 3
    keep = _masks(N, 52)["half"]
    S = _scores(q, rows)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        sh = ShardedIndex(dim, N)
        sh.append_shard(rows)
        assert G.same(sh.search_grouped(q, 5, groups), G.grouped_topk(S, groups, 5))
        assert G.same(sh.search_grouped(q, 5, groups, allow=keep), G.grouped_topk(S, groups, 5, keep))
        with pytest.raises(ValueError):
            sh.search_grouped(q, 5, groups[:-1])
        sh.local.close()
    finally:
        dist.destroy_process_group()
