"""Host side of the grouped search: the ctypes prototype of clm_topk_distinct and its argument answers
(no device needed), the restatement tests/group_ref.py against a brute-force walk, the row bound
(k - 1) m + 1 of the list route, the group_by key-to-id mapping, and ShardedIndex.search_grouped over
gloo on CPU stand-in shards (tests/dist_group_worker.py)."""
import socket

import numpy as np
import pytest
import torch

import group_ref as G
from clip_lora_match_amd import _capi
from clip_lora_match_amd.search import (GroupPlan, TextSearchIndex, group_ids_from_keys, group_row_bound, pack_mask,
                                        unpack_mask)


def test_hook_is_exported_and_refuses_bad_arguments():
    assert "clm_topk_distinct" in _capi.EXPORTED
    f = _capi.lib().clm_topk_distinct
    assert f(0, None, None, None, None, 4, 0, 5, None, None, None, None, None) == _capi.CLM_OK       # nq == 0
    assert f(0, None, None, None, None, 4, 2, 5, None, None, None, None, None) == _capi.CLM_E_ARG    # null, nq > 0
    buf = (_capi.c_int64 * 64)()
    p = _capi.ctypes.addressof(buf)
    for nq, ld, k in ((1, 4, 0), (1, 4, 1025), (-1, 4, 5), (1, -1, 5)):
        assert f(0, p, p, p, None, ld, nq, k, p, p, p, p, None) == _capi.CLM_E_ARG, (nq, ld, k)
    assert f(0, p, p, p, None, 4, 1, 5, p, p, p, p, None) == _capi.CLM_E_ARG   # host memory is refused
    assert b"device" in _capi.lib().clm_last_error()


def _walk(S, groups, k, allow, offset):
    """the rule, by selection: repeatedly take the best remaining allowed row (NaN before numbers,
    then the larger score, then the smaller id), keep it iff its group is new"""
    nq, N = S.shape
    res = []
    for q in range(nq):
        left = [j for j in range(N) if allow[j]]
        seen, kept = set(), []
        while left and len(kept) < k:
            best = left[0]
            for j in left[1:]:
                a, b = S[q, j], S[q, best]
                ahead = (np.isnan(a) and not np.isnan(b)) or (not np.isnan(a) and not np.isnan(b) and a > b) or \
                    ((a == b or (np.isnan(a) and np.isnan(b))) and j < best)
                if ahead:
                    best = j
            left.remove(best)
            if groups[best] not in seen:
                seen.add(groups[best])
                kept.append((S[q, best], best + offset, groups[best]))
        kept += [(np.float32(-np.inf), -1, -1)] * (k - len(kept))
        res.append(kept)
    return res


@pytest.mark.parametrize("seed", range(8))
def test_reference_equals_the_brute_force_walk(seed):
    rng = np.random.default_rng(seed)
    N, nq = int(rng.integers(1, 40)), 5
    S = rng.integers(-3, 4, (nq, N)).astype(np.float32) / 4          # few values: many exact ties
    if seed % 2:
        S[:, rng.integers(0, N, 2)] = np.nan                          # NaN columns (a zero row)
        S[0, :] = np.nan                                              # and an all-NaN query
    groups = rng.integers(0, max(N // 3, 1), N) * (1 << 33) + 5
    allow = rng.random(N) < 0.7 if seed % 3 else np.ones(N, bool)
    for k in (1, 4, N, N + 3):
        got = G.grouped_topk(S, groups, k, allow, offset=1000)
        want = _walk(S, groups, k, allow, 1000)
        ws = torch.tensor([[e[0] for e in row] for row in want], dtype=torch.float32)
        wi = torch.tensor([[e[1] for e in row] for row in want], dtype=torch.int64)
        wg = torch.tensor([[e[2] for e in row] for row in want], dtype=torch.int64)
        assert G.same(got, (ws, wi, wg)), (seed, k)
    # every row a group of its own: the plain (masked) search
    own = G.grouped_topk(S, np.arange(N), 4, allow, 7)
    import mask_ref
    assert mask_ref.same(own[:2], mask_ref.masked_topk(S, allow, 4, 7))
    assert torch.equal(own[2], torch.where(own[1] >= 0, own[1] - 7, own[1]))


def test_distinct_lists_by_hand():
    s = np.array([.9, .8, .8, .7, .6, .5], np.float32)
    i = np.array([4, 1, -1, 9, 2, 3], np.int64)
    g = np.array([7, 7, 5, 8, 7, 9], np.int64)
    os_, oi, og, found = G.distinct_lists(s, i, g, [0, 6, 6], 3)
    assert oi.tolist() == [[4, 9, 3], [-1, -1, -1]] and og.tolist() == [[7, 8, 9], [-1, -1, -1]]
    assert os_[0].tolist() == [np.float32(.9), np.float32(.7), np.float32(.5)] and found.tolist() == [3, 0]
    assert torch.isinf(os_[1]).all()


@pytest.mark.parametrize("seed", range(6))
def test_row_bound(seed):
    """the first (k - 1) m + 1 rows of ANY order hold k distinct groups or every row; one row fewer
    does not when k - 1 groups of m rows lead"""
    rng = np.random.default_rng(seed)
    N = int(rng.integers(5, 60))
    groups = rng.integers(0, max(N // 4, 1), N)
    m = int(np.bincount(groups).max())
    for k in (1, 2, 5, 9):
        b = group_row_bound(k, m)
        assert b == (k - 1) * m + 1
        for _ in range(20):
            order = rng.permutation(N)
            head = groups[order[:b]]
            assert len(set(head.tolist())) >= k or b >= N
    # tight: k - 1 full groups first
    k, m = 4, 3
    groups = np.array([0] * 3 + [1] * 3 + [2] * 3 + [3, 4])
    assert len(set(groups[: group_row_bound(k, m) - 1].tolist())) == k - 1
    assert len(set(groups[: group_row_bound(k, m)].tolist())) == k


def test_group_by_key_mapping():
    assert group_ids_from_keys(["b", "a", "b", ("x", 1), "a", 3]).tolist() == [0, 1, 0, 2, 1, 3]
    assert group_ids_from_keys([]).dtype == torch.int64
    t = TextSearchIndex.__new__(TextSearchIndex)
    t.num_items = 6
    t.image_paths = ["p0", "p1", "p0", "p2", "p1"]          # shorter than the index: row 5 has no path
    t.texts = ["a", "a", "b", "b", "a", "c"]
    assert t.group_ids("image_path").tolist() == [0, 1, 0, 2, 1, 3]
    assert t.group_ids("text").tolist() == [0, 0, 1, 1, 0, 2]
    assert t.group_ids(lambda i, p, x: (p, x)).tolist() == [0, 1, 2, 3, 1, 4]
    assert t.group_ids(lambda i, p, x: i // 4).tolist() == [0, 0, 0, 0, 1, 1]
    assert t.group_ids([5, 5, 9, 9, 0, 0]).tolist() == [5, 5, 9, 9, 0, 0]   # ids are taken as they are
    assert torch.equal(t.group_ids(torch.arange(6)), torch.arange(6))
    t.image_paths = ["row", "row"]                           # a path never collides with a pathless row's key
    assert t.group_ids("image_path").tolist() == [0, 0, 1, 2, 3, 4]
    with pytest.raises(ValueError):
        t.group_ids("caption")


def test_unpack_mask_inverts_pack_mask():
    g = torch.Generator().manual_seed(3)
    for n in (1, 31, 32, 33, 255, 3000):
        keep = torch.rand(n, generator=g) < 0.5
        keep[n - 1] = True
        assert torch.equal(unpack_mask(pack_mask(keep), n), keep)
    assert GroupPlan.__dataclass_fields__.keys() >= {"gids", "allow", "m", "n_groups", "reps"}


def test_sharded_grouped_search_over_gloo():
    """world 2: n = 1 leaves rank 1 an empty shard, n = 2 one row each, 41 / 90 groups that span both
    shards with ties across them; every rank's result equals the whole index's restatement"""
    import torch.multiprocessing as mp

    import dist_group_worker as W
    import mask_ref
    sizes, world = (1, 2, 41, 90), 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=W.run, args=(r, world, port, sizes, out)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(out.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    for n in sizes:
        rows, q, groups, keep = W.problem(n)
        S = mask_ref.cosines(q, rows)
        if n >= 41:   # the groups do span the shards
            assert set(groups[: n // 2].tolist()) & set(groups[n // 2:].tolist())
        for k in (1, 3, 8):
            for name, allow in (("all", None), ("half", keep), ("ids", keep)):
                want = G.grouped_topk(S, groups, k, allow)
                for r in range(world):
                    assert not isinstance(got[r], str), got[r]
                    res = tuple(torch.from_numpy(a) for a in got[r][(n, k, name)])
                    assert G.same(res, want), (n, k, name, r)
