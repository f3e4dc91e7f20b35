"""In-place mutation of the resident index (CosineIndex.remove / .update, clm_index_remove /
clm_index_update, include/clm.h) and the layers on top (TextSearchIndex, FinderIndex, ShardedIndex).

Yardstick: a FRESH index -- one built by appending the final rows in order, each run of rows in
its final dtype. "Equal" is byte-equal clm_index_export output (fp16 operands, inverse norms, fp32
rows), equal size and has_f32, and bitwise-equal search scores and ids. Nothing here has a
tolerance except the TextSearchIndex / oracle comparison, which uses the suite's existing 2e-6
near-tie rule (oracle/search_ref.py).

CLM_MUTATE_CHUNK_ROWS=256 makes a removal over 3000 rows span a dozen chunks (the default chunk is
what 64 MiB of staging holds: tens of thousands of rows), so every pattern crosses chunk borders;
one pattern runs with the default chunk, and one index is large enough to cross a default chunk.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

from clip_lora_match_amd import _capi as C
from clip_lora_match_amd import synthetic as syn
from clip_lora_match_amd.search import CosineIndex, TextSearchIndex
from oracle import search_ref as S

pytestmark = pytest.mark.gpu
N = 3000
CHUNK = 256


# ------------------------------------------------------------------ helpers --
def _state(ix):
    """(n, has_f32, rows16, inv, rows32) as integer tensors (bit patterns)"""
    n, L = len(ix), C.lib()
    has32 = int(L.clm_index_has_f32(ix._h))
    r16 = torch.zeros((n, ix.dim_p), dtype=torch.float16)
    inv = torch.zeros((n,), dtype=torch.float32)
    r32 = torch.zeros((n, ix.dim_p), dtype=torch.float32) if has32 else None
    if n:
        C.check(L.clm_index_export(ix._h, 0, n, C.ptr(r16), C.ptr(inv), C.ptr(r32) if has32 else None,
                                   C.stream_of(ix.device)), "export")
    return (n, has32, r16.view(torch.int16), inv.view(torch.int32),
            r32.view(torch.int32) if has32 else torch.zeros(0, dtype=torch.int32))


def _same_state(a, b):
    sa, sb = _state(a), _state(b)
    assert sa[0] == sb[0], f"size {sa[0]} vs fresh {sb[0]}"
    if sa[0]:   # an emptied index keeps its fp32 copy, an index built from no rows never had one
        assert sa[1] == sb[1], f"has_f32 {sa[1]} vs fresh {sb[1]}"
    for name, x, y in zip(("rows16", "inv", "rows32"), sa[2:], sb[2:]):
        if name == "rows32" and not sa[0]:
            continue
        assert x.shape == y.shape, name
        if not torch.equal(x, y):
            bad = torch.nonzero((x != y).reshape(x.shape[0], -1).any(1)).flatten()
            raise AssertionError(f"{name} differs from the fresh index in {bad.numel()} rows, first {bad[:5].tolist()}")


def _same_search(a, b, queries, k):
    s1, i1 = a.search(queries, k)
    s2, i2 = b.search(queries, k)
    assert torch.equal(i1, i2), "search ids differ from the fresh index"
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32)), "search scores differ from the fresh index"


def _same(a, b, queries, k=10):
    _same_state(a, b)
    _same_search(a, b, queries, max(1, min(k, len(b))) if len(b) else 3)


def _build(items, dim, offset=0):
    """a CosineIndex from a list of per-row tensors (fp16 or fp32): runs of one dtype are appended
    together, in order -- the fresh index of the module docstring"""
    ix = CosineIndex(dim, capacity=8)
    i = 0
    while i < len(items):
        j = i
        while j < len(items) and items[j].dtype == items[i].dtype:
            j += 1
        ix.append(torch.stack(items[i:j]))
        i = j
    if offset:
        ix.set_offset(offset)
    return ix


_data = {}


def _items(dim, kind, n=N, seed=11):
    """n rows of varied norms as per-row tensors; kind f16 / f32 / mixed (f16, f32, f16 thirds)"""
    key = (dim, kind, n, seed)
    if key not in _data:
        rng = np.random.Generator(np.random.PCG64(seed + dim))
        x = rng.standard_normal((n, dim), dtype=np.float32) * rng.uniform(0.25, 4.0, (n, 1)).astype(np.float32)
        t32 = torch.from_numpy(x)
        t16 = t32.half()
        if kind == "f16":
            rows = list(t16)
        elif kind == "f32":
            rows = list(t32)
        else:
            a, b = n // 3, 2 * n // 3
            rows = list(t16[:a]) + list(t32[a:b]) + list(t16[b:])
        _data[key] = rows
    return _data[key]


def _queries(dim, nq=8, seed=5):
    return torch.from_numpy(syn.gaussian_rows(nq, dim, seed, fp16=False))


PATTERNS = {
    "empty": [],
    "first": [0],
    "last": [N - 1],
    "every_other": list(range(0, N, 2)),
    "all": list(range(N)),
    # chunks start at the first removed row: 100 + 256 is the first chunk boundary
    "straddle": [100] + list(range(100 + CHUNK - 10, 100 + CHUNK + 10)),
    "more_than_a_chunk": list(range(500, 500 + 3 * CHUNK - 68)),
    "unsorted_dups": [2999, 5, 5, 1700, 0, 1700, 256, 255, 1024, 5],
}


# ------------------------------------------------------------------- remove --
@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("kind", ["f16", "f32", "mixed"])
@pytest.mark.parametrize("dim", [64, 100, 512])
def test_remove_equals_fresh_index(monkeypatch, dim, kind, pattern):
    monkeypatch.setenv("CLM_MUTATE_CHUNK_ROWS", str(CHUNK))
    items = _items(dim, kind)
    ids = PATTERNS[pattern]
    ix = _build(items, dim)
    assert C.lib().clm_index_has_f32(ix._h) == (0 if kind == "f16" else 1)
    removed = ix.remove(ids)
    gone = set(ids)
    assert removed == len(gone) and len(ix) == N - len(gone)
    assert C.lib().clm_index_has_f32(ix._h) == (0 if kind == "f16" else 1)
    fresh_items = [r for j, r in enumerate(items) if j not in gone]
    fresh = _build(fresh_items, dim)
    _same(ix, fresh, _queries(dim))
    # the index goes on working: appending after a removal equals appending to the fresh index
    # (an fp16 row: it leaves has_f32 as it is on both)
    if fresh_items:
        extra = _items(dim, "f16", 5, seed=99)
        ix.append(torch.stack(extra))
        fresh.append(torch.stack(extra))
        _same(ix, fresh, _queries(dim))
    ix.close()
    fresh.close()


def test_remove_default_chunk(monkeypatch):
    monkeypatch.delenv("CLM_MUTATE_CHUNK_ROWS", raising=False)
    items = _items(512, "mixed")
    ix = _build(items, 512)
    ids = PATTERNS["every_other"]
    assert ix.remove(torch.tensor(ids, device="cuda")) == len(ids)   # a device id list
    fresh = _build([r for j, r in enumerate(items) if j % 2], 512)
    _same(ix, fresh, _queries(512))
    ix.close()
    fresh.close()


def test_remove_crosses_a_default_chunk(monkeypatch):
    """600,000 x 64 fp16 rows are 132 B of staging each: the default 64 MiB chunk holds 508,400 of
    them, so removing row 0 (every row moves, by one) takes two chunks through the staging buffer."""
    monkeypatch.delenv("CLM_MUTATE_CHUNK_ROWS", raising=False)
    n, dim = 600_000, 64
    g = torch.Generator(device="cuda").manual_seed(3)
    rows = torch.randn((n, dim), generator=g, device="cuda", dtype=torch.float32).half()
    ix = CosineIndex(dim, capacity=n)
    ix.append(rows)
    assert ix.remove([0, 508_399, 508_400, n - 1]) == 4
    keep = torch.ones(n, dtype=torch.bool, device="cuda")
    keep[[0, 508_399, 508_400, n - 1]] = False
    fresh = CosineIndex(dim, capacity=n)
    fresh.append(rows[keep])
    _same(ix, fresh, _queries(dim))
    ix.close()
    fresh.close()


# ------------------------------------------------------------------- update --
@pytest.mark.parametrize("chunk", [64, None])
@pytest.mark.parametrize("index_kind,row_dtype", [("f32", torch.float32), ("f16", torch.float16),
                                                  ("f16", torch.float32), ("mixed", torch.float16)])
def test_update_equals_fresh_index(monkeypatch, index_kind, row_dtype, chunk):
    if chunk is None:
        monkeypatch.delenv("CLM_MUTATE_CHUNK_ROWS", raising=False)
    else:
        monkeypatch.setenv("CLM_MUTATE_CHUNK_ROWS", str(chunk))
    dim = 100
    items = _items(dim, index_kind)
    ix = _build(items, dim)
    rng = np.random.Generator(np.random.PCG64(21))
    ids = rng.permutation(N)[:300].tolist()
    ids[0], ids[1] = 0, N - 1
    ids = list(dict.fromkeys(ids))
    new = _items(dim, "f32", len(ids), seed=77)
    new = [r.to(row_dtype) for r in new]
    ix.update(ids, torch.stack(new))
    assert len(ix) == N
    want32 = 0 if (index_kind == "f16" and row_dtype == torch.float16) else 1
    assert C.lib().clm_index_has_f32(ix._h) == want32
    final = list(items)
    for i, r in zip(ids, new):
        final[i] = r
    fresh = _build(final, dim)
    _same(ix, fresh, torch.cat([_queries(dim), torch.stack(new[:4]).float()]))
    ix.close()
    fresh.close()


def test_update_from_device_rows_and_ids():
    dim = 64
    items = _items(dim, "f32")
    ix = _build(items, dim)
    ids = [7, 2999, 1500]
    new = torch.stack(_items(dim, "f32", 3, seed=78))
    ix.update(torch.tensor(ids, device="cuda"), new.cuda())
    final = list(items)
    for i, r in zip(ids, new):
        final[i] = r
    fresh = _build(final, dim)
    _same(ix, fresh, _queries(dim))
    ix.close()
    fresh.close()


# ------------------------------------------------------------- stale caches --
BIG_N, BIG_DIM, BIG_NQ = 40_000, 64, 32


def _big(kind):
    rows = syn.gaussian_rows(BIG_N, BIG_DIM, 31, fp16=(kind == "f16"))
    qs = syn.gaussian_rows(BIG_NQ, BIG_DIM, 32, fp16=True)   # fp16-exact: a copy is a copy in either dtype
    return torch.from_numpy(rows), torch.from_numpy(qs)


def _fresh_big(rows):
    ix = CosineIndex(BIG_DIM, capacity=BIG_N)
    ix.append(rows)
    return ix


def _check_other_entry_points(ix, fresh, qs, n):
    tg = torch.arange(0, BIG_NQ, dtype=torch.int64) * 997 % n
    r1, s1 = ix.rank(qs, tg)
    r2, s2 = fresh.rank(qs, tg)
    assert torch.equal(r1, r2) and torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    assert torch.equal(ix.count_above(qs, s2, tg), fresh.count_above(qs, s2, tg))
    l1, e1 = ix.logsumexp(qs, 100.0)
    l2, e2 = fresh.logsumexp(qs, 100.0)
    assert torch.equal(l1.view(torch.int64), l2.view(torch.int64)) and torch.equal(e1, e2)


@pytest.mark.parametrize("kind", ["f16", "f32"])
def test_update_rebuilds_the_threshold_sample_and_order_keys(monkeypatch, kind):
    """The sampled threshold and the [cmin, cmax] order keys of the inverse norms are cached per
    index size; update leaves the size alone. After 200 replaced rows -- among them, for every
    query, an exact copy of the query, some at norms outside the old range -- a search must see
    the new rows exactly as a fresh index does."""
    monkeypatch.setenv("CLM_SEARCH_BOUNDED", "1")
    rows, qs = _big(kind)
    ix = _fresh_big(rows)
    f0 = ix.stats()["filtered"]
    ix.search(qs.float(), 10)   # caches the sample and the order keys
    assert ix.stats()["filtered"] - f0 == BIG_NQ, "the sampled bounded search did not serve the queries"
    rng = np.random.Generator(np.random.PCG64(33))
    ids = rng.permutation(BIG_N)[:200]
    new = torch.from_numpy(syn.gaussian_rows(200, BIG_DIM, 34, fp16=(kind == "f16"))).clone()
    new[:BIG_NQ] = qs.to(new.dtype)
    # rows of norm 8 and 1/8 (exact in fp16): inverse norms outside the old [cmin, cmax] ~ 1
    new[:8] *= 8
    new[8:16] /= 8
    new[100:104] *= 8
    ix.update(ids, new)
    final = rows.clone()
    final[torch.from_numpy(ids)] = new
    fresh = _fresh_big(final)
    _, i = ix.search(qs.float(), 10)
    assert torch.equal(i[:, 0].cpu(), torch.from_numpy(ids[:BIG_NQ])), "a query's own copy is not its best match"
    _same(ix, fresh, qs.float())
    _check_other_entry_points(ix, fresh, qs.float(), BIG_N)
    ix.close()
    fresh.close()


def test_remove_after_a_cached_search(monkeypatch):
    monkeypatch.setenv("CLM_SEARCH_BOUNDED", "1")
    rows, qs = _big("f32")
    ix = _fresh_big(rows)
    _, top = ix.search(qs.float(), 10)
    ids = torch.unique(top[:, :3].reshape(-1).cpu())          # every query loses its three best matches
    ids = torch.unique(torch.cat([ids, torch.arange(5, BIG_N, 211)]))
    assert ix.remove(ids) == ids.numel()
    keep = torch.ones(BIG_N, dtype=torch.bool)
    keep[ids] = False
    fresh = _fresh_big(rows[keep])
    assert len(fresh) >= 4 * 8192
    _same(ix, fresh, qs.float())
    _check_other_entry_points(ix, fresh, qs.float(), len(fresh))
    ix.close()
    fresh.close()


# ------------------------------------------------------ other search routes --
@pytest.mark.parametrize("route", ["scan16", "exact_scan", "large_k"])
def test_other_search_routes_after_a_mutation(monkeypatch, route):
    monkeypatch.setenv("CLM_MUTATE_CHUNK_ROWS", str(CHUNK))
    dim = 512
    items = _items(dim, "mixed")
    ix = _build(items, dim)
    gone = set(range(3, N, 5))
    ix.remove(sorted(gone))
    final = [r for j, r in enumerate(items) if j not in gone]
    upd = [0, 17, len(final) - 1]
    new = _items(dim, "f32", 3, seed=55)
    ix.update(upd, torch.stack(new))
    for i, r in zip(upd, new):
        final[i] = r
    fresh = _build(final, dim)
    key = {"scan16": "small_scan", "exact_scan": "full_exact", "large_k": "full_exact"}[route]
    before = ix.stats()[key]
    if route == "scan16":
        monkeypatch.setenv("CLM_SEARCH_SMALLQ", "1")
        qs, k = _queries(dim, 4), 10
    elif route == "exact_scan":
        qs, k = _queries(dim, 8), 10
    else:
        qs, k = _queries(dim, 8), 1500
    _same_state(ix, fresh)
    _same_search(ix, fresh, qs, k)
    served = ix.stats()[key] - before
    assert served == qs.shape[0] if route != "scan16" else served >= 1
    ix.close()
    fresh.close()


# -------------------------------------------------------------- offset, errors --
def test_ids_are_global(monkeypatch):
    monkeypatch.setenv("CLM_MUTATE_CHUNK_ROWS", str(CHUNK))
    dim = 64
    items = _items(dim, "f32")
    ix = _build(items, dim, offset=1000)
    before = _state(ix)
    new = torch.stack(_items(dim, "f32", 2, seed=56))
    for bad in ([0], [999], [1000 + N], [1000, 5]):
        with pytest.raises(ValueError):
            ix.remove(bad)
        with pytest.raises(ValueError):
            ix.update(bad, new[: len(bad)])
    after = _state(ix)
    assert all(torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b for a, b in zip(before, after))
    assert ix.remove([1000, 1000 + N - 1, 1500]) == 3
    ix.update([1000, 1000 + N - 4], new)
    final = [r for j, r in enumerate(items) if j not in (0, N - 1, 500)]
    final[0], final[N - 4] = new[0], new[1]
    fresh = _build(final, dim, offset=1000)
    _same(ix, fresh, _queries(dim))
    assert int(ix.search(_queries(dim), 1)[1].min()) >= 1000
    ix.close()
    fresh.close()


def test_errors_leave_the_index_untouched():
    L, dim = C.lib(), 64
    ix = _build(_items(dim, "mixed"), dim)
    st = C.stream_of(ix.device)
    before = _state(ix)
    ids = torch.tensor([3, 4], dtype=torch.int64)
    dup = torch.tensor([3, 3], dtype=torch.int64)
    neg = torch.tensor([3, -1], dtype=torch.int64)
    past = torch.tensor([3, N], dtype=torch.int64)
    rows = torch.ones((2, dim), dtype=torch.float32)
    E = C.CLM_E_ARG
    assert L.clm_index_remove(None, C.ptr(ids), 2, st) == E
    assert L.clm_index_remove(ix._h, None, 2, st) == E
    assert L.clm_index_remove(ix._h, C.ptr(ids), -1, st) == E
    assert L.clm_index_remove(ix._h, C.ptr(neg), 2, st) == E
    assert L.clm_index_remove(ix._h, C.ptr(past), 2, st) == E
    assert L.clm_index_remove(ix._h, C.ptr(past.cuda()), 2, st) == E
    assert L.clm_index_update(None, C.ptr(ids), C.ptr(rows), C.CLM_F32, 2, st) == E
    assert L.clm_index_update(ix._h, None, C.ptr(rows), C.CLM_F32, 2, st) == E
    assert L.clm_index_update(ix._h, C.ptr(ids), None, C.CLM_F32, 2, st) == E
    assert L.clm_index_update(ix._h, C.ptr(ids), C.ptr(rows), C.CLM_F32, -1, st) == E
    assert L.clm_index_update(ix._h, C.ptr(ids), C.ptr(rows), C.CLM_BF16, 2, st) == E
    assert L.clm_index_update(ix._h, C.ptr(ids), C.ptr(rows), C.CLM_I32, 2, st) == E
    assert L.clm_index_update(ix._h, C.ptr(neg), C.ptr(rows), C.CLM_F32, 2, st) == E
    assert L.clm_index_update(ix._h, C.ptr(past), C.ptr(rows), C.CLM_F32, 2, st) == E
    assert L.clm_index_update(ix._h, C.ptr(dup), C.ptr(rows), C.CLM_F32, 2, st) == E
    assert b"duplicate" in L.clm_last_error()
    # n == 0: CLM_OK and a no-op, with or without pointers
    assert L.clm_index_remove(ix._h, None, 0, st) == C.CLM_OK
    assert L.clm_index_remove(ix._h, C.ptr(ids), 0, st) == C.CLM_OK
    assert L.clm_index_update(ix._h, None, None, C.CLM_F32, 0, st) == C.CLM_OK
    after = _state(ix)
    assert all(torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b for a, b in zip(before, after))
    # the Python layer's own checks
    with pytest.raises(ValueError):
        ix.update([1, 2], rows[:1])
    with pytest.raises(ValueError):
        ix.update([1], torch.ones((1, dim + 1)))
    ix.close()


# ---------------------------------------------------------- TextSearchIndex --
TD = 128   # dim == the padded dim: load_shard maps the file's fp32 rows as the host mirror


def _text_index(n=500, dim=TD, short=False):
    E = torch.from_numpy(syn.gaussian_rows(n, dim, 61, fp16=False)) * 3.0
    paths = [f"p{i}" for i in range(n if not short else 200)]
    texts = [f"t{i}" for i in range(n if not short else 450)]
    return E, paths, texts


def test_text_index_remove_and_update_against_the_oracle(tmp_path):
    E, paths, texts = _text_index()
    ix = TextSearchIndex(embeddings=E, image_paths=paths, texts=texts)
    gone = [499, 3, 3, 250, 0, 77]
    assert ix.remove(gone) == 5
    keep = [i for i in range(500) if i not in set(gone)]
    assert ix.num_items == 495 == len(ix.image_paths) == len(ix.texts) == ix.embeddings.shape[0]
    assert ix.image_paths == [paths[i] for i in keep] and ix.texts == [texts[i] for i in keep]
    new = torch.from_numpy(syn.gaussian_rows(2, TD, 62, fp16=False)) * 0.5
    ix.update([10, 494], new, image_paths=["np10", "np494"], texts=["nt10", "nt494"])
    surv = (E / E.norm(dim=-1, keepdim=True))[keep].clone()
    surv[[10, 494]] = new / new.norm(dim=-1, keepdim=True)
    assert torch.equal(ix.embeddings, surv)
    want_paths = [paths[i] for i in keep]
    want_paths[10], want_paths[494] = "np10", "np494"
    qs = torch.cat([surv[[0, 10, 123, 494]], torch.from_numpy(syn.gaussian_rows(4, TD, 63, fp16=False))])
    exact = S.cosine_scores(qs.numpy().astype(np.float64), surv.numpy().astype(np.float64))
    _, oi = S.topk(exact, 5)
    for j in range(qs.shape[0]):
        res = ix.search_with_embedding(qs[j], top_k=5)
        got = np.array([r.index for r in res])
        assert S.same_topk_up_to_ties(got, oi[j], exact[j], 2e-6)
        for r in res:   # the survivors' metadata at their new positions
            assert r.image_path == want_paths[r.index]
            assert r.text == ("nt%d" % r.index if r.index in (10, 494) else texts[keep[r.index]])
    assert [ix.search_with_embedding(qs[j], 1)[0].index for j in range(4)] == [0, 10, 123, 494]
    # save + reload and save_shard + load_shard reproduce the mutated index
    ix.save(tmp_path / "m.pt")
    ix.save_shard(tmp_path / "m.shard")
    a = TextSearchIndex(tmp_path / "m.pt")
    b = TextSearchIndex.load_shard(tmp_path / "m.shard")
    for other in (a, b):
        assert other.num_items == 495 and other.image_paths == want_paths and other.texts == ix.texts
        assert torch.equal(other.embeddings, ix.embeddings) or other is a
    _same(b._gpu, ix._gpu, qs)
    s1, i1 = ix.search_batch(qs, 5)
    s2, i2 = a.search_batch(qs, 5)   # the .pt reload re-normalises the saved rows (search.py:68)
    assert torch.equal(i1, i2) and torch.allclose(s1, s2, atol=1e-6, rtol=0)
    # a shard-loaded index (host mirror = a copy-on-write map of the file) mutates like any other
    b.remove([1, 2])
    b.update([0], new[:1])
    ix.remove([1, 2])
    ix.update([0], new[:1])
    assert torch.equal(b.embeddings, ix.embeddings) and b.image_paths == ix.image_paths
    _same(b._gpu, ix._gpu, qs)
    b.save_shard(tmp_path / "m2.shard")
    c = TextSearchIndex.load_shard(tmp_path / "m2.shard")
    assert torch.equal(c.embeddings, ix.embeddings) and c.texts == ix.texts
    _same(c._gpu, ix._gpu, qs)
    with pytest.raises(ValueError):
        ix.remove([ix.num_items])
    with pytest.raises(ValueError):
        ix.update([1, 1], new)


def test_text_index_from_gpu_index_stays_unfetched_and_short_metadata():
    E, paths, texts = _text_index(short=True)   # 200 paths and 450 texts for 500 rows
    gpu = CosineIndex(TD)
    gpu.append(E)
    ix = TextSearchIndex.from_gpu_index(gpu, paths, texts)
    gone = [100, 300, 480]
    assert ix.remove(gone) == 3
    ix.update([150, 460], E[:2], image_paths=["a", "b"], texts=["c", "d"])
    assert ix._host is None, "remove / update fetched the host mirror"
    assert ix.num_items == 497 and ix._n == 497 and len(gpu) == 497
    # paths: position 100 deleted (199 left), 150 replaced; texts: 100 and 300 deleted (448 left),
    # 150 replaced; position 460 has no text and no path
    assert len(ix.image_paths) == 199 and ix.image_paths[150] == "a" and ix.image_paths[100] == "p101"
    assert len(ix.texts) == 448 and ix.texts[150] == "c" and ix.texts[299] == "t301" and ix.texts[447] == "t449"
    r = ix.search_with_embedding(E[499], top_k=1)[0]   # old row 499 is row 496 now, past both lists
    assert r.index == 496 and r.image_path == "" and r.text == ""
    r = ix.search_with_embedding(E[0], top_k=2)
    assert {x.index for x in r} == {0, 150}
    keep = [i for i in range(500) if i not in gone]
    want = E[keep].clone()     # the wrapped index keeps its rows as they were appended ...
    want[[150, 460]] = (E / E.norm(dim=-1, keepdim=True))[[0, 1]]   # ... update re-normalises the new ones
    assert torch.equal(ix.embeddings, gpu.read(0, 497))     # fetched now, from the mutated index
    assert torch.allclose(ix.embeddings, want, atol=1e-7, rtol=0)


# -------------------------------------------------------------- FinderIndex --
class _WordTokenizer:
    """a stand-in tokenizer for the tiny preset (vocab 1000): one id per word"""

    def __init__(self, cfg):
        self.cfg = cfg

    def __call__(self, texts, padding=True, truncation=True, max_length=None, return_tensors="pt"):
        import zlib
        rows = []
        for t in texts:
            ids = [2 + zlib.crc32(w.encode()) % 900 for w in t.replace(",", " ").split()][: max_length - 2]
            rows.append([self.cfg.bos_token_id] + ids + [self.cfg.eos_token_id])
        width = max(len(r) for r in rows)
        rows = [r + [self.cfg.eos_token_id] * (width - len(r)) for r in rows]
        return {"input_ids": torch.tensor(rows, dtype=torch.int64)}


def test_finder_resolve_and_update(tmp_path):
    import clip_lora_match_amd as clm
    from clip_lora_match_amd import weights as W
    from clip_lora_match_amd.engine import ClipLoraModel
    from clip_lora_match_amd.finder import FinderIndex
    from clip_lora_match_amd.processor import ClipProcessor
    from PIL import Image

    cfg = clm.get_preset("tiny")
    model = ClipLoraModel(cfg, device="cuda:0", compute_dtype="float16", max_batch=8)
    model.load_tensors(W.synthetic_state_dict(cfg, 0))
    model.load_tensors(W.synthetic_lora(cfg, 1))
    model.finalize()
    proc = ClipProcessor(cfg)
    proc.tokenizer = _WordTokenizer(cfg)
    assert max(cfg.bos_token_id, cfg.eos_token_id) < cfg.vocab
    imgs = syn.images_u8(3, cfg.image_size, 91)
    paths = []
    for i in range(3):
        paths.append(tmp_path / f"img{i}.png")
        Image.fromarray(imgs[i]).save(paths[-1])
    up = tmp_path / "data" / "reported"
    pt = tmp_path / "data" / "index.pt"
    fi = FinderIndex(model, proc, "cuda:0", pt, root_dir=tmp_path, upload_dir=up, save_every=0)
    desc = ["dompet hitam kulit", "red backpack with laptop", "payung biru lipat"]
    recs = fi.report_items(paths, desc, locations=["kantin", None, "perpustakaan"])
    assert [r["id"] for r in recs] == [0, 1, 2]

    def emb(text):
        return model.encode_ids(proc.token_ids(text).to(model.device)).cpu()[0]

    # each description's own embedding, as the index stores it: it finds its item with score 1
    q = [fi.index.embeddings[j].clone() for j in range(3)]
    full = [fi.search(q[j], 3) for j in range(3)]
    assert [h[0].index for h in full] == [0, 1, 2] and all(abs(h[0].score - 1.0) < 1e-6 for h in full)
    fi.save_every = 1
    rec = fi.resolve_item(1)
    assert rec == {"id": 1, "image_path": "data/reported/img1.png", "description": "red backpack with laptop"}
    assert (up / "img1.png").exists()   # uploaded files are kept
    assert fi.index.num_items == 2
    # the resolved item's own embedding finds only the other two, at the scores they had, under
    # their new ids: 0 and 1 are the old 0 and 2
    renum = {0: 0, 2: 1}
    for j in range(3):
        want = [(renum[h.index], h.score, h.text, h.image_path) for h in full[j] if h.index != 1]
        got = [(h.index, h.score, h.text, h.image_path) for h in fi.search(q[j], 5)]
        assert got == want, (j, got, want)
    r0, r2 = fi.search(q[0], 1)[0], fi.search(q[2], 1)[0]
    assert (r0.index, r0.text, r0.image_path) == (0, recs[0]["description"], "data/reported/img0.png")
    assert (r2.index, r2.text, r2.image_path) == (1, recs[2]["description"], "data/reported/img2.png")
    # save_every=1: the resolve flushed, and the .pt has two rows
    obj = torch.load(pt, map_location="cpu", weights_only=True)
    assert obj["embeddings"].shape == (2, cfg.proj_dim) and obj["texts"] == [recs[0]["description"], recs[2]["description"]]
    assert obj["image_paths"] == ["data/reported/img0.png", "data/reported/img2.png"]
    # update_item: the corrected description's embedding is the item's row now
    os.remove(pt)
    new = fi.update_item(0, "black leather wallet", location="kantin")
    assert new["id"] == 0 and new["description"] == "black leather wallet, ditemukan di kantin"
    qn = emb(new["description"])
    assert not torch.equal(qn, q[0])
    hit = [h for h in fi.search(qn, 2) if h.index == 0][0]
    assert abs(hit.score - 1.0) < 1e-6 and hit.text == new["description"]
    assert hit.image_path == "data/reported/img0.png"
    assert torch.allclose(fi.index.embeddings[0], qn / qn.norm(), atol=1e-7, rtol=0)
    old = [h for h in fi.search(q[0], 2) if h.index == 0][0]   # the old description scores as any other query
    assert abs(old.score - float(q[0].double() @ (qn / qn.norm()).double())) < 1e-6
    assert pt.exists()   # counted toward save_every
    obj = torch.load(pt, map_location="cpu", weights_only=True)
    assert obj["texts"][0] == new["description"] and obj["embeddings"].shape[0] == 2
    with pytest.raises(ValueError):
        fi.resolve_item(2)
    with pytest.raises(ValueError):
        fi.resolve_items([0, 0])
    with pytest.raises(ValueError):
        fi.update_item(5, "x")
    assert fi.resolve_items([1, 0]) == [
        {"id": 1, "image_path": "data/reported/img2.png", "description": recs[2]["description"]},
        {"id": 0, "image_path": "data/reported/img0.png", "description": new["description"]}]
    assert fi.index.num_items == 0 and fi.search(qn, 3) == []
    model.close()


# ------------------------------------------------------------ ShardedIndex --
def test_sharded_remove_world2(tmp_path):
    """ShardedIndex.remove at world 2 on one GPU (gloo), through tests/dist_mutate_worker.py."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = tmp_path / "res.json"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.join(REPO, "tests", "dist_mutate_worker.py"),
           str(out)]
    p = subprocess.run(cmd, env=dict(os.environ, MASTER_ADDR="127.0.0.1"), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads(out.read_text())
    assert r["world"] == 2 and r["removed"] == [r["n_ids"]] * 2
    assert r["ranges"] == [[0, r["ranges"][0][1]], [r["ranges"][0][1], 1000 - r["n_ids"]]]   # contiguous
    assert r["local_sizes"] == [r["ranges"][0][1], 1000 - r["n_ids"] - r["ranges"][0][1]]
    assert r["n_total"] == [1000 - r["n_ids"]] * 2
    m = r["ranges2"][0][1]
    assert r["ranges2"] == [[0, m], [m, 1000 - r["n_ids"] - 4]] and m == r["ranges"][0][1] - 2
    assert r["took_from_both"] and r["bad_id_raised"] == [True, True]
    for key in ("search_idx_equal", "search_scores_equal", "second_remove_equal"):
        assert r[key], (key, r)
