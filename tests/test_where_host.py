"""Host side of the keyed search: key_ranks / key_bounds against brute force (no device needed), the
ctypes prototypes of clm_index_search_keyed and clm_gemm_select_keyed and their null-index answer, and
ShardedIndex.search_where over gloo on CPU stand-in shards (tests/dist_where_worker.py)."""
import ctypes
import math
import socket

import numpy as np
import pytest
import torch

import mask_ref as M
import where_ref as R
from clip_lora_match_amd import _capi
from clip_lora_match_amd.search import KeyPlan, key_bounds, key_ranks


def _brute_ranks(values, allow=None):
    v = [float(x) for x in values.tolist()]
    uniq = sorted(set(v))
    keep = [True] * len(v) if allow is None else [bool(a) for a in allow.tolist()]
    keys = [uniq.index(x) if kp else -1 for x, kp in zip(v, keep)]
    cum = [sum(1 for x, kp in zip(v, keep) if kp and x < u) for u in uniq] + [sum(keep)]
    return keys, uniq, cum


VALUE_SETS = {
    "ints_with_duplicates": torch.tensor([5, 3, 5, 9, 3, 3, 12, 0, 9, 5], dtype=torch.int64),
    "int32": torch.tensor([2, 2, 2, 7, 1], dtype=torch.int32),
    "floats": torch.tensor([0.5, -1.25, 3.0, 0.5, 2.75, -1.25, 100.0], dtype=torch.float32),
    "doubles": torch.tensor([1e-3, 1e12, -1e12, 1e-3], dtype=torch.float64),
    "negatives": torch.tensor([-7, -7, -1, -300, 4, -1, 0], dtype=torch.int64),
    "one": torch.tensor([42], dtype=torch.int64),
    "all_equal": torch.full((6,), 3, dtype=torch.int16),
}


@pytest.mark.parametrize("name", sorted(VALUE_SETS))
def test_key_ranks_against_brute_force(name):
    v = VALUE_SETS[name]
    g = torch.Generator().manual_seed(len(name))
    for allow in (None, torch.rand(v.numel(), generator=g) < 0.5, torch.zeros(v.numel(), dtype=torch.bool)):
        keys, uniq, cum = key_ranks(v, allow)
        bk, bu, bc = _brute_ranks(v, allow)
        assert keys.dtype == torch.int32 and cum.dtype == torch.int64
        assert keys.tolist() == bk and [float(u) for u in uniq.tolist()] == bu and cum.tolist() == bc
        assert uniq.dtype == v.dtype
        if allow is not None:   # the sentinel: below every rank, so no range of key_bounds holds it
            assert bool((keys[~allow] == -1).all()) and bool((keys[allow] >= 0).all())


def _bounds_cases(v):
    """per-query (lo, hi) pairs: on values, between them, below and above them all, open, crossed"""
    s = sorted(set(float(x) for x in v.tolist()))
    inf = math.inf
    cases = [(None, None), (-inf, inf), (s[0], s[-1]), (s[0], s[0]), (s[-1], s[-1]), (s[0] - 10, s[0] - 1),
             (s[-1] + 1, s[-1] + 10), (s[0] - 1, s[-1] + 1), (None, s[len(s) // 2]), (s[len(s) // 2], None),
             (s[len(s) // 2], inf), (-inf, s[0]), (s[-1], s[0] - 1 if len(s) == 1 else s[0]), (inf, -inf),
             (inf, inf), (-inf, -inf)]
    for a, b in zip(s, s[1:]):
        mid = (a + b) / 2
        cases += [(mid, mid), (a, mid), (mid, b), (mid, inf)]
    return cases


@pytest.mark.parametrize("name", sorted(VALUE_SETS))
def test_key_bounds_against_brute_force(name):
    v = VALUE_SETS[name]
    g = torch.Generator().manual_seed(7 + len(name))
    for allow in (None, torch.rand(v.numel(), generator=g) < 0.6):
        keys, uniq, cum = key_ranks(v, allow)
        cases = _bounds_cases(v)
        lo = torch.tensor([-math.inf if a is None else a for a, _ in cases], dtype=torch.float64)
        hi = torch.tensor([math.inf if b is None else b for _, b in cases], dtype=torch.float64)
        klo, khi, n_in = key_bounds(uniq, cum, lo, hi)
        assert klo.dtype == torch.int32 and khi.dtype == torch.int32 and n_in.dtype == torch.int64
        assert klo.shape == khi.shape == n_in.shape == (len(cases),)
        want = R.open_rows(v, lo, hi, len(cases), allow)
        got = (keys[None, :] >= klo[:, None]) & (keys[None, :] <= khi[:, None])
        assert np.array_equal(got.numpy(), want), name
        assert n_in.tolist() == want.sum(1).tolist()          # n_in = the brute-force count
        crossed = lo > hi
        assert bool((klo[crossed] > khi[crossed]).all()) and bool((n_in[crossed] == 0).all())
        # one case at a time, as scalars and None: the same answer
        for j, (a, b) in enumerate(cases):
            o = key_bounds(uniq, cum, a, b, nq=1)
            assert (o[0].item(), o[1].item(), o[2].item()) == (klo[j].item(), khi[j].item(), n_in[j].item()), (a, b)


def test_key_bounds_broadcast_and_integer_bounds():
    v = torch.tensor([5, 3, 5, 9, 3, 3, 12, 0, 9, 5])
    keys, uniq, cum = key_ranks(v)
    klo, khi, n_in = key_bounds(uniq, cum, 3, torch.tensor([3, 5, 100, 2]))     # a scalar lo broadcasts
    assert n_in.tolist() == [3, 6, 9, 0] and klo.tolist() == [1, 1, 1, 1] and khi.tolist() == [1, 2, 4, 0]
    klo, khi, n_in = key_bounds(uniq, cum, None, None, nq=4)
    assert n_in.tolist() == [10] * 4 and klo.tolist() == [0] * 4 and khi.tolist() == [4] * 4
    klo, khi, n_in = key_bounds(uniq, cum, torch.tensor([4.5, 5.0]), 9.5)       # fractional bounds on integers
    assert n_in.tolist() == [5, 5] and klo.tolist() == [2, 2] and khi.tolist() == [3, 3]
    with pytest.raises(ValueError):
        key_bounds(uniq, cum, torch.tensor([1, 2, 3]), torch.tensor([1, 2]))
    with pytest.raises(ValueError):
        key_bounds(uniq, cum, float("nan"), 3)
    # no values at all: every range is empty
    k0, u0, c0 = key_ranks(torch.empty(0, dtype=torch.int64))
    assert k0.numel() == 0 and u0.numel() == 0 and c0.tolist() == [0]
    assert key_bounds(u0, c0, None, None, nq=2)[2].tolist() == [0, 0]


def test_nan_values_raise_and_allow_is_checked():
    with pytest.raises(ValueError):
        key_ranks(torch.tensor([1.0, float("nan"), 2.0]))
    with pytest.raises(ValueError):
        key_ranks(torch.tensor([1, 2, 3]), torch.tensor([True, False]))
    with pytest.raises(ValueError):
        key_ranks(torch.tensor([1, 2, 3]), torch.tensor([1, 0, 1]))
    assert KeyPlan.__dataclass_fields__.keys() >= {"keys", "uniq", "cum", "n"}


def test_prototypes_and_null_index():
    c_int, c_int64, c_void_p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert {"clm_index_search_keyed", "clm_gemm_select_keyed"} <= set(_capi.EXPORTED)
    L = _capi.lib()
    f = L.clm_index_search_keyed
    assert f.restype is c_int
    assert list(f.argtypes) == [c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                c_void_p, c_void_p, c_void_p]
    h = L.clm_gemm_select_keyed
    assert h.restype is c_int
    assert list(h.argtypes) == [c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_void_p,
                                c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_int, c_void_p]
    assert _capi.CLM_EPI_FILTER_KEYS == 9
    assert f(None, None, _capi.CLM_F32, 1, 1, None, None, None, None, 0, None, None, None) == _capi.CLM_E_ARG
    assert f(None, None, _capi.CLM_F32, 0, 1, None, None, None, None, 0, None, None, None) == _capi.CLM_E_ARG
    # the hook's argument answers come before any launch: no device needed
    buf = (c_int64 * 64)()
    p = ctypes.addressof(buf)
    assert h(0, 99, p, 64, p, 64, 1, 4, 64, None, p, p, 1, p, p, p, 4, 0, None, p, p, p, 1, None) == _capi.CLM_E_ARG
    assert h(0, -1, p, 64, p, 64, 1, 4, 64, None, p, p, 1, p, p, p, 4, 0, None, None, p, p, 1, None) == _capi.CLM_E_ARG
    assert h(0, -1, p, 64, p, 64, 1, 4, 64, None, p, p, 1, p, p, p, 4, 0, None, p, None, p, 1, None) == _capi.CLM_E_ARG
    assert h(0, -1, p, 64, p, 64, 1, 4, 64, None, p, p, 1, p, p, p, 4, 0, None, p, p, None, 1, None) == _capi.CLM_E_ARG
    assert h(0, -1, p, 64, p, 64, 1, 4, 64, None, p, p, 1, p, p, p, 4, 0, None, p + 4, p, p, 1, None) == _capi.CLM_E_ARG
    assert h(0, -1, None, 64, None, 64, 0, 4, 64, None, None, None, 1, None, None, None, 4, 0, None, None, None, None,
             1, None) == _capi.CLM_OK   # M == 0: nothing to do


def test_sharded_keyed_search_over_gloo():
    """world 2: n = 1 leaves rank 1 an empty shard, n = 2 one row each, 41 / 90 rows whose values repeat
    across both shards with score ties across them; every rank's result equals the whole index's
    yardstick, so the shards read the ranks alike"""
    import torch.multiprocessing as mp

    import dist_where_worker as W
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
        rows, q, values, keep = W.problem(n)
        S = M.cosines(q, rows)
        if n >= 41:   # the values do repeat across the shards
            assert set(values[: n // 2].tolist()) & set(values[n // 2:].tolist())
        for k in (1, 3, 8):
            for name, allow in (("all", None), ("half", keep), ("ids", keep)):
                lo, hi, kinds = R.ranges(values, allow, q.shape[0], k, n + k)
                want = R.keyed_topk(S, R.open_rows(values, lo, hi, q.shape[0], allow), k)
                for r in range(world):
                    assert not isinstance(got[r], str), got[r]
                    res = tuple(torch.from_numpy(a) for a in got[r][(n, k, name)])
                    assert M.same(res, want), (n, k, name, r, kinds)
