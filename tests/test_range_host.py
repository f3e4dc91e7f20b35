"""Host side of the threshold search: the ctypes prototypes of clm_index_search_above / _rows /
_read and their null-index answers (no device needed), merge_ragged on hand-worked cases,
ShardedIndex.search_above over gloo on CPU stand-in shards (tests/range_ref.py), and
threshold_metrics against the reference's own functions through the golden."""
import os
import socket

import numpy as np
import pytest
import torch

from conftest import golden

import range_ref as R
from clip_lora_match_amd.distributed import merge_ragged
from clip_lora_match_amd.evaluate import threshold_metrics

NAN = float("nan")


def test_ctypes_prototypes_exist():
    from ctypes import c_int, c_int64, c_void_p
    from clip_lora_match_amd import _capi
    lib = _capi.lib()
    want = {
        "clm_index_search_above": [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p, c_int, c_void_p],
        "clm_index_search_above_rows": [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int, c_void_p],
        "clm_index_search_above_read": [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p],
    }
    for name, args in want.items():
        assert name in _capi.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is c_int and list(fn.argtypes) == args


def test_null_index_is_an_argument_error_without_a_device():
    import ctypes
    from clip_lora_match_amd import _capi
    lib = _capi.lib()
    q = (ctypes.c_float * 128)()
    tau = (ctypes.c_float * 2)(0.5, 0.5)
    off = (ctypes.c_int64 * 3)()
    s = (ctypes.c_float * 2)()
    ids = (ctypes.c_int64 * 2)()
    for n in (0, 2, -1):
        assert lib.clm_index_search_above(None, q, _capi.CLM_F32, n, tau, off, 0, None) == _capi.CLM_E_ARG
        assert lib.clm_last_error()
        assert lib.clm_index_search_above_rows(None, 0, n, tau, off, 0, None) == _capi.CLM_E_ARG
        assert lib.clm_index_search_above_read(None, 0, n, s, ids, None) == _capi.CLM_E_ARG
    assert lib.clm_index_search_above(None, None, _capi.CLM_BF16, 0, None, None, 0, None) == _capi.CLM_E_ARG


def _triple(off, s, i):
    return torch.tensor(off, dtype=torch.int64), torch.tensor(s, dtype=torch.float32), torch.tensor(i, dtype=torch.int64)


def test_merge_ragged_hand_worked():
    # three queries over three shards (rows 0-3 | 4-6 | 7-9); the middle shard has nothing for
    # query 0, the last shard nothing at all
    a = _triple([0, 2, 3, 3], [0.9, 0.5, 0.8], [3, 1, 0])
    b = _triple([0, 0, 2, 3], [0.8, 0.7, 0.6], [5, 4, 6])
    c = _triple([0, 0, 0, 0], [], [])
    off, s, i = merge_ragged([a, b, c])
    assert off.tolist() == [0, 2, 5, 6]
    assert i.tolist() == [3, 1, 0, 5, 4, 6]          # query 1: the 0.8 tie across shards goes by id
    assert torch.equal(s, torch.tensor([0.9, 0.5, 0.8, 0.8, 0.7, 0.6]))
    assert off.dtype == torch.int64 and s.dtype == torch.float32 and i.dtype == torch.int64
    # the parts in another order merge to the same thing
    again = merge_ragged([c, b, a])
    assert all(torch.equal(x, y) for x, y in zip(again, (off, s, i)))
    # NaN above every number, NaNs among themselves by id; -0.0 below 0.0 only by its bits' order
    a = _triple([0, 3], [NAN, 0.2, -1.0], [9, 2, 0])
    b = _triple([0, 3], [NAN, float("inf"), 0.2], [4, 11, 1])
    off, s, i = merge_ragged([a, b])
    assert i.tolist() == [4, 9, 11, 1, 2, 0] and torch.isnan(s[:2]).all() and s[2:].tolist()[0] == float("inf")
    # one shard is the identity; no shard, or shards that disagree on nq, are errors
    one = merge_ragged([_triple([0, 1, 1], [0.5], [7])])
    assert one[0].tolist() == [0, 1, 1] and one[2].tolist() == [7]
    empty = merge_ragged([_triple([0], [], []), _triple([0], [], [])])
    assert empty[0].tolist() == [0] and empty[1].numel() == 0
    with pytest.raises(ValueError):
        merge_ragged([])
    with pytest.raises(ValueError):
        merge_ragged([_triple([0, 1], [0.5], [7]), _triple([0, 1, 1], [0.5], [8])])
    with pytest.raises(ValueError):
        merge_ragged([_triple([0, 2], [0.5], [7])])


def _problem():
    g = torch.Generator().manual_seed(41)
    rows = torch.randn(103, 32, generator=g)
    q = torch.randn(9, 32, generator=g)
    q[::2] = rows[torch.arange(0, 100, 20)] + 0.4 * q[::2]
    q[3] = 0          # a zero query: every score NaN, every row returned in id order
    tau = torch.tensor([0.3, 0.3, -float("inf"), 0.3, 0.3, 2.0, 0.1, NAN, 0.3])
    return rows, q, tau


def _worker(rank, world, port, out):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch.distributed as dist
    import range_ref
    from clip_lora_match_amd.distributed import ShardedIndex
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        rows, q, tau = _problem()
        sh = ShardedIndex(32, rows.shape[0], local_factory=lambda: range_ref.TorchIndex(32))
        sh.append_shard(rows[sh.start: sh.stop])
        res = [tuple(t.clone() for t in sh.search_above(q, tau))]
        res.append(tuple(t.clone() for t in sh.search_above(q[0], 0.3)))      # one query, a scalar threshold
        out.put((rank, res))
    except Exception as e:  # pragma: no cover
        out.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_search_above_over_gloo(world):
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, out)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(out.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    rows, q, tau = _problem()
    whole = R.TorchIndex(32)
    whole.append(rows)
    want = [whole.search_above(q, tau), whole.search_above(q[:1], 0.3)]
    lens = want[0][0][1:] - want[0][0][:-1]
    assert lens[2] == 103 and lens[3] == 103 and lens[5] == 0 and lens[7] == 0 and 0 < lens[0] < 103
    for r in range(world):
        assert not isinstance(got[r], str), got[r]
        for g, w in zip(got[r], want):
            assert R.same(g, w), f"rank {r}"


def test_threshold_metrics_against_the_reference():
    """the golden holds what the reference's evaluate_single_query + calculate_* + evaluate_epoch's
    means give on the fixture (tests/golden/make_threshold_golden.py); threshold_metrics gets the
    same numbers from the relevant-set sizes alone"""
    g = golden("threshold_metrics.npz")
    assert float(g["min_gap"]) > 1e-5
    ks = [int(k) for k in g["k_values"]]
    counts = np.diff(g["relevant_offsets"])
    n_index = g["index"].shape[0]
    assert (counts == 0).sum() >= 5 and (counts == 1).sum() >= 5 and (counts > max(ks)).sum() >= 3   # every branch
    m = threshold_metrics(counts, n_index, ks)
    assert m["num_queries"] == counts.size == g["queries"].shape[0]
    for j, k in enumerate(ks):
        assert abs(m["recall"][k] - g["recall"][j]) <= 1e-12
        assert abs(m["precision"][k] - g["precision"][j]) <= 1e-12
    assert abs(m["mrr"] - g["mrr"]) <= 1e-12 and abs(m["map"] - g["map"]) <= 1e-12
    # per query too: a single query's metrics are its own means
    for i in range(counts.size):
        one = threshold_metrics(counts[i: i + 1], n_index, ks)
        for j, k in enumerate(ks):
            assert abs(one["recall"][k] - 100 * g["q_recall"][j, i]) <= 1e-12
            assert abs(one["precision"][k] - 100 * g["q_precision"][j, i]) <= 1e-12
        assert one["mrr"] == g["q_rr"][i] and one["map"] == pytest.approx(g["q_ap"][i], abs=1e-12)
    # the CPU restatement of the rule finds the golden's relevant sets (float64 cosines: the gap
    # check makes membership independent of the arithmetic)
    off, _, ids = R.above_from_scores(R.cosines(g["queries"], g["index"]), float(g["threshold"]))
    assert torch.equal(off, torch.from_numpy(g["relevant_offsets"]))
    for i in range(counts.size):
        a, b = int(off[i]), int(off[i + 1])
        assert sorted(ids[a:b].tolist()) == g["relevant_ids"][a:b].tolist()
    for bad in ([], [-1], [n_index + 1]):
        with pytest.raises(ValueError):
            threshold_metrics(bad, n_index, ks)
