"""Host side of the filtered search: the ctypes prototype of clm_index_search_masked and its
null-argument answers (no device needed), the mask layout (mask_ref.pack, search.pack_mask,
CosineIndex.allow_mask on a stand-in), masked_topk on a hand-worked case, and
ShardedIndex.search(allow=) over gloo on CPU stand-in shards (tests/mask_ref.py)."""
import os
import socket

import numpy as np
import pytest
import torch

import mask_ref as M

NAN = float("nan")
INF = float("inf")


def test_ctypes_prototype_exists():
    from ctypes import c_int, c_int64, c_void_p
    from clip_lora_match_amd import _capi
    lib = _capi.lib()
    assert "clm_index_search_masked" in _capi.EXPORTED
    fn = lib.clm_index_search_masked
    assert fn.restype is c_int
    assert list(fn.argtypes) == [c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                 c_void_p]
    assert (_capi.CLM_MASK_EXACT, _capi.CLM_MASK_PASS, _capi.CLM_MASK_GATHER) == (1 << 30, 1 << 29, 1 << 28)
    # the statistics grew to 20 entries; a null index is still refused
    import ctypes
    assert lib.clm_index_stats2(None, (ctypes.c_int64 * 20)(), 20) == _capi.CLM_E_ARG


def test_null_arguments_are_argument_errors_without_a_device():
    import ctypes
    from clip_lora_match_amd import _capi
    lib = _capi.lib()
    q = (ctypes.c_float * 128)()
    allow = (ctypes.c_uint32 * 1)(3)
    s = (ctypes.c_float * 2)()
    ids = (ctypes.c_int64 * 2)()
    for n in (0, 2, -1):
        assert lib.clm_index_search_masked(None, q, _capi.CLM_F32, n, 1, allow, 0, s, ids, None) == _capi.CLM_E_ARG
        assert lib.clm_last_error()
        assert lib.clm_index_search_masked(None, None, _capi.CLM_F32, n, 1, None, 0, None, None, None) == _capi.CLM_E_ARG
        assert lib.clm_index_search_masked(None, q, _capi.CLM_BF16, n, 1, allow, 0, s, ids, None) == _capi.CLM_E_ARG
    assert lib.clm_index_search_masked(None, None, _capi.CLM_BF16, 0, 1, None, 0, None, None, None) == _capi.CLM_E_ARG


def test_pack_bit_order():
    from clip_lora_match_amd.search import pack_mask

    def both(keep):
        a = M.pack(keep)
        b = pack_mask(torch.tensor(keep, dtype=torch.bool))
        assert a.dtype == np.uint32 and b.dtype == torch.int32
        assert np.array_equal(a, b.numpy().view(np.uint32))
        return a.tolist()

    assert both([True]) == [1]
    assert both([False]) == [0]
    assert both([False] * 30 + [True]) == [1 << 30]                         # N = 31
    assert both([True] + [False] * 30 + [True]) == [0x80000001]             # N = 32: bit 31 is row 31
    assert both([True] * 32) == [0xFFFFFFFF]
    assert both([False] * 32 + [True]) == [0, 1]                            # N = 33: row 32 is bit 0 of word 1
    assert both([False, True] + [False] * 29 + [True, True]) == [0x80000002, 1]
    assert both([True] * 33) == [0xFFFFFFFF, 1]                             # the bits past N stay clear
    assert both([]) == []


class _StandIn:
    """what CosineIndex.allow_mask reads of its index: the size, the offset, the device"""

    def __init__(self, n, offset):
        self.n, self._offset, self.device = n, offset, torch.device("cpu")

    def __len__(self):
        return self.n


def test_allow_mask_forms_agree():
    from clip_lora_match_amd.search import CosineIndex
    for n, offset in ((1, 0), (33, 0), (70, 1000)):
        x = _StandIn(n, offset)
        g = torch.Generator().manual_seed(n)
        keep = torch.rand(n, generator=g) < 0.4
        keep[0] = True
        ids = torch.nonzero(keep).reshape(-1) + offset
        gone = torch.nonzero(~keep).reshape(-1) + offset
        a = CosineIndex.allow_mask(x, keep=keep)
        assert a.dtype == torch.int32 and a.numel() == (n + 31) // 32
        assert np.array_equal(a.numpy().view(np.uint32), M.pack(keep.numpy()))
        assert torch.equal(CosineIndex.allow_mask(x, ids=ids), a)
        assert torch.equal(CosineIndex.allow_mask(x, ids=ids.flip(0).tolist() + ids[:1].tolist()), a)   # order, duplicates
        assert torch.equal(CosineIndex.allow_mask(x, exclude=gone), a)
        assert torch.equal(CosineIndex.allow_mask(x, exclude=[]), CosineIndex.allow_mask(x, keep=torch.ones(n, dtype=torch.bool)))
        assert int(CosineIndex.allow_mask(x, ids=[]).abs().sum()) == 0
        for bad in (offset - 1, offset + n):
            with pytest.raises(ValueError):
                CosineIndex.allow_mask(x, ids=[offset, bad])
            with pytest.raises(ValueError):
                CosineIndex.allow_mask(x, exclude=[bad])
        with pytest.raises(ValueError):
            CosineIndex.allow_mask(x, keep=torch.ones(n + 1, dtype=torch.bool))
        with pytest.raises(ValueError):
            CosineIndex.allow_mask(x)
        with pytest.raises(ValueError):
            CosineIndex.allow_mask(x, keep=keep, ids=ids)


def test_allow_is_told_apart_by_dtype():
    """bool = keep, int64 = ids, int32 / uint32 = words; any other dtype is refused, so ids are never
    read as words"""
    from clip_lora_match_amd.search import CosineIndex
    x = _StandIn(70, 1000)
    x.allow_mask = lambda **kw: CosineIndex.allow_mask(x, **kw)
    keep = torch.zeros(70, dtype=torch.bool)
    keep[[0, 33, 69]] = True
    words = CosineIndex.allow_mask(x, keep=keep)
    assert torch.equal(CosineIndex._allow_words(x, keep), words)
    assert torch.equal(CosineIndex._allow_words(x, [1000, 1033, 1069]), words)
    assert torch.equal(CosineIndex._allow_words(x, torch.tensor([1069, 1000, 1033])), words)
    assert CosineIndex._allow_words(x, words) is not None and torch.equal(CosineIndex._allow_words(x, words), words)
    assert int(CosineIndex._allow_words(x, []).abs().sum()) == 0
    for bad in (torch.tensor([1000.0]), torch.tensor([1000], dtype=torch.int16), torch.tensor([3], dtype=torch.uint8)):
        with pytest.raises(TypeError):
            CosineIndex._allow_words(x, bad)


def test_masked_topk_hand_worked():
    # 2 queries x 6 rows. Query 0: a tie (rows 1 and 4 at 0.5) and a NaN on an allowed row (5), the best
    # number on a disallowed row (0). Query 1: the NaN sits on the disallowed row 2.
    S = torch.tensor([[0.9, 0.5, 0.7, -0.2, 0.5, NAN],
                      [0.1, 0.3, NAN, 0.3, -0.4, 0.2]])
    allow = [False, True, False, True, True, True]
    s, i = M.masked_topk(S, allow, 3)
    assert i.tolist() == [[5, 1, 4], [1, 3, 5]]
    assert torch.isnan(s[0, 0]) and s[0, 1:].tolist() == [0.5, 0.5]
    assert torch.equal(s[1], torch.tensor([0.3, 0.3, 0.2]))
    # k past the allowed rows: a (-inf, -1) tail; an offset moves the ids only
    s, i = M.masked_topk(S, allow, 6, offset=100)
    assert i.tolist() == [[105, 101, 104, 103, -1, -1], [101, 103, 105, 104, -1, -1]]
    assert s[:, 4:].tolist() == [[-INF, -INF], [-INF, -INF]] and s[1, 3] == torch.tensor(-0.4)
    # nothing allowed; everything allowed
    s, i = M.masked_topk(S, [False] * 6, 2)
    assert i.tolist() == [[-1, -1], [-1, -1]] and bool((s == -INF).all())
    s, i = M.masked_topk(S, [True] * 6, 2)
    assert i.tolist() == [[5, 0], [2, 1]]
    assert M.same((s, i), (s.clone(), i.clone())) and not M.same((s, i), (s, i + 1))


def _problem():
    g = torch.Generator().manual_seed(43)
    rows = torch.randn(10, 16, generator=g)
    rows[8] = rows[1]        # a tie across shards
    q = torch.randn(4, 16, generator=g)
    q[1] = rows[1] + 0.1 * q[1]
    q[2] = 0                 # a zero query: NaN scores, the allowed rows in id order
    masks = [torch.tensor([1, 1, 0, 1, 0, 0, 0, 0, 1, 0], dtype=torch.bool),    # world 3: shard [4, 7) has none
             torch.tensor([1, 1, 0, 1, 0, 0, 0, 0, 0, 0], dtype=torch.bool),    # world 2: shard [5, 10) has none
             torch.zeros(10, dtype=torch.bool), torch.ones(10, dtype=torch.bool)]
    return rows, q, masks


def _worker(rank, world, port, out):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch.distributed as dist
    import mask_ref
    from clip_lora_match_amd.distributed import ShardedIndex
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        rows, q, masks = _problem()
        sh = ShardedIndex(16, rows.shape[0], local_factory=lambda: mask_ref.TorchIndex(16))
        sh.append_shard(rows[sh.start: sh.stop])
        res = []
        for m in masks:
            res.append(tuple(t.numpy().copy() for t in sh.search(q, 3, merge=mask_ref.merge, allow=m)))
            res.append(tuple(t.numpy().copy() for t in sh.search(q, 3, merge=mask_ref.merge,
                                                          allow=torch.nonzero(m).reshape(-1))))   # the ids form
        res.append(tuple(t.numpy().copy() for t in sh.search(q[0], 6, merge=mask_ref.merge, allow=masks[0])))
        out.put((rank, res))   # numpy arrays: pickled by value, no descriptor outlives the worker
    except Exception as e:  # pragma: no cover
        out.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_masked_search_over_gloo(world):
    import torch.multiprocessing as mp
    from clip_lora_match_amd.distributed import shard_range
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
    rows, q, masks = _problem()
    # the case holds a shard without an allowed row
    assert any(not bool(m[slice(*shard_range(10, r, world))].any()) for m in masks[:2] for r in range(world))
    whole = M.TorchIndex(16)
    whole.append(rows)
    want = []
    for m in masks:
        want += [whole.search(q, 3, allow=m)] * 2
    want.append(whole.search(q[:1], 6, allow=masks[0]))
    assert want[0][1][1].tolist()[:2] == [1, 8]   # the tie across shards, by id
    assert want[-1][1][0].tolist()[4:] == [-1, -1]
    assert torch.isnan(want[0][0][2]).all() and want[0][1][2].tolist() == [0, 1, 3]
    for r in range(world):
        assert not isinstance(got[r], str), got[r]
        assert len(got[r]) == len(want)
        for g, w in zip(got[r], want):
            assert M.same(tuple(torch.from_numpy(a) for a in g), w), f"rank {r}"
