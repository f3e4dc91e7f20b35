"""Host side of the mutable index: the shard bookkeeping of ShardedIndex.remove on hand-worked
cases, ShardedIndex.remove itself over gloo on CPU stand-in shards, the ctypes prototypes of
clm_index_remove / clm_index_update, and their null-index answers (no device needed)."""
import os
import socket

import pytest
import torch

from clip_lora_match_amd.distributed import ranges_after_remove


def test_ranges_after_remove_hand_worked():
    # three shards of 4, 3, 3 rows: global rows 0-3 | 4-6 | 7-9
    sizes, starts = [4, 3, 3], [0, 4, 7]
    # nothing removed
    assert ranges_after_remove(sizes, starts, []) == ([[], [], []], [4, 3, 3], [0, 4, 7])
    # 1 and 3 from shard 0, 7 from shard 2 (unsorted, 3 twice): 2 | 3 | 2 rows -> starts 0, 2, 5
    assert ranges_after_remove(sizes, starts, [7, 3, 1, 3]) == ([[1, 3], [], [7]], [2, 3, 2], [0, 2, 5])
    # the whole middle shard goes: it is left empty, at the start of the next one
    assert ranges_after_remove(sizes, starts, [6, 4, 5]) == ([[], [4, 5, 6], []], [4, 0, 3], [0, 4, 4])
    # the first shard emptied, one row of the last
    assert ranges_after_remove(sizes, starts, [0, 1, 2, 3, 9]) == ([[0, 1, 2, 3], [], [9]], [0, 3, 2], [0, 0, 3])
    # everything
    local, new_sizes, new_starts = ranges_after_remove(sizes, starts, range(10))
    assert local == [[0, 1, 2, 3], [4, 5, 6], [7, 8, 9]] and new_sizes == [0, 0, 0] and new_starts == [0, 0, 0]
    # shards that start at an offset and were already uneven (after an earlier remove); tensor ids
    assert ranges_after_remove([2, 0, 5], [0, 2, 2], torch.tensor([2, 6])) == ([[], [], [2, 6]], [2, 0, 3], [0, 2, 2])
    for bad in ([10], [-1], [3, 99]):
        with pytest.raises(ValueError):
            ranges_after_remove(sizes, starts, bad)
    with pytest.raises(ValueError):
        ranges_after_remove([1, 2], [0], [0])


class _ListIndex:
    """stand-in for CosineIndex: a list of row labels with the same remove / set_offset contract"""

    def __init__(self):
        self.rows, self.offset = [], 0

    def __len__(self):
        return len(self.rows)

    def set_offset(self, off):
        self.offset = off

    def append(self, rows):
        self.rows.extend(int(r) for r in rows)

    def remove(self, ids):
        gone = {int(i) - self.offset for i in ids}
        assert all(0 <= g < len(self.rows) for g in gone)
        self.rows = [r for j, r in enumerate(self.rows) if j not in gone]
        return len(gone)


def _worker(rank, world, port, q):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    from clip_lora_match_amd.distributed import ShardedIndex
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        sh = ShardedIndex(4, 10, local_factory=_ListIndex)      # rows 0-3 | 4-6 | 7-9
        sh.append_shard(torch.arange(sh.start, sh.stop))
        res = [sh.remove([5, 4, 6, 0, 9, 9])]                   # the middle rank is left empty
        res.append((sh.start, sh.stop, sh.n_total, sh.local.offset, list(sh.local.rows)))
        res.append(sh.remove([3, 2]))                           # new ids: old rows 7 and 3
        res.append((sh.start, sh.stop, sh.n_total, sh.local.offset, list(sh.local.rows)))
        try:
            sh.remove([sh.n_total])
            res.append("no error")
        except ValueError:
            res.append("ValueError")
        q.put((rank, res))
    except Exception as e:  # pragma: no cover
        q.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


def test_sharded_remove_over_gloo():
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 3, port, q)) for r in range(3)]
    for p in procs:
        p.start()
    out = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert out[0] == [5, (0, 3, 5, 0, [1, 2, 3]), 2, (0, 2, 3, 0, [1, 2]), "ValueError"]
    assert out[1] == [5, (3, 3, 5, 3, []), 2, (2, 2, 3, 2, []), "ValueError"]
    assert out[2] == [5, (3, 5, 5, 3, [7, 8]), 2, (2, 3, 3, 2, [8]), "ValueError"]


def test_ctypes_prototypes_exist():
    from ctypes import c_int, c_int64, c_void_p
    from clip_lora_match_amd import _capi
    assert "clm_index_remove" in _capi.EXPORTED and "clm_index_update" in _capi.EXPORTED
    lib = _capi.lib()
    assert lib.clm_index_remove.restype is c_int
    assert list(lib.clm_index_remove.argtypes) == [c_void_p, c_void_p, c_int64, c_void_p]
    assert lib.clm_index_update.restype is c_int
    assert list(lib.clm_index_update.argtypes) == [c_void_p, c_void_p, c_void_p, c_int, c_int64, c_void_p]


def test_null_index_is_an_argument_error_without_a_device():
    import ctypes
    from clip_lora_match_amd import _capi
    lib = _capi.lib()
    ids = (ctypes.c_int64 * 2)(0, 1)
    rows = (ctypes.c_float * 128)()
    for n in (0, 2, -1):
        assert lib.clm_index_remove(None, ids, n, None) == _capi.CLM_E_ARG
        assert lib.clm_last_error()
        assert lib.clm_index_update(None, ids, rows, _capi.CLM_F32, n, None) == _capi.CLM_E_ARG
    assert lib.clm_index_remove(None, None, 0, None) == _capi.CLM_E_ARG
    assert lib.clm_index_update(None, None, None, _capi.CLM_BF16, 0, None) == _capi.CLM_E_ARG
