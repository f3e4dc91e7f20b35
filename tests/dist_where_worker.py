"""Worker of tests/test_where_host.py::test_sharded_keyed_search_over_gloo: ShardedIndex.search_where over
gloo on the CPU stand-in shards of tests/where_ref.py, merged by mask_ref.merge. Every rank puts its
results on the queue as numpy arrays; the test compares them with the single-index yardstick."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def problem(n, dim=16, nq=9):
    """rows with duplicates (exact ties across the shards), integer values with repeats spread over the
    whole index, a half mask, and one range of every kind per batch"""
    g = torch.Generator().manual_seed(200 + n)
    rows = torch.randn(n, dim, generator=g)
    if n > 8:
        rows[n - 2] = rows[1]
        rows[5] = rows[2]
    q = torch.randn(nq, dim, generator=g)
    q[0] = rows[1 % n] + 0.01 * q[0]
    values = torch.randint(-5, max(n // 2, 1), (n,), generator=g)
    keep = torch.rand(n, generator=g) < 0.5
    return rows, q, values, keep


def run(rank, world, port, sizes, out):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import torch.distributed as dist

    import mask_ref
    import where_ref
    from clip_lora_match_amd.distributed import ShardedIndex
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        res = {}
        for n in sizes:
            rows, q, values, keep = problem(n)
            sh = ShardedIndex(16, n, local_factory=lambda: where_ref.TorchIndex(16))
            if sh.stop > sh.start:
                sh.append_shard(rows[sh.start: sh.stop])
            for k in (1, 3, 8):
                for name, allow in (("all", None), ("half", keep), ("ids", torch.nonzero(keep).reshape(-1))):
                    lo, hi, _ = where_ref.ranges(values, keep if allow is not None else None, q.shape[0], k, n + k)
                    got = sh.search_where(q, k, values, lo, hi, allow=allow, merge=mask_ref.merge)
                    res[(n, k, name)] = tuple(np.array(t.numpy()) for t in got)
        out.put((rank, res))   # numpy arrays: pickled by value, no descriptor outlives the worker
    except Exception as e:  # pragma: no cover
        import traceback
        out.put((rank, repr(e) + traceback.format_exc()))
    finally:
        dist.destroy_process_group()
