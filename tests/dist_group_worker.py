"""Worker of tests/test_group_host.py::test_sharded_grouped_search_over_gloo: ShardedIndex.search_grouped
over gloo on the CPU stand-in shards of tests/group_ref.py, merged by group_ref.merge_grouped. Every rank
puts its results on the queue as numpy arrays; the test compares them with the single-index restatement."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def problem(n, dim=16, nq=6):
    """rows with duplicates (exact ties), groups of about 3 rows spread over the whole index -- so they
    span the shards --, a half mask, queries near a row and Gaussian"""
    g = torch.Generator().manual_seed(100 + n)
    rows = torch.randn(n, dim, generator=g)
    if n > 8:
        rows[n - 2] = rows[1]          # a tie across the two shards of world 2
        rows[5] = rows[2]
    q = torch.randn(nq, dim, generator=g)
    q[0] = rows[1 % n] + 0.01 * q[0]
    groups = torch.randint(0, max(n // 3, 1), (n,), generator=g) * 7 + 3   # sparse ids
    keep = torch.rand(n, generator=g) < 0.5
    return rows, q, groups, keep


def run(rank, world, port, sizes, out):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import torch.distributed as dist

    import group_ref
    from clip_lora_match_amd.distributed import ShardedIndex
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        res = {}
        for n in sizes:
            rows, q, groups, keep = problem(n)
            sh = ShardedIndex(16, n, local_factory=lambda: group_ref.TorchIndex(16))
            if sh.stop > sh.start:
                sh.append_shard(rows[sh.start: sh.stop])
            for k in (1, 3, 8):
                for name, allow in (("all", None), ("half", keep), ("ids", torch.nonzero(keep).reshape(-1))):
                    got = sh.search_grouped(q, k, groups, allow=allow, merge=group_ref.merge_grouped)
                    res[(n, k, name)] = tuple(np.array(t.numpy()) for t in got)
        out.put((rank, res))   # numpy arrays: pickled by value, no descriptor outlives the worker
    except Exception as e:  # pragma: no cover
        import traceback
        out.put((rank, repr(e) + traceback.format_exc()))
    finally:
        dist.destroy_process_group()
