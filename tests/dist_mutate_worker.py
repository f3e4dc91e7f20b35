"""Worker of tests/test_gpu_index_mutate.py::test_sharded_remove_world2: one rank of a world-2 job on
ONE GPU over gloo (RCCL refuses two ranks per device), launched by torch.distributed.run. 1000 fp32
rows row-sharded over the ranks (ShardedIndex over CosineIndex), ids from both shards removed on
every rank; rank 0 compares the merged search with a single fresh index of the surviving rows and
writes a JSON verdict."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from clip_lora_match_amd import synthetic as syn  # noqa: E402
from clip_lora_match_amd.distributed import ShardedIndex  # noqa: E402
from clip_lora_match_amd.search import CosineIndex  # noqa: E402


def _gather(obj):
    out = [None] * dist.get_world_size()
    dist.all_gather_object(out, obj)
    return out


def main(out_path):
    torch.cuda.set_device(0)
    os.environ["CLM_MUTATE_CHUNK_ROWS"] = "64"   # several chunks per shard
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    n, dim, nq, k = 1000, 64, 16, 10
    rows = torch.from_numpy(syn.gaussian_rows(n, dim, 71, fp16=False)) * 2.0
    qs = torch.from_numpy(syn.gaussian_rows(nq, dim, 72, fp16=False))
    qs[:4] = rows[[0, 499, 500, 999]]   # survivors at the shard edges
    sh = ShardedIndex(dim, n)
    sh.append_shard(rows[sh.start:sh.stop])
    rng = np.random.Generator(np.random.PCG64(73))
    ids = sorted(set(rng.permutation(n)[:120].tolist()) - {0, 499, 500, 999}) + [498, 501, 501]
    res = {"world": world, "n_ids": len(set(ids)),
           "took_from_both": any(i < 500 for i in ids) and any(i >= 500 for i in ids)}
    try:
        sh.remove(ids + [n])
        bad = False
    except ValueError:
        bad = len(sh.local) == sh.stop - sh.start == 500
    removed = sh.remove(ids)
    res["removed"] = _gather(removed)
    res["ranges"] = _gather([sh.start, sh.stop])
    res["local_sizes"] = _gather(len(sh.local))
    res["n_total"] = _gather(sh.n_total)
    s1, i1 = sh.search(qs, k)
    # a second removal: the renumbered ids are what the ranks now take
    second = [0, sh.n_total - 1, sh.stop - 1 if rank == 0 else sh.start]
    second = sorted(set(sum(_gather(second), [])))
    sh.remove(second)
    s2, i2 = sh.search(qs, k)
    res["bad_id_raised"] = _gather(bad)
    res["ranges2"] = _gather([sh.start, sh.stop])
    if rank == 0:
        keep = torch.ones(n, dtype=torch.bool)
        keep[ids] = False
        one = CosineIndex(dim)
        one.append(rows[keep])
        so, io = one.search(qs, k)
        res["search_idx_equal"] = bool(torch.equal(i1, io))
        res["search_scores_equal"] = bool(torch.equal(s1, so))
        keep2 = torch.ones(len(one), dtype=torch.bool)
        keep2[second] = False
        two = CosineIndex(dim)
        two.append(rows[keep][keep2])
        st, it = two.search(qs, k)
        res["second_remove_equal"] = bool(torch.equal(i2, it) and torch.equal(s2, st))
        json.dump(res, open(out_path, "w"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
