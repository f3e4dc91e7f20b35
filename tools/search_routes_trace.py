"""One call per route of the search host layer (capi_search.cpp), for a kernel trace that two builds
can be compared on: the same kernel names with the same call counts mean the same launches.

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o routes -- python tools/search_routes_trace.py
  python tools/search_routes_trace.py --table OUT/.../routes_kernel_stats.csv

The index is 262,144 x 128 fp16 with 64 queries (nq x N = 2^24 is the exact scan's bound, so the
routes are asked for by flag or environment); the small-batch call has 4 queries, the overflow call
an index of 300,000 x 96 with two groups of near-duplicate rows. The route counters are printed at
the end, one JSON line."""
import csv
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def table(path):
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "")
            name = re.sub(r"\(.*", "", name).replace("clm::", "")   # no argument list; template arguments kept
            rows[name] = rows.get(name, 0) + int(r["Calls"])
    for name in sorted(rows):
        print(f"{rows[name]:6d}  {name}")
    print(f"{sum(rows.values()):6d}  total, {len(rows)} kernels")


def env(**kv):
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def main():
    import torch

    from clip_lora_match_amd import _capi as C
    from clip_lora_match_amd.search import CosineIndex

    n, dim, nq, k = 262_144, 128, 64, 5
    g = torch.Generator(device="cuda").manual_seed(7)
    rows = torch.randn((n, dim), generator=g, device="cuda").half()
    q = torch.randn((nq, dim), generator=g, device="cuda").half()
    idx = CosineIndex(dim, capacity=n)
    idx.append(rows)
    env(CLM_SEARCH_BOUNDED="1")
    idx.search(q, k)                                              # unmasked bounded (sampled)
    env(CLM_SEARCH_BOUNDED=None)
    idx.search(q[:4], k)                                          # unmasked small-batch
    keep = torch.rand((n,), generator=g, device="cuda") < 0.75
    words = idx.allow_mask(keep=keep)
    for route in (C.CLM_MASK_PASS, C.CLM_MASK_GATHER, C.CLM_MASK_EXACT):
        idx.search(q, k, allow=words, route=route)                # masked pass / gather / exact
    plan = idx.key_plan(torch.randint(0, 1000, (n,), generator=g, device="cuda"))
    lo = torch.randint(0, 400, (nq,), generator=g, device="cuda")
    for route in (C.CLM_MASK_PASS, C.CLM_MASK_EXACT):
        idx.search_where(q, k, plan, lo, lo + 500, route=route)   # keyed pass / exact
    targets = torch.randint(0, n, (nq,), generator=g, device="cuda")
    idx.rank(q, targets, band_cap=C.CLM_RANK_BAND)                # rank band
    idx.logsumexp(q, 100.0, band_cap=C.CLM_LSE_FAST)              # lse fast
    idx.search_above(q, 0.3, band_cap=C.CLM_RANK_BAND)            # threshold band
    stats = {"search": idx.stats(), "mask": idx.mask_stats(), "where": idx.where_stats(), "rank": idx.rank_stats(),
             "lse": idx.lse_stats(), "range": idx.range_stats()}
    idx.close()

    n2, dim2 = 300_000, 96                                        # lists that overflow CAND_CAP
    rows2 = torch.randn((n2, dim2), generator=g, device="cuda")
    dups = torch.randn((2, dim2), generator=g, device="cuda")
    rows2[10_000:70_000] = dups[0] + 1e-3 * torch.randn((60_000, dim2), generator=g, device="cuda")
    rows2[200_000:205_000] = dups[1] + 1e-3 * torch.randn((5_000, dim2), generator=g, device="cuda")
    idx2 = CosineIndex(dim2, capacity=n2)
    idx2.append(rows2.half())
    q2 = torch.cat([dups.repeat(3, 1), torch.randn((5, dim2), generator=g, device="cuda")]).half()
    env(CLM_SEARCH_BOUNDED="1")
    idx2.search(q2, 8)
    env(CLM_SEARCH_BOUNDED=None)
    stats["overflow"] = idx2.stats()
    idx2.close()
    torch.cuda.synchronize()
    print(json.dumps(stats))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--table":
        table(sys.argv[2])
    else:
        main()
