#!/usr/bin/env python3
"""Timing of the threshold search (CosineIndex.search_above) against the two routes that existed
before it.

  python tools/range_bench.py [--rows 1000000] [--queries 4096] [--dim 512] [--tau 0.7]
                              [--warmup 1] [--repeats 3] [--matrix-mb 8192] [--only-new]

Data: `rows / copies` base vectors a (Gaussian, 512 dims); the index holds `copies` rows
b = a + noise * gaussian per base vector, the queries are the first `queries` base vectors. With
noise 0.8 a query's own copies score 1 / sqrt(1.64) = 0.78 and everything else ~0 +- 0.044, so at
tau = 0.7 a result is a handful of rows (the copies that stayed above the threshold).

Legs (hipEvent timing on the current stream, every leg warmed up first, median of the repeats):
  new     search_above(q, tau): offsets, scores, ids.
  route1  count_above(q, tau, INT64_MAX) for the lengths, then search(q, k = the longest list) and a
          mask -- impossible when a list is longer than 1024 (reported as such, not timed).
  route2  cosine_similarity() to the full [nq, N] matrix, then compare / nonzero / sort in torch,
          with nq cut until the matrix fits --matrix-mb and 2^31 elements (the time is reported
          for the cut batch and scaled to the full one).
The legs' results are asserted equal where they can be compared (route2 on its cut batch).
One JSON line per leg on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clip_lora_match_amd.search import CosineIndex  # noqa: E402
from clip_lora_match_amd.similarity import cosine_similarity  # noqa: E402

I64_MAX = 2 ** 63 - 1


def timed(fn, warmup, repeats):
    """(median ms, all ms, last result) by device events"""
    out = None
    for _ in range(warmup):
        out = fn()
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2], ms, out


def build(args, dev):
    """(index, queries): the rows are generated and appended in chunks of 2^20"""
    g = torch.Generator(device=dev).manual_seed(0)
    bases = max(args.rows // args.copies, args.queries)
    a = torch.randn(bases, args.dim, generator=g, device=dev)
    idx = CosineIndex(args.dim, capacity=args.rows, device=dev)
    for r0 in range(0, args.rows, 1 << 20):
        n = min(1 << 20, args.rows - r0)
        j = torch.arange(r0, r0 + n, device=dev) % bases
        idx.append(a[j] + args.noise * torch.randn(n, args.dim, generator=g, device=dev))
    return idx, a[: args.queries].contiguous()


def route1(idx, q, tau):
    nq = q.shape[0]
    lens = idx.count_above(q, torch.full((nq,), tau), torch.full((nq,), I64_MAX, dtype=torch.int64))
    k = int(lens.max())
    if k > 1024:
        return None
    off = torch.zeros((nq + 1,), dtype=torch.int64, device=q.device)
    off[1:] = torch.cumsum(lens, 0)
    if k == 0:
        return off, torch.empty((0,), device=q.device), torch.empty((0,), dtype=torch.int64, device=q.device)
    s, i = idx.search(q, k)
    keep = torch.arange(k, device=q.device)[None, :] < lens[:, None]
    return off, s[keep], i[keep]


def route2(q, rows, tau):
    S = cosine_similarity(q, rows)
    keep = (S >= tau) | torch.isnan(S)
    qi, ji = keep.nonzero(as_tuple=True)
    s = S[qi, ji]
    # (query asc, score desc, id asc): stable sorts from the last key to the first
    o = torch.argsort(s, descending=True, stable=True)
    qi, ji, s = qi[o], ji[o], s[o]
    o = torch.argsort(qi, stable=True)
    off = torch.zeros((q.shape[0] + 1,), dtype=torch.int64, device=q.device)
    off[1:] = torch.cumsum(torch.bincount(qi, minlength=q.shape[0]), 0)
    return off, s[o], ji[o]


def same(a, b):
    return bool(torch.equal(a[0].cpu(), b[0].cpu()) and torch.equal(a[1].cpu(), b[1].cpu())
                and torch.equal(a[2].cpu(), b[2].cpu()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--noise", type=float, default=0.8)
    ap.add_argument("--tau", type=float, default=0.7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--matrix-mb", type=int, default=8192)
    ap.add_argument("--only-new", action="store_true", help="the search_above leg alone (kernel traces)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("range_bench needs a HIP device: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", torch.cuda.current_device())
    idx, q = build(args, dev)
    nq, N = q.shape[0], len(idx)
    head = {"rows": N, "queries": nq, "dim": args.dim, "tau": args.tau}
    s0 = idx.range_stats()
    ms, all_ms, new = timed(lambda: idx.search_above(q, args.tau), args.warmup, args.repeats)
    s1 = idx.range_stats()
    calls = args.warmup + args.repeats
    lens = new[0][1:] - new[0][:-1]
    print(json.dumps({**head, "leg": "new", "what": "search_above", "ms": round(ms, 2),
                      "all_ms": [round(x, 2) for x in all_ms], "entries": int(new[0][-1]),
                      "mean_len": round(float(lens.float().mean()), 3), "max_len": int(lens.max()),
                      "empty": int((lens == 0).sum()),
                      "per_call": {k: (s1[k] - s0[k]) / calls for k in s1}}), flush=True)
    if args.only_new:
        idx.close()
        return
    r1 = route1(idx, q, args.tau)
    if r1 is None:
        print(json.dumps({**head, "leg": "route1", "what": "count_above + search(k = longest) + mask",
                          "impossible": "a list is longer than 1024"}), flush=True)
    else:
        ms1, all1, r1 = timed(lambda: route1(idx, q, args.tau), args.warmup, args.repeats)
        print(json.dumps({**head, "leg": "route1", "what": "count_above + search(k = longest) + mask",
                          "ms": round(ms1, 2), "all_ms": [round(x, 2) for x in all1], "k": int(lens.max()),
                          "equal_to_new": same(r1, new), "new_speedup": round(ms1 / ms, 2)}), flush=True)
        assert same(r1, new), "route 1 and search_above disagree"
    # route 2 needs the rows as a tensor: read back from the index in chunks
    rows = torch.empty((N, args.dim), dtype=torch.float32, device=dev)
    for r0 in range(0, N, 1 << 18):
        n = min(1 << 18, N - r0)
        rows[r0: r0 + n] = idx.read(r0, n).to(dev)
    # ... and below 2^31 elements: torch's nonzero does not take a larger mask
    nqc = max(1, min(nq, (args.matrix_mb << 20) // (N * 4), (2 ** 31 - 1) // N))
    ms2, all2, r2 = timed(lambda: route2(q[:nqc], rows, args.tau), args.warmup, args.repeats)
    cut = (new[0][: nqc + 1], new[1][: int(new[0][nqc])], new[2][: int(new[0][nqc])])
    print(json.dumps({**head, "leg": "route2", "what": "cosine_similarity matrix + compare / nonzero / sort",
                      "queries_in_matrix": nqc, "ms": round(ms2, 2), "all_ms": [round(x, 2) for x in all2],
                      "ms_scaled_to_all_queries": round(ms2 * nq / nqc, 2), "equal_to_new": same(r2, cut),
                      "new_speedup": round(ms2 * nq / nqc / ms, 2)}), flush=True)
    assert same(r2, cut), "route 2 and search_above disagree"
    idx.close()


if __name__ == "__main__":
    main()
