#!/usr/bin/env python3
"""Timing of the retrieval evaluator (clip_lora_match_amd.evaluate) against the route that existed
before it: cosine_similarity() to the full [N, N] fp32 score matrix, then a torch comparison-and-
sum per direction for the ranks.

  python tools/rank_bench.py [--pairs 32768] [--large 100000] [--dim 512] [--warmup 1] [--repeats 3]

Legs (hipEvent timing on the current stream, every leg warmed up first, median of the repeats):
  A  evaluate_retrieval on `pairs` x `pairs` synthetic pair embeddings, both directions, vs the
     matrix route on the same embeddings; ranks compared for equality; peak memory of each
     (torch's allocator peak for the matrix route; the drop in free HBM with the index and its
     workspaces still allocated for the rank route, which allocates through libclm).
  B  `large` x `large`, one direction (the matrix route's 4 N^2 bytes do not fit there):
     B1 count_above with every target score 2.0 -- nothing is ahead and no band: the EPI_RANK
        pass alone (its skip test rejects every block), a call time, so a lower bound of the
        kernel's TF/s;
     B2 rank on pair embeddings (the target in the sparse tail of the scores, as on trained
        retrieval data), with the mean band length per query;
     B3 rank with random targets on Gaussian rows (the target in the bulk: the dense-band limit).
Algorithmic FLOPs of a pass: 2 * nq * N * dim. One JSON line per leg on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clip_lora_match_amd import evaluate as EV  # noqa: E402
from clip_lora_match_amd.search import CosineIndex  # noqa: E402
from clip_lora_match_amd.similarity import cosine_similarity  # noqa: E402


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


def pairs(n, dim, noise, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    a = torch.randn(n, dim, generator=g, device=dev)
    b = a + noise * torch.randn(n, dim, generator=g, device=dev)
    return a / a.norm(dim=-1, keepdim=True), b / b.norm(dim=-1, keepdim=True)


def matrix_ranks(S):
    """ranks of the diagonal, ties by column: 1 + #{j : S[i, j] > t or (S[i, j] == t and j < i)}"""
    n = S.shape[0]
    t = S.diagonal()[:, None]
    j = torch.arange(n, device=S.device)
    return 1 + ((S > t) | ((S == t) & (j[None, :] < j[:, None]))).sum(dim=1)


def matrix_route(a, b):
    S = cosine_similarity(a, b)
    return matrix_ranks(S), matrix_ranks(S.T)


def rank_route(a, b):
    return EV.retrieval_ranks(a, b, device=a.device), EV.retrieval_ranks(b, a, device=a.device)


def leg_a(n, dim, args, dev):
    a, b = pairs(n, dim, args.noise, 0, dev)
    torch.cuda.synchronize()
    ms_new, all_new, (i2t, t2i) = timed(lambda: rank_route(a, b), args.warmup, args.repeats)
    free0 = torch.cuda.mem_get_info(dev)[0]
    idx = CosineIndex(dim, capacity=n, device=dev)
    idx.append(b)
    idx.rank(a, torch.arange(n))
    torch.cuda.synchronize()
    new_bytes = free0 - torch.cuda.mem_get_info(dev)[0]
    st = idx.rank_stats()
    idx.close()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    ms_old, all_old, (o_i2t, o_t2i) = timed(lambda: matrix_route(a, b), args.warmup, args.repeats)
    old_bytes = torch.cuda.max_memory_allocated(dev) - base
    same = bool(torch.equal(i2t, o_i2t.cpu()) and torch.equal(t2i, o_t2i.cpu()))
    print(json.dumps({"leg": "A", "pairs": n, "dim": dim, "rank_route_ms": round(ms_new, 2),
                      "rank_route_all_ms": [round(x, 2) for x in all_new], "rank_route_bytes": int(new_bytes),
                      "matrix_route_ms": round(ms_old, 2), "matrix_route_all_ms": [round(x, 2) for x in all_old],
                      "matrix_route_bytes": int(old_bytes), "ranks_equal": same,
                      "recall@1": EV.recall_at_k(i2t, (1,))["recall@1"], "mrr": EV.mrr(i2t),
                      "band_rows_per_query": st["band_rows"] / max(st["band"], 1), "stats": st}), flush=True)


def leg_b(n, dim, args, dev):
    a, b = pairs(n, dim, args.noise, 1, dev)
    idx = CosineIndex(dim, capacity=n, device=dev)
    idx.append(b)
    flops = 2.0 * n * n * dim
    tgt = torch.arange(n, device=dev)
    two = torch.full((n,), 2.0, device=dev)
    ms, all_ms, above = timed(lambda: idx.count_above(a, two, tgt), args.warmup, args.repeats)
    assert int(above.abs().sum()) == 0
    print(json.dumps({"leg": "B1", "n": n, "dim": dim, "what": "count_above, t = 2.0: the EPI_RANK pass alone",
                      "ms": round(ms, 2), "all_ms": [round(x, 2) for x in all_ms],
                      "call_tflops": round(flops / ms * 1e-9, 1)}), flush=True)
    s0 = idx.rank_stats()
    ms, all_ms, (r, _) = timed(lambda: idx.rank(a, tgt), args.warmup, args.repeats)
    s1 = idx.rank_stats()
    calls = args.warmup + args.repeats
    print(json.dumps({"leg": "B2", "n": n, "dim": dim, "what": "rank, pair embeddings (target in the tail)",
                      "ms": round(ms, 2), "all_ms": [round(x, 2) for x in all_ms],
                      "call_tflops": round(flops / ms * 1e-9, 1), "recall@1": EV.recall_at_k(r, (1,))["recall@1"],
                      "band_rows_per_query": (s1["band_rows"] - s0["band_rows"]) / calls / n,
                      "exact_route_queries_per_call": (s1["exact"] - s0["exact"]) / calls}), flush=True)
    idx.close()
    g = torch.Generator(device=dev).manual_seed(2)
    rows = torch.randn(n, dim, generator=g, device=dev)
    q = torch.randn(n, dim, generator=g, device=dev)
    tg = torch.randint(0, n, (n,), generator=g, device=dev)
    idx = CosineIndex(dim, capacity=n, device=dev)
    idx.append(rows)
    s0 = idx.rank_stats()
    ms, all_ms, (r, _) = timed(lambda: idx.rank(q, tg), args.warmup, args.repeats)
    s1 = idx.rank_stats()
    print(json.dumps({"leg": "B3", "n": n, "dim": dim, "what": "rank, Gaussian rows, random targets (target in the bulk)",
                      "ms": round(ms, 2), "all_ms": [round(x, 2) for x in all_ms],
                      "call_tflops": round(flops / ms * 1e-9, 1), "median_rank": int(r.median()),
                      "band_rows_per_query": (s1["band_rows"] - s0["band_rows"]) / calls / n,
                      "exact_route_queries_per_call": (s1["exact"] - s0["exact"]) / calls}), flush=True)
    idx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32768)
    ap.add_argument("--large", type=int, default=100000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--noise", type=float, default=5.0, help="pair noise: b = a + noise * gaussian")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rank_bench needs a HIP device: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", torch.cuda.current_device())
    if args.pairs > 0:
        leg_a(args.pairs, args.dim, args, dev)
    if args.large > 0:
        leg_b(args.large, args.dim, args, dev)


if __name__ == "__main__":
    main()
