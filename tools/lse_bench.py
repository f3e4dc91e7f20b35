#!/usr/bin/env python3
"""Timing of the streaming log-sum-exp (CosineIndex.logsumexp, evaluate.contrastive_loss) against
the route that existed before it: cosine_similarity() to the full [N, N] fp32 score matrix, then
torch.logsumexp in fp64 per direction.

  python tools/lse_bench.py [--pairs 32768] [--large 100000] [--dim 512] [--warmup 1] [--repeats 3]

Legs (hipEvent timing on the current stream, every leg warmed up first, median of the repeats):
  A  contrastive_loss on `pairs` x `pairs` synthetic pair embeddings, both directions (T = 0.07,
     head = 64), vs the matrix route on the same embeddings; the losses compared; peak memory of
     each (torch's allocator peak for the matrix route; the drop in free HBM with the index and its
     workspaces still allocated for the streaming route, which allocates through libclm); the
     largest certified bound and the largest |fast - exact route| over the queries of one direction.
  B  `large` x `large`, one direction (the matrix route's 4 N^2 bytes do not fit there):
     B1 count_above with every target score 2.0: the EPI_RANK pass alone (rank_bench's B1);
     B2 clm_index_lse with the floors given (no search inside the timing): the EPI_LSE pass, the
        band re-score and the finish -- the same tiles as B1 streamed once; B2b: the same with
        the top-1 score as the floor (a band of one or two rows: the pass almost alone);
     B3 logsumexp as called (search for the floors + B2), with the largest bound.
Algorithmic FLOPs of a pass: 2 * nq * N * dim. One JSON line per leg on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clip_lora_match_amd import _capi as C  # noqa: E402
from clip_lora_match_amd import evaluate as EV  # noqa: E402
from clip_lora_match_amd.search import CosineIndex  # noqa: E402
from clip_lora_match_amd.similarity import cosine_similarity  # noqa: E402

from rank_bench import pairs, timed  # noqa: E402


def matrix_route(a, b, T):
    """the loss from the full matrix; the fp64 logits in row blocks so the peak stays near the
    fp32 matrix itself"""
    S = cosine_similarity(a, b)
    n = S.shape[0]
    t = S.diagonal().double() / T
    li = torch.cat([torch.logsumexp(S[i:i + 4096].double() / T, dim=1) for i in range(0, n, 4096)])
    lt = torch.cat([torch.logsumexp(S[:, i:i + 4096].double() / T, dim=0) for i in range(0, n, 4096)])
    return float(((li - t).mean() + (lt - t).mean()) / 2)


def lse_given_floors(idx, q, scale, floor, flags=0):
    nq = q.shape[0]
    lse = torch.empty((nq,), dtype=torch.float64, device=q.device)
    err = torch.empty((nq,), dtype=torch.float32, device=q.device)
    C.check(C.lib().clm_index_lse(idx._h, C.ptr(q), C.CLM_F32, nq, float(scale), C.ptr(floor), C.ptr(lse), C.ptr(err),
                                  int(flags), C.stream_of(q.device)), "clm_index_lse")
    return lse, err


def leg_a(n, dim, args, dev):
    T = 0.07
    a, b = pairs(n, dim, args.noise, 0, dev)
    torch.cuda.synchronize()
    ms_new, all_new, out = timed(lambda: EV.contrastive_loss(a, b, T, device=dev), args.warmup, args.repeats)
    free0 = torch.cuda.mem_get_info(dev)[0]
    idx = CosineIndex(dim, capacity=n, device=dev)
    idx.append(b)
    lse, err = idx.logsumexp(a, 1.0 / T)
    idx.rank(a, torch.arange(n))
    torch.cuda.synchronize()
    new_bytes = free0 - torch.cuda.mem_get_info(dev)[0]
    st = idx.lse_stats()
    ms_ex, _, (ex, _) = timed(lambda: idx.logsumexp(a, 1.0 / T, head=0), 0, 1)
    idx.close()
    diff = (lse - ex).abs()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    ms_old, all_old, old = timed(lambda: matrix_route(a, b, T), args.warmup, args.repeats)
    old_bytes = torch.cuda.max_memory_allocated(dev) - base
    print(json.dumps({"leg": "A", "pairs": n, "dim": dim, "T": T, "loss_route_ms": round(ms_new, 2),
                      "loss_route_all_ms": [round(x, 2) for x in all_new], "loss_route_bytes": int(new_bytes),
                      "matrix_route_ms": round(ms_old, 2), "matrix_route_all_ms": [round(x, 2) for x in all_old],
                      "matrix_route_bytes": int(old_bytes), "loss": out["loss"], "loss_err": out["err"],
                      "matrix_loss": old, "loss_diff": abs(out["loss"] - old),
                      "exact_route_one_direction_ms": round(ms_ex, 2),
                      "max_err": float(err.max()), "max_fast_minus_exact": float(diff.max()),
                      "bound_holds": bool((diff <= err.double() + 1e-10).all()), "stats": st}), flush=True)


def leg_b(n, dim, args, dev):
    scale = 1.0 / 0.07
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
    ms_s, all_s, (s, _) = timed(lambda: idx.search(a, 64), args.warmup, args.repeats)
    floor = s[:, -1].contiguous()
    s0 = idx.lse_stats()
    ms, all_ms, (lse, err) = timed(lambda: lse_given_floors(idx, a, scale, floor), args.warmup, args.repeats)
    s1 = idx.lse_stats()
    calls = args.warmup + args.repeats
    print(json.dumps({"leg": "B2", "n": n, "dim": dim, "what": "clm_index_lse, floors given: EPI_LSE pass + band + finish",
                      "ms": round(ms, 2), "all_ms": [round(x, 2) for x in all_ms],
                      "call_tflops": round(flops / ms * 1e-9, 1), "search64_ms": round(ms_s, 2),
                      "fast_queries_per_call": (s1["fast"] - s0["fast"]) / calls,
                      "exact_route_queries_per_call": (s1["exact"] - s0["exact"]) / calls,
                      "max_err": float(err.max()), "median_err": float(err.median())}), flush=True)
    top1 = s[:, 0].contiguous()
    ms1, all_1, (_, err1) = timed(lambda: lse_given_floors(idx, a, scale, top1), args.warmup, args.repeats)
    print(json.dumps({"leg": "B2b", "n": n, "dim": dim, "what": "the same with the top-1 score as the floor: a band of "
                      "one or two rows, so the EPI_LSE pass with almost no re-score",
                      "ms": round(ms1, 2), "all_ms": [round(x, 2) for x in all_1],
                      "call_tflops": round(flops / ms1 * 1e-9, 1), "max_err": float(err1.max())}), flush=True)
    ms, all_ms, (lse2, err2) = timed(lambda: idx.logsumexp(a, scale), args.warmup, args.repeats)
    print(json.dumps({"leg": "B3", "n": n, "dim": dim, "what": "logsumexp as called (search 64 + B2)",
                      "ms": round(ms, 2), "all_ms": [round(x, 2) for x in all_ms],
                      "same_bits_as_B2": bool(torch.equal(lse, lse2)), "max_err": float(err2.max())}), flush=True)
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
        raise SystemExit("lse_bench needs a HIP device: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", torch.cuda.current_device())
    if args.pairs > 0:
        leg_a(args.pairs, args.dim, args, dev)
    if args.large > 0:
        leg_b(args.large, args.dim, args, dev)


if __name__ == "__main__":
    main()
