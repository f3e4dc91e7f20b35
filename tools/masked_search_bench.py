#!/usr/bin/env python3
"""Timing of the filtered search (CosineIndex.search(allow=)) on each route against the unmasked
search and the two things a caller could do before it.

  python tools/masked_search_bench.py [--rows 1000000] [--queries 4096] [--dim 512] [--k 5]
                                      [--select 1,0.5,0.125,0.01,0.001] [--warmup 1] [--repeats 3]
                                      [--skip-old] [--old-select 0.125,0.001] [--exact-max 2147483648]

Data: Gaussian fp16 rows and queries. Masks: for each selectivity a random one (Bernoulli) and a
contiguous one (the first rows), built once outside the timed region (allow_mask).

Legs (hipEvent timing on the current stream, every leg warmed up first, median of the repeats):
  masked/default, masked/exact, masked/pass, masked/gather   search(q, k, allow=mask, route=...)
  unmasked                                                    search(q, k)
  overfetch   search(q, k') with k' doubling from k until k allowed rows survive a host-side filter of
              the ids -- stops at k' = 1024 (reported as failed when k rows still did not survive)
  rebuild     read back the allowed rows, append them to a second index, search it
`served` is the mask_stats() delta of the leg's last call (which route answered). The masked legs'
ids are asserted equal to each other. One JSON line per leg on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clip_lora_match_amd import _capi as C  # noqa: E402
from clip_lora_match_amd.search import CosineIndex  # noqa: E402

ROUTES = {"default": 0, "exact": C.CLM_MASK_EXACT, "pass": C.CLM_MASK_PASS, "gather": C.CLM_MASK_GATHER}


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


def overfetch(idx, q, k, keep):
    """search with a growing k and a filter of the ids until k allowed rows survive for every query"""
    kk = k
    while True:
        s, i = idx.search(q, min(kk, len(idx)))
        ok = keep[i.clamp(min=0)] & (i >= 0)
        if bool((ok.sum(1) >= k).all()) or kk >= 1024 or kk >= len(idx):
            return bool((ok.sum(1) >= min(k, int(keep.sum()))).all()), kk
        kk = min(kk * 2, 1024)


def rebuild(idx, q, k, keep, dev):
    """read the allowed rows back, build a second index from them, search it, map the ids"""
    ids = torch.nonzero(keep).reshape(-1)
    sub = CosineIndex(idx.dim, capacity=max(ids.numel(), 1), device=dev)
    rows = idx.read(0, len(idx))          # the only read-back the public interface has: every row
    sub.append(rows[ids.cpu()])
    s, i = sub.search(q, k)
    sub.close()
    return s, torch.where(i >= 0, ids[i.clamp(min=0)], i)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--select", default="1,0.5,0.125,0.01,0.001")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-old", action="store_true", help="skip the overfetch / rebuild legs")
    ap.add_argument("--old-select", default=None,
                    help="selectivities at which the overfetch / rebuild legs run (default: all of --select); the "
                         "rebuild leg reads every row back to the host, 20 GB at 10 M x 512")
    ap.add_argument("--exact-max", type=int, default=1 << 31,
                    help="the forced exact route (fp64 cosines of every pair) is timed up to this many queries x rows")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    idx = CosineIndex(args.dim, capacity=args.rows, device=dev)
    for r0 in range(0, args.rows, 1 << 20):
        n = min(1 << 20, args.rows - r0)
        idx.append(torch.randn(n, args.dim, generator=g, device=dev).half())
    q = torch.randn(args.queries, args.dim, generator=g, device=dev).half()
    old_sel = None if args.old_select is None else [float(v) for v in args.old_select.split(",") if v]
    base = {"rows": args.rows, "queries": args.queries, "dim": args.dim, "k": args.k}
    ms, all_ms, _ = timed(lambda: idx.search(q, args.k), args.warmup, args.repeats)
    print(json.dumps({**base, "leg": "unmasked", "ms": round(ms, 3), "all_ms": [round(v, 3) for v in all_ms]}), flush=True)
    for sel in [float(v) for v in args.select.split(",")]:
        masks = {"random": torch.rand(args.rows, generator=g, device=dev) < sel,
                 "contiguous": torch.arange(args.rows, device=dev) < int(round(sel * args.rows))}
        for kind, keep in masks.items():
            words = idx.allow_mask(keep=keep)
            tag = {**base, "select": sel, "mask": kind, "allowed": int(keep.sum())}
            ref = None
            for name, flag in ROUTES.items():
                if name == "exact" and args.queries * args.rows > args.exact_max:
                    print(json.dumps({**tag, "leg": "masked/exact", "skipped": "queries x rows > --exact-max"}), flush=True)
                    continue
                before = idx.mask_stats()
                ms, all_ms, out = timed(lambda: idx.search(q, args.k, allow=words, route=flag), args.warmup, args.repeats)
                now = idx.mask_stats()
                calls = args.warmup + args.repeats
                served = {r: (now[r] - before[r]) // calls for r in now}
                if ref is None:
                    ref = out[1]
                assert torch.equal(out[1], ref), f"route {name} disagrees"
                print(json.dumps({**tag, "leg": "masked/" + name, "ms": round(ms, 3),
                                  "all_ms": [round(v, 3) for v in all_ms], "served": served}), flush=True)
            if args.skip_old or (old_sel is not None and sel not in old_sel):
                continue
            ms, all_ms, (ok, kk) = timed(lambda: overfetch(idx, q, args.k, keep), args.warmup, args.repeats)
            print(json.dumps({**tag, "leg": "overfetch", "ms": round(ms, 3), "all_ms": [round(v, 3) for v in all_ms],
                              "k_reached": kk, "complete": ok}), flush=True)
            ms, all_ms, out = timed(lambda: rebuild(idx, q, args.k, keep, dev), 0, 1)
            print(json.dumps({**tag, "leg": "rebuild", "ms": round(ms, 3), "all_ms": [round(v, 3) for v in all_ms],
                              "same_ids": bool(torch.equal(out[1], ref))}), flush=True)
    idx.close()


if __name__ == "__main__":
    main()
