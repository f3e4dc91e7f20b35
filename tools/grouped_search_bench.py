#!/usr/bin/env python3
"""Timing of the grouped search (CosineIndex.search_grouped) against what a caller could do without it.

  python tools/grouped_search_bench.py [--rows 1000000,10000000] [--queries 4096,1] [--dim 512] [--k 5]
                                       [--layouts g1,g2,g8,giant] [--warmup 1] [--repeats 5]
                                       [--step-timeout 300] [--out profiles/grouped_search_ab.txt]

The driver starts one child process per (rows, layout) step, each under its own `timeout`, appends the
child's JSON lines to --out and stops at the first step that fails (a non-zero exit status, a time
limit included): nothing more is started on the GPU after a failure. The driver itself never opens
the GPU.

Data: Gaussian fp16 rows and queries. Layouts: g1 / g2 / g8 = groups of 1, 2 and 8 consecutive rows,
giant = a random half of the rows in one group and every other row a group of its own.

Legs of a step, for each query count (device events on the current stream around the whole call, host
work included; every leg warmed up first; median and all repeats reported):
  grouped/default    search_grouped(q, k, plan)                       -- list route, threshold route for the rest
  torch-dedup        search(q, L) as the list route runs it, then a torch-only first-occurrence
                     de-duplication (stable sort of the gids, run heads, scatter back, prefix sum, scatter)
                     -- complete only where the list route is (the leg says so)
  search             search(q, k), the floor: no grouping at all
  grouped/threshold  search_grouped(..., route=GROUP_ROUTE_THRESHOLD)
The grouped legs' results are asserted equal to each other, and to torch-dedup where that is complete.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(fn, warmup, repeats):
    """(median ms, all ms, last result) by device events"""
    import torch
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


def torch_dedup(idx, q, k, L, gids):
    """search(q, L) + the first k first-occurrences of a gid per row, torch ops only"""
    import torch
    s, i = idx.search(q, L)
    g = torch.where(i >= 0, gids[i.clamp(min=0)], torch.full_like(i, -1))
    gs, order = torch.sort(g, dim=1, stable=True)
    head = torch.ones_like(gs, dtype=torch.bool)
    head[:, 1:] = gs[:, 1:] != gs[:, :-1]
    keep = torch.zeros_like(head).scatter_(1, order, head) & (i >= 0)
    rank = torch.cumsum(keep, dim=1) - 1
    slot = torch.where(keep & (rank < k), rank, torch.full_like(rank, k))   # column k: the bin
    nq = s.shape[0]
    os_ = torch.full((nq, k + 1), float("-inf"), dtype=torch.float32, device=s.device).scatter_(1, slot, s)
    oi = torch.full((nq, k + 1), -1, dtype=torch.int64, device=s.device).scatter_(1, slot, i)
    og = torch.full((nq, k + 1), -1, dtype=torch.int64, device=s.device).scatter_(1, slot, g)
    found = keep.sum(1).clamp(max=k)
    return os_[:, :k], oi[:, :k], og[:, :k], found


def step(args):
    """one (rows, layout): every leg at every query count, one JSON line each"""
    import torch

    from clip_lora_match_amd.search import GROUP_ROUTE_THRESHOLD, CosineIndex, group_row_bound
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    rows, k, layout = args.step_rows, args.k, args.step_layout
    idx = CosineIndex(args.dim, capacity=rows, device=dev)
    for r0 in range(0, rows, 1 << 20):
        n = min(1 << 20, rows - r0)
        idx.append(torch.randn(n, args.dim, generator=g, device=dev).half())
    if layout == "giant":
        gids = torch.arange(rows, device=dev) + 1
        gids[torch.rand(rows, generator=g, device=dev) < 0.5] = 0
    else:
        gids = torch.arange(rows, device=dev) // int(layout[1:])
    plan = idx.group_plan(gids)
    L = min(group_row_bound(k, plan.m), 1024, plan.n_allowed)
    for nq in [int(v) for v in args.queries.split(",")]:
        q = torch.randn(nq, args.dim, generator=g, device=dev).half()
        tag = {"rows": rows, "dim": args.dim, "queries": nq, "k": k, "layout": layout, "m": plan.m,
               "groups": plan.n_groups, "L": L}

        def line(leg, ms, all_ms, **more):
            print(json.dumps({**tag, "leg": leg, "ms": round(ms, 3), "all_ms": [round(v, 3) for v in all_ms], **more}),
                  flush=True)

        before = idx.group_stats()
        ms, all_ms, ref = timed(lambda: idx.search_grouped(q, k, plan), args.warmup, args.repeats)
        now = idx.group_stats()
        calls = args.warmup + args.repeats
        line("grouped/default", ms, all_ms, served={r: (now[r] - before[r]) // calls for r in now})
        ms, all_ms, out = timed(lambda: torch_dedup(idx, q, k, L, plan.gids), args.warmup, args.repeats)
        complete = bool((out[3] == k).all()) or L == plan.n_allowed or L == group_row_bound(k, plan.m)
        if complete:
            assert all(torch.equal(a, b) for a, b in zip(out[1:3], ref[1:3])), "torch-dedup disagrees"
        line("torch-dedup", ms, all_ms, complete=complete)
        ms, all_ms, _ = timed(lambda: idx.search(q, k), args.warmup, args.repeats)
        line("search", ms, all_ms)
        ms, all_ms, out = timed(lambda: idx.search_grouped(q, k, plan, route=GROUP_ROUTE_THRESHOLD), args.warmup,
                                args.repeats)
        assert all(torch.equal(a, b) for a, b in zip(out[1:], ref[1:])), "the threshold route disagrees"
        assert torch.equal(out[0].view(torch.int32), ref[0].view(torch.int32)), "the threshold route's scores differ"
        line("grouped/threshold", ms, all_ms)
    idx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000")
    ap.add_argument("--queries", default="4096,1")
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--layouts", default="g1,g2,g8,giant")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds one (rows, layout) step may take")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "grouped_search_ab.txt"))
    ap.add_argument("--step-rows", type=int, default=0, help=argparse.SUPPRESS)      # set by the driver
    ap.add_argument("--step-layout", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step_rows:
        step(args)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/grouped_search_bench.py: one JSON line per leg; ms = median of all_ms (device events)\n")
    for rows in [int(v) for v in args.rows.split(",")]:
        for layout in [v for v in args.layouts.split(",") if v]:
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__),
                   "--step-rows", str(rows), "--step-layout", layout, "--queries", args.queries, "--dim", str(args.dim),
                   "--k", str(args.k), "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            with open(args.out, "a") as f:
                f.write(res.stdout)
            sys.stdout.write(res.stdout)
            if res.returncode != 0:   # a failure, a fault or a time limit: nothing more is started
                msg = f"# step rows={rows} layout={layout} ended with status {res.returncode}; stopped here\n"
                with open(args.out, "a") as f:
                    f.write(msg)
                sys.stderr.write(msg)
                return res.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
