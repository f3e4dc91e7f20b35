#!/usr/bin/env python3
"""Timing of the keyed search (CosineIndex.search_where: one value range per query in one batched pass)
against what a caller could do without it.

  python tools/where_search_bench.py [--rows 1000000,10000000] [--queries 4096,1] [--dim 512] [--k 5]
                                     [--layouts random,rownum] [--fractions 1,0.5,0.125,0.01,0.001]
                                     [--loop-queries 64] [--exact-queries 16] [--warmup 1] [--repeats 5]
                                     [--step-timeout 600] [--out profiles/where_search_ab.txt]

The driver starts one child process per (rows, layout) step, each under its own `timeout`, appends the
child's JSON lines to --out and stops at the first step that fails (a non-zero exit status, a time
limit included): nothing more is started on the GPU after a failure. The driver itself never opens
the GPU.

Data: Gaussian fp16 rows and queries. Layouts: random = the rows' values are a random permutation of
0 .. N - 1 (a range's rows are scattered over the index), rownum = value = row number (a range is one
contiguous run of rows). Query i of a batch gets its own range [s_i, s_i + f N) with a random start, for
each fraction f of the rows.

Legs (device events on the current stream around the whole call, host work included; every leg warmed up
first; median and all repeats reported; the key plan and the loop's masks are built outside the timing):
  where/default   search_where(q, k, plan, lo, hi)
  where/pass      ... route=CLM_MASK_PASS
  where/exact     ... route=CLM_MASK_EXACT, on the first --exact-queries queries only, one repeat (the
                  exact route computes every cosine in fp64: seconds per call at these sizes); the line
                  carries ms_per_query
  loop            one search(q_i, k, allow=mask_i) call per query, today's only way: timed on the first
                  --loop-queries queries, reported per query (ms_per_query; ms = the whole loop)
  masked-ones     search(q, k, allow=all ones, route=CLM_MASK_PASS): the floor, one shared mask (once per
                  query count, under fraction 1)
  search          search(q, k): no filter at all (likewise)
where/pass and the loop are asserted equal to where/default on the queries they share.
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


def step(args):
    """one (rows, layout): every leg at every fraction and query count, one JSON line each"""
    import torch

    from clip_lora_match_amd import _capi as C
    from clip_lora_match_amd.search import CosineIndex, pack_mask
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    rows, k, layout = args.step_rows, args.k, args.step_layout
    idx = CosineIndex(args.dim, capacity=rows, device=dev)
    for r0 in range(0, rows, 1 << 20):
        n = min(1 << 20, rows - r0)
        idx.append(torch.randn(n, args.dim, generator=g, device=dev).half())
    values = torch.randperm(rows, generator=g, device=dev) if layout == "random" else torch.arange(rows, device=dev)
    plan = idx.key_plan(values)
    ones = idx.allow_mask(keep=torch.ones(rows, dtype=torch.bool, device=dev))
    same = lambda a, b: torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))  # noqa
    for nq in [int(v) for v in args.queries.split(",")]:
        q = torch.randn(nq, args.dim, generator=g, device=dev).half()
        for frac in [float(v) for v in args.fractions.split(",")]:
            width = max(int(frac * rows), 1)
            lo = (torch.rand(nq, generator=g, device=dev) * (rows - width + 1)).long().clamp(0, rows - width)
            hi = lo + width - 1
            tag = {"rows": rows, "dim": args.dim, "queries": nq, "k": k, "layout": layout, "fraction": frac,
                   "in_range": width}

            def line(leg, ms, all_ms, **more):
                print(json.dumps({**tag, "leg": leg, "ms": round(ms, 3), "all_ms": [round(v, 3) for v in all_ms],
                                  **more}), flush=True)

            calls = args.warmup + args.repeats
            before = idx.where_stats()
            ms, all_ms, ref = timed(lambda: idx.search_where(q, k, plan, lo, hi), args.warmup, args.repeats)
            now = idx.where_stats()
            line("where/default", ms, all_ms, served={r: (now[r] - before[r]) // calls for r in now})
            before = idx.where_stats()
            ms, all_ms, out = timed(lambda: idx.search_where(q, k, plan, lo, hi, route=C.CLM_MASK_PASS), args.warmup,
                                    args.repeats)
            now = idx.where_stats()
            assert same(out, ref), "the pass route disagrees"
            line("where/pass", ms, all_ms, served={r: (now[r] - before[r]) // calls for r in now})
            ne = min(nq, args.exact_queries)
            if ne:
                ms, all_ms, out = timed(lambda: idx.search_where(q[:ne], k, plan, lo[:ne], hi[:ne], route=C.CLM_MASK_EXACT),
                                        0, 1)
                assert same(out, (ref[0][:ne], ref[1][:ne])), "the exact route disagrees"
                line("where/exact", ms, all_ms, timed_queries=ne, ms_per_query=round(ms / ne, 4))
            nl = min(nq, args.loop_queries)
            masks = [pack_mask((values >= lo[i]) & (values <= hi[i])) for i in range(nl)]

            def loop():
                return [idx.search(q[i], k, allow=masks[i]) for i in range(nl)]
            ms, all_ms, outs = timed(loop, args.warmup, args.repeats)
            assert all(torch.equal(o[1][0], ref[1][i]) and
                       torch.equal(o[0][0].view(torch.int32), ref[0][i].view(torch.int32)) for i, o in enumerate(outs)), \
                "the per-query masked loop disagrees"
            line("loop", ms, all_ms, timed_queries=nl, ms_per_query=round(ms / nl, 4))
            del masks
            if frac == 1.0:
                ms, all_ms, out = timed(lambda: idx.search(q, k, allow=ones, route=C.CLM_MASK_PASS), args.warmup,
                                        args.repeats)
                assert same(out, ref), "the all-ones masked search disagrees"
                line("masked-ones", ms, all_ms)
                ms, all_ms, _ = timed(lambda: idx.search(q, k), args.warmup, args.repeats)
                line("search", ms, all_ms)
    idx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000")
    ap.add_argument("--queries", default="4096,1")
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--layouts", default="random,rownum")
    ap.add_argument("--fractions", default="1,0.5,0.125,0.01,0.001")
    ap.add_argument("--loop-queries", type=int, default=64)
    ap.add_argument("--exact-queries", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds one (rows, layout) step may take")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "where_search_ab.txt"))
    ap.add_argument("--step-rows", type=int, default=0, help=argparse.SUPPRESS)      # set by the driver
    ap.add_argument("--step-layout", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step_rows:
        step(args)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/where_search_bench.py: one JSON line per leg; ms = median of all_ms (device events).\n"
                f"# loop: one search(q_i, k, allow=mask_i) per query, timed on {args.loop_queries} queries and reported\n"
                f"# per query (ms_per_query); where/exact: timed once on {args.exact_queries} queries, likewise\n")
    for rows in [int(v) for v in args.rows.split(",")]:
        for layout in [v for v in args.layouts.split(",") if v]:
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__),
                   "--step-rows", str(rows), "--step-layout", layout, "--queries", args.queries, "--dim", str(args.dim),
                   "--k", str(args.k), "--fractions", args.fractions, "--loop-queries", str(args.loop_queries),
                   "--exact-queries", str(args.exact_queries), "--warmup", str(args.warmup),
                   "--repeats", str(args.repeats)]
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
