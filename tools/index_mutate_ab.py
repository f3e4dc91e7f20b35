#!/usr/bin/env python3
"""Timing of the in-place index mutation (CosineIndex.remove / .update) against the two yardsticks
it has, in one process:

  rebuild  the only route there was before: `read` every row back to the host, `reset`, `append`
           the surviving (or corrected) rows;
  copy     a plain device-to-device copy of as many bytes as the mutation has to move (the rows from
           the first removed one to the end, or the updated rows: fp16 row + fp32 row + inverse
           norm each) -- the roof of an HBM-bound mover. Removal goes through a staging buffer, so
           about 2x the copy is expected.

  python tools/index_mutate_ab.py [--rows 1000000] [--dim 512] [--repeats 3] [--rebuild-repeats 2]
                                  [--out profiles/index_mutate_ab.txt]

Legs on an index of `rows` x `dim` fp32 rows (so it keeps the fp32 copy):
  a  remove a random 1 % of the rows;
  b  remove row 0: every other row moves;
  c  update a random 1 % of the rows.
Every timing is a host clock around a call that ends in a device synchronise (remove, update, read
and append all do; the copy is followed by one), after a warm-up of the same call; the index is
restored outside the timed window; the legs of one repeat run back to back, the median is
reported. After each leg the mutated index and the rebuilt one answer 64 queries with the same
bits. One JSON line per leg, on stdout and in --out.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clip_lora_match_amd.search import CosineIndex  # noqa: E402


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def fill(ix, rows):
    ix.reset()
    ix.append(rows)


def rebuild_remove(ix, keep_host):
    host = ix.read()
    ix.reset()
    ix.append(host[keep_host])


def rebuild_update(ix, ids_host, new_host):
    host = ix.read()
    ix.reset()
    host = host.contiguous()
    host[ids_host] = new_host
    ix.append(host)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rebuild-repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "index_mutate_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("index_mutate_ab needs a HIP device: nothing is timed without one")
    n, dim = a.rows, a.dim
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev).manual_seed(1)
    rows = torch.randn((n, dim), generator=g, device=dev)
    rows /= rows.norm(dim=1, keepdim=True)
    sel = rows[:: max(1, n // 64)][:64]
    qs = sel + 0.05 * torch.randn(sel.shape, generator=g, device=dev)   # queries near rows spread over the index
    row_bytes = dim * 6 + 4
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(2))
    some = perm[: max(1, n // 100)].sort().values
    new = torch.randn((some.numel(), dim), generator=g, device=dev)
    legs = {
        "a": ("remove a random 1 %", some, None),
        "b": ("remove row 0", torch.tensor([0]), None),
        "c": ("update a random 1 %", some, new),
    }
    ix = CosineIndex(dim, capacity=n)
    other = CosineIndex(dim, capacity=n)
    lines = []
    for leg, (what, ids, new_rows) in legs.items():
        keep = torch.ones(n, dtype=torch.bool)
        if new_rows is None:
            keep[ids] = False
            moved_rows = n - int(ids[0]) - ids.numel()
            mutate = lambda: ix.remove(ids)                                           # noqa: E731
            rebuild = lambda: rebuild_remove(other, keep)                              # noqa: E731
        else:
            moved_rows = ids.numel()
            new_host = new_rows.cpu()
            mutate = lambda: ix.update(ids, new_rows)                                  # noqa: E731
            rebuild = lambda: rebuild_update(other, ids, new_host)                     # noqa: E731
        moved = moved_rows * row_bytes
        src = torch.empty(moved, dtype=torch.uint8, device=dev)
        dst = torch.empty(moved, dtype=torch.uint8, device=dev)
        copy = lambda: dst.copy_(src)                                                  # noqa: E731
        fill(ix, rows)
        mutate()    # warm-up: code objects, the staging buffer
        copy()
        t_mut, t_reb, t_copy = [], [], []
        for r in range(a.repeats):
            fill(ix, rows)
            t_mut.append(clock(mutate))
            if r < a.rebuild_repeats:
                fill(other, rows)
                t_reb.append(clock(rebuild))
            t_copy.append(clock(copy))
        s1, i1 = ix.search(qs, 10)
        s2, i2 = other.search(qs, 10)
        same = bool(len(ix) == len(other) and torch.equal(i1, i2) and torch.equal(s1, s2))
        del src, dst
        m, rb, cp = statistics.median(t_mut), statistics.median(t_reb), statistics.median(t_copy)
        line = {"leg": leg, "what": what, "rows": n, "dim": dim, "ids": int(ids.numel()), "moved_rows": moved_rows,
                "moved_bytes": moved, "in_place_ms": round(m, 3), "in_place_all_ms": [round(v, 3) for v in t_mut],
                "rebuild_ms": round(rb, 1), "rebuild_all_ms": [round(v, 1) for v in t_reb],
                "copy_ms": round(cp, 3), "copy_all_ms": [round(v, 3) for v in t_copy],
                "copy_gb_s": round(2 * moved / cp / 1e6, 1), "in_place_over_copy": round(m / cp, 2),
                "rebuild_over_in_place": round(rb / m, 1), "beats_rebuild": bool(m < rb),
                "same_search_bits_as_rebuild": same}
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    ix.close()
    other.close()
    if not all(json.loads(ln)["beats_rebuild"] and json.loads(ln)["same_search_bits_as_rebuild"] for ln in lines):
        raise SystemExit("a leg did not beat the rebuild route, or its results differ from it")


if __name__ == "__main__":
    main()
