#!/usr/bin/env python3
"""Timing and memory of the streaming contrastive-loss gradient (evaluate.contrastive_loss_grad,
CosineIndex.softmax_grad) against the only route there was before it: torch autograd through the full
fp32 [N, N] logits on the GPU.

  python tools/loss_grad_bench.py [--pairs 4096,32768] [--dim 512] [--temperature 0.07]
                                  [--chunk-rows 0,2048,4096,8192] [--query-block 0,8192] [--slices -1,0]
                                  [--warmup 2] [--repeats 7] [--step-timeout 600]
                                  [--out profiles/loss_grad_ab.txt]

The driver starts one child process per (pairs, slices) step, each under its own `timeout`, appends the
child's JSON lines to --out and stops at the first step that fails (a non-zero exit status, a time
limit included): nothing more is started on the GPU after a failure. The driver itself never opens the
GPU. slices: $CLM_GRAD_SLICES of the child (-1 = the library's rule, 0 = never split K); the library reads
it once per process.

Data: N Gaussian image rows, text = image + 2 x noise (pairs that retrieve each other), fp32 on the GPU.
Legs (device events around the whole call, host work included; every leg warmed up first; median and all
repeats reported; peak_mb = the largest drop of torch.cuda.mem_get_info's free bytes during one more
call, sampled from a second thread, after torch.cuda.empty_cache(); for grad/pass it is taken on the
leg's first call and counts what the index's grow-only workspaces had to grow by, so the first leg of a
step -- the defaults -- shows the whole workspace and later legs only what they need beyond it):
  grad/e2e     contrastive_loss_grad(a, b, T): two log-sum-exps, the pair scores, one softmax_grad pass,
               the O(N d) tail (slices = -1 only)
  grad/pass    softmax_grad(a, 1 / T, lse, row_lse) alone on a resident text index, per (chunk_rows,
               query_block); tflops = 3 * 2 * N^2 * dim / time (the weights' GEMM and the two accumulating
               ones); passes = the (block, chunk) passes of one call
  torch/full   normalise, logits = a^ b^T / T in fp32, the two cross entropies, backward() to a and b
               (slices = -1 only); the largest gradient difference to grad/e2e is reported
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import threading

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


def peak_mb(fn):
    """MiB of device memory one call of fn takes at its peak, beyond what was held before it"""
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    start = torch.cuda.mem_get_info()[0]
    low, stop = [start], threading.Event()

    def watch():
        while not stop.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info()[0])
            stop.wait(0.0005)
    t = threading.Thread(target=watch)
    t.start()
    try:
        out = fn()
        torch.cuda.synchronize()
        low[0] = min(low[0], torch.cuda.mem_get_info()[0])
    finally:
        stop.set()
        t.join()
    del out
    return round((start - low[0]) / 2 ** 20, 1)


def torch_full(a, b, T):
    import torch
    la, lb = a.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    ua, ub = la / la.norm(dim=1, keepdim=True), lb / lb.norm(dim=1, keepdim=True)
    logits = ua @ ub.T / T
    tgt = torch.arange(a.shape[0], device=a.device)
    loss = (torch.nn.functional.cross_entropy(logits, tgt) + torch.nn.functional.cross_entropy(logits.T, tgt)) / 2
    loss.backward()
    return loss.detach(), la.grad, lb.grad


def step(args):
    import torch

    from clip_lora_match_amd import evaluate as EV
    from clip_lora_match_amd.search import CosineIndex
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    n, dim, T = args.step_pairs, args.dim, args.temperature
    a = torch.randn(n, dim, generator=g, device=dev)
    b = a + 2.0 * torch.randn(n, dim, generator=g, device=dev)
    tag = {"pairs": n, "dim": dim, "T": T, "slices": args.step_slices}

    def line(leg, ms, all_ms, **more):
        print(json.dumps({**tag, "leg": leg, "ms": round(ms, 3), "all_ms": [round(v, 3) for v in all_ms], **more}),
              flush=True)

    ref = None
    if args.step_slices < 0:
        ms, all_ms, ref = timed(lambda: EV.contrastive_loss_grad(a, b, T), args.warmup, args.repeats)
        line("grad/e2e", ms, all_ms, peak_mb=peak_mb(lambda: EV.contrastive_loss_grad(a, b, T)), loss=ref["loss"],
             err=ref["err"], rho=round(ref["rho"], 5))
    txt, img = CosineIndex(dim, capacity=n, device=dev), CosineIndex(dim, capacity=n, device=dev)
    txt.append(b)
    img.append(a)
    lse, _ = txt.logsumexp(a, 1.0 / T)
    rlse, _ = img.logsumexp(b, 1.0 / T)
    img.close()
    for cr in [int(v) for v in args.chunk_rows.split(",")]:
        for qb in [int(v) for v in args.query_block.split(",")]:
            call = lambda: txt.softmax_grad(a, 1.0 / T, lse, row_lse=rlse, chunk_rows=cr, query_block=qb)  # noqa: E731
            peak = peak_mb(call)   # before the timed calls: the index's grow-only workspaces are part of it
            before = txt.grad_stats()["passes"]
            ms, all_ms, _ = timed(call, args.warmup, args.repeats)
            passes = (txt.grad_stats()["passes"] - before) // (args.warmup + args.repeats)
            line("grad/pass", ms, all_ms, chunk_rows=cr, query_block=qb, passes=passes,
                 tflops=round(3 * 2 * n * n * dim / (ms * 1e-3) / 1e12, 1), peak_mb=peak)
    txt.close()
    if args.step_slices < 0:
        ms, all_ms, out = timed(lambda: torch_full(a, b, T), args.warmup, args.repeats)
        diff = max(float((out[1] - ref["grad_image"]).abs().max()), float((out[2] - ref["grad_text"]).abs().max()))
        line("torch/full", ms, all_ms, peak_mb=peak_mb(lambda: torch_full(a, b, T)), loss=float(out[0]),
             max_grad_diff=diff, max_grad=float(out[1].abs().max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="4096,32768")
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--temperature", type=float, default=0.07)
    ap.add_argument("--chunk-rows", default="0,2048,4096,8192")
    ap.add_argument("--query-block", default="0,8192")
    ap.add_argument("--slices", default="-1,0")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds one (pairs, slices) step may take")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "loss_grad_ab.txt"))
    ap.add_argument("--step-pairs", type=int, default=0, help=argparse.SUPPRESS)      # set by the driver
    ap.add_argument("--step-slices", type=int, default=-1, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step_pairs:
        step(args)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/loss_grad_bench.py: one JSON line per leg; ms = median of all_ms (device events around the\n"
                "# whole call); peak_mb = device memory taken over one call (mem_get_info deltas); slices = the child's\n"
                "# $CLM_GRAD_SLICES (-1: the library's rule, 0: no split-K); tflops = 3 * 2 * N^2 * dim / ms\n")
    for pairs in [int(v) for v in args.pairs.split(",")]:
        for slices in [int(v) for v in args.slices.split(",")]:
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__),
                   "--step-pairs", str(pairs), "--step-slices", str(slices), "--dim", str(args.dim),
                   "--temperature", str(args.temperature), "--chunk-rows", args.chunk_rows,
                   "--query-block", args.query_block, "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
            env = dict(os.environ)
            env.pop("CLM_GRAD_SLICES", None)
            if slices >= 0:
                env["CLM_GRAD_SLICES"] = str(slices)
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
            with open(args.out, "a") as f:
                f.write(res.stdout)
            sys.stdout.write(res.stdout)
            if res.returncode != 0:   # a failure, a fault or a time limit: nothing more is started
                msg = f"# step pairs={pairs} slices={slices} ended with status {res.returncode}; stopped here\n"
                with open(args.out, "a") as f:
                    f.write(msg)
                sys.stderr.write(msg)
                return res.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
