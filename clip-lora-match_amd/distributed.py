"""Batch data parallelism for the encode / index-build / search path over the
GPUs of one node: one process per GPU, torch.distributed with the "nccl"
backend (RCCL on ROCm) over xGMI.

The reference has no parallelism at all; this adds exactly the
exchange steps the path has:

* index build (scripts/rebuild_index.py:64-96 generalised to N GPUs): rank r
  encodes rows [shard_range(n, r, world)) and one all_gather of the fp32 (or
  fp16) embeddings gives every rank the whole index in global order;
* sharded search: each rank keeps rows [start, stop) of the HBM index with
  global offset `start`, searches its shard locally (GEMM + exact top-k), one
  all_gather of the [nq, k] (score, index) lists, then the same
  (score desc, index asc) merge -- top-k of a union equals top-k of the
  per-shard top-ks, so the result is identical to the single-GPU order.

The collective plumbing takes injectable local-search / merge functions so it
is testable with the gloo backend on CPU (tests/test_distributed_cpu.py); the
product defaults are the GPU index and the clm_topk_merge kernel.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import torch
import torch.distributed as dist


def shard_range(n: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous balanced shard [start, stop) of n rows for `rank` of `world`."""
    if world <= 0 or not (0 <= rank < world) or n < 0:
        raise ValueError("bad shard arguments")
    base, rem = divmod(n, world)
    start = rank * base + min(rank, rem)
    return start, start + base + (1 if rank < rem else 0)


def all_gather_rows(local: torch.Tensor, n_total: int, group=None) -> torch.Tensor:
    """Concatenate every rank's shard (shard_range layout, uneven sizes allowed) on every rank."""
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    start, stop = shard_range(n_total, rank, world)
    if local.shape[0] != stop - start:
        raise ValueError(f"rank {rank} holds {local.shape[0]} rows, shard is {stop - start}")
    width = (n_total + world - 1) // world
    buf = torch.zeros((width,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    buf[: local.shape[0]] = local
    out = torch.empty((world * width,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(out, buf, group=group)
    pieces = []
    for r in range(world):
        s, e = shard_range(n_total, r, world)
        pieces.append(out[r * width: r * width + (e - s)])
    return torch.cat(pieces, 0)


def gather_candidates(scores: torch.Tensor, idx: torch.Tensor, group=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """[nq, k] per rank -> [nq, world*k] on every rank (rank-major within a row)."""
    world = dist.get_world_size(group)
    nq, k = scores.shape
    s_all = torch.empty((world * nq, k), dtype=scores.dtype, device=scores.device)
    i_all = torch.empty((world * nq, k), dtype=idx.dtype, device=idx.device)
    dist.all_gather_into_tensor(s_all, scores.contiguous(), group=group)
    dist.all_gather_into_tensor(i_all, idx.contiguous(), group=group)
    s_all = s_all.view(world, nq, k).permute(1, 0, 2).reshape(nq, world * k)
    i_all = i_all.view(world, nq, k).permute(1, 0, 2).reshape(nq, world * k)
    return s_all, i_all


def gather_lists(*lists: torch.Tensor, group=None) -> Tuple[torch.Tensor, ...]:
    """gather_candidates for any number of [nq, k] tensors: each becomes [nq, world * k], rank-major"""
    world = dist.get_world_size(group)
    out = []
    for t in lists:
        nq, k = t.shape
        buf = torch.empty((world * nq, k), dtype=t.dtype, device=t.device)
        dist.all_gather_into_tensor(buf, t.contiguous(), group=group)
        out.append(buf.view(world, nq, k).permute(1, 0, 2).reshape(nq, world * k))
    return tuple(out)


def merge_topk_gpu(scores: torch.Tensor, idx: torch.Tensor, parts: int, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(score desc, index asc) merge of `parts` candidate lists per row on the GPU (clm_topk_merge)."""
    from . import _capi as C
    nq, n_in = scores.shape
    k_in = n_in // parts
    s = scores.contiguous()
    i = idx.contiguous()
    os_ = torch.empty((nq, k), dtype=torch.float32, device=s.device)
    oi = torch.empty((nq, k), dtype=torch.int64, device=s.device)
    C.check(C.lib().clm_topk_merge(s.device.index, C.ptr(s), C.ptr(i), nq, parts, k_in, k, C.ptr(os_), C.ptr(oi),
                                   C.stream_of(s.device)), "clm_topk_merge")
    return os_, oi


def merge_grouped_gpu(scores: torch.Tensor, idx: torch.Tensor, gids: torch.Tensor, parts: int,
                      k: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Merge of the row shards' search_grouped lists on the GPU: scores / idx / gids [nq, parts * k_in]
    -> (scores, idx, gids) [nq, k], the first k distinct groups of the concatenation in the search
    order. clm_topk_merge orders all parts * k_in entries by (score desc, id asc); the gids follow
    their ids (unique across shards, so a sort of the input ids finds each merged id's gid; an empty
    slot keeps -1); clm_topk_distinct keeps each group's first entry. Exact: a group of the whole
    index's answer is represented by its best row, that row's shard ranks the group among its own k
    best groups (every group ahead of it there is ahead of it globally), and what other shards list
    of the same group comes later in the order and is dropped. Past 8192 entries per query, or 1024
    of them, clm_topk_merge takes ids below 2^32."""
    from . import _capi as C
    nq, n_in = scores.shape
    if nq == 0 or n_in == 0:
        dev = scores.device
        return (torch.full((nq, k), float("-inf"), dtype=torch.float32, device=dev),
                torch.full((nq, k), -1, dtype=torch.int64, device=dev),
                torch.full((nq, k), -1, dtype=torch.int64, device=dev))
    ms, mi = merge_topk_gpu(scores, idx, parts, n_in)
    si, perm = idx.sort(dim=1)
    pos = torch.searchsorted(si, mi.clamp(min=0)).clamp(max=n_in - 1)
    mg = torch.where(mi >= 0, gids.gather(1, perm.gather(1, pos)), torch.full_like(mi, -1)).contiguous()
    dev = ms.device
    os_ = torch.empty((nq, k), dtype=torch.float32, device=dev)
    oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
    og = torch.empty((nq, k), dtype=torch.int64, device=dev)
    found = torch.empty((nq,), dtype=torch.int32, device=dev)
    C.check(C.lib().clm_topk_distinct(dev.index, C.ptr(ms), C.ptr(mi), C.ptr(mg), None, n_in, nq, int(k),
                                      C.ptr(os_), C.ptr(oi), C.ptr(og), C.ptr(found), C.stream_of(dev)),
            "clm_topk_distinct")
    return os_, oi, og


def merge_lse(lses, errs=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lse f64 [nq], err f64 [nq]) of the whole index from its row shards' CosineIndex.logsumexp
    results (host function): lse = logaddexp over the shards, and the error is the share-weighted
    combination sum_s w_s err_s, w_s = exp(lse_s - lse) the shard's share of the sum -- each
    shard's true sum lies within e^(+-err_s) of its computed one, so the whole lies within
    e^(+-max err), and the weighted mean is the first-order value of that. To stay a bound at any
    size it is taken as log sum_s w_s e^(err_s) (>= the weighted mean, <= the maximum)."""
    L = torch.stack([torch.as_tensor(v).detach().double().cpu().reshape(-1) for v in lses])
    if errs is None:
        E = torch.zeros_like(L)
    else:
        E = torch.stack([torch.as_tensor(v).detach().double().cpu().reshape(-1) for v in errs])
    if L.shape != E.shape or L.shape[0] == 0:
        raise ValueError("one lse vector (and one err vector) per shard expected")
    lse = torch.logsumexp(L, dim=0)
    err = torch.logsumexp(L + E, dim=0) - lse
    return lse, torch.clamp(err, min=0.0)


def ranges_after_remove(sizes, starts, ids):
    """Bookkeeping of ShardedIndex.remove (host function). Shard r holds global rows
    [starts[r], starts[r] + sizes[r]), the shards in global order. For the global ids to remove
    (any order, duplicates count once) returns (local, new_sizes, new_starts): local[r] = the
    sorted distinct ids that fall in shard r (still global ids, as clm_index_remove takes them),
    new_sizes[r] = what shard r keeps, new_starts = the exclusive prefix sums of new_sizes -- the
    survivors renumbered contiguously in order. ValueError for an id no shard holds."""
    sizes, starts = [int(s) for s in sizes], [int(s) for s in starts]
    if len(sizes) != len(starts):
        raise ValueError("one size and one start per shard expected")
    local = [[] for _ in sizes]
    for g in sorted({int(i) for i in ids}):
        for r, (s, n) in enumerate(zip(starts, sizes)):
            if s <= g < s + n:
                local[r].append(g)
                break
        else:
            raise ValueError(f"global id {g} is in no shard")
    new_sizes = [n - len(loc) for n, loc in zip(sizes, local)]
    new_starts, acc = [], 0
    for n in new_sizes:
        new_starts.append(acc)
        acc += n
    return local, new_sizes, new_starts


def merge_ragged(parts):
    """Merge of the row shards' CosineIndex.search_above results (host function). parts: one
    (offsets [nq + 1], scores [total], ids [total]) per shard, ids global. Returns the same triple
    (CPU tensors) for the whole index: each query's entries are the concatenation of the shards'
    lists, ordered by (score desc, id asc) with NaN above every number -- the order of `search`,
    so the merged result is what one index over all the rows returns. Shards may be empty."""
    import numpy as np
    parts = [tuple(torch.as_tensor(t).detach().cpu() for t in p) for p in parts]
    if not parts:
        raise ValueError("one (offsets, scores, ids) triple per shard expected")
    nq = parts[0][0].numel() - 1
    qid, sc, ix = [], [], []
    for off, s, i in parts:
        if off.numel() != nq + 1 or s.numel() != int(off[-1]) or i.numel() != s.numel():
            raise ValueError("shard results disagree on the number of queries or entries")
        qid.append(np.repeat(np.arange(nq, dtype=np.int64), np.diff(off.numpy().astype(np.int64))))
        sc.append(s.to(torch.float32).numpy())
        ix.append(i.to(torch.int64).numpy())
    qid, sc, ix = np.concatenate(qid), np.concatenate(sc), np.concatenate(ix)
    bits = np.where(np.isnan(sc), sc.view(np.uint32) & np.uint32(0x7FFFFFFF), sc.view(np.uint32))   # any NaN first
    key = np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.int64)   # float_key
    order = np.lexsort((ix, -key, qid))
    counts = np.bincount(qid, minlength=nq) if nq else np.zeros((0,), dtype=np.int64)
    off = np.zeros((nq + 1,), dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    return torch.from_numpy(off), torch.from_numpy(sc[order].copy()), torch.from_numpy(ix[order].copy())


class ShardedIndex:
    """Row-sharded cosine index: this rank holds rows [start, stop) of n_total."""

    def __init__(self, dim: int, n_total: int, group=None, device=None,
                 local_factory: Optional[Callable] = None):
        self.group = group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.dim = dim
        self.n_total = n_total
        self.start, self.stop = shard_range(n_total, self.rank, self.world)
        if local_factory is None:
            from .search import CosineIndex
            local_factory = lambda: CosineIndex(dim, capacity=max(self.stop - self.start, 1), device=device)  # noqa
        self.local = local_factory()
        self.local.set_offset(self.start)
        # every rank's shard size (shard_range until a remove changes them)
        self._sizes = [e - s for s, e in (shard_range(n_total, r, self.world) for r in range(self.world))]

    def append_shard(self, rows: torch.Tensor) -> None:
        if rows.shape[0] != self.stop - self.start:
            raise ValueError("rows must be exactly this rank's shard")
        self.local.append(rows)

    def remove(self, global_ids) -> int:
        """Remove rows by global id; every rank passes the same ids (a collective call). Each rank
        removes the ids inside its [start, stop) from its resident shard in place, one all_gather
        of the new local sizes follows, and every rank renumbers: start / stop / the local offset
        become the exclusive prefix sums of those sizes, so the survivors are numbered
        contiguously in their old order -- as in one index that removed the same ids. Returns the
        number of rows removed over all shards. ValueError (on every rank, before anything
        changes) for an id outside [0, n_total)."""
        starts, acc = [], 0
        for n in self._sizes:
            starts.append(acc)
            acc += n
        local, new_sizes, new_starts = ranges_after_remove(self._sizes, starts, global_ids)
        if local[self.rank]:
            self.local.remove(local[self.rank])
        mine = torch.tensor([len(self.local)], dtype=torch.int64, device=getattr(self.local, "device", "cpu"))
        if self.world > 1:
            got = torch.empty((self.world,), dtype=torch.int64, device=mine.device)
            dist.all_gather_into_tensor(got, mine, group=self.group)
        else:
            got = mine
        sizes = [int(v) for v in got.tolist()]
        if sizes != new_sizes:
            raise RuntimeError(f"ShardedIndex.remove: the ranks hold {sizes} rows, expected {new_sizes} "
                               "(did every rank pass the same ids?)")
        removed = self.n_total - sum(sizes)
        self._sizes = sizes
        self.start = new_starts[self.rank]
        self.stop = self.start + sizes[self.rank]
        self.n_total = sum(sizes)
        self.local.set_offset(self.start)
        return removed

    def search(self, queries: torch.Tensor, k: int,
               merge: Callable = merge_topk_gpu, allow=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """allow: a row filter over the WHOLE index, the same on every rank -- a bool [n_total] or
        global ids to keep; each rank applies its slice [start, stop) (CosineIndex.search's allow) and
        the lists merge as ever. A shard without rows or without an allowed row contributes
        (-inf, -1) lists."""
        if allow is None:
            s, i = self.local.search(queries, k)
        else:
            from .search import _allowed_rows
            a = torch.as_tensor(allow)
            keep = _allowed_rows(self.n_total, 0, keep=a) if a.dtype == torch.bool else \
                _allowed_rows(self.n_total, 0, ids=a)
            mine = keep[self.start: self.stop]
            if len(self.local) == 0:   # an empty index refuses the call
                nq = 1 if torch.as_tensor(queries).dim() == 1 else torch.as_tensor(queries).shape[0]
                dev = getattr(self.local, "device", "cpu")
                s = torch.full((nq, k), float("-inf"), dtype=torch.float32, device=dev)
                i = torch.full((nq, k), -1, dtype=torch.int64, device=dev)
            else:
                s, i = self.local.search(queries, k, allow=mine)
        if self.world == 1:
            return s, i
        s_all, i_all = gather_candidates(s, i, self.group)
        return merge(s_all, i_all, self.world, k)

    def search_where(self, queries: torch.Tensor, k: int, values, lo, hi, allow=None,
                     merge: Callable = merge_topk_gpu) -> Tuple[torch.Tensor, torch.Tensor]:
        """CosineIndex.search_where over the whole sharded index (a collective call): one inclusive value
        range per query. values: one number per row of the WHOLE index [n_total], the same on every rank;
        lo / hi: as CosineIndex.search_where takes them; allow: as in `search`. The ranks are planned on
        the full values (key_ranks), so every shard reads the bounds alike; each rank searches its slice of
        the keys and the lists merge as `search`'s do. A shard without rows contributes (-inf, -1) lists."""
        from .search import KeyPlan, _allowed_rows, key_ranks
        v = torch.as_tensor(values).reshape(-1)
        if v.numel() != self.n_total:
            raise ValueError(f"values must hold one number per row of the whole index ({self.n_total}), got {v.numel()}")
        keep = None
        if allow is not None:
            a = torch.as_tensor(allow)
            keep = _allowed_rows(self.n_total, 0, keep=a) if a.dtype == torch.bool else \
                _allowed_rows(self.n_total, 0, ids=a)
        dev = getattr(self.local, "device", "cpu")
        if len(self.local) == 0:   # an empty index refuses the call
            nq = 1 if torch.as_tensor(queries).dim() == 1 else torch.as_tensor(queries).shape[0]
            s = torch.full((nq, k), float("-inf"), dtype=torch.float32, device=dev)
            i = torch.full((nq, k), -1, dtype=torch.int64, device=dev)
        else:
            keys, uniq, _ = key_ranks(v, keep)
            mine = keys[self.start: self.stop].to(dev).contiguous()
            # the shard's own prefix counts: what its lists must hold
            cum = torch.zeros((uniq.numel() + 1,), dtype=torch.int64, device=dev)
            cum[1:] = torch.cumsum(torch.bincount(mine[mine >= 0].to(torch.int64), minlength=uniq.numel()), 0)
            plan = KeyPlan(mine, uniq.to(dev), cum, self.stop - self.start)
            s, i = self.local.search_where(queries, k, plan, lo, hi)
        if self.world == 1:
            return s, i
        s_all, i_all = gather_candidates(s, i, self.group)
        return merge(s_all, i_all, self.world, k)

    def search_grouped(self, queries: torch.Tensor, k: int, groups, allow=None,
                       merge: Callable = merge_grouped_gpu) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """CosineIndex.search_grouped over the whole sharded index (a collective call): (scores, idx,
        gids) [nq, k], the k best distinct groups. groups: int64 [n_total] group ids of the WHOLE
        index, the same on every rank (a group may span shards); allow: as in `search`. Each rank
        searches its slice for its k best groups, one gather of the (score, id, gid) lists follows and
        `merge` (merge_grouped_gpu) keeps the first k distinct groups of their union -- exact, see
        there. A shard without rows or without an allowed row contributes (-inf, -1, -1) lists."""
        g = torch.as_tensor(groups).reshape(-1)
        if g.numel() != self.n_total:
            raise ValueError(f"groups must hold one id per row of the whole index ({self.n_total}), got {g.numel()}")
        mine = None
        if allow is not None:
            from .search import _allowed_rows
            a = torch.as_tensor(allow)
            keep = _allowed_rows(self.n_total, 0, keep=a) if a.dtype == torch.bool else \
                _allowed_rows(self.n_total, 0, ids=a)
            mine = keep[self.start: self.stop]
        if len(self.local) == 0:   # an empty index refuses the call
            nq = 1 if torch.as_tensor(queries).dim() == 1 else torch.as_tensor(queries).shape[0]
            dev = getattr(self.local, "device", "cpu")
            s = torch.full((nq, k), float("-inf"), dtype=torch.float32, device=dev)
            i = torch.full((nq, k), -1, dtype=torch.int64, device=dev)
            gi = torch.full((nq, k), -1, dtype=torch.int64, device=dev)
        else:
            s, i, gi = self.local.search_grouped(queries, k, g[self.start: self.stop], allow=mine)
        if self.world == 1:
            return s, i, gi
        s_all, i_all, g_all = gather_lists(s, i, gi, group=self.group)
        return merge(s_all, i_all, g_all, self.world, k)

    def search_above(self, queries: torch.Tensor, threshold):
        """CosineIndex.search_above over the whole sharded index (a collective call): each rank
        searches its shard, one gather of the ragged lists follows -- the offsets first (equal
        sizes), then scores and ids padded to the longest shard result -- and merge_ragged orders
        every query's concatenation. Returns (offsets, scores, ids), identical on every rank and to
        one index holding all the rows, on the device of the local result."""
        if len(self.local) == 0:   # a shard a remove emptied: no entries (an empty index refuses the call)
            nq = 1 if torch.as_tensor(queries).dim() == 1 else torch.as_tensor(queries).shape[0]
            dev = getattr(self.local, "device", "cpu")
            off = torch.zeros((nq + 1,), dtype=torch.int64, device=dev)
            s = torch.empty((0,), dtype=torch.float32, device=dev)
            i = torch.empty((0,), dtype=torch.int64, device=dev)
        else:
            off, s, i = self.local.search_above(queries, threshold)
        if self.world == 1:
            return off, s, i
        dev = s.device
        off = off.to(dev).contiguous()
        offs = torch.empty((self.world * off.numel(),), dtype=torch.int64, device=dev)
        dist.all_gather_into_tensor(offs, off, group=self.group)
        offs = offs.view(self.world, -1).cpu()
        width = max(int(offs[:, -1].max()), 1)
        sp = torch.zeros((width,), dtype=torch.float32, device=dev)
        ip = torch.zeros((width,), dtype=torch.int64, device=dev)
        sp[: s.numel()] = s
        ip[: i.numel()] = i
        s_all = torch.empty((self.world * width,), dtype=torch.float32, device=dev)
        i_all = torch.empty((self.world * width,), dtype=torch.int64, device=dev)
        dist.all_gather_into_tensor(s_all, sp, group=self.group)
        dist.all_gather_into_tensor(i_all, ip, group=self.group)
        s_all, i_all = s_all.view(self.world, width).cpu(), i_all.view(self.world, width).cpu()
        parts = [(offs[r], s_all[r, : int(offs[r, -1])], i_all[r, : int(offs[r, -1])]) for r in range(self.world)]
        return tuple(t.to(dev) for t in merge_ragged(parts))


def build_index_sharded(encode_rows: Callable[[int, int], torch.Tensor], n_total: int, batch: int,
                        group=None, exchange: Optional[Callable[[torch.Tensor], torch.Tensor]] = None,
                        restore: Optional[Callable[[torch.Tensor], torch.Tensor]] = None) -> torch.Tensor:
    """Index build over N GPUs: encode_rows(start, stop) encodes global rows [start, stop)
    (e.g. a slice of images or captions) on this rank's GPU; returns all n_total embeddings
    on every rank (one all_gather). exchange / restore (optional) map the local rows to the form
    that crosses the links and the gathered rows back (index_build's fp16 exchange: half the
    bytes of the fp32 rows)."""
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    start, stop = shard_range(n_total, rank, world)
    outs = [encode_rows(s, min(s + batch, stop)) for s in range(start, stop, batch)]
    local = torch.cat(outs, 0) if outs else encode_rows(start, start)   # [0, D] for an empty shard
    if exchange is not None:
        local = exchange(local)
    rows = all_gather_rows(local, n_total, group)
    return restore(rows) if restore is not None else rows
