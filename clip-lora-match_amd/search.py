"""Drop-in for src/embedding/search.py: SearchResult + TextSearchIndex, backed by
an HBM-resident fp16 index (libclm clm_index_*) and the gfx950 cosine GEMM +
exact top-k kernels.

  SearchResult                       search.py:14-20
  TextSearchIndex.__init__           search.py:24-68  (key variants :41-56, re-normalise :68)
  .search_with_embedding             search.py:70-115 (shape checks :80-90, safe metadata :103-105)
  .search_by_text / .search_by_image search.py:117-151
New: .append / .save keep the index resident with amortised
O(1) append instead of FinderService's torch.cat + full re-save per report
(finder_service.py:93-103,172-185; the report flow itself is finder.py), and
.search_batch serves many queries per launch. .save_shard / .load_shard persist the HBM
index itself (SURVEY §5 checkpoint row): a raw shard of the fp16 MFMA operands, their fp32
inverse norms and the fp32 rows, streamed back to HBM without re-normalising or re-rounding
anything (the .pt reload of search.py:29-36,68 costs torch.load + an fp32 normalise of every
row + the fp16 rounding), bit-identical in search.

.remove / .update (CosineIndex and TextSearchIndex) take rows out of the resident index or replace
them in place (clm_index_remove / clm_index_update): an item handed back stops matching, a
corrected description changes its row, without the read-back / reset / re-append of the whole
index; the result is bit for bit the index built from the final rows.

.search_grouped (CosineIndex; group_by= on TextSearchIndex.search_*) answers "which k ITEMS match
best" when an item owns several rows: the first k rows of the search order that open a new group
(clm_topk_distinct), each group standing by its exact best row.

Scores are the exact cosines of the stored fp32 rows (fp64 arithmetic, rounded
once): the fp16 MFMA pass only bounds the candidates (clm_index_search). Top-k
order is (score desc, index asc); CPU torch.topk leaves exact ties in arbitrary
order (SURVEY §7 hard part 2).
"""
from __future__ import annotations

import ctypes
import json
import math
import struct
from dataclasses import dataclass
from pathlib import Path
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _capi as C


@dataclass
class SearchResult:
    """Satu hasil pencarian."""
    index: int
    score: float
    image_path: str
    text: str


def _pad_dim(x: torch.Tensor, dim_p: int) -> torch.Tensor:
    if x.shape[-1] == dim_p:
        return x
    return torch.nn.functional.pad(x, (0, dim_p - x.shape[-1]))


# |fp16-pass score - exact cosine| for dim <= 8192 (LSE_E in csrc/capi_search.cpp; DESIGN.md derives it)
PASS_E = 1.95e-3 + 4.9e-4 + 1e-6


def softmax_grad_bound(scale: float, n_terms: int, wq: float = 1.0, wr: float = 1.0, dim: Optional[int] = None):
    """(rho, tau) of CosineIndex.softmax_grad: per output row ||computed - true|| <= rho * A + tau, A =
    the row's weight mass, n_terms = the terms summed into the row (N for dq, nq for dr). DESIGN.md
    derives every factor:
      the weights' scores   expm1(scale * E + eps_x); dim=None: E = PASS_E against the caller's own
                            rows (the certified bound); dim given: E = dim * 2^-24 + 1e-6 against the
                            fp64 value from the same fp16 operands (the tight bound);
                            eps_x = 2^-24 (4.04 scale + 70) + 2^-23: the exponent's fp32 forming, v_exp_f32
      W's rounding to fp16  2^-11
      the operand           certified: 3 * 2^-11 (rounded to fp16 when stored, renormalised by the
                            inverse norm of the rounded row, re-rounded by the transposing copy);
                            tight: 2^-11 (the copy's re-rounding alone)
      fp32 accumulation     (n_terms / 32 + n_terms / 64 + 16) 2^-24: MFMA steps, chunk and slice sums
    tau = n_terms * 2^-14 * (wq + wr) * exp(2 scale PASS_E) / 65504: weights below fp16's normal range
    (under 9.3e-10 of the largest possible one) may lose everything."""
    e_score = PASS_E if dim is None else dim * 2.0 ** -24 + 1e-6
    eps_x = 2.0 ** -24 * (4.04 * scale + 70.0) + 2.0 ** -23
    e1 = math.expm1(scale * e_score + eps_x)
    u = 2.0 ** -11
    acc = (n_terms / 32 + n_terms / 64 + 16) * 2.0 ** -24
    rho = (1 + e1) * (1 + u) * (1 + (3 * u if dim is None else u) + acc) - 1
    tau = n_terms * 2.0 ** -14 * (wq + wr) * math.exp(2 * scale * PASS_E) / 65504
    return rho, tau


def pack_mask(keep: torch.Tensor) -> torch.Tensor:
    """bool [N] -> the ceil(N / 32) little-endian uint32 words of a row filter (bit j & 31 of word
    j >> 5 = keep[j]; the bits past N clear), stored as int32 on keep's device"""
    keep = torch.as_tensor(keep).reshape(-1)
    n = keep.numel()
    nw = (n + 31) // 32
    bits = torch.zeros((nw * 32,), dtype=torch.int64, device=keep.device)
    bits[:n] = keep.to(torch.int64)
    w = (bits.view(nw, 32) << torch.arange(32, dtype=torch.int64, device=keep.device)).sum(1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def _allowed_rows(n: int, offset: int, keep=None, ids=None, exclude=None, device=None) -> torch.Tensor:
    """bool [n] (local row order) from a bool [n], global ids to keep, or global ids to exclude"""
    if keep is not None:
        k = torch.as_tensor(keep).reshape(-1)
        if k.dtype != torch.bool or k.numel() != n:
            raise ValueError(f"keep must be a bool tensor of {n} rows, got {k.dtype} x {k.numel()}")
        return k.to(device)
    g = torch.as_tensor(ids if ids is not None else exclude).reshape(-1).to(device=device, dtype=torch.int64)
    loc = g - int(offset)
    if g.numel() and (int(loc.min()) < 0 or int(loc.max()) >= n):
        raise ValueError(f"a row id is outside the index [{int(offset)}, {int(offset) + n})")
    out = torch.zeros((n,), dtype=torch.bool, device=device) if ids is not None else \
        torch.ones((n,), dtype=torch.bool, device=device)
    out[loc] = ids is not None
    return out


def unpack_mask(words: torch.Tensor, n: int) -> torch.Tensor:
    """the inverse of pack_mask: mask words (int32 / uint32 storage) -> bool [n] on their device"""
    w = torch.as_tensor(words).reshape(-1).to(torch.int64)
    bits = (w[:, None] >> torch.arange(32, dtype=torch.int64, device=w.device)) & 1
    return bits.reshape(-1)[:n].to(torch.bool)


def group_row_bound(k: int, m: int) -> int:
    """(k - 1) * m + 1: with at most m rows in a group, the first that many rows of any order hold k
    distinct groups -- k - 1 groups fill at most (k - 1) * m of them (pigeonhole) -- or else every row"""
    return (int(k) - 1) * int(m) + 1


def group_ids_from_keys(keys) -> torch.Tensor:
    """hashable keys [N] -> dense int64 group ids [N], numbered by first occurrence (CPU)"""
    seen: dict = {}
    return torch.tensor([seen.setdefault(key, len(seen)) for key in keys], dtype=torch.int64)


def key_ranks(values, allow=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """values [N] (any integer or floating dtype, no NaN) -> (keys int32 [N], uniq [U], cum int64 [U + 1]):
    uniq = the sorted distinct values, keys[j] = the rank of values[j] among them -- or -1, which no range
    of key_bounds holds, where allow (bool [N]) excludes row j: a batch-wide filter rides on the keys --,
    cum[r] = the allowed rows of rank < r. Torch ops on values' device."""
    if not isinstance(values, torch.Tensor):   # Python floats at their own precision (float64)
        values = np.asarray(values)
    v = torch.as_tensor(values).reshape(-1)
    if v.dtype == torch.bool:
        v = v.to(torch.int64)
    if v.is_complex():
        raise TypeError("key values must be integers or floats")
    if v.is_floating_point() and bool(torch.isnan(v).any()):
        raise ValueError("key values must not hold NaN: a NaN has no rank")
    uniq, inv = torch.unique(v, sorted=True, return_inverse=True)
    keys = inv.to(torch.int32)
    if allow is not None:
        keep = torch.as_tensor(allow).reshape(-1)
        if keep.dtype != torch.bool or keep.numel() != v.numel():
            raise ValueError(f"allow must be a bool tensor of {v.numel()} rows, got {keep.dtype} x {keep.numel()}")
        keep = keep.to(v.device)
        keys = torch.where(keep, keys, torch.full_like(keys, -1))
        inv = inv[keep]
    cum = torch.zeros((uniq.numel() + 1,), dtype=torch.int64, device=v.device)
    cum[1:] = torch.cumsum(torch.bincount(inv, minlength=uniq.numel()), 0)
    return keys, uniq, cum


def _key_edge(uniq: torch.Tensor, bound, nq: Optional[int], lower: bool) -> torch.Tensor:
    """one side of key_bounds: the bound values [nq] (a scalar broadcasts, None = open) -> the first rank
    inside (lower) or the last rank inside (upper), int64 on uniq's device"""
    U = uniq.numel()
    if bound is None:
        bound = -math.inf if lower else math.inf
    if not isinstance(bound, torch.Tensor):   # Python floats at their own precision (float64), not torch's float32
        bound = np.asarray(bound)
    b = torch.as_tensor(bound).reshape(-1).to(uniq.device)
    if b.dtype == torch.bool or b.is_complex():
        raise TypeError("key bounds must be integers or floats")
    if b.is_floating_point() and bool(torch.isnan(b).any()):
        raise ValueError("a key bound is NaN")
    if nq is not None and b.numel() not in (1, nq):
        raise ValueError(f"key bounds: {b.numel()} values for {nq} queries")
    if b.is_floating_point() and not uniq.is_floating_point():
        # integer values against a fractional or infinite bound: the nearest integer inside, clamped to
        # what int64 holds (a bound beyond it lies beyond every value)
        lim = float(2 ** 62)
        b = (torch.ceil(b.double()) if lower else torch.floor(b.double())).clamp(-lim, lim).to(torch.int64)
        u = uniq.to(torch.int64).clamp(-(2 ** 62) + 1, 2 ** 62 - 1)
    elif uniq.is_floating_point() or b.is_floating_point():
        b, u = b.double(), uniq.double()
    else:
        b, u = b.to(torch.int64), uniq.to(torch.int64)
    r = torch.searchsorted(u, b, right=not lower) if U else torch.zeros_like(b, dtype=torch.int64)
    r = r if lower else r - 1
    return r.expand(nq).contiguous() if nq is not None and r.numel() == 1 else r


def key_bounds(uniq, cum, lo, hi, nq: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Per-query value bounds, inclusive, -> (klo int32 [nq], khi int32 [nq], n_in int64 [nq]) over the
    ranks of key_ranks: klo = the first rank with uniq >= lo, khi = the last with uniq <= hi (klo > khi: no
    value lies inside), n_in = the allowed rows inside. lo / hi: [nq] values, a scalar (every query), or
    None / -inf / +inf for an open side; nq (optional) is what two scalars broadcast to."""
    uniq, cum = torch.as_tensor(uniq), torch.as_tensor(cum).to(torch.int64)
    klo, khi = _key_edge(uniq, lo, nq, True), _key_edge(uniq, hi, nq, False)
    if klo.numel() != khi.numel():
        n = max(klo.numel(), khi.numel())
        if min(klo.numel(), khi.numel()) != 1:
            raise ValueError(f"key bounds: {klo.numel()} lower vs {khi.numel()} upper values")
        klo, khi = klo.expand(n).contiguous(), khi.expand(n).contiguous()
    n_in = torch.where(klo <= khi, cum[(khi + 1).clamp(0, uniq.numel())] - cum[klo.clamp(0, uniq.numel())],
                       torch.zeros_like(klo))
    return klo.to(torch.int32), khi.to(torch.int32), n_in


@dataclass
class KeyPlan:
    """What search_where needs of the rows' key values (CosineIndex.key_plan), reusable until the index's
    rows change: keys [N] int32 on the device (local row order; -1 = excluded by the plan's filter), the
    sorted distinct values uniq and the prefix counts cum of key_ranks, n = the rows planned for."""
    keys: torch.Tensor
    uniq: torch.Tensor
    cum: torch.Tensor
    n: int


GROUP_ROUTE_THRESHOLD = 1   # search_grouped(route=): every query by the threshold route
GROUP_BLOCK_BUDGET = 1 << 25   # list entries one query block of the threshold route may hold


@dataclass
class GroupPlan:
    """What search_grouped needs of a group assignment (CosineIndex.group_plan), reusable until the
    index's rows change: gids [N] int64 on the device (local row order), the row filter as mask words
    and as bool [N] (None: every row), n_allowed = the allowed rows, m = the most allowed rows any one
    group holds, n_groups = the groups with an allowed row, reps = the mask words of one representative
    per such group, its lowest allowed row. list_allow = the mask the list route searches under: the
    filter, or -- without a filter, when the index holds rows that score NaN (a zero or non-finite norm)
    -- all ones, because only the filtered search is bound to list NaN-scoring rows first; else None."""
    gids: torch.Tensor
    allow: Optional[torch.Tensor]
    keep: Optional[torch.Tensor]
    list_allow: Optional[torch.Tensor]
    n: int
    n_allowed: int
    m: int
    n_groups: int
    reps: torch.Tensor


class CosineIndex:
    """GPU index of fp16 rows + fp32 inverse norms (score = q.row / (|q| |row|))."""

    def __init__(self, dim: int, capacity: int = 1024, device=None):
        C.require_gpu()
        self.dim = int(dim)
        self.dim_p = (self.dim + 63) // 64 * 64          # GEMM K granule; zero padding keeps dots/norms
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None
                                   else (torch.device(device).index or 0))
        h = ctypes.c_void_p()
        C.check(C.lib().clm_index_create(self.device.index, max(int(capacity), 1), self.dim_p, ctypes.byref(h)),
                "clm_index_create")
        self._h = h
        self._offset = 0

    def __len__(self) -> int:
        return int(C.lib().clm_index_size(self._h))

    def append(self, rows) -> None:
        t = torch.as_tensor(rows)
        if t.dim() == 1:
            t = t.unsqueeze(0)
        if t.dim() != 2 or t.shape[1] != self.dim:
            raise ValueError(f"rows must be [n, {self.dim}], got {tuple(t.shape)}")
        if t.dtype not in (torch.float32, torch.float16):
            t = t.float()
        t = _pad_dim(t.to(self.device), self.dim_p).contiguous()
        code = C.CLM_F32 if t.dtype == torch.float32 else C.CLM_F16
        C.check(C.lib().clm_index_append(self._h, C.ptr(t), code, t.shape[0], C.stream_of(self.device)),
                "clm_index_append")

    def remove(self, ids) -> int:
        """Remove the rows with these global ids (what `search` returns; any order, a duplicate
        counts once) in place in HBM; returns the number of rows removed. The survivors keep their
        order: a row's new number is its old one minus the removed rows below it. ValueError for
        an id outside the index, which is then left untouched (clm_index_remove)."""
        t = torch.as_tensor(ids, dtype=torch.int64).reshape(-1).contiguous()
        before = len(self)
        C.check(C.lib().clm_index_remove(self._h, C.ptr(t) if t.numel() else None, t.numel(),
                                         C.stream_of(self.device)), "clm_index_remove")
        return before - len(self)

    def update(self, ids, rows) -> None:
        """Replace row ids[i] (global ids, distinct) by rows[i] in place in HBM, through the same
        conversion as `append`: the result equals an index built with the new rows in the first
        place. ValueError for an id outside the index or a duplicate (clm_index_update)."""
        i = torch.as_tensor(ids, dtype=torch.int64).reshape(-1).contiguous()
        t = torch.as_tensor(rows)
        if t.dim() == 1:
            t = t.unsqueeze(0)
        if t.dim() != 2 or t.shape[1] != self.dim:
            raise ValueError(f"rows must be [n, {self.dim}], got {tuple(t.shape)}")
        if t.shape[0] != i.numel():
            raise ValueError(f"{i.numel()} ids vs {t.shape[0]} rows")
        if t.dtype not in (torch.float32, torch.float16):
            t = t.float()
        t = _pad_dim(t.to(self.device), self.dim_p).contiguous()
        code = C.CLM_F32 if t.dtype == torch.float32 else C.CLM_F16
        n = i.numel()
        C.check(C.lib().clm_index_update(self._h, C.ptr(i) if n else None, C.ptr(t) if n else None, code, n,
                                         C.stream_of(self.device)), "clm_index_update")

    def reset(self) -> None:
        C.check(C.lib().clm_index_reset(self._h))

    def set_offset(self, offset: int) -> None:
        C.check(C.lib().clm_index_set_offset(self._h, int(offset)))
        self._offset = int(offset)

    def read(self, start: int = 0, n: Optional[int] = None) -> torch.Tensor:
        n = len(self) - start if n is None else n
        out = torch.empty((n, self.dim_p), dtype=torch.float32)
        C.check(C.lib().clm_index_read(self._h, start, n, C.ptr(out), C.stream_of(self.device)), "clm_index_read")
        return out[:, :self.dim]

    def search(self, queries, k: int, allow=None, route: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """queries [nq, dim] (f32/f16, any device) -> (scores [nq,k] f32, idx [nq,k] i64) on the GPU.
        allow: a row filter -- the first k of the ALLOWED rows in the same order, the same exact
        scores, (-inf, -1) past the number of allowed rows (clm_index_search_masked). Told apart by
        dtype: a bool [N], int64 global ids to keep (a list of ints), or the int32 / uint32 word
        tensor of allow_mask(); any other dtype is a TypeError (_allow_words). route: 0, or
        C.CLM_MASK_EXACT / _PASS / _GATHER to ask for a route (the results do not depend on it)."""
        if allow is not None:
            return self._search_masked(queries, k, allow, route)
        q = torch.as_tensor(queries)
        if q.dim() == 1:
            q = q.unsqueeze(0)
        if q.dim() != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must be [nq, {self.dim}], got {tuple(q.shape)}")
        if q.dtype not in (torch.float32, torch.float16):
            q = q.float()
        q = _pad_dim(q.to(self.device), self.dim_p).contiguous()
        nq = q.shape[0]
        s = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        i = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        code = C.CLM_F32 if q.dtype == torch.float32 else C.CLM_F16
        C.check(C.lib().clm_index_search(self._h, C.ptr(q), code, nq, int(k), C.ptr(s), C.ptr(i),
                                         C.stream_of(self.device)), "clm_index_search")
        return s, i

    # -------------------------------------------------------- filtered search --
    def allow_mask(self, keep=None, ids=None, exclude=None) -> torch.Tensor:
        """The device word tensor of a row filter (int32 storage of the ceil(N / 32) little-endian
        uint32 words: bit j & 31 of word j >> 5 = local row j is allowed), from exactly one of
        keep (bool [N], local row order), ids (global ids to keep) or exclude (global ids to drop).
        ValueError for an id outside the index. Torch ops only; reusable across searches until the
        index's rows change."""
        if sum(a is not None for a in (keep, ids, exclude)) != 1:
            raise ValueError("allow_mask takes exactly one of keep, ids, exclude")
        return pack_mask(_allowed_rows(len(self), getattr(self, "_offset", 0), keep, ids, exclude, self.device))

    def _allow_words(self, allow) -> torch.Tensor:
        """The word tensor of an `allow` argument, told apart by dtype alone: bool = keep [N]; int64 (what
        a Python list of ints or torch.nonzero gives) = global ids to keep; int32 / uint32 = mask words
        as allow_mask() returns them. Anything else (floats, other integer widths) is a TypeError, so
        ids are never read as words by accident: convert them to int64 or call allow_mask(ids=)."""
        a = torch.as_tensor(allow)
        if isinstance(allow, (list, tuple)) and len(allow) == 0:   # no ids (an empty list has no integer dtype)
            a = a.to(torch.int64)
        if a.dtype == torch.bool:
            return self.allow_mask(keep=a)
        if a.dtype == torch.int64:
            return self.allow_mask(ids=a)
        if a.dtype in (torch.int32, torch.uint32):
            return a.to(self.device).contiguous()
        raise TypeError(f"allow must be bool (keep), int64 (ids) or int32 / uint32 (mask words), got {a.dtype}")

    def _search_masked(self, queries, k: int, allow, route: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        q = self._queries(queries)
        nq, n = q.shape[0], len(self)
        a = self._allow_words(allow)
        if a.numel() != (n + 31) // 32:
            raise ValueError(f"allow: an int32 / uint32 tensor is read as mask words, and a mask of {n} rows holds "
                             f"{(n + 31) // 32} of them, got {a.numel()} (ids go as int64 or through allow_mask(ids=))")
        s = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        i = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        code = C.CLM_F32 if q.dtype == torch.float32 else C.CLM_F16
        C.check(C.lib().clm_index_search_masked(self._h, C.ptr(q) if nq else None, code, nq, int(k),
                                                C.ptr(a) if nq else None, int(route), C.ptr(s) if nq else None,
                                                C.ptr(i) if nq else None, C.stream_of(self.device)),
                "clm_index_search_masked")
        return s, i

    def mask_stats(self) -> dict:
        """filtered-search queries served by the MFMA pass route (`pass`), the gather route (`gather`)
        and the exact route (`exact`; a pass-route query redone exactly counts here)"""
        v = (ctypes.c_int64 * 20)()
        C.check(C.lib().clm_index_stats2(self._h, v, 20))
        return {"pass": v[17], "gather": v[18], "exact": v[19]}

    # ----------------------------------------------------------- keyed search --
    def key_plan(self, values, allow=None) -> KeyPlan:
        """The KeyPlan of one value per row (values [N], local row order: timestamps, categories, prices
        -- any integer or floating dtype, no NaN) and an optional batch-wide row filter (allow as `search`
        takes it). Torch ops only; reusable across search_where calls until the index's rows change."""
        n = len(self)
        v = torch.as_tensor(values).reshape(-1)
        if v.numel() != n:
            raise ValueError(f"key values: {v.numel()} for an index of {n} rows")
        keep = None if allow is None else unpack_mask(self._allow_words(allow), n)
        keys, uniq, cum = key_ranks(v.to(self.device), keep)
        return KeyPlan(keys.contiguous(), uniq, cum, n)

    def search_where(self, queries, k: int, keys, lo, hi, allow=None,
                     route: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """Exact top-k under one value range PER QUERY, in one batched pass: row j competes for query i
        iff lo[i] <= value[j] <= hi[i] (inclusive; lo / hi as key_bounds takes them: [nq], a scalar, None
        or an infinity for an open side). keys: a key_plan(), or the values [N] themselves, planned on
        the fly with `allow` (a batch-wide filter as `search` takes it; a KeyPlan holds its own, so allow
        must then be None). Row i of the result is search(queries[i], k, allow=the rows in its range):
        the same order, exact scores and ids, (-inf, -1) past the rows in range. k <= 1024. route: 0, or
        C.CLM_MASK_EXACT / _PASS (the results do not depend on it). (clm_index_search_keyed)"""
        if isinstance(keys, KeyPlan):
            if allow is not None:
                raise ValueError("search_where: a KeyPlan holds its own filter (key_plan(values, allow=)); allow must be None")
            plan = keys
        else:
            plan = self.key_plan(keys, allow)
        q = self._queries(queries)
        nq, n = q.shape[0], len(self)
        if plan.n != n or plan.keys.numel() != n:
            raise ValueError(f"search_where: the key plan holds {plan.n} rows, the index {n}: plan again after the rows change")
        klo, khi, n_in = key_bounds(plan.uniq, plan.cum, lo, hi, nq)
        klo, khi, n_in = klo.contiguous(), khi.contiguous(), n_in.contiguous()
        s = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        i = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        code = C.CLM_F32 if q.dtype == torch.float32 else C.CLM_F16
        some = nq > 0
        C.check(C.lib().clm_index_search_keyed(self._h, C.ptr(q) if some else None, code, nq, int(k),
                                               C.ptr(plan.keys) if some else None, C.ptr(klo) if some else None,
                                               C.ptr(khi) if some else None, C.ptr(n_in) if some else None,
                                               int(route), C.ptr(s) if some else None, C.ptr(i) if some else None,
                                               C.stream_of(self.device)), "clm_index_search_keyed")
        return s, i

    def where_stats(self) -> dict:
        """keyed-search queries served by the MFMA pass route (`pass`) and by the exact route (`exact`; a
        pass-route query redone exactly counts here)"""
        v = (ctypes.c_int64 * 22)()
        C.check(C.lib().clm_index_stats2(self._h, v, 22))
        return {"pass": v[20], "exact": v[21]}

    # ------------------------------------------------------------------ ranks --
    def _queries(self, queries) -> torch.Tensor:
        q = torch.as_tensor(queries)
        if q.dim() == 1:
            q = q.unsqueeze(0)
        if q.dim() != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must be [nq, {self.dim}], got {tuple(q.shape)}")
        if q.dtype not in (torch.float32, torch.float16):
            q = q.float()
        return _pad_dim(q.to(self.device), self.dim_p).contiguous()

    def rank(self, queries, targets, band_cap: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """Exact retrieval rank of each query's target row (a global id, see set_offset) in the whole
        index: (ranks [nq] i64, scores [nq] f32) on the GPU, rank = 1 + the number of rows ahead of
        the target in the search order (exact score desc, index asc), score = the target's exact
        score -- search(q, k)[1][rank - 1] == target for every k >= rank. No score matrix and no
        sort: one fp16 MFMA pass counts, the rows too close to call are re-scored exactly
        (clm_index_rank). band_cap: clm.h (0 = default; CLM_RANK_EXACT / CLM_RANK_BAND force a route).
        ValueError for a target outside the index or an empty index."""
        q = self._queries(queries)
        nq = q.shape[0]
        t = torch.as_tensor(targets).to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
        if t.numel() != nq:
            raise ValueError(f"targets must hold one row id per query ({nq}), got {t.numel()}")
        ranks = torch.empty((nq,), dtype=torch.int64, device=self.device)
        scores = torch.empty((nq,), dtype=torch.float32, device=self.device)
        code = C.CLM_F32 if q.dtype == torch.float32 else C.CLM_F16
        C.check(C.lib().clm_index_rank(self._h, C.ptr(q), code, nq, C.ptr(t), C.ptr(ranks), C.ptr(scores),
                                       int(band_cap), C.stream_of(self.device)), "clm_index_rank")
        return ranks, scores

    def count_above(self, queries, scores, indices, band_cap: int = 0) -> torch.Tensor:
        """[nq] i64: the rows of THIS index ahead of a target with exact score scores[i] and global id
        indices[i] (which may belong to another shard) for query i; the counts of row shards add up
        to the whole index's (clm_index_count_above)."""
        q = self._queries(queries)
        nq = q.shape[0]
        s = torch.as_tensor(scores).to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        g = torch.as_tensor(indices).to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
        if s.numel() != nq or g.numel() != nq:
            raise ValueError(f"scores and indices must hold one entry per query ({nq})")
        out = torch.empty((nq,), dtype=torch.int64, device=self.device)
        code = C.CLM_F32 if q.dtype == torch.float32 else C.CLM_F16
        C.check(C.lib().clm_index_count_above(self._h, C.ptr(q), code, nq, C.ptr(s), C.ptr(g), C.ptr(out),
                                              int(band_cap), C.stream_of(self.device)), "clm_index_count_above")
        return out

    def rank_stats(self) -> dict:
        """rank / count_above queries served by the MFMA band pass (`band`), by the exact route
        (`exact`), those of the latter whose band list overflowed its capacity (`overflow`), and the
        band rows the band pass left to the exact re-score (`band_rows`)"""
        v = (ctypes.c_int64 * 11)()
        C.check(C.lib().clm_index_stats2(self._h, v, 11))
        return {"band": v[7], "exact": v[8], "overflow": v[9], "band_rows": v[10]}

    # ------------------------------------------------------- threshold search --
    def _thresholds(self, threshold, nq: int) -> torch.Tensor:
        t = torch.as_tensor(threshold, dtype=torch.float32).reshape(-1)
        if t.numel() == 1 and nq != 1:
            t = t.expand(nq)
        if t.numel() != nq:
            raise ValueError(f"threshold must be a float or hold one value per query ({nq}), got {t.numel()}")
        return t.to(self.device).contiguous()

    def _held_result(self, off: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        total = int(off[-1])
        s = torch.empty((total,), dtype=torch.float32, device=self.device)
        i = torch.empty((total,), dtype=torch.int64, device=self.device)
        if total:
            C.check(C.lib().clm_index_search_above_read(self._h, 0, total, C.ptr(s), C.ptr(i),
                                                        C.stream_of(self.device)), "clm_index_search_above_read")
        return off.to(self.device), s, i

    def search_above(self, queries, threshold, band_cap: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Every row at or above a cosine, exactly: (offsets [nq + 1] i64, scores [total] f32, ids
        [total] i64) on the GPU. Query i owns entries [offsets[i], offsets[i + 1]): the rows whose
        exact score (that of `search`) is >= threshold[i] or NaN, in the search order (score desc, id
        asc) -- as many as count_above(q, threshold, INT64_MAX) says, and bit for bit the first
        entries of search(q, k) for any k that holds them. threshold: a float or one value per query
        (-inf: every row; a NaN threshold: only NaN-scoring rows). No [nq, N] matrix; a low
        threshold returns up to nq x N entries, each re-scored exactly (clm_index_search_above).
        band_cap: as in `rank`. ValueError for an empty index."""
        q = self._queries(queries)
        nq = q.shape[0]
        t = self._thresholds(threshold, nq)
        off = torch.empty((nq + 1,), dtype=torch.int64)
        code = C.CLM_F32 if q.dtype == torch.float32 else C.CLM_F16
        C.check(C.lib().clm_index_search_above(self._h, C.ptr(q) if nq else None, code, nq, C.ptr(t) if nq else None,
                                               C.ptr(off), int(band_cap), C.stream_of(self.device)),
                "clm_index_search_above")
        return self._held_result(off)

    def search_above_rows(self, start: int, n: int, threshold, band_cap: int = 0):
        """search_above with the index's own rows [start, start + n) (global ids) as the queries,
        taken where they lie in HBM (clm_index_search_above_rows)."""
        n = int(n)
        t = self._thresholds(threshold, n)
        off = torch.empty((n + 1,), dtype=torch.int64)
        C.check(C.lib().clm_index_search_above_rows(self._h, int(start), n, C.ptr(t) if n else None, C.ptr(off),
                                                    int(band_cap), C.stream_of(self.device)),
                "clm_index_search_above_rows")
        return self._held_result(off)

    def range_stats(self) -> dict:
        """search_above queries served by the MFMA filter pass (`fast`), by the exact route (`exact`),
        and those whose candidate list overflowed its capacity (`overflow`)"""
        v = (ctypes.c_int64 * 17)()
        C.check(C.lib().clm_index_stats2(self._h, v, 17))
        return {"fast": v[14], "exact": v[15], "overflow": v[16]}

    def near_duplicates(self, threshold: float, block: int = 4096):
        """The self-join under a threshold: (pairs [P, 2] i64, scores [P] f32) on the GPU, every
        unordered pair of rows i < j (global ids) whose exact
        cosine is >= threshold, once, without the self match, ordered by (i asc, score desc, j asc).
        search_above_rows over row blocks of `block`: the memory is that of one block's result."""
        n, offset = len(self), getattr(self, "_offset", 0)
        pairs, scores = [], []
        for r0 in range(0, n, max(int(block), 1)):
            m = min(int(block), n - r0)
            off, s, j = self.search_above_rows(int(offset) + r0, m, float(threshold))
            i = torch.repeat_interleave(torch.arange(int(offset) + r0, int(offset) + r0 + m, device=self.device),
                                        off[1:] - off[:-1])
            keep = j > i   # the result is already (i asc, score desc, j asc); a mask keeps that order
            pairs.append(torch.stack([i[keep], j[keep]], 1))
            scores.append(s[keep])
        if not pairs:
            return (torch.empty((0, 2), dtype=torch.int64, device=self.device),
                    torch.empty((0,), dtype=torch.float32, device=self.device))
        return torch.cat(pairs, 0), torch.cat(scores, 0)

    # --------------------------------------------------------- grouped search --
    def group_plan(self, groups, allow=None) -> GroupPlan:
        """Validate a group assignment once for many searches. groups: int64-able integers [N] >= 0 in
        local row order (row j of the index belongs to group groups[j]); allow: a row filter as `search`
        takes it. ValueError for a wrong length, a negative id or a non-integer dtype. Torch ops, and
        without a filter one single-query count_above pass that asks whether any row scores NaN
        (GroupPlan.list_allow); valid until the index's rows change, like allow_mask()."""
        n = len(self)
        g = torch.as_tensor(groups)
        if g.dtype in (torch.bool,) or g.is_floating_point() or g.is_complex():
            raise ValueError(f"groups must hold integer group ids, got {g.dtype}")
        g = g.reshape(-1)
        if g.numel() != n:
            raise ValueError(f"groups must hold one id per row ({n}), got {g.numel()}")
        g = g.to(device=self.device, dtype=torch.int64).contiguous()
        if n and int(g.min()) < 0:
            raise ValueError("group ids must be >= 0")
        words = keep = None
        if allow is not None:
            words = self._allow_words(allow)
            if words.numel() != (n + 31) // 32:
                raise ValueError(f"allow: a mask of {n} rows holds {(n + 31) // 32} words, got {words.numel()}")
            keep = unpack_mask(words, n)
        rows = torch.arange(n, device=self.device) if keep is None else torch.nonzero(keep).reshape(-1)
        ga = g[rows]
        m = n_groups = 0
        rep = torch.zeros((n,), dtype=torch.bool, device=self.device)
        if rows.numel():
            order = torch.argsort(ga, stable=True)   # rows ascending inside a group
            gs = ga[order]
            first = torch.ones_like(gs, dtype=torch.bool)
            first[1:] = gs[1:] != gs[:-1]
            starts = torch.nonzero(first).reshape(-1)
            counts = torch.diff(starts, append=torch.tensor([gs.numel()], device=self.device))
            m, n_groups = int(counts.max()), int(starts.numel())
            rep[rows[order[starts]]] = True
        list_allow = words
        if words is None and n:
            # a row of zero or non-finite norm scores NaN against any query, and leads the order; the
            # unfiltered search's MFMA routes cannot list such rows, the filtered search always does
            probe = torch.ones((1, self.dim), dtype=torch.float32, device=self.device)
            if int(self.count_above(probe, torch.tensor([float("nan")]), torch.tensor([2 ** 63 - 1]))[0]) > 0:
                list_allow = pack_mask(torch.ones((n,), dtype=torch.bool, device=self.device))
        return GroupPlan(gids=g, allow=words, keep=keep, list_allow=list_allow, n=n, n_allowed=int(rows.numel()),
                         m=m, n_groups=n_groups, reps=pack_mask(rep))

    def _topk_distinct(self, s, i, g, k: int, offsets=None):
        """clm_topk_distinct over fixed-width [nq, ld] lists, or ragged ones through offsets [nq + 1]"""
        s, i, g = s.contiguous(), i.contiguous(), g.contiguous()
        if offsets is None:
            nq, ld = s.shape
        else:
            offsets = offsets.to(device=self.device, dtype=torch.int64).contiguous()
            nq, ld = offsets.numel() - 1, 0
        os_ = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        oi = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        og = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        found = torch.empty((nq,), dtype=torch.int32, device=self.device)
        if nq == 0 or s.numel() == 0:   # no entry anywhere (an empty tensor has no pointer to pass)
            return os_.fill_(float("-inf")), oi.fill_(-1), og.fill_(-1), found.zero_()
        C.check(C.lib().clm_topk_distinct(self.device.index, C.ptr(s), C.ptr(i), C.ptr(g),
                                          C.ptr(offsets) if offsets is not None else None, ld, nq, int(k),
                                          C.ptr(os_), C.ptr(oi), C.ptr(og), C.ptr(found), C.stream_of(self.device)),
                "clm_topk_distinct")
        return os_, oi, og, found

    def search_grouped(self, queries, k: int, groups, allow=None, route: int = 0,
                       block_budget: int = GROUP_BLOCK_BUDGET) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The k best DISTINCT groups: (scores [nq, k] f32, idx [nq, k] i64, gids [nq, k] i64) on the GPU.
        Walk the rows in the order of `search` (NaN first, exact score desc, global id asc; with allow=
        only the allowed rows) and keep a row iff no earlier row belongs to its group: the result is the
        first k kept rows -- each group stands by its exact best row, ties by id --, scores bit for bit
        those of `search`, (-inf, -1, -1) past the number of distinct allowed groups. groups: int64 [N]
        ids >= 0 in local row order, or a group_plan() (which then holds the filter: allow must be None).
        k in [1, 1024].
        List route: with at most m allowed rows per group the first (k - 1) m + 1 rows of the order hold
        k groups or every row (group_row_bound), so search(q, L), L = min(that bound, 1024, allowed
        rows), and clm_topk_distinct over the list answer every query that found k groups -- and all of
        them when L is the bound or every allowed row. (An index that holds NaN-scoring rows is searched
        under an all-ones filter, GroupPlan.list_allow: those rows lead the order.)
        Threshold route, for the rest: theta = the k-th best score among one representative row per
        group (search(q, k, allow=plan.reps); -inf with fewer than k groups) is <= the k-th best group's
        score, so search_above(q, theta) lists every
        answer row in order; rows outside the filter are struck out and clm_topk_distinct runs over the
        ragged lists, in query blocks of at most block_budget list entries (count_above gives the
        lengths; a single query may exceed it alone). route: 0, or GROUP_ROUTE_THRESHOLD to send every
        query by the threshold route; the results do not depend on it (group_stats says who served).
        The threshold route runs search_above, so it REPLACES the index's held threshold-search result
        (clm_index_search_above_read); results search_above() already returned are copies and stay.
        ValueError for an empty index, k outside [1, 1024], or groups that group_plan refuses."""
        k = int(k)
        if not 1 <= k <= 1024:
            raise ValueError(f"search_grouped: k must be in [1, 1024], got {k}")
        n = len(self)
        if n == 0:
            raise ValueError("search_grouped: the index is empty")
        if isinstance(groups, GroupPlan):
            if allow is not None:
                raise ValueError("search_grouped: a group_plan() holds its own filter; pass allow to group_plan")
            plan = groups
        else:
            plan = self.group_plan(groups, allow)
        if plan.n != n:
            raise ValueError(f"search_grouped: the plan was made for {plan.n} rows, the index holds {n}")
        q = torch.as_tensor(queries)
        if q.dim() == 1:
            q = q.unsqueeze(0)
        if q.dim() != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must be [nq, {self.dim}], got {tuple(q.shape)}")
        q = q.to(self.device)   # unpadded: search / search_above / count_above take it as the caller's
        nq, offset = q.shape[0], int(getattr(self, "_offset", 0))
        stats = self._group_counters()
        out_s = torch.full((nq, k), float("-inf"), dtype=torch.float32, device=self.device)
        out_i = torch.full((nq, k), -1, dtype=torch.int64, device=self.device)
        out_g = torch.full((nq, k), -1, dtype=torch.int64, device=self.device)
        if nq == 0:
            return out_s, out_i, out_g
        if plan.n_allowed == 0:   # nothing competes: every slot is a pad
            stats["threshold" if int(route) == GROUP_ROUTE_THRESHOLD else "list"] += nq
            return out_s, out_i, out_g
        todo = torch.arange(nq, device=self.device)
        if int(route) != GROUP_ROUTE_THRESHOLD:
            bound = group_row_bound(k, plan.m)
            L = min(bound, 1024, plan.n_allowed)
            ls, li = self.search(q, L, allow=plan.list_allow) if plan.list_allow is not None else self.search(q, L)
            lg = torch.where(li >= 0, plan.gids[(li - offset).clamp(min=0)], torch.full_like(li, -1))
            out_s, out_i, out_g, found = self._topk_distinct(ls, li, lg, k)
            if L == bound or L == plan.n_allowed:
                todo = todo[:0]
            else:
                todo = torch.nonzero(found < k).reshape(-1)
            stats["list"] += nq - int(todo.numel())
        if todo.numel() == 0:
            return out_s, out_i, out_g
        stats["threshold"] += int(todo.numel())
        qs = q[todo]
        theta = self.search(qs, k, allow=plan.reps)[0][:, k - 1].contiguous()
        lens = self.count_above(qs, theta, torch.full((qs.shape[0],), 2 ** 63 - 1, dtype=torch.int64)).tolist()
        b0 = 0
        while b0 < len(lens):
            b1, total = b0 + 1, lens[b0]
            while b1 < len(lens) and total + lens[b1] <= int(block_budget):
                total += lens[b1]
                b1 += 1
            off, ts, ti = self.search_above(qs[b0:b1], theta[b0:b1])
            loc = ti - offset
            tg = plan.gids[loc]
            if plan.keep is not None:
                ti = torch.where(plan.keep[loc], ti, torch.full_like(ti, -1))
            bs, bi, bg, _ = self._topk_distinct(ts, ti, tg, k, offsets=off)
            rows = todo[b0:b1]
            out_s[rows], out_i[rows], out_g[rows] = bs, bi, bg
            b0 = b1
        return out_s, out_i, out_g

    def group_stats(self) -> dict:
        """search_grouped queries answered by the list route (`list`) and by the threshold route
        (`threshold`), counted in Python since the index was made"""
        return dict(self._group_counters())

    def _group_counters(self) -> dict:
        if not hasattr(self, "_group_stats"):
            self._group_stats = {"list": 0, "threshold": 0}
        return self._group_stats

    # ------------------------------------------------------------ log-sum-exp --
    def logsumexp(self, queries, scale: float, head: int = 64, band_cap: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """(lse [nq] f64, err [nq] f32) on the GPU: lse = log sum_j exp(scale * score_j) over every row
        of the index, score_j the exact score of `search`, in fp64 and without a [nq, N] matrix
        (clm_index_lse). head > 0: the fast route -- search(q, min(head, N)) gives each query's head
        floor (its last exact score), one fp16 MFMA pass sums the rows below it on chip and lists the
        rest for an exact re-score; err >= |lse - the exact route's lse|, certified. head = 0 (or a
        small problem, or band_cap | CLM_LSE_EXACT): the exact route, err = 0. Two calls return the
        same bits on either route. ValueError for an empty index or a scale that is not finite and
        positive."""
        q = self._queries(queries)
        nq = q.shape[0]
        n = len(self)
        lse = torch.empty((nq,), dtype=torch.float64, device=self.device)
        err = torch.empty((nq,), dtype=torch.float32, device=self.device)
        floor = None
        if int(head) > 0 and n > 0 and nq > 0 and not (int(band_cap) > 0 and int(band_cap) & C.CLM_LSE_EXACT):
            floor = self.search(q, min(int(head), n))[0][:, -1].contiguous()
        code = C.CLM_F32 if q.dtype == torch.float32 else C.CLM_F16
        C.check(C.lib().clm_index_lse(self._h, C.ptr(q), code, nq, float(scale),
                                      C.ptr(floor) if floor is not None else None, C.ptr(lse), C.ptr(err),
                                      int(band_cap), C.stream_of(self.device)), "clm_index_lse")
        return lse, err

    def logsumexp64(self, queries, scale: float, targets=None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """(lse [nq] f64, pair [nq] f64 or None): the reference route (clm_index_lse64). As the exact
        route of `logsumexp`, but on the unrounded fp64 cosines instead of the exact scores (fp64
        cosines rounded to fp32), and pair[i] = the fp64 cosine of query i and row targets[i] (global
        row ids, as in `rank`): what the same reduction gives on float64 tensors, to fp64 rounding."""
        q = self._queries(queries)
        nq = q.shape[0]
        lse = torch.empty((nq,), dtype=torch.float64, device=self.device)
        tg = pair = None
        if targets is not None:
            tg = torch.as_tensor(targets).to(device=self.device, dtype=torch.int64).contiguous()
            if tg.shape != (nq,):
                raise ValueError(f"targets must be [{nq}], got {tuple(tg.shape)}")
            pair = torch.empty((nq,), dtype=torch.float64, device=self.device)
        code = C.CLM_F32 if q.dtype == torch.float32 else C.CLM_F16
        C.check(C.lib().clm_index_lse64(self._h, C.ptr(q), code, nq, float(scale),
                                        C.ptr(tg) if tg is not None else None, C.ptr(lse),
                                        C.ptr(pair) if pair is not None else None, C.stream_of(self.device)),
                "clm_index_lse64")
        return lse, pair

    def softmax_topk(self, queries, k: int, scale: float = 100.0, head: int = 64):
        """(probs [nq, k] f64, idx [nq, k] i64, err [nq] f32): the k most probable rows of
        softmax(scale * score) over the whole index, probs = exp(scale * score - lse) from `search`
        and `logsumexp`; err bounds lse (so a probability is off by a factor within e^(+-err)).
        Slots past the index size hold (0, -1)."""
        s, i = self.search(queries, int(k))
        lse, err = self.logsumexp(queries, scale, head=head)
        p = torch.exp(float(scale) * s.double() - lse[:, None])
        return torch.where(i >= 0, p, torch.zeros_like(p)), i, err

    def lse_stats(self) -> dict:
        """logsumexp queries served by the MFMA pass (`fast`), by the exact route (`exact`), and those
        whose band list overflowed its capacity (`overflow`; they are among `exact`)"""
        v = (ctypes.c_int64 * 14)()
        C.check(C.lib().clm_index_stats2(self._h, v, 14))
        return {"fast": v[11], "exact": v[12], "overflow": v[13]}

    # ------------------------------------------------------------ softmax gradients --
    def softmax_grad(self, queries, scale: float, lse, row_lse=None, wq: float = 1.0, wr: float = 1.0,
                     want_rows: bool = True, chunk_rows: int = 0, query_block: int = 0):
        """(dq [nq, dim] f32, dr [N, dim] f32 or None) on the GPU: the softmax-weighted sums over the
        index, both ways, without a [nq, N] matrix (clm_index_softmax_grad). With unit vectors q^_i,
        r^_j and s_ij = q^_i . r^_j,
            W_ij = wq * exp(scale * s_ij - lse[i]) + wr * exp(scale * s_ij - row_lse[j]),
        dq[i] = sum_j W_ij r^_j and dr[j] = sum_i W_ij q^_i, dr in local row order (want_rows=False: not
        computed). lse [nq] as `logsumexp` returns it; row_lse [N] the log-sum-exp of each index row
        over the queries. One direction: wr = 0 and no row_lse -- with wq = 1, dq is the softmax read-out
        of the index and dr its adjoint; with both terms it is all of the symmetric contrastive loss's
        gradient but its diagonal.
        The scores inside W are fp16-pass scores: per output row ||computed - true|| <= rho * A + tau, A
        the row's weight mass sum W_ij, (rho, tau) = softmax_grad_bound(...) -- rho = 0.038 at scale 1 /
        0.07 and 0.28 at 100 in the certified worst case (every score off by the pass's whole bound E the
        same way); measured ratios sit near 1e-3. Two identical calls return the same bits;
        the bits may depend on nq, chunk_rows and query_block (index rows / queries per pass; 0 =
        default). ValueError: an empty index, a scale that is not finite and positive, a negative
        weight, wr > 0 without row_lse, lse of the wrong length, a zero row in the index or a zero query
        (the reference's gradient is NaN there)."""
        q = self._queries(queries)
        nq, n = q.shape[0], len(self)
        l = torch.as_tensor(lse).to(device=self.device, dtype=torch.float64).contiguous()
        if l.shape != (nq,):
            raise ValueError(f"lse must be [{nq}], got {tuple(l.shape)}")
        rl = None
        if row_lse is not None:
            rl = torch.as_tensor(row_lse).to(device=self.device, dtype=torch.float64).contiguous()
            if rl.shape != (n,):
                raise ValueError(f"row_lse must be [{n}], got {tuple(rl.shape)}")
        if int(chunk_rows) < 0 or int(query_block) < 0:
            raise ValueError("chunk_rows and query_block must not be negative")
        dq = torch.empty((nq, self.dim_p), dtype=torch.float32, device=self.device)
        dr = torch.empty((n, self.dim_p), dtype=torch.float32, device=self.device) if want_rows else None
        code = C.CLM_F32 if q.dtype == torch.float32 else C.CLM_F16
        C.check(C.lib().clm_index_softmax_grad(self._h, C.ptr(q), code, nq, float(scale), C.ptr(l),
                                               C.ptr(rl) if rl is not None else None, float(wq), float(wr),
                                               C.ptr(dq), C.ptr(dr) if dr is not None else None, int(chunk_rows),
                                               int(query_block), C.stream_of(self.device)), "clm_index_softmax_grad")
        if self.dim_p != self.dim:
            dq = dq[:, :self.dim].contiguous()
            dr = dr[:, :self.dim].contiguous() if dr is not None else None
        return dq, dr

    def grad_stats(self) -> dict:
        """softmax_grad queries served (`queries`) and the (query block, row chunk) passes run (`passes`)"""
        v = (ctypes.c_int64 * 24)()
        C.check(C.lib().clm_index_stats2(self._h, v, 24))
        return {"queries": v[22], "passes": v[23]}

    # ------------------------------------------------------------ shard file --
    def save_shard(self, path: Union[str, Path], meta: Optional[dict] = None, chunk_rows: int = 1 << 20) -> None:
        """Write the index's internal state (fp16 operands, fp32 inverse norms, the fp32 rows if
        kept) to a shard file (format: _SHARD_MAGIC, u64 header length, JSON header, then the
        sections at 4 KiB boundaries), streamed through a pinned host buffer; atomic rename."""
        path = Path(path)
        path.parent.mkdir(parents=True, exist_ok=True)
        n = len(self)
        has32 = int(C.lib().clm_index_has_f32(self._h)) == 1
        header = {"format": "clm-index-shard", "version": 1, "dim": self.dim, "dim_p": self.dim_p, "n": n,
                  "has_f32": has32, "meta": meta or {}}
        hb = json.dumps(header).encode()
        tmp = path.with_name(path.name + ".tmp")
        chunk = max(1, min(int(chunk_rows), max(n, 1)))
        b16 = torch.empty((chunk, self.dim_p), dtype=torch.float16, pin_memory=True)
        binv = torch.empty((chunk,), dtype=torch.float32, pin_memory=True)
        b32 = torch.empty((chunk, self.dim_p), dtype=torch.float32, pin_memory=True) if has32 else None
        secs = _shard_sections(len(hb), n, self.dim_p, has32)
        with open(tmp, "wb") as f:
            f.write(_SHARD_MAGIC + struct.pack("<Q", len(hb)) + hb)
            for r0 in range(0, n, chunk):
                m = min(chunk, n - r0)
                C.check(C.lib().clm_index_export(self._h, r0, m, C.ptr(b16), C.ptr(binv),
                                                 C.ptr(b32) if b32 is not None else None,
                                                 C.stream_of(self.device)), "clm_index_export")
                for name, buf in (("rows16", b16), ("inv", binv), ("rows32", b32)):
                    if buf is None:
                        continue
                    f.seek(secs[name][0] + r0 * buf[0].numel() * buf.element_size())
                    f.write(memoryview(buf[:m].numpy()).cast("B"))
            f.truncate(_shard_size(secs))
        tmp.replace(path)

    @classmethod
    def load_shard(cls, path: Union[str, Path], device=None, capacity: Optional[int] = None,
                   chunk_rows: int = 1 << 20) -> Tuple["CosineIndex", dict]:
        """(index, header) from a shard file: the sections are read chunk by chunk into a pinned
        buffer and imported into HBM as they are (clm_index_import)."""
        path = Path(path)
        if not path.exists():
            raise FileNotFoundError(f"Index shard not found: {path}")
        header, secs = read_shard_header(path)
        n, dim_p = header["n"], header["dim_p"]
        idx = cls(header["dim"], capacity=max(capacity or n, 1), device=device)
        if idx.dim_p != dim_p:
            raise ValueError(f"shard dim_p {dim_p} does not match dim {header['dim']}")
        chunk = max(1, min(int(chunk_rows), max(n, 1)))
        b16 = torch.empty((chunk, dim_p), dtype=torch.float16, pin_memory=True)
        binv = torch.empty((chunk,), dtype=torch.float32, pin_memory=True)
        b32 = torch.empty((chunk, dim_p), dtype=torch.float32, pin_memory=True) if header["has_f32"] else None
        with open(path, "rb", buffering=0) as f:
            for r0 in range(0, n, chunk):
                m = min(chunk, n - r0)
                for name, buf in (("rows16", b16), ("inv", binv), ("rows32", b32)):
                    if buf is None:
                        continue
                    row_bytes = buf[0].numel() * buf.element_size()
                    f.seek(secs[name][0] + r0 * row_bytes)
                    view = memoryview(buf.numpy()).cast("B")[: m * row_bytes]
                    if f.readinto(view) != m * row_bytes:
                        raise ValueError(f"truncated index shard {path} (section {name})")
                d16 = b16[:m].to(idx.device, non_blocking=True)
                dinv = binv[:m].to(idx.device, non_blocking=True)
                d32 = b32[:m].to(idx.device, non_blocking=True) if b32 is not None else None
                C.check(C.lib().clm_index_import(idx._h, C.ptr(d16), C.ptr(dinv), C.ptr(d32) if d32 is not None else None,
                                                 m, C.stream_of(idx.device)), "clm_index_import")
        return idx, header

    def stats(self) -> dict:
        """queries served by the sampled single-pass bounded search (`filtered`), the bounded
        search with a chunked fp16 scan as its first step (`scan_bounded`), the full exact
        scan (`full_exact`), their sum `exact`, overflow re-runs, and the queries whose filter
        pass ran on the G2 256 x 192 tiles (`filter_g2`) or, in blocks whose sampled candidate
        windows mostly exceed the list capacity, on gemm_kernel 256 x 256 (`filter_dense`)
        (include/clm.h), and the small batches (nq <= 16) served by the one-pass streaming search
        (`small_scan`)"""
        v = (ctypes.c_int64 * 7)()
        C.check(C.lib().clm_index_stats2(self._h, v, 7))
        return {"filtered": v[0], "scan_bounded": v[1], "full_exact": v[2], "exact": v[1] + v[2],
                "overflow": v[3], "filter_g2": v[4], "filter_dense": v[5], "small_scan": v[6]}

    def close(self) -> None:
        if getattr(self, "_h", None):
            C.lib().clm_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_SHARD_MAGIC = b"CLMIDX01"


def _shard_sections(header_len: int, n: int, dim_p: int, has32: bool) -> dict:
    """byte offset and length of each section, every one at a 4 KiB boundary"""
    def up(x):
        return (x + 4095) // 4096 * 4096
    off = up(len(_SHARD_MAGIC) + 8 + header_len)
    secs = {}
    for name, nbytes in (("rows16", n * dim_p * 2), ("inv", n * 4), ("rows32", n * dim_p * 4 if has32 else 0)):
        if nbytes or name != "rows32":
            secs[name] = (off, nbytes)
            off = up(off + nbytes)
    return secs


def _shard_size(secs: dict) -> int:
    return max(o + b for o, b in secs.values())


def read_shard_header(path: Union[str, Path]) -> Tuple[dict, dict]:
    """(header, sections) of a shard file; ValueError if it is not one"""
    with open(path, "rb") as f:
        magic = f.read(len(_SHARD_MAGIC))
        if magic != _SHARD_MAGIC:
            raise ValueError(f"{path} is not a clm index shard")
        (hl,) = struct.unpack("<Q", f.read(8))
        header = json.loads(f.read(hl).decode())
    if header.get("format") != "clm-index-shard" or header.get("version") != 1:
        raise ValueError(f"{path}: unsupported shard header {header.get('format')} v{header.get('version')}")
    secs = _shard_sections(hl, header["n"], header["dim_p"], header["has_f32"])
    if Path(path).stat().st_size < _shard_size(secs):
        raise ValueError(f"truncated index shard {path}")
    return header, secs


class TextSearchIndex:
    def __init__(self, index_path: Union[str, Path, None] = None, *, embeddings=None, image_paths=None,
                 texts=None, device=None):
        if index_path is not None:
            index_path = Path(index_path)
            if not index_path.exists():
                raise FileNotFoundError(f"Index file not found: {index_path}")
            obj = torch.load(index_path, map_location="cpu", weights_only=True)
        else:
            obj = {"embeddings": embeddings, "image_paths": image_paths, "texts": texts}

        embs = obj.get("embeddings")
        if embs is None:
            raise ValueError("Index file does not contain 'embeddings'")
        self.embeddings: torch.Tensor = torch.as_tensor(embs).float().cpu()
        if self.embeddings.dim() == 1:
            self.embeddings = self.embeddings.unsqueeze(0)

        images = obj.get("image_paths")
        if images is None:
            images = obj.get("image_path")
        if images is None:
            images = []
        self.image_paths: list = list(images)

        texts_ = obj.get("texts")
        if texts_ is None:
            texts_ = obj.get("text")
        if texts_ is None:
            texts_ = []
        self.texts: list = list(texts_)

        if self.embeddings.size(0) != len(self.image_paths):
            print(f"[TextSearchIndex] WARNING: embeddings rows ({self.embeddings.size(0)}) "
                  f"!= len(image_paths) ({len(self.image_paths)})")

        self.num_items, self.dim = self.embeddings.shape
        print(f"[TextSearchIndex] Loaded {self.num_items} items with dim={self.dim}")

        # Pastikan normalized (search.py:68) -- fp32 on the host, as the reference does; the GPU
        # index keeps these fp32 rows for its exact re-score
        self.embeddings = self.embeddings / self.embeddings.norm(dim=-1, keepdim=True)
        self._gpu = CosineIndex(self.dim, capacity=max(self.num_items, 1024), device=device)
        if self.num_items:
            self._gpu.append(self.embeddings)

    @classmethod
    def from_gpu_index(cls, index: "CosineIndex", image_paths: Sequence[str] = (),
                       texts: Sequence[str] = ()) -> "TextSearchIndex":
        """Wrap an HBM-resident CosineIndex (e.g. one built by index_build or load_shard) as a
        TextSearchIndex without a host copy of its rows: searches go straight to the GPU index;
        the host mirror (`embeddings`, used by save / append) is read back from HBM on first use."""
        self = cls.__new__(cls)
        self._gpu = index
        n = len(index)
        self._host, self._n = None, n
        self.num_items, self.dim = n, index.dim
        self.image_paths, self.texts = list(image_paths), list(texts)
        return self

    # host mirror of the rows: a capacity-doubling buffer, so append is amortised O(1) (the
    # reference's FinderService torch.cat's the whole index per report, finder_service.py:180)
    @property
    def embeddings(self) -> torch.Tensor:
        if self._host is None:   # from_gpu_index: the rows as the index keeps them, fetched once
            self._host = self._gpu.read(0, self._n).float()[:, : self.dim].contiguous()
        return self._host[: self._n]

    @embeddings.setter
    def embeddings(self, value) -> None:
        t = torch.as_tensor(value).float().cpu()
        self._host = t.contiguous() if t.dim() == 2 else t
        self._n = self._host.shape[0] if self._host.dim() >= 1 else 0

    # --------------------------------------------------------------- search --
    def _allow(self, allow):
        """a row filter for the GPU index: a mask / bool / ids as CosineIndex.search takes them, or a
        callable (i, image_path, text) -> bool evaluated over the host metadata"""
        if callable(allow):
            keep = [bool(allow(i, self.image_paths[i] if i < len(self.image_paths) else "",
                               self.texts[i] if i < len(self.texts) else "")) for i in range(self.num_items)]
            return torch.tensor(keep, dtype=torch.bool)
        return allow

    def group_ids(self, group_by) -> torch.Tensor:
        """int64 group ids [num_items] (CPU) from a group_by= argument: "image_path" or "text" -- rows
        with equal metadata form a group, a row without that entry is a group of its own --, a callable
        (i, image_path, text) -> hashable key, or an int sequence / tensor [num_items] taken as the
        ids themselves. Keys map to dense ids by first occurrence (group_ids_from_keys)."""
        n = self.num_items
        if isinstance(group_by, str):
            if group_by not in ("image_path", "text"):
                raise ValueError(f'group_by must be "image_path", "text", a callable or group ids, got {group_by!r}')
            meta = self.image_paths if group_by == "image_path" else self.texts
            return group_ids_from_keys([("key", meta[i]) if i < len(meta) else ("row", i) for i in range(n)])
        if callable(group_by):
            return group_ids_from_keys([group_by(i, self.image_paths[i] if i < len(self.image_paths) else "",
                                                 self.texts[i] if i < len(self.texts) else "") for i in range(n)])
        return torch.as_tensor(group_by)   # CosineIndex.group_plan validates length, dtype and sign

    def key_values(self, keys):
        """the per-row values of a keys= argument: a KeyPlan or values [num_items] as they are, or a
        callable (i, image_path, text) -> number evaluated over the host metadata"""
        if callable(keys):
            return torch.tensor([keys(i, self.image_paths[i] if i < len(self.image_paths) else "",
                                      self.texts[i] if i < len(self.texts) else "") for i in range(self.num_items)])
        return keys

    def search_batch(self, queries, top_k: int = 5, allow=None, group_by=None, keys=None, lo=None, hi=None):
        """[nq, d] queries -> (scores [nq, k], indices [nq, k]) on the GPU, k = min(top_k, num_items).
        allow: only these rows compete (see _allow); slots past their number hold (-inf, -1).
        keys (see key_values) with lo / hi: one inclusive value range per query -- row j competes for
        query i iff lo[i] <= keys[j] <= hi[i] (CosineIndex.search_where; top_k <= 1024, not with group_by).
        group_by (see group_ids; or a CosineIndex.group_plan(), which holds its own filter): at most one
        row per group, its best -- (scores, indices, group ids), (-inf, -1, -1) past the number of
        distinct allowed groups (CosineIndex.search_grouped; top_k <= 1024)."""
        k = min(int(top_k), self.num_items)
        if k < 0:
            raise RuntimeError("selected index k out of range")
        if k == 0:
            q = torch.as_tensor(queries)
            nq = 1 if q.dim() == 1 else q.shape[0]
            empty = (torch.empty((nq, 0)), torch.empty((nq, 0), dtype=torch.int64))
            return empty if group_by is None else empty + (torch.empty((nq, 0), dtype=torch.int64),)
        if keys is not None:
            if group_by is not None:
                raise ValueError("search_batch: keys= and group_by= do not combine")
            return self._gpu.search_where(queries, k, self.key_values(keys), lo, hi,
                                          allow=None if allow is None else self._allow(allow))
        if group_by is not None:
            groups = group_by if isinstance(group_by, GroupPlan) else self.group_ids(group_by)
            return self._gpu.search_grouped(queries, k, groups, allow=None if allow is None else self._allow(allow))
        if allow is not None:
            return self._gpu.search(queries, k, allow=self._allow(allow))
        return self._gpu.search(queries, k)

    def search_with_embedding(self, query_emb: torch.Tensor, top_k: int = 5, allow=None,
                              group_by=None) -> List[SearchResult]:
        """query_emb: shape (d,) atau (1, d). allow: a row filter (search_batch); fewer than top_k
        results when fewer rows are allowed. group_by (search_batch): at most one SearchResult per
        group, the group's best row; fewer than top_k when fewer groups compete."""
        query_emb = torch.as_tensor(query_emb)
        if query_emb.ndim == 1:
            query_emb = query_emb.unsqueeze(0)
        elif query_emb.ndim != 2 or query_emb.shape[0] != 1:
            raise ValueError(f"query_emb must be shape (d,) or (1, d), got {tuple(query_emb.shape)}")
        if query_emb.shape[-1] != self.dim:
            raise ValueError(f"query_emb dim {query_emb.shape[-1]} != index dim {self.dim}")
        if group_by is not None:
            scores, indices, _ = self.search_batch(query_emb, top_k, allow=allow, group_by=group_by)
        elif allow is None:   # today's call, untouched
            scores, indices = self.search_batch(query_emb, top_k)
        else:
            scores, indices = self.search_batch(query_emb, top_k, allow=allow)
        results: List[SearchResult] = []
        for idx, score in zip(indices[0].tolist(), scores[0].tolist()):
            if (allow is not None or group_by is not None) and idx < 0:   # the pad of a short list
                continue
            # an index outside [0, len) has no metadata: the (-inf, -1) pad of a short result must
            # not read the last item's through Python's negative indexing
            img = self.image_paths[idx] if 0 <= idx < len(self.image_paths) else ""
            txt = self.texts[idx] if 0 <= idx < len(self.texts) else ""
            results.append(SearchResult(index=idx, score=float(score), image_path=img, text=txt))
        return results

    def search_by_text(self, query, model, processor, device, top_k: int = 5, allow=None,
                       group_by=None) -> List[SearchResult]:
        from .clip_model import encode_text
        emb = encode_text(query, model, processor, device)
        if group_by is None:
            return self.search_with_embedding(emb, top_k=top_k, allow=allow)
        return self.search_with_embedding(emb, top_k=top_k, allow=allow, group_by=group_by)

    def search_by_image(self, image_path, model, processor, device, top_k: int = 5, allow=None,
                        group_by=None) -> List[SearchResult]:
        from .clip_model import encode_image
        emb = encode_image(image_path, model, processor, device)
        if group_by is None:
            return self.search_with_embedding(emb, top_k=top_k, allow=allow)
        return self.search_with_embedding(emb, top_k=top_k, allow=allow, group_by=group_by)

    def search_above_with_embedding(self, query_emb: torch.Tensor, threshold: float) -> List[SearchResult]:
        """Every item whose cosine with the query is >= threshold (CosineIndex.search_above), best
        first; query_emb: shape (d,) or (1, d), metadata looked up as search_with_embedding does."""
        query_emb = torch.as_tensor(query_emb)
        if query_emb.ndim == 1:
            query_emb = query_emb.unsqueeze(0)
        elif query_emb.ndim != 2 or query_emb.shape[0] != 1:
            raise ValueError(f"query_emb must be shape (d,) or (1, d), got {tuple(query_emb.shape)}")
        if query_emb.shape[-1] != self.dim:
            raise ValueError(f"query_emb dim {query_emb.shape[-1]} != index dim {self.dim}")
        if self.num_items == 0:
            return []
        _, scores, indices = self._gpu.search_above(query_emb, float(threshold))
        results: List[SearchResult] = []
        for idx, score in zip(indices.tolist(), scores.tolist()):
            img = self.image_paths[idx] if 0 <= idx < len(self.image_paths) else ""
            txt = self.texts[idx] if 0 <= idx < len(self.texts) else ""
            results.append(SearchResult(index=idx, score=float(score), image_path=img, text=txt))
        return results

    def search_above_by_text(self, query, model, processor, device, threshold: float) -> List[SearchResult]:
        from .clip_model import encode_text
        return self.search_above_with_embedding(encode_text(query, model, processor, device), threshold)

    def search_above_by_image(self, image_path, model, processor, device, threshold: float) -> List[SearchResult]:
        from .clip_model import encode_image
        return self.search_above_with_embedding(encode_image(image_path, model, processor, device), threshold)

    # ------------------------------------------------------- resident append --
    def append(self, embeddings, image_paths: Sequence[str] = (), texts: Sequence[str] = ()) -> None:
        """Add rows (re-normalised in fp32, as finder_service.py:169 does) and their metadata:
        amortised O(1) per row on the host and in HBM."""
        e = torch.as_tensor(embeddings).float().cpu()
        if e.dim() == 1:
            e = e.unsqueeze(0)
        if e.dim() != 2 or e.shape[1] != self.dim:
            raise ValueError(f"embedding dim {e.shape[-1]} != index dim {self.dim}")
        e = e / e.norm(dim=-1, keepdim=True)
        if self._host is None:
            self.embeddings   # noqa: B018 -- materialise the host mirror before growing it
        n_new = self._n + e.shape[0]
        if n_new > self._host.shape[0]:
            cap = max(n_new, 2 * self._host.shape[0], 1024)
            buf = torch.empty((cap, self.dim), dtype=torch.float32)
            buf[: self._n] = self._host[: self._n]
            self._host = buf
        self._host[self._n: n_new] = e
        self._gpu.append(e)
        self._n = n_new
        self.image_paths.extend(image_paths)
        self.texts.extend(texts)
        self.num_items = n_new

    # ------------------------------------------------------ resident mutation --
    def _positions(self, indices) -> List[int]:
        pos = [int(i) for i in torch.as_tensor(indices, dtype=torch.int64).reshape(-1).tolist()]
        for p in pos:
            if not 0 <= p < self.num_items:
                raise ValueError(f"index {p} is outside [0, {self.num_items})")
        return pos

    def remove(self, indices) -> int:
        """Remove the items at these positions (any order, a duplicate counts once) from the HBM
        index, the host mirror and the metadata; returns the number removed. The items above a
        removed one move down by one position each, keeping their order (the reference's .pt is
        positional: row i, image_paths[i], texts[i]). image_paths / texts may be shorter than the
        index (search.py:103-105): entries are deleted only where the list has that position. An
        index wrapped by from_gpu_index whose host mirror was never read stays that way."""
        gone = sorted(set(self._positions(indices)))
        if not gone:
            return 0
        self._gpu.remove(gone)
        n_new = self._n - len(gone)
        if self._host is not None:
            keep = torch.ones(self._n, dtype=torch.bool)
            keep[gone] = False
            first = gone[0]   # rows below the first removed one stay where they are
            self._host[first: n_new] = self._host[first: self._n][keep[first:]]
        for lst in (self.image_paths, self.texts):
            for p in reversed(gone):
                if p < len(lst):
                    del lst[p]
        self._n = self.num_items = n_new
        return len(gone)

    def update(self, indices, embeddings, image_paths: Optional[Sequence[str]] = None,
               texts: Optional[Sequence[str]] = None) -> None:
        """Replace the rows at these (distinct) positions by `embeddings`, re-normalised in fp32 as
        `append` does, in HBM and in the host mirror; image_paths / texts, when given, replace the
        items' metadata where the list is long enough to have that position."""
        pos = self._positions(indices)
        if len(set(pos)) != len(pos):
            raise ValueError("duplicate index in update")
        e = torch.as_tensor(embeddings).float().cpu()
        if e.dim() == 1:
            e = e.unsqueeze(0)
        if e.dim() != 2 or e.shape[1] != self.dim:
            raise ValueError(f"embedding dim {e.shape[-1]} != index dim {self.dim}")
        if e.shape[0] != len(pos):
            raise ValueError(f"{len(pos)} indices vs {e.shape[0]} embeddings")
        for name, new in (("image_paths", image_paths), ("texts", texts)):
            if new is not None and len(new) != len(pos):
                raise ValueError(f"{len(pos)} indices vs {len(new)} {name}")
        if not pos:
            return
        e = e / e.norm(dim=-1, keepdim=True)
        self._gpu.update(pos, e)
        if self._host is not None:
            self._host[torch.tensor(pos)] = e
        for lst, new in ((self.image_paths, image_paths), (self.texts, texts)):
            if new is not None:
                for p, v in zip(pos, new):
                    if p < len(lst):
                        lst[p] = v

    def save(self, path: Union[str, Path]) -> None:
        """The reference .pt format ({"embeddings": [N, D] f32, "image_paths", "texts"},
        finder_service.py:93-103), written to a temporary file and renamed into place."""
        path = Path(path)
        path.parent.mkdir(parents=True, exist_ok=True)
        tmp = path.with_name(path.name + ".tmp")
        torch.save({"embeddings": self.embeddings.clone(), "image_paths": list(self.image_paths),
                    "texts": list(self.texts)}, tmp)
        tmp.replace(path)

    # ------------------------------------------------------------ shard file --
    def save_shard(self, path: Union[str, Path]) -> None:
        """The HBM index as a raw shard (CosineIndex.save_shard) with this index's metadata; the
        reference .pt stays available through .save."""
        self._gpu.save_shard(path, meta={"image_paths": [str(p) for p in self.image_paths],
                                         "texts": [str(t) for t in self.texts]})

    @classmethod
    def load_shard(cls, path: Union[str, Path], device=None) -> "TextSearchIndex":
        """Reload a save_shard file straight into HBM (no torch.load, no re-normalisation): the
        same rows, metadata and search results, bit for bit, as the index that was saved."""
        gpu, header = CosineIndex.load_shard(path, device=device, capacity=max(header_n(path), 1024))
        self = cls.__new__(cls)
        n, dim, dim_p = header["n"], header["dim"], header["dim_p"]
        _, secs = read_shard_header(path)
        if n == 0:   # an empty index has no data sections to map (mmap refuses 0 bytes at EOF)
            host = torch.empty((0, dim), dtype=torch.float32)
        else:
            if header["has_f32"]:   # the host mirror: the fp32 rows, paged in lazily (copy-on-write map)
                host = np.memmap(path, dtype=np.float32, mode="c", offset=secs["rows32"][0], shape=(n, dim_p))
            else:
                host = np.memmap(path, dtype=np.float16, mode="r", offset=secs["rows16"][0], shape=(n, dim_p))
            host = torch.from_numpy(np.ascontiguousarray(host[:, :dim]) if dim != dim_p or not header["has_f32"]
                                    else host).float()
        self._host, self._n = host, n
        self.image_paths = list(header["meta"].get("image_paths", []))
        self.texts = list(header["meta"].get("texts", []))
        self.num_items, self.dim = n, dim
        self._gpu = gpu
        print(f"[TextSearchIndex] Loaded {n} items with dim={dim} (shard)")
        return self


def header_n(path) -> int:
    return read_shard_header(path)[0]["n"]
