"""CPU restatement of the grouped search (CosineIndex.search_grouped, clm_topk_distinct) for the tests:
the rule and the order, from a score matrix.

    walk the allowed rows ordered (NaN first, score desc, id asc); keep a row iff no earlier row of the
    walk belongs to its group; result(q) = the first k kept rows as (score, id, gid), padded with
    (-inf, -1, -1)

`grouped_topk` takes the scores as given (the GPU tests pass cosine_similarity()'s, the routine every
exact score comes from, so the comparison is bitwise); `distinct_lists` restates clm_topk_distinct on
explicit lists; `merge_grouped` is the CPU merge of shard lists; `TorchIndex` is a CPU stand-in for
CosineIndex with float64 cosines rounded once to fp32, for the collective plumbing (the route
tests/mask_ref.py takes).
"""
import numpy as np
import torch

import mask_ref


def order_of(v, ids):
    """positions of (scores v, ids) sorted by (NaN first, score desc, id asc)"""
    vn = np.isnan(v)
    return np.lexsort((ids, np.where(vn, 0.0, -v.astype(np.float64)), ~vn))


def first_distinct(v, ids, gids, k):
    """the first k entries of an ORDERED list that open a new group; id < 0 entries are skipped"""
    out_s = np.full((k,), -np.inf, np.float32)
    out_i = np.full((k,), -1, np.int64)
    out_g = np.full((k,), -1, np.int64)
    seen, n = set(), 0
    for s, i, g in zip(v.tolist(), ids.tolist(), gids.tolist()):
        if n == k:
            break
        if i < 0 or g in seen:
            continue
        seen.add(g)
        out_s[n], out_i[n], out_g[n] = np.float32(s), i, g
        n += 1
    return out_s, out_i, out_g, n


def grouped_topk(S, groups, k, allow=None, offset=0):
    """(scores [nq, k] f32, ids [nq, k] i64, gids [nq, k] i64) (CPU tensors) from S [nq, N] f32"""
    S = torch.as_tensor(S).detach().cpu().to(torch.float32).numpy()
    groups = np.asarray(torch.as_tensor(groups).cpu().numpy(), dtype=np.int64).reshape(-1)
    nq, N = S.shape
    assert groups.size == N
    allow = np.ones((N,), bool) if allow is None else \
        np.asarray(torch.as_tensor(allow).cpu().numpy(), dtype=bool).reshape(-1)
    assert allow.size == N
    cols = np.nonzero(allow)[0]
    out = [np.empty((nq, k), np.float32), np.empty((nq, k), np.int64), np.empty((nq, k), np.int64)]
    for q in range(nq):
        v = S[q, cols]
        o = order_of(v, cols)
        out[0][q], out[1][q], out[2][q], _ = first_distinct(v[o], cols[o] + offset, groups[cols[o]], k)
    return tuple(torch.from_numpy(a) for a in out)


def distinct_lists(scores, ids, gids, offsets, k):
    """clm_topk_distinct on ragged lists (numpy 1-D arrays + offsets [nq + 1]): (s, i, g [nq, k], found [nq])"""
    nq = len(offsets) - 1
    out = [np.empty((nq, k), np.float32), np.empty((nq, k), np.int64), np.empty((nq, k), np.int64),
           np.empty((nq,), np.int32)]
    for q in range(nq):
        a, b = int(offsets[q]), int(offsets[q + 1])
        out[0][q], out[1][q], out[2][q], out[3][q] = first_distinct(scores[a:b], ids[a:b], gids[a:b], k)
    return tuple(torch.from_numpy(a) for a in out)


def same(got, want):
    """equality of two (scores, ids, gids) triples: ids and gids equal, scores by their bits, NaN = NaN"""
    return mask_ref.same(got[:2], want[:2]) and torch.equal(got[2].cpu(), want[2].cpu())


def merge_grouped(s_all, i_all, g_all, parts, k):
    """CPU merge of `parts` grouped lists per row: ordered (NaN first, score desc, id asc), then the
    first k distinct groups; id < 0 = an empty slot"""
    s, i, g = (torch.as_tensor(t).cpu().numpy() for t in (s_all, i_all, g_all))
    nq = s.shape[0]
    out = [np.empty((nq, k), np.float32), np.empty((nq, k), np.int64), np.empty((nq, k), np.int64)]
    for q in range(nq):
        live = np.nonzero(i[q] >= 0)[0]
        o = live[order_of(s[q, live], i[q, live])]
        out[0][q], out[1][q], out[2][q], _ = first_distinct(s[q, o], i[q, o], g[q, o], k)
    return tuple(torch.from_numpy(a) for a in out)


class TorchIndex(mask_ref.TorchIndex):
    """mask_ref's CPU stand-in for CosineIndex plus search_grouped(q, k, groups, allow=)"""

    def search_grouped(self, queries, k, groups, allow=None, route=0):
        if len(self) == 0:
            raise ValueError("search_grouped: the index is empty")
        q = torch.as_tensor(queries).float()
        q = q.unsqueeze(0) if q.dim() == 1 else q
        return grouped_topk(mask_ref.cosines(q, self.rows), groups, k, allow, self._offset)
