"""CPU restatement of the filtered search (CosineIndex.search(allow=), clm_index_search_masked) for
the tests: the rule and the order, from a score matrix.

    result(q) = the first k of { j : allow[j] } ordered (NaN first, score desc, id asc),
                padded with (-inf, -1)

`masked_topk` takes the scores as given (the GPU tests pass cosine_similarity()'s, the routine every
exact score comes from, so the comparison is bitwise); `pack` restates the mask layout; `TorchIndex`
is a CPU stand-in for CosineIndex with float64 cosines rounded once to fp32, for the collective
plumbing (the route tests/range_ref.py takes).
"""
import numpy as np
import torch


def pack(allow):
    """bool [N] -> ceil(N / 32) little-endian uint32 words (numpy): bit j & 31 of word j >> 5 = allow[j]"""
    a = np.asarray(allow, dtype=bool).reshape(-1)
    nw = (a.size + 31) // 32
    bits = np.zeros((nw * 32,), np.uint64)
    bits[: a.size] = a
    return (bits.reshape(nw, 32) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)


def masked_topk(S, allow_bool, k, offset=0):
    """(scores [nq, k] f32, ids [nq, k] i64) (CPU tensors) from S [nq, N] f32"""
    S = torch.as_tensor(S).detach().cpu().to(torch.float32).numpy()
    allow = np.asarray(torch.as_tensor(allow_bool).cpu().numpy(), dtype=bool).reshape(-1)
    nq, N = S.shape
    assert allow.size == N
    cols = np.nonzero(allow)[0]
    out_s = np.full((nq, k), -np.inf, np.float32)
    out_i = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        v = S[q, cols]
        vn = np.isnan(v)
        order = np.lexsort((cols, np.where(vn, 0.0, -v.astype(np.float64)), ~vn))[:k]   # NaN first, score desc, id asc
        out_s[q, : order.size] = v[order]
        out_i[q, : order.size] = cols[order] + offset
    return torch.from_numpy(out_s), torch.from_numpy(out_i)


def same(got, want):
    """equality of two (scores, ids) pairs: ids equal, scores by their bits, a NaN matching any NaN"""
    gs, ws = got[0].cpu(), want[0].cpu()
    if gs.shape != ws.shape or not torch.equal(got[1].cpu(), want[1].cpu()):
        return False
    nan = torch.isnan(ws)
    return torch.equal(torch.isnan(gs), nan) and torch.equal(gs[~nan].view(torch.int32), ws[~nan].view(torch.int32))


def cosines(q, rows):
    """float64 cosines rounded once to fp32 (CPU)"""
    q, rows = torch.as_tensor(q).double(), torch.as_tensor(rows).double()
    return ((q @ rows.T) / (q.norm(dim=1)[:, None] * rows.norm(dim=1)[None, :])).float()


def merge(s_all, i_all, parts, k):
    """CPU merge of `parts` lists per row by (NaN first, score desc, id asc); id < 0 = an empty slot"""
    s, i = s_all.numpy(), i_all.numpy()
    out_s = np.full((s.shape[0], k), -np.inf, np.float32)
    out_i = np.full((s.shape[0], k), -1, np.int64)
    for q in range(s.shape[0]):
        live = np.nonzero(i[q] >= 0)[0]
        v, g = s[q, live], i[q, live]
        vn = np.isnan(v)
        order = np.lexsort((g, np.where(vn, 0.0, -v.astype(np.float64)), ~vn))[:k]
        out_s[q, : order.size], out_i[q, : order.size] = v[order], g[order]
    return torch.from_numpy(out_s), torch.from_numpy(out_i)


class TorchIndex:
    """stand-in for CosineIndex on the CPU: append / set_offset / len / search(q, k, allow=)"""

    def __init__(self, dim):
        self.rows, self._offset, self.device = torch.empty((0, dim)), 0, torch.device("cpu")

    def __len__(self):
        return self.rows.shape[0]

    def set_offset(self, off):
        self._offset = int(off)

    def append(self, rows):
        self.rows = torch.cat([self.rows, torch.as_tensor(rows).float()], 0)

    def search(self, queries, k, allow=None, route=0):
        q = torch.as_tensor(queries).float()
        q = q.unsqueeze(0) if q.dim() == 1 else q
        keep = np.ones((len(self),), bool) if allow is None else torch.as_tensor(allow).numpy().astype(bool)
        return masked_topk(cosines(q, self.rows), keep, k, self._offset)
