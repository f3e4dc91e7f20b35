"""CPU restatement of the threshold search (CosineIndex.search_above, clm_index_search_above) for
the tests: the rule, the order and the CSR layout, from a score matrix.

    result(q) = { j : S[q, j] >= tau[q]  or  S[q, j] is NaN }     ordered (score desc, id asc),
                                                                 NaN above every number

`above_from_scores` takes the scores as given (the GPU tests pass cosine_similarity()'s, the
routine every exact score comes from, so the comparison is bitwise); `TorchIndex` is a CPU stand-in
for CosineIndex with float64 cosines rounded once to fp32, for the collective plumbing.
"""
import numpy as np
import torch


def thresholds(threshold, nq):
    t = torch.as_tensor(threshold, dtype=torch.float32).reshape(-1)
    return t.expand(nq).clone() if t.numel() == 1 and nq != 1 else t


def above_from_scores(S, threshold, offset=0):
    """(offsets [nq + 1] i64, scores [total] f32, ids [total] i64) from S [nq, N] f32 (CPU)"""
    S = torch.as_tensor(S).detach().cpu().to(torch.float32)
    nq, N = S.shape
    tau = thresholds(threshold, nq).numpy()
    s = S.numpy()
    off = np.zeros((nq + 1,), np.int64)
    sc, ix = [], []
    for q in range(nq):
        row = s[q]
        nan = np.isnan(row)
        with np.errstate(invalid="ignore"):
            keep = np.nonzero(nan | (row >= tau[q]))[0]
        v = row[keep]
        vn = np.isnan(v)
        order = np.lexsort((keep, np.where(vn, 0.0, -v.astype(np.float64)), ~vn))   # NaN first, score desc, id asc
        sc.append(v[order])
        ix.append(keep[order].astype(np.int64) + offset)
        off[q + 1] = off[q] + keep.size
    return (torch.from_numpy(off), torch.from_numpy(np.concatenate(sc) if sc else np.zeros((0,), np.float32)),
            torch.from_numpy(np.concatenate(ix) if ix else np.zeros((0,), np.int64)))


def same(got, want):
    """equality of two (offsets, scores, ids) triples: scores by their bits, a NaN matching any NaN
    (the library returns NaN scores with the sign bit cleared)"""
    gs, ws = got[1].cpu(), want[1].cpu()
    if not (torch.equal(got[0].cpu(), want[0].cpu()) and torch.equal(got[2].cpu(), want[2].cpu())):
        return False
    nan = torch.isnan(ws)
    return torch.equal(torch.isnan(gs), nan) and torch.equal(gs[~nan].view(torch.int32), ws[~nan].view(torch.int32))


def cosines(q, rows):
    """float64 cosines rounded once to fp32 (CPU)"""
    q, rows = torch.as_tensor(q).double(), torch.as_tensor(rows).double()
    return ((q @ rows.T) / (q.norm(dim=1)[:, None] * rows.norm(dim=1)[None, :])).float()


class TorchIndex:
    """stand-in for CosineIndex on the CPU: append / set_offset / len / search_above"""

    def __init__(self, dim):
        self.rows, self.offset, self.device = torch.empty((0, dim)), 0, torch.device("cpu")

    def __len__(self):
        return self.rows.shape[0]

    def set_offset(self, off):
        self.offset = int(off)

    def append(self, rows):
        self.rows = torch.cat([self.rows, torch.as_tensor(rows).float()], 0)

    def search_above(self, queries, threshold, band_cap=0):
        q = torch.as_tensor(queries).float()
        q = q.unsqueeze(0) if q.dim() == 1 else q
        if len(self) == 0:
            return torch.zeros((q.shape[0] + 1,), dtype=torch.int64), torch.empty((0,)), torch.empty((0,), dtype=torch.int64)
        return above_from_scores(cosines(q, self.rows), threshold, self.offset)
