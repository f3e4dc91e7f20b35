"""CPU restatement of the keyed search (CosineIndex.search_where, clm_index_search_keyed) for the tests.

    result(q_i) = mask_ref.masked_topk(q_i, mask_i),  mask_i = { j : keep[j] and lo[i] <= value[j] <= hi[i] }

The yardstick is mask_ref.masked_topk itself, applied query by query with that query's mask; nothing here
orders or scores anything. `open_rows` states the predicate on the VALUES in float64 (the tests' values
and bounds are integers or halves, exact there), so key_ranks / key_bounds are checked against it and
not against themselves. `ranges` builds the mixed batch of range kinds the tests share; `TorchIndex` is
the CPU stand-in of the collective test.
"""
import numpy as np
import torch

import mask_ref as M


def _side(b, nq, open_value):
    if b is None:
        return np.full((nq,), open_value, np.float64)
    a = np.asarray(torch.as_tensor(b).cpu().numpy(), dtype=np.float64).reshape(-1)
    return np.broadcast_to(a, (nq,)).copy() if a.size == 1 else a


def open_rows(values, lo, hi, nq, keep=None):
    """bool [nq, N] (numpy): row j is open to query i"""
    v = np.asarray(torch.as_tensor(values).cpu().numpy(), dtype=np.float64).reshape(-1)
    lo, hi = _side(lo, nq, -np.inf), _side(hi, nq, np.inf)
    assert lo.size == nq and hi.size == nq
    m = (v[None, :] >= lo[:, None]) & (v[None, :] <= hi[:, None])
    if keep is not None:
        m &= np.asarray(torch.as_tensor(keep).cpu().numpy(), dtype=bool).reshape(1, -1)
    return m


def keyed_topk(S, open_, k, offset=0):
    """masked_topk query by query: (scores [nq, k] f32, ids [nq, k] i64)"""
    S = torch.as_tensor(S).detach().cpu().to(torch.float32)
    parts = [M.masked_topk(S[i: i + 1], open_[i], k, offset) for i in range(S.shape[0])]
    if not parts:
        return torch.empty((0, k)), torch.empty((0, k), dtype=torch.int64)
    return torch.cat([p[0] for p in parts], 0), torch.cat([p[1] for p in parts], 0)


def exact_count_range(allowed_values, c):
    """an inclusive (lo, hi) holding exactly c >= 1 of the values, or None where ties leave none"""
    v = np.sort(np.asarray(allowed_values, dtype=np.float64))
    for a in range(0, v.size - c + 1):
        if (a == 0 or v[a - 1] < v[a]) and (a + c == v.size or v[a + c] > v[a + c - 1]):
            return float(v[a]), float(v[a + c - 1])
    return None


KINDS = ("all", "empty", "one_key", "half_open", "no_row", "one_row", "k_minus_1")


def ranges(values, keep, nq, k, seed):
    """float64 (lo [nq], hi [nq], kind names [nq]): the kinds cycle through the batch. `one_row` /
    `k_minus_1` hold exactly 1 / k - 1 allowed rows where the values have such a range (else one key /
    no row); `no_row` alternates a gap between two values with a range above them all."""
    v = np.asarray(torch.as_tensor(values).cpu().numpy(), dtype=np.float64).reshape(-1)
    va = v if keep is None else v[np.asarray(torch.as_tensor(keep).cpu().numpy(), dtype=bool)]
    rng = np.random.default_rng(seed)
    lo, hi, kinds = np.empty(nq), np.empty(nq), []
    top = v.max() if v.size else 0.0
    one_row, k_minus_1 = exact_count_range(va, 1), exact_count_range(va, k - 1) if k > 1 else None
    for i in range(nq):
        kind = KINDS[i % len(KINDS)]
        pick = float(v[rng.integers(v.size)])
        if kind == "k_minus_1":
            kind, r = ("k_minus_1", k_minus_1) if k_minus_1 else ("no_row", None)
        if kind == "one_row":
            kind, r = ("one_row", one_row) if one_row else ("one_key", None)
        if kind == "all":
            r = (-np.inf, np.inf)
        elif kind == "empty":
            r = (pick + 1.0, pick - 1.0)
        elif kind == "one_key":
            r = (pick, pick)
        elif kind == "half_open":
            r = (float(np.median(v)), np.inf) if (i // len(KINDS)) % 2 == 0 else (-np.inf, float(np.median(v)))
        elif kind == "no_row":
            r = (pick + 0.25, pick + 0.75) if (i // len(KINDS)) % 2 == 0 else (top + 1.0, top + 5.0)
        lo[i], hi[i] = r
        kinds.append(kind)
    return torch.from_numpy(lo), torch.from_numpy(hi), kinds


class TorchIndex(M.TorchIndex):
    """mask_ref's CPU stand-in for CosineIndex plus search_where(q, k, plan, lo, hi): the plan's keys
    against the bounds key_bounds makes of its uniq / cum, then the yardstick"""

    def search_where(self, queries, k, plan, lo, hi, allow=None, route=0):
        from clip_lora_match_amd.search import key_bounds
        if len(self) == 0:
            raise ValueError("search_where: the index is empty")
        assert allow is None and plan.n == len(self)
        q = torch.as_tensor(queries).float()
        q = q.unsqueeze(0) if q.dim() == 1 else q
        klo, khi, n_in = key_bounds(plan.uniq, plan.cum, lo, hi, q.shape[0])
        keys = plan.keys.numpy()
        op = (keys[None, :] >= klo.numpy()[:, None]) & (keys[None, :] <= khi.numpy()[:, None])
        assert np.array_equal(op.sum(1), n_in.numpy())
        return keyed_topk(M.cosines(q, self.rows), op, k, self._offset)
