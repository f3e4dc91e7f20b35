"""Generate tests/golden/threshold_metrics.npz: inputs and outputs of the reference's threshold
evaluator (scripts/evaluate.py:33-99,141-168,221-267), run where the read-only reference exists:

  python tests/golden/make_threshold_golden.py [REFERENCE_ROOT]      (or $CLM_REFERENCE_ROOT)

Per query the reference's own evaluate_single_query gives the relevant set (cosine >= threshold)
and the ranking, its calculate_recall_at_k / _precision_at_k / _mrr / _average_precision the
per-query metrics; the means are taken as evaluate_epoch takes them (:262-265). evaluate.py imports
pandas, tqdm and the model loader at module level; whatever is missing is stubbed in sys.modules
for the import, as make_eval_golden.py does -- none of it is reached by these functions.

Fixture: 60 cluster centres at 64 dims; the index holds 30 / 15 / 10 / 5 clusters of 1 / 3 / 12 / 20
rows `centre + 0.25 noise` plus 100 unrelated rows (395 rows); the queries are `centre + c noise`,
c spread over [0.2, 1.6], one per cluster, plus 4 unrelated ones. The relevant-set sizes then
spread from 0 over 1 and a few to more than 10: every branch of the metrics is reached (an empty
set; more relevant rows than k).

Stored: queries, index, threshold, k_values, relevant_offsets (CSR) with relevant_ids (ascending
within a query: the reference orders near-equal fp32 scores its own way) and relevant_scores (the
reference's fp32 cosines, same order), the per-query metrics, their means, and min_gap.

Membership must not depend on fp32 rounding: the generator checks in fp64 that no score lies
within 1e-5 of the threshold and refuses to write otherwise. The tests then exclude nothing.
"""
from __future__ import annotations

import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
K_VALUES = [1, 5, 10]
THRESHOLD = 0.7
MIN_GAP = 1e-5


def _load_reference(root):
    stubs = {}
    for name in ("pandas", "tqdm", "models", "models.clip_model"):
        try:
            importlib.import_module(name)
        except Exception:
            stubs[name] = types.ModuleType(name)
    for name, mod in stubs.items():
        mod.__path__ = []
        sys.modules[name] = mod
    if "tqdm" in stubs:
        stubs["tqdm"].tqdm = lambda it, **kw: it
    if "models.clip_model" in stubs:
        for fn in ("load_clip_model", "encode_text"):
            setattr(stubs["models.clip_model"], fn, None)
    try:
        spec = importlib.util.spec_from_file_location("ref_evaluate", os.path.join(root, "scripts/evaluate.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for name in stubs:
            sys.modules.pop(name, None)
    return mod


def fixture(seed=0):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((60, 64))
    sizes = [1] * 30 + [3] * 15 + [12] * 10 + [20] * 5
    rows = [centres[c] + 0.25 * rng.standard_normal((n, 64)) for c, n in enumerate(sizes)]
    rows.append(rng.standard_normal((100, 64)))
    index = np.concatenate(rows, 0)
    index = index[rng.permutation(index.shape[0])].astype(np.float32)
    c = np.linspace(0.2, 1.6, 60)[rng.permutation(60)]
    queries = np.concatenate([centres + c[:, None] * rng.standard_normal((60, 64)), rng.standard_normal((4, 64))], 0)
    return queries.astype(np.float32), index


def min_gap(queries, index, threshold):
    q = queries.astype(np.float64)
    x = index.astype(np.float64)
    s = (q / np.linalg.norm(q, axis=1, keepdims=True)) @ (x / np.linalg.norm(x, axis=1, keepdims=True)).T
    return float(np.abs(s - threshold).min())


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CLM_REFERENCE_ROOT")
    if not root:
        raise SystemExit("give the reference's root directory (argument or $CLM_REFERENCE_ROOT)")
    ref = _load_reference(root)
    queries, index = fixture()
    gap = min_gap(queries, index, THRESHOLD)
    if not gap > MIN_GAP:
        raise SystemExit(f"a score lies within {gap:.3e} of the threshold: membership would depend on fp32 rounding")
    tq, tx = torch.from_numpy(queries), torch.from_numpy(index)
    tx = tx / tx.norm(dim=-1, keepdim=True)           # build_index_from_train, evaluate.py:132
    idx = {"embeddings": tx}
    off, ids, scores = [0], [], []
    rec = {k: [] for k in K_VALUES}
    prec = {k: [] for k in K_VALUES}
    rr, ap = [], []
    for i in range(queries.shape[0]):
        relevant, sorted_scores, ranking = ref.evaluate_single_query("", tq[i], idx, THRESHOLD)
        for k in K_VALUES:
            rec[k].append(ref.calculate_recall_at_k(relevant, ranking, k))
            prec[k].append(ref.calculate_precision_at_k(relevant, ranking, k))
        rr.append(ref.calculate_mrr(relevant, ranking))
        ap.append(ref.calculate_average_precision(relevant, ranking))
        by_id = dict(zip(ranking, sorted_scores))
        rel = sorted(relevant)
        ids += rel
        scores += [by_id[j] for j in rel]
        off.append(len(ids))
    out = {
        "queries": queries, "index": index, "threshold": np.float64(THRESHOLD), "k_values": np.asarray(K_VALUES, np.int64),
        "relevant_offsets": np.asarray(off, np.int64), "relevant_ids": np.asarray(ids, np.int64),
        "relevant_scores": np.asarray(scores, np.float32),
        "q_recall": np.asarray([rec[k] for k in K_VALUES], np.float64),
        "q_precision": np.asarray([prec[k] for k in K_VALUES], np.float64),
        "q_rr": np.asarray(rr, np.float64), "q_ap": np.asarray(ap, np.float64),
        # evaluate_epoch's aggregation, evaluate.py:262-265
        "recall": np.asarray([np.mean(rec[k]) * 100 for k in K_VALUES], np.float64),
        "precision": np.asarray([np.mean(prec[k]) * 100 for k in K_VALUES], np.float64),
        "mrr": np.float64(np.mean(rr)), "map": np.float64(np.mean(ap)), "min_gap": np.float64(gap),
    }
    np.savez_compressed(os.path.join(HERE, "threshold_metrics.npz"), **out)
    sizes = np.diff(out["relevant_offsets"])
    print(f"threshold_metrics.npz: min gap {gap:.3e}; relevant-set sizes: 0 x{(sizes == 0).sum()}, 1 x{(sizes == 1).sum()}, "
          f"2-10 x{((sizes >= 2) & (sizes <= 10)).sum()}, >10 x{(sizes > 10).sum()} (max {sizes.max()}); "
          f"recall {out['recall']}, precision {out['precision']}, mrr {out['mrr']:.4f}, map {out['map']:.4f}")


if __name__ == "__main__":
    main()
