"""Generate tests/golden/eval_metrics.npz: inputs and outputs of the reference's own
CLIPEvaluator.compute_recall_at_k / compute_mrr / compute_map (scripts/evaluate_model.py:38-107),
run in the build container where the read-only reference exists (as make_golden.py):

  python tests/golden/make_eval_golden.py

The three methods never touch `self`, so they are called unbound (self=None) on
sims = A_hat @ B_hat^T (image -> text) and on its transpose (text -> image), exactly the matrices
evaluate_retrieval builds (:183-188,206). evaluate_model.py imports pandas, tqdm and the model
loader at module level; whatever is missing here is stubbed in sys.modules for the import -- none
of it is reached by the three methods.

Stored: the inputs a, b (float32 [257, 64]), sims, k_values, the metrics of both directions, and
each query's rank taken from the reference's argsort position (:85-87).

The comparison must not depend on how the reference's fp32 matmul orders near-ties: the generator
checks in fp64 that no other score lies within 1e-5 of a target's score, in either direction, and
refuses to write otherwise. The test then excludes nothing.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
K_VALUES = [1, 5, 10]
MIN_GAP = 1e-5


def _load_reference_evaluator():
    stubs = {}
    for name in ("pandas", "tqdm", "peft", "models", "models.clip_model", "src", "src.embedding",
                 "src.embedding.similarity"):
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
        for fn in ("load_clip_model", "encode_text", "encode_image"):
            setattr(stubs["models.clip_model"], fn, None)
    if "src.embedding.similarity" in stubs:
        stubs["src.embedding.similarity"].cosine_similarity = None
    try:
        spec = importlib.util.spec_from_file_location("ref_evaluate_model", os.path.join(REF, "scripts/evaluate_model.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for name in stubs:
            sys.modules.pop(name, None)
    return mod.CLIPEvaluator


def _ranks(sims: torch.Tensor) -> np.ndarray:
    """the rank compute_mrr takes for each query (evaluate_model.py:85-87)"""
    out = []
    for i in range(sims.shape[0]):
        order = torch.argsort(sims[i], descending=True)
        out.append((order == i).nonzero(as_tuple=True)[0].item() + 1)
    return np.asarray(out, np.int64)


def _min_gap(a: np.ndarray, b: np.ndarray) -> float:
    a64 = a.astype(np.float64)
    b64 = b.astype(np.float64)
    a64 /= np.linalg.norm(a64, axis=1, keepdims=True)
    b64 /= np.linalg.norm(b64, axis=1, keepdims=True)
    s = a64 @ b64.T
    gap = np.inf
    for m in (s, s.T):
        d = np.abs(m - np.diag(m)[:, None])
        np.fill_diagonal(d, np.inf)
        gap = min(gap, d.min())
    return float(gap)


def main():
    E = _load_reference_evaluator()
    rng = np.random.default_rng(0)
    a = rng.standard_normal((257, 64)).astype(np.float32)
    b = (a + 3.0 * rng.standard_normal((257, 64))).astype(np.float32)
    gap = _min_gap(a, b)
    if not gap > MIN_GAP:
        raise SystemExit(f"a score lies within {gap:.3e} of a target's: the fixture would depend on fp32 tie order")
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    ta = ta / ta.norm(dim=-1, keepdim=True)       # evaluate_model.py:183-184
    tb = tb / tb.norm(dim=-1, keepdim=True)
    sims = torch.matmul(ta, tb.T)                 # :188
    out = {"a": a, "b": b, "sims": sims.numpy(), "k_values": np.asarray(K_VALUES, np.int64),
           "min_gap": np.float64(gap)}
    for tag, m in (("i2t", sims), ("t2i", sims.T)):
        rec = E.compute_recall_at_k(None, m, K_VALUES)
        out[f"{tag}_recall"] = np.asarray([rec[f"recall@{k}"] for k in K_VALUES], np.float64)
        out[f"{tag}_mrr"] = np.float64(E.compute_mrr(None, m))
        out[f"{tag}_map"] = np.float64(E.compute_map(None, m))
        out[f"{tag}_ranks"] = _ranks(m)
    np.savez_compressed(os.path.join(HERE, "eval_metrics.npz"), **out)
    print(f"eval_metrics.npz: min gap {gap:.3e}, recall {out['i2t_recall']}, mrr {out['i2t_mrr']:.4f}, "
          f"deepest rank {out['i2t_ranks'].max()}")


if __name__ == "__main__":
    main()
