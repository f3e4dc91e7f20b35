"""Retrieval evaluation on the GPU index: the reference's scripts/evaluate_model.py
(CLIPEvaluator and its compute_recall_at_k / compute_mrr / compute_map / evaluate_retrieval /
evaluate_matching_accuracy) without its [N, N] similarity matrix.

Every metric of that flow is a function of one number per query, the rank of its ground-truth item
among all candidates. The reference reads it off torch.topk / torch.argsort of each row of
image_emb @ text_emb.T (evaluate_model.py:60,85,101: an O(N^2 log N) pattern); here
CosineIndex.rank counts the candidates ahead of the target in one streaming MFMA pass over the
resident index (clm_index_rank), so no score matrix exists on the embeddings path.

  retrieval_ranks(queries, candidates, targets=None)   rank of candidates[targets[i]] for queries[i]
  recall_at_k / mrr / mean_average_precision            the metrics, from a rank vector
  evaluate_retrieval(image_emb, text_emb, k_values)     evaluate_model.py:186-211's result dict
  matching_accuracy(image_emb, text_emb)                evaluate_model.py:276-286
  CLIPEvaluator                                         evaluate_model.py:17-286, same method names

Ranks order equal scores by candidate index (the search order); the reference's argsort leaves
ties in arbitrary order.
"""
from __future__ import annotations

import csv
from pathlib import Path
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from .search import CosineIndex

IMAGE_COLUMNS = ("image_path", "image_file", "filename", "image")   # evaluate_model.py:127
TEXT_COLUMNS = ("text", "caption", "description")                   # evaluate_model.py:129


# ------------------------------------------------------------------ ranks -> metrics --
def _rank_array(ranks) -> np.ndarray:
    r = ranks.detach().cpu().numpy() if isinstance(ranks, torch.Tensor) else np.asarray(ranks)
    r = r.astype(np.int64).reshape(-1)
    if r.size == 0:
        raise ValueError("no ranks: the metrics need at least one query")
    if (r < 1).any():
        raise ValueError("ranks start at 1")
    return r


def recall_at_k(ranks, k_values: Sequence[int] = (1, 5, 10)) -> Dict[str, float]:
    """{"recall@K": share of queries whose target ranks within the first K} (compute_recall_at_k)"""
    r = _rank_array(ranks)
    return {f"recall@{k}": int((r <= k).sum()) / r.size for k in k_values}


def mrr(ranks) -> float:
    """mean of 1 / rank (compute_mrr)"""
    return float(np.mean(1.0 / _rank_array(ranks)))


def mean_average_precision(ranks) -> float:
    """mAP with one relevant item per query: AP = 1 / rank, so it equals MRR (compute_map,
    evaluate_model.py:104-105)"""
    return mrr(ranks)


# ------------------------------------------------------------------ embeddings -> ranks --
def retrieval_ranks(queries, candidates, targets=None, device=None) -> torch.Tensor:
    """[nq] int64 (CPU): the exact rank of candidate targets[i] (default i) for query i among all
    candidates, by cosine (rows need not be normalised). One CosineIndex is built, appended to,
    ranked against and closed; replaces a per-query top_k_similar / argsort loop."""
    q = torch.as_tensor(queries)
    c = torch.as_tensor(candidates)
    if q.dim() != 2 or c.dim() != 2 or q.shape[1] != c.shape[1]:
        raise ValueError(f"queries [nq, d] and candidates [n, d] expected, got {tuple(q.shape)} and {tuple(c.shape)}")
    if targets is None:
        if q.shape[0] != c.shape[0]:
            raise ValueError("without targets, query i is paired with candidate i: the counts must match")
        targets = torch.arange(q.shape[0], dtype=torch.int64)
    idx = CosineIndex(c.shape[1], capacity=max(c.shape[0], 1), device=device)
    try:
        idx.append(c)
        ranks, _ = idx.rank(q, targets)
        return ranks.cpu()
    finally:
        idx.close()


def evaluate_retrieval(image_emb, text_emb, k_values: Sequence[int] = (1, 5, 10)) -> Dict[str, float]:
    """The reference's result dict (evaluate_model.py:191-211), keys in its order: recall@K for
    image -> text, mrr, map, then t2i_recall@K for text -> image. Pair i is (image i, text i)."""
    i2t = retrieval_ranks(image_emb, text_emb)
    t2i = retrieval_ranks(text_emb, image_emb)
    results: Dict[str, float] = {}
    results.update(recall_at_k(i2t, k_values))
    results["mrr"] = mrr(i2t)
    results["map"] = mean_average_precision(i2t)
    for k, v in recall_at_k(t2i, k_values).items():
        results[f"t2i_{k}"] = v
    return results


def matching_accuracy(image_emb, text_emb) -> float:
    """share of images whose own caption scores highest (evaluate_model.py:276-286): recall@1"""
    return recall_at_k(retrieval_ranks(image_emb, text_emb), (1,))["recall@1"]


# ------------------------------------------------------------------ similarity matrix -> ranks --
def _diagonal_ranks(similarities) -> np.ndarray:
    """ranks of the diagonal of a similarity matrix a caller already holds (the compute_* methods'
    input), ties ordered by column"""
    s = torch.as_tensor(similarities)
    if s.dim() != 2 or s.shape[0] > s.shape[1]:
        raise ValueError(f"similarities must be [N, M >= N], got {tuple(s.shape)}")
    n = s.shape[0]
    t = s.diagonal()[:, None]
    cols = torch.arange(s.shape[1])[None, :]
    ahead = (s > t) | ((s == t) & (cols < torch.arange(n)[:, None]))
    return (1 + ahead.sum(dim=1)).cpu().numpy()


def _columns(fieldnames) -> Tuple[str, str]:
    image_col = text_col = None
    for col in fieldnames or []:
        if col.lower() in IMAGE_COLUMNS:
            image_col = col
        if col.lower() in TEXT_COLUMNS:
            text_col = col
    if image_col is None or text_col is None:
        raise ValueError(f"CSV must have image and text columns. Found: {list(fieldnames or [])}")
    return image_col, text_col


def read_pairs(test_csv, image_root_dir, warn: bool = True) -> Tuple[List[Path], List[str]]:
    """(image paths, captions) of the rows of test_csv whose image exists, with the reference's
    column names and path fallbacks (evaluate_model.py:126-161): root / name, root / basename, the
    name as given; a missing image is skipped (with the reference's warning if `warn`)."""
    image_root_dir = Path(image_root_dir)
    with open(test_csv, newline="", encoding="utf-8") as f:
        reader = csv.DictReader(f)
        image_col, text_col = _columns(reader.fieldnames)
        rows = list(reader)
    print(f"[Evaluator] Using columns: image='{image_col}', text='{text_col}'")
    print(f"[Evaluator] Loading {len(rows)} test samples...")
    paths, texts = [], []
    for row in rows:
        name = row[image_col]
        found = None
        for p in (image_root_dir / name, image_root_dir / Path(name).name, Path(name)):
            if p.exists():
                found = p
                break
        if found is None:
            if warn:
                print(f"Warning: Image not found: {name}, skipping...")
            continue
        paths.append(found)
        texts.append(row[text_col])
    return paths, texts


class CLIPEvaluator:
    """The reference's evaluator (evaluate_model.py:17-286) on the GPU encoder and index."""

    def __init__(self, clip_config_path, lora_weights_path=None, use_lora: bool = True, **load_kwargs):
        from .clip_model import load_clip_model
        self.model, self.processor, self.device = load_clip_model(
            config_path=clip_config_path, use_lora=use_lora,
            lora_weights_path=lora_weights_path if use_lora else None, **load_kwargs)
        print(f"[Evaluator] Model loaded on device: {self.device}")

    def close(self) -> None:
        if getattr(self, "model", None) is not None:
            self.model.close()
            self.model = None

    # the reference's compute_* take the similarity matrix their caller built
    def compute_recall_at_k(self, similarities, k_values: Sequence[int] = (1, 5, 10)) -> Dict[str, float]:
        return recall_at_k(_diagonal_ranks(similarities), k_values)

    def compute_mrr(self, similarities) -> float:
        return mrr(_diagonal_ranks(similarities))

    def compute_map(self, similarities) -> float:
        return mean_average_precision(_diagonal_ranks(similarities))

    def encode_pairs(self, test_csv, image_root_dir, warn: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
        """(image embeddings, text embeddings) [N, d] of the CSV's usable rows, batched"""
        from .embed_image import embed_images_batch
        from .embed_text import embed_text
        paths, texts = read_pairs(test_csv, image_root_dir, warn=warn)
        if not paths:
            return torch.empty(0), torch.empty(0)
        chunk = max(1, int(getattr(self.model, "max_batch", 16)))
        img = embed_images_batch(self.model, self.processor, paths, self.device, normalize=True, batch_size=chunk)
        txt = torch.cat([embed_text(self.model, self.processor, texts[i:i + chunk], self.device, normalize=True)
                         for i in range(0, len(texts), chunk)], dim=0)
        print(f"[Evaluator] Successfully loaded {len(paths)} samples")
        return img, txt

    def evaluate_retrieval(self, test_csv, image_root_dir, k_values: Sequence[int] = (1, 5, 10)) -> Dict[str, float]:
        img, txt = self.encode_pairs(test_csv, image_root_dir)
        if img.numel() == 0:
            raise ValueError("No valid samples found! Check image paths.")
        return evaluate_retrieval(img, txt, k_values)

    def evaluate_matching_accuracy(self, test_csv, image_root_dir) -> float:
        img, txt = self.encode_pairs(test_csv, image_root_dir, warn=False)
        if img.numel() == 0:
            return 0.0
        return matching_accuracy(img, txt)


__all__ = ["retrieval_ranks", "recall_at_k", "mrr", "mean_average_precision", "evaluate_retrieval",
           "matching_accuracy", "read_pairs", "CLIPEvaluator"]
