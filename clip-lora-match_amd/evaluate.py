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
  contrastive_loss(image_emb, text_emb, temperature)    scripts/train_lora.py:83-108 over the whole
                                                        set (or :213-241's per-batch mean), the
                                                        reference's model-selection signal
  contrastive_loss_grad / contrastive_loss_tensor       the same loss with its gradient (what
                                                        train_lora.py's loss.backward() delivers to
                                                        the embeddings), streamed: no [N, N] logits
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


# ------------------------------------------------------------------ threshold evaluator --
def threshold_metrics(counts, n_index: int, k_values: Sequence[int] = (1, 5, 10)) -> Dict:
    """The aggregation of the reference's second evaluator (scripts/evaluate.py:221-267,
    evaluate_epoch) from one number per query: counts[i] = how many index rows are relevant to query
    i. That evaluator calls relevant every row whose cosine is >= a threshold and ranks the index by
    the same cosines (evaluate_single_query, :158-166), so the relevant set IS A PREFIX of the
    ranking -- its first counts[i] entries. Hence, per query with c relevant rows,
      recall@k    = min(c, k) / c      (0 when c = 0; calculate_recall_at_k, :50-58)
      precision@k = min(c, k) / k      (calculate_precision_at_k, :61-67)
      mrr = ap    = 1 when c > 0 else 0  (the first hit is at rank 1, every hit r of the prefix has
                                        precision r / r; calculate_mrr / _average_precision :70-99)
    and no N-long argsort is needed. Returns the reference's metrics dict without its epoch and
    timing entries: num_queries, recall / precision {k: percent}, mrr and map as means."""
    c = counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    c = c.astype(np.int64).reshape(-1)
    if c.size == 0:
        raise ValueError("no queries: the metrics need at least one")
    if (c < 0).any() or (c > int(n_index)).any():
        raise ValueError("a relevant count lies outside [0, n_index]")
    recall, precision = {}, {}
    for k in k_values:
        k = int(k)
        hit = np.minimum(c, k).astype(np.float64)
        recall[k] = float(np.mean(np.where(c > 0, hit / np.maximum(c, 1), 0.0)) * 100)
        precision[k] = float(np.mean(hit / k if k > 0 else np.zeros_like(hit)) * 100)
    found = float(np.mean((c > 0).astype(np.float64)))
    return {"num_queries": int(c.size), "recall": recall, "precision": precision, "mrr": found, "map": found}


def evaluate_threshold_retrieval(query_emb, index, threshold: float = 0.7, k_values: Sequence[int] = (1, 5, 10),
                                 return_sets: bool = False, device=None):
    """scripts/evaluate.py's evaluate_epoch on embeddings: every row of `index` (a CosineIndex, or
    [N, d] embeddings to build one from) with cosine >= threshold is relevant to a query; metrics as
    threshold_metrics, plus "threshold". The relevant sets come from CosineIndex.search_above -- the
    lengths are all the metrics need (the relevant set is a prefix of the ranking), and no [nq, N]
    matrix or per-query argsort exists. return_sets: also (offsets, scores, ids) on the CPU, the
    relevant rows of each query, best first."""
    own = not isinstance(index, CosineIndex)
    if own:
        rows = torch.as_tensor(index)
        if rows.dim() != 2:
            raise ValueError(f"index embeddings [N, d] expected, got {tuple(rows.shape)}")
        idx = CosineIndex(rows.shape[1], capacity=max(rows.shape[0], 1), device=device)
    else:
        idx = index
    try:
        if own:
            idx.append(rows)
        off, s, i = idx.search_above(query_emb, float(threshold))
        off = off.cpu()
        m = threshold_metrics(off[1:] - off[:-1], len(idx), k_values)
        m["threshold"] = float(threshold)
        return (m, (off, s.cpu(), i.cpu())) if return_sets else m
    finally:
        if own:
            idx.close()


# ------------------------------------------------------------------ contrastive loss --
def loss_from_lse(lse_i2t, lse_t2i, pair_scores, temperature: float, err_i2t=None, err_t2i=None) -> Dict[str, float]:
    """The symmetric InfoNCE loss of train_lora.py:83-108 from its row reductions, in fp64:
    cross_entropy(logits, arange) = mean_i(lse_i - t_i / T) per direction, lse_i the log-sum-exp of
    row i of scores / T and t_i = pair_scores[i] the score of pair i (the diagonal, shared by both
    directions); loss = (loss_i2t + loss_t2i) / 2. err: the mean of the lse bounds (0 without)."""
    li = torch.as_tensor(lse_i2t).detach().double().cpu().reshape(-1)
    lt = torch.as_tensor(lse_t2i).detach().double().cpu().reshape(-1)
    t = torch.as_tensor(pair_scores).detach().double().cpu().reshape(-1)
    if li.numel() == 0 or li.numel() != lt.numel() or li.numel() != t.numel():
        raise ValueError("one lse per direction and one pair score per pair expected, at least one pair")
    if not (temperature > 0 and np.isfinite(temperature)):
        raise ValueError("temperature must be finite and positive")
    l_i = float((li - t / temperature).mean())
    l_t = float((lt - t / temperature).mean())
    err = 0.0
    if err_i2t is not None and err_t2i is not None:
        ei = torch.as_tensor(err_i2t).detach().double().cpu()
        et = torch.as_tensor(err_t2i).detach().double().cpu()
        err = float((ei.mean() + et.mean()) / 2)
    return {"loss": (l_i + l_t) / 2, "loss_i2t": l_i, "loss_t2i": l_t, "err": err}


def _cosines64(a, b) -> torch.Tensor:
    """[len(a), len(b)] cosines in fp64 on the host"""
    a64, b64 = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return (a64 / a64.norm(dim=1, keepdim=True)) @ (b64 / b64.norm(dim=1, keepdim=True)).T


def batched_loss(image_emb, text_emb, temperature: float, batch_size: int, scores=None) -> Dict[str, float]:
    """train_lora.py:213-241's validation number: the mean over consecutive batches of batch_size
    pairs (the last one may be short) of the per-batch loss, block-diagonal B x B problems done on
    the host in fp64 from scores(image_block, text_block) -> [B, B]. Default: fp64 cosines, since
    scores rounded to fp32 (cosine_similarity's) move this number by several 1e-9."""
    if int(batch_size) < 1:
        raise ValueError("batch_size must be at least 1")
    if scores is None:
        scores = _cosines64
    a, b = torch.as_tensor(image_emb), torch.as_tensor(text_emb)
    keys = ("loss", "loss_i2t", "loss_t2i")
    total = dict.fromkeys(keys, 0.0)
    nb = 0
    for s0 in range(0, a.shape[0], int(batch_size)):
        ab, bb = a[s0:s0 + batch_size], b[s0:s0 + batch_size]
        S = torch.as_tensor(scores(ab, bb)).detach().double().cpu().reshape(ab.shape[0], bb.shape[0])
        L = S / temperature
        part = loss_from_lse(torch.logsumexp(L, dim=1), torch.logsumexp(L, dim=0), S.diagonal(), temperature)
        for k in keys:
            total[k] += part[k]
        nb += 1
    out = {k: total[k] / nb for k in keys}
    out["err"] = 0.0
    return out


def contrastive_loss(image_emb, text_emb, temperature: float = 0.07, batch_size=None, head: int = 64,
                     band_cap: int = 0, device=None) -> Dict[str, float]:
    """{"loss", "loss_i2t", "loss_t2i", "err"}: the reference's CLIP contrastive loss
    (compute_clip_contrastive_loss, train_lora.py:83-108) of N pairs against each other, without
    the [N, N] logits: per direction CosineIndex.logsumexp streams the index once (scale = 1 / T as
    a double) and CosineIndex.rank gives the exact pair scores. err = the mean certified bound of
    the log-sum-exps, so |loss - the loss of the exact scores| <= err; the exact scores are fp64
    cosines rounded to fp32, which alone moves the loss by up to 2^-24 / T (a few 1e-9 at N in the
    hundreds). head = 0: the reference route instead (CosineIndex.logsumexp64): log-sum-exps and pair
    scores of the unrounded fp64 cosines, the reference function on float64 tensors to fp64
    rounding, err = 0, at the cost of an exact pass over all N x N pairs.
    batch_size = B: the mean of the per-batch losses instead (batched_loss), the number
    train_lora.py:213-241 prints after every epoch."""
    a, b = torch.as_tensor(image_emb), torch.as_tensor(text_emb)
    if a.dim() != 2 or b.dim() != 2 or a.shape != b.shape or a.shape[0] == 0:
        raise ValueError(f"image_emb and text_emb must be [N >= 1, d] pairs, got {tuple(a.shape)} and {tuple(b.shape)}")
    if not (temperature > 0 and np.isfinite(temperature)):
        raise ValueError("temperature must be finite and positive")
    if batch_size is not None:
        return batched_loss(a, b, temperature, batch_size)
    res = {}
    for tag, qs, rows in (("i2t", a, b), ("t2i", b, a)):
        idx = CosineIndex(rows.shape[1], capacity=a.shape[0], device=device)
        try:
            idx.append(rows)
            res[tag] = _direction(idx, qs, temperature, head, band_cap)
        finally:
            idx.close()
    return _loss_of(res, temperature)


def _check_pairs(image_emb, text_emb, temperature) -> Tuple[torch.Tensor, torch.Tensor]:
    a, b = torch.as_tensor(image_emb), torch.as_tensor(text_emb)
    if a.dim() != 2 or b.dim() != 2 or a.shape != b.shape or a.shape[0] == 0:
        raise ValueError(f"image_emb and text_emb must be [N >= 1, d] pairs, got {tuple(a.shape)} and {tuple(b.shape)}")
    if not (temperature > 0 and np.isfinite(temperature)):
        raise ValueError("temperature must be finite and positive")
    return a, b


def _direction(idx: CosineIndex, qs, temperature: float, head: int, band_cap: int = 0):
    """(lse, err, pair scores) of queries qs against the index holding their partners, query i's
    partner being row i: what contrastive_loss and contrastive_loss_grad share, on the index's device"""
    n = qs.shape[0]
    targets = torch.arange(n, dtype=torch.int64)
    if int(head) <= 0 and not int(band_cap):
        lse, t = idx.logsumexp64(qs, 1.0 / temperature, targets)
        return lse, torch.zeros(n), t
    lse, err = idx.logsumexp(qs, 1.0 / temperature, head=head, band_cap=band_cap)
    _, t = idx.rank(qs, targets)
    return lse, err, t


def _loss_of(res, temperature: float) -> Dict[str, float]:
    return loss_from_lse(res["i2t"][0], res["t2i"][0], res["i2t"][2], temperature, res["i2t"][1], res["t2i"][1])


# ------------------------------------------------------------------ the loss's gradient --
def unit_gradients(dq, dr, image_unit, text_unit, temperature: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """The loss's gradients with respect to the UNIT vectors, fp64, from the weighted sums of
    CosineIndex.softmax_grad (images as queries, texts as the index, wq = wr = 1). With s_ij = a^_i .
    b^_j, dL/ds_ij = (exp(s_ij / T - lse_i) + exp(s_ij / T - lse'_j)) / (2 N T) - [i = j] / (N T), so
        g_a^_i = dq[i] / (2 N T) - b^_i / (N T),      g_b^_j = dr[j] / (2 N T) - a^_j / (N T).
    Plain tensor arithmetic: any device."""
    dq, dr = torch.as_tensor(dq).double(), torch.as_tensor(dr).double()
    au, bu = torch.as_tensor(image_unit).double(), torch.as_tensor(text_unit).double()
    n = au.shape[0]
    return (dq / (2 * n * temperature) - bu / (n * temperature),
            dr / (2 * n * temperature) - au / (n * temperature))


def normalize_backward(g, x) -> torch.Tensor:
    """Backward of x -> x / |x| (rows): (g - (g . x^) x^) / |x|, fp64"""
    g, x = torch.as_tensor(g).double(), torch.as_tensor(x).double()
    nrm = x.norm(dim=1, keepdim=True)
    xu = x / nrm
    return (g - (g * xu).sum(dim=1, keepdim=True) * xu) / nrm


def loss_grad_from_sums(dq, dr, image_emb, text_emb, temperature: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(grad_image, grad_text) fp64 with respect to the raw embeddings, from softmax_grad's sums: the
    O(N d) tail of contrastive_loss_grad (unit_gradients, then normalize_backward on each side)"""
    a, b = torch.as_tensor(image_emb).double(), torch.as_tensor(text_emb).double()
    ga, gb = unit_gradients(dq, dr, a / a.norm(dim=1, keepdim=True), b / b.norm(dim=1, keepdim=True), temperature)
    return normalize_backward(ga, a), normalize_backward(gb, b)


def contrastive_loss_grad(image_emb, text_emb, temperature: float = 0.07, head: int = 64, device=None) -> Dict:
    """contrastive_loss and its gradient, without the [N, N] logits: {"loss", "loss_i2t", "loss_t2i",
    "err"} as contrastive_loss computes them (the same calls: the same bits), plus
      grad_image, grad_text   [N, d] fp32 on the GPU: dL / d(image_emb), dL / d(text_emb) with respect
                              to the RAW, unnormalised inputs -- what autograd returns through the
                              reference function, which normalises inside (train_lora.py:83-108);
      rho                     the certified relative bound of the streamed sums (below).
    Route: one log-sum-exp per direction, one CosineIndex.softmax_grad pass (wq = wr = 1) over the text
    index with the images as queries, then O(N d) tensor ops: the factor 1 / (2 N T), the diagonal
    term and the normalise backward (loss_grad_from_sums).
    Accuracy: row i of grad_image is within (rho * A_i + tau) / (2 N T |image_i|) of the exact
    gradient in the 2-norm, A_i = sum_j (exp(s_ij / T - lse_i) + exp(s_ij / T - lse'_j)) the row's
    weight mass (grad_text alike), (rho, tau) from search.softmax_grad_bound widened by exp(the
    largest log-sum-exp bound). rho is the honest worst case -- every fp16-pass score off by its whole
    bound in the same direction: 0.038 at T = 0.07, 0.28 at T = 0.01; measured errors sit near 1e-3 of
    A."""
    from .search import softmax_grad_bound
    a, b = _check_pairs(image_emb, text_emb, temperature)
    n = a.shape[0]
    res = {}
    txt = CosineIndex(b.shape[1], capacity=n, device=device)
    try:
        txt.append(b)
        res["i2t"] = _direction(txt, a, temperature, head)
        img = CosineIndex(a.shape[1], capacity=n, device=device)
        try:
            img.append(a)
            res["t2i"] = _direction(img, b, temperature, head)
        finally:
            img.close()
        dq, dr = txt.softmax_grad(a, 1.0 / temperature, res["i2t"][0], row_lse=res["t2i"][0], wq=1.0, wr=1.0)
        dev = txt.device
    finally:
        txt.close()
    out = _loss_of(res, temperature)
    ga, gb = loss_grad_from_sums(dq, dr, a.to(dev), b.to(dev), temperature)
    rho, _ = softmax_grad_bound(1.0 / temperature, n)
    lse_err = max(float(torch.as_tensor(res["i2t"][1]).max()), float(torch.as_tensor(res["t2i"][1]).max()))
    out.update(grad_image=ga.float(), grad_text=gb.float(), rho=(1 + rho) * float(np.exp(lse_err)) - 1)
    return out


class ContrastiveLoss(torch.autograd.Function):
    """contrastive_loss_grad as an autograd node: forward returns the loss as a 0-dim tensor on the
    inputs' device and keeps the two gradients, backward hands them on times the upstream gradient,
    so loss.backward() reaches whatever torch module produced the embeddings."""

    @staticmethod
    def forward(ctx, image_emb, text_emb, temperature=0.07, head=64):
        r = contrastive_loss_grad(image_emb.detach(), text_emb.detach(), temperature, head)
        ctx.save_for_backward(r["grad_image"].to(device=image_emb.device, dtype=image_emb.dtype),
                              r["grad_text"].to(device=text_emb.device, dtype=text_emb.dtype))
        return torch.tensor(r["loss"], dtype=image_emb.dtype, device=image_emb.device)

    @staticmethod
    def backward(ctx, grad_out):
        ga, gb = ctx.saved_tensors
        return grad_out.to(ga.device) * ga, grad_out.to(gb.device) * gb, None, None


def contrastive_loss_tensor(image_emb, text_emb, temperature: float = 0.07, head: int = 64) -> torch.Tensor:
    """The contrastive loss of N pairs as a differentiable 0-dim tensor (ContrastiveLoss): the
    training-side twin of contrastive_loss. image_emb / text_emb: [N, d] floating-point tensors, raw
    or normalised; the whole set is one global batch (the per-batch validation number stays
    contrastive_loss(batch_size=))."""
    if not (isinstance(image_emb, torch.Tensor) and isinstance(text_emb, torch.Tensor)):
        raise ValueError("image_emb and text_emb must be tensors")
    if not (image_emb.is_floating_point() and text_emb.is_floating_point()):
        raise ValueError("image_emb and text_emb must be floating-point tensors")
    _check_pairs(image_emb, text_emb, temperature)
    return ContrastiveLoss.apply(image_emb, text_emb, float(temperature), int(head))


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

    def evaluate_threshold_retrieval(self, test_csv, image_root_dir, threshold: float = 0.7,
                                     k_values: Sequence[int] = (1, 5, 10)) -> Dict:
        """The threshold evaluator (scripts/evaluate.py) on the CSV's pairs: the captions are the
        queries, the images the index -- every image at or above the cosine is relevant."""
        img, txt = self.encode_pairs(test_csv, image_root_dir)
        if img.numel() == 0:
            raise ValueError("No valid samples found! Check image paths.")
        return evaluate_threshold_retrieval(txt, img, threshold, k_values)

    def evaluate_loss(self, test_csv, image_root_dir, temperature: float = 0.07, batch_size=None) -> Dict[str, float]:
        """contrastive_loss of the CSV's pairs (train_lora.py's validation loss on this adapter)"""
        img, txt = self.encode_pairs(test_csv, image_root_dir)
        if img.numel() == 0:
            raise ValueError("No valid samples found! Check image paths.")
        return contrastive_loss(img, txt, temperature, batch_size)

    def evaluate_matching_accuracy(self, test_csv, image_root_dir) -> float:
        img, txt = self.encode_pairs(test_csv, image_root_dir, warn=False)
        if img.numel() == 0:
            return 0.0
        return matching_accuracy(img, txt)


__all__ = ["retrieval_ranks", "recall_at_k", "mrr", "mean_average_precision", "evaluate_retrieval",
           "matching_accuracy", "threshold_metrics", "evaluate_threshold_retrieval", "contrastive_loss", "loss_from_lse", "batched_loss", "read_pairs", "CLIPEvaluator",
           "contrastive_loss_grad", "contrastive_loss_tensor", "ContrastiveLoss", "unit_gradients", "normalize_backward",
           "loss_grad_from_sums"]
