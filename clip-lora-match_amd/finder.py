"""The finder's report flow (src/embedding/finder_service.py:41-216) on a resident index.

FinderService.report_item copies the uploaded image, encodes the item's *description text*
(+ ", ditemukan di <location>", :158-161) with CLIP+LoRA, re-normalises it (:165-169), then
re-loads the whole .pt index, torch.cat's one row onto it and re-saves the whole file on every
report (:171-185), and inserts a Postgres row (:187-204). Here:

* the index stays resident (TextSearchIndex: fp32 host mirror in a capacity-doubling buffer +
  the HBM index): one report appends in amortised O(1), and a search right after a report
  sees the new row without a reload;
* persistence keeps the reference .pt format ({"embeddings", "image_paths", "texts"},
  :93-103) and is decoupled from the append: `save_every=1` re-saves after every report as the
  reference does, `save_every=n` after every n-th, `save_every=0` only on `flush()`;
* reports can be batched (`report_items`): one encoder launch sequence for many descriptions;
* the Postgres insert and the YOLO crop (:140-156, off by default in the API, main.py:34) are
  outside the encode/search path and are not part of this module: the returned record carries
  the index row number where the reference returns the database id.
"""
from __future__ import annotations

import shutil
from datetime import datetime
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Union

import torch

from .clip_model import encode_text
from .search import SearchResult, TextSearchIndex

PathLike = Union[str, Path]


def _full_text(description: str, location: Optional[str]) -> str:
    # finder_service.py:159-161
    return f"{description}, ditemukan di {location}" if location else description


class FinderIndex:
    """Resident index + report flow. `index_path` need not exist yet (a new index, :86-91)."""

    def __init__(self, model, processor, device, index_path: PathLike, root_dir: PathLike,
                 upload_dir: PathLike, save_every: int = 1, dim: Optional[int] = None):
        self.model, self.processor, self.device = model, processor, device
        self.index_path = Path(index_path)
        self.root_dir = Path(root_dir).resolve()
        self.upload_dir = Path(upload_dir)
        self.upload_dir.mkdir(parents=True, exist_ok=True)
        if save_every < 0:
            raise ValueError("save_every must be >= 0")
        self.save_every = int(save_every)
        self._unsaved = 0
        if self.index_path.exists():
            self.index = TextSearchIndex(self.index_path, device=device)
        else:
            d = int(dim if dim is not None else model.cfg.proj_dim)
            self.index = TextSearchIndex(embeddings=torch.empty((0, d)), image_paths=[], texts=[], device=device)

    def _store_image(self, src_image_path: PathLike) -> str:
        src = Path(src_image_path).resolve()
        if not src.exists():
            raise FileNotFoundError(f"Source image not found: {src}")
        dest = (self.upload_dir / src.name).resolve()
        if src != dest:
            shutil.copy2(src, dest)
        return str(dest.relative_to(self.root_dir)).replace("\\", "/")

    def report_items(self, src_image_paths: Sequence[PathLike], descriptions: Sequence,
                     locations: Optional[Sequence[Optional[str]]] = None,
                     reporters: Optional[Sequence[Optional[str]]] = None,
                     found_at: Optional[Sequence[Optional[datetime]]] = None) -> List[Dict]:
        """Report n items at once: n descriptions encoded in one batch, n rows appended."""
        n = len(descriptions)
        if len(src_image_paths) != n:
            raise ValueError(f"{len(src_image_paths)} images vs {n} descriptions")
        locations = list(locations) if locations is not None else [None] * n
        reporters = list(reporters) if reporters is not None else [None] * n
        found_at = list(found_at) if found_at is not None else [None] * n
        # checked before any image is copied: token-id descriptions have no text to append a
        # location to (finder_service.py:123-131 builds "<description>, ditemukan di <location>"),
        # and one batch is either all strings or all token ids
        is_str = [isinstance(d, str) for d in descriptions]
        if any(is_str) and not all(is_str):
            raise ValueError("descriptions must be all strings or all token-id lists, not a mix")
        if not all(is_str) and any(loc for loc in locations):
            raise ValueError("a location needs a string description (token ids cannot carry it)")
        rel_paths = [self._store_image(p) for p in src_image_paths]
        texts = []
        for d, loc in zip(descriptions, locations):
            texts.append(_full_text(d, loc) if isinstance(d, str) else d)
        if n == 0:
            return []
        if all(isinstance(t, str) for t in texts) or n == 1:
            ids = self.processor.token_ids(texts if n > 1 or isinstance(texts[0], str) else texts[0])
        else:
            ids = self.processor.token_ids(texts)
        emb = self.model.encode_ids(ids.to(self.model.device), normalize=True).to("cpu", torch.float32)
        first = self.index.num_items
        self.index.append(emb, rel_paths, [t if isinstance(t, str) else "" for t in texts])
        self._unsaved += n
        if self.save_every and self._unsaved >= self.save_every:
            self.flush()
        out = []
        for j in range(n):
            ts = found_at[j] or datetime.now()
            out.append({"id": first + j, "image_path": rel_paths[j],
                        "description": texts[j] if isinstance(texts[j], str) else "",
                        "location": locations[j], "found_at": ts.isoformat(), "reporter": reporters[j]})
        return out

    def report_item(self, src_image_path: PathLike, description, location: Optional[str] = None,
                    reporter: Optional[str] = None, found_at: Optional[datetime] = None) -> Dict:
        """finder_service.py:107-216 (without the database insert)."""
        return self.report_items([src_image_path], [description], [location], [reporter], [found_at])[0]

    def _saved(self, n: int) -> None:
        self._unsaved += n
        if self.save_every and self._unsaved >= self.save_every:
            self.flush()

    def resolve_items(self, ids: Sequence[int]) -> List[Dict]:
        """Items handed back to their owners stop matching: their rows leave the index (in place,
        TextSearchIndex.remove). Returns the removed records ({"id": the old row number,
        "image_path", "description"}), in the order given. The .pt model is positional
        (finder_service.py:93-103: row i, image_paths[i], texts[i]), so the row number of every
        item above a removed one shifts down by the number of removed rows below it; ids handed out
        by earlier reports must be re-read after a resolve. Uploaded image files are not deleted.
        Counts toward `save_every` like a report does."""
        ids = [int(i) for i in ids]
        idx = self.index
        for i in ids:
            if not 0 <= i < idx.num_items:
                raise ValueError(f"item id {i} is outside [0, {idx.num_items})")
        if len(set(ids)) != len(ids):
            raise ValueError("duplicate item id")
        out = [{"id": i, "image_path": idx.image_paths[i] if i < len(idx.image_paths) else "",
                "description": idx.texts[i] if i < len(idx.texts) else ""} for i in ids]
        if ids:
            idx.remove(ids)
            self._saved(len(ids))
        return out

    def resolve_item(self, id: int) -> Dict:
        """resolve_items for one item."""
        return self.resolve_items([id])[0]

    def update_item(self, id: int, description, location: Optional[str] = None) -> Dict:
        """Correct an item's description: the text is re-encoded as report_items encodes it, and
        the item's row and text are replaced in place; its id and image stay."""
        id = int(id)
        if not 0 <= id < self.index.num_items:
            raise ValueError(f"item id {id} is outside [0, {self.index.num_items})")
        if not isinstance(description, str) and location:
            raise ValueError("a location needs a string description (token ids cannot carry it)")
        text = _full_text(description, location) if isinstance(description, str) else description
        tok = self.processor.token_ids(text)
        emb = self.model.encode_ids(tok.to(self.model.device), normalize=True).to("cpu", torch.float32)
        stored = text if isinstance(text, str) else ""
        self.index.update([id], emb, texts=[stored])
        self._saved(1)
        return {"id": id, "image_path": self.index.image_paths[id] if id < len(self.index.image_paths) else "",
                "description": stored, "location": location}

    def similar_items(self, descriptions: Sequence, threshold: float,
                      locations: Optional[Sequence[Optional[str]]] = None) -> List[List[Dict]]:
        """Which existing reports describe the same thing: for each description (encoded as
        report_items encodes it) every item of the index whose cosine is >= threshold, best first,
        as {"id", "score", "image_path", "description"}. Nothing in the index changes."""
        n = len(descriptions)
        locations = list(locations) if locations is not None else [None] * n
        is_str = [isinstance(d, str) for d in descriptions]
        if any(is_str) and not all(is_str):
            raise ValueError("descriptions must be all strings or all token-id lists, not a mix")
        if not all(is_str) and any(loc for loc in locations):
            raise ValueError("a location needs a string description (token ids cannot carry it)")
        idx = self.index
        if n == 0:
            return []
        if idx.num_items == 0:
            return [[] for _ in range(n)]
        texts = [_full_text(d, loc) if isinstance(d, str) else d for d, loc in zip(descriptions, locations)]
        if all(isinstance(t, str) for t in texts) or n == 1:
            ids = self.processor.token_ids(texts if n > 1 or isinstance(texts[0], str) else texts[0])
        else:
            ids = self.processor.token_ids(texts)
        emb = self.model.encode_ids(ids.to(self.model.device), normalize=True).to(torch.float32)
        off, scores, rows = idx._gpu.search_above(emb, float(threshold))
        off, scores, rows = off.tolist(), scores.tolist(), rows.tolist()
        out = []
        for q in range(n):
            out.append([{"id": r, "score": float(s),
                         "image_path": idx.image_paths[r] if 0 <= r < len(idx.image_paths) else "",
                         "description": idx.texts[r] if 0 <= r < len(idx.texts) else ""}
                        for r, s in zip(rows[off[q]: off[q + 1]], scores[off[q]: off[q + 1]])])
        return out

    def flush(self) -> None:
        """Write the index in the reference .pt format (finder_service.py:93-103)."""
        self.index.save(self.index_path)
        self._unsaved = 0
        print(f"[FinderService] Index updated and saved to: {self.index_path}")

    def search(self, query_emb: torch.Tensor, top_k: int = 5, where=None, group_by=None):
        """where: a row filter (TextSearchIndex.search_with_embedding's allow): a mask, item
        positions, or a callable (i, image_path, text) -> bool -- only those items compete.
        group_by: at most one result per group, its best row ("image_path", "text", a callable
        (i, image_path, text) -> key, or group ids; TextSearchIndex.search_with_embedding's group_by)"""
        if group_by is not None:
            return self.index.search_with_embedding(query_emb, top_k=top_k, allow=where, group_by=group_by)
        if where is None:
            return self.index.search_with_embedding(query_emb, top_k=top_k)
        return self.index.search_with_embedding(query_emb, top_k=top_k, allow=where)

    def search_many(self, query_embs, top_k: int, keys, lo, hi) -> List[List[SearchResult]]:
        """Many seekers in one batched search, each with its own inclusive value range over the items:
        query i sees the items with lo[i] <= keys[j] <= hi[i] (keys: one number per item -- a found_at
        timestamp, a location or category code --, a callable (i, image_path, text) -> number, or a
        CosineIndex.key_plan(); lo / hi: [nq], a scalar, or None for an open side;
        TextSearchIndex.search_batch's keys=). One SearchResult list per query, best first, shorter than
        top_k where fewer items lie in its range."""
        scores, indices = self.index.search_batch(query_embs, top_k, keys=keys, lo=lo, hi=hi)
        paths, texts = self.index.image_paths, self.index.texts
        out: List[List[SearchResult]] = []
        for row_i, row_s in zip(indices.tolist(), scores.tolist()):
            out.append([SearchResult(index=j, score=float(sc), image_path=paths[j] if j < len(paths) else "",
                                     text=texts[j] if j < len(texts) else "")
                        for j, sc in zip(row_i, row_s) if j >= 0])
        return out


__all__ = ["FinderIndex"]
