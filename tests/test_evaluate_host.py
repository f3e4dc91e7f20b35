"""Host-side half of the retrieval evaluator (clip_lora_match_amd.evaluate): the metrics from
hand-made rank vectors, the result dict's keys, CSV column detection, and no silent CPU path."""
import numpy as np
import pytest
import torch

import clip_lora_match_amd as clm
from clip_lora_match_amd import evaluate as EV


def test_metrics_from_hand_made_ranks():
    ranks = [1, 2, 4, 10, 11]
    assert EV.recall_at_k(ranks, (1, 5, 10)) == {"recall@1": 0.2, "recall@5": 0.6, "recall@10": 0.8}
    want = (1 + 1 / 2 + 1 / 4 + 1 / 10 + 1 / 11) / 5
    assert abs(EV.mrr(ranks) - want) < 1e-15
    assert EV.mean_average_precision(ranks) == EV.mrr(ranks)
    assert EV.recall_at_k(torch.tensor([3, 1]), [1]) == {"recall@1": 0.5}
    assert EV.mrr(np.array([1, 1, 1])) == 1.0
    for bad in ([], [0, 1], [-2]):
        with pytest.raises(ValueError):
            EV.mrr(bad)
    assert clm.recall_at_k is EV.recall_at_k and clm.CLIPEvaluator is EV.CLIPEvaluator


def test_compute_methods_key_names_and_order():
    """a 4 x 4 matrix whose diagonal ranks 1, 2, 3, 1 (the tie in row 2 is ordered by column)"""
    sims = torch.tensor([[0.9, 0.1, 0.2, 0.3],
                         [0.8, 0.5, 0.1, 0.2],
                         [0.7, 0.6, 0.6, 0.1],
                         [0.0, 0.1, 0.2, 0.3]])
    ev = EV.CLIPEvaluator.__new__(EV.CLIPEvaluator)
    rec = ev.compute_recall_at_k(sims, [1, 2, 5])
    assert list(rec) == ["recall@1", "recall@2", "recall@5"]
    assert rec == {"recall@1": 0.5, "recall@2": 0.75, "recall@5": 1.0}
    want = (1 + 1 / 2 + 1 / 3 + 1) / 4
    assert abs(ev.compute_mrr(sims) - want) < 1e-15 and ev.compute_map(sims) == ev.compute_mrr(sims)


def test_csv_without_image_or_text_column(tmp_path):
    for header in ("id,caption", "image_file,label", "a,b"):
        p = tmp_path / "bad.csv"
        p.write_text(header + "\nx,y\n")
        with pytest.raises(ValueError, match="CSV must have image and text columns"):
            EV.read_pairs(p, tmp_path)
    (tmp_path / "im.png").write_bytes(b"x")
    p = tmp_path / "ok.csv"
    p.write_text("IMAGE,Description\nim.png,one\nsub/im.png,two\ngone.png,three\n")
    paths, texts = EV.read_pairs(p, tmp_path)
    assert [q.name for q in paths] == ["im.png", "im.png"] and texts == ["one", "two"]


def test_retrieval_ranks_without_a_device_fails_loudly():
    if torch.cuda.is_available():
        pytest.skip("a device is visible")
    e = torch.eye(4)
    with pytest.raises(RuntimeError):
        EV.retrieval_ranks(e, e)
    with pytest.raises(RuntimeError):
        EV.evaluate_retrieval(e, e)
