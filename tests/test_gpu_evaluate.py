"""The retrieval evaluator (clip_lora_match_amd.evaluate) against the reference's own
CLIPEvaluator.compute_recall_at_k / compute_mrr / compute_map, recorded in
tests/golden/eval_metrics.npz by tests/golden/make_eval_golden.py. In the fixture no other score
lies within 1e-5 of a target's (the generator asserts it), so the reference's fp32 tie order plays
no part and nothing is excluded here.
"""
import csv
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import GOLDEN, golden

import clip_lora_match_amd as clm
from clip_lora_match_amd import evaluate as EV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return golden("eval_metrics.npz")


def _expected(fx):
    ks = [int(k) for k in fx["k_values"]]
    want = {f"recall@{k}": float(v) for k, v in zip(ks, fx["i2t_recall"])}
    want["mrr"] = float(fx["i2t_mrr"])
    want["map"] = float(fx["i2t_map"])
    want.update({f"t2i_recall@{k}": float(v) for k, v in zip(ks, fx["t2i_recall"])})
    return ks, want


def test_evaluate_retrieval_equals_reference(fx):
    ks, want = _expected(fx)
    got = EV.evaluate_retrieval(torch.from_numpy(fx["a"]), torch.from_numpy(fx["b"]), ks)
    assert list(got) == list(want)
    for k in want:
        if "recall" in k:
            assert got[k] == want[k], k
        else:
            assert abs(got[k] - want[k]) <= 1e-12, k
    assert clm.evaluate_retrieval is EV.evaluate_retrieval


def test_retrieval_ranks_equal_reference_argsort_positions(fx):
    a, b = torch.from_numpy(fx["a"]), torch.from_numpy(fx["b"])
    assert np.array_equal(EV.retrieval_ranks(a, b).numpy(), fx["i2t_ranks"])
    assert np.array_equal(EV.retrieval_ranks(b, a).numpy(), fx["t2i_ranks"])
    # explicit targets: a permutation of the pairs ranks the same items
    perm = torch.randperm(a.shape[0], generator=torch.Generator().manual_seed(0))
    assert np.array_equal(EV.retrieval_ranks(a[perm], b, perm).numpy(), fx["i2t_ranks"][perm.numpy()])
    assert EV.matching_accuracy(a, b) == float(fx["i2t_recall"][0])


def test_compute_methods_on_the_similarity_matrix(fx):
    ks, want = _expected(fx)
    ev = EV.CLIPEvaluator.__new__(EV.CLIPEvaluator)      # the compute_* methods need no model
    sims = torch.from_numpy(fx["sims"])
    assert ev.compute_recall_at_k(sims, ks) == {k: want[k] for k in want if k.startswith("recall")}
    assert abs(ev.compute_mrr(sims) - want["mrr"]) <= 1e-12
    assert abs(ev.compute_map(sims) - want["map"]) <= 1e-12
    assert ev.compute_recall_at_k(sims.T, ks) == {k[4:]: want[k] for k in want if k.startswith("t2i_")}


def test_csv_flow_equals_functional_api(tmp_path, capsys):
    """CLIPEvaluator.evaluate_retrieval / evaluate_matching_accuracy over CSVs of the committed
    reference images (two header variants, one missing image) == the functional API on embeddings
    encoded directly"""
    from golden_images import write_ref_files
    from clip_lora_match_amd.embed_image import embed_images_batch
    from clip_lora_match_amd.embed_text import embed_text
    root = tmp_path / "images"
    root.mkdir()
    paths = write_ref_files(root)
    captions = [f"a photo of item number {i}, {os.path.splitext(p.name)[0]}" for i, p in enumerate(paths)]
    cfg = {"model": {"name": "openai/clip-vit-base-patch32", "device": "cpu", "dtype": "float32",
                     "weights_dir": "synthetic", "tokenizer_dir": os.path.join(GOLDEN, "clip_bpe")},
           "preprocess": {"image_size": 224}}
    y = tmp_path / "clip_config.yaml"
    y.write_text(yaml.safe_dump(cfg))
    ev = EV.CLIPEvaluator(y, lora_weights_path="synthetic", use_lora=True, max_batch=16)
    img = embed_images_batch(ev.model, ev.processor, paths, ev.device)
    txt = embed_text(ev.model, ev.processor, captions, ev.device)
    want = EV.evaluate_retrieval(img, txt, (1, 3))
    want_acc = EV.matching_accuracy(img, txt)
    # variant 1: image_file / caption, names relative to the root; variant 2: filename / text with a
    # directory prefix that only the basename fallback resolves, and one image that does not exist
    c1, c2 = tmp_path / "v1.csv", tmp_path / "v2.csv"
    with open(c1, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["image_file", "caption"])
        w.writerows([p.name, c] for p, c in zip(paths, captions))
    with open(c2, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["id", "Filename", "Text"])
        for i, (p, c) in enumerate(zip(paths, captions)):
            if i == 2:
                w.writerow([99, "nowhere/missing.jpg", "no such image"])
            w.writerow([i, f"some/dir/{p.name}", c])
    capsys.readouterr()
    for c in (c1, c2):
        got = ev.evaluate_retrieval(c, root, (1, 3))
        assert list(got) == ["recall@1", "recall@3", "mrr", "map", "t2i_recall@1", "t2i_recall@3"]
        assert got == want
        assert ev.evaluate_matching_accuracy(c, root) == want_acc
    out = capsys.readouterr().out
    assert out.count("Warning: Image not found: nowhere/missing.jpg, skipping...") == 1
    assert "Using columns: image='Filename', text='Text'" in out
    ev.close()
