"""Threshold search on the resident index (CosineIndex.search_above / search_above_rows /
near_duplicates, clm_index_search_above*, include/clm.h) and the layers on top.

Yardstick: cosine_similarity() on the same rows -- exact_scores, the routine the re-score goes
through -- so the expected lists are S >= tau (NaN included) ordered by (score desc, id asc)
(tests/range_ref.py) and offsets, scores and ids must be EQUAL, no exclusions (scores by their
bits; a NaN score must be a NaN).

Every case runs on the default route, with the MFMA filter pass forced (CLM_RANK_BAND: at these
sizes the default is the exact route) and with the exact route forced (CLM_RANK_EXACT).
"""
import pytest
import torch

from conftest import golden

import range_ref as R
from clip_lora_match_amd import _capi as C
from clip_lora_match_amd import synthetic as syn
from clip_lora_match_amd.distributed import merge_ragged
from clip_lora_match_amd.search import CosineIndex, TextSearchIndex
from clip_lora_match_amd.similarity import cosine_similarity

pytestmark = pytest.mark.gpu
ROUTES = {"default": 0, "band": C.CLM_RANK_BAND, "exact": C.CLM_RANK_EXACT}
I64_MAX = 2 ** 63 - 1


def _problem(N, dim, nq, seed):
    """Gaussian rows; half the queries are a row + 0.3 noise (cosine ~0.96 with it), half Gaussian"""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn(N, dim, generator=g)
    tgt = torch.randint(0, N, (nq,), generator=g)
    q = torch.randn(nq, dim, generator=g)
    near = torch.arange(nq) % 2 == 0
    q[near] = rows[tgt[near]] + 0.3 * q[near]
    return rows, q


def _scores(q, rows):
    return cosine_similarity(q.float(), rows.float()).reshape(q.shape[0], rows.shape[0]).cpu()


def _index(rows, offset=0):
    idx = CosineIndex(rows.shape[1], capacity=max(rows.shape[0], 1))
    idx.append(rows)
    if offset:
        idx.set_offset(offset)
    return idx


def _all_routes(idx, q, tau, want, cap=0, routes=ROUTES):
    for name, flag in routes.items():
        got = idx.search_above(q, tau, band_cap=flag | cap)
        assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[2].dtype == torch.int64
        assert got[1].is_cuda and got[2].is_cuda
        assert torch.equal(got[0].cpu(), want[0]), f"route {name}: offsets differ"
        assert R.same(got, want), f"route {name}: entries differ"


@pytest.mark.parametrize("dim", [64, 192, 512])
@pytest.mark.parametrize("N", [1, 255, 3000])
def test_range_shapes(N, dim):
    """N = 255: the ragged (scalar) epilogue; 3000: no multiple of the 192 / 256 tiles. The
    invariants: lengths == count_above(q, tau, INT64_MAX), result == prefix of search()."""
    for nq in (1, 17, 300):
        rows, q = _problem(N, dim, nq, 1000 * N + dim + nq)
        idx = _index(rows)
        tau = 0.5
        want = R.above_from_scores(_scores(q, rows), tau)
        lens = want[0][1:] - want[0][:-1]
        if nq > 1:
            assert (lens == 0).any() and (lens > 0).any(), "both empty and non-empty lists occur"
        _all_routes(idx, q, tau, want)
        st = idx.range_stats()
        assert st["fast"] == nq and st["exact"] == 2 * nq and st["overflow"] == 0
        above = idx.count_above(q, torch.full((nq,), tau), torch.full((nq,), I64_MAX, dtype=torch.int64))
        assert torch.equal(above.cpu(), lens)
        k = min(N, 1024)
        ss, si = idx.search(q, k)
        ss, si = ss.cpu(), si.cpu()
        for i in range(nq):
            a, b = int(want[0][i]), int(want[0][i + 1])
            assert b - a <= k
            assert torch.equal(si[i, : b - a], want[2][a:b])
            assert torch.equal(ss[i, : b - a].view(torch.int32), want[1][a:b].view(torch.int32))
        idx.close()


def test_range_two_query_blocks():
    """nq = 2600 > the 2560-query block: two balanced blocks of the filter pass"""
    rows, q = _problem(1000, 64, 2600, 7)
    idx = _index(rows)
    want = R.above_from_scores(_scores(q, rows), 0.5)
    assert int(want[0][-1]) > 1300
    _all_routes(idx, q, 0.5, want)
    idx.close()


def test_range_per_query_thresholds():
    """one call mixes -inf (all N rows, in search order), 0.0, 0.5, 2.0 and +inf (nothing), NaN
    (nothing: no row of this index scores NaN)"""
    N = 700
    rows, q = _problem(N, 128, 24, 11)
    taus = torch.tensor([-float("inf"), 0.0, 0.5, 2.0, float("inf"), float("nan")]).repeat(4)
    idx = _index(rows)
    want = R.above_from_scores(_scores(q, rows), taus)
    lens = (want[0][1:] - want[0][:-1]).reshape(4, 6)
    assert (lens[:, 0] == N).all() and (lens[:, 3:] == 0).all() and (lens[:, 1] > lens[:, 2]).all()
    _all_routes(idx, q, taus, want)
    ss, si = idx.search(q[::6], N)
    got = idx.search_above(q, taus, band_cap=C.CLM_RANK_BAND)
    for j in range(4):
        a = int(got[0][6 * j])
        assert torch.equal(got[2][a: a + N], si[j]) and torch.equal(got[1][a: a + N], ss[j])
    # a scalar threshold is every query's
    assert R.same(idx.search_above(q, 0.5), R.above_from_scores(_scores(q, rows), 0.5))
    idx.close()


def test_range_exact_ties():
    """50 rows, each present 3 times: the copies score equal bits and appear in id order"""
    g = torch.Generator().manual_seed(5)
    base = torch.randn(50, 64, generator=g)
    rows = torch.cat([base, base, base], 0)
    q = base[:16] + 0.5 * torch.randn(16, 64, generator=g)
    S = _scores(q, rows)
    assert torch.equal(S[:, :50], S[:, 50:100]) and torch.equal(S[:, :50], S[:, 100:])
    # between each query's 2nd and 3rd distinct score (a midpoint, not a score): 2 x 3 entries
    top = torch.sort(S[:, :50], dim=1, descending=True)[0]
    taus = (top[:, 1] + top[:, 2]) / 2
    want = R.above_from_scores(S, taus)
    assert torch.equal(want[0], 6 * torch.arange(17))
    ids = want[2].reshape(16, 2, 3)
    assert (ids[:, :, 1] == ids[:, :, 0] + 50).all() and (ids[:, :, 2] == ids[:, :, 0] + 100).all()
    idx = _index(rows)
    _all_routes(idx, q, taus, want)
    idx.close()


def _long_problem(N, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(64, generator=g)
    rows = v[None, :] + 1e-4 * torch.randn(N, 64, generator=g)
    q = torch.randn(24, 64, generator=g)
    q[:12] = v[None, :] + 1e-3 * q[:12]
    return rows, q


@pytest.mark.parametrize("N", [9000, 4097])
def test_range_long_segments(N):
    """12 queries return all N rows -- 9000: longer than an 8192-entry LDS run, so the merge passes
    run; 4097: one past a 4096 boundary -- past the default capacity of 2048 and past a forced one
    of 4 (range_stats counts the overflows), 12 return nothing. Two calls return equal bits."""
    rows, q = _long_problem(N, 3)
    idx = _index(rows)
    want = R.above_from_scores(_scores(q, rows), 0.9)
    lens = want[0][1:] - want[0][:-1]
    assert (lens[:12] == N).all() and (lens[12:] == 0).all()
    over = 0
    for cap in (0, 4):
        _all_routes(idx, q, 0.9, want, cap=cap)
        over += 12
        assert idx.range_stats()["overflow"] == over      # the band route's 12 near queries, each time
    a = idx.search_above(q, 0.9, band_cap=C.CLM_RANK_BAND)
    b = idx.search_above(q, 0.9, band_cap=C.CLM_RANK_BAND)
    assert R.same(a, b) and R.same(a, want)
    idx.close()


def test_range_nan_rows_lead():
    """a zero row and an fp16 inf row: the whole call takes the exact route (range_stats), and the
    NaN-scoring rows lead every list in id order, as they lead search()"""
    rows, q = _problem(600, 64, 10, 13)
    rows = rows.half()
    rows[77] = 0
    rows[401, 5] = float("inf")
    idx = _index(rows)
    S = _scores(q, idx.read())
    assert torch.isnan(S[:, 77]).all() and torch.isnan(S[:, 401]).all()
    want = R.above_from_scores(S, 0.5)
    for i in range(10):
        assert want[2][int(want[0][i]): int(want[0][i]) + 2].tolist() == [77, 401]
    _all_routes(idx, q, 0.5, want)
    assert idx.range_stats() == {"fast": 0, "exact": 30, "overflow": 0}
    # a NaN threshold returns the NaN-scoring rows alone
    got = idx.search_above(q, float("nan"), band_cap=C.CLM_RANK_BAND)
    assert torch.equal(got[0].cpu(), 2 * torch.arange(11)) and got[2].cpu().reshape(10, 2).tolist() == [[77, 401]] * 10
    # the finite part of every list is still the head of search()'s finite part (the search orders
    # a NaN by its bit pattern, so a zero row's negative NaN trails there)
    ss, si = idx.search(q, 600)
    ss, si = ss.cpu(), si.cpu()
    for i in range(10):
        a, b = int(want[0][i]) + 2, int(want[0][i + 1])
        fin = ~torch.isnan(ss[i])
        assert torch.equal(si[i][fin][: b - a], want[2][a:b])
        assert torch.equal(ss[i][fin][: b - a], want[1][a:b])
    idx.close()


def test_range_fp16_index_and_queries():
    """an index appended in fp16 keeps no fp32 copy: the scores are those of the fp16 rows"""
    rows, q = _problem(1500, 128, 40, 21)
    idx = _index(rows.half())
    assert C.lib().clm_index_has_f32(idx._h) == 0
    kept = idx.read()
    _all_routes(idx, q, 0.5, R.above_from_scores(_scores(q, kept), 0.5))
    _all_routes(idx, q.half(), 0.5, R.above_from_scores(_scores(q.half().float(), kept), 0.5))
    idx.close()


def test_range_offset_shards_and_rows():
    """set_offset(1000): ids are global; two half-indices merge (merge_ragged) to the whole; the
    index's own rows as queries equal the same rows read back and passed in"""
    rows, q = _problem(900, 64, 30, 17)
    idx = _index(rows, 1000)
    want = R.above_from_scores(_scores(q, rows), 0.5, offset=1000)
    _all_routes(idx, q, 0.5, want)
    lo, hi = _index(rows[:400], 1000), _index(rows[400:], 1400)
    for flag in ROUTES.values():
        parts = [lo.search_above(q, 0.5, band_cap=flag), hi.search_above(q, 0.5, band_cap=flag)]
        assert R.same(merge_ragged(parts), want)
    lo.close()
    hi.close()
    r0, n = 123, 45
    for flag in ROUTES.values():
        a = idx.search_above_rows(1000 + r0, n, 0.3, band_cap=flag)
        b = idx.search_above(idx.read(r0, n), 0.3, band_cap=flag)
        assert R.same(a, b)
        assert R.same(a, R.above_from_scores(_scores(rows[r0: r0 + n], rows), 0.3, offset=1000))
    for bad in ((999, 1), (1000, 901), (1900, 1), (1000, -1)):
        with pytest.raises(ValueError):
            idx.search_above_rows(bad[0], bad[1], 0.3)
    idx.close()
    empty = CosineIndex(64)
    with pytest.raises(ValueError):
        empty.search_above(q, 0.5)
    empty.close()


def test_range_after_mutation_and_read():
    """after remove and update the result equals the yardstick on the final rows; a result held
    from before a mutation cannot be read (CLM_E_STATE); a held result reads in pieces"""
    rows, q = _problem(800, 64, 20, 19)
    idx = _index(rows)
    L = C.lib()
    st = C.stream_of(idx.device)

    def read(start, n):
        s = torch.empty((n,), dtype=torch.float32, device=idx.device)
        i = torch.empty((n,), dtype=torch.int64, device=idx.device)
        return L.clm_index_search_above_read(idx._h, start, n, C.ptr(s), C.ptr(i), st), s, i

    s0 = torch.empty((1,), dtype=torch.float32)
    i0 = torch.empty((1,), dtype=torch.int64)
    assert L.clm_index_search_above_read(idx._h, 0, 0, C.ptr(s0), C.ptr(i0), st) == C.CLM_E_STATE   # nothing held yet
    off, s, i = idx.search_above(q, 0.5)
    total = int(off[-1])
    assert total >= 10
    cut = total // 3
    (ra, sa, ia), (rb, sb, ib) = read(0, cut), read(cut, total - cut)
    assert ra == rb == C.CLM_OK
    assert torch.equal(torch.cat([sa, sb]), s) and torch.equal(torch.cat([ia, ib]), i)
    hs = torch.empty((total,), dtype=torch.float32)     # host destinations too
    hi = torch.empty((total,), dtype=torch.int64)
    assert L.clm_index_search_above_read(idx._h, 0, total, C.ptr(hs), C.ptr(hi), st) == C.CLM_OK
    assert torch.equal(hs, s.cpu()) and torch.equal(hi, i.cpu())
    assert read(1, total)[0] == C.CLM_E_STATE and read(-1, 1)[0] == C.CLM_E_STATE   # outside the held result
    gone = [5, 300, 301, 799]
    idx.remove(gone)
    assert read(0, 1)[0] == C.CLM_E_STATE
    keep = torch.ones(800, dtype=torch.bool)
    keep[gone] = False
    final = rows[keep].clone()
    _all_routes(idx, q, 0.5, R.above_from_scores(_scores(q, final), 0.5))
    assert read(0, 1)[0] == C.CLM_OK
    new = q[:3] + 0.1 * torch.randn(3, 64, generator=torch.Generator().manual_seed(1))
    idx.update([10, 20, 700], new)
    assert read(0, 1)[0] == C.CLM_E_STATE
    final[[10, 20, 700]] = new
    want = R.above_from_scores(_scores(q, final), 0.5)
    assert {10, 20, 700} <= set(want[2].tolist())
    _all_routes(idx, q, 0.5, want)
    idx.reset()
    assert read(0, 1)[0] == C.CLM_E_STATE
    idx.close()


def test_near_duplicates():
    """200 Gaussian rows + 30 planted near-copies, several row blocks: the pairs are the full
    matrix's upper triangle at or above the threshold, ordered (i asc, score desc, j asc)"""
    g = torch.Generator().manual_seed(23)
    rows = torch.randn(200, 64, generator=g)
    src = torch.randint(0, 200, (30,), generator=g)
    rows = torch.cat([rows, rows[src] + 0.05 * torch.randn(30, 64, generator=g)], 0)
    rows = rows[torch.randperm(230, generator=g)]
    S = _scores(rows, rows)
    want_p, want_s = [], []
    for i in range(230):
        js = [j for j in range(i + 1, 230) if S[i, j] >= 0.95]
        js.sort(key=lambda j: (-float(S[i, j]), j))
        want_p += [[i, j] for j in js]
        want_s += [S[i, j] for j in js]
    assert len(want_p) >= 30
    idx = _index(rows)
    for block in (64, 4096):
        pairs, scores = idx.near_duplicates(0.95, block=block)
        assert pairs.dtype == torch.int64 and pairs.shape == (len(want_p), 2)
        assert pairs.cpu().tolist() == want_p and torch.equal(scores.cpu(), torch.stack(want_s))
    idx.set_offset(500)
    pairs, _ = idx.near_duplicates(0.95, block=64)
    assert (pairs.cpu() - 500).tolist() == want_p
    idx.close()


class _WordTokenizer:
    """a stand-in tokenizer for the tiny preset (vocab 1000): one id per word"""

    def __init__(self, cfg):
        self.cfg = cfg

    def __call__(self, texts, padding=True, truncation=True, max_length=None, return_tensors="pt"):
        import zlib
        rows = []
        for t in texts:
            ids = [2 + zlib.crc32(w.encode()) % 900 for w in t.replace(",", " ").split()][: max_length - 2]
            rows.append([self.cfg.bos_token_id] + ids + [self.cfg.eos_token_id])
        width = max(len(r) for r in rows)
        rows = [r + [self.cfg.eos_token_id] * (width - len(r)) for r in rows]
        return {"input_ids": torch.tensor(rows, dtype=torch.int64)}


def test_text_index_and_finder_similar_items(tmp_path):
    """TextSearchIndex.search_above_with_embedding (ids, texts, paths, both query forms, short
    metadata) and FinderIndex.similar_items on the tiny preset; the index is unchanged"""
    import clip_lora_match_amd as clm
    from clip_lora_match_amd import weights as W
    from clip_lora_match_amd.engine import ClipLoraModel
    from clip_lora_match_amd.finder import FinderIndex
    from clip_lora_match_amd.processor import ClipProcessor
    from PIL import Image

    rows, q = _problem(300, 64, 4, 29)
    ix = TextSearchIndex(embeddings=rows, image_paths=[f"p{i}" for i in range(300)], texts=[f"t{i}" for i in range(250)])
    S = _scores(q, ix.embeddings)
    seen = set()
    for i in range(4):
        want = R.above_from_scores(S[i: i + 1], 0.2)
        for form in (q[i], q[i: i + 1]):
            res = ix.search_above_with_embedding(form, 0.2)
            assert [r.index for r in res] == want[2].tolist()
            assert [r.score for r in res] == [float(v) for v in want[1]]
            assert all(r.image_path == f"p{r.index}" for r in res)
            assert all(r.text == (f"t{r.index}" if r.index < 250 else "") for r in res)
        seen |= set(want[2].tolist())
    assert any(j >= 250 for j in seen) and any(j < 250 for j in seen)    # with and without a text
    with pytest.raises(ValueError):
        ix.search_above_with_embedding(q[:2], 0.2)
    with pytest.raises(ValueError):
        ix.search_above_with_embedding(q[0, :32], 0.2)
    assert ix.search_above_with_embedding(q[0], 2.0) == []

    cfg = clm.get_preset("tiny")
    model = ClipLoraModel(cfg, device="cuda:0", compute_dtype="float16", max_batch=8)
    model.load_tensors(W.synthetic_state_dict(cfg, 0))
    model.load_tensors(W.synthetic_lora(cfg, 1))
    model.finalize()
    proc = ClipProcessor(cfg)
    proc.tokenizer = _WordTokenizer(cfg)
    imgs = syn.images_u8(4, cfg.image_size, 91)
    paths = []
    for i in range(4):
        paths.append(tmp_path / f"img{i}.png")
        Image.fromarray(imgs[i]).save(paths[-1])
    fi = FinderIndex(model, proc, "cuda:0", tmp_path / "data" / "index.pt", root_dir=tmp_path,
                     upload_dir=tmp_path / "data" / "reported", save_every=0)
    assert fi.similar_items(["dompet hitam"], 0.5) == [[]]          # an empty index matches nothing
    desc = ["dompet hitam kulit", "red backpack with laptop", "payung biru lipat", "dompet hitam kulit"]
    fi.report_items(paths, desc, locations=["kantin", None, "perpustakaan", "kantin"])
    before = fi.index.embeddings.clone()
    ask = ["dompet hitam kulit", "red backpack with laptop", "kunci motor"]
    locs = ["kantin", None, None]
    emb = model.encode_ids(proc.token_ids(["dompet hitam kulit, ditemukan di kantin", ask[1], ask[2]]).to(model.device),
                           normalize=True).float()
    want = R.above_from_scores(_scores(emb.cpu(), before), 0.999)
    got = fi.similar_items(ask, 0.999, locations=locs)
    assert [[h["id"] for h in hits] for hits in got] == [want[2][int(want[0][i]): int(want[0][i + 1])].tolist() for i in range(3)]
    assert [h["id"] for h in got[0]] == [0, 3] and [h["id"] for h in got[1]] == [1]
    assert got[0][0]["description"] == "dompet hitam kulit, ditemukan di kantin"
    assert got[0][1]["image_path"] == "data/reported/img3.png" and got[1][0]["score"] > 0.999
    everything = fi.similar_items(ask, -1.0)
    assert [len(h) for h in everything] == [4, 4, 4]
    assert fi.index.num_items == 4 and torch.equal(fi.index.embeddings, before)
    assert torch.equal(fi.index._gpu.read(0, 4), before)
    model.close()


def test_threshold_evaluator_matches_the_reference_golden():
    """evaluate_threshold_retrieval on the golden's inputs: the reference's metrics (scripts/
    evaluate.py evaluate_epoch's aggregation, to 1e-12) and its per-query relevant sets"""
    from clip_lora_match_amd.evaluate import evaluate_threshold_retrieval
    g = golden("threshold_metrics.npz")
    ks = [int(k) for k in g["k_values"]]
    m, (off, s, ids) = evaluate_threshold_retrieval(torch.from_numpy(g["queries"]), torch.from_numpy(g["index"]),
                                                    float(g["threshold"]), ks, return_sets=True)
    assert torch.equal(off, torch.from_numpy(g["relevant_offsets"]))
    # the golden lists each query's relevant ids ascending (the reference orders near-equal fp32
    # scores its own way); ours come best first
    ref_s = torch.from_numpy(g["relevant_scores"])
    for i in range(m["num_queries"]):
        a, b = int(off[i]), int(off[i + 1])
        order = torch.argsort(ids[a:b])
        assert torch.equal(ids[a:b][order], torch.from_numpy(g["relevant_ids"][a:b]))
        # the scores are the exact cosines: within fp32 rounding of the reference's own
        assert (s[a:b][order] - ref_s[a:b]).abs().max().item() < 1e-5 if b > a else True
    assert m["num_queries"] == g["queries"].shape[0] and m["threshold"] == float(g["threshold"])
    for j, k in enumerate(ks):
        assert abs(m["recall"][k] - g["recall"][j]) <= 1e-12 and abs(m["precision"][k] - g["precision"][j]) <= 1e-12
    assert abs(m["mrr"] - g["mrr"]) <= 1e-12 and abs(m["map"] - g["map"]) <= 1e-12
