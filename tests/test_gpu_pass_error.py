"""The bound every approximate route rests on, measured, and the exact routine held to its claim.

1. E. capi_search.cpp derives |fp16-pass score - exact cosine| <= E = 1.95e-3 + dim * 2^-24 on paper
   (RESCORE_MARGIN, RANK_MARGIN, the LSE and threshold windows all follow from it). Here the pass
   scores -- clm_gemm SCORE with rscale / cscale on the heuristic config and on config 1, and clm_scan16
   at dim <= 1024 -- are measured against the fp64 numpy cosine of the rows as the index keeps them, on
   input families that stress the fp16 rounding. The operands are the product's own: fp32 rows appended
   to a CosineIndex (rows_to_f16 mode 2) and, for the queries, to a second one; clm_index_export gives
   rows16 / inv exactly as every pass reads them. Rows appended as fp16 take mode 0 (row side only: fp16
   QUERIES are staged to fp32 and converted by mode 2 inside the search, a path export cannot show, so
   they are not measured here). The largest error per (dim, family) is printed; DESIGN.md records the
   table.

2. The exact routine claims fp32(cos64). clm_cosine_scores and CosineIndex.search(k = N) on an fp16-only
   index: for every pair |got - ref| <= ulp32(ref) / 2 + 2^-44 with ref in np.longdouble
   (select_ref.rounding_excess), no pair excluded, a NaN must be a NaN.
"""
import numpy as np
import pytest
import torch

import select_ref as SR
from clip_lora_match_amd import _capi as C
from clip_lora_match_amd.search import CosineIndex

pytestmark = pytest.mark.gpu

N_ROWS, N_Q = 2048, 16


def E_bound(dim):
    return 1.95e-3 + dim * 2.0 ** -24


# ---- input families -----------------------------------------------------------------------------------

def _sparse(rng, m, dim, nnz):
    """rows with min(nnz, dim) non-zero Gaussian elements among the first 16 columns (so that two sparse
    rows overlap)"""
    c = min(dim, 16)
    nnz = min(nnz, c)
    cols = np.argsort(rng.random((m, c)), axis=1)[:, :nnz]
    v = rng.standard_normal((m, nnz)).astype(np.float32)
    v[v == 0] = 1.0
    out = np.zeros((m, dim), np.float32)
    np.put_along_axis(out, cols, v, axis=1)
    return out


def _half_sparse_queries(rng, nq, dim, nnz):
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    q[::2] = _sparse(rng, (nq + 1) // 2, dim, nnz)
    return q


def _worst_rounding(rng, m, dim):
    """+-2^e (1 + odd 2^-11): every element halfway between two fp16 values"""
    e = rng.integers(-4, 4, (m, dim))
    odd = 2 * rng.integers(0, 1024, (m, dim)) + 1
    sign = rng.integers(0, 2, (m, dim)) * 2 - 1
    return (sign * np.ldexp(1.0 + odd * 2.0 ** -11, e)).astype(np.float32)


def _pairs(rng, q, n):
    """row i against query i % nq: near-parallel, anti-parallel, orthogonal (to fp32 rounding) in turn"""
    nq, dim = q.shape
    out = np.empty((n, dim), np.float32)
    for i in range(n):
        qj = q[i % nq].astype(np.float64)
        g = rng.standard_normal(dim)
        kind = (i // nq) % 3
        if kind == 0:
            r = qj * rng.uniform(0.5, 2.0) + 1e-3 * g
        elif kind == 1:
            r = -qj * rng.uniform(0.5, 2.0) + 1e-3 * g
        else:
            r = g - (g @ qj) / (qj @ qj) * qj
        out[i] = r.astype(np.float32)
    return out


def families32(rng, n, nq, dim):
    """name -> (rows [n, dim], queries [nq, dim]) fp32"""
    g = lambda m: rng.standard_normal((m, dim)).astype(np.float32)
    fam = {"gaussian": (g(n), g(nq))}
    for nnz in (1, 2, 3, 8):
        fam[f"sparse{nnz}"] = (_sparse(rng, n, dim, nnz), _half_sparse_queries(rng, nq, dim, nnz))
    fam["half-ulp"] = (_worst_rounding(rng, n, dim), _worst_rounding(rng, nq, dim))
    fam["heavy-tail"] = ((g(n) * np.exp(3.0 * g(n))).astype(np.float32), (g(nq) * np.exp(3.0 * g(nq))).astype(np.float32))
    q = g(nq)
    fam["pairs"] = (_pairs(rng, q, n), q)
    fam["row-scales"] = ((g(n) * 10.0 ** rng.uniform(-15, 15, (n, 1))).astype(np.float32),
                         (g(nq) * 10.0 ** rng.uniform(-15, 15, (nq, 1))).astype(np.float32))
    return fam


def families16(rng, n, nq, dim):
    """name -> (rows [n, dim] float16, queries [nq, dim] fp32): rows appended as fp16"""
    g = lambda m: rng.standard_normal((m, dim)).astype(np.float32)
    fam = {"gaussian": (g(n).astype(np.float16), g(nq))}
    for nnz in (1, 2, 3, 8):
        fam[f"sparse{nnz}"] = (_sparse(rng, n, dim, nnz).astype(np.float16), _half_sparse_queries(rng, nq, dim, nnz))
    fam["heavy-tail"] = (np.clip(g(n) * np.exp(2.0 * g(n)), -6e4, 6e4).astype(np.float16), g(nq))
    q = g(nq)
    fam["pairs"] = (_pairs(rng, q, n).astype(np.float16), q)
    # 2^-10 .. 2^6: small rows are made of fp16 subnormals, large ones reach 2^6 * 4 sigma
    fam["row-scales"] = ((g(n) * np.exp2(rng.integers(-10, 7, (n, 1)))).astype(np.float16), g(nq))
    for name, (r, _) in fam.items():
        assert np.all(np.isfinite(r)) and np.all((r.astype(np.float32) ** 2).sum(axis=1) > 0), name
    return fam


# ---- 1. the pass error --------------------------------------------------------------------------------

def _export(rows):
    """append rows (np fp32 or float16) to a fresh index; returns (rows16 int16 [n, dim_p], inv f32 [n]) on
    the device and the rows as the index keeps them (fp32 copy, or the fp16 values) in fp64"""
    n, dim = rows.shape
    ix = CosineIndex(dim)
    ix.append(torch.from_numpy(rows))
    has32 = int(C.lib().clm_index_has_f32(ix._h))
    assert has32 == (rows.dtype == np.float32)
    r16 = torch.zeros((n, ix.dim_p), dtype=torch.float16)
    inv = torch.zeros((n,), dtype=torch.float32)
    r32 = torch.zeros((n, ix.dim_p), dtype=torch.float32) if has32 else None
    C.check(C.lib().clm_index_export(ix._h, 0, n, C.ptr(r16), C.ptr(inv), C.ptr(r32) if has32 else None,
                                     C.stream_of(ix.device)), "clm_index_export")
    ix.close()
    kept = (r32 if has32 else r16).numpy().astype(np.float64)
    assert np.array_equal(kept[:, :dim], rows.astype(np.float64))
    return r16.view(torch.int16).cuda(), inv.cuda(), kept


def _truth(q64, r64):
    return (q64 @ r64.T) / (np.linalg.norm(q64, axis=1)[:, None] * np.linalg.norm(r64, axis=1)[None, :])


def _pass_scores(rows, q):
    """{path: scores [nq, n] fp64} of the fp16 pass over the exported operands, and the fp64 truth"""
    n, nq = rows.shape[0], q.shape[0]
    r16, rinv, r64 = _export(rows)
    q16, qinv, q64 = _export(q)
    K = r16.shape[1]
    st = C.stream_of(r16.device)
    out = {}
    for cfg, name in ((-1, "gemm"), (1, "gemm cfg 1")):
        S = torch.full((nq, n), float("nan"), dtype=torch.float32, device="cuda")
        C.check(C.lib().clm_gemm(0, C.CLM_F16, C.CLM_EPI_SCORE, cfg, C.ptr(q16), K, C.ptr(r16), K, nq, n, K, C.ptr(S), n,
                                 None, C.ptr(qinv), C.ptr(rinv), st), "clm_gemm")
        torch.cuda.synchronize()
        out[name] = S.cpu().numpy().astype(np.float64)
    if K <= 1024:
        nchunk = (n + 255) // 256
        W = int(C.lib().clm_scan16_waves(0, n, K))
        ldw = 8 * W + 8
        S = torch.full((n, 16), float("nan"), dtype=torch.float32, device="cuda")
        cmax = torch.zeros((nq * nchunk,), dtype=torch.float32, device="cuda")
        wtop = torch.zeros((nq, ldw), dtype=torch.float32, device="cuda")
        C.check(C.lib().clm_scan16(0, C.ptr(r16), C.ptr(rinv), n, K, C.ptr(q16), C.ptr(qinv), nq, C.ptr(S), 16,
                                   C.ptr(cmax), C.ptr(wtop), ldw, st), "clm_scan16")
        torch.cuda.synchronize()
        out["scan16"] = S.cpu().numpy().astype(np.float64).T[:nq]
    return out, _truth(q64, r64)


def _measure(dim, fams, label):
    worst = {}
    print()
    for name, (rows, q) in fams.items():
        scores, truth = _pass_scores(rows, q)
        assert np.all(np.isfinite(truth)), name
        errs = {}
        for path, s in scores.items():
            assert np.all(np.isfinite(s)), (name, path)
            errs[path] = float(np.abs(s - truth).max())
        worst[name] = max(errs.values())
        print(f"pass error {label} dim {dim:5d} {name:11s} " + "  ".join(f"{p} {e:.3e}" for p, e in errs.items()) +
              f"   (E {E_bound(dim):.3e})")
    bad = {n: e for n, e in worst.items() if not e <= E_bound(dim)}
    assert not bad, f"{label} dim {dim}: pass error above E = {E_bound(dim):.3e}: {bad}"
    return worst


@pytest.mark.parametrize("dim", [64, 128, 512, 1024, 8192])
def test_pass_error_within_E_f32_rows(dim):
    """2048 rows x 16 queries, both appended as fp32 (rows_to_f16 mode 2): max |s - truth| <= E on every
    family and every pass"""
    _measure(dim, families32(np.random.default_rng(dim), N_ROWS, N_Q, dim), "f32 rows")


@pytest.mark.parametrize("dim", [64, 128, 512, 1024, 8192])
def test_pass_error_within_E_f16_rows(dim):
    """rows appended as fp16 (mode 0: the fp16 values as they are, the inverse norm of those values), whole
    rows scaled from 2^-10 to 2^6; queries fp32"""
    _measure(dim, families16(np.random.default_rng(dim + 1), N_ROWS, N_Q, dim), "f16 rows")


# ---- 2. the exact routine -----------------------------------------------------------------------------

def _ld_matrix(q, r):
    """cosines [nq, n] in np.longdouble of fp32 / fp16 operands"""
    ql, rl = np.asarray(q).astype(np.longdouble), np.asarray(r).astype(np.longdouble)
    with np.errstate(invalid="ignore", divide="ignore"):
        dots = np.stack([(rl * ql[j]).sum(axis=1) for j in range(ql.shape[0])])
        return dots / (np.sqrt((ql * ql).sum(axis=1))[:, None] * np.sqrt((rl * rl).sum(axis=1))[None, :])


def _assert_rounded(got, ref, what):
    ex = SR.rounding_excess(got, ref)
    bad = np.argwhere(ex > 0)
    assert bad.size == 0, (f"{what}: {bad.shape[0]} of {ex.size} pairs off the correctly rounded cosine, first "
                           f"{tuple(bad[0])}: got {got[tuple(bad[0])]!r}, ref {float(ref[tuple(bad[0])])!r}, excess "
                           f"{ex[tuple(bad[0])]:.3e}")


@pytest.mark.parametrize("dim", [1, 63, 64, 65, 100, 512, 8192])
def test_cosine_scores_correctly_rounded(dim):
    """clm_cosine_scores on every family: the fp32 score is the correctly rounded cosine up to fp64 noise.
    The Gaussian family carries one zero row and one zero query: their scores are NaN on both sides."""
    n, nq = (256, 8) if dim > 1024 else (512, 16)
    fams = families32(np.random.default_rng(7 * dim), n, nq, dim)
    fams["gaussian"][0][5] = 0.0
    fams["gaussian"][1][3] = 0.0
    saw_nan = False
    for name, (rows, q) in fams.items():
        d_r, d_q = torch.from_numpy(rows).cuda(), torch.from_numpy(q).cuda()
        out = torch.full((nq, n), 7.0, dtype=torch.float32, device="cuda")
        C.check(C.lib().clm_cosine_scores(0, C.ptr(d_q), nq, C.ptr(d_r), n, dim, C.ptr(out), C.stream_of(out.device)))
        got = out.cpu().numpy()
        ref = _ld_matrix(q, rows)
        saw_nan |= bool(np.isnan(got).any())
        _assert_rounded(got, ref, f"dim {dim} {name}")
    assert saw_nan


@pytest.mark.parametrize("dim", [64, 100, 512])
def test_search_all_scores_correctly_rounded_f16_index(dim):
    """CosineIndex.search(k = N) on an index that holds fp16 rows only: every (query, id) score is the
    correctly rounded cosine of the fp32 query and the fp16 row"""
    n, nq = 1500, 8
    for name, (rows, q) in families16(np.random.default_rng(3 * dim), n, nq, dim).items():
        ix = CosineIndex(dim)
        ix.append(torch.from_numpy(rows))
        s, i = ix.search(torch.from_numpy(q), n)
        s, i = s.cpu().numpy(), i.cpu().numpy()
        ix.close()
        assert np.array_equal(np.sort(i, axis=1), np.tile(np.arange(n), (nq, 1))), name
        ref = np.take_along_axis(_ld_matrix(q, rows), i, axis=1)
        _assert_rounded(s, ref, f"dim {dim} {name}")
